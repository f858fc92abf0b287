"""GPU parity: multi-ms coherent acquisition (gnsscorr_acq_set_coherent) on every engine.

The setter is implemented three times -- acq_fwd16_kernel (fp32, csrc/acq32.hip),
acq64_wipe_kernel<P> (the compiled fp64 plans) and g_wipe_kernel (the generic fp64
engine: mixed-radix passes, four-step plan, chirp-z; csrc/acq64_gen.hip) -- and each folds
coh code periods of a block into one N-point row with the carrier phase running on over
n + p*N.  The scenes of tests/acq_coh_scenes.py make every way of getting that fold wrong
change the signal row by 0.37 of its peak or more (tests/test_acq_coh_cpu.py), and here
every engine searches them with coh = 2, 3 and 5 in both block modes, from IQ and real
IF, int8 and 2-bit packed, one record and three.

Reference: GLONASS/L1/acquisition.sci:52-72, 113-135 through oracle/acq_oracle.py
acquire(coh=, noncoherent=), coh*N-point transforms in fp64.  Tolerances are the
project's: check_rows of test_acq_gpu.py (fp64: 1e-6 relative, the 1e-9 class bound,
decisions exact; fp32: powers 2e-5 of the row maximum, peaks 1e-4), and 1e-9 of the row
maximum for full fp64 power rows (test_power_row_generic).
"""
import numpy as np
import pytest

import acq_coh_scenes as S
from test_acq_gpu import check_rows

pytestmark = pytest.mark.gpu
WORST = {}


def _is64(engine):
    return not S.ENGINES[engine].get("f32")


def _ctx(gpu, monkeypatch, engine, max_blocks):
    e = S.ENGINES[engine]
    for k in ("GNSSCORR_ACQ_GENERIC", "GNSSCORR_ACQ_BLUESTEIN", "GNSSCORR_ACQ_MIX4"):
        monkeypatch.delenv(k, raising=False)
    for k, v in e.get("env", {}).items():     # the engine choice is read at create
        monkeypatch.setenv(k, v)
    ctx = gpu.AcqCtx(e["fs"], e["n"], max_freqs=8, max_blocks=max_blocks, max_codes=2,
                     precision=gpu.ACQ_F64 if _is64(engine) else gpu.ACQ_F32)
    ctx.set_codes(S.codes(e["fs"]))
    return ctx


def _mode(gpu, mode):
    return gpu.ACQ_NONCOHERENT if mode == "noncoherent" else gpu.ACQ_BEST_OF_BLOCKS


def _search(gpu, ctx, sc, IF, mode, packed=False):
    return ctx.search(gpu.pack2(IF) if packed else IF, sc.n_blocks, S.freqs(sc), S.GCODE, S.GF,
                      spc=sc.spc, iq=gpu.iq_flags(sc.iq, packed), mode=_mode(gpu, mode))


def _held_to_oracle(engine, sc, mode, res, rows, rec=0, label=""):
    nc = mode == "noncoherent"
    ref, ref_rows = S.reference(sc, nc, rec)
    label = f"{engine}-coh{sc.coh}-{mode}{label}"
    worst = check_rows(res, rows, ref, ref_rows, _is64(engine), label=label)
    WORST[engine] = max(WORST.get(engine, 0.0), worst)
    if _is64(engine):
        print(f"[coh engines] {engine}: worst relative error so far {WORST[engine]:.3e}")
    sig = rows[S.SIG_GROUP, S.SIG_BIN]
    assert sig["block"] == (-1 if nc else 1) and sig["argmax"] == sc.phases[rec]
    assert res[S.SIG_GROUP]["bin"] == S.SIG_BIN
    assert res[S.SIG_GROUP]["code_phase"] == sc.phases[rec] + 1
    assert res[S.SIG_GROUP]["metric"] > res[1 - S.SIG_GROUP]["metric"]


SEARCH_CASES = [pytest.param(e, coh, mode, id=f"{e}-coh{coh}-{mode}")
                for e in S.ENGINES for coh, mode in S.search_cases(e)]


@pytest.mark.parametrize("engine,coh,mode", SEARCH_CASES)
def test_search_vs_oracle(gpu, monkeypatch, engine, coh, mode):
    sc = S.scene(engine, coh, mode)
    ctx = _ctx(gpu, monkeypatch, engine, sc.n_blocks * coh)
    ctx.set_coherent(coh)
    res, rows = _search(gpu, ctx, sc, S.record(sc), mode)
    ctx.close()
    _held_to_oracle(engine, sc, mode, res, rows)


@pytest.mark.parametrize("engine", ["mixed-5000", "bluestein-4111", "m4-16368", "f64-16368",
                                    "f64-16000"])
def test_power_row_vs_literal(gpu, monkeypatch, engine):
    """Whole rows of both blocks at coh = 3 against the literal 3 N-point correlation."""
    sc = S.scene(engine, 3, "best")
    ctx = _ctx(gpu, monkeypatch, engine, sc.n_blocks * sc.coh)
    ctx.set_coherent(sc.coh)
    f = S.freqs(sc)
    for blk, freq, code in [(0, f[S.SIG_BIN], S.SIG_GROUP), (1, f[S.SIG_BIN], S.SIG_GROUP),
                            (1, f[5], S.SIG_GROUP), (0, f[1], 1 - S.SIG_GROUP)]:
        got = ctx.power_row(S.record(sc), sc.n_blocks, blk, freq, code)
        ref = S.literal_row(sc, freq, code, blk)
        err = np.abs(got - ref).max() / ref.max()
        print(f"[coh power row {engine}] block {blk} code {code}: {err:.3e}")
        assert err < 1e-9
        assert np.argmax(got) == np.argmax(ref)
    ctx.close()


@pytest.mark.parametrize("packed", [False, True], ids=["int8", "packed"])
@pytest.mark.parametrize("engine", S.REAL_IF_ENGINES)
def test_real_if(gpu, monkeypatch, engine, packed):
    """Real IF (the e0 + ne*m element indexing) at coh = 2, both modes: int8 against the
    oracle (iq=False), 2-bit packed byte-identical to int8."""
    for mode in S.MODES:
        sc = S.scene(engine, 2, mode, iq=False)
        ctx = _ctx(gpu, monkeypatch, engine, sc.n_blocks * sc.coh)
        ctx.set_coherent(sc.coh)
        res, rows = _search(gpu, ctx, sc, S.record(sc), mode)
        if packed:
            pres, prows = _search(gpu, ctx, sc, S.record(sc), mode, packed=True)
            assert pres.tobytes() == res.tobytes() and prows.tobytes() == rows.tobytes()
            assert prows[S.SIG_GROUP, S.SIG_BIN]["argmax"] == sc.phases[0]
        else:
            _held_to_oracle(engine, sc, mode, res, rows, label="-real")
        ctx.close()


@pytest.mark.parametrize("engine", ["mixed-5000", "m4-16368"])
def test_iq_packed_equals_int8(gpu, monkeypatch, engine):
    for mode in S.MODES:
        sc = S.scene(engine, 5, mode)
        ctx = _ctx(gpu, monkeypatch, engine, sc.n_blocks * sc.coh)
        ctx.set_coherent(sc.coh)
        res, rows = _search(gpu, ctx, sc, S.record(sc), mode)
        pres, prows = _search(gpu, ctx, sc, S.record(sc), mode, packed=True)
        ctx.close()
        assert pres.tobytes() == res.tobytes() and prows.tobytes() == rows.tobytes()
        assert rows[S.SIG_GROUP, S.SIG_BIN]["argmax"] == sc.phases[0]


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("engine", S.RECORD_ENGINES)
def test_generic_records_coherent(gpu, monkeypatch, engine, mode):
    """Three records at coh = 2, record r at r * n_blocks * coh * N, each with its own
    code phase: every record byte-identical to its single-record search, record 1 also
    held to the oracle."""
    R = S.N_RECORDS
    sc = S.scene(engine, 2, mode, records=R)
    single = _ctx(gpu, monkeypatch, engine, sc.n_blocks * sc.coh)
    single.set_coherent(sc.coh)
    one = [_search(gpu, single, sc, S.record(sc, r), mode) for r in range(R)]
    single.close()
    batch = _ctx(gpu, monkeypatch, engine, sc.n_blocks * sc.coh * R)
    batch.set_coherent(sc.coh)
    batch.set_records(R)
    res, rows = _search(gpu, batch, sc, S.if_records(sc), mode)
    batch.close()
    assert res.shape == (R, 2) and rows.shape == (R, 2, S.N_BINS)
    for r in range(R):
        assert res[r].tobytes() == one[r][0].tobytes(), f"record {r} results"
        assert rows[r].tobytes() == one[r][1].tobytes(), f"record {r} rows"
        assert rows[r, S.SIG_GROUP, S.SIG_BIN]["argmax"] == sc.phases[r]
    _held_to_oracle(engine, sc, mode, res[1], rows[1], rec=1, label="-records[1]")


@pytest.mark.parametrize("engine", ["f64-16368", "mixed-5000"])
def test_coherent_off_again_is_a_fresh_context(gpu, monkeypatch, engine):
    """set_coherent(5), search, set_coherent(1), search: the second search equals that of
    a context that never had a coherent length, byte for byte."""
    sc5 = S.scene(engine, 5, "best")
    sc1 = sc5._replace(coh=1)
    IF1 = S.record(sc5)[:2 * sc1.rec_samples]
    ctx = _ctx(gpu, monkeypatch, engine, sc5.n_blocks * sc5.coh)
    ctx.set_coherent(5)
    res5, rows5 = _search(gpu, ctx, sc5, S.record(sc5), "best")
    assert rows5[S.SIG_GROUP, S.SIG_BIN]["block"] == 1
    ctx.set_coherent(1)
    res, rows = _search(gpu, ctx, sc1, IF1, "best")
    ctx.close()
    fresh = _ctx(gpu, monkeypatch, engine, sc5.n_blocks * sc5.coh)
    fres, frows = _search(gpu, fresh, sc1, IF1, "best")
    fresh.close()
    assert res.tobytes() == fres.tobytes() and rows.tobytes() == frows.tobytes()
    # and it is a 1-ms search: block 0 of the 5-ms record is all amplitude 1, no block 1
    assert rows[S.SIG_GROUP, S.SIG_BIN]["peak"] < 0.5 * rows5[S.SIG_GROUP, S.SIG_BIN]["peak"]


def test_bounds_generic(gpu, monkeypatch):
    """n_blocks * coh * records within max_blocks on the generic engine too, and no
    coherent length on a zero-padded context."""
    n = S.ENGINES["mixed-5000"]["n"]
    ctx = _ctx(gpu, monkeypatch, "mixed-5000", 8)
    f, gc, gf = [1.25e6], [0], [[0]]
    IF = np.ones(2 * 12 * n, np.int8)
    ctx.set_coherent(2)
    ctx.search(IF, 4, f, gc, gf, spc=5)                 # 4 x 2 x 1 = 8 fits
    with pytest.raises(gpu.GnssCorrError):
        ctx.search(IF, 5, f, gc, gf, spc=5)             # 5 x 2 x 1
    ctx.set_records(2)
    ctx.search(IF, 2, f, gc, gf, spc=5)                 # 2 x 2 x 2 = 8 fits
    with pytest.raises(gpu.GnssCorrError):
        ctx.search(IF, 3, f, gc, gf, spc=5)             # 3 x 2 x 2
    ctx.set_records(1)
    ctx.set_coherent(1)
    ctx.set_zero_padded(n // 2)
    with pytest.raises(gpu.GnssCorrError):
        ctx.set_coherent(2)
    ctx.close()
