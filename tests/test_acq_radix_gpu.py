"""GPU: every compiled radix of the generic fp64 acquisition engine's mixed-radix passes
(csrc/acq64_gen.hip mx_pass<R, MODE>, R in 16 8 4 2 3 5 7 11 13 17 19 23 29 31) in every
position and mode, against the fp64 oracle (oracle/acq_oracle.py; the zero-padded
searches against tests/e1b_scenarios.py).

The lengths (tests/acq_radix_scenes.py TABLE, all below 2000 samples) are chosen so that
every radix runs as the first pass (MODE 1: the fused correlation product; MODE 5: the
zero-extended first pass), as a middle pass (MODE 0), as the last pass (MODE 2: the fused
power) and as the last pass of the zero-padded order (MODE 3: bounded; MODE 4, even
radices: the half pass, dft_first_half<R>); tests/test_acq_mixplan_cpu.py holds that
coverage to the library's own gnsscorr_acq_mix_plan.  The test ids carry the pass order,
so a failure names its radices.  Partial 128-thread blocks and N / R < 128 run here in the
unpadded search as well.

Two bars on the power rows.  The project's: 1e-9 of the row maximum with equal argmax
(test_acq_generic_gpu.py test_power_row_generic).  The tight one, 1e-12 of the row
maximum: one wrong entry of a constexpr twiddle table kTw<R> or one wrong term of a prime
butterfly moves a row by far more, and 1e-9 would let some of those through.  The
oracle's own error at these rows is 1.4e-15 .. 2.8e-15 (long-double direct DFT,
test_acq_mixplan_cpu.py test_reference_floor, held below 1e-14); 1e-12 leaves ~300 times
that for three cascaded transforms, prime butterflies of up to 15 fused terms and the
table twiddles, stays ten times above the ~1e-13 the engine's searches print at N = 38192
and is three orders below the 1e-9 bar.  Every case prints what it observed; DESIGN.md
section 5 lists the MI355X values.
"""
import numpy as np
import pytest

import acq_oracle as A
import acq_radix_scenes as S
import e1b_scenarios as E
import test_acq_padded_gpu as P
from test_acq_gpu import check_rows

pytestmark = pytest.mark.gpu

TIGHT = 1e-12      # of the row maximum: the per-radix bar (module docstring)
PROJECT = 1e-9     # of the row maximum: the bar of test_power_row_generic


@pytest.fixture(autouse=True)
def _mixed_radix_engine(monkeypatch):
    monkeypatch.setenv("GNSSCORR_ACQ_BLUESTEIN", "0")
    for var in ("GNSSCORR_ACQ_GENERIC", "GNSSCORR_ACQ_MIX4", "GNSSCORR_ACQ_GCHUNK_MB"):
        monkeypatch.delenv(var, raising=False)


def _row_error(got, ref, label):
    """The largest difference of a power row from the oracle's, in row maxima; the
    project's bar and the argmax are asserted here, on a row whose maximum is decided."""
    top = np.sort(ref)[-2:]
    assert top[1] > top[0] * (1 + 1e-6), ("the oracle row's maximum is not decidable", label)
    err = float(np.abs(got - ref).max() / ref.max())
    assert err < PROJECT, (label, err)
    assert int(np.argmax(got)) == int(np.argmax(ref)), label
    return err


def _both_orders(gpu, n):
    plan = gpu.acq_mix_plan(n)
    assert (tuple(plan[0]), tuple(plan[1])) == S.TABLE[n], "the test id names other radices"
    return plan


# ---- a. power rows: MODE 1, 0, 2 in the unpadded order (and MODE 0 of the forward
# transforms of codes and IF), at the tight bar ------------------------------------------
@pytest.mark.parametrize("n", S.LENGTHS, ids=S.case_id)
def test_power_rows(gpu, n):
    _both_orders(gpu, n)
    codes, IF = S.scene(n)
    ctx = gpu.AcqCtx(S.fs_of(n), n, max_freqs=8, max_blocks=2, max_codes=2)
    ctx.set_codes(codes)
    worst = 0.0
    for b in S.ROW_BINS:
        ref = S.oracle_rows(n, 0, b)
        for blk in (0, 1):
            got = ctx.power_row(IF, 2, blk, S.BINS[b], 0)
            worst = max(worst, _row_error(got, ref[blk], (n, b, blk)))
    assert int(np.argmax(S.oracle_rows(n, 0, S.PLANTED)[1])) == n // 3     # the planted lag
    print(f"[radix power rows N={S.case_id(n)}] {worst:.3e}")
    assert worst < TIGHT, (S.case_id(n), worst)


# ---- b. unpadded search, both modes: the statistics after MODE 2, partial blocks ---------
@pytest.mark.parametrize("mode", ["best", "noncoherent"])
@pytest.mark.parametrize("n", S.LENGTHS, ids=S.case_id)
def test_search_unpadded(gpu, n, mode):
    _both_orders(gpu, n)
    codes, IF = S.scene(n)
    fs, nc, spc = S.fs_of(n), mode == "noncoherent", max(2, n // 64)
    gf = np.tile(np.arange(len(S.BINS)), (2, 1))
    ref, ref_rows = A.acquire(IF, fs, codes, S.BINS, gf, spc=spc, n_blocks=2, noncoherent=nc,
                              return_rows=True)
    # decidable in the oracle (e1b_scenarios.assert_decidable wants the rows themselves:
    # its restatement with L = keep = N is the same search)
    dref, drows, _ = E.acquire(IF, fs, codes, n, n, S.BINS, gf, spc=spc, n_blocks=2,
                               noncoherent=nc)
    E.assert_decidable(dref, drows, spc)
    for g in range(2):
        assert [r["peak"] for r in drows[g]] == [r["peak"] for r in ref_rows[g]]
        if nc:                                  # the non-coherent rows carry no block choice
            for r in ref_rows[g]:
                r["block"] = -1
    ctx = gpu.AcqCtx(fs, n, max_freqs=8, max_blocks=2, max_codes=2)
    ctx.set_codes(codes)
    m = gpu.ACQ_NONCOHERENT if nc else gpu.ACQ_BEST_OF_BLOCKS
    res, rows = ctx.search(IF, 2, S.BINS, np.arange(2), gf, spc=spc, mode=m)
    check_rows(res, rows, ref, ref_rows, True, label=f"radix-{S.case_id(n)}-{mode}")
    assert ref[0]["code_phase"] == n // 3 + 1 and ref[0]["bin"] == S.PLANTED


# ---- c. zero-padded search: the padded order, MODE 4 (keep = N/2, even last radix) and
# MODE 3 (odd keep), one and two blocks, both modes ----------------------------------------
PADDED = [(n, keep) for n in S.LENGTHS for keep in S.keeps_of(n)]


@pytest.mark.parametrize("n,keep", PADDED, ids=[f"{S.padded_id(n)}-keep{k}" for n, k in PADDED])
def test_search_zero_padded(gpu, n, keep):
    _, rp = _both_orders(gpu, n)
    assert keep % 2 == 1 or (2 * keep == n and rp[-1] % 2 == 0)   # bounded / half last pass
    codes, IF = S.padded_scene(n, keep)
    fs, spc = S.fs_of(n), max(2, n // 64)
    ctx = P._ctx(gpu, n, keep, codes, fs=fs)
    gf = np.tile(np.arange(len(S.BINS)), (2, 1))
    for nb in (1, 2):
        for nc in (False, True):
            res, rows, ref, ref_rows, _ = P._search(gpu, ctx, IF, n, keep, codes, S.BINS, gf,
                                                    spc, nb, nc, fs=fs)
            check_rows(res, rows, ref, ref_rows, True,
                       label=f"radix-padded-{S.padded_id(n)}-keep{keep}-nb{nb}-"
                             f"{'nc' if nc else 'best'}")
            # (keep samples resolve ~2.7 kHz: the planted lag is found, the bin is any near one)
            assert ref[0]["code_phase"] == keep // 3 + 1
            assert (rows["argmax"] < keep).all()


# ---- d. the zero-extended first pass (MODE 5) against the plain one ----------------------
@pytest.mark.parametrize("n,first", [(770, 2), (1232, 7), (221, 13), (961, 31)],
                         ids=lambda v: str(v))
def test_zero_extended_first_pass(gpu, n, first):
    """set_codes_padded(code[:n_in]) skips the first pass's loads of the inputs that are
    zero for every butterfly (r >= ceil(n_in / (N/R))); set_codes of the same row
    zero-extended loads them.  The skipped values are exact zeros and every later
    operation is the same, so the power rows are byte-identical; the row is also held
    to the oracle at the tight bar."""
    r, _ = _both_orders(gpu, n)
    assert r[0] == first
    codes, IF = S.scene(n)
    fs, f = S.fs_of(n), S.BINS[S.PLANTED]
    short = gpu.AcqCtx(fs, n, max_freqs=2, max_blocks=2, max_codes=1)
    full = gpu.AcqCtx(fs, n, max_freqs=2, max_blocks=2, max_codes=1)
    worst = 0.0
    for n_in in (1, n // first - 1, n // first, n // first + 1, n - 1):
        ext = np.zeros((1, n), np.int8)
        ext[0, :n_in] = codes[0, :n_in]
        short.set_codes_padded(ext[:, :n_in])
        full.set_codes(ext)
        ref = A.power_rows(IF, fs, ext[0], f)
        for blk in (0, 1):
            a = short.power_row(IF, 2, blk, f, 0)
            b = full.power_row(IF, 2, blk, f, 0)
            assert a.tobytes() == b.tobytes(), (n, n_in, blk)
            worst = max(worst, _row_error(a, ref[blk], (n, n_in, blk)))
    print(f"[radix zero-extended first pass N={S.case_id(n)}] {worst:.3e}")
    assert worst < TIGHT, (S.case_id(n), worst)


# ---- e. the ends of the accepted range -----------------------------------------------------
@pytest.mark.parametrize("n,fs,plan", [
    (64, 64.0e3, (4, 16)),                    # the shortest: N / R = 4 butterflies of the last pass
    (1 << 19, 1000.0 * (1 << 19), (8, 16, 16, 16, 16)),   # the longest: the largest indices
    #                                           of d_twN, of the row stride and of the pass grid
    (67, 67.0e3, ()),                         # prime: the chirp-z engine at its shortest (M = 256)
    (524287, 524.287e6, ()),                  # prime: and at its longest (M = 2^20)
    (16100, 16.1e6, (4, 5, 7, 23, 5)),        # 4 x 5^2 x 7 x 23: a receiver's length with a 23
], ids=["64-4x16", "524288-8x16x16x16x16", "67-chirpz", "524287-chirpz", "16100-4x5x7x23x5"])
def test_range_ends(gpu, n, fs, plan):
    assert tuple(gpu.acq_mix_plan(n)[0]) == plan
    assert fs == S.fs_of(n)
    codes, IF = S.scene(n)
    ctx = gpu.AcqCtx(fs, n, max_freqs=2, max_blocks=2, max_codes=1)
    ctx.set_codes(codes[:1])
    got = ctx.power_row(IF, 2, 1, S.BINS[S.PLANTED], 0)
    ref = S.oracle_rows(n, 0, S.PLANTED)[1]
    err = _row_error(got, ref, n)
    assert int(np.argmax(ref)) == n // 3
    print(f"[radix range end N={n}] {err:.3e}")
