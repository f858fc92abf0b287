"""GPU parity of the zero-padded long-code acquisition (Galileo E1B search semantics,
GALILEO/E1/acquisition.sci:45-165): gnsscorr_acq_set_zero_padded +
gnsscorr_acq_set_codes_padded against the fp64 numpy restatement in
tests/e1b_scenarios.py.

Held to the project's fp64 bar (test_acq_gpu.check_rows, f64): powers, peaks, second
peaks and metrics within 1e-6 relative, argmax, bin, block and code phase exact.  Every
scene is first shown decidable in the restatement itself (e1b_scenarios.assert_decidable:
peak and second peak clear of their runners-up by more than 1e-6 relative), so no
comparison can turn on rounding.
"""
import os

import numpy as np
import pytest

import e1b_scenarios as E
from test_acq_gpu import check_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 2.0e6
EINVAL = -1


def _codes(n, code_len, seed):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([-1, 1], np.int8), (n, code_len))


def _ctx(gpu, L, keep, codes, fs=FS, max_blocks=2, max_freqs=8):
    ctx = gpu.AcqCtx(fs, L, max_freqs=max_freqs, max_blocks=max_blocks, max_codes=len(codes))
    ctx.set_zero_padded(keep)
    ctx.set_codes_padded(codes)
    return ctx


def _search(gpu, ctx, IF, L, keep, codes, freqs, gf, spc, nb, nc, fs=FS):
    mode = gpu.ACQ_NONCOHERENT if nc else gpu.ACQ_BEST_OF_BLOCKS
    ref, ref_rows, full = E.acquire(IF, fs, codes, L, keep, freqs, gf, spc=spc, n_blocks=nb,
                                    noncoherent=nc)
    E.assert_decidable(ref, ref_rows, spc)
    res, rows = ctx.search(IF, nb, freqs, np.arange(len(codes)), gf, spc=spc, mode=mode)
    return res, rows, ref, ref_rows, full


# ---- 1. parity at small L, both engines -----------------------------------------------
@pytest.mark.parametrize("engine", ["mixed", "bluestein"])
@pytest.mark.parametrize("L,keep", [(2000, 1000),    # 16 x 5^3: the pruned half last pass
                                    (2046, 1023),    # 2 x 3 x 11 x 31: last radix 2
                                    (2018, 1009),    # 1009 prime: Bluestein either way
                                    (2000, 750)])    # keep != L/2: the bounded last pass
def test_parity_small(gpu, L, keep, engine, monkeypatch):
    monkeypatch.setenv("GNSSCORR_ACQ_BLUESTEIN", "1" if engine == "bluestein" else "0")
    codes = _codes(2, keep, 100 + L + keep)
    ctx = _ctx(gpu, L, keep, codes)
    freqs = 0.4e6 + 250.0 * np.arange(5)
    gf = np.tile(np.arange(5), (2, 1))
    # code 0 at lag 37 in both blocks (stronger in the second), code 1 at lag keep - 3
    # of the first block; Doppler on bin 3 / bin 1
    parts = [(codes[0], 3.0, 37, freqs[3]), (codes[0], 4.0, L + 37, freqs[3]),
             (codes[1], 3.5, keep - 3, freqs[1])]
    IF = E.synth_if(2 * L, parts, FS, noise=3.0, seed=L + keep)
    for nb in (1, 2):
        for nc in (False, True):
            res, rows, ref, ref_rows, _ = _search(gpu, ctx, IF, L, keep, codes, freqs, gf, 4,
                                                  nb, nc)
            check_rows(res, rows, ref, ref_rows, True,
                       label=f"padded-{L}-{keep}-{engine}-nb{nb}-{'nc' if nc else 'best'}")
            assert ref[0]["code_phase"] == 38 and ref[0]["bin"] == 3
            assert ref[1]["code_phase"] == keep - 2 and ref[1]["bin"] == 1
            assert (rows["argmax"] < keep).all()
            if nb == 2 and not nc:              # the stronger second block was chosen
                assert ref_rows[0][3]["block"] == 1 and rows[0, 3]["block"] == 1


def test_four_step_context_runs_the_plain_passes(gpu, monkeypatch):
    """N = 16368 on the generic engine has a compiled four-step plan (48 x 341); a
    zero-padded search on such a context runs the plain mixed-radix passes instead."""
    monkeypatch.setenv("GNSSCORR_ACQ_GENERIC", "1")
    monkeypatch.setenv("GNSSCORR_ACQ_BLUESTEIN", "0")
    L, keep = 16368, 8184
    codes = _codes(1, keep, 16368)
    ctx = _ctx(gpu, L, keep, codes, fs=16.368e6, max_blocks=1, max_freqs=4)
    freqs = 2.42e6 + 500.0 * np.arange(3)
    gf = np.arange(3)[None, :]
    x = np.tile(codes[0], 3)[keep - 4000:keep - 4000 + L].astype(np.float64)
    x[4000 + keep:] *= 2.0                       # the discarded half holds the larger peak
    IF = E.synth_if(L, [(x, 2.0, 0, freqs[1])], 16.368e6, noise=3.0, seed=4)
    res, rows, ref, ref_rows, full = _search(gpu, ctx, IF, L, keep, codes, freqs, gf, 16, 1,
                                             False, fs=16.368e6)
    assert int(np.argmax(full[0][1])) == 4000 + keep
    check_rows(res, rows, ref, ref_rows, True, label="padded-16368-four-step-context")
    assert res[0]["code_phase"] == 4001 and res[0]["bin"] == 1


# ---- 2. the discarded half stays discarded --------------------------------------------
@pytest.mark.parametrize("engine", ["mixed", "bluestein"])
def test_discarded_half(gpu, engine, monkeypatch):
    """The second code period has twice the amplitude of the first, so the full
    L-lag row peaks at a lag >= keep; the search must answer from the kept lags."""
    monkeypatch.setenv("GNSSCORR_ACQ_BLUESTEIN", "1" if engine == "bluestein" else "0")
    L, keep, lag = 2000, 1000, 100
    codes = _codes(2, keep, 7)
    ctx = _ctx(gpu, L, keep, codes, max_blocks=1)
    freqs = 0.4e6 + 250.0 * np.arange(5)
    gf = np.tile(np.arange(5), (2, 1))
    # periodic code from sample lag - keep on (its tail fills samples 0 .. lag), the
    # period starting at lag + keep twice as strong
    x = np.tile(codes[0], 3)[keep - lag:keep - lag + L].astype(np.float64)
    x[lag + keep:] *= 2.0
    IF = E.synth_if(L, [(x, 3.0, 0, freqs[2])], FS, noise=3.0, seed=21)
    res, rows, ref, ref_rows, full = _search(gpu, ctx, IF, L, keep, codes, freqs, gf, 4, 1, False)
    assert int(np.argmax(full[0][2])) == lag + keep          # numpy: full-row maximum discarded
    assert int(np.argmax(full[0][2])) >= keep
    assert ref_rows[0][2]["argmax"] == lag
    assert rows[0, 2]["argmax"] == lag and (rows["argmax"] < keep).all()
    assert res[0]["code_phase"] == lag + 1 and res[0]["bin"] == 2
    check_rows(res, rows, ref, ref_rows, True, label=f"discarded-half-{engine}")


# ---- 3. the exclusion window wraps at keep ---------------------------------------------
@pytest.mark.parametrize("engine", ["mixed", "bluestein"])
@pytest.mark.parametrize("lag,lag2", [(0, 995), (1, 996), (999, 3)])
def test_window_wraps_at_keep(gpu, lag, lag2, engine, monkeypatch):
    """A strong second correlation peak within spc of the main one across the wrap at
    keep: excluded by the window circular in keep, and it would be `second` itself for
    a window circular in L (or one that does not wrap)."""
    monkeypatch.setenv("GNSSCORR_ACQ_BLUESTEIN", "1" if engine == "bluestein" else "0")
    L, keep, spc = 2000, 1000, 8
    codes = _codes(2, keep, 11)
    ctx = _ctx(gpu, L, keep, codes, max_blocks=1)
    freqs = 0.4e6 + 250.0 * np.arange(5)
    gf = np.tile(np.arange(5), (2, 1))
    IF = E.synth_if(L, [(codes[0], 4.0, lag, freqs[2]), (codes[0], 3.0, lag2, freqs[2])], FS,
                    noise=3.0, seed=31 + lag)
    res, rows, ref, ref_rows, full = _search(gpu, ctx, IF, L, keep, codes, freqs, gf, spc, 1,
                                             False)
    row = ref[0]["results"][2]
    assert ref_rows[0][2]["argmax"] == lag
    assert (lag2 - lag) % keep < spc or (lag - lag2) % keep < spc
    # the planted second peak is the largest kept value after the main peak, and a
    # window circular in L would report it
    assert int(np.argsort(row)[-2]) == lag2
    wrong = E.second_peak(full[0][2], lag, spc)
    assert wrong >= row[lag2] > 2.0 * ref_rows[0][2]["second"]
    check_rows(res, rows, ref, ref_rows, True, label=f"wrap-{lag}-{engine}")
    assert rows[0, 2]["argmax"] == lag
    assert abs(rows[0, 2]["second"] - ref_rows[0][2]["second"]) <= 1e-6 * ref_rows[0][2]["second"]


# ---- 4. the E1B shape ------------------------------------------------------------------
def test_e1b_shape(gpu):
    """L = 128000 = 2 x 64000 samples of 16 Msps against the three fixture codes sampled
    as makeE1BCodesTable.sci does; PRN 12 planted at 1234.5 chips, +250 Hz."""
    fs, S, L, spc = 16.0e6, 64000, 128000, 16
    chips = np.load(os.path.join(ROOT, "tests", "golden", "e1b_codes.npz"))["codes"]
    codes = np.stack([gpu.sample_boc_code(c, 1.023e6, fs, S) for c in chips])
    assert np.array_equal(codes[1], E.sample_boc(chips[1], 1.023e6, fs, S))
    bins = gpu.e1b_bins(2.42e6, 14, 4)
    assert len(bins) == 113
    k0 = int(np.argmin(np.abs(bins - (2.42e6 + 250.0))))
    assert bins[k0] == 2.42e6 + 250.0
    freqs = bins[k0 - 1:k0 + 2]
    gf = np.tile(np.arange(3), (3, 1))
    lag = int(round(1234.5 * fs / 1.023e6))
    # PRN 12's sampled code, periodic, its period starting at sample `lag`; the second
    # period sign-flipped (a data / secondary-code transition)
    x = np.tile(codes[1], 3)[S - lag:S - lag + L].astype(np.float64)
    x[lag + S:] *= -1.0
    IF = E.synth_if(L, [(x, 1.0, 0, 2.42e6 + 250.0)], fs, noise=4.0, seed=12)
    ctx = _ctx(gpu, L, S, codes, fs=fs, max_blocks=1, max_freqs=4)
    res, rows, ref, ref_rows, _ = _search(gpu, ctx, IF, L, S, codes, freqs, gf, spc, 1, False,
                                          fs=fs)
    check_rows(res, rows, ref, ref_rows, True, label="e1b-128000")
    assert res[1]["metric"] > 3.0                                  # acqThreshold
    assert res[1]["bin"] == 1 and res[1]["code_phase"] == lag + 1
    assert res[1]["carr_freq"] == 2.42e6 + 250.0
    assert res[0]["metric"] < 3.0 and res[2]["metric"] < 3.0


# ---- 5. refusals and isolation ---------------------------------------------------------
def test_refusals(gpu, monkeypatch):
    monkeypatch.delenv("GNSSCORR_ACQ_GENERIC", raising=False)
    L = gpu.lib()

    def refused(rc, word):
        assert rc == EINVAL
        assert word in L.gnsscorr_last_error().decode()

    f32 = gpu.AcqCtx(16.368e6, 16368, max_freqs=2, max_blocks=2, max_codes=1,
                     precision=gpu.ACQ_F32)
    refused(L.gnsscorr_acq_set_zero_padded(f32.h, 8184), "fp64")
    for fs, n in ((16.368e6, 16368), (16.0e6, 16000)):     # the register-resident plans
        c = gpu.AcqCtx(fs, n, max_freqs=2, max_blocks=2, max_codes=1)
        refused(L.gnsscorr_acq_set_zero_padded(c.h, n // 2), "generic")
        if n == 16368:                                      # with a group-record table too
            tab = gpu.DevBuf.from_array(np.zeros(1, np.int32))
            c.set_group_records(tab)
            refused(L.gnsscorr_acq_set_zero_padded(c.h, n // 2), "generic")
        assert L.gnsscorr_acq_set_zero_padded(c.h, 0) == 0  # turning it off is always fine
    c = gpu.AcqCtx(FS, 2000, max_freqs=2, max_blocks=4, max_codes=1)
    refused(L.gnsscorr_acq_set_zero_padded(c.h, 2001), "keep")
    refused(L.gnsscorr_acq_set_zero_padded(c.h, -1), "keep")
    c.set_coherent(2)
    refused(L.gnsscorr_acq_set_zero_padded(c.h, 1000), "code period")
    c.set_coherent(1)
    c.set_records(2)
    refused(L.gnsscorr_acq_set_zero_padded(c.h, 1000), "record")
    c.set_records(1)
    c.set_zero_padded(1000)
    # the other direction, while the mode is on
    refused(L.gnsscorr_acq_set_coherent(c.h, 2), "zero-padded")
    refused(L.gnsscorr_acq_set_records(c.h, 2), "zero-padded")
    tab = gpu.DevBuf.from_array(np.zeros(1, np.int32))
    assert L.gnsscorr_acq_set_group_records(c.h, tab.ptr) == EINVAL
    assert L.gnsscorr_acq_set_coherent(c.h, 1) == 0 and L.gnsscorr_acq_set_records(c.h, 1) == 0
    assert L.gnsscorr_acq_set_group_records(c.h, None) == 0
    # codes longer than the transform, and a window wider than the kept lags
    with pytest.raises(gpu.GnssCorrError):
        c.set_codes_padded(_codes(1, 2001, 1))
    c.set_codes_padded(_codes(1, 1000, 1))
    with pytest.raises(gpu.GnssCorrError):
        c.search(np.zeros(4000, np.int8), 1, np.array([0.4e6]), [0], [[0]], spc=501)


@pytest.mark.parametrize("engine", ["mixed", "bluestein"])
def test_mode_off_again_is_a_fresh_context(gpu, engine, monkeypatch):
    monkeypatch.setenv("GNSSCORR_ACQ_BLUESTEIN", "1" if engine == "bluestein" else "0")
    L = 2000
    codes = _codes(2, L, 5)
    freqs = 0.4e6 + 250.0 * np.arange(5)
    gf = np.tile(np.arange(5), (2, 1))
    IF = E.synth_if(2 * L, [(codes[0], 3.0, 1500, freqs[1]), (codes[1], 3.0, L + 20, freqs[4])],
                    FS, noise=3.0, seed=77)
    used = _ctx(gpu, L, 1000, codes[:, :1000])
    used.search(IF, 2, freqs, np.arange(2), gf, spc=4)          # a padded search first
    used.set_zero_padded(0)
    used.set_codes(codes)
    fresh = gpu.AcqCtx(FS, L, max_freqs=8, max_blocks=2, max_codes=2)
    fresh.set_codes(codes)
    for mode in (gpu.ACQ_BEST_OF_BLOCKS, gpu.ACQ_NONCOHERENT):
        a = used.search(IF, 2, freqs, np.arange(2), gf, spc=4, mode=mode)
        b = fresh.search(IF, 2, freqs, np.arange(2), gf, spc=4, mode=mode)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert (b[1]["argmax"] >= 1000).any()      # the unpadded search does see the far lags


# ---- 6. set_codes_padded against set_codes, mode off -----------------------------------
@pytest.mark.parametrize("fs,L,engine", [(FS, 2000, "mixed"), (FS, 2000, "bluestein"),
                                         (16.368e6, 16368, "compiled")])
def test_codes_padded_full_length_equals_set_codes(gpu, fs, L, engine, monkeypatch):
    monkeypatch.setenv("GNSSCORR_ACQ_BLUESTEIN", "1" if engine == "bluestein" else "0")
    codes = _codes(2, L, 9)
    IF = E.synth_if(2 * L, [(codes[1], 3.0, 300, 0.4e6)], fs, noise=3.0, seed=5)
    rows = []
    for padded in (False, True):
        ctx = gpu.AcqCtx(fs, L, max_freqs=2, max_blocks=2, max_codes=2)
        (ctx.set_codes_padded if padded else ctx.set_codes)(codes)
        rows.append([ctx.power_row(IF, 2, blk, 0.4e6, code) for code in (0, 1) for blk in (0, 1)])
    for a, b in zip(*rows):
        assert a.shape == (L,) and a.tobytes() == b.tobytes()
    assert int(np.argmax(rows[0][2])) == 300


def test_power_row_is_the_full_row_in_padded_mode(gpu):
    """gnsscorr_acq_power_row is unchanged by the mode: L doubles, the full
    linear-correlation row, equal to the restatement's."""
    L, keep = 2000, 1000
    codes = _codes(1, keep, 3)
    ctx = _ctx(gpu, L, keep, codes, max_blocks=1)
    IF = E.synth_if(L, [(codes[0], 3.0, 1200, 0.4e6)], FS, noise=3.0, seed=8)
    got = ctx.power_row(IF, 1, 0, 0.4e6, 0)
    _, _, full = E.acquire(IF, FS, codes, L, keep, np.array([0.4e6]), [[0]], spc=4)
    assert got.shape == (L,) and int(np.argmax(got)) == 1200
    assert np.abs(got - full[0][0]).max() <= 1e-9 * full[0][0].max()
    res, rows = ctx.search(IF, 1, np.array([0.4e6]), [0], [[0]], spc=4)
    assert rows[0, 0]["argmax"] < keep                    # and the mode is still on
