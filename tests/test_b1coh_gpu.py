"""GPU: the COMPASS B1 coherent searches (COMPASS/B1/acquisition_7x3ms.sci,
acquisition_4x5ms.sci) on the generic engines -- overlapping blocks
(gnsscorr_acq_set_block_stride) and the concatenated row (GNSSCORR_ACQ_CONCAT) --
against the restatement in tests/b1coh_scenarios.py.

Small shape: fs 2 Msps, S = 200, M = keep = stride = 600, L = 1200, 7 blocks, a row of
4200 lags, an aperiodic random +-1 code, noise-free integer records (a copy of the code
placed from record sample p correlates at concatenated lag p).  Each case plants the
peak (amplitude 6), a decoy (3) one period away that only the circular window admits,
and a copy (2) on an edge of the range of :159-176; tests/test_b1coh_cpu.py shows every
scene decidable at 1e-6.  Held to the project's fp64 bar (test_acq_gpu.check_rows:
argmax, block, bin and code phase exact, values within 1e-6 and in the fp64 class).
Every test here fails on the parent, which has neither the setter nor the mode.
"""
import numpy as np
import pytest

import b1coh_scenarios as C
import b1i_scenarios as B
from test_acq_gpu import check_rows

pytestmark = pytest.mark.gpu
EINVAL = -1


def _engine(monkeypatch, engine):
    monkeypatch.setenv("GNSSCORR_ACQ_BLUESTEIN", "1" if engine == "bluestein" else "0")


def _ctx(gpu, max_blocks=C.NB, stride=C.M, **kw):
    kw.setdefault("max_freqs", 4)
    kw.setdefault("max_codes", 1)
    ctx = gpu.AcqCtx(C.FS, C.L, max_blocks=max_blocks, **kw)
    ctx.set_zero_padded(C.M)
    ctx.set_codes_padded(C.code()[None, :])
    if stride:
        ctx.set_block_stride(stride)
    return ctx


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("period", [C.S, 0], ids=["period", "circular"])
@pytest.mark.parametrize("engine", ["mixed", "bluestein"])
def test_concatenated_row_statistics(gpu, engine, period, monkeypatch):
    """Peaks at s, s + 1, S - s - 1, S - s, M - 1, M, M + s, M + S - s - 1, M + S - s, 6 M and
    7 M - 1 for s = 2 and 7: every branch of the range, its edges on either side of a block
    boundary, the first and the last lag of the row."""
    _engine(monkeypatch, engine)
    ctx = _ctx(gpu)
    ctx.set_peak_period(period)
    for a, s, edge in C.cases():
        ref, ref_rows = C.reference(a, s, edge, period)
        res, rows = ctx.search(C.scene_if(a, s, edge), C.NB, C.FREQS, [0], C.GF, spc=s,
                               mode=gpu.ACQ_CONCAT)
        check_rows(res, rows, ref, ref_rows, True, label=f"b1coh-{engine}-{period}-{a}-{s}")
        assert rows[0, 1]["argmax"] == a and rows[0, 1]["block"] == a // C.M
        assert res[0]["code_phase"] == a + 1 and res[0]["bin"] == 1
        assert res[0]["carr_freq"] == 0.0 and res[0]["pad"] == 0


@pytest.mark.parametrize("engine", ["mixed", "bluestein"])
def test_chunks_hold_whole_rows(gpu, engine, monkeypatch):
    """max_codes 1 x max_freqs 3 x max_blocks 8 caps the chunk at 24 rows, no multiple of
    7; 5 groups x 3 bins x 7 blocks are 105 units, so several chunks of 21.  The groups'
    peaks lie in blocks 1, 4 and 6.  Equal to the restatement and, byte for byte, to the
    same groups searched one at a time."""
    _engine(monkeypatch, engine)
    G, nb = C.CH_GF.shape
    cap = 1 * 3 * 8
    assert cap % C.NB and G * nb * C.NB > cap          # more than one chunk, none of whole rows
    ctx = _ctx(gpu, max_blocks=8, max_freqs=3)
    ctx.set_peak_period(C.S)
    IF = C.chunk_if()
    res, rows = ctx.search(IF, C.NB, C.CH_FREQS, np.zeros(G, int), C.CH_GF, spc=7,
                           mode=gpu.ACQ_CONCAT)
    ref, ref_rows = C.search(IF, C.FS, C.code()[None, :], C.L, C.NB, C.CH_FREQS, C.CH_GF,
                             group_code=np.zeros(G, int), spc=7, period=C.S)
    check_rows(res, rows, ref, ref_rows, True, label=f"b1coh-chunks-{engine}")
    assert [int(rows[g, res[g]["bin"]]["block"]) for g in range(G)] == [1, 4, 6, 1, 4]
    for g in range(G):
        one = ctx.search(IF, C.NB, C.CH_FREQS, [0], C.CH_GF[g:g + 1], spc=7, mode=gpu.ACQ_CONCAT)
        assert one[0].tobytes() == res[g:g + 1].tobytes(), g
        assert one[1].tobytes() == rows[g:g + 1].tobytes(), g


def _levels(seed, n):
    return (2 * np.random.default_rng(seed).integers(0, 4, n) - 3).astype(np.int8)


@pytest.mark.parametrize("fmt", ["int8-iq", "packed-iq", "packed-real"])
@pytest.mark.parametrize("engine", ["mixed", "bluestein"])
def test_stride_alone_is_a_shifted_record(gpu, engine, fmt, monkeypatch):
    """Best-of-blocks and non-coherent searches of 3 blocks at stride = keep equal, byte
    for byte, the same searches without a stride of a record that holds the three
    overlapping blocks copied out end to end; so does every block's power row.  The
    strided record is exactly (n_blocks - 1) * stride + n_samples samples long and the
    context fresh, so a host copy of another length would show."""
    _engine(monkeypatch, engine)
    iq, packed = fmt.endswith("iq"), fmt.startswith("packed")
    ne, nblk = (2 if iq else 1), 3
    n_rec = (nblk - 1) * C.M + C.L
    lv = _levels(77, n_rec * ne)
    c8 = C.code().astype(np.int64)
    for p in (130, 900, 1700):       # a copy of the code per block, on the I arm
        lv[p * ne:(p + C.M) * ne:ne] = np.where(c8 > 0, 3, -3)
    unrolled = np.concatenate([lv[b * C.M * ne:(b * C.M + C.L) * ne] for b in range(nblk)])
    flags = gpu.iq_flags(iq, packed)
    enc = gpu.pack2 if packed else (lambda v: v)
    strided, plain = _ctx(gpu, max_blocks=nblk), _ctx(gpu, max_blocks=nblk, stride=0)
    for mode in (gpu.ACQ_BEST_OF_BLOCKS, gpu.ACQ_NONCOHERENT):
        for period in (0, C.S):
            strided.set_peak_period(period)
            plain.set_peak_period(period)
            a = strided.search(enc(lv), nblk, C.FREQS, [0], C.GF, spc=7, iq=flags, mode=mode)
            b = plain.search(enc(unrolled), nblk, C.FREQS, [0], C.GF, spc=7, iq=flags, mode=mode)
            assert _same(a, b), (mode, period)
            assert a[0][0]["peak"] > 0
    for blk in range(nblk):
        pa = strided.power_row(enc(lv), nblk, blk, 0.0, 0, iq=flags)
        pb = plain.power_row(enc(unrolled), nblk, blk, 0.0, 0, iq=flags)
        assert pa.tobytes() == pb.tobytes(), blk
    # a shorter host record is refused before anything is copied
    with pytest.raises(gpu.GnssCorrError, match="stride"):
        strided.search(enc(lv[:-4 * ne]), nblk, C.FREQS, [0], C.GF, spc=7, iq=flags)


@pytest.mark.parametrize("engine", ["mixed", "bluestein"])
def test_identical_blocks_report_the_first(gpu, engine, monkeypatch):
    """A record periodic in M makes the 7 blocks bit-identical: the concatenated row's
    argmax is in block 0 (Scilab's max keeps the first), while best-of-blocks on the same
    record still reports the last block (acq_peak.h's pinned rule)."""
    _engine(monkeypatch, engine)
    IF = np.zeros(2 * C.N_REC, np.int8)
    IF[0::2] = np.tile(5 * np.roll(C.code(), 37), C.N_REC // C.M + 1)[:C.N_REC]
    ctx = _ctx(gpu)
    res, rows = ctx.search(IF, C.NB, C.FREQS, [0], C.GF, spc=7, mode=gpu.ACQ_CONCAT)
    assert (rows["block"] == 0).all() and (rows["argmax"] < C.M).all()
    assert rows[0, 1]["argmax"] == 37 and res[0]["code_phase"] == 38
    best, brows = ctx.search(IF, C.NB, C.FREQS, [0], C.GF, spc=7, mode=gpu.ACQ_BEST_OF_BLOCKS)
    assert (brows["block"] == C.NB - 1).all()
    assert (brows["peak"] == rows["peak"]).all() and (brows["argmax"] == rows["argmax"]).all()


def test_refusals_and_reset(gpu):
    lib = gpu.lib()

    def refused(rc, word):
        assert rc == EINVAL
        assert word in lib.gnsscorr_last_error().decode()

    IF = C.scene_if(C.M, 7, "hi")
    end_to_end = np.zeros(2 * C.NB * C.L, np.int8)      # 7 blocks without a stride
    c = gpu.AcqCtx(C.FS, C.L, max_freqs=4, max_blocks=C.NB, max_codes=1)
    refused(lib.gnsscorr_acq_set_block_stride(c.h, C.M), "zero-padded")       # mode off
    assert lib.gnsscorr_acq_set_block_stride(c.h, 0) == 0
    c.set_codes_padded(C.code()[None, :])
    with pytest.raises(gpu.GnssCorrError, match="zero-padded"):               # CONCAT, mode off
        c.search(end_to_end, C.NB, C.FREQS, [0], C.GF, spc=7, mode=gpu.ACQ_CONCAT)
    c.set_zero_padded(C.M)
    refused(lib.gnsscorr_acq_set_block_stride(c.h, C.L + 1), "stride")
    refused(lib.gnsscorr_acq_set_block_stride(c.h, -1), "stride")
    c.set_block_stride(C.L)                                                   # == n_samples: fine
    for stride in (0, C.M - 1, C.L):                                          # stride != keep
        c.set_block_stride(stride)
        with pytest.raises(gpu.GnssCorrError, match="stride"):
            c.search(end_to_end, C.NB, C.FREQS, [0], C.GF, spc=7, mode=gpu.ACQ_CONCAT)
    c.set_block_stride(C.M)
    c.set_peak_period(C.S)
    for spc in (C.S // 2, C.S // 2 + 1):                                      # period <= 2 spc
        with pytest.raises(gpu.GnssCorrError, match="2 spc < period"):
            c.search(IF, C.NB, C.FREQS, [0], C.GF, spc=spc, mode=gpu.ACQ_CONCAT)
    with pytest.raises(gpu.GnssCorrError, match="bad arguments"):             # no mode 3
        c.search(IF, C.NB, C.FREQS, [0], C.GF, spc=7, mode=3)
    res, _ = c.search(IF, C.NB, C.FREQS, [0], C.GF, spc=C.S // 2 - 1, mode=gpu.ACQ_CONCAT)
    assert res[0]["code_phase"] == C.M + 1
    # set_zero_padded(0) clears the stride (and the period); the context then equals a
    # fresh one, unpadded and padded again
    c.set_zero_padded(0)
    assert c.block_stride == 0
    fresh = gpu.AcqCtx(C.FS, C.L, max_freqs=4, max_blocks=C.NB, max_codes=1)
    fresh.set_codes_padded(C.code()[None, :])
    two = IF[:2 * 2 * C.L]
    assert _same(c.search(two, 2, C.FREQS, [0], C.GF, spc=7),
                 fresh.search(two, 2, C.FREQS, [0], C.GF, spc=7))
    c.set_zero_padded(C.M)
    fresh.set_zero_padded(C.M)
    for mode in (gpu.ACQ_BEST_OF_BLOCKS, gpu.ACQ_NONCOHERENT):
        assert _same(c.search(two, 2, C.FREQS, [0], C.GF, spc=7, mode=mode),
                     fresh.search(two, 2, C.FREQS, [0], C.GF, spc=7, mode=mode))
    with pytest.raises(gpu.GnssCorrError, match="stride"):                    # cleared: refused
        c.search(end_to_end, C.NB, C.FREQS, [0], C.GF, spc=7, mode=gpu.ACQ_CONCAT)


# ---- the receiver's shapes -------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    IF, chans = B.scene()
    return IF, chans, B.settings()


def _real_search(gc, IF, chans, s, mode, band_khz):
    coh, nblk = C.MODES[mode]["coh"], C.MODES[mode]["segments"]
    fs, S_ = 16e6, 16000
    M = coh * S_
    prns = [c[0] for c in chans]
    ref = C.acquire(IF, s, prns, mode, band_khz=band_khz)
    frq = gc.b1_coh_bins(s["IF"], band_khz, coh)
    assert np.array_equal(frq, C.bins(s, coh, band_khz))
    rows = np.stack([gc.sample_code(gc.b1i_code(p), 2.046e6, fs, S_) for p in prns])
    acq = gc.AcqCtx(fs, 2 * M, max_freqs=len(frq), max_blocks=nblk, max_codes=4)
    acq.set_zero_padded(M)
    acq.set_block_stride(M)
    acq.set_peak_period(S_)
    acq.set_codes_padded(-np.tile(rows, (1, coh)))
    n_rec = (nblk - 1) * M + 2 * M
    assert n_rec == {3: 24, 5: 25}[mode] * S_          # within postProcessing.sce:91's 25 periods
    res, _ = acq.search(IF[:2 * n_rec], nblk, frq, np.arange(4),
                        np.tile(np.arange(len(frq)), (4, 1)), spc=8, mode=gc.ACQ_CONCAT)
    for g, a in enumerate(ref):
        assert res[g]["bin"] == a["bin"] and res[g]["code_phase"] == a["code_phase"], g
        assert res[g]["carr_freq"] == a["carr_freq"]
        assert abs(res[g]["metric"] - a["metric"]) <= 1e-6 * a["metric"]
        assert abs(res[g]["peak"] - a["peak"]) <= 1e-6 * a["peak"]
    return prns, ref, res


def test_3ms_search(gpu, scene):
    """acquisition_7x3ms.sci, the receiver's default (initSettings.sci:84): L = 96 000,
    7 blocks, 49 bins of 1000/6 Hz over 8 kHz, spc 8, period 16 000, on the scene's four
    PRNs; three of the four second-peak ranges straddle a block boundary
    (tests/test_b1coh_cpu.py holds the restatement's table and margins).  Bin, code phase
    and carr_freq exact, metric and peak within 1e-6."""
    IF, chans, s = scene
    _, ref, res = _real_search(gpu, IF, chans, s, 3, 8.0)
    assert sum(a["straddles"] for a in ref) == 3 and (res["code_phase"] > 16000).all()


def test_3ms_search_hands_over_to_the_tracker(gpu):
    """The same search, then init_chans from its concatenated code phases and 30
    closed-loop epochs that agree with the restatement started from the same values and
    end locked.  On the scene generated 52 ms long: a peak in the last segment starts its
    channel up to 21 code periods into the record, and the 43 ms record ends 27 epochs
    after PRN 6's start (sample 249 931).  The longer record draws other noise, so its
    decisions are shown decidable here (margins >= 1e-4, as the CPU tier asks of the
    43 ms one)."""
    from test_b1i_gpu import _check_closed_loop
    gc = gpu
    IF, chans = B.scene(n_ms=52)
    s = B.settings()
    prns, ref, res = _real_search(gc, IF, chans, s, 3, 8.0)
    assert all(min(a["margins"]) >= 1e-4 for a in ref)
    assert any(a["straddles"] for a in ref) and (res["code_phase"] > 16000).any()
    n = len(IF) // 2
    d_if = gc.DevBuf.from_array(IF)
    ctx = gc.SgtCtx(2)
    ch = ctx.init_chans(prns, res["code_phase"], res["carr_freq"])
    ep = ctx.track(d_if.ptr, 0, n, ch, 30, closed_loop=True)
    for i, a in enumerate(ref):
        r = B.track(IF, s, prns[i], a["code_phase"], a["carr_freq"], 30)
        _check_closed_loop(ep, i, r, 30)
        assert (np.abs(ep["I_P"][i][-10:]) > np.abs(ep["Q_P"][i][-10:])).all()


def test_5ms_search(gpu, scene):
    """acquisition_4x5ms.sci: L = 160 000, 4 blocks, 61 bins of 100 Hz over 6 kHz (the
    planted Dopplers are within +-2.5 kHz)."""
    IF, chans, s = scene
    _, ref, _ = _real_search(gpu, IF, chans, s, 5, 6.0)
    assert any(a["straddles"] for a in ref)
