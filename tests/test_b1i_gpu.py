"""GPU parity of BeiDou B1I in the float tracker (system 2 of gnsscorr_sgt_*) against the
restatement of COMPASS/B1/tracking.sci:123-357 and acquisition.sci:86-168 in
tests/b1i_scenarios.py.

Tolerances are those of tests/test_sgt_gpu.py: blksize, pos, rem_code and rem_carr
exact; the six sums within 1e-6 |ref| + 1e-6; closed-loop fields within 1e-6 relative
with every blksize exact (the scene is shown decidable at a ten times tighter bound in
tests/test_b1i_cpu.py).
"""
import numpy as np
import pytest

import b1i_scenarios as B
import sgt_oracle as S
from tracker_checks import close as _close

pytestmark = pytest.mark.gpu
SUMS = B.SUMS


def _random_chans(gc, rng, C, n, fs, basis=2.046e6, spread=80.0):
    ch = np.zeros(C, gc.SGT_CHAN)
    ch["code_id"] = rng.integers(1, 38, C)
    ch["pos"] = rng.integers(0, n - int(fs * 0.00125), C)
    ch["code_freq"] = basis + rng.uniform(-spread, spread, C)
    ch["rem_code"] = rng.uniform(0, 1, C) * (ch["code_freq"] / fs)
    ch["rem_carr"] = rng.uniform(-6.2, 6.2, C)
    ch["carr_freq"] = rng.uniform(-3e6, 3e6, C)
    return ch


def _check_open_loop(IF, s, ch0, ch, ep):
    for i in range(len(ch0)):
        sums, blk, pos, rc, rcar = S.correlate(IF, s, B.padded_code(int(ch0["code_id"][i])),
                                               int(ch0["pos"][i]), float(ch0["rem_code"][i]),
                                               float(ch0["rem_carr"][i]),
                                               float(ch0["code_freq"][i]),
                                               float(ch0["carr_freq"][i]))
        assert ep["status"][i] == 0 and ep["blksize"][i] == blk, i
        assert ch["pos"][i] == pos
        assert ch["rem_code"][i] == rc, (i, ch["rem_code"][i], rc)
        assert ch["rem_carr"][i] == rcar, (i, ch["rem_carr"][i], rcar)
        got = np.array([ep[f][i] for f in SUMS])
        assert _close(got, sums).all(), (i, got, sums)
    assert (ch["carr_freq"] == ch0["carr_freq"]).all()
    assert (ch["code_freq"] == ch0["code_freq"]).all()


def _open_loop(gc, IF, n, ch, **kw):
    d_if = gc.DevBuf.from_array(IF)
    ctx = gc.SgtCtx(2, **kw)
    ch0 = ch.copy()
    ep = ctx.track(d_if.ptr, 0, n, ch, 1, closed_loop=False)[:, 0]
    _check_open_loop(IF, B.settings(**kw), ch0, ch, ep)
    return ch, ep


@pytest.mark.parametrize("fs", [16e6, 16.368e6])
@pytest.mark.parametrize("threads", [None, "64", "1024"])
@pytest.mark.parametrize("file_type", [2, 1])
def test_open_loop_epoch_matches_restatement(gpu, file_type, threads, fs, monkeypatch):
    """96 channels on random states over a 200 000-sample record, 7.82 (16 Msps) and 8.0
    (16.368 Msps) samples per chip, in the 256-thread, the wave and the 1024-thread
    shape.  The wave shape (threads "64") with fileType 2 takes the select form on
    8-sample chunks, every other case the per-sample loop (DESIGN.md "BeiDou B1I")."""
    gc = gpu
    if threads:
        monkeypatch.setenv("GNSSCORR_SGT_THREADS", threads)
    rng = np.random.default_rng(300 + file_type + (7 if fs > 16e6 else 0))
    n = 200000
    IF = gc.ifgen(n, [], fs=fs, iq=file_type == 2, seed=41)
    _open_loop(gc, IF, n, _random_chans(gc, rng, 96, n, fs), fileType=file_type, samplingFreq=fs)


@pytest.mark.parametrize("threads", [None, "64"])
@pytest.mark.parametrize("spc", [0.125, 0.25, 0.1])
def test_open_loop_crossings_on_exact_samples(gpu, spc, threads, monkeypatch):
    """16.368 Msps at exactly 2.046 Mcps: step = 0.125, and with rem_code on the 1/8 grid
    every prompt crossing (and for spacings on the grid every early / late crossing) lies
    on an exact sample, where the select form's crossing estimate has no margin and its
    exact per-sample rescan decides (threads "64"; the 256-thread shape runs the
    per-sample loop either way).  The chunk path and GNSSCORR_SGT_CHUNK=0 both agree with
    the restatement, and with each other exactly on the exact fields."""
    gc = gpu
    fs = 16.368e6
    if threads:
        monkeypatch.setenv("GNSSCORR_SGT_THREADS", threads)
    rng = np.random.default_rng(int(spc * 1000))
    n = 120000
    IF = gc.ifgen(n, [], fs=fs, seed=43)
    C = 32
    ch = _random_chans(gc, rng, C, n, fs, spread=0.0)
    assert (ch["code_freq"] == 2.046e6).all()
    ch["rem_code"] = 0.125 * rng.integers(0, 4, C)      # 0 or 0.125 j
    ch["rem_code"][:4] = 0.0
    out = {}
    for chunk in ("1", "0"):
        monkeypatch.setenv("GNSSCORR_SGT_CHUNK", chunk)
        out[chunk] = _open_loop(gc, IF, n, ch.copy(), samplingFreq=fs, dllCorrelatorSpacing=spc)
    (ca, ea), (cb, eb) = out["1"], out["0"]
    for f in ("pos", "rem_code", "rem_carr"):
        assert (ca[f] == cb[f]).all(), f
    assert (ea["blksize"] == eb["blksize"]).all()
    if threads == "64":
        # the select form adds each chunk's samples before it rotates and accumulates, the
        # per-sample loop adds sample by sample: 32 x 6 sums of 16 368 terms in two orders
        # cannot all be bit-equal, so equal sums would mean the chunk path was not taken
        assert any((ea[f] != eb[f]).any() for f in SUMS)


@pytest.mark.parametrize("threads", [None, "64"])
def test_open_loop_wide_spacing_takes_the_select_form(gpu, threads, monkeypatch):
    """dllCorrelatorSpacing = 0.6 at 16 Msps is floor(0.6 / 0.128) = 4 samples, above the
    limit of 3 a chip-aligned chunk path has: the select form in the wave shape (threads
    "64"), whose early and late crossings then lie in other chunks than the prompt one;
    the per-sample loop in the 256-thread shape."""
    gc = gpu
    if threads:
        monkeypatch.setenv("GNSSCORR_SGT_THREADS", threads)
    rng = np.random.default_rng(61)
    n = 200000
    IF = gc.ifgen(n, [], fs=16e6, seed=47)
    _open_loop(gc, IF, n, _random_chans(gc, rng, 96, n, 16e6), dllCorrelatorSpacing=0.6)


def test_open_loop_low_rate_takes_the_per_sample_path(gpu):
    """4.092 Msps: two samples per chip, no chunk shape applies."""
    gc = gpu
    fs = 4.092e6
    rng = np.random.default_rng(67)
    n = int(fs * 0.012)
    IF = gc.ifgen(n, [], fs=fs, seed=53)
    ch = _random_chans(gc, rng, 64, n, fs)
    ch["rem_code"][:4] = 0.0
    ch["rem_code"][4:8] = np.nextafter(ch["code_freq"][4:8] / fs, 0)
    _open_loop(gc, IF, n, ch, samplingFreq=fs)


@pytest.fixture(scope="module")
def scene():
    IF, chans = B.scene()
    s = B.settings()
    runs = [B.track(IF, s, c[0], c[1], B.scene_acq_freq(c), B.SCENE_MS) for c in chans]
    return IF, chans, s, runs


def _scene_chans(ctx, chans):
    return ctx.init_chans([c[0] for c in chans], [c[1] for c in chans],
                          [B.scene_acq_freq(c) for c in chans])


def _check_closed_loop(ep, i, r, n):
    assert (ep["status"][i][:n] == 0).all()
    assert (ep["blksize"][i][:n] == r["blksize"][:n]).all()
    for f in B.FIELDS:
        ok = _close(ep[f][i][:n], r[f][:n])
        assert ok.all(), (i, f, np.flatnonzero(~ok)[:5], ep[f][i][:n][~ok][:3], r[f][:n][~ok][:3])


@pytest.mark.parametrize("threads", [None, "64"])
def test_closed_loop_scene_continuation_and_replay(gpu, scene, threads, monkeypatch):
    """4 PRNs x 40 epochs against the restatement; 20 + 20 epochs through the saved channel
    state equal the 40-epoch call bit for bit; gnsscorr_sgt_replay on the run's own sums
    reproduces its records.  threads "64": the wave shape, i.e. the select form."""
    gc = gpu
    if threads:
        monkeypatch.setenv("GNSSCORR_SGT_THREADS", threads)
    IF, chans, s, runs = scene
    n = len(IF) // 2
    d_if = gc.DevBuf.from_array(IF)
    ctx = gc.SgtCtx(2)
    ch = _scene_chans(ctx, chans)
    ch_init = ch.copy()
    ep = ctx.track(d_if.ptr, 0, n, ch, B.SCENE_MS, closed_loop=True)
    for i, r in enumerate(runs):
        _check_closed_loop(ep, i, r, B.SCENE_MS)
        assert (np.abs(ep["I_P"][i][-10:]) > np.abs(ep["Q_P"][i][-10:])).all()
    # continuation
    ch2 = ch_init.copy()
    e1 = ctx.track(d_if.ptr, 0, n, ch2, 20, closed_loop=True)
    assert (ch2["n_epochs"] == 20).all()
    e2 = ctx.track(d_if.ptr, 0, n, ch2, 20, closed_loop=True)
    assert np.concatenate([e1, e2], axis=1).tobytes() == ep.tobytes()
    assert ch2.tobytes() == ch.tobytes()
    # replay of the run's own sums
    sums = np.stack([ep[f] for f in SUMS], axis=2)
    ch3 = ch_init.copy()
    rp = ctx.replay(ch3, sums)
    assert (rp["blksize"] == ep["blksize"]).all() and (rp["status"] == 0).all()
    for f in B.FIELDS:
        assert np.array_equal(rp[f], ep[f]), f
    for f in ("pos", "rem_code", "code_freq", "carr_freq", "old_code_nco", "old_carr_nco", "i1",
              "q1", "n_epochs"):
        assert np.array_equal(ch3[f], ch[f]), f


def test_out_of_data_stops_like_tracking_sci(gpu, scene):
    """tracking.sci:236-240: a record that ends mid-run gives status 1 and the blksize
    that did not fit."""
    gc = gpu
    IF, chans, s, _ = scene
    n = 16000 * 12 + 500
    short = IF[:2 * n]
    d_if = gc.DevBuf.from_array(short)
    ctx = gc.SgtCtx(2)
    ch = _scene_chans(ctx, chans)
    ep = ctx.track(d_if.ptr, 0, n, ch, 16, closed_loop=True)
    for i, c in enumerate(chans):
        r = B.track(short, s, c[0], c[1], B.scene_acq_freq(c), 16)
        k = len(r["I_P"])
        assert 0 < k < 16 and r["stop_blksize"] is not None
        _check_closed_loop(ep, i, r, k)
        assert (ep["status"][i][k:] == 1).all()
        assert ep["blksize"][i][k] == r["stop_blksize"]
        assert ch["status"][i] == 1 and ch["n_epochs"][i] == k


def test_search_hands_over_to_the_tracker(gpu, scene):
    """acquisition.sci:45-170 on the generic engine: n_samples = 32000, the first 16000
    lags kept, four sampled B1I codes zero-extended, 29 bins of 500 Hz around IF +- 7 kHz,
    one chip (8 samples) around the peak excluded, over the first 2 ms of the scene.  Bin
    and code phase exact, metrics within 1e-6; then init_chans from those results and 30
    closed-loop epochs that agree with the restatement and stay locked."""
    gc = gpu
    IF, chans, s, _ = scene
    fs, S_ = 16e6, 16000
    prns = [c[0] for c in chans]
    ref = B.acquire(IF, s, prns)
    codes = np.stack([gc.sample_code(gc.b1i_code(p), 2.046e6, fs, S_) for p in prns])
    frq = B.bins(s)
    assert len(frq) == 29
    acq = gc.AcqCtx(fs, 2 * S_, max_freqs=32, max_blocks=1, max_codes=4)
    acq.set_zero_padded(S_)
    acq.set_codes_padded(codes)
    res, _ = acq.search(IF[:4 * S_], 1, frq, np.arange(4), np.tile(np.arange(29), (4, 1)), spc=8)
    for g, a in enumerate(ref):
        assert res[g]["bin"] == a["bin"] and res[g]["code_phase"] == a["code_phase"], g
        assert res[g]["carr_freq"] == a["carr_freq"]
        assert abs(res[g]["metric"] - a["metric"]) <= 1e-6 * a["metric"]
        assert abs(res[g]["peak"] - a["peak"]) <= 1e-6 * a["peak"]
    n = len(IF) // 2
    d_if = gc.DevBuf.from_array(IF)
    ctx = gc.SgtCtx(2)
    ch = ctx.init_chans(prns, res["code_phase"], res["carr_freq"])
    ep = ctx.track(d_if.ptr, 0, n, ch, 30, closed_loop=True)
    for i, a in enumerate(ref):
        r = B.track(IF, s, prns[i], a["code_phase"], a["carr_freq"], 30)
        _check_closed_loop(ep, i, r, 30)
        assert (np.abs(ep["I_P"][i][-10:]) > np.abs(ep["Q_P"][i][-10:])).all()
