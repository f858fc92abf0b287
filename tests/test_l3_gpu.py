"""GPU parity: GLONASS L3OC float tracking (l3t.hip) and the L3 search hand-over against
the fp64 restatement of GLONASS/L3 (tests/l3_scenarios.py).

Tolerances are those of tests/test_e1t_gpu.py:
  * blksize, pos: exact; rem_code / rem_carr after open-loop epochs and every epoch's
    absoluteSample: bit-equal (same fp64 operation sequence, no contraction)
  * the twelve open-loop sums: |gpu - ref| <= 1e-6 |ref| + 1e-6
  * closed loop and replay: every per-epoch field within 1e-7 |ref| + 1e-7 of the
    restatement over the whole run, blksize exact: the bound tests/test_l3_cpu.py shows
    the scene decides under 1e-9 offsets of the sums.
"""
import numpy as np
import pytest

import l3_scenarios as L3
from tracker_checks import close as _close, noise

pytestmark = pytest.mark.gpu
_cache = {}
LOOP_TOL = 1e-7               # closed loop and replay: the bound of tests/test_l3_cpu.py
SHAPES = [None, "64"]          # GNSSCORR_L3T_THREADS: the 256-thread default, one wave per channel


def _noise(gc, n, fs):
    return noise(gc, n, fs, seed=33)


def _rows(prn):
    return L3.padded(L3.generate_code(prn)), L3.padded(L3.generate_code(prn + 32))


def _check_open_loop(gc, ctx, IF, s, ch, n_ep):
    """n_ep open-loop epochs of every channel in one call against L3.correlate."""
    n = len(IF) // 2
    ch0 = ch.copy()
    d_if = gc.DevBuf.from_array(IF)
    ep = ctx.track(d_if.ptr, 0, n, ch, n_ep, closed_loop=False)
    worst = 0.0
    for i in range(len(ch)):
        c = ch0[i]
        prow, drow = _rows(int(c["code_id"]))
        pos, rc, rcar = int(c["pos"]), float(c["rem_code"]), float(c["rem_carr"])
        for e in range(n_ep):
            st, blk, r = L3.correlate(IF, s, prow, drow, pos, rc, rcar, float(c["code_freq"]),
                                      float(c["carr_freq"]))
            assert st == 0, (i, e)
            sums, pos, rc, rcar = r
            assert ep["status"][i, e] == 0 and ep["blksize"][i, e] == blk, (i, e)
            want_abs = pos - rc * (s["samplingFreq"] / 1000) / s["codeLength"]
            assert ep["absoluteSample"][i, e] == want_abs, (i, e)
            got = np.array([ep[f][i, e] for f in L3.SUMS])
            assert _close(got, sums).all(), (i, e, got, sums)
            worst = max(worst, float((np.abs(got - sums) / np.abs(sums)).max()))
        assert ch["pos"][i] == pos and ch["n_epochs"][i] == n_ep
        assert ch["rem_code"][i] == rc, (i, ch["rem_code"][i], rc)
        assert ch["rem_carr"][i] == rcar, (i, ch["rem_carr"][i], rcar)
    for f in ("carr_freq", "code_freq"):
        assert (ch[f] == ch0[f]).all()
    print(f"[l3t open loop] max relative error of the sums: {worst:.3e}")
    return ep


def _chans(gc, rng, fs, n, n_ep, rem_codes, code_freq=None, carr=3e6):
    C = len(rem_codes)
    ch = np.zeros(C, gc.L3T_CHAN)
    ch["code_id"] = [1, 30, 31, 17, 9, 22][:C]
    ch["pos"] = rng.integers(0, n - int(fs * 0.00101 * n_ep) - 64, C)
    ch["code_freq"] = 10.23e6 + rng.uniform(-40, 40, C) if code_freq is None else code_freq
    ch["rem_code"] = rem_codes
    ch["rem_carr"] = rng.uniform(-6.2, 6.2, C)
    ch["carr_freq"] = rng.uniform(-carr, carr, C)
    ch["carr_freq_basis"] = ch["carr_freq"]
    return ch


@pytest.mark.parametrize("threads", SHAPES)
@pytest.mark.parametrize("switch_iq", [0, 1])
def test_open_loop_epochs_match_restatement(gpu, switch_iq, threads, monkeypatch):
    """24 Msps, 4 channels x 6 epochs.  rem_code 0 and 0.2 put the first early index
    ceil(rem_code - 0.4) on the front pad (entry 0 of [c(L) c c(1)]); 0.41 and 0.425
    (just under one step) start past it."""
    gc = gpu
    if threads:
        monkeypatch.setenv("GNSSCORR_L3T_THREADS", threads)
    fs, n = 24e6, 200000
    IF = _noise(gc, n, fs)
    s = L3.settings(switchIQ=switch_iq)
    ctx = gc.L3tCtx(switchIQ=switch_iq)
    ch = _chans(gc, np.random.default_rng(5 + switch_iq), fs, n, 6, [0.0, 0.2, 0.41, 0.425])
    _check_open_loop(gc, ctx, IF, s, ch, 6)


def test_many_channels_take_the_wave_shape(gpu):
    """1024 channels: the dispatcher's one-wave-per-channel launch, no override."""
    gc = gpu
    fs, n = 24e6, 200000
    IF = _noise(gc, n, fs)
    ctx = gc.L3tCtx()
    base = _chans(gc, np.random.default_rng(8), fs, n, 1, [0.0, 0.2, 0.41, 0.1])
    ch = np.tile(base, 256)
    d_if = gc.DevBuf.from_array(IF)
    ep = ctx.track(d_if.ptr, 0, n, ch, 1, closed_loop=False)[:, 0]
    few = base.copy()
    ep4 = _check_open_loop(gc, ctx, IF, L3.settings(), few, 1)[:, 0]
    for f in ("blksize", "status", "absoluteSample"):
        assert (ep[f].reshape(256, 4) == ep4[f]).all(), f
    assert ep.reshape(256, 4)[1:].tobytes() == np.tile(ep[:4], 255).tobytes()
    for f in L3.SUMS:                                   # 64 lanes against 256: other sum order
        assert _close(ep[f][:4], ep4[f]).all(), f


@pytest.mark.parametrize("threads", SHAPES)
def test_each_sum_has_its_own_code(gpu, threads, monkeypatch):
    """A scene with the pilot only, then the data channel only: the other code's six sums
    stay at the cross-correlation floor (a swapped row or a shared mask fails this)."""
    gc = gpu
    if threads:
        monkeypatch.setenv("GNSSCORR_L3T_THREADS", threads)
    fs, n = 24e6, 60000
    ctx = gc.L3tCtx()
    for which in ("pilot", "data"):
        IF = L3.synth_l3(n, 30, 3000.6, 1800.0, seed=6, pilot=which == "pilot",
                         data=which == "data")
        ch = ctx.init_chan(30, 3002, -2.025e6 + 1800.0)
        ep = ctx.track(gc.DevBuf.from_array(IF).ptr, 0, n, ch, 1, closed_loop=False)[0, 0]
        mag = {t: [np.hypot(ep["I_" + a + t], ep["Q_" + a + t]) for a in "EPL"] for t in ("", "2")}
        own, other = (mag[""], mag["2"]) if which == "pilot" else (mag["2"], mag[""])
        assert own[1] > 0.5 * 12.0 * 24000, (which, own)
        assert own[1] > own[0] and own[1] > own[2]
        assert max(other) < 0.05 * own[1], (which, own, other)


def test_open_loop_low_rate(gpu):
    """12 Msps: 1.17 samples per chip (step 0.85), where no several-samples-per-chip
    form could apply."""
    gc = gpu
    fs = 12e6
    n = int(fs * 0.006)
    IF = _noise(gc, n, fs)
    ctx = gc.L3tCtx(samplingFreq=fs)
    ch = _chans(gc, np.random.default_rng(41), fs, n, 2, [0.0, 0.3, 0.84, 0.5], carr=1e6)
    _check_open_loop(gc, ctx, IF, L3.settings(samplingFreq=fs), ch, 2)


@pytest.mark.parametrize("threads", SHAPES)
def test_open_loop_crossings_on_exact_chips(gpu, threads, monkeypatch):
    """fs = 20.46 Msps with codeFreq = 10.23 MHz: step = 0.5 exactly, and rem_code chosen
    so that the early (0.4 -> 0.0), prompt (0.0, 0.5) or late (0.6 -> 1.0, 0.1 -> 0.5)
    sequence lands on exact integers at every second sample."""
    gc = gpu
    if threads:
        monkeypatch.setenv("GNSSCORR_L3T_THREADS", threads)
    fs = 20.46e6
    n = int(fs * 0.004)
    IF = _noise(gc, n, fs)
    ctx = gc.L3tCtx(samplingFreq=fs)
    rem = [0.0, 0.5, 0.4, 0.6, 0.1]
    ch = _chans(gc, np.random.default_rng(3), fs, n, 1, rem, code_freq=10.23e6)
    ep = _check_open_loop(gc, ctx, IF, L3.settings(samplingFreq=fs), ch, 1)
    assert list(ep["blksize"][:, 0]) == [int(np.ceil((10230 - r) / 0.5)) for r in rem]


def _scene(gc):
    if "scene" not in _cache:
        IF, prn, cp, f0, _ = L3.closed_loop_scene()
        s = L3.settings()
        _cache["scene"] = (IF, prn, cp, f0, s, L3.track(IF, s, prn, cp, f0, L3.SCENE_MS))
    return _cache["scene"]


def _scene_ctx(gc):
    IF, prn, cp, f0, s, ref = _scene(gc)
    ctx = gc.L3tCtx()
    return ctx, gc.DevBuf.from_array(IF), len(IF) // 2, ctx.init_chan(prn, cp, f0)


@pytest.mark.parametrize("threads", SHAPES)
def test_closed_loop_20_ms(gpu, threads, monkeypatch):
    gc = gpu
    if threads:
        monkeypatch.setenv("GNSSCORR_L3T_THREADS", threads)
    r = _scene(gc)[5]
    ctx, d_if, n, ch = _scene_ctx(gc)
    ep = ctx.track(d_if.ptr, 0, n, ch, L3.SCENE_MS, closed_loop=True)
    assert (ep["status"][0] == 0).all()
    assert (ep["blksize"][0] == r["blksize"]).all()
    for f in L3.FIELDS:
        d = np.abs(ep[f][0] - r[f]) / (np.abs(r[f]) + 1.0)
        print(f"[l3t closed loop {threads}] {f}: max |gpu - ref| / (|ref| + 1) = {d.max():.3e}")
    for f in L3.FIELDS:
        ok = _close(ep[f][0], r[f], LOOP_TOL, LOOP_TOL)
        assert ok.all(), (f, np.flatnonzero(~ok)[:5], ep[f][0][~ok][:3], r[f][~ok][:3])
    assert ch["n_epochs"][0] == L3.SCENE_MS
    if threads is None:
        _cache["closed"] = ep.copy()


@pytest.mark.parametrize("threads", SHAPES)
def test_continuation_is_bit_exact(gpu, threads, monkeypatch):
    """20 epochs in one call = 8 + 12: every state field and record, bit for bit."""
    gc = gpu
    if threads:
        monkeypatch.setenv("GNSSCORR_L3T_THREADS", threads)
    ctx, d_if, n, ch = _scene_ctx(gc)
    ch2 = ch.copy()
    ep = ctx.track(d_if.ptr, 0, n, ch, 20, closed_loop=True)
    parts = [ctx.track(d_if.ptr, 0, n, ch2, k, closed_loop=True) for k in (8, 12)]
    assert np.concatenate(parts, axis=1).tobytes() == ep.tobytes()
    assert ch2.tobytes() == ch.tobytes()


def test_out_of_data_stops_the_channel(gpu):
    """A channel 1.5 epochs from the end of the record: status 1 on its second epoch, the
    record holding the blksize that did not fit; the channel beside it is untouched."""
    gc = gpu
    IF, prn, cp, f0, s, ref = _scene(gc)
    ctx, d_if, n, good = _scene_ctx(gc)
    late = ctx.init_chan(prn, n - 36000 + 1, f0)
    both = np.concatenate([late, good])
    alone = good.copy()
    e_both = ctx.track(d_if.ptr, 0, n, both, 4, closed_loop=True)
    e_alone = ctx.track(d_if.ptr, 0, n, alone, 4, closed_loop=True)
    assert e_both[1:].tobytes() == e_alone.tobytes() and both[1:].tobytes() == alone.tobytes()
    r = L3.track(IF, s, prn, n - 36000 + 1, f0, 4)
    assert r["status"] == 1 and len(r["blksize"]) == 1
    assert list(e_both["status"][0]) == [0, 1, 1, 1]
    assert e_both["blksize"][0][0] == r["blksize"][0]
    assert e_both["blksize"][0][1] == r["stop_blksize"]
    assert both["status"][0] == 1 and both["n_epochs"][0] == 1
    assert both["pos"][0] == n - 36000 + r["blksize"][0]


def test_host_argument_checks(gpu):
    gc = gpu
    ctx, d_if, n, ch = _scene_ctx(gc)
    for prn in (0, 32, 33):
        bad = ch.copy()
        bad["code_id"] = prn
        with pytest.raises(gc.GnssCorrError, match="outside 1..31"):
            ctx.track(d_if.ptr, 0, n, bad, 1)
    with pytest.raises(gc.GnssCorrError):
        gc.L3tCtx(fileType=1)


def test_replay_runs_the_trackers_loop(gpu):
    """replay on the restatement's sums: blksize exact, loop fields within the bound; on
    the sums the closed-loop run recorded it reproduces that run bit for bit."""
    gc = gpu
    IF, prn, cp, f0, s, ref = _scene(gc)
    ctx, d_if, n, ch = _scene_ctx(gc)
    sums = np.stack([ref[f] for f in L3.SUMS], axis=1)[None]
    rp = ctx.replay(ch.copy(), sums)
    want = L3.replay(sums[0], s, cp, f0)
    assert (rp["status"][0] == 0).all() and (rp["blksize"][0] == want["blksize"]).all()
    for f in L3.LOOP_FIELDS:
        d = np.abs(rp[f][0] - want[f]) / (np.abs(want[f]) + 1.0)
        print(f"[l3t replay] {f}: max |gpu - ref| / (|ref| + 1) = {d.max():.3e}")
    for f in L3.LOOP_FIELDS:
        assert _close(rp[f][0], want[f], LOOP_TOL, LOOP_TOL).all(), f
    ep = _cache.get("closed")
    if ep is None:
        ep = ctx.track(d_if.ptr, 0, n, ch.copy(), L3.SCENE_MS, closed_loop=True)
    rp = ctx.replay(ch.copy(), np.stack([ep[f] for f in L3.SUMS], axis=2))
    for f in L3.LOOP_FIELDS + ("blksize", "status"):
        assert rp[f].tobytes() == ep[f].tobytes(), f


def test_search_hands_over_to_the_tracker(gpu):
    """The full reference shape once: L = 240000, keep = 120000, period 24000, spc 2, 51
    bins, PRN 30.  The replica is built on the host as acquisition.sci:94-97 has it; bin
    and code phase equal the restatement's exactly, the metric within 1e-6; then 10
    closed-loop epochs from the result keep the pilot on its I arm."""
    gc = gpu
    IF, prn = L3.search_scene()
    s = L3.settings()
    fs, S_ = 24e6, 24000
    ref = L3.acquire(IF, s, prn)
    assert ref["metric"] > s["acqThreshold"]
    row = gc.sample_code(gc.l3_code(prn + 32), 10.23e6, fs, S_)
    replica = np.concatenate([b * row for b in (-1, -1, -1, 1, -1)]).astype(np.int8)
    assert np.array_equal(replica, L3.overlay_replica(s, prn))
    frq = gc.l3_bins(s["IF"], s["acqSearchBand"])
    acq = gc.AcqCtx(fs, 10 * S_, max_freqs=64, max_blocks=1, max_codes=1)
    acq.set_zero_padded(5 * S_)
    acq.set_peak_period(S_)
    acq.set_codes_padded(replica)
    res, _ = acq.search(IF[:2 * 10 * S_], 1, frq, [0], np.arange(51)[None, :], spc=2)
    assert res[0]["bin"] == ref["bin"] and res[0]["code_phase"] == ref["code_phase"]
    assert res[0]["carr_freq"] == ref["carr_freq"]
    assert abs(res[0]["metric"] - ref["metric"]) <= 1e-6 * ref["metric"]
    assert abs(res[0]["peak"] - ref["peak"]) <= 1e-6 * ref["peak"]
    n = len(IF) // 2
    ctx = gc.L3tCtx()
    ch = ctx.init_chans([prn], res["code_phase"], res["carr_freq"])
    ep = ctx.track(gc.DevBuf.from_array(IF).ptr, 0, n, ch, 10, closed_loop=True)
    assert (ep["status"] == 0).all()
    assert (np.abs(ep["I_P"][0]) > np.abs(ep["Q_P"][0])).all()
    r = L3.track(IF, s, prn, ref["code_phase"], ref["carr_freq"], 10)
    assert (ep["blksize"][0] == r["blksize"]).all()
