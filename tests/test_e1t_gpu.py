"""GPU parity: Galileo E1B float tracking (e1t.hip) vs the fp64 restatement of
GALILEO/E1/tracking.sci:95-455 (tests/e1t_scenarios.py).

Tolerances are those of tests/test_sgt_gpu.py:
  * blksize, pos, segment: exact; rem_code / rem_meandr / rem_carr after an open-loop
    epoch: bit-equal (same fp64 operation sequence, no contraction)
  * the ten sums: |gpu - ref| <= 1e-6 |ref| + 1e-6
  * closed loop: every per-epoch field within that bound of the restatement over the
    whole run, blksize exact (tests/test_e1t_cpu.py shows the scene is decidable).
Both E1 paths run the same tests: GNSSCORR_E1T_CHUNK=0 forces the per-sample one.
"""
import numpy as np
import pytest

import e1t_scenarios as E
from tracker_checks import close as _close, noise as _noise

pytestmark = pytest.mark.gpu
_cache = {}


def _tables():
    if "tab" not in _cache:
        codes, _ = E.fixture_codes()
        _cache["tab"] = (codes, [E.split_code(c) for c in codes], E.meandr_table())
    return _cache["tab"]


def _check_open_loop(gc, ctx, IF, n, s, ch):
    """One open-loop epoch of every channel against E.correlate."""
    codes, rows, mtab = _tables()
    ch0 = ch.copy()
    d_if = gc.DevBuf.from_array(IF)
    ep = ctx.track(d_if.ptr, 0, n, ch, 1, closed_loop=False)[:, 0]
    for i in range(len(ch)):
        c = ch0[i]
        st, blk, r = E.correlate(IF, s, rows[int(c["code_id"])], mtab, int(c["pos"]),
                                 int(c["segment"]), float(c["rem_code"]), float(c["rem_meandr"]),
                                 float(c["rem_carr"]), float(c["code_freq"]),
                                 float(c["meandr_freq"]), float(c["carr_freq"]))
        assert st == 0, (i, st)
        sums, pos, seg, rc, rm, rcar = r
        assert ep["status"][i] == 0 and ep["blksize"][i] == blk, (i, ep["blksize"][i], blk)
        assert ep["segment"][i] == c["segment"]
        assert ch["pos"][i] == pos and ch["segment"][i] == seg
        assert ch["rem_code"][i] == rc, (i, ch["rem_code"][i], rc)
        assert ch["rem_meandr"][i] == rm, (i, ch["rem_meandr"][i], rm)
        assert ch["rem_carr"][i] == rcar, (i, ch["rem_carr"][i], rcar)
        got = np.array([ep[f][i] for f in E.SUMS])
        assert _close(got, sums).all(), (i, got, sums)
    # frequencies are held in open loop
    for f in ("carr_freq", "code_freq", "meandr_freq"):
        assert (ch[f] == ch0[f]).all()
    return ep


def _random_chans(gc, rng, C, n, fs, carr=3e6):
    ch = np.zeros(C, gc.E1T_CHAN)
    ch["code_id"] = rng.integers(0, 3, C)
    ch["segment"] = rng.integers(0, 4, C)
    ch["segment"][:4] = [0, 3, 0, 3][:C]                   # the wrap-around pads of rows 1 and 4
    ch["pos"] = rng.integers(0, n - int(fs * 0.00101) - 64, C)
    ch["code_freq"] = 1.023e6 + rng.uniform(-40, 40, C)
    ch["meandr_freq"] = 2.046e6 + rng.uniform(-80, 80, C)
    step = ch["code_freq"] / fs
    ch["rem_code"] = rng.uniform(0, 1, C) * step
    if C >= 4:
        ch["rem_code"][:2] = 0.0
        ch["rem_code"][2:4] = np.nextafter(step[2:4], 0)
    ch["rem_meandr"] = rng.uniform(-0.5, 1.5, C)
    ch["rem_carr"] = rng.uniform(-6.2, 6.2, C)
    ch["carr_freq"] = rng.uniform(-carr, carr, C)
    return ch


@pytest.mark.parametrize("fs", [16e6, 16.368e6])
@pytest.mark.parametrize("threads", [None, "64", "128"])
@pytest.mark.parametrize("chunk", ["1", "0"])
@pytest.mark.parametrize("file_type", [2, 1])
def test_open_loop_epoch_matches_restatement(gpu, file_type, chunk, threads, fs, monkeypatch):
    """96 channels on a 200 000-sample noise record, then a single-channel call.  threads:
    launch shape (GNSSCORR_E1T_THREADS; None = the dispatcher's 256-thread workgroups, 64 =
    one wave per channel, the shape of 1024 channels and more)."""
    gc = gpu
    monkeypatch.setenv("GNSSCORR_E1T_CHUNK", chunk)
    if threads:
        monkeypatch.setenv("GNSSCORR_E1T_THREADS", threads)
    rng = np.random.default_rng(int(fs) % 97 + 3 * file_type)
    n = 200000
    IF = _noise(gc, n, fs, file_type)
    ctx = gc.E1tCtx(fileType=file_type, samplingFreq=fs)
    ctx.set_codes(_tables()[0])
    s = E.settings(fileType=file_type, samplingFreq=fs)
    _check_open_loop(gc, ctx, IF, n, s, _random_chans(gc, rng, 96, n, fs))
    _check_open_loop(gc, ctx, IF, n, s, _random_chans(gc, rng, 1, n, fs))


def test_many_channels_take_the_wave_shape(gpu):
    """1024 channels: the dispatcher's one-wave-per-channel launch, no override."""
    gc = gpu
    fs, n = 16e6, 200000
    IF = _noise(gc, n, fs, 2)
    ctx = gc.E1tCtx()
    ctx.set_codes(_tables()[0])
    ch = np.tile(_random_chans(gc, np.random.default_rng(8), 16, n, fs), 64)
    ch0 = ch.copy()
    d_if = gc.DevBuf.from_array(IF)
    ep = ctx.track(d_if.ptr, 0, n, ch, 1, closed_loop=False)[:, 0]
    _check_open_loop(gc, ctx, IF, n, E.settings(), ch0[:16])
    assert ep.reshape(64, 16)[1:].tobytes() == np.tile(ep[:16], 63).tobytes()


@pytest.mark.parametrize("chunk", ["1", "0"])
def test_open_loop_low_rate(gpu, chunk, monkeypatch):
    """4.096 Msps, 64 channels: four samples per chip, the chunked path does not apply."""
    gc = gpu
    monkeypatch.setenv("GNSSCORR_E1T_CHUNK", chunk)
    fs = 4.096e6
    n = int(fs * 0.012)
    IF = _noise(gc, n, fs, 2)
    ctx = gc.E1tCtx(samplingFreq=fs)
    ctx.set_codes(_tables()[0])
    ch = _random_chans(gc, np.random.default_rng(41), 64, n, fs, carr=1e6)
    _check_open_loop(gc, ctx, IF, n, E.settings(samplingFreq=fs), ch)


@pytest.mark.parametrize("threads", [None, "64"])
@pytest.mark.parametrize("chunk", ["1", "0"])
def test_chunk_edges(gpu, chunk, threads, monkeypatch):
    """blksize an exact multiple of chunk length x lanes (16 x 64 = 1024 and 16 x 256 = 4096
    both divide 16384), that +-1, and epochs shorter than one pass (360 and 15 samples),
    set through code_freq and rem_code; positions on and off the 16-byte grid of the
    record.  Also crossings on exact chips: code_freq = fs/16 with rem_code on the 1/16
    grid, where the chunked path's crossing estimates have no margin."""
    gc = gpu
    monkeypatch.setenv("GNSSCORR_E1T_CHUNK", chunk)
    if threads:
        monkeypatch.setenv("GNSSCORR_E1T_THREADS", threads)
    fs, n = 16e6, 200000
    IF = _noise(gc, n, fs, 2)
    ctx = gc.E1tCtx()
    ctx.set_codes(_tables()[0])
    s = E.settings()
    rng = np.random.default_rng(12)
    want, cf, rem = [], [], []
    for blk in (16384, 16383, 16385):
        for _ in range(4):
            r = float(rng.uniform(0, 0.05))
            cf.append((1023.0 - r) * fs / (blk - 0.5))      # ceil((1023 - r)/step) = blk
            rem.append(r)
            want.append(blk)
    for blk, r in ((360, 1000.0), (15, 1022.05), (360, 1000.3), (1, 1022.99)):
        cf.append((1023.0 - r) * fs / (blk - 0.5))
        rem.append(r)
        want.append(blk)
    for r in (0.0, 1 / 16, 3 / 16, 0.0):
        cf.append(fs / 16)
        rem.append(r)
        want.append(int(np.ceil((1023 - r) * 16)))
    C = len(want)
    ch = _random_chans(gc, rng, C, n, fs)
    ch["code_freq"], ch["rem_code"] = cf, rem
    ch["meandr_freq"] = 2.0 * ch["code_freq"]               # the subcarrier range stays in its table
    ch["meandr_freq"][-4:] = fs / 8                         # subcarrier steps on exact samples too
    ch["rem_meandr"][-4:] = [0.0, 0.125, 0.4, 1.0]
    ch["pos"][::2] &= ~7                                    # 16-byte aligned (2 bytes per sample)
    ch["pos"][1::2] |= 3
    ep = _check_open_loop(gc, ctx, IF, n, s, ch)
    assert list(ep["blksize"]) == want


def _scene(gc):
    if "scene" not in _cache:
        IF, codes, chans = E.closed_loop_scene()
        s = E.settings()
        ref = [E.track(IF, s, codes[row], cp, f0, E.SCENE_MS) for row, cp, f0, _ in chans]
        _cache["scene"] = (IF, codes, chans, s, ref)
    return _cache["scene"]


def _scene_ctx(gc):
    IF, codes, chans, s, ref = _scene(gc)
    ctx = gc.E1tCtx()
    ctx.set_codes(codes)
    ch = ctx.init_chans([c[0] for c in chans], [c[1] for c in chans], [c[2] for c in chans])
    return ctx, gc.DevBuf.from_array(IF), len(IF) // 2, ch


@pytest.mark.parametrize("threads", [None, "64"])
@pytest.mark.parametrize("chunk", ["1", "0"])
def test_closed_loop_three_prns_40_ms(gpu, chunk, threads, monkeypatch):
    """PRN 11, 12, 19 at different Dopplers and code phases on one 40 ms record: ten
    segment wraps, all three loops closed on the GPU."""
    gc = gpu
    monkeypatch.setenv("GNSSCORR_E1T_CHUNK", chunk)
    if threads:
        monkeypatch.setenv("GNSSCORR_E1T_THREADS", threads)
    ref = _scene(gc)[4]
    ctx, d_if, n, ch = _scene_ctx(gc)
    ep = ctx.track(d_if.ptr, 0, n, ch, E.SCENE_MS, closed_loop=True)
    for i, r in enumerate(ref):
        assert (ep["status"][i] == 0).all()
        assert (ep["blksize"][i] == r["blksize"]).all()
        assert (ep["segment"][i] == r["segment"]).all()
        for f in E.FIELDS:
            ok = _close(ep[f][i], r[f])
            assert ok.all(), (i, f, np.flatnonzero(~ok)[:5], ep[f][i][~ok][:3], r[f][~ok][:3])
    assert (ch["n_epochs"] == E.SCENE_MS).all() and (ch["segment"] == E.SCENE_MS % 4).all()
    if chunk == "1" and threads is None:
        _cache["closed"] = ep.copy()


def test_open_loop_with_host_loop_equals_closed_loop(gpu):
    """closed_loop=0, the loop filters on the host between six one-epoch calls."""
    gc = gpu
    IF, codes, chans, s, ref = _scene(gc)
    ctx, d_if, n, ch = _scene_ctx(gc)
    loops = [E.Loop(s, cp - 1, f0) for _, cp, f0, _ in chans]
    for e in range(6):
        ep = ctx.track(d_if.ptr, 0, n, ch, 1, closed_loop=False)[:, 0]
        for i, lp in enumerate(loops):
            assert ep["blksize"][i] == ref[i]["blksize"][e]
            lp.pos, lp.rem_code = int(ch["pos"][i]), float(ch["rem_code"][i])
            vals = dict(zip(E.FIELDS, lp.update([ep[f][i] for f in E.SUMS])))
            for f in E.FIELDS:
                assert _close(vals[f], ref[i][f][e]), (e, i, f)
            ch["carr_freq"][i], ch["code_freq"][i] = lp.carr_freq, lp.code_freq
            ch["meandr_freq"][i] = lp.meandr_freq


@pytest.mark.parametrize("chunk", ["1", "0"])
def test_continuation_is_bit_exact(gpu, chunk, monkeypatch):
    """20 epochs in one call = 4 calls of 5: every state field and record, bit for bit."""
    gc = gpu
    monkeypatch.setenv("GNSSCORR_E1T_CHUNK", chunk)
    ctx, d_if, n, ch = _scene_ctx(gc)
    ch4 = ch.copy()
    ep = ctx.track(d_if.ptr, 0, n, ch, 20, closed_loop=True)
    parts = [ctx.track(d_if.ptr, 0, n, ch4, 5, closed_loop=True) for _ in range(4)]
    assert np.concatenate(parts, axis=1).tobytes() == ep.tobytes()
    assert ch4.tobytes() == ch.tobytes()


def test_stops_leave_other_channels_alone(gpu):
    """A channel 1.5 epochs from the end of the record stops with status 1 on its second
    epoch (record: the blksize that did not fit); one with rem_meandr = 5.0 stops with
    status 2 on its first.  The other channels of the launch are bit-equal to a launch
    without them."""
    gc = gpu
    IF, codes, chans, s, ref = _scene(gc)
    ctx, d_if, n, good = _scene_ctx(gc)
    late = ctx.init_chan(0, n - 24000 + 1, 2.42e6)
    bad = ctx.init_chan(1, chans[1][1], chans[1][2])
    bad["rem_meandr"] = 5.0
    mixed = np.concatenate([good[:1], late, good[1:2], bad, good[2:]])
    alone = good.copy()
    e_mixed = ctx.track(d_if.ptr, 0, n, mixed, 4, closed_loop=True)
    e_alone = ctx.track(d_if.ptr, 0, n, alone, 4, closed_loop=True)
    assert e_mixed[[0, 2, 4]].tobytes() == e_alone.tobytes()
    assert mixed[[0, 2, 4]].tobytes() == alone.tobytes()
    r = E.track(IF, s, codes[0], n - 24000 + 1, 2.42e6, 4)
    assert r["status"] == 1 and len(r["blksize"]) == 1
    assert list(e_mixed["status"][1]) == [0, 1, 1, 1]
    assert e_mixed["blksize"][1][0] == r["blksize"][0]
    assert e_mixed["blksize"][1][1] == r["stop_blksize"]
    assert mixed["status"][1] == 1 and mixed["n_epochs"][1] == 1
    assert mixed["pos"][1] == n - 24000 + r["blksize"][0]
    assert list(e_mixed["status"][3]) == [2, 2, 2, 2]
    assert e_mixed["blksize"][3][0] == ref[1]["blksize"][0]
    assert mixed["status"][3] == 2 and mixed["n_epochs"][3] == 0
    assert mixed["pos"][3] == bad["pos"][0] and mixed["rem_meandr"][3] == 5.0


def test_host_argument_checks(gpu):
    """Tracking before set_codes, a code_id outside the table, chips not +-1: EINVAL on the
    host, with a context this time."""
    gc = gpu
    IF, codes, chans, s, ref = _scene(gc)
    ctx = gc.E1tCtx()
    d_if = gc.DevBuf.from_array(IF[:80000])
    ch = ctx.init_chan(0, 1, 2.42e6)
    with pytest.raises(gc.GnssCorrError, match="no codes"):
        ctx.track(d_if.ptr, 0, 40000, ch, 1)
    bad = codes.copy()
    bad[2, 4091] = 3
    with pytest.raises(gc.GnssCorrError, match="chips must be"):
        ctx.set_codes(bad)
    with pytest.raises(gc.GnssCorrError, match="no codes"):
        ctx.track(d_if.ptr, 0, 40000, ch, 1)
    ctx.set_codes(codes[:2])
    ch["code_id"] = 2
    with pytest.raises(gc.GnssCorrError, match="code_id 2 outside"):
        ctx.track(d_if.ptr, 0, 40000, ch, 1)
    ch["code_id"] = 1
    assert ctx.track(d_if.ptr, 0, 40000, ch, 1)["status"][0, 0] == 0


def test_replay_runs_the_trackers_loop(gpu):
    """replay on the sums the closed-loop run recorded reproduces that run's loop fields bit
    for bit (the same device function), and matches the restatement's replay to 1e-6."""
    gc = gpu
    IF, codes, chans, s, ref = _scene(gc)
    ctx, d_if, n, ch = _scene_ctx(gc)
    ch_r = ch.copy()
    ep = _cache.get("closed")
    if ep is None:
        ep = ctx.track(d_if.ptr, 0, n, ch, E.SCENE_MS, closed_loop=True)
    sums = np.stack([ep[f] for f in E.SUMS], axis=2)
    rp = ctx.replay(ch_r, sums)
    for f in E.LOOP_FIELDS + ("blksize", "status", "segment"):
        assert rp[f].tobytes() == ep[f].tobytes(), f
    for i, (row, cp, f0, _) in enumerate(chans):
        r = E.replay(sums[i], s, cp, f0)
        assert (rp["blksize"][i] == r["blksize"]).all()
        for f in E.LOOP_FIELDS:
            assert _close(rp[f][i], r[f]).all(), (i, f)
