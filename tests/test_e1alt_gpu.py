"""GPU parity: the Galileo E1 tracking alternatives (e1t.hip with epoch_ms / ambiguous) vs
the fp64 restatements of GALILEO/E1/BOC_tracking_alternatives/ (tests/e1alt_scenarios.py).

Tolerances are those of tests/test_sgt_gpu.py and tests/test_e1t_gpu.py:
  * blksize, pos, segment, status: exact; rem_code / rem_meandr / rem_carr after an
    open-loop epoch: bit-equal
  * sums and closed-loop fields: |gpu - ref| <= 1e-6 |ref| + 1e-6
    (tests/test_e1alt_cpu.py shows each mode's scene is decidable).
Every test runs with GNSSCORR_E1T_CHUNK = 1 and 0.  Launch shapes: each docstring says which
(256 = the dispatcher's 256-thread workgroups, 64 = one wave per channel).
"""
import numpy as np
import pytest

import e1alt_scenarios as A
import e1t_scenarios as E
from tracker_checks import close as _close, noise as _noise

pytestmark = pytest.mark.gpu
MODES = ("4ms", "amb1", "amb4")
_cache = {}
EPOCH = {"4ms": 4092.0, "amb1": 2046.0, "amb4": 8184.0}       # entries per epoch
RATE = {"4ms": 1.023e6, "amb1": 2.046e6, "amb4": 2.046e6}


def _tables(mode):
    if mode not in _cache:
        codes, _ = E.fixture_codes()
        _cache[mode] = (codes, [A.tables(mode, c) for c in codes])
    return _cache[mode]


def _ctx(gc, mode, **kw):
    ctx = gc.E1tCtx(**kw, **A.MODES[mode])
    ctx.set_codes(_tables(mode)[0])
    return ctx


def _env(monkeypatch, chunk, threads=None):
    monkeypatch.setenv("GNSSCORR_E1T_CHUNK", chunk)
    if threads:
        monkeypatch.setenv("GNSSCORR_E1T_THREADS", threads)


def _loop_of(mode, s, c):
    lp = A.Loop(mode, s, int(c["pos"]), float(c["carr_freq"]))
    lp.segment, lp.rem_code, lp.rem_meandr = int(c["segment"]), float(c["rem_code"]), \
        float(c["rem_meandr"])
    lp.rem_carr, lp.code_freq, lp.meandr_freq = float(c["rem_carr"]), float(c["code_freq"]), \
        float(c["meandr_freq"])
    return lp


def _check_open_loop(gc, mode, ctx, IF, n, s, ch):
    """One open-loop epoch of every channel against the restatement's correlator."""
    tabs = _tables(mode)[1]
    ch0 = ch.copy()
    d_if = gc.DevBuf.from_array(IF)
    ep = ctx.track(d_if.ptr, 0, n, ch, 1, closed_loop=False)[:, 0]
    for i in range(len(ch)):
        c = ch0[i]
        lp = _loop_of(mode, s, c)
        st, blk, sums = A.correlate(mode, IF, s, tabs[int(c["code_id"])], lp)
        assert st == 0, (i, st)
        assert ep["status"][i] == 0 and ep["blksize"][i] == blk, (i, ep["blksize"][i], blk)
        assert ep["segment"][i] == c["segment"]
        assert ch["pos"][i] == lp.pos and ch["segment"][i] == lp.segment
        assert ch["rem_code"][i] == lp.rem_code, (i, ch["rem_code"][i], lp.rem_code)
        assert ch["rem_meandr"][i] == lp.rem_meandr, (i, ch["rem_meandr"][i], lp.rem_meandr)
        assert ch["rem_carr"][i] == lp.rem_carr, (i, ch["rem_carr"][i], lp.rem_carr)
        got = np.array([ep[f][i] for f in E.SUMS])
        assert _close(got, sums).all(), (i, got, sums)
        if A.is_amb(mode):
            for f in ("I_E_P", "I_L_P", "Q_E_P", "Q_L_P", "meandrFreq", "sllDiscr", "sllDiscrFilt"):
                assert ep[f][i] == 0.0, f
    for f in ("carr_freq", "code_freq", "meandr_freq"):     # held in open loop
        assert (ch[f] == ch0[f]).all()
    return ep


def _random_chans(gc, mode, rng, C, n, fs, carr=3e6):
    """As _random_chans of tests/test_e1t_gpu.py, with the mode's rate and epoch."""
    ch = np.zeros(C, gc.E1T_CHAN)
    ch["code_id"] = rng.integers(0, 3, C)
    if mode == "amb1":
        ch["segment"] = rng.integers(0, 4, C)
        ch["segment"][:4] = [0, 3, 0, 3][:C]               # the wrap-around pads of rows 1 and 4
    room = int(np.ceil(EPOCH[mode] / (RATE[mode] - 100) * fs)) + 64
    if mode != "amb1" and n >= 200000:
        room = 66000
    ch["pos"] = rng.integers(0, n - room, C)
    ch["code_freq"] = RATE[mode] + rng.uniform(-40, 40, C) * (RATE[mode] / 1.023e6)
    step = ch["code_freq"] / fs
    ch["rem_code"] = rng.uniform(0, 1, C) * step
    if C >= 4:
        ch["rem_code"][:2] = 0.0
        ch["rem_code"][2:4] = np.nextafter(step[2:4], 0)
    if mode == "4ms":
        ch["meandr_freq"] = 2.046e6 + rng.uniform(-20, 20, C)
        ch["rem_meandr"] = rng.uniform(-0.5, 0.5, C)       # one back pad: the range ends at 8185
    ch["rem_carr"] = rng.uniform(-6.2, 6.2, C)
    ch["carr_freq"] = rng.uniform(-carr, carr, C)
    return ch


@pytest.mark.parametrize("fs", [16e6, 16.368e6])
@pytest.mark.parametrize("threads", [None, "64"])
@pytest.mark.parametrize("chunk", ["1", "0"])
@pytest.mark.parametrize("file_type", [2, 1])
@pytest.mark.parametrize("mode", MODES)
def test_open_loop_epoch_matches_restatement(gpu, mode, file_type, chunk, threads, fs, monkeypatch):
    """24 channels on a 200 000-sample noise record (positions at most n - 66 000 in the 4 ms
    modes), then a single-channel call.  Shapes: 256 (threads None) and 64."""
    gc = gpu
    _env(monkeypatch, chunk, threads)
    rng = np.random.default_rng(int(fs) % 97 + 3 * file_type + MODES.index(mode))
    n = 200000
    IF = _noise(gc, n, fs, file_type)
    ctx = _ctx(gc, mode, fileType=file_type, samplingFreq=fs)
    s = E.settings(fileType=file_type, samplingFreq=fs)
    ch = _random_chans(gc, mode, rng, 24, n, fs)
    if mode != "amb1":
        assert ch["pos"].max() <= n - 66000
    _check_open_loop(gc, mode, ctx, IF, n, s, ch)
    _check_open_loop(gc, mode, ctx, IF, n, s, _random_chans(gc, mode, rng, 1, n, fs))


@pytest.mark.parametrize("chunk", ["1", "0"])
@pytest.mark.parametrize("mode", MODES)
def test_open_loop_low_rate(gpu, mode, chunk, monkeypatch):
    """4.096 Msps, 16 channels: the chunked predicate fails (15 steps pass one entry, or two
    of the composite sequence) and the per-sample path runs; a 4 ms epoch is 16 384 samples.
    Shape: 256."""
    gc = gpu
    _env(monkeypatch, chunk)
    fs = 4.096e6
    n = int(fs * 0.012)
    IF = _noise(gc, n, fs, 2)
    ctx = _ctx(gc, mode, samplingFreq=fs)
    ch = _random_chans(gc, mode, np.random.default_rng(41), 16, n, fs, carr=1e6)
    ep = _check_open_loop(gc, mode, ctx, IF, n, E.settings(samplingFreq=fs), ch)
    assert (np.abs(ep["blksize"] - 4096 * A.EPOCH_MS[mode]) <= 2).all()


@pytest.mark.parametrize("threads", [None, "64"])
@pytest.mark.parametrize("chunk", ["1", "0"])
@pytest.mark.parametrize("mode", MODES)
def test_chunk_edges(gpu, mode, chunk, threads, monkeypatch):
    """blksize an exact multiple of chunk length x lanes (65 536 in the 4 ms modes, 16 384 in
    the ambiguous 1 ms one: both 16 x 64 and 16 x 256 divide them) and that +-1, epochs of
    360, 15 and 1 samples through rem_code near the row's end, positions on and off the
    16-byte grid, and crossings on exact samples: code_freq = fs/16 with rem_code on the
    1/16 grid (ambiguous: fs/8 and the 1/8 grid; five-arm: the subcarrier at fs/8 as well).
    Shapes: 256 and 64."""
    gc = gpu
    _env(monkeypatch, chunk, threads)
    fs, n = 16e6, 200000
    IF = _noise(gc, n, fs, 2)
    ctx = _ctx(gc, mode)
    s = E.settings()
    rng = np.random.default_rng(12)
    L = EPOCH[mode]
    big = 16384 if mode == "amb1" else 65536
    want, cf, rem = [], [], []
    for blk in (big, big - 1, big + 1):
        for _ in range(3):
            r = float(rng.uniform(0, 0.05))
            cf.append((L - r) * fs / (blk - 0.5))           # ceil((L - r)/step) = blk
            rem.append(r)
            want.append(blk)
    m = RATE[mode] / 1.023e6                                # entries per chip
    for blk, r in ((360, L - 23.0 * m), (15, L - 0.95 * m), (360, L - 22.7 * m), (1, L - 0.01 * m)):
        cf.append((L - r) * fs / (blk - 0.5))
        rem.append(r)
        want.append(blk)
    grid = 8 if A.is_amb(mode) else 16
    n_exact = 4
    for r in (0.0, 1 / grid, 3 / grid, 0.0):
        cf.append(fs / grid)
        rem.append(r)
        want.append(int(np.ceil((L - r) * grid)))
    C = len(want)
    ch = _random_chans(gc, mode, rng, C, n, fs)
    ch["code_freq"], ch["rem_code"] = cf, rem
    if mode == "4ms":
        ch["meandr_freq"] = 2.0 * ch["code_freq"]           # the subcarrier range stays in its table
        ch["rem_meandr"] = rng.uniform(-0.4, 0.4, C)
        ch["rem_meandr"][-n_exact:] = [0.0, 0.125, 0.4, 0.5]   # steps on exact samples too
        short = np.asarray(want) < 1000
        ch["rem_meandr"][short] = rng.uniform(-0.4, 1.5, int(short.sum()))
    ch["pos"] = rng.integers(0, n - max(want) - 64, C)
    ch["pos"][::2] &= ~7                                    # 16-byte aligned (2 bytes per sample)
    ch["pos"][1::2] |= 3
    ep = _check_open_loop(gc, mode, ctx, IF, n, s, ch)
    assert list(ep["blksize"]) == want


def _scene(gc, mode):
    key = ("scene", mode)
    if key not in _cache:
        IF, codes, chans = A.closed_loop_scene(mode)
        s = E.settings()
        ref = [A.track(mode, IF, s, codes[row], cp, f0, A.SCENE_EPOCHS[mode])
               for row, cp, f0, _ in chans]
        _cache[key] = (IF, codes, chans, s, ref)
    return _cache[key]


def _scene_ctx(gc, mode):
    IF, codes, chans, s, ref = _scene(gc, mode)
    ctx = gc.E1tCtx(**A.MODES[mode])
    ctx.set_codes(codes)
    ch = ctx.init_chans([c[0] for c in chans], [c[1] for c in chans], [c[2] for c in chans])
    return ctx, gc.DevBuf.from_array(IF), len(IF) // 2, ch


@pytest.mark.parametrize("threads", [None, "64"])
@pytest.mark.parametrize("chunk", ["1", "0"])
@pytest.mark.parametrize("mode", MODES)
def test_closed_loop_scene(gpu, mode, chunk, threads, monkeypatch):
    """PRN 11, 12, 19 on the 40 ms record, every loop of the mode closed on the GPU: 10
    epochs at 4 ms, 40 at 1 ms.  Shapes: 256 and 64."""
    gc = gpu
    _env(monkeypatch, chunk, threads)
    ref = _scene(gc, mode)[4]
    ctx, d_if, n, ch = _scene_ctx(gc, mode)
    N = A.SCENE_EPOCHS[mode]
    ep = ctx.track(d_if.ptr, 0, n, ch, N, closed_loop=True)
    for i, r in enumerate(ref):
        assert (ep["status"][i] == 0).all()
        assert (ep["blksize"][i] == r["blksize"]).all()
        assert (ep["segment"][i] == r["segment"]).all()
        for f in E.FIELDS:
            ok = _close(ep[f][i], r[f])
            assert ok.all(), (i, f, np.flatnonzero(~ok)[:5], ep[f][i][~ok][:3], r[f][~ok][:3])
    assert (ch["n_epochs"] == N).all()
    assert (ch["segment"] == (N % 4 if mode == "amb1" else 0)).all()
    if A.is_amb(mode):
        for f in ("rem_meandr", "meandr_freq", "old_meandr_nco", "old_meandr_error"):
            assert (ch[f] == 0.0).all(), f


@pytest.mark.parametrize("chunk", ["1", "0"])
@pytest.mark.parametrize("mode", MODES)
def test_continuation_is_bit_exact(gpu, mode, chunk, monkeypatch):
    """N epochs in one call = N/2 + N/2: every state field and record, bit for bit.
    Shape: 256."""
    gc = gpu
    _env(monkeypatch, chunk)
    ctx, d_if, n, ch = _scene_ctx(gc, mode)
    N = 8 if mode == "amb1" else 4
    ch2 = ch.copy()
    ep = ctx.track(d_if.ptr, 0, n, ch, N, closed_loop=True)
    parts = [ctx.track(d_if.ptr, 0, n, ch2, N // 2, closed_loop=True) for _ in range(2)]
    assert np.concatenate(parts, axis=1).tobytes() == ep.tobytes()
    assert ch2.tobytes() == ch.tobytes()


@pytest.mark.parametrize("chunk", ["1", "0"])
@pytest.mark.parametrize("mode", MODES)
def test_stops_leave_other_channels_alone(gpu, mode, chunk, monkeypatch):
    """A channel 1.5 epochs from the record's end stops with status 1 on its second epoch,
    carrying the blksize that did not fit; in the five-arm mode one with rem_meandr beyond
    the 8186-entry range stops with status 2 on its first (the ambiguous modes know status 1
    only: the same rem_meandr is carried through untouched).  The other channels of the
    launch are bit-equal to a launch without them.  Shape: 256."""
    gc = gpu
    _env(monkeypatch, chunk)
    IF, codes, chans, s, ref = _scene(gc, mode)
    ctx, d_if, n, good = _scene_ctx(gc, mode)
    back = 24000 * A.EPOCH_MS[mode]
    late = ctx.init_chan(0, n - back + 1, 2.42e6)
    bad = ctx.init_chan(1, chans[1][1], chans[1][2])
    bad["rem_meandr"] = 5.0
    mixed = np.concatenate([good[:1], late, good[1:2], bad, good[2:]])
    alone = good.copy()
    e_mixed = ctx.track(d_if.ptr, 0, n, mixed, 3, closed_loop=True)
    e_alone = ctx.track(d_if.ptr, 0, n, alone, 3, closed_loop=True)
    assert e_mixed[[0, 2, 4]].tobytes() == e_alone.tobytes()
    assert mixed[[0, 2, 4]].tobytes() == alone.tobytes()
    r = A.track(mode, IF, s, codes[0], n - back + 1, 2.42e6, 3)
    assert r["status"] == 1 and len(r["blksize"]) == 1
    assert list(e_mixed["status"][1]) == [0, 1, 1]
    assert e_mixed["blksize"][1][0] == r["blksize"][0]
    assert e_mixed["blksize"][1][1] == r["stop_blksize"]
    assert mixed["status"][1] == 1 and mixed["n_epochs"][1] == 1
    assert mixed["pos"][1] == n - back + r["blksize"][0]
    if mode == "4ms":
        assert list(e_mixed["status"][3]) == [2, 2, 2]
        assert e_mixed["blksize"][3][0] == ref[1]["blksize"][0]
        assert mixed["status"][3] == 2 and mixed["n_epochs"][3] == 0
        assert mixed["pos"][3] == bad["pos"][0]
    else:
        assert list(e_mixed["status"][3]) == [0, 0, 0]
        assert e_mixed[3].tobytes() == e_alone[1].tobytes()
    assert mixed["rem_meandr"][3] == 5.0


@pytest.mark.parametrize("chunk", ["1", "0"])
@pytest.mark.parametrize("mode", MODES)
def test_replay_runs_the_trackers_loop(gpu, mode, chunk, monkeypatch):
    """replay on the sums the closed-loop run recorded reproduces that run's loop fields bit
    for bit and matches the restatement's replay to 1e-6; the ambiguous modes ignore what
    stands in the four slots they do not use.  One thread per channel."""
    gc = gpu
    _env(monkeypatch, chunk)
    IF, codes, chans, s, ref = _scene(gc, mode)
    ctx, d_if, n, ch = _scene_ctx(gc, mode)
    ch_r = ch.copy()
    N = A.SCENE_EPOCHS[mode]
    ep = ctx.track(d_if.ptr, 0, n, ch, N, closed_loop=True)
    sums = np.stack([ep[f] for f in E.SUMS], axis=2)
    given = sums.copy()
    if A.is_amb(mode):
        given[:, :, [0, 4, 5, 9]] = 123.5
    rp = ctx.replay(ch_r, given)
    for f in E.FIELDS + ("blksize", "status", "segment"):
        assert rp[f].tobytes() == ep[f].tobytes(), f
    for i, (row, cp, f0, _) in enumerate(chans):
        r = A.replay(mode, sums[i], s, cp, f0)
        assert (rp["blksize"][i] == r["blksize"]).all()
        assert (rp["segment"][i] == r["segment"]).all()
        for f in E.LOOP_FIELDS:
            assert _close(rp[f][i], r[f]).all(), (i, f)


@pytest.mark.parametrize("chunk", ["1", "0"])
def test_many_channels_take_the_wave_shape(gpu, chunk, monkeypatch):
    """1024 channels (16 distinct, tiled) in the 4 ms five-arm mode: the dispatcher's
    one-wave-per-channel launch with no override; the tiles are byte-equal.  The test cannot
    see the launch shape itself.  It infers it: the first tile must be byte-equal to a launch
    of the same 16 channels forced to 64 threads, and a 256-thread launch adds the samples in
    another order (four waves' partials), which moves the last bits of the sums."""
    gc = gpu
    _env(monkeypatch, chunk)
    mode = "4ms"
    fs, n = 16e6, 200000
    IF = _noise(gc, n, fs, 2)
    ctx = _ctx(gc, mode)
    ch16 = _random_chans(gc, mode, np.random.default_rng(8), 16, n, fs)
    ch = np.tile(ch16, 64)
    d_if = gc.DevBuf.from_array(IF)
    ep = ctx.track(d_if.ptr, 0, n, ch, 1, closed_loop=False)[:, 0]
    assert ep.reshape(64, 16)[1:].tobytes() == np.tile(ep[:16], 63).tobytes()
    assert ch.reshape(64, 16)[1:].tobytes() == np.tile(ch[:16], 63).tobytes()
    monkeypatch.setenv("GNSSCORR_E1T_THREADS", "64")
    ep16 = _check_open_loop(gc, mode, ctx, IF, n, E.settings(), ch16.copy())
    assert ep16.tobytes() == ep[:16].tobytes()
