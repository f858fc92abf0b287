"""GPU parity: osg_track_kernel<PK>, the real-sample (I-only) tracking kernel, against
the scalar oracle at every launch shape.

I-only streams are use_iq_processing = 0 of the reference Sim_GP2021_int
(osgnss_next_step/src/correlator/correlator.c:148-316).  Every TrackCtx(iq=False), every
OSG(use_iq=False) and the I-only branch of trackshard run on this kernel.  All
comparisons are bit-exact against OracleOSG(1, False, 16.368e6, 0.0) (oracle/osg_corr.c,
pinned to the compiled reference for I-only scenarios by test_oracle_osg.py), one
instance per channel: every dump of every call (all_dumps against sim_dumps()), n_dumps,
msbit_reg and the final channel state.

(a) every threads / cpw / block combination track_real_launch() can pick, 37 channels (a last
    workgroup with idle thread groups, 10..37 workgroups: a non-trivial XCD order) on 3
    streams at a stride the host call has to re-stride;
(b) code words of about one and of half a half-chip per sample: many dumps per call,
    against the ep_cap = nsamp / 2046 + 2 bound;
(c) slews and stored half-chip counts around the edges of chan_setup (j1 = 1, j1 = kNever,
    the staged-row limits of the IQ kernel) and epoch loads;
(d) gnsscorr_track_replay_dev's one-launch-per-step form, the only way an I-only context
    replays, against single calls and the oracle;
(e) a replay (or closed loop) whose later step would start misaligned is refused before
    anything moved: state, results and the TIC counter.
"""
import numpy as np
import pytest

import osg_scenarios as S
from test_packed_gpu import _layout
from test_track_gpu import _random_cmds

pytestmark = pytest.mark.gpu

FS = 16.368e6
KEYS = ("carrier_phase", "carrier_cycle", "code_phase", "half_chip", "acc")
FMT = pytest.mark.parametrize("packed", [False, True], ids=["int8", "packed2"])


def _oracle_real(oracle, streams, nsamp, cmds, half_chip0=None):
    """Each channel through its own emulated GP2021 (channel 0, I-only): every dump of
    every call [k][c] -> [n, 6], REG_read[7] after every call and the final state."""
    n_calls, C = cmds.shape
    dumps = [[None] * C for _ in range(n_calls)]
    msbit = np.zeros((n_calls, C), np.int32)
    state = []
    for c in range(C):
        o = oracle.OracleOSG(1, False, FS, 0.0)
        if half_chip0 is not None:
            o._st["half_chip"][0] = half_chip0
        rw = o.REG_write
        rw[7] = -1
        for k in range(n_calls):
            cm = cmds[k, c]
            rw[0] = cm["prn"]
            rw[3], rw[4] = int(cm["carrier_incr"]) >> 16, int(cm["carrier_incr"]) & 0xFFFF
            rw[5], rw[6] = int(cm["code_incr"]) >> 16, int(cm["code_incr"]) & 0xFFFF
            rw[0x84] = cm["slew"]
            if cm["epoch_load"] >= 0:
                rw[7] = cm["epoch_load"]
            s = streams[cm["stream"]]
            dumps[k][c] = o.sim_dumps(s[k * nsamp:(k + 1) * nsamp], nsamp)[:, 1:]
            msbit[k, c] = o.REG_read[7]
        state.append(o.chan_state())
    return dumps, msbit, state


def _check_call(res, d, want_k, msbit_k, max_dumps, tag):
    for c, w in enumerate(want_k):
        assert len(w) <= max_dumps, (tag, c, len(w), max_dumps)
        assert res["n_dumps"][c] == len(w), (tag, c, int(res["n_dumps"][c]), len(w))
        if d is not None:
            np.testing.assert_array_equal(d[c, :len(w)], w, err_msg=f"{tag} ch{c} all dumps")
        if len(w):
            np.testing.assert_array_equal(res["dump"][c], w[-1], err_msg=f"{tag} ch{c} last dump")
    np.testing.assert_array_equal(res["msbit_reg"], msbit_k, err_msg=f"{tag} msbit_reg")


def _check_state(st, want_state, tag=""):
    for c, w in enumerate(want_state):
        for key in KEYS:
            np.testing.assert_array_equal(st[key][c], w[key][0], err_msg=f"{tag} {key} ch{c}")


def _host_stride(total):
    """Samples per host stream: a multiple of 4 (whole packed bytes) that is neither a
    multiple of 16 nor of 32, so gnsscorr_track re-strides int8 and packed streams alike
    (its hipMemcpy2DAsync path)."""
    return (total + 15) // 16 * 16 + 4


def _run_host(gpu, ctx, buf, stride, n_streams, nsamp, cmds, packed):
    """The calls of cmds through gnsscorr_track with all dumps."""
    out = []
    for k in range(len(cmds)):
        chunk = buf[k * nsamp:]
        res, _, d = ctx.track(gpu.pack2(chunk) if packed else chunk, nsamp, cmds[k],
                              n_streams=n_streams, stream_stride=stride, all_dumps=True)
        out.append((res.copy(), d.copy()))
    return out


# ---------------------------------------------------------------- (a) launch shapes
# track_real_launch() (track_real.hip): threads per channel T = ceil(nsamp / 64) rounded up to 64,
# cpw = min(kMaxCpw = 4, 1024 / T), block = T * cpw, grid = ceil(C / cpw):
#   nsamp                 runs   T     cpw          block  grid (C = 37)
#   1, 63, 64, 65         1-2    64    4 (16 -> 4)  256    10
#   2043, 4096            32/64  64    4            256    10     last lane partial / all full
#   4097                  65     128   4 (8 -> 4)   512    10     1-sample tail run in wave 2
#   8380                  131    192   4 (5 -> 4)   768    10
#   16368                 256    256   4            1024   10     the 1-ms call
#   16385, 20480          257,320 320  3            960    13     cpw not a power of two
#   32768                 512    512   2            1024   19
#   32769                 513    576   1            576    37
#   65535, 65536          1024   1024  1            1024   37     kMaxNsamp and below it
SHAPES = {1: (64, 4), 63: (64, 4), 64: (64, 4), 65: (64, 4), 2043: (64, 4), 4096: (64, 4),
          4097: (128, 4), 8380: (192, 4), 16368: (256, 4), 16385: (320, 3), 20480: (320, 3),
          32768: (512, 2), 32769: (576, 1), 65535: (1024, 1), 65536: (1024, 1)}
C_A, STREAMS_A, CALLS_A = 37, 3, 2
_CASE_A = {}


def test_shape_table_follows_launch():
    """The table above is what track_real_launch() computes, and it holds every block size."""
    for nsamp, (T, cpw) in SHAPES.items():
        t = ((nsamp + 63) // 64 + 63) // 64 * 64
        assert (t, min(4, 1024 // t)) == (T, cpw), nsamp
    assert {T * cpw for T, cpw in SHAPES.values()} == {256, 512, 768, 1024, 960, 576}
    assert {-(-C_A // cpw) for _, cpw in SHAPES.values()} == {10, 13, 19, 37}


def _case_a(oracle, nsamp):
    """Streams, commands and the oracle's answers of one nsamp (shared by both formats)."""
    if nsamp not in _CASE_A:
        rng = np.random.default_rng(1000 + nsamp)
        streams = [S.synth_if(nsamp * CALLS_A, 40 + i, [(i + 2, 61 * i, 0, 3)], iq=False)
                   for i in range(STREAMS_A)]
        cmds = _random_cmds(rng, CALLS_A, C_A, STREAMS_A, slew=True)
        cmds["prn"][:, 5] = 0         # one idle channel
        cmds["prn"][:, 36] = 32       # the row over-read past the last PRN, in the last workgroup
        cmds["prn"][:, 0] = 7
        assert len(np.unique(cmds[0]["stream"])) == STREAMS_A
        _CASE_A[nsamp] = (streams, cmds) + _oracle_real(oracle, streams, nsamp, cmds)
    return _CASE_A[nsamp]


@FMT
@pytest.mark.parametrize("nsamp", sorted(SHAPES))
def test_launch_shapes_vs_oracle(gpu, oracle, nsamp, packed):
    streams, cmds, want, msbit, state = _case_a(oracle, nsamp)
    if nsamp >= 8380:     # the sums are checked, not only the NCO state
        assert sum(len(w) for k in range(CALLS_A) for w in want[k]) >= 1
    stride = _host_stride(nsamp * CALLS_A)
    assert stride % 4 == 0 and stride % 16 and stride % 32
    buf = _layout(streams, stride)
    ctx = gpu.TrackCtx(C_A, iq=False, max_nsamp=nsamp, packed=packed)
    assert ctx.max_dumps == nsamp // 2046 + 2
    got = _run_host(gpu, ctx, buf, stride, STREAMS_A, nsamp, cmds, packed)
    for k, (res, d) in enumerate(got):
        _check_call(res, d, want[k], msbit[k], ctx.max_dumps, f"nsamp {nsamp} call {k}")
    _check_state(ctx.get_state(), state, f"nsamp {nsamp}")


# ---------------------------------------------------------------- (b) many dumps per call
# kinc2 = code_incr << 1 (mod 2^32) is the code NCO step: (1 << 31) - 1 gives a rollover
# (half-chip) at nearly every sample, 1 << 30 one every second sample.  The first word
# takes its random offset downwards only: above 1 << 31 the shift wraps to a tiny step.
CODE_WORDS = {"1_per_sample": ((1 << 31) - 1, 1), "1_per_2_samples": (1 << 30, 2)}
_CASE_B = {}


def _case_b(oracle, word, nsamp):
    if (word, nsamp) not in _CASE_B:
        C, n_calls = 9, 2
        rng = np.random.default_rng(nsamp + len(word))
        streams = [S.synth_if(nsamp * n_calls, 70 + i, [(3 * i + 1, 29 * i, 0, 3)], iq=False)
                   for i in range(C)]
        cmds = _random_cmds(rng, n_calls, C, C)
        base, per = CODE_WORDS[word]
        for k in range(n_calls):
            cmds[k]["prn"] = 3 * np.arange(C) + 1
            cmds[k]["stream"] = np.arange(C)
            off = rng.integers(0, 20000, size=C)
            cmds[k]["code_incr"] = base - off if per == 1 else base + off - 10000
        _CASE_B[word, nsamp] = (streams, cmds) + _oracle_real(oracle, streams, nsamp, cmds, 2045)
    return _CASE_B[word, nsamp]


@FMT
@pytest.mark.parametrize("nsamp", [4096, 16368, 65536])
@pytest.mark.parametrize("word", sorted(CODE_WORDS))
def test_many_dumps_per_call_vs_oracle(gpu, oracle, word, nsamp, packed):
    streams, cmds, want, msbit, state = _case_b(oracle, word, nsamp)
    n_calls, C = cmds.shape
    # the oracle itself: the first carry dumps (half_chip 2045), then one dump per 2046
    # rollovers; `per` samples per rollover
    per = CODE_WORDS[word][1]
    for k in range(n_calls):
        for c in range(C):
            assert len(want[k][c]) >= max(1, (nsamp // per) // 2046 - 1), (k, c, len(want[k][c]))
    stride = _host_stride(nsamp * n_calls)
    buf = _layout(streams, stride)
    ctx = gpu.TrackCtx(C, iq=False, max_nsamp=nsamp, packed=packed)
    assert ctx.max_dumps == nsamp // 2046 + 2
    st = ctx.get_state()
    st["half_chip"] = 2045
    ctx.set_state(st)
    got = _run_host(gpu, ctx, buf, stride, C, nsamp, cmds, packed)
    for k, (res, d) in enumerate(got):
        assert (res["n_dumps"] <= nsamp // 2046 + 2).all()
        _check_call(res, d, want[k], msbit[k], ctx.max_dumps, f"{word} nsamp {nsamp} call {k}")
    _check_state(ctx.get_state(), state, word)


# ---------------------------------------------------------------- (c) chan_setup edges
SLEWS_C = [0, 1, 1025, 1026, 3000, 65535]
# channels whose stored half-chip count meets a smaller D = 2046 + slew in a later call
# (h1 >= D: the first rollover dumps, j1 = 1): a large slew, then a small one
DROPS_C = [(65535, 65535, 0), (3000, 3000, 0), (3000, 3000, 1025), (65535, 0, 0), (3000, 0, 3000),
           (65535, 1026, 1)]
_CASE_C = {}


def _case_c(oracle):
    if not _CASE_C:
        nsamp, n_calls, n_streams = 16368, 3, 2
        n_cyc = 2 * len(SLEWS_C)
        C = n_cyc + len(DROPS_C) + 2
        rng = np.random.default_rng(77)
        streams = [S.synth_if(nsamp * n_calls, 90 + i, [(i + 9, 83 * i, 0, 3)], iq=False)
                   for i in range(n_streams)]
        cmds = _random_cmds(rng, n_calls, C, n_streams)
        cmds["prn"] = rng.integers(1, 33, size=C)
        cmds["slew"][:, :n_cyc] = np.resize(np.array(SLEWS_C, np.uint32), n_cyc)
        cmds["slew"][:, n_cyc:n_cyc + len(DROPS_C)] = np.array(DROPS_C, np.uint32).T
        idle, active = C - 1, C - 2
        cmds["prn"][:, idle] = 0
        # epoch loads in the second call: bit 49 / ms 19 wraps both counters at the next dump
        cmds["epoch_load"][1, active] = (49 << 8) | 19
        cmds["epoch_load"][1, idle] = 0x2A07
        cmds["epoch_load"][1, 0] = 0x0113
        _CASE_C["v"] = (streams, cmds) + _oracle_real(oracle, streams, nsamp, cmds)
    return _CASE_C["v"]


@FMT
def test_slews_and_half_chip_edges_vs_oracle(gpu, oracle, packed):
    streams, cmds, want, msbit, state = _case_c(oracle)
    nsamp, n_streams = 16368, len(streams)
    n_calls, C = cmds.shape
    n_cyc = 2 * len(SLEWS_C)
    # the oracle itself shows the edges: D = 2046 + 65535 never dumps (j1 = kNever) ...
    for c in np.flatnonzero(cmds[0]["slew"][:n_cyc] == 65535):
        assert all(len(want[k][c]) == 0 for k in range(n_calls)), c
    # ... the other slews do dump, and a stored half-chip count at or above the new D dumps
    # at the first rollover of that call (a dump no nominal 2046-rollover call holds at
    # slew >= 3000 otherwise)
    assert all(sum(len(want[k][c]) for k in range(n_calls)) >= 1
               for c in np.flatnonzero(cmds[0]["slew"][:n_cyc] <= 1026))
    for j, drop in enumerate(DROPS_C):
        k = 1 if drop[1] < drop[0] else 2
        assert len(want[k][n_cyc + j]) >= 1, (drop, [len(want[i][n_cyc + j]) for i in range(3)])
    assert msbit[1, C - 1] == 0x2A07 and msbit[0, C - 1] == 0     # the idle channel's load
    stride = _host_stride(nsamp * n_calls)
    buf = _layout(streams, stride)
    ctx = gpu.TrackCtx(C, iq=False, max_nsamp=nsamp, packed=packed)
    got = _run_host(gpu, ctx, buf, stride, n_streams, nsamp, cmds, packed)
    for k, (res, d) in enumerate(got):
        _check_call(res, d, want[k], msbit[k], ctx.max_dumps, f"call {k}")
    _check_state(ctx.get_state(), state)
    st = ctx.get_state()
    np.testing.assert_array_equal(st["msbit_reg"], msbit[-1])


# ---------------------------------------------------------------- (d) replay fallback
@FMT
def test_replay_ionly_equals_single_calls_and_oracle(gpu, oracle, packed):
    """An I-only context replays as one osg_track_kernel launch per step.  37 channels on 3
    device streams, 4 steps of the 1-ms call (4092 packed bytes a step: step 1 of a packed
    record sits at & 7 == 4), commands that change PRN, slew and stream between steps; the
    packed record starts at an odd byte address.  Byte-identical to 4 track_dev calls on a
    second context, and step K - 1 of 8 channels equals the oracle."""
    rng = np.random.default_rng(404 + packed)
    C, K, nsamp, n_streams = 37, 4, 16368, 3
    stride = K * nsamp + 16                       # samples: 16-byte (int8) / whole-byte strides
    assert stride % 16 == 0 and stride % 32
    streams = [S.synth_if(nsamp * K, 120 + i, [(i + 4, 71 * i, 0, 3)], iq=False)
               for i in range(n_streams)]
    buf = _layout(streams, stride)
    cmds = _random_cmds(rng, K, C, n_streams, slew=True)
    for k in range(1, K):
        sw = rng.random(C) < 0.3
        cmds[k]["prn"][sw] = rng.integers(0, 33, sw.sum())
        cmds[k]["slew"] = np.where(rng.random(C) < 0.3, rng.integers(0, 1200, C), cmds[k]["slew"])
        mv = rng.random(C) < 0.3
        cmds[k]["stream"] = np.where(mv, rng.integers(0, n_streams, C), cmds[k - 1]["stream"])
    rep = gpu.TrackCtx(C, iq=False, max_nsamp=nsamp, packed=packed)
    seq = gpu.TrackCtx(C, iq=False, max_nsamp=nsamp, packed=packed)
    base = 1 if packed else 0                     # packed I-only: any byte address
    raw = gpu.pack2(buf) if packed else buf
    d_if = gpu.DevBuf(base + raw.nbytes + 64)
    d_if.upload(raw, base)
    assert rep.if_bytes(nsamp) == (4092 if packed else nsamp)
    d_cmds = gpu.DevBuf.from_array(cmds)
    d_res = gpu.DevBuf(K * C * gpu.TRACK_RESULT.itemsize)
    rep.replay_dev(d_if.ptr + base, stride, nsamp, K, d_cmds.ptr, d_res.ptr)
    rep.sync()
    got = d_res.download(gpu.TRACK_RESULT).reshape(K, C)
    d_r1 = gpu.DevBuf(C * gpu.TRACK_RESULT.itemsize)
    for k in range(K):
        seq.track_dev(d_if.ptr + base + seq.if_bytes(k * nsamp), stride, nsamp,
                      d_cmds.ptr + k * C * gpu.NCO_CMD.itemsize, d_r1.ptr, 0, seq.next_tic(nsamp))
        seq.sync()
        r = d_r1.download(gpu.TRACK_RESULT)
        assert got[k].tobytes() == r.tobytes(), \
            (k, np.flatnonzero((got[k]["dump"] != r["dump"]).any(axis=1))[:8])
    assert rep.get_state().tobytes() == seq.get_state().tobytes()
    assert rep.next_tic(nsamp) == seq.next_tic(nsamp)
    sel = np.sort(rng.choice(C, 8, replace=False))
    want, msbit, state = _oracle_real(oracle, streams, nsamp, cmds[:, sel].copy())
    assert sum(len(w) for k in range(K) for w in want[k]) >= 8
    for k in range(K):     # every step, K - 1 with the state it leaves
        _check_call(got[k][sel], None, want[k], msbit[k], rep.max_dumps, f"step {k}")
    _check_state(rep.get_state()[sel], state)


# ---------------------------------------------------------------- (e) all or nothing
REFUSED = {
    "ionly_int8_8380": (False, False, 8380),      # step 1 at & 15 == 12
    "iq_int8_8380": (True, False, 8380),          # 16760 bytes a step: & 15 == 8
    "iq_packed_8188": (True, True, 8184 + 4),     # 4094 bytes a step: & 7 == 6
    "ionly_packed_8382": (False, True, 8382),     # step 1 starts inside a byte
}
TIC_PERIOD = 0.0007                               # 11457 samples: the TIC moves at every call


@pytest.mark.parametrize("shape", sorted(REFUSED))
def test_refused_replay_changes_nothing(gpu, shape):
    iq, packed, nsamp = REFUSED[shape]
    C, K = 8, 2
    rng = np.random.default_rng(len(shape))
    ctx, twin = (gpu.TrackCtx(C, iq=iq, max_nsamp=nsamp, packed=packed, samp_rate=FS,
                              tic_period=TIC_PERIOD) for _ in range(2))
    st = ctx.get_state()
    st["carrier_phase"] = rng.integers(0, 1 << 32, C, dtype=np.uint64)
    st["code_phase"] = rng.integers(0, 1 << 32, C, dtype=np.uint64)
    st["half_chip"] = rng.integers(0, 2046, C)
    st["acc"] = rng.integers(-1000, 1000, (C, 6))
    ctx.set_state(st)
    before = ctx.get_state().tobytes()
    d_if = gpu.DevBuf(ctx.if_bytes(K * nsamp) + 64)
    d_if.upload(np.full(d_if.nbytes, 0x1B, np.uint8))     # valid in either format
    cmds = _random_cmds(rng, K, C, 1)
    cmds["prn"] = rng.integers(1, 33, C)
    d_cmds = gpu.DevBuf.from_array(cmds)
    sentinel = np.full(K * C * gpu.TRACK_RESULT.itemsize, 0xA5, np.uint8)
    d_res = gpu.DevBuf.from_array(sentinel)
    # (a single call of this size is served: only the later step is off its alignment)
    with pytest.raises(gpu.GnssCorrError, match="step 1"):
        ctx.replay_dev(d_if.ptr, 0, nsamp, K, d_cmds.ptr, d_res.ptr)
    ctx.sync()
    assert ctx.get_state().tobytes() == before
    np.testing.assert_array_equal(d_res.download(np.uint8), sentinel)
    for _ in range(3):
        assert ctx.next_tic(nsamp) == twin.next_tic(nsamp)


def test_refused_closed_loop_changes_nothing(gpu):
    """The closed loop's correlator + gpsisr launches per call step through the record as
    the replay does: a later call off its alignment refuses the whole request."""
    C, K, nsamp = 12, 2, 8380
    cfg = gpu.osg_loop_cfg()
    loops, cmds = gpu.osg_loop_reset(cfg, np.arange(1, C + 1))
    ctx, twin = (gpu.TrackCtx(C, iq=True, max_nsamp=nsamp, samp_rate=16.0e6,
                              tic_period=TIC_PERIOD) for _ in range(2))
    before = ctx.get_state().tobytes()
    d_if = gpu.DevBuf(ctx.if_bytes(K * nsamp) + 64)
    d_if.upload(np.full(d_if.nbytes, 1, np.int8))
    d_loops, d_cmds = gpu.DevBuf.from_array(loops), gpu.DevBuf.from_array(cmds)
    sentinel = np.full(K * C * gpu.TRACK_RESULT.itemsize, 0xA5, np.uint8)
    d_res = gpu.DevBuf.from_array(sentinel)
    with pytest.raises(gpu.GnssCorrError, match="step 1"):
        gpu.osg_closed_loop_dev(ctx, cfg, d_if.ptr, 0, nsamp, K, C, d_loops.ptr, d_cmds.ptr,
                                d_res.ptr)
    ctx.sync()
    assert ctx.get_state().tobytes() == before
    np.testing.assert_array_equal(d_res.download(np.uint8), sentinel)
    assert d_loops.download(gpu.OSG_LOOP).tobytes() == loops.tobytes()
    assert d_cmds.download(gpu.NCO_CMD).tobytes() == cmds.tobytes()
    for _ in range(3):
        assert ctx.next_tic(nsamp) == twin.next_tic(nsamp)
