"""GPU: 2-bit packed records (GNSSCORR_IF_PACKED2) in the float trackers sgt, e1t, l3t.

gnsscorr_{sgt,e1t,l3t}_set_packed(ctx, 1) makes the records of later track calls packed
element streams.  The kernels unpack in registers to the int8 words their arithmetic
consumes and keep the chunk partition of an int8 record on a 16-byte-aligned base, so for
the same settings, channels and epochs the packed run's epoch records and final channel
array are BYTE-EQUAL to the int8 run on the unpacked levels: no tolerance.  The int8 path
is held to the Scilab restatements by the other GPU tests; one case per tracker here is
checked against its Python oracle directly as well, with the tolerance that tracker's own
GPU test applies to the same quantities.

Records are int8 levels in {-3,-1,1,3}: gc.ifgen for GPS / GLONASS, the scene generators
of tests/*_scenarios.py for B1I, E1B and L3OC requantised to four levels (the sign, the
magnitude thresholded at the scene's noise sigma, zero -> +1).  The int8 record sits in a
DevBuf (16-byte-aligned base) with strides that are multiples of 64 bytes, pack2 of it is
the packed record with a quarter of the stride.
"""
import functools

import numpy as np
import pytest

import b1i_scenarios as B
import e1alt_scenarios as EA
import e1t_scenarios as E
import l3_scenarios as L3
import sgt_oracle as S
from test_sgt_gpu import _glonass_scene
from tracker_checks import close as _close, noise

pytestmark = pytest.mark.gpu
FS = 16e6
OFFS64 = (0, 1, 2, 3, 5, 31, 32, 63)     # pos mod 64: every 2-bit, nibble and byte offset


def requantise(x, sigma):
    """int8 samples -> the four GN3S levels: sign, |x| > sigma -> 3 else 1, zero -> +1."""
    x = np.asarray(x, np.int16)
    return (np.where(x < 0, -1, 1) * np.where(np.abs(x) > sigma, 3, 1)).astype(np.int8)


@functools.lru_cache(maxsize=None)
def _b1i_record(file_type):
    IF, chans = B.scene(n_ms=8)
    lv = requantise(IF, 24)                 # unit-variance noise scaled by 24
    return (lv if file_type == 2 else lv[0::2].copy()), chans


@functools.lru_cache(maxsize=None)
def _e1b_record(file_type):
    IF, codes, chans = E.closed_loop_scene()
    lv = requantise(IF, 6)                  # synth_e1b: noise sigma 6 per component
    return (lv if file_type == 2 else lv[0::2].copy()), codes, chans


@functools.lru_cache(maxsize=None)
def _l3_record():
    IF, prn, cp, f0, _ = L3.closed_loop_scene()
    return requantise(IF, 6), prn, cp, f0   # synth_l3: noise sigma 6 per component


def _pair(gc, ctx, rec, n, ch, n_ep, closed, stride=0):
    """The int8 run, then the packed run of the same call on one context; asserts that the
    epoch records and the channel arrays are byte-equal and returns the int8 run's."""
    rec = np.ascontiguousarray(rec, np.int8)
    d8, dp = gc.DevBuf.from_array(rec), gc.DevBuf.from_array(gc.pack2(rec))
    assert d8.ptr % 16 == 0 and dp.ptr % 16 == 0 and stride % 64 == 0
    ca, cb = ch.copy(), ch.copy()
    ctx.set_packed(False)
    ea = ctx.track(d8.ptr, stride, n, ca, n_ep, closed_loop=closed)
    ctx.set_packed(True)
    eb = ctx.track(dp.ptr, stride // 4, n, cb, n_ep, closed_loop=closed)
    ctx.set_packed(False)
    for f in ea.dtype.names:
        assert ea[f].tobytes() == eb[f].tobytes(), \
            (f, np.argwhere(ea[f] != eb[f])[:4], ea[f][ea[f] != eb[f]][:4], eb[f][ea[f] != eb[f]][:4])
    assert ea.tobytes() == eb.tobytes()
    assert ca.tobytes() == cb.tobytes()
    return ea, ca


def _sgt_record(gc, system, file_type, fs=FS, n=100000):
    if system == 2:
        return _b1i_record(file_type)[0]
    return noise(gc, n, fs, file_type, seed=21 + system)


def _sgt_chans(gc, rng, system, fs, n_samples, offs=OFFS64, mod=64, basis=None):
    C = len(offs)
    s = S.settings(system) if system != 2 else B.settings()
    basis = basis or s["codeFreqBasis"]
    ch = np.zeros(C, gc.SGT_CHAN)
    ch["code_id"] = (rng.integers(-7, 7, C) if system == 1 else
                     rng.integers(1, 38 if system == 2 else 33, C))
    room = n_samples - int(3.2e-3 * fs) - mod
    ch["pos"] = mod * rng.integers(0, room // mod, C) + np.asarray(offs)
    ch["code_freq"] = basis + rng.uniform(-40, 40, C)
    ch["rem_code"] = rng.uniform(0, 1, C) * (ch["code_freq"] / fs)
    ch["rem_carr"] = rng.uniform(-6.2, 6.2, C)
    ch["carr_freq"] = rng.uniform(-3e6, 3e6, C)
    return ch


def _ran(ep):
    assert (ep["status"] == 0).all() and (ep["blksize"] > 0).all()
    assert (ep[ep.dtype.names[1]] != 0).all()


# ---------------------------------------------------------------- 1. sgt, all shapes
@pytest.mark.parametrize("chunk", ["1", "0"])
@pytest.mark.parametrize("threads", [None, "64", "1024"])
@pytest.mark.parametrize("system,file_type,switch",
                         [(0, 2, 0), (1, 2, 0), (1, 1, 0), (0, 1, 0), (2, 2, 0), (2, 1, 0),
                          (1, 2, 1)])
def test_sgt_open_loop_every_shape(gpu, system, file_type, switch, threads, chunk, monkeypatch):
    """16 Msps, open loop, 2 epochs, 8 channels at every 2-bit / nibble / byte offset and
    with a chunk straddling a 16-byte word: run_chips (GPS kC 16, GLONASS kC 32; the 256-
    thread and the wave shape), run_chunks (the 1024-thread shape; B1I wave shape kC 8),
    the per-sample pass (GNSSCORR_SGT_CHUNK=0; B1I elsewhere); one switchIQ case."""
    gc = gpu
    monkeypatch.setenv("GNSSCORR_SGT_CHUNK", chunk)
    if threads:
        monkeypatch.setenv("GNSSCORR_SGT_THREADS", threads)
    rec = _sgt_record(gc, system, file_type)
    n = len(rec) // file_type
    ctx = gc.SgtCtx(system, fileType=file_type, switchIQ=switch, samplingFreq=FS)
    ch = _sgt_chans(gc, np.random.default_rng(7 + system + 3 * file_type), system, FS, n)
    ep, _ = _pair(gc, ctx, rec, n, ch, 2, False)
    _ran(ep)


# ---------------------------------------------------------------- 2. sgt path selection
@pytest.mark.parametrize("threads", [None, "64"])
@pytest.mark.parametrize("system,file_type", [(0, 2), (1, 2), (1, 1)])
def test_sgt_wide_spacing_runs_chunk_grid(gpu, system, file_type, threads, monkeypatch):
    """dllCorrelatorSpacing = 0.5 at 16 Msps: run_chunks (prefix columns in the 256-thread
    shape, the code select in the wave shape), kC 16 (GPS) and 32 (GLONASS)."""
    gc = gpu
    if threads:
        monkeypatch.setenv("GNSSCORR_SGT_THREADS", threads)
    rec = _sgt_record(gc, system, file_type)
    n = len(rec) // file_type
    ctx = gc.SgtCtx(system, fileType=file_type, samplingFreq=FS, dllCorrelatorSpacing=0.5)
    ch = _sgt_chans(gc, np.random.default_rng(29 + system + 3 * file_type), system, FS, n)
    _ran(_pair(gc, ctx, rec, n, ch, 2, False)[0])


@pytest.mark.parametrize("threads", [None, "64"])
@pytest.mark.parametrize("system,file_type", [(0, 2), (1, 2), (0, 1), (1, 1)])
def test_sgt_16368_runs_the_odd_chip_forms(gpu, system, file_type, threads, monkeypatch):
    """16.368 Msps: 16.0 / 32.03 samples per chip, run_chips with kC 17 and 33."""
    gc = gpu
    fs = 16.368e6
    if threads:
        monkeypatch.setenv("GNSSCORR_SGT_THREADS", threads)
    rec = _sgt_record(gc, system, file_type, fs)
    n = len(rec) // file_type
    ctx = gc.SgtCtx(system, fileType=file_type, samplingFreq=fs)
    ch = _sgt_chans(gc, np.random.default_rng(31 + system + 3 * file_type), system, fs, n)
    _ran(_pair(gc, ctx, rec, n, ch, 2, False)[0])


@pytest.mark.parametrize("system,file_type", [(0, 2), (1, 1)])
def test_sgt_low_rate_takes_the_per_sample_path(gpu, system, file_type):
    """4.096 Msps: chunking is ineligible (15 * step >= 1)."""
    gc = gpu
    fs = 4.096e6
    rec = _sgt_record(gc, system, file_type, fs, n=40000)
    n = len(rec) // file_type
    ctx = gc.SgtCtx(system, fileType=file_type, samplingFreq=fs)
    ch = _sgt_chans(gc, np.random.default_rng(37 + system), system, fs, n)
    _ran(_pair(gc, ctx, rec, n, ch, 2, False)[0])


@pytest.mark.parametrize("threads", [None, "64"])
@pytest.mark.parametrize("system,file_type", [(1, 2), (0, 2), (1, 1)])
def test_sgt_crossings_on_exact_chips(gpu, system, file_type, threads, monkeypatch):
    """codeFreq = fs/32 (GPS fs/16), remCode on the 1/32 grid: every crossing on an exact
    sample, so the chunk paths' estimates have no margin and the exact recompute decides."""
    gc = gpu
    if threads:
        monkeypatch.setenv("GNSSCORR_SGT_THREADS", threads)
    rng = np.random.default_rng(5 + system + 2 * file_type)
    rec = _sgt_record(gc, system, file_type)
    n = len(rec) // file_type
    ctx = gc.SgtCtx(system, fileType=file_type, samplingFreq=FS)
    ch = _sgt_chans(gc, rng, system, FS, n)
    ch["code_freq"] = FS / (32 if system == 1 else 16)
    ch["rem_code"] = rng.integers(0, 2, len(ch)) / 32.0
    _ran(_pair(gc, ctx, rec, n, ch, 2, False)[0])


@pytest.mark.parametrize("threads", [None, "64"])
def test_sgt_state_from_outside_takes_the_clamped_path(gpu, threads, monkeypatch):
    """rem_code < spc - 1 (a state set from outside): the per-sample pass with its indices
    clamped into the table, beside channels on the chunk path in the same launch."""
    gc = gpu
    if threads:
        monkeypatch.setenv("GNSSCORR_SGT_THREADS", threads)
    rec = _sgt_record(gc, 0, 2)
    n = len(rec) // 2
    ctx = gc.SgtCtx(0, samplingFreq=FS)
    ch = _sgt_chans(gc, np.random.default_rng(43), 0, FS, n)
    ch["rem_code"][::2] = -1.5
    assert (ch["rem_code"][::2] < ctx.cfg.dll_spacing - 1).all()
    _ran(_pair(gc, ctx, rec, n, ch, 2, False)[0])


# ---------------------------------------------------------------- 3. sgt closed loop
def test_sgt_glonass_14_fch_closed_loop(gpu):
    gc = gpu
    IF, fchs, starts, acq = _glonass_scene(gc, 4)
    ctx = gc.SgtCtx(1)
    ch = ctx.init_chans(fchs, starts, acq)
    ep, _ = _pair(gc, ctx, IF, len(IF) // 2, ch, 3, True)
    _ran(ep)


def test_sgt_two_records_closed_loop(gpu):
    """Two records (streams) of 2 GPS channels each; the int8 stride is a multiple of 64
    bytes, the packed one a quarter of it."""
    gc = gpu
    n = 80000
    stride = 2 * n + 64                       # bytes; the gap holds valid levels
    buf = np.ones(2 * stride, np.int8)
    meta = []
    for r in range(2):
        prns, cps, dops = [3 + r, 17 + r], [200.5 + 300 * r, 811.25], [-2500.0 + 900 * r, 3100.0]
        sigs = [dict(system=0, prn=p, code_phase=c, doppler=d, cn0=47.0, data_bits=1)
                for p, c, d in zip(prns, cps, dops)]
        buf[r * stride: r * stride + 2 * n] = gc.ifgen(n, sigs, fs=FS, seed=90 + r)
        meta += [(r, p, int(round((1023 - c) / 1.023e6 * FS)) + 1, 2.42e6 + d + 7.0)
                 for p, c, d in zip(prns, cps, dops)]
    ctx = gc.SgtCtx(0)
    ch = ctx.init_chans([m[1] for m in meta], [m[2] for m in meta], [m[3] for m in meta],
                        streams=[m[0] for m in meta])
    ep, _ = _pair(gc, ctx, buf, n, ch, 3, True, stride=stride)
    _ran(ep)
    assert (ep["I_P"][:2] != ep["I_P"][2:]).all()       # the streams are different records


def test_sgt_many_channels_switch_to_one_wave_per_channel(gpu):
    gc = gpu
    IF, fchs, starts, acq = _glonass_scene(gc, 4)
    ctx = gc.SgtCtx(1)
    big = np.tile(ctx.init_chans(fchs, starts, acq), 80)      # 1120 channels
    ep, _ = _pair(gc, ctx, IF, len(IF) // 2, big, 1, True)
    _ran(ep)


# ---------------------------------------------------------------- 4. e1t
E1_MODES = {"5arm": {}, "4ms": EA.MODES["4ms"], "amb1": EA.MODES["amb1"], "amb4": EA.MODES["amb4"]}


def _e1t_chans(gc, ctx, rng, n, mode, offs=(0, 1, 7, 31)):
    C = len(offs)
    ch = ctx.init_chans(rng.integers(0, 3, C), [1] * C, [2.42e6] * C)
    ms4 = mode in ("4ms", "amb4")
    room = n - int((4.3e-3 if ms4 else 2.3e-3) * FS) - 32
    ch["pos"] = 32 * rng.integers(0, room // 32, C) + np.asarray(offs)
    ch["code_freq"] += rng.uniform(-20, 20, C)
    ch["rem_code"] = rng.uniform(0, 1, C) * (ch["code_freq"] / FS)
    ch["rem_meandr"] = 0.0 if mode.startswith("amb") else 2 * ch["rem_code"]
    ch["rem_carr"] = rng.uniform(-6.2, 6.2, C)
    ch["carr_freq"] = 2.42e6 + rng.uniform(-4000, 4000, C)
    ch["carr_freq_basis"] = ch["carr_freq"]
    ch["segment"] = 0 if ms4 else rng.integers(0, 4, C)
    return ch


@pytest.mark.parametrize("chunk", ["1", "0"])
@pytest.mark.parametrize("threads", [None, "64"])
@pytest.mark.parametrize("file_type", [2, 1])
@pytest.mark.parametrize("mode", list(E1_MODES))
def test_e1t_every_mode_and_shape(gpu, mode, file_type, threads, chunk, monkeypatch):
    """The four loop modes, IQ and real records, both launch shapes, the chunked (kC = 16)
    and the per-sample path; open and closed loop; 4 channels at pos mod 32 in 0, 1, 7, 31."""
    gc = gpu
    monkeypatch.setenv("GNSSCORR_E1T_CHUNK", chunk)
    if threads:
        monkeypatch.setenv("GNSSCORR_E1T_THREADS", threads)
    rec, codes, _ = _e1b_record(file_type)
    n = len(rec) // file_type
    ctx = gc.E1tCtx(fileType=file_type, **E1_MODES[mode])
    ctx.set_codes(codes)
    ch = _e1t_chans(gc, ctx, np.random.default_rng(11 + file_type), n, mode)
    n_ep = 1 if mode in ("4ms", "amb4") else 2
    for closed in (False, True):
        _ran(_pair(gc, ctx, rec, n, ch, n_ep, closed)[0])


# ---------------------------------------------------------------- 5. l3t
@pytest.mark.parametrize("threads", [None, "64"])
@pytest.mark.parametrize("switch_iq", [0, 1])
def test_l3t_closed_loop(gpu, switch_iq, threads, monkeypatch):
    gc = gpu
    if threads:
        monkeypatch.setenv("GNSSCORR_L3T_THREADS", threads)
    rec, prn, cp, f0 = _l3_record()
    ctx = gc.L3tCtx(switchIQ=switch_iq)
    ch = ctx.init_chans([prn, prn], [cp, cp + 24000 + 1], [f0, f0])
    assert ch["pos"][0] % 2 != ch["pos"][1] % 2
    _ran(_pair(gc, ctx, rec, len(rec) // 2, ch, 2, True)[0])


# ---------------------------------------------------------------- 6. the record's end
def _end_case(gc, ctx, rec, bps, ch):
    """Channel 0's second epoch ends on the record's last sample, n_samples is no multiple
    of 4, the buffer goes on with other nonzero codes: two epochs equal, the third stops
    with status 1 and the int8 run's blksize."""
    full = len(rec) // bps
    ch[:] = ch[np.argsort(-ch["pos"], kind="stable")]     # the latest channel first
    assert ch["pos"][0] - ch["pos"][1:].max() >= 16        # the others end inside the record
    d8 = gc.DevBuf.from_array(rec)
    probe = ch.copy()
    blk = ctx.track(d8.ptr, 0, full, probe, 2, closed_loop=False)["blksize"][0]
    n = int(ch["pos"][0] + blk.sum())
    if n % 4 == 0:                      # blksize does not depend on the position
        ch["pos"][0] += 1
        n += 1
    assert n % 4 != 0 and n + 64 < full
    assert np.count_nonzero(gc.pack2(rec)[(bps * n + 3) // 4:][:64]) > 32
    ep, cf = _pair(gc, ctx, rec, n, ch, 3, False)
    assert (ep["status"][0] == [0, 0, 1]).all() and cf["status"][0] == 1
    assert cf["pos"][0] == n and ep["blksize"][0][2] > 0
    assert (ep["status"][1:, :2] == 0).all()
    return ep


@pytest.mark.parametrize("path", ["chips", "chunks", "sample", "wave"])
@pytest.mark.parametrize("file_type", [2, 1])
def test_sgt_record_end(gpu, file_type, path, monkeypatch):
    gc = gpu
    if path == "sample":
        monkeypatch.setenv("GNSSCORR_SGT_CHUNK", "0")
    if path == "wave":
        monkeypatch.setenv("GNSSCORR_SGT_THREADS", "64")
    rec = _sgt_record(gc, 0, file_type)
    kw = dict(dllCorrelatorSpacing=0.5) if path == "chunks" else {}
    ctx = gc.SgtCtx(0, fileType=file_type, samplingFreq=FS, **kw)
    ch = _sgt_chans(gc, np.random.default_rng(53), 0, FS, len(rec) // file_type - 40000,
                    offs=(3, 0, 9))
    _end_case(gc, ctx, rec, file_type, ch)


@pytest.mark.parametrize("chunk", ["1", "0"])
@pytest.mark.parametrize("file_type", [2, 1])
def test_e1t_record_end(gpu, file_type, chunk, monkeypatch):
    gc = gpu
    monkeypatch.setenv("GNSSCORR_E1T_CHUNK", chunk)
    rec, codes, _ = _e1b_record(file_type)
    ctx = gc.E1tCtx(fileType=file_type)
    ctx.set_codes(codes)
    ch = _e1t_chans(gc, ctx, np.random.default_rng(59), len(rec) // file_type - 40000, "5arm",
                    offs=(3, 0))
    _end_case(gc, ctx, rec, file_type, ch)


def test_l3t_record_end(gpu):
    gc = gpu
    rec, prn, cp, f0 = _l3_record()
    ctx = gc.L3tCtx()
    ch = ctx.init_chans([prn, prn], [cp + 65, cp], [f0, f0])
    _end_case(gc, ctx, rec, 2, ch)


# ---------------------------------------------------------------- 7. against the oracles
def test_sgt_packed_against_the_oracle(gpu):
    """GLONASS closed loop on the packed record against oracle/sgt_oracle.py on the levels
    (the bound of test_config4_glonass_14_fch_closed_loop)."""
    gc = gpu
    IF, fchs, starts, acq = _glonass_scene(gc, 4)
    ctx = gc.SgtCtx(1)
    ch = ctx.init_chans(fchs[:4], starts[:4], acq[:4])
    ctx.set_packed()
    dp = gc.DevBuf.from_array(gc.pack2(IF))
    ep = ctx.track(dp.ptr, 0, len(IF) // 2, ch, 3, closed_loop=True)
    s = S.settings(1)
    for i in range(4):
        r = S.track(IF, s, int(fchs[i]), starts[i], float(acq[i]), 3)
        assert (ep["status"][i] == 0).all() and (ep["blksize"][i] == r["blksize"]).all()
        for f in S.FIELDS:
            assert _close(ep[f][i], r[f], rtol=1e-6, atol=1e-6).all(), (i, f, ep[f][i], r[f])


def test_e1t_packed_against_the_oracle(gpu):
    """Default mode, closed loop, against e1t_scenarios.track on the level record (the
    bound of test_closed_loop_three_prns_40_ms)."""
    gc = gpu
    rec, codes, chans = _e1b_record(2)
    ctx = gc.E1tCtx()
    ctx.set_codes(codes)
    ch = ctx.init_chans([c[0] for c in chans], [c[1] for c in chans], [c[2] for c in chans])
    ctx.set_packed()
    dp = gc.DevBuf.from_array(gc.pack2(rec))
    ep = ctx.track(dp.ptr, 0, len(rec) // 2, ch, 3, closed_loop=True)
    s = E.settings()
    for i, (row, cp, f0, _) in enumerate(chans):
        r = E.track(rec, s, codes[row], cp, f0, 3)
        assert (ep["status"][i] == 0).all() and (ep["blksize"][i] == r["blksize"]).all()
        assert (ep["segment"][i] == r["segment"]).all()
        for f in E.FIELDS:
            assert _close(ep[f][i], r[f]).all(), (i, f, ep[f][i], r[f])


def test_l3t_packed_against_the_oracle(gpu):
    """Closed loop against l3_scenarios.track on the level record (LOOP_TOL of
    tests/test_l3_gpu.py, 1e-7)."""
    gc = gpu
    rec, prn, cp, f0 = _l3_record()
    ctx = gc.L3tCtx()
    ch = ctx.init_chans([prn], [cp], [f0])
    ctx.set_packed()
    dp = gc.DevBuf.from_array(gc.pack2(rec))
    ep = ctx.track(dp.ptr, 0, len(rec) // 2, ch, 3, closed_loop=True)
    r = L3.track(rec, L3.settings(), prn, cp, f0, 3)
    assert (ep["status"][0] == 0).all() and (ep["blksize"][0] == r["blksize"]).all()
    for f in L3.FIELDS:
        assert _close(ep[f][0], r[f], 1e-7, 1e-7).all(), (f, ep[f][0], r[f])


# ---------------------------------------------------------------- 8. arguments
def _ctxs(gc):
    e = gc.E1tCtx()
    e.set_codes(_e1b_record(2)[1])
    return [gc.SgtCtx(0), e, gc.L3tCtx()]


def test_set_packed_refuses_other_values(gpu):
    gc = gpu
    for ctx in _ctxs(gc):
        fn = getattr(gc.lib(), ctx._prefix + "_set_packed")
        for bad in (2, -1):
            assert fn(ctx.h, bad) == -1                               # GNSSCORR_EINVAL
            assert b"set_packed" in gc.lib().gnsscorr_last_error()
        assert fn(None, 1) == -1
        with pytest.raises(gc.GnssCorrError):
            ctx.set_packed(2)


def test_packed_alignment_is_checked_before_any_launch(gpu):
    gc = gpu
    d = gc.DevBuf(1 << 20)
    for ctx in _ctxs(gc):
        ch = np.zeros(1, ctx._CHAN)
        ch["code_id"] = 1
        ch["code_freq"] = ctx.cfg.code_freq_basis
        ctx.set_packed()
        for ptr, stride in ((d.ptr, 24), (d.ptr + 4, 0), (d.ptr + 4, 64)):
            c = ch.copy()
            ep = np.zeros((1, 1), ctx._EPOCH)
            rc = ctx._track(ctx.h, ptr, stride, 1000, 1, c.ctypes.data, 1, 0, ep.ctypes.data)
            assert rc == -1 and b"16" in gc.lib().gnsscorr_last_error()
            assert c.tobytes() == ch.tobytes()                        # nothing ran
        # the same arguments are fine for int8 records
        ctx.set_packed(False)
        c = ch.copy()
        ctx.track(d.ptr + 4, 24, 1000, c, 1, closed_loop=False)


def test_set_packed_0_gives_the_int8_results_again(gpu):
    gc = gpu
    rec = _sgt_record(gc, 0, 2)
    n = len(rec) // 2
    ctx, ref = gc.SgtCtx(0), gc.SgtCtx(0)
    ch = _sgt_chans(gc, np.random.default_rng(61), 0, FS, n)
    d8 = gc.DevBuf.from_array(rec)
    want_c = ch.copy()
    want = ref.track(d8.ptr, 0, n, want_c, 2, closed_loop=False)      # never packed
    _pair(gc, ctx, rec, n, ch, 2, False)                              # packed, then back to 0
    got_c = ch.copy()
    got = ctx.track(d8.ptr, 0, n, got_c, 2, closed_loop=False)
    assert got.tobytes() == want.tobytes() and got_c.tobytes() == want_c.tobytes()
