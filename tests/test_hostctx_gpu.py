"""The host scaffolding every context family shares (csrc/hostctx.h), on a device: the
device range check of each create, stream / sync / destroy of a live context, and the
growable staging buffers of each family's host API.

Growth: a host-API call at a small size, the same call at a larger size that makes
every staging buffer of the family grow (the old block is freed and a new one
allocated), then the small call again.  The two small calls must answer bit-equal: the
kernels are deterministic, so any difference would come from a stale pointer or
capacity.  Every configuration is the family's smallest.
"""
import ctypes as C

import numpy as np
import pytest

import e1t_scenarios as E

pytestmark = pytest.mark.gpu

OK, EINVAL = 0, -1
FS = 16e6


def _creates(gc, device):
    """(function name, family prefix, call(handle)) with each family's smallest
    valid configuration on `device`."""
    L = gc.lib()
    track = gc.TrackCfg(1, gc.IF_IQ, device, 2046, 16.368e6, 0.0)
    acq = gc.AcqCfg(64e3, 64, device, 1, 1, 1, gc.ACQ_F64)
    sgt, e1t = gc.sgt_cfg(0, device), gc.e1t_cfg(device, maxCodes=1)
    sdr_acq, sdr_corr = gc.SdrAcqCfg(38400.0, device, 0), gc.SdrCorrCfg(device, 0)
    return [
        ("gnsscorr_track_create", "gnsscorr_track",
         lambda h: L.gnsscorr_track_create(C.byref(h), C.byref(track))),
        ("gnsscorr_acq_create", "gnsscorr_acq",
         lambda h: L.gnsscorr_acq_create(C.byref(h), C.byref(acq))),
        ("gnsscorr_sgt_create", "gnsscorr_sgt",
         lambda h: L.gnsscorr_sgt_create(C.byref(h), C.byref(sgt))),
        ("gnsscorr_e1t_create", "gnsscorr_e1t",
         lambda h: L.gnsscorr_e1t_create(C.byref(h), C.byref(e1t))),
        ("gnsscorr_sdr_acq_create", "gnsscorr_sdr_acq",
         lambda h: L.gnsscorr_sdr_acq_create(C.byref(h), C.byref(sdr_acq))),
        ("gnsscorr_sdr_corr_create", "gnsscorr_sdr_corr",
         lambda h: L.gnsscorr_sdr_corr_create(C.byref(h), C.byref(sdr_corr))),
        ("gnsscorr_sdr_fe_create", "gnsscorr_sdr_fe",
         lambda h: L.gnsscorr_sdr_fe_create(C.byref(h), device)),
    ]


FAMILIES = ["track", "acq", "sgt", "e1t", "sdr_acq", "sdr_corr", "sdr_fe"]


@pytest.mark.parametrize("family", range(7), ids=FAMILIES)
def test_device_out_of_range(gpu, family):
    L, n = gpu.lib(), gpu.device_count()
    name, _, create = _creates(gpu, n)[family]
    h = C.c_void_p(0xdead)
    assert create(h) == EINVAL
    assert L.gnsscorr_last_error().decode() == f"{name}: device {n} out of range"
    assert not h.value
    h = C.c_void_p(0xdead)
    assert _creates(gpu, -1)[family][2](h) == EINVAL
    assert L.gnsscorr_last_error().decode() == f"{name}: device -1 out of range"
    assert not h.value


@pytest.mark.parametrize("family", range(7), ids=FAMILIES)
def test_stream_sync_destroy(gpu, family):
    L = gpu.lib()
    name, prefix, create = _creates(gpu, 0)[family]
    h = C.c_void_p()
    assert create(h) == OK, L.gnsscorr_last_error()
    assert h.value
    assert getattr(L, prefix + "_stream")(h)
    assert getattr(L, prefix + "_stream")(None) is None
    assert getattr(L, prefix + "_sync")(h) == OK
    assert getattr(L, prefix + "_sync")(None) == EINVAL
    assert getattr(L, prefix + "_destroy")(h) == OK
    assert getattr(L, prefix + "_destroy")(None) == OK


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert a.tobytes() == b.tobytes()


def test_growth_sdr_fe(gpu):
    """d_in, d_out: 1 block, then 3."""
    rng = np.random.default_rng(1)
    data = rng.integers(0, 4, 3 * gpu.GN3S_BLOCK_IN).astype(np.uint8)
    ctx = gpu.SdrFeCtx()
    small, ph = ctx.gn3s(data[:gpu.GN3S_BLOCK_IN])
    large, ph3 = ctx.gn3s(data)
    again, ph_again = ctx.gn3s(data[:gpu.GN3S_BLOCK_IN])
    assert small.any() and ph == ph_again
    _same(small, again)
    _same(large[:len(small)], small)              # the first block of three is the one block
    ctx.close()


def test_growth_sdr_acq(gpu):
    """d_X, d_rows and the per-call staging: 1 record x 1 SV, then 2 x 2; the medium
    search goes through the same staging with 10-ms records."""
    rng = np.random.default_rng(2)
    buf = rng.integers(-200, 200, (2, 10 * 2048, 2)).astype(np.int16)
    ctx = gpu.SdrAcqCtx()
    kw = dict(doppmin=-2000, doppmax=2000)
    small = ctx.strong(buf[:1, :2048], [3], **kw)
    large = ctx.strong(buf[:, :2048], [3, 7], **kw)
    again = ctx.strong(buf[:1, :2048], [3], **kw)
    assert small.shape == (1, 1) and large.shape == (2, 2) and small["magnitude"][0, 0] > 0
    _same(small, again)
    _same(large[:1, :1], small)
    small = ctx.acquire(gpu.SDR_ACQ_MEDIUM, buf[:1], [3], **kw)
    large = ctx.acquire(gpu.SDR_ACQ_MEDIUM, buf, [3, 7], **kw)
    again = ctx.acquire(gpu.SDR_ACQ_MEDIUM, buf[:1], [3], **kw)
    assert small["magnitude"][0, 0] > 0
    _same(small, again)
    _same(large[:1, :1], small)
    ctx.close()


def test_growth_sdr_correlate(gpu):
    """d_packets and the job staging (device and pinned): 1 packet x 1 channel, then
    2 packets x 3 channels.  Every call starts from the same channel state."""
    rng = np.random.default_rng(3)
    pk = rng.integers(-60, 60, (2, 2048, 2)).astype(np.int16)
    ctx = gpu.SdrCorrCtx()
    st0 = np.zeros(3, gpu.SDR_CHAN)
    for c, (sv, cp, dop) in enumerate([(4, 100, 500), (9, 900, -1500), (30, 1700, 2500)]):
        st0[c] = ctx.init_chan(sv, cp, dop)

    def run(n_pk, n_ch):
        st, corr = st0[:n_ch].copy(), np.zeros(n_ch, gpu.SDR_CORR)
        ctx.correlate(pk[:n_pk], st, corr, None, rx=np.arange(n_ch) % n_pk)
        return st, corr

    small, large, again = run(1, 1), run(2, 3), run(1, 1)
    assert small[1]["i"].any() or small[1]["q"].any()
    for a, b in zip(small, again):
        _same(a, b)
    for a, b in zip(small, large):                 # channel 0 reads packet 0 in both
        _same(a, b[:1])
    ctx.close()


def test_growth_track(gpu):
    """d_if: 1023 samples, then 2046 (max_nsamp).  The channel state is put back before
    each call; the TIC period is long enough for no call to see a TIC."""
    rng = np.random.default_rng(4)
    IF = rng.integers(-3, 4, 2046 * 2).astype(np.int8)
    ctx = gpu.TrackCtx(1, iq=True, max_nsamp=2046, tic_period=100.0)
    cmd = np.zeros(1, gpu.NCO_CMD)
    cmd["prn"], cmd["carrier_incr"], cmd["code_incr"] = 5, 635008600, 6710886 * 40
    cmd["epoch_load"] = -1
    st0 = ctx.get_state()

    def run(nsamp):
        ctx.set_state(st0)
        res, tic = ctx.track(IF[:2 * nsamp], nsamp, cmd)
        assert not tic
        return res, ctx.get_state()

    small, large, again = run(1023), run(2046), run(1023)
    assert small[1]["acc"].any() and large[1].tobytes() != small[1].tobytes()
    for a, b in zip(small, again):
        _same(a, b)
    ctx.close()


def test_growth_acq(gpu):
    """N = 64, the generic fp64 engine's lower bound: 1 group x 1 frequency, then
    2 groups x 3 frequencies (d_in64, d_X64, d_stats, d_rows, d_res, d_gcode and d_gfreq
    all grow; d_codes8 at set_codes)."""
    rng = np.random.default_rng(5)
    n = 64
    ctx = gpu.AcqCtx(64e3, n, max_freqs=3, max_blocks=1, max_codes=1)
    code = np.where(rng.random(n) < 0.5, -1, 1).astype(np.int8)
    ctx.set_codes(code[None])
    IF = rng.integers(-3, 4, 2 * n).astype(np.int8)
    IF[0::2] += 2 * np.roll(code, 11)               # a peak to find, at lag 11
    freqs = np.array([0.0, 1000.0, -1000.0])

    def run(n_groups, n_freqs):
        gf = np.tile(np.arange(n_freqs), (n_groups, 1))
        return ctx.search(IF, 1, freqs[:n_freqs], np.zeros(n_groups, np.int32), gf, spc=2)

    small, large, again = run(1, 1), run(2, 3), run(1, 1)
    assert small[1]["peak"][0, 0] > 0
    for a, b in zip(small, again):
        _same(a, b)
    _same(large[1][:1, :1], small[1])               # the same code and frequency
    ctx.close()


def _float_growth(gpu, ctx, ids, sums_per_epoch):
    """track: d_chan, d_ep (1 channel x 1 epoch, then 3 x 2); replay: buffers of the call."""
    n = 40000
    d_if = gpu.DevBuf.from_array(gpu.ifgen(n, [], fs=FS, seed=6))
    ch0 = ctx.init_chans(ids, [1, 700, 1500], [2.42e6, 2.42e6 + 900.0, 2.42e6 - 1700.0])

    def track(n_ch, n_ep):
        ch = ch0[:n_ch].copy()
        return ctx.track(d_if.ptr, 0, n, ch, n_ep, closed_loop=True), ch

    small, large, again = track(1, 1), track(3, 2), track(1, 1)
    assert (large[0]["status"] == 0).all() and (large[0]["blksize"] > 0).all()
    for a, b in zip(small, again):
        _same(a, b)
    _same(large[0][:1, :1], small[0])               # channel 0's first epoch
    d_if.free()

    sums = np.random.default_rng(7).normal(0.0, 4000.0, (3, 2, sums_per_epoch))

    def replay(n_ch, n_ep):
        ch = ch0[:n_ch].copy()
        return ctx.replay(ch, sums[:n_ch, :n_ep]), ch

    small, large, again = replay(1, 1), replay(3, 2), replay(1, 1)
    for a, b in zip(small, again):
        _same(a, b)
    _same(large[0][:1, :1], small[0])
    ctx.close()


def test_growth_sgt(gpu):
    _float_growth(gpu, gpu.SgtCtx(0, samplingFreq=FS), [1, 2, 3], 6)


def test_growth_e1t(gpu):
    codes, _ = E.fixture_codes()
    ctx = gpu.E1tCtx(samplingFreq=FS, maxCodes=3)
    ctx.set_codes(codes)
    _float_growth(gpu, ctx, [0, 1, 2], 10)
