"""GPU: int16 IF records: GNSSCORR_IF_INT16 in the fp64 acquisition, record format 2
(gnsscorr_{sgt,e1t,l3t}_set_record_format) in the float trackers.

1. Bit identity, no tolerance: a record of int8-range levels stored as int16 gives
   results BYTE-EQUAL to the int8 path on the same levels (int8 record on a
   16-byte-aligned base): the int16 kernels keep the int8 kernels' lane-to-sample
   assignment and convert the same values.
2. Full range: the same scenes scaled to the whole int16 range, with the elements 0x00FF,
   0xFF00, 0x7FFF, -32768 and low bytes >= 0x80 planted, against the numpy restatements
   fed the int16 array, with the tolerance each family's own int8 GPU test applies.  The
   restatement is first shown decidable at that scale (blksize unchanged under a 1e-9
   perturbation of the sums; peak and second peak separated).
3. Arguments: what is refused, before any launch.
"""
import functools

import numpy as np
import pytest

import acq_oracle as A
import b1i_scenarios as B
import e1b_scenarios as E1B
import e1t_scenarios as E
import l3_scenarios as L3
import sgt_oracle as S
from test_ftrack_packed_gpu import (E1_MODES, _e1b_record, _e1t_chans, _l3_record,
                                    _ran, _sgt_chans, _sgt_record)
from test_sgt_gpu import _glonass_scene
from tracker_checks import close as _close

pytestmark = pytest.mark.gpu
FS = 16e6
OFFS = (0, 1, 5, 31)          # pos mod 64: on the chunk grid, odd, off the grid
# 0x00FF 0xFF00 0x7FFF 0x8000, then low bytes >= 0x80 under positive and negative high bytes
PLANT = np.array([0x00FF, -256, 0x7FFF, -32768, 0x0080, 0x12F0, -0x0180, 0x7F80], np.int16)


def _pair16(gc, ctx, rec, n, ch, n_ep, closed, stride=0, calls=1):
    """The int8 run, then the int16 run of the same call(s) on one context; asserts that
    the epoch records and the channel arrays are byte-equal and returns the int8 run's."""
    rec = np.ascontiguousarray(rec, np.int8)
    d8, d16 = gc.DevBuf.from_array(rec), gc.DevBuf.from_array(rec.astype(np.int16))
    assert d8.ptr % 16 == 0 and d16.ptr % 16 == 0 and stride % 16 == 0
    out = []
    for fmt, d, st in (("int8", d8, stride), ("int16", d16, 2 * stride)):
        c = ch.copy()
        ctx.set_format(fmt)
        eps = [ctx.track(d.ptr, st, n, c, n_ep, closed_loop=closed) for _ in range(calls)]
        out.append((np.concatenate(eps, axis=1), c))
    ctx.set_format("int8")
    (ea, ca), (eb, cb) = out
    for f in ea.dtype.names:
        assert ea[f].tobytes() == eb[f].tobytes(), \
            (f, np.argwhere(ea[f] != eb[f])[:4], ea[f][ea[f] != eb[f]][:4], eb[f][ea[f] != eb[f]][:4])
    assert ea.tobytes() == eb.tobytes() and ca.tobytes() == cb.tobytes()
    return ea, ca


# ---------------------------------------------------------------- 1a. trackers, identity
@functools.lru_cache(maxsize=None)
def _b1i_long():
    IF = np.asarray(B.scene(n_ms=12)[0])
    assert np.abs(IF).max() <= 127
    return IF.astype(np.int8)


def _long_record(gc, system, file_type):
    """12 ms (12.5 ms for GPS / GLONASS noise): room for 8 epochs from any start."""
    if system == 2:
        return _b1i_long() if file_type == 2 else _b1i_long()[0::2].copy()
    return _sgt_record(gc, system, file_type, n=200000)


@pytest.mark.parametrize("chunk", ["1", "0"])
@pytest.mark.parametrize("threads", [None, "64", "1024"])
@pytest.mark.parametrize("system,file_type,switch",
                         [(0, 2, 0), (1, 2, 0), (1, 1, 0), (0, 1, 0), (2, 2, 0), (2, 1, 0),
                          (1, 2, 1)])
def test_sgt_identity_every_shape(gpu, system, file_type, switch, threads, chunk, monkeypatch):
    """16 Msps, 4 channels x 8 epochs in two calls (the second continues the first), open
    and closed loop: run_chips (GPS kC 16, GLONASS kC 32; 256 threads and the wave shape),
    run_chunks (1024 threads; B1I wave shape kC 8), the per-sample pass
    (GNSSCORR_SGT_CHUNK=0; B1I elsewhere); file_type 1 and 2, GLONASS with switchIQ."""
    gc = gpu
    monkeypatch.setenv("GNSSCORR_SGT_CHUNK", chunk)
    if threads:
        monkeypatch.setenv("GNSSCORR_SGT_THREADS", threads)
    rec = _long_record(gc, system, file_type)
    n = len(rec) // file_type
    ctx = gc.SgtCtx(system, fileType=file_type, switchIQ=switch, samplingFreq=FS)
    ch = _sgt_chans(gc, np.random.default_rng(7 + system + 3 * file_type), system, FS,
                    n - int(5.2e-3 * FS), offs=OFFS)
    for closed in (False, True):
        _ran(_pair16(gc, ctx, rec, n, ch, 4, closed, calls=2)[0])


@pytest.mark.parametrize("threads", [None, "64"])
@pytest.mark.parametrize("system,file_type", [(0, 2), (1, 2), (1, 1)])
def test_sgt_identity_chunk_grid(gpu, system, file_type, threads, monkeypatch):
    """dllCorrelatorSpacing = 0.5: run_chunks (prefix columns at 256 threads, the code
    select in the wave shape), kC 16 (GPS) and 32 (GLONASS)."""
    gc = gpu
    if threads:
        monkeypatch.setenv("GNSSCORR_SGT_THREADS", threads)
    rec = _sgt_record(gc, system, file_type)
    n = len(rec) // file_type
    ctx = gc.SgtCtx(system, fileType=file_type, samplingFreq=FS, dllCorrelatorSpacing=0.5)
    ch = _sgt_chans(gc, np.random.default_rng(29 + system + 3 * file_type), system, FS, n,
                    offs=OFFS)
    _ran(_pair16(gc, ctx, rec, n, ch, 2, False)[0])


@pytest.mark.parametrize("threads", [None, "64"])
@pytest.mark.parametrize("system,file_type", [(0, 2), (1, 2), (0, 1), (1, 1)])
def test_sgt_identity_odd_chip_forms(gpu, system, file_type, threads, monkeypatch):
    """16.368 Msps: run_chips with kC 17 and 33."""
    gc = gpu
    fs = 16.368e6
    if threads:
        monkeypatch.setenv("GNSSCORR_SGT_THREADS", threads)
    rec = _sgt_record(gc, system, file_type, fs)
    n = len(rec) // file_type
    ctx = gc.SgtCtx(system, fileType=file_type, samplingFreq=fs)
    ch = _sgt_chans(gc, np.random.default_rng(31 + system + 3 * file_type), system, fs, n,
                    offs=OFFS)
    _ran(_pair16(gc, ctx, rec, n, ch, 2, False)[0])


def test_sgt_identity_two_streams_closed_loop(gpu):
    """Two records (streams) with a non-zero stride, 2 GPS channels each."""
    gc = gpu
    n = 80000
    stride = 2 * n + 48                       # bytes of the int8 record; the int16 one twice
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
    ep, _ = _pair16(gc, ctx, buf, n, ch, 3, True, stride=stride)
    _ran(ep)
    assert (ep["I_P"][:2] != ep["I_P"][2:]).all()


def test_sgt_identity_many_channels_one_wave_each(gpu):
    gc = gpu
    IF, fchs, starts, acq = _glonass_scene(gc, 4)
    ctx = gc.SgtCtx(1)
    big = np.tile(ctx.init_chans(fchs, starts, acq), 80)      # 1120 channels
    _ran(_pair16(gc, ctx, IF, len(IF) // 2, big, 1, True)[0])


@pytest.mark.parametrize("chunk", ["1", "0"])
@pytest.mark.parametrize("threads", [None, "64"])
@pytest.mark.parametrize("file_type", [2, 1])
@pytest.mark.parametrize("mode", list(E1_MODES))
def test_e1t_identity_every_mode(gpu, mode, file_type, threads, chunk, monkeypatch):
    """The four loop modes, IQ and real records, both launch shapes, the 16-sample chunks
    and the per-sample path (GNSSCORR_E1T_CHUNK=0); open and closed loop; 4 channels x 8
    epochs (4 ms modes: 2) in two calls, pos mod 32 in 0, 1, 7, 31."""
    gc = gpu
    monkeypatch.setenv("GNSSCORR_E1T_CHUNK", chunk)
    if threads:
        monkeypatch.setenv("GNSSCORR_E1T_THREADS", threads)
    rec, codes, _ = _e1b_record(file_type)
    n = len(rec) // file_type
    ctx = gc.E1tCtx(fileType=file_type, **E1_MODES[mode])
    ctx.set_codes(codes)
    ms4 = mode in ("4ms", "amb4")
    ch = _e1t_chans(gc, ctx, np.random.default_rng(11 + file_type), n - int(8e-3 * FS), mode)
    for closed in (False, True):
        _ran(_pair16(gc, ctx, rec, n, ch, 1 if ms4 else 4, closed, calls=2)[0])


def test_e1t_identity_low_rate_per_sample_path(gpu):
    """4.096 Msps: 15 * cstep >= 1, so the per-sample path is taken."""
    gc = gpu
    fs = 4.096e6
    rec, codes, chans = E.closed_loop_scene(fs)
    ctx = gc.E1tCtx(samplingFreq=fs)
    ctx.set_codes(codes)
    ch = ctx.init_chans([c[0] for c in chans] + [0], [c[1] for c in chans] + [chans[0][1] + 7],
                        [c[2] for c in chans] + [chans[0][2]])
    assert 15 * ch["code_freq"][0] / fs >= 1.0
    _ran(_pair16(gc, ctx, rec, len(rec) // 2, ch, 2, True)[0])


@pytest.mark.parametrize("threads", [None, "64"])
@pytest.mark.parametrize("switch_iq", [0, 1])
def test_l3t_identity(gpu, switch_iq, threads, monkeypatch):
    gc = gpu
    if threads:
        monkeypatch.setenv("GNSSCORR_L3T_THREADS", threads)
    rec, prn, cp, f0 = _l3_record()
    ctx = gc.L3tCtx(switchIQ=switch_iq)
    ch = ctx.init_chans([prn] * 4, [cp, cp + 24000 + 1, cp + 5, cp + 48000 + 31], [f0] * 4)
    for closed in (False, True):
        _ran(_pair16(gc, ctx, rec, len(rec) // 2, ch, 1, closed, calls=2)[0])


def _two_streams(rec, n, shift):
    """Two records of n I,Q samples in one int8 buffer: samples [0, n) and [shift, shift +
    n) of rec, the second at a stride that is no multiple of 32 bytes."""
    stride = 2 * n + 48
    buf = np.ones(2 * stride, np.int8)
    buf[:2 * n] = rec[:2 * n]
    buf[stride:stride + 2 * n] = rec[2 * shift:2 * (shift + n)]
    return buf, stride


@pytest.mark.parametrize("chunk", ["1", "0"])
def test_e1t_identity_two_streams(gpu, chunk, monkeypatch):
    """Channels 2, 3 are channels 0, 1 on the other stream: the int16 stride is twice the
    int8 one, in the 16-sample chunks and in the per-sample path."""
    gc = gpu
    monkeypatch.setenv("GNSSCORR_E1T_CHUNK", chunk)
    rec, codes, _ = _e1b_record(2)
    n = 200000
    buf, stride = _two_streams(rec, n, 100003)
    ctx = gc.E1tCtx()
    ctx.set_codes(codes)
    two = _e1t_chans(gc, ctx, np.random.default_rng(71), n - int(4e-3 * FS), "5arm", offs=(1, 30))
    ch = np.concatenate([two, two])
    ch["stream"] = [0, 0, 1, 1]
    ep, _ = _pair16(gc, ctx, buf, n, ch, 3, True, stride=stride)
    _ran(ep)
    assert (ep["I_P_P"][:2] != ep["I_P_P"][2:]).all()


def test_l3t_identity_two_streams(gpu):
    gc = gpu
    rec, prn, cp, f0 = _l3_record()
    n = 200000
    buf, stride = _two_streams(rec, n, 60001)
    ctx = gc.L3tCtx()
    two = ctx.init_chans([prn] * 2, [cp, cp + 24000 + 7], [f0] * 2)
    ch = np.concatenate([two, two])
    ch["stream"] = [0, 0, 1, 1]
    ep, _ = _pair16(gc, ctx, buf, n, ch, 2, True, stride=stride)
    _ran(ep)
    assert (ep[ep.dtype.names[1]][:2] != ep[ep.dtype.names[1]][2:]).all()


# ---------------------------------------------------------------- 1b. the record's end
def _end_case16(gc, ctx, rec, bps, ch):
    """Channel 0's second epoch ends on the record's last sample and the int16 record on
    the last byte of its allocation: two epochs equal to int8's, the third stops with
    status 1 and the int8 run's record."""
    full = len(rec) // bps
    ch[:] = ch[np.argsort(-ch["pos"], kind="stable")]     # the latest channel first
    assert ch["pos"][0] - ch["pos"][1:].max() >= 16
    d8 = gc.DevBuf.from_array(rec)
    ctx.set_format("int8")
    blk = ctx.track(d8.ptr, 0, full, ch.copy(), 2, closed_loop=False)["blksize"][0]
    n = int(ch["pos"][0] + blk.sum())
    if n % 8 == 0:                      # an end inside a 16-byte word of the int16 record
        ch["pos"][0] += 1
        n += 1
    assert n + 64 < full
    d16 = gc.DevBuf.from_array(rec[:bps * n].astype(np.int16))
    assert d16.nbytes == 2 * bps * n and d16.ptr % 16 == 0
    ca, cb = ch.copy(), ch.copy()
    ea = ctx.track(d8.ptr, 0, n, ca, 3, closed_loop=False)
    ctx.set_format("int16")
    eb = ctx.track(d16.ptr, 0, n, cb, 3, closed_loop=False)
    ctx.set_format("int8")
    assert ea.tobytes() == eb.tobytes() and ca.tobytes() == cb.tobytes()
    assert (eb["status"][0] == [0, 0, 1]).all() and cb["status"][0] == 1
    assert cb["pos"][0] == n and eb["blksize"][0][2] > 0
    assert (eb["status"][1:, :2] == 0).all()


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
    _end_case16(gc, ctx, rec, file_type, ch)


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
    _end_case16(gc, ctx, rec, file_type, ch)


def test_l3t_record_end(gpu):
    gc = gpu
    rec, prn, cp, f0 = _l3_record()
    ctx = gc.L3tCtx()
    ch = ctx.init_chans([prn, prn], [cp + 65, cp], [f0, f0])
    _end_case16(gc, ctx, rec, 2, ch)


# ---------------------------------------------------------------- 1c. search, identity
ENGINES = {"headline-16368": (16.368e6, 16368), "generic-2048": (2.048e6, 2048),
           "generic-4096": (4.096e6, 4096)}


@functools.lru_cache(maxsize=None)
def _search_scene(engine):
    """2 codes x 3 bins; records of 4 blocks (2 blocks x 2 coherent ms, or 2 records x 2)."""
    fs, n = ENGINES[engine]
    import gnsscorr as gc
    sigs = [dict(system=0, prn=7, code_phase=100.25, doppler=500.0, cn0=50.0)]
    IF = gc.ifgen(4 * n, sigs, fs=fs, seed=0x16 + n)
    codes = np.stack([A.make_ca_table_row(p, fs) for p in (7, 9)])
    assert codes.shape[1] == n
    return IF, codes, 2.42e6 + np.array([0.0, 500.0, 1000.0]), np.tile(np.arange(3), (2, 1))


def _both(ctx_of, run):
    """run(ctx, record, iq flags) on the int8 record and on its int16 copy, each on a
    context of its own: byte-equal results."""
    import gnsscorr as gc
    out = []
    for int16 in (False, True):
        ctx = ctx_of()
        conv = (lambda r: np.asarray(r, np.int8).astype(np.int16)) if int16 else (lambda r: r)
        out.append(run(ctx, conv, gc.iq_flags(True, int16=int16)))
        ctx.close()
    for a, b in zip(out[0], out[1]):
        assert a.tobytes() == b.tobytes()
    return out[0]


@pytest.mark.parametrize("engine", list(ENGINES))
def test_search_identity_plain_modes(gpu, engine):
    """Best-of-blocks, non-coherent, set_coherent(2), set_records(2), set_group_records
    (the compiled plan only: the generic engine has none) and power_row: every row and result byte-equal to the int8 search."""
    gc = gpu
    fs, n = ENGINES[engine]
    IF, codes, freqs, gf = _search_scene(engine)
    spc = max(2, int(round(fs / 1.023e6)))

    def ctx_of():
        ctx = gc.AcqCtx(fs, n, max_freqs=4, max_blocks=4, max_codes=2)
        ctx.set_codes(codes)
        return ctx

    def run(ctx, conv, iq):
        got = []
        for mode in (gc.ACQ_BEST_OF_BLOCKS, gc.ACQ_NONCOHERENT):
            got += ctx.search(conv(IF[:4 * n]), 2, freqs, [0, 1], gf, spc=spc, iq=iq, mode=mode)
        ctx.set_coherent(2)
        got += ctx.search(conv(IF), 2, freqs, [0, 1], gf, spc=spc, iq=iq)
        ctx.set_coherent(1)
        ctx.set_records(2)
        got += ctx.search(conv(IF), 2, freqs, [0, 1], gf, spc=spc, iq=iq)
        if engine.startswith("headline"):       # per-group records need a compiled plan
            d_rec = gc.DevBuf.from_array(np.array([1, 0], np.int32))
            ctx.set_group_records(d_rec)
            got += ctx.search(conv(IF), 2, freqs, [0, 1], gf, spc=spc, iq=iq)
            ctx.set_group_records(None)
        ctx.set_records(1)
        got.append(ctx.power_row(conv(IF[:4 * n]), 2, 1, freqs[1], 0, iq=iq))
        return got

    got = _both(ctx_of, run)
    res, rows = got[0], got[1]
    assert res[0]["bin"] == 1 and res[0]["metric"] > 2.5
    assert int(np.argmax(got[-1])) == rows[0, 1]["argmax"]


@pytest.mark.parametrize("engine", ["generic-2048", "generic-4096"])
def test_search_identity_zero_padded_and_concat(gpu, engine):
    """A zero-padded search (blocks end to end, then overlapping with a block stride) and
    GNSSCORR_ACQ_CONCAT with stride == keep."""
    gc = gpu
    fs, n = ENGINES[engine]
    keep = n // 2
    codes = np.random.default_rng(n).choice(np.array([-1, 1], np.int8), (2, keep))
    freqs = 0.4e6 + 250.0 * np.arange(3)
    gf = np.tile(np.arange(3), (2, 1))
    parts = [(codes[0], 3.0, 37, freqs[1]), (codes[1], 3.5, n + keep - 3, freqs[2])]
    IF = E1B.synth_if(2 * n, parts, fs, noise=3.0, seed=n)

    def ctx_of():
        ctx = gc.AcqCtx(fs, n, max_freqs=4, max_blocks=4, max_codes=2)
        ctx.set_zero_padded(keep)
        ctx.set_codes_padded(codes)
        return ctx

    def run(ctx, conv, iq):
        got = []
        for mode in (gc.ACQ_BEST_OF_BLOCKS, gc.ACQ_NONCOHERENT):
            got += ctx.search(conv(IF), 2, freqs, [0, 1], gf, spc=4, iq=iq, mode=mode)
        ctx.set_block_stride(keep)
        rec = IF[:2 * (2 * keep + n)]                    # 3 blocks at stride keep
        for mode in (gc.ACQ_BEST_OF_BLOCKS, gc.ACQ_CONCAT):
            got += ctx.search(conv(rec), 3, freqs, [0, 1], gf, spc=4, iq=iq, mode=mode)
        return got

    got = _both(ctx_of, run)
    assert got[0][0]["code_phase"] == 38 and got[0][0]["bin"] == 1


def test_search_dev_reads_a_device_int16_record(gpu):
    """search_dev on an int16 device record equals the host search of the same record."""
    gc = gpu
    fs, n = ENGINES["generic-2048"]
    IF, codes, freqs, gf = _search_scene("generic-2048")
    rec = IF[:4 * n].astype(np.int16)
    ctx = gc.AcqCtx(fs, n, max_freqs=4, max_blocks=4, max_codes=2)
    ctx.set_codes(codes)
    iq = gc.iq_flags(True, int16=True)
    res, rows = ctx.search(rec, 2, freqs, [0, 1], gf, spc=2, iq=iq)
    d = [gc.DevBuf.from_array(a) for a in (rec, freqs, np.array([0, 1], np.int32),
                                           gf.astype(np.int32))]
    d_rows, d_res = gc.DevBuf(6 * gc.ACQ_ROW.itemsize), gc.DevBuf(2 * gc.ACQ_RESULT.itemsize)
    ctx.search_dev(d[0].ptr, 2, 3, d[1].ptr, 2, 3, d[2].ptr, d[3].ptr, d_rows.ptr, d_res.ptr,
                   spc=2, iq=iq)
    ctx.sync()
    assert d_rows.download(gc.ACQ_ROW).tobytes() == rows.tobytes()
    assert d_res.download(gc.ACQ_RESULT).tobytes() == res.tobytes()


# ---------------------------------------------------------------- 2. the whole int16 range
def _full_range(rec8, bps):
    """int8-range levels scaled so that the largest reaches the int16 range, PLANT written
    over sample-aligned elements inside the first epochs."""
    x = np.asarray(rec8, np.int32)
    k = 32767 // int(np.abs(x).max())
    out = (x * k).astype(np.int16)
    at = 40000 * bps + 2 * np.arange(len(PLANT)) * 257
    out[at] = PLANT
    out[at + 1] = PLANT[::-1]
    assert out.max() == 32767 and out.min() == -32768
    return out


def test_e1t_full_range_against_the_restatement(gpu):
    """Default mode, closed loop, the closed-loop scene scaled to the int16 range, against
    e1t_scenarios.track on the int16 array (the bound of
    test_closed_loop_three_prns_40_ms: tracker_checks.close, 1e-6 relative + 1e-6)."""
    gc = gpu
    IF, codes, chans = E.closed_loop_scene()
    rec = _full_range(IF, 2)
    s, n_ep = E.settings(), 3
    refs = [E.track(rec, s, codes[row], cp, f0, n_ep) for row, cp, f0, _ in chans]
    # decidable at this scale: blksize unchanged under a 1e-9 perturbation of the sums
    pat = 1e-9 * np.array([1, -1, 1, -1, 1, -1, 1, -1, 1, -1.0])
    for (row, cp, f0, _), r in zip(chans, refs):
        for p in (pat, -pat):
            rr = E.track(rec, s, codes[row], cp, f0, n_ep, perturb=p)
            assert np.array_equal(rr["blksize"], r["blksize"])
    ctx = gc.E1tCtx()
    ctx.set_codes(codes)
    ch = ctx.init_chans([c[0] for c in chans], [c[1] for c in chans], [c[2] for c in chans])
    ctx.set_format("int16")
    d = gc.DevBuf.from_array(rec)
    ep = ctx.track(d.ptr, 0, len(rec) // 2, ch, n_ep, closed_loop=True)
    for i, r in enumerate(refs):
        assert (ep["status"][i] == 0).all() and (ep["blksize"][i] == r["blksize"]).all()
        assert (ep["segment"][i] == r["segment"]).all()
        for f in E.FIELDS:
            print(f"[e1t int16] ch {i} {f}: max rel "
                  f"{np.max(np.abs(ep[f][i] - r[f]) / (np.abs(r[f]) + 1e-300)):.3e}")
            assert _close(ep[f][i], r[f]).all(), (i, f, ep[f][i], r[f])


def test_l3t_full_range_against_the_restatement(gpu):
    """Closed loop against l3_scenarios.track on the int16 array (LOOP_TOL of
    tests/test_l3_gpu.py, 1e-7)."""
    gc = gpu
    IF, prn, cp, f0, _ = L3.closed_loop_scene()
    rec = _full_range(IF, 2)
    s, n_ep = L3.settings(), 3
    r = L3.track(rec, s, prn, cp, f0, n_ep)
    pat = 1e-9 * np.array([1, -1] * 6, np.float64)
    for p in (pat, -pat):
        assert np.array_equal(L3.track(rec, s, prn, cp, f0, n_ep, perturb=p)["blksize"],
                              r["blksize"])
    ctx = gc.L3tCtx()
    ch = ctx.init_chans([prn], [cp], [f0])
    ctx.set_format("int16")
    d = gc.DevBuf.from_array(rec)
    ep = ctx.track(d.ptr, 0, len(rec) // 2, ch, n_ep, closed_loop=True)
    assert (ep["status"][0] == 0).all() and (ep["blksize"][0] == r["blksize"]).all()
    for f in L3.FIELDS:
        assert _close(ep[f][0], r[f], 1e-7, 1e-7).all(), (f, ep[f][0], r[f])


def _sgt_track_perturbed(IF, s, code_id, code_phase_1b, acquired_freq, n_ms, perturb):
    """sgt_oracle.track with every epoch's six sums scaled by 1 + perturb before the loop
    filters (the oracle's own loop driver, which the e1t and l3t restatements call with
    their perturb argument)."""
    code_pad = S.padded_code(s["system"], code_id)
    lp = S.Loop(s, code_id, code_phase_1b - 1, acquired_freq)
    return S.T.track(lp, S.FIELDS, n_ms, lambda lp: S.epoch(IF, s, code_pad, lp), perturb)[0]


def test_sgt_full_range_against_the_oracle(gpu):
    """GLONASS closed loop on the scaled scene against oracle/sgt_oracle.py on the int16
    array (the bound of test_config4_glonass_14_fch_closed_loop: 1e-6 relative + 1e-6)."""
    gc = gpu
    IF, fchs, starts, acq = _glonass_scene(gc, 4)
    rec = _full_range(IF, 2)
    s = S.settings(1)
    refs = [S.track(rec, s, int(fchs[i]), starts[i], float(acq[i]), 3) for i in range(4)]
    # decidable at this scale: blksize unchanged under a 1e-9 perturbation of the sums
    pat = 1e-9 * np.array([1, -1, 1, -1, 1, -1.0])
    for i, r in enumerate(refs):
        for p in (pat, -pat):
            rr = _sgt_track_perturbed(rec, s, int(fchs[i]), starts[i], float(acq[i]), 3, p)
            assert np.array_equal(rr["blksize"], r["blksize"])
    assert np.array_equal(_sgt_track_perturbed(rec, s, int(fchs[0]), starts[0], float(acq[0]),
                                               3, None)["I_P"], refs[0]["I_P"])
    ctx = gc.SgtCtx(1)
    ch = ctx.init_chans(fchs[:4], starts[:4], acq[:4])
    ctx.set_format("int16")
    d = gc.DevBuf.from_array(rec)
    ep = ctx.track(d.ptr, 0, len(rec) // 2, ch, 3, closed_loop=True)
    for i, r in enumerate(refs):
        assert (ep["status"][i] == 0).all() and (ep["blksize"][i] == r["blksize"]).all()
        for f in S.FIELDS:
            assert _close(ep[f][i], r[f], rtol=1e-6, atol=1e-6).all(), (i, f, ep[f][i], r[f])


@pytest.mark.parametrize("engine", ["headline-16368", "generic-2048"])
def test_search_full_range_against_the_oracle(gpu, engine):
    """oracle/acq_oracle.py fed the int16 array; test_acq_gpu.check_rows' fp64 bar (1e-6
    relative, argmax / bin / code phase exact).  Peak and second peak are separated in the
    oracle itself."""
    from test_acq_gpu import check_rows
    gc = gpu
    fs, n = ENGINES[engine]
    IF, codes, freqs, gf = _search_scene(engine)
    x = IF[:4 * n].astype(np.int32)
    rec = (x * (32767 // int(np.abs(x).max()))).astype(np.int16)
    rec[2 * 300: 2 * 300 + len(PLANT)] = PLANT
    rec[2 * n + 2 * 301: 2 * n + 2 * 301 + len(PLANT)] = PLANT[::-1]
    spc = max(2, int(round(fs / 1.023e6)))
    ref, ref_rows = A.acquire(rec, fs, codes, freqs, gf, spc=spc, n_blocks=2, return_rows=True)
    assert ref[0]["peak"] > 1.5 * ref[0]["second"] and ref[0]["bin"] == 1
    ctx = gc.AcqCtx(fs, n, max_freqs=4, max_blocks=2, max_codes=2)
    ctx.set_codes(codes)
    res, rows = ctx.search(rec, 2, freqs, [0, 1], gf, spc=spc, iq=gc.iq_flags(True, int16=True))
    check_rows(res, rows, ref, ref_rows, True, label=f"int16-{engine}")


# ---------------------------------------------------------------- 2b. the pipeline joins
GN3S_FIN = 4.0e6                                    # 20000 real samples per 5-ms block
PIPE = dict(prn=11, chips0=300.4, doppler=1000.0, IF=40e3, fs=2.048e6, n=2048, blocks=3)


def _gn3s_stream():
    """3 blocks of 2-bit GN3S codes, one per byte: one C/A signal (PRN 11, 300.4 chips into
    its code at sample 0, +1 kHz Doppler) on a real carrier IF + Doppler below the front
    end's NCO frequency, so that Read_GN3S leaves it as exp(-i 2 pi (IF + Doppler) t), the
    sign the receivers' wipe-off stops; unit-variance noise; thresholds -1, 0, 1."""
    n = PIPE["blocks"] * 20000
    t = np.arange(n) / GN3S_FIN
    f_nco = 2557223528 / 2.0 ** 32 * GN3S_FIN           # GN3S_STEP cycles per sample
    ca = A.generate_ca_code(PIPE["prn"]).astype(np.float64)
    chips = (PIPE["chips0"] + t * 1.023e6 * (1 + PIPE["doppler"] / 1575.42e6)) % 1023
    x = ca[chips.astype(np.int64)] * np.cos(
        2 * np.pi * (f_nco - PIPE["IF"] - PIPE["doppler"]) * t + 0.7)
    x += np.random.default_rng(5).standard_normal(n)
    return np.digitize(x, [-1.0, 0.0, 1.0]).astype(np.uint8)


def test_front_end_output_feeds_the_search_and_the_tracker_on_the_device(gpu, oracle):
    """GN3S bytes -> SdrFeCtx.gn3s_dev -> its int16 device buffer, with no host copy, to
    AcqCtx(2.048e6, 2048) under IF_IQ | IF_INT16 and to SgtCtx(0, 2.048 Msps) in format 2.
    Expected: the CPU chain sdr_oracle gn3s (bit-exact) -> acq_oracle (check_rows' fp64
    bar) -> sgt_oracle (1e-6 relative + 1e-6, the sgt bound); the planted PRN, code phase
    and Doppler bin come out."""
    import sdr_oracle as SO
    from test_acq_gpu import check_rows
    gc = gpu
    fs, n, prn = PIPE["fs"], PIPE["n"], PIPE["prn"]
    raw = _gn3s_stream()
    # --- the CPU chain
    want16, want_ph = SO.OracleSDR().gn3s(raw)
    rec = want16.reshape(-1)                           # int16 I,Q, 3 x 10240 samples
    codes = np.stack([A.make_ca_table_row(p, fs) for p in (prn, 20)])
    freqs = PIPE["IF"] + 500.0 * np.arange(-2, 5)
    gf = np.tile(np.arange(len(freqs)), (2, 1))
    ref, ref_rows = A.acquire(rec[:2 * 2 * n], fs, codes, freqs, gf, spc=2, n_blocks=2,
                              return_rows=True)
    start = (1023 - PIPE["chips0"]) / 1.023e6 * fs + 1
    assert abs(ref[0]["code_phase"] - start) <= 2.0 and ref[0]["bin"] == 4
    assert ref[0]["peak"] > 4 * ref[0]["second"] and ref[0]["metric"] > 10 * ref[1]["metric"]
    s = S.settings(0, samplingFreq=fs, IF=PIPE["IF"])
    n_ep = 5
    r = S.track(rec, s, prn, int(ref[0]["code_phase"]), float(ref[0]["carr_freq"]), n_ep)
    pat = 1e-9 * np.array([1, -1, 1, -1, 1, -1.0])
    for p in (pat, -pat):
        assert np.array_equal(_sgt_track_perturbed(rec, s, prn, int(ref[0]["code_phase"]),
                                                   float(ref[0]["carr_freq"]), n_ep,
                                                   p)["blksize"], r["blksize"])
    # --- the GPU chain on one device buffer
    fe = gc.SdrFeCtx()
    d_in = gc.DevBuf.from_array(gc.pack_2bit(raw))
    n_out = PIPE["blocks"] * gc.GN3S_BLOCK_OUT
    d_cpx = gc.DevBuf(n_out * 4)
    assert d_cpx.ptr % 16 == 0
    assert fe.gn3s_dev(d_in.ptr, True, PIPE["blocks"], 0, d_cpx.ptr) == want_ph
    fe.sync()
    acq = gc.AcqCtx(fs, n, max_freqs=8, max_blocks=2, max_codes=2)
    acq.set_codes(codes)
    d = [gc.DevBuf.from_array(a) for a in (freqs, np.arange(2, dtype=np.int32),
                                           gf.astype(np.int32))]
    d_rows = gc.DevBuf(gf.size * gc.ACQ_ROW.itemsize)
    d_res = gc.DevBuf(2 * gc.ACQ_RESULT.itemsize)
    acq.search_dev(d_cpx.ptr, 2, len(freqs), d[0].ptr, 2, len(freqs), d[1].ptr, d[2].ptr,
                   d_rows.ptr, d_res.ptr, spc=2, iq=gc.iq_flags(True, int16=True))
    acq.sync()
    res = d_res.download(gc.ACQ_RESULT)
    rows = d_rows.download(gc.ACQ_ROW).reshape(gf.shape)
    check_rows(res, rows, ref, ref_rows, True, label="pipeline-int16")
    assert res[0]["bin"] == 4 and abs(float(res[0]["code_phase"]) - start) <= 2.0
    assert res[0]["carr_freq"] == PIPE["IF"] + PIPE["doppler"]
    trk = gc.SgtCtx(0, samplingFreq=fs, IF=PIPE["IF"])
    ch = trk.init_chans([prn], res["code_phase"][:1], res["carr_freq"][:1])
    trk.set_format("int16")
    ep = trk.track(d_cpx.ptr, 0, n_out, ch, n_ep, closed_loop=True)
    assert np.array_equal(d_cpx.download(np.int16), rec)      # the buffer the chain read
    assert (ep["status"][0] == 0).all() and (ep["blksize"][0] == r["blksize"]).all()
    for f in S.FIELDS:
        assert _close(ep[f][0], r[f], rtol=1e-6, atol=1e-6).all(), (f, ep[f][0], r[f])


# ---------------------------------------------------------------- 3. arguments
def _ctxs(gc):
    e = gc.E1tCtx()
    e.set_codes(_e1b_record(2)[1])
    return [gc.SgtCtx(0), e, gc.L3tCtx()]


def test_set_record_format_values_and_set_packed_are_interchangeable(gpu):
    gc = gpu
    for ctx in _ctxs(gc):
        fn = getattr(gc.lib(), ctx._prefix + "_set_record_format")
        for bad in (3, -1):
            assert fn(ctx.h, bad) == -1                               # GNSSCORR_EINVAL
            assert b"set_record_format" in gc.lib().gnsscorr_last_error()
        with pytest.raises(ValueError):
            ctx.set_format("int32")
    rec = _sgt_record(gc, 0, 2)                                       # four levels
    n = len(rec) // 2
    ctx = gc.SgtCtx(0, samplingFreq=FS)
    ch = _sgt_chans(gc, np.random.default_rng(61), 0, FS, n, offs=OFFS)
    dp = gc.DevBuf.from_array(gc.pack2(rec))
    out = []
    for select in (lambda: ctx.set_packed(True), lambda: ctx.set_format("packed2")):
        ctx.set_format("int16")
        select()
        c = ch.copy()
        out.append((ctx.track(dp.ptr, 0, n, c, 2, closed_loop=False), c))
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
    # and set_packed(0) leaves format 2
    ctx.set_format("int16")
    ctx.set_packed(False)
    d8 = gc.DevBuf.from_array(rec)
    c = ch.copy()
    ep = ctx.track(d8.ptr + 2, 24, n - 1, c, 1, closed_loop=False)    # fine for int8 only
    _ran(ep)


def test_int16_alignment_is_checked_before_any_launch(gpu):
    gc = gpu
    d = gc.DevBuf(1 << 20)
    for ctx in _ctxs(gc):
        ch = np.zeros(1, ctx._CHAN)
        ch["code_id"] = 1
        ch["code_freq"] = ctx.cfg.code_freq_basis
        ctx.set_format("int16")
        for ptr, stride in ((d.ptr, 24), (d.ptr + 4, 0), (d.ptr + 8, 64)):
            c = ch.copy()
            ep = np.zeros((1, 1), ctx._EPOCH)
            rc = ctx._track(ctx.h, ptr, stride, 1000, 1, c.ctypes.data, 1, 0, ep.ctypes.data)
            assert rc == -1 and b"16" in gc.lib().gnsscorr_last_error()
            assert c.tobytes() == ch.tobytes()                        # nothing ran


def test_acq_refuses_int16_with_packed_on_f32_and_misaligned(gpu):
    gc = gpu
    fs, n = 16.368e6, 16368
    IF = np.ones(4 * n, np.int16)
    codes = np.ones((1, n), np.int8)
    f64 = gc.AcqCtx(fs, n, max_freqs=2, max_blocks=2, max_codes=1)
    f64.set_codes(codes)
    with pytest.raises(gc.GnssCorrError, match="exclude"):
        f64.search(IF, 1, [2.42e6], [0], [[0]], iq=gc.IF_IQ | gc.IF_INT16 | gc.IF_PACKED2)
    d = gc.DevBuf.from_array(IF)
    d_f = gc.DevBuf.from_array(np.array([2.42e6]))
    with pytest.raises(gc.GnssCorrError, match="4-byte aligned"):
        f64.spectra_dev(d.ptr + 2, 1, 1, d_f.ptr, iq=gc.IF_IQ | gc.IF_INT16)
    with pytest.raises(gc.GnssCorrError, match="2-byte aligned"):
        f64.spectra_dev(d.ptr + 1, 1, 1, d_f.ptr, iq=gc.IF_INT16)
    f64.spectra_dev(d.ptr + 2, 1, 1, d_f.ptr, iq=gc.IF_INT16)          # real: 2 bytes suffice
    f64.sync()
    f32 = gc.AcqCtx(fs, n, max_freqs=2, max_blocks=2, max_codes=1, precision=gc.ACQ_F32)
    f32.set_codes(codes)
    with pytest.raises(gc.GnssCorrError, match="GNSSCORR_ACQ_F64"):
        f32.search(IF, 1, [2.42e6], [0], [[0]], iq=gc.IF_IQ | gc.IF_INT16)
    with pytest.raises(gc.GnssCorrError, match="GNSSCORR_ACQ_F64"):
        f32.power_row(IF, 1, 0, 2.42e6, 0, iq=gc.IF_IQ | gc.IF_INT16)
