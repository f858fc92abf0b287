"""What the float trackers' timing tools share (e1t_time.py, l3t_time.py, b1i_time.py):
the record and channel set-up, the timed track_dev loop and the report under the op model.

N channels x E epochs, closed loop, device-resident (track_dev), HIP events on each
context's stream, on a seeded noise record long enough for every channel; the channel
state is uploaded again before every launch, so each launch does the same work.
`--runs` timed launches after `--warmup` untimed ones give min / median / max.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "gnss-sdr.ru_amd"))
import gnsscorr as gc  # noqa: E402

PEAK = 78.6e12      # fp64 FLOP/s, an FMA as two
GPS_OPS = 27        # fp64 operations per sample of the GPS L1 C/A tracker


def add_args(ap, fs):
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--fs", type=float, default=fs)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)


def setup(a, tool, file_type=2):
    """(rng, n, d_if, starts, dops): the seeded generator the tool goes on drawing its
    code ids from, the record of n samples on the device, and each channel's 1-based start
    and Doppler."""
    if gc.device_count() < 1:
        raise SystemExit(f"{tool}: no HIP device visible")
    rng = np.random.default_rng(1)
    n = int(a.fs * (a.epochs + 4) / 1000)
    d_if = gc.DevBuf.from_array(gc.ifgen(n, [], fs=a.fs, iq=file_type == 2, seed=5))
    starts = rng.integers(1, int(a.fs * 0.002), a.channels)
    dops = rng.uniform(-4000, 4000, a.channels)
    return rng, n, d_if, starts, dops


def time_ctx(ctx, chans, dtype_ep, d_if, n, epochs, warmup, runs):
    C = len(chans)
    d_ch = gc.DevBuf.from_array(chans)
    d_ep = gc.DevBuf(dtype_ep.itemsize * C * epochs)
    e0, e1 = gc.Event(), gc.Event()
    out = []
    for r in range(warmup + runs):
        d_ch.upload(chans)
        e0.record(ctx.stream)
        ctx.track_dev(d_if.ptr, 0, n, C, d_ch.ptr, epochs, d_ep.ptr, closed_loop=True)
        e1.record(ctx.stream)
        ctx.sync()
        if r >= warmup:
            out.append(e0.elapsed_ms(e1))
    ep = d_ep.download(dtype_ep)
    assert (ep["status"] == 0).all(), "a channel stopped: the record is too short"
    return out, int(ep["blksize"].astype(np.int64).sum())


def report(ops, ms, samples, C, epochs):
    med = float(np.median(ms))
    return dict(ms=[round(x, 4) for x in ms], min=round(min(ms), 4), median=round(med, 4),
                max=round(max(ms), 4), us_per_channel_ms=round(med * 1e3 / (C * epochs), 4),
                samples_per_s=round(samples / (med * 1e-3), 1),
                fp64_frac=round(samples * ops / (med * 1e-3) / PEAK, 4))


def time_tracker(a, ctx, chans, dtype_ep, ops, d_if, n):
    ms, samples = time_ctx(ctx, chans, dtype_ep, d_if, n, a.epochs, a.warmup, a.runs)
    return report(ops, ms, samples, a.channels, a.epochs)


def time_gps(a, rng, starts, dops, d_if, n, file_type=2):
    """The yardstick: the GPS L1 C/A float tracker on the same record, starts and Dopplers."""
    gps = gc.SgtCtx(0, fileType=file_type, samplingFreq=a.fs)
    ch = gps.init_chans(rng.integers(1, 33, a.channels), starts, 2.42e6 + dops)
    return time_tracker(a, gps, ch, gc.SGT_EPOCH, GPS_OPS, d_if, n)
