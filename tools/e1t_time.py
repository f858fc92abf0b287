#!/usr/bin/env python3
"""Time the Galileo E1B float tracker (E1tCtx, GALILEO/E1/tracking.sci) and, as the
yardstick, the GPS L1 C/A float tracker (SgtCtx) at the same channels, epochs and rate.

N channels x E epochs, closed loop, device-resident (track_dev), HIP events on each
context's stream, on a seeded noise record long enough for every channel; the channel
state is uploaded again before every launch, so each launch does the same work.
`--runs` timed launches after `--warmup` untimed ones give min / median / max.

Reports per tracker: us per channel-ms, samples/s and the fraction of fp64 peak under
the op model (E1: 41 fp64 ops per sample, GPS: 27; peak 78.6 TFLOP/s, an FMA as two).
GNSSCORR_E1T_CHUNK=0 times the E1 per-sample path.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "gnss-sdr.ru_amd"))
import gnsscorr as gc  # noqa: E402

PEAK = 78.6e12
OPS = dict(e1t=41, sgt=27)


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


def report(name, ms, samples, C, epochs):
    med = float(np.median(ms))
    return dict(ms=[round(x, 4) for x in ms], min=round(min(ms), 4), median=round(med, 4),
                max=round(max(ms), 4), us_per_channel_ms=round(med * 1e3 / (C * epochs), 4),
                samples_per_s=round(samples / (med * 1e-3), 1),
                fp64_frac=round(samples * OPS[name] / (med * 1e-3) / PEAK, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--fs", type=float, default=16e6)
    ap.add_argument("--file-type", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    if gc.device_count() < 1:
        raise SystemExit("e1t_time: no HIP device visible")
    C, E = a.channels, a.epochs
    rng = np.random.default_rng(1)
    n = int(a.fs * (E + 4) / 1000)
    IF = gc.ifgen(n, [], fs=a.fs, iq=a.file_type == 2, seed=5)
    d_if = gc.DevBuf.from_array(IF)
    starts = rng.integers(1, int(a.fs * 0.002), C)
    dops = rng.uniform(-4000, 4000, C)

    e1 = gc.E1tCtx(fileType=a.file_type, samplingFreq=a.fs)
    codes = rng.choice(np.array([-1, 1], np.int8), (50, 4092))   # the time does not depend on the chips
    e1.set_codes(codes)
    ch = e1.init_chans(rng.integers(0, 50, C), starts, 2.42e6 + dops)
    ms, samples = time_ctx(e1, ch, gc.E1T_EPOCH, d_if, n, E, a.warmup, a.runs)
    res = dict(tool="e1t_time", channels=C, epochs=E, fs=a.fs, file_type=a.file_type,
               e1_path="per-sample" if os.environ.get("GNSSCORR_E1T_CHUNK", "1")[:1] == "0"
               else "chunked", e1t=report("e1t", ms, samples, C, E))

    gps = gc.SgtCtx(0, fileType=a.file_type, samplingFreq=a.fs)
    ch = gps.init_chans(rng.integers(1, 33, C), starts, 2.42e6 + dops)
    ms, samples = time_ctx(gps, ch, gc.SGT_EPOCH, d_if, n, E, a.warmup, a.runs)
    res["sgt_gps"] = report("sgt", ms, samples, C, E)
    res["e1t_over_sgt"] = round(res["e1t"]["median"] / res["sgt_gps"]["median"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
