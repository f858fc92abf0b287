#!/usr/bin/env python3
"""Time the BeiDou B1I float tracker (SgtCtx(2), COMPASS/B1/tracking.sci) and, as the
yardstick, the GPS L1 C/A float tracker (SgtCtx(0)) at the same channels, epochs and rate.

N channels x E epochs, closed loop, device-resident (track_dev), HIP events on each
context's stream, on a seeded noise record long enough for every channel; the channel
state is uploaded again before every launch, so each launch does the same work.
`--runs` timed launches after `--warmup` untimed ones give min / median / max.

Without --one: for each channel count (1024: one wave per channel; 14: 256-thread
workgroups; 4: 512 threads, the 1024-thread kernel) and each variant ("chunked": the
library's default path choice; "per-sample": GNSSCORR_SGT_CHUNK=0) starts `--procs` fresh
processes of itself with --one, one at a time, and prints one JSON line with every
process's medians and their spread.  The GPS column comes from the same processes.
System 2 has a chunk path (the select form on 8-sample chunks) in the wave shape only, so
at 14 and 4 channels its two variants time the same loop.  The chunk shapes and table
forms that were measured and deleted were separate builds of the library timed with this
tool ("BeiDou B1I").  Op model: 27 fp64 operations per sample for both (peak
78.6 TFLOP/s, an FMA as two).
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "gnss-sdr.ru_amd"))
import gnsscorr as gc  # noqa: E402

PEAK = 78.6e12
OPS = 27


def time_ctx(ctx, chans, d_if, n, epochs, warmup, runs):
    C = len(chans)
    d_ch = gc.DevBuf.from_array(chans)
    d_ep = gc.DevBuf(gc.SGT_EPOCH.itemsize * C * epochs)
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
    ep = d_ep.download(gc.SGT_EPOCH)
    assert (ep["status"] == 0).all(), "a channel stopped: the record is too short"
    return out, int(ep["blksize"].astype(np.int64).sum())


def report(ms, samples, C, epochs):
    med = float(np.median(ms))
    return dict(min=round(min(ms), 4), median=round(med, 4), max=round(max(ms), 4),
                us_per_channel_ms=round(med * 1e3 / (C * epochs), 4),
                fp64_frac=round(samples * OPS / (med * 1e-3) / PEAK, 4))


def one(a):
    if gc.device_count() < 1:
        raise SystemExit("b1i_time: no HIP device visible")
    C, E = a.channels, a.epochs
    rng = np.random.default_rng(1)
    n = int(a.fs * (E + 4) / 1000)
    IF = gc.ifgen(n, [], fs=a.fs, iq=a.file_type == 2, seed=5)
    d_if = gc.DevBuf.from_array(IF)
    starts = rng.integers(1, int(a.fs * 0.002), C)
    dops = rng.uniform(-4000, 4000, C)
    res = {}
    b1 = gc.SgtCtx(2, fileType=a.file_type, samplingFreq=a.fs)
    ch = b1.init_chans(rng.integers(1, 38, C), starts, 0.098e6 + dops)
    ms, samples = time_ctx(b1, ch, d_if, n, E, a.warmup, a.runs)
    res["b1i"] = report(ms, samples, C, E)
    gps = gc.SgtCtx(0, fileType=a.file_type, samplingFreq=a.fs)
    ch = gps.init_chans(rng.integers(1, 33, C), starts, 2.42e6 + dops)
    ms, samples = time_ctx(gps, ch, d_if, n, E, a.warmup, a.runs)
    res["gps"] = report(ms, samples, C, E)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", action="store_true", help="time one configuration in this process")
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--fs", type=float, default=16e6)
    ap.add_argument("--file-type", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--procs", type=int, default=3)
    a = ap.parse_args()
    if a.one:
        return one(a)
    out = dict(tool="b1i_time", epochs=a.epochs, fs=a.fs, file_type=a.file_type, runs=a.runs,
               procs=a.procs, rows=[])
    for C in (1024, 14, 4):
        for variant, chunk in (("chunked", "1"), ("per-sample", "0")):
            env = dict(os.environ, GNSSCORR_SGT_CHUNK=chunk)
            reps = []
            for _ in range(a.procs):        # one process at a time
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one",
                                    "--channels", str(C), "--epochs", str(a.epochs),
                                    "--fs", str(a.fs), "--file-type", str(a.file_type),
                                    "--warmup", str(a.warmup), "--runs", str(a.runs)],
                                   env=env, capture_output=True, text=True, timeout=300)
                if p.returncode != 0:
                    raise SystemExit(f"b1i_time: child failed ({p.returncode}): {p.stderr[-400:]}")
                reps.append(json.loads(p.stdout.strip().splitlines()[-1]))
            row = dict(channels=C, variant=variant)
            for k in ("b1i", "gps"):
                med = [r[k]["median"] for r in reps]
                row[k] = dict(medians_ms=med, min=min(med), max=max(med),
                              us_per_channel_ms=[r[k]["us_per_channel_ms"] for r in reps],
                              fp64_frac=[r[k]["fp64_frac"] for r in reps])
            out["rows"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
