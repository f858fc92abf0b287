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

import ftrack_time as F
from ftrack_time import gc

KEYS = ("min", "median", "max", "us_per_channel_ms", "fp64_frac")   # of ftrack_time.report


def one(a):
    rng, n, d_if, starts, dops = F.setup(a, "b1i_time", a.file_type)
    b1 = gc.SgtCtx(2, fileType=a.file_type, samplingFreq=a.fs)
    ch = b1.init_chans(rng.integers(1, 38, a.channels), starts, 0.098e6 + dops)
    res = dict(b1i=F.time_tracker(a, b1, ch, gc.SGT_EPOCH, F.GPS_OPS, d_if, n),
               gps=F.time_gps(a, rng, starts, dops, d_if, n, a.file_type))
    print(json.dumps({k: {f: r[f] for f in KEYS} for k, r in res.items()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", action="store_true", help="time one configuration in this process")
    F.add_args(ap, fs=16e6)
    ap.add_argument("--file-type", type=int, default=2)
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
