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

import numpy as np

import ftrack_time as F
from ftrack_time import gc

E1T_OPS = 41        # fp64 operations per sample


def main():
    ap = argparse.ArgumentParser()
    F.add_args(ap, fs=16e6)
    ap.add_argument("--file-type", type=int, default=2)
    a = ap.parse_args()
    C, E = a.channels, a.epochs
    rng, n, d_if, starts, dops = F.setup(a, "e1t_time", a.file_type)

    e1 = gc.E1tCtx(fileType=a.file_type, samplingFreq=a.fs)
    codes = rng.choice(np.array([-1, 1], np.int8), (50, 4092))   # the time does not depend on the chips
    e1.set_codes(codes)
    ch = e1.init_chans(rng.integers(0, 50, C), starts, 2.42e6 + dops)
    res = dict(tool="e1t_time", channels=C, epochs=E, fs=a.fs, file_type=a.file_type,
               e1_path="per-sample" if os.environ.get("GNSSCORR_E1T_CHUNK", "1")[:1] == "0"
               else "chunked",
               e1t=F.time_tracker(a, e1, ch, gc.E1T_EPOCH, E1T_OPS, d_if, n))
    res["sgt_gps"] = F.time_gps(a, rng, starts, dops, d_if, n, a.file_type)
    res["e1t_over_sgt"] = round(res["e1t"]["median"] / res["sgt_gps"]["median"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
