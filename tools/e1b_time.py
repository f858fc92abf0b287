#!/usr/bin/env python3
"""Time the full Galileo E1B acquisition search (GALILEO/E1/acquisition.sci shape):
50 codes x 113 bins (e1b_bins(2.42e6, 14, 4)), L = 128000 = 2 x 64000 samples at
16 Msps, one block, fp64, device-resident (gnsscorr_acq_search_dev: spectra, correlation
passes, row statistics, selection), HIP events on the context stream, warm.

  padded (default)  set_zero_padded(64000) + set_codes_padded: codes of 64000 samples
                    zero-extended, statistics over the 64000 kept lags
  --unpadded        the search a library without the mode can run at this length:
                    +-1 codes of the full 128000 samples, statistics over all lags
                    (the only form available before the mode existed; with
                    GNSSCORR_LIB set to such a library this is what to run)

Each run times `--steps` searches between two events after `--warmup` untimed ones;
`--runs` runs give the spread (min / median / max of ms per search).  Prints one JSON line.
The codes are seeded random chips: the time does not depend on their values.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "gnss-sdr.ru_amd"))
import gnsscorr as gc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--unpadded", action="store_true")
    ap.add_argument("--codes", type=int, default=50)
    ap.add_argument("--bins", type=int, default=113)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    fs, S, L, spc = 16.0e6, 64000, 128000, 16
    if gc.device_count() < 1:
        raise SystemExit("e1b_time: no HIP device visible")
    rng = np.random.default_rng(1)
    ms = 4
    freqs = 2.42e6 - 7000.0 + (1000.0 / (2 * ms)) * np.arange(a.bins)
    ctx = gc.AcqCtx(fs, L, max_freqs=a.bins, max_blocks=1, max_codes=a.codes)
    if a.unpadded:
        ctx.set_codes(rng.choice(np.array([-1, 1], np.int8), (a.codes, L)))
    else:
        ctx.set_zero_padded(S)
        ctx.set_codes_padded(rng.choice(np.array([-1, 1], np.int8), (a.codes, S)))
    IF = rng.choice(np.array([-3, -1, 1, 3], np.int8), 2 * L)
    d_if = gc.DevBuf.from_array(IF)
    d_freqs = gc.DevBuf.from_array(freqs)
    d_gcode = gc.DevBuf.from_array(np.arange(a.codes, dtype=np.int32))
    d_gfreq = gc.DevBuf.from_array(np.tile(np.arange(a.bins, dtype=np.int32), (a.codes, 1)))
    d_rows = gc.DevBuf(gc.ACQ_ROW.itemsize * a.codes * a.bins)
    d_res = gc.DevBuf(gc.ACQ_RESULT.itemsize * a.codes)

    def search():
        ctx.search_dev(d_if.ptr, 1, a.bins, d_freqs.ptr, a.codes, a.bins, d_gcode.ptr,
                       d_gfreq.ptr, d_rows.ptr, d_res.ptr, spc=spc)

    e0, e1 = gc.Event(), gc.Event()
    runs = []
    for _ in range(a.runs):
        for _ in range(a.warmup):
            search()
        ctx.sync()
        e0.record(ctx.stream)
        for _ in range(a.steps):
            search()
        e1.record(ctx.stream)
        ctx.sync()
        runs.append(e0.elapsed_ms(e1) / a.steps)
    rows = d_rows.download(gc.ACQ_ROW)
    print(json.dumps(dict(tool="e1b_time", mode="unpadded" if a.unpadded else "padded",
                          lib=os.path.basename(os.path.dirname(os.path.dirname(gc.LIB_PATH))),
                          codes=a.codes, bins=a.bins, L=L, keep=L if a.unpadded else S,
                          steps=a.steps, warmup=a.warmup,
                          ms_per_search=[round(r, 4) for r in runs],
                          min=round(min(runs), 4), median=round(float(np.median(runs)), 4),
                          max=round(max(runs), 4),
                          max_argmax=int(rows["argmax"].max()))))


if __name__ == "__main__":
    main()
