#!/usr/bin/env python3
"""Time the COMPASS B1 coherent searches (COMPASS/B1/acquisition_7x3ms.sci and
acquisition_4x5ms.sci: overlapping blocks, concatenated rows, the period second-peak rule)
and, as the yardstick on the same box, the 1 ms zero-padded search of acquisition.sci.

The receiver's default shape: --codes PRNs (32), the --band kHz band (14: 85 bins of
1000/6 Hz at 3 ms, 141 of 100 Hz at 5 ms, 29 of 500 Hz at 1 ms), 16 Msps, spc 8, period
16 000, on a seeded noise record.  Whole searches (search_dev: spectra, correlation,
statistics, selection), device-resident, HIP events on the context stream, --warmup
untimed then --runs timed calls: min / median / max in ms.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "gnss-sdr.ru_amd"))
import gnsscorr as gc  # noqa: E402

FS, S, IF_FREQ = 16e6, 16000, 0.098e6
SHAPES = {"1ms": (1, 1), "3ms": (3, 7), "5ms": (5, 4)}      # code periods per block, blocks


def time_search(name, a, IF, rows):
    coh, nblk = SHAPES[name]
    M, G = coh * S, a.codes
    frq = gc.b1_coh_bins(IF_FREQ, a.band, coh)
    B = len(frq)
    acq = gc.AcqCtx(FS, 2 * M, max_freqs=B, max_blocks=nblk, max_codes=G)
    acq.set_zero_padded(M)
    mode = gc.ACQ_BEST_OF_BLOCKS
    if nblk > 1:
        acq.set_block_stride(M)
        acq.set_peak_period(S)
        mode = gc.ACQ_CONCAT
    acq.set_codes_padded(-np.tile(rows, (1, coh)) if nblk > 1 else rows)
    d_if, d_f = gc.DevBuf.from_array(IF), gc.DevBuf.from_array(frq)
    d_gc = gc.DevBuf.from_array(np.arange(G, dtype=np.int32))
    d_gf = gc.DevBuf.from_array(np.tile(np.arange(B, dtype=np.int32), (G, 1)))
    d_rows, d_res = gc.DevBuf(gc.ACQ_ROW.itemsize * G * B), gc.DevBuf(gc.ACQ_RESULT.itemsize * G)
    e0, e1 = gc.Event(), gc.Event()
    ms = []
    for r in range(a.warmup + a.runs):
        e0.record(acq.stream)
        acq.search_dev(d_if.ptr, nblk, B, d_f.ptr, G, B, d_gc.ptr, d_gf.ptr, d_rows.ptr,
                       d_res.ptr, spc=8, mode=mode)
        e1.record(acq.stream)
        acq.sync()
        if r >= a.warmup:
            ms.append(e0.elapsed_ms(e1))
    acq.close()
    return dict(L=2 * M, blocks=nblk, bins=B, units=G * B * nblk, min=round(min(ms), 3),
                median=round(float(np.median(ms)), 3), max=round(max(ms), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--codes", type=int, default=32)
    ap.add_argument("--band", type=float, default=14.0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--shapes", default="1ms,3ms,5ms")
    a = ap.parse_args()
    if gc.device_count() < 1:
        raise SystemExit("b1coh_time: no HIP device visible")
    IF = gc.ifgen(25 * S, [], fs=FS, iq=True, seed=5)
    rows = np.stack([gc.sample_code(gc.b1i_code(1 + g % 37), 2.046e6, FS, S)
                     for g in range(a.codes)])
    res = dict(tool="b1coh_time", codes=a.codes, band_khz=a.band, fs=FS)
    for name in a.shapes.split(","):
        res[name] = time_search(name, a, IF, rows)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
