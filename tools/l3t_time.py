#!/usr/bin/env python3
"""Time the GLONASS L3OC float tracker (L3tCtx, GLONASS/L3/tracking.sci) and, as the
yardstick, the GPS L1 C/A float tracker (SgtCtx) at the same channels, epochs and rate.

N channels x E epochs, closed loop, device-resident (track_dev), HIP events on each
context's stream, on a seeded noise record long enough for every channel; the channel
state is uploaded again before every launch, so each launch does the same work.
`--runs` timed launches after `--warmup` untimed ones give min / median / max.

Reports per tracker: us per channel-ms, samples/s and the fraction of fp64 peak under
the op model (L3: 39 fp64 ops per sample = GPS's 27 + 12 for the second code's sums;
peak 78.6 TFLOP/s, an FMA as two).  At 24 Msps an L3 epoch has 1.5 times the samples of
a 16 Msps GPS epoch; both trackers run here at the same --fs.  Prints one JSON line.

--search times the full L3 search instead (L = 10 ms, keep = 5 ms, period 1 ms, spc 2,
51 bins, --codes replicas): 3 warm-up + 20 timed correlate_dev + select calls on resident
spectra, with the period rule on and off.
"""
import argparse
import json

import numpy as np

import ftrack_time as F
from ftrack_time import gc

L3T_OPS = 39        # fp64 operations per sample


def search(a):
    fs, S = a.fs, int(round(a.fs / 1000))
    G, B = a.codes, 51
    IF = gc.ifgen(10 * S, [], fs=fs, iq=True, seed=5)
    rows = [gc.sample_code(gc.l3_code(33 + g % 31), 10.23e6, fs, S) for g in range(G)]
    codes = np.stack([np.concatenate([b * r for b in (-1, -1, -1, 1, -1)]) for r in rows])
    frq = gc.l3_bins(-2.025e6, 5)
    acq = gc.AcqCtx(fs, 10 * S, max_freqs=64, max_blocks=1, max_codes=G)
    acq.set_zero_padded(5 * S)
    acq.set_codes_padded(codes.astype(np.int8))
    d_if, d_f = gc.DevBuf.from_array(IF), gc.DevBuf.from_array(frq)
    d_gc = gc.DevBuf.from_array(np.arange(G, dtype=np.int32))
    d_gf = gc.DevBuf.from_array(np.tile(np.arange(B, dtype=np.int32), (G, 1)))
    d_rows, d_res = gc.DevBuf(gc.ACQ_ROW.itemsize * G * B), gc.DevBuf(gc.ACQ_RESULT.itemsize * G)
    res = dict(tool="l3t_time --search", codes=G, bins=B, fs=fs, L=10 * S, keep=5 * S, period=S)
    e0, e1 = gc.Event(), gc.Event()
    for period in (S, 0):
        acq.set_peak_period(period)
        ms = []
        for r in range(3 + 20):
            e0.record(acq.stream)
            acq.search_dev(d_if.ptr, 1, B, d_f.ptr, G, B, d_gc.ptr, d_gf.ptr, d_rows.ptr,
                           d_res.ptr, spc=2)
            e1.record(acq.stream)
            acq.sync()
            if r >= 3:
                ms.append(e0.elapsed_ms(e1))
        res["period_on" if period else "period_off"] = dict(
            min=round(min(ms), 4), median=round(float(np.median(ms)), 4), max=round(max(ms), 4))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    F.add_args(ap, fs=24e6)
    ap.add_argument("--search", action="store_true")
    ap.add_argument("--codes", type=int, default=1)
    a = ap.parse_args()
    if a.search:
        if gc.device_count() < 1:
            raise SystemExit("l3t_time: no HIP device visible")
        return search(a)
    C, E = a.channels, a.epochs
    rng, n, d_if, starts, dops = F.setup(a, "l3t_time")

    l3 = gc.L3tCtx(samplingFreq=a.fs)
    ch = l3.init_chans(rng.integers(1, 32, C), starts, -2.025e6 + dops)
    res = dict(tool="l3t_time", channels=C, epochs=E, fs=a.fs,
               l3t=F.time_tracker(a, l3, ch, gc.L3T_EPOCH, L3T_OPS, d_if, n))
    res["sgt_gps"] = F.time_gps(a, rng, starts, dops, d_if, n)
    res["l3t_over_sgt"] = round(res["l3t"]["median"] / res["sgt_gps"]["median"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
