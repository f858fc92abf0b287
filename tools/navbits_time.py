#!/usr/bin/env python3
"""Time nav_pattern_hits_kernel (NavCtx.pattern_hits_dev) and the three chains of
csrc/navbits.hip at the shape a receiver farm runs: 4096 channels x 40 000 epochs of
gnsscorr_sgt_epoch records read in place (stride 112), T = 160, 220 and 300 taps, and
gps_frames_dev / glo_strings_dev / b1_subframes_dev on the same records.

Each timed window is `--inner` calls between two HIP events on the context's stream, ended
by a stream synchronise; `--warmup` untimed windows, then `--runs` timed ones give min /
median / max per call.  The series touches every 112-byte record, so the read floor of a
call is n_ch * n_epochs * 112 B over the HBM stream rate (`--hbm-tbps`, by default the
6.29 TB/s a float4 copy reaches on an MI355X); the JSON gives each median's ratio to it.
The chains read the records a second time for their bits, a few per cent of them.

The device array is `--block` generated channels repeated; before timing, the first
`--check` channels are compared with the fast restatement of tests/navbits_scenarios.py.
GNSSCORR_LIB selects another build of the library (the tap-loop baseline of DESIGN.md) for
the same inputs.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnss-sdr.ru_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gnsscorr as gc  # noqa: E402
import navbits_scenarios as S  # noqa: E402

MAX_HITS = 8


def make_records(a, system):
    """d_epochs [n_ch, n_epochs] of SGT_EPOCH with generated I_P, and the generated block"""
    rng = np.random.default_rng(11 + len(system))
    gen = {"gps": lambda i: S.gps_series(rng, a.epochs, 5200 + 20 * i, polarity=1 - 2 * (i & 1),
                                         flip_rate=0.01, n_zeros=20)[0],
           "glo": lambda i: S.glo_series(rng, a.epochs, 37 * i, polarity=1 - 2 * (i & 1),
                                         flip_rate=0.01, n_zeros=20)[0],
           "b1": lambda i: S.b1_series(rng, a.epochs, 41 * i, polarity=1 - 2 * (i & 1),
                                       flip_rate=0.01, n_zeros=20)[0]}[system]
    block = np.stack([gen(i) for i in range(a.block)])
    ep = np.zeros((a.block, a.epochs), gc.SGT_EPOCH)
    ep["I_P"] = block
    ep["Q_P"] = 0.1 * block[:, ::-1]
    d_ep = gc.DevBuf(a.channels * a.epochs * gc.SGT_EPOCH.itemsize)
    for c0 in range(0, a.channels, a.block):
        n = min(a.block, a.channels - c0)
        d_ep.upload(ep[:n], c0 * a.epochs * gc.SGT_EPOCH.itemsize)
    return d_ep, block


def timed(a, nav, call):
    e0, e1 = gc.Event(), gc.Event()
    ms = []
    for r in range(a.warmup + a.runs):
        e0.record(nav.stream)
        for _ in range(a.inner):
            call()
        e1.record(nav.stream)
        nav.sync()
        if r >= a.warmup:
            ms.append(e0.elapsed_ms(e1) / a.inner)
    floor_ms = a.channels * a.epochs * gc.SGT_EPOCH.itemsize / (a.hbm_tbps * 1e12) * 1e3
    med = float(np.median(ms))
    return dict(min_ms=round(min(ms), 4), median_ms=round(med, 4), max_ms=round(max(ms), 4),
                floor_ms=round(floor_ms, 4), over_floor=round(med / floor_ms, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--epochs", type=int, default=40000)
    ap.add_argument("--block", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--check", type=int, default=4)
    ap.add_argument("--hbm-tbps", type=float, default=6.29)
    ap.add_argument("--only", default="", help="comma list of gps,glo,b1")
    a = ap.parse_args()
    if gc.device_count() < 1:
        raise SystemExit("navbits_time: no HIP device visible")
    a.block = min(a.block, a.channels)
    nav = gc.NavCtx()
    off, stride = gc.epoch_field(gc.SGT_EPOCH, "I_P")
    cs, n_ch, n_ep = a.epochs * stride, a.channels, a.epochs
    res = dict(tool="navbits_time", lib=os.path.basename(gc.LIB_PATH), channels=n_ch,
               epochs=n_ep, warmup=a.warmup, runs=a.runs, inner=a.inner, hbm_tbps=a.hbm_tbps)
    d_first, d_n = gc.DevBuf(4 * n_ch), gc.DevBuf(4 * n_ch)
    d_hits = gc.DevBuf(4 * n_ch * MAX_HITS)
    systems = {
        "gps": (S.GPS_PATTERN, 153, 5000, S.gps_frames_fast, (1500,),
                lambda p, b: nav.gps_frames_dev(p, stride, cs, n_ep, n_ch, 5000, 5, d_first.ptr,
                                                d_n.ptr, b)),
        "glo": (S.GLO_PATTERN, 290, 0, S.glo_strings_fast, (15, 85),
                lambda p, b: nav.glo_strings_dev(p, stride, cs, n_ep, n_ch, 15, d_first.ptr,
                                                 d_n.ptr, b)),
        "b1": (S.B1_PATTERN, 200, 0, S.b1_subframes_fast, (5, 213),
               lambda p, b: nav.b1_subframes_dev(p, stride, cs, n_ep, n_ch, 5, d_first.ptr,
                                                 d_n.ptr, b)),
    }
    for name, (pattern, thr, first_k, fast, shape, chain) in systems.items():
        if a.only and name not in a.only.split(","):
            continue
        d_ep, block = make_records(a, name)
        src = d_ep.ptr + off
        d_bits = gc.DevBuf(n_ch * int(np.prod(shape)))

        def hits():
            nav.pattern_hits_dev(src, stride, cs, n_ep, n_ch, pattern, thr, first_k, MAX_HITS,
                                 d_first.ptr, d_n.ptr, d_hits.ptr)

        hits()
        nav.sync()
        first, n_hits = d_first.download(np.int32), d_n.download(np.int32)
        hl = d_hits.download(np.int32).reshape(n_ch, MAX_HITS)
        for i in range(min(a.check, a.block)):
            want = S.pattern_hits_fast(block[i], pattern, thr, first_k)
            k = min(len(want), MAX_HITS)
            if n_hits[i] != len(want) or hl[i, :k].tolist() != want[:k].tolist() or \
                    first[i] != (want[0] if len(want) else -1):
                raise SystemExit(f"navbits_time: {name}: hits of channel {i} differ")
        chain(src, d_bits.ptr)
        nav.sync()
        first, cnt = d_first.download(np.int32), d_n.download(np.int32)
        bits = d_bits.download(np.uint8).reshape(n_ch, -1)
        for i in range(min(a.check, a.block)):
            w_first, w_bits = fast(block[i])
            if first[i] != w_first or bits[i, :w_bits.size].tobytes() != w_bits.tobytes():
                raise SystemExit(f"navbits_time: {name}: chain of channel {i} differs")
        res[f"hits_T{len(pattern)}"] = timed(a, nav, hits)
        res[f"{name}_chain"] = dict(timed(a, nav, lambda: chain(src, d_bits.ptr)),
                                    found=int((first >= 0).sum()), units=int(cnt.sum()))
        d_ep.free()
        d_bits.free()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
