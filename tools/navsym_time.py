#!/usr/bin/env python3
"""Time nav_viterbi_kernel (NavCtx.viterbi_dev) at the two shapes a receiver runs: 4096
streams of 120 bits (Galileo E1B page parts) and 1024 streams of 6000 bits (one minute of
GLONASS L3OC per channel), hard and soft input.

Each timed window is `--inner` launches between two HIP events on the context's stream,
ended by a stream synchronise; `--warmup` untimed windows, then `--runs` timed ones give
min / median / max per launch.  The kernel is one serial chain of L + 41 steps per stream
(one wave64 each), so the time is latency, not throughput: the JSON also gives ns per
trellis step of one stream and the streams that were in flight.

Before timing, the first `--check` streams of each shape are compared with viterbi_fast
of tests/navsym_scenarios.py at the timed size; the same runs give the single-core time
of viterbi_fast per stream, scaled to the shape's stream count in `cpu_fast_s`.
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnss-sdr.ru_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gnsscorr as gc  # noqa: E402
import navsym_scenarios as S  # noqa: E402

SHAPES = {"e1_4096x120": (4096, 120), "l3_1024x6000": (1024, 6000)}


def make_code(rng, n, L, soft):
    """n code words of L pairs: a few distinct messages with 3 % flips (hard) or noise of
    sigma 0.4 (soft), repeated to n streams"""
    base = min(n, 32)
    rows = []
    for _ in range(base):
        if soft:
            rows.append(S.soft_code(rng, L, sigma=0.4)[1])
        else:
            rows.append(S.noisy_code(rng, L, 0.03)[1])
    return np.ascontiguousarray(np.tile(np.array(rows), (n // base + 1, 1))[:n])


def time_shape(a, nav, name, soft):
    n, L = SHAPES[name]
    rng = np.random.default_rng(1)
    code = make_code(rng, n, L, soft)
    d_code, d_bits = gc.DevBuf.from_array(code), gc.DevBuf(n * L)
    stride = code.strides[0]
    nav.viterbi_dev(d_code.ptr, stride, n, L, soft, d_bits.ptr)
    nav.sync()
    got = d_bits.download(np.uint8).reshape(n, L)
    t0 = time.perf_counter()
    for i in range(a.check):
        want = S.viterbi_fast(code[i], soft)
        if got[i].tobytes() != want.tobytes():
            raise SystemExit(f"navsym_time: {name} soft={soft}: stream {i} differs")
    cpu_per_stream = (time.perf_counter() - t0) / max(a.check, 1)
    e0, e1 = gc.Event(), gc.Event()
    ms = []
    for r in range(a.warmup + a.runs):
        e0.record(nav.stream)
        for _ in range(a.inner):
            nav.viterbi_dev(d_code.ptr, stride, n, L, soft, d_bits.ptr)
        e1.record(nav.stream)
        nav.sync()
        if r >= a.warmup:
            ms.append(e0.elapsed_ms(e1) / a.inner)
    med = float(np.median(ms))
    return dict(streams=n, bits=L, soft=bool(soft), min_ms=round(min(ms), 4),
                median_ms=round(med, 4), max_ms=round(max(ms), 4),
                ns_per_step=round(med * 1e6 / (L + 41), 1),
                mbit_per_s=round(n * L / med / 1e3, 1),
                cpu_fast_s=round(cpu_per_stream * n, 2), cpu_streams_timed=a.check)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--check", type=int, default=4)
    a = ap.parse_args()
    if gc.device_count() < 1:
        raise SystemExit("navsym_time: no HIP device visible")
    nav = gc.NavCtx()
    res = dict(tool="navsym_time", warmup=a.warmup, runs=a.runs, inner=a.inner)
    for name in SHAPES:
        for soft in (False, True):
            res[name + ("_soft" if soft else "_hard")] = time_shape(a, nav, name, soft)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
