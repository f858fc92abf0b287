#!/usr/bin/env python3
"""Time nav_glo_satpos_kernel and nav_glo_fix_kernel (NavCtx.glo_satpos_dev, glo_fix_dev,
csrc/navglo.hip) at the shape of tools/navfix_time.py: 341 receivers x 12 channels x 70
measurements (navSolPeriod 20 over 1460 epochs).  glo_ephemeris_dev on the same channels is
timed too.

Each timed window is `--inner` calls between two HIP events on the context's stream, ended
by a stream synchronise; `--warmup` untimed windows, then `--runs` timed ones give min /
median / max per call.  The scene is `--block` generated receivers repeated (states on the
ICD grid, frame times within 15 minutes of t_b, absoluteSample planted for a receiver near
the surface); before timing, the first `--check` receivers are compared with the restatement
of tests/navglo_scenarios.py at the timed size, with that module's tolerances.  Prints one
JSON line.
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
import navglo_scenarios as S  # noqa: E402


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
    return dict(min_ms=round(min(ms), 4), median_ms=round(float(np.median(ms)), 4),
                max_ms=round(max(ms), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--receivers", type=int, default=341)
    ap.add_argument("--channels", type=int, default=12, help="per receiver")
    ap.add_argument("--meas", type=int, default=70)
    ap.add_argument("--block", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--check", type=int, default=2)
    a = ap.parse_args()
    if gc.device_count() < 1:
        raise SystemExit("navglo_time: no HIP device visible")
    a.block = min(a.block, a.receivers)
    period, n_ep = 20, 60 + 20 * a.meas
    s = S.make_fix_scene(31, (a.channels,) * a.block, n_epochs=n_ep, period=period,
                         max_meas=a.meas)
    reps = -(-a.receivers // a.block)
    n_ch = a.receivers * a.channels
    tile = lambda x: np.concatenate([x] * reps)[:n_ch]
    bits, n_str, first, abs_sample = (tile(s[k]) for k in ("bits", "n_strings", "first", "abs_sample"))
    rx_first = (np.arange(a.receivers + 1) * a.channels).astype(np.int32)
    cfg = gc.glo_fix_cfg(**s["cfg"])
    nav = gc.NavCtx()
    d_bits, d_ns, d_first, d_x = (gc.DevBuf.from_array(x) for x in (bits, n_str, first, abs_sample))
    d_eph = gc.DevBuf(n_ch * gc.GLO_EPH.itemsize)
    d_sat = gc.DevBuf(n_ch * gc.GLO_SAT.itemsize)
    d_n = gc.DevBuf(4 * a.receivers)
    d_sol = gc.DevBuf(a.receivers * a.meas * gc.GPS_FIX_SOL.itemsize)
    d_chan = gc.DevBuf(n_ch * a.meas * gc.GPS_FIX_CHAN.itemsize)

    def eph():
        nav.glo_ephemeris_dev(d_bits.ptr, d_ns.ptr, d_first.ptr, n_ch, d_eph.ptr)

    def satpos():
        nav.glo_satpos_dev(d_eph.ptr, n_ch, cfg, d_sat.ptr)

    def fix():
        nav.glo_fix_dev(d_eph.ptr, d_sat.ptr, d_first.ptr, d_x.ptr, 8, 8 * n_ep, n_ep, rx_first,
                        cfg, d_n.ptr, d_sol.ptr, d_chan.ptr)

    def both():
        satpos()
        fix()

    eph()
    both()
    nav.sync()
    n_meas = d_n.download(np.int32)
    sat = d_sat.download(gc.GLO_SAT)
    sol = d_sol.download(gc.GPS_FIX_SOL).reshape(a.receivers, a.meas)
    chan = d_chan.download(gc.GPS_FIX_CHAN).reshape(n_ch, a.meas)
    k = min(a.check, a.block)
    kc = k * a.channels
    if d_eph.download(gc.GLO_EPH)[:kc].tobytes() != s["eph"][:kc].tobytes():
        raise SystemExit("navglo_time: ephemerides differ")
    lit = S.satpos_literal(s["eph"][:kc], period)
    for key in ("n10", "n1", "n001", "ready", "deltat", "clk"):
        if not np.array_equal(sat[key][:kc], lit[key]):
            raise SystemExit(f"navglo_time: {key} differs")
    for g in S.STATE_GROUPS:
        dist = S.state_distance(sat[:kc], lit, g)
        if dist > S.TOL[g]:
            raise SystemExit(f"navglo_time: {g} differs by {dist} (tolerance {S.TOL[g]})")
    w_n, Sx, Cx = S.fix_literal(s["eph"][:kc], s["first"][:kc], s["abs_sample"][:kc],
                                rx_first[:k + 1], s["cfg"], sat=lit)
    want = S.G.as_records(w_n, Sx, Cx)
    if n_meas[:k].tolist() != w_n.tolist() or (n_meas != a.meas).any():
        raise SystemExit(f"navglo_time: n_meas {n_meas[:k]} vs {w_n}")
    if chan["rawP"][:kc].tobytes() != want[1]["rawP"].tobytes() or \
            not np.array_equal(sol["status"][:k], want[0]["status"]):
        raise SystemExit("navglo_time: rawP or status differ")
    for g in S.GROUPS:
        dist = S.group_distance((sol[:k], chan[:kc]), want, g)
        if dist > S.TOL[g]:
            raise SystemExit(f"navglo_time: {g} differs by {dist} (tolerance {S.TOL[g]})")
    steps = sat["n10"] + sat["n1"] + sat["n001"]
    res = dict(tool="navglo_time", receivers=a.receivers, channels=a.channels, meas=a.meas,
               warmup=a.warmup, runs=a.runs, inner=a.inner,
               solved=int((sol["status"] == gc.GPS_FIX_OK).sum()),
               rk4_steps_max=int(steps.max()), rk4_steps_mean=round(float(steps.mean()), 1),
               ephemeris=timed(a, nav, eph), satpos=timed(a, nav, satpos), fix=timed(a, nav, fix),
               satpos_and_fix=timed(a, nav, both))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
