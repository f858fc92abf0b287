#!/usr/bin/env python3
"""Time nav_b1_eph_kernel and nav_b1_fix_kernel (NavCtx.b1_ephemeris_dev, b1_fix_dev,
csrc/navb1.hip) at the shape of tools/navfix_time.py and tools/navglo_time.py: 341 receivers x
12 channels x 70 measurements (navSolPeriod 20 over 1460 epochs), and gps_fix_dev and
glo_fix_dev at the same shape in the same process, so that the three fixes can be compared.

Each timed window is `--inner` calls between two HIP events on the context's stream, ended
by a stream synchronise; `--warmup` untimed windows, then `--runs` timed ones give min /
median / max per call.  Each scene is `--block` generated receivers repeated; the troposphere
is on in all three so that the least squares do the same work.  Before timing, the first
`--check` BeiDou receivers are compared with the restatement of tests/navb1_scenarios.py at the
timed size, with that module's tolerances.  Prints one JSON line.
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
import navb1_scenarios as S  # noqa: E402
import navfix_scenarios as G  # noqa: E402
import navglo_scenarios as GL  # noqa: E402


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
        raise SystemExit("navb1_time: no HIP device visible")
    a.block = min(a.block, a.receivers)
    period, n_ep = 20, 60 + 20 * a.meas
    sizes = (a.channels,) * a.block
    reps = -(-a.receivers // a.block)
    n_ch = a.receivers * a.channels
    tile = lambda x: np.concatenate([x] * reps)[:n_ch]
    rx_first = (np.arange(a.receivers + 1) * a.channels).astype(np.int32)
    nav = gc.NavCtx()
    d_n = gc.DevBuf(4 * a.receivers)
    d_sol = gc.DevBuf(a.receivers * a.meas * gc.GPS_FIX_SOL.itemsize)
    d_chan = gc.DevBuf(n_ch * a.meas * gc.GPS_FIX_CHAN.itemsize)

    def solved():
        nav.sync()
        sol = d_sol.download(gc.GPS_FIX_SOL).reshape(a.receivers, a.meas)
        return int((sol["status"] == gc.GPS_FIX_OK).sum())

    # BeiDou B1I
    s = S.make_fix_scene(31, sizes, n_epochs=n_ep, period=period, max_meas=a.meas, trop=1)
    bits, n_sub, first, x = (tile(s[k]) for k in ("bits", "n_subframes", "first", "abs_sample"))
    cfg = gc.b1_fix_cfg(**s["cfg"])
    d_bits, d_ns, d_first, d_x = (gc.DevBuf.from_array(v) for v in (bits, n_sub, first, x))
    d_eph = gc.DevBuf(n_ch * gc.B1_EPH.itemsize)

    def b1_eph():
        nav.b1_ephemeris_dev(d_bits.ptr, d_ns.ptr, d_first.ptr, n_ch, d_eph.ptr)

    def b1_fix():
        nav.b1_fix_dev(d_eph.ptr, d_first.ptr, d_x.ptr, 8, 8 * n_ep, n_ep, rx_first, cfg,
                       d_n.ptr, d_sol.ptr, d_chan.ptr)

    b1_eph()
    b1_fix()
    nav.sync()
    n_meas = d_n.download(np.int32)
    sol = d_sol.download(gc.GPS_FIX_SOL).reshape(a.receivers, a.meas)
    chan = d_chan.download(gc.GPS_FIX_CHAN).reshape(n_ch, a.meas)
    k = min(a.check, a.block)
    kc = k * a.channels
    if d_eph.download(gc.B1_EPH)[:kc].tobytes() != s["eph"][:kc].tobytes():
        raise SystemExit("navb1_time: ephemerides differ")
    w_n, Sx, Cx = S.fix_literal(s["eph"][:kc], s["first"][:kc], s["abs_sample"][:kc],
                                rx_first[:k + 1], s["cfg"])
    want = S.as_records(w_n, Sx, Cx)
    if n_meas[:k].tolist() != w_n.tolist() or (n_meas != a.meas).any():
        raise SystemExit(f"navb1_time: n_meas {n_meas[:k]} vs {w_n}")
    if chan["rawP"][:kc].tobytes() != want[1]["rawP"].tobytes() or \
            not np.array_equal(sol["status"][:k], want[0]["status"]):
        raise SystemExit("navb1_time: rawP or status differ")
    for g in S.GROUPS:
        dist = S.group_distance((sol[:k], chan[:kc]), want, g)
        if dist > S.TOL[g]:
            raise SystemExit(f"navb1_time: {g} differs by {dist} (tolerance {S.TOL[g]})")
    res = dict(tool="navb1_time", receivers=a.receivers, channels=a.channels, meas=a.meas,
               warmup=a.warmup, runs=a.runs, inner=a.inner, b1_solved=solved(),
               b1_ephemeris=timed(a, nav, b1_eph), b1_fix=timed(a, nav, b1_fix))

    # GPS L1 at the same shape
    g = G.make_fix_scene(31, sizes, n_epochs=n_ep, period=period, max_meas=a.meas)
    g_cfg = gc.gps_fix_cfg(**g["cfg"])
    dg_eph, dg_first, dg_x = (gc.DevBuf.from_array(tile(g[k])) for k in ("eph", "first", "abs_sample"))

    def gps_fix():
        nav.gps_fix_dev(dg_eph.ptr, dg_first.ptr, dg_x.ptr, 8, 8 * n_ep, n_ep, rx_first, g_cfg,
                        d_n.ptr, d_sol.ptr, d_chan.ptr)

    gps_fix()
    res.update(gps_solved=solved(), gps_fix=timed(a, nav, gps_fix))

    # GLONASS L1OF at the same shape
    q = GL.make_fix_scene(31, sizes, n_epochs=n_ep, period=period, max_meas=a.meas)
    q_cfg = gc.glo_fix_cfg(**q["cfg"])
    dq_eph, dq_first, dq_x = (gc.DevBuf.from_array(tile(q[k])) for k in ("eph", "first", "abs_sample"))
    dq_sat = gc.DevBuf(n_ch * gc.GLO_SAT.itemsize)
    nav.glo_satpos_dev(dq_eph.ptr, n_ch, q_cfg, dq_sat.ptr)

    def glo_fix():
        nav.glo_fix_dev(dq_eph.ptr, dq_sat.ptr, dq_first.ptr, dq_x.ptr, 8, 8 * n_ep, n_ep,
                        rx_first, q_cfg, d_n.ptr, d_sol.ptr, d_chan.ptr)

    glo_fix()
    res.update(glo_solved=solved(), glo_fix=timed(a, nav, glo_fix))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
