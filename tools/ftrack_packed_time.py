"""Packed and int16 against int8 records in the float trackers ("Packed
records", "int16 records").

Closed loop, device-resident (track_dev), HIP events on the context's stream; the channel
state is uploaded again before every launch, so each launch does the same work.  The int8
and the packed launch of a shape alternate (with --int16 the int16 launch too, the same
levels stored as int16), `--warmup` untimed rounds first, then `--runs` timed ones: min /
median / max per format and the ratio of the medians.

Shapes:
  sgt_bench   bench.py's GLONASS shape: 256 records x 14 FCH = 3584 channels x 30 epochs
  sgt_config4 one 14-channel receiver x 30 epochs (per-epoch latency)
  e1t         Galileo E1B default mode, --channels channels x --epochs epochs
  l3t         GLONASS L3OC, --channels channels x --epochs epochs

--int8-only times the int8 launches alone: with GNSSCORR_LIB set to another build of the
library (one without the packed setters too) this is the A/B of the int8 path.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("gnss-sdr.ru_amd", "tests", os.path.join("tests", "golden"), "oracle"):
    sys.path.insert(0, os.path.join(ROOT, p))
import gnsscorr as gc  # noqa: E402


def levels(x, sigma):
    x = np.asarray(x, np.int16)
    return (np.where(x < 0, -1, 1) * np.where(np.abs(x) > sigma, 3, 1)).astype(np.int8)


def time_pair(a, ctx, rec, stride, n, chans, dtype_ep, epochs):
    """rec: the int8 record(s); returns {format: [ms]} and checks that both formats give
    the same epochs."""
    C = len(chans)
    bufs = {"int8": (gc.DevBuf.from_array(rec), stride)}
    if not a.int8_only:
        bufs["packed"] = (gc.DevBuf.from_array(gc.pack2(rec)), stride // 4)
    if a.int16:
        bufs["int16"] = (gc.DevBuf.from_array(rec.astype(np.int16)), 2 * stride)
    d_ch = gc.DevBuf.from_array(chans)
    d_ep = gc.DevBuf(dtype_ep.itemsize * C * epochs)
    e0, e1 = gc.Event(), gc.Event()
    ms = {k: [] for k in bufs}
    last = {}
    for r in range(a.warmup + a.runs):
        for k, (d_if, st) in bufs.items():
            if a.int16:
                ctx.set_format({"packed": "packed2"}.get(k, k))
            elif not a.int8_only:
                ctx.set_packed(k == "packed")
            d_ch.upload(chans)
            e0.record(ctx.stream)
            ctx.track_dev(d_if.ptr, st, n, C, d_ch.ptr, epochs, d_ep.ptr, closed_loop=True)
            e1.record(ctx.stream)
            ctx.sync()
            if r >= a.warmup:
                ms[k].append(e0.elapsed_ms(e1))
            last[k] = d_ep.download(dtype_ep)
    assert (last["int8"]["status"] == 0).all(), "a channel stopped: the record is too short"
    if "packed" in last:
        assert last["packed"].tobytes() == last["int8"].tobytes(), "packed differs from int8"
    out = {k: dict(ms=[round(x, 4) for x in v], min=round(min(v), 4),
                   median=round(float(np.median(v)), 4), max=round(max(v), 4))
           for k, v in ms.items()}
    if "packed" in out:
        out["packed_over_int8"] = round(out["packed"]["median"] / out["int8"]["median"], 4)
    if "int16" in out:
        assert last["int16"].tobytes() == last["int8"].tobytes(), "int16 differs from int8"
        out["int16_over_int8"] = round(out["int16"]["median"] / out["int8"]["median"], 4)
    out.update(channels=C, epochs=epochs)
    return out


def sgt_bench(a, rx, epochs=30):
    fs = 16e6
    ns = int(fs * (epochs + 4) / 1000)
    stride = 2 * ns
    rng = np.random.default_rng(44)
    rec = rng.choice(np.array([-3, -1, 1, 3], np.int8), rx * stride)
    ctx = gc.SgtCtx(1, samplingFreq=fs)
    fch = np.tile(np.arange(-7, 7), rx)
    ch = ctx.init_chans(fch, rng.integers(1, 16000, len(fch)),
                        1e6 + 0.5625e6 * fch + rng.uniform(-3000, 3000, len(fch)),
                        streams=np.repeat(np.arange(rx), 14))
    return time_pair(a, ctx, rec, stride, ns, ch, gc.SGT_EPOCH, epochs)


def e1t(a):
    import e1t_scenarios as E
    IF, codes, chans = E.closed_loop_scene()
    rec = levels(IF, 6)
    ctx = gc.E1tCtx()
    ctx.set_codes(codes)
    reps = -(-a.channels // len(chans))
    ch = np.tile(ctx.init_chans([c[0] for c in chans], [c[1] for c in chans],
                                [c[2] for c in chans]), reps)[:a.channels]
    return time_pair(a, ctx, rec, 0, len(rec) // 2, ch, gc.E1T_EPOCH, a.epochs)


def l3t(a):
    import l3_scenarios as L3
    IF, prn, cp, f0, _ = L3.closed_loop_scene()
    rec = levels(IF, 6)
    ctx = gc.L3tCtx()
    cps = cp + (np.arange(a.channels) % 64)
    ch = ctx.init_chans([prn] * a.channels, cps, [f0] * a.channels)
    return time_pair(a, ctx, rec, 0, len(rec) // 2, ch, gc.L3T_EPOCH, a.epochs)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="sgt_bench,sgt_config4,e1t,l3t")
    ap.add_argument("--channels", type=int, default=1024)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--int8-only", action="store_true")
    ap.add_argument("--int16", action="store_true", help="time int16 records as well")
    a = ap.parse_args()
    if gc.device_count() < 1:
        raise SystemExit("ftrack_packed_time: no HIP device visible")
    run = {"sgt_bench": lambda: sgt_bench(a, 256), "sgt_config4": lambda: sgt_bench(a, 1),
           "e1t": lambda: e1t(a), "l3t": lambda: l3t(a)}
    formats = ["int8"] + ([] if a.int8_only else ["packed"]) + (["int16"] if a.int16 else [])
    out = {"lib": os.path.realpath(gc.LIB_PATH), "formats": formats}
    for s in a.shapes.split(","):
        out[s] = run[s]()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
