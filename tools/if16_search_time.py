"""int16 against int8 records in the fp64 search ("int16 records").

search_dev on a device-resident record between HIP events on the context's stream, as
bench.py times its searches; the int8 and the int16 launch (the same levels stored as
int16) alternate, `--warmup` untimed rounds first, then `--runs` timed ones: min / median /
max per format and the ratio of the medians.  Both formats must give byte-equal rows.

Shapes: `headline` N = 16368 at 16.368 Msps (the compiled plan), `n2048` N = 2048 at
2.048 Msps (the generic engine); --codes PRNs x --bins 500 Hz bins x 2 blocks each.

--int8-only times the int8 launches alone: with GNSSCORR_LIB set to another build of the
library this is the A/B of the int8 path.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("gnss-sdr.ru_amd", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, p))
import acq_oracle as A  # noqa: E402
import gnsscorr as gc  # noqa: E402

SHAPES = {"headline": (16.368e6, 16368), "n2048": (2.048e6, 2048)}


def time_shape(a, fs, n):
    G, B = a.codes, a.bins
    IF = gc.ifgen(2 * n, [dict(system=0, prn=3, code_phase=210.0, doppler=1000.0, cn0=48.0)],
                  fs=fs, seed=7)
    freqs = 2.42e6 + 500.0 * (np.arange(B) - B // 2)
    ctx = gc.AcqCtx(fs, n, max_freqs=B, max_blocks=2, max_codes=G)
    ctx.set_codes(np.stack([A.make_ca_table_row(p, fs) for p in range(1, G + 1)]))
    bufs = {"int8": (gc.DevBuf.from_array(IF), gc.iq_flags(True))}
    if not a.int8_only:
        bufs["int16"] = (gc.DevBuf.from_array(IF.astype(np.int16)), gc.iq_flags(True, int16=True))
    d_f = gc.DevBuf.from_array(freqs)
    d_gc = gc.DevBuf.from_array(np.arange(G, dtype=np.int32))
    d_gf = gc.DevBuf.from_array(np.tile(np.arange(B, dtype=np.int32), (G, 1)))
    d_rows = gc.DevBuf(G * B * gc.ACQ_ROW.itemsize)
    d_res = gc.DevBuf(G * gc.ACQ_RESULT.itemsize)
    e0, e1 = gc.Event(), gc.Event()
    ms = {k: [] for k in bufs}
    last = {}
    spc = max(2, int(round(fs / 1.023e6)))
    for r in range(a.warmup + a.runs):
        for k, (d_if, iq) in bufs.items():
            e0.record(ctx.stream)
            ctx.search_dev(d_if.ptr, 2, B, d_f.ptr, G, B, d_gc.ptr, d_gf.ptr, d_rows.ptr,
                           d_res.ptr, spc=spc, iq=iq)
            e1.record(ctx.stream)
            ctx.sync()
            if r >= a.warmup:
                ms[k].append(e0.elapsed_ms(e1))
            last[k] = d_rows.download(gc.ACQ_ROW)
    out = {k: dict(min=round(min(v), 4), median=round(float(np.median(v)), 4),
                   max=round(max(v), 4)) for k, v in ms.items()}
    if "int16" in out:
        assert last["int16"].tobytes() == last["int8"].tobytes(), "int16 differs from int8"
        out["int16_over_int8"] = round(out["int16"]["median"] / out["int8"]["median"], 4)
    out.update(n=n, codes=G, bins=B, blocks=2)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="headline,n2048")
    ap.add_argument("--codes", type=int, default=32)
    ap.add_argument("--bins", type=int, default=41)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--int8-only", action="store_true")
    a = ap.parse_args()
    if gc.device_count() < 1:
        raise SystemExit("if16_search_time: no HIP device visible")
    out = {"lib": os.path.realpath(gc.LIB_PATH),
           "formats": ["int8"] if a.int8_only else ["int8", "int16"]}
    for s in a.shapes.split(","):
        out[s] = time_shape(a, *SHAPES[s])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
