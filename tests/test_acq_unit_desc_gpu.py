"""GPU: the unit descriptors of the compiled fp64 correlation kernel.

acq64_corr_kernel reads one descriptor per workgroup (rows, shift digits, output slot),
written by acq64_unit_desc_kernel in every correlate call from the caller's tables.
Held here: tables that are permuted and repeat a code, against the generic engine;
tables whose contents change behind the same device pointers; records and clamped
per-group records; the non-coherent mode and the 400-thread 16 000 plan against the
oracle; and a row with two exactly equal maxima (first index on ties).
"""
import numpy as np
import pytest

import acq_oracle as A
from test_acq_gpu import check_rows

pytestmark = pytest.mark.gpu

FS, N = 16.368e6, 16368
SIGS = [dict(system=0, prn=9, code_phase=500.5, doppler=1500.0, cn0=47.0),
        dict(system=0, prn=23, code_phase=77.0, doppler=-1000.0, cn0=46.0)]
# 500 Hz steps on a 1 kHz fs/N grid: both spectrum classes; the negative frequency
# has a negative shift (m = -2, stored mod N)
FREQS = np.concatenate([2.42e6 + 500.0 * np.arange(-3, 4), [-1500.0]])


@pytest.fixture(scope="module")
def scene(gpu):
    IF = gpu.ifgen(2 * N, SIGS, fs=FS, seed=0x5EED0090)
    codes = np.stack([A.make_ca_table_row(p, FS) for p in (9, 4, 23)])
    return IF, codes


def test_permuted_and_repeated_maps_match_generic_engine(gpu, scene, monkeypatch):
    IF, codes = scene
    gcode = [2, 0, 2]
    gf = np.array([[6, 0, 7], [1, 5, 2], [7, 4, 1]], np.int32)
    out = []
    for generic in ("0", "1"):
        monkeypatch.setenv("GNSSCORR_ACQ_GENERIC", generic)
        ctx = gpu.AcqCtx(FS, N, max_freqs=16, max_blocks=2, max_codes=3)
        ctx.set_codes(codes)
        out.append(ctx.search(IF, 2, FREQS, gcode, gf, spc=16))
    (r0, w0), (r1, w1) = out
    for k in ("argmax", "block"):
        assert (w0[k] == w1[k]).all(), k
    for k in ("bin", "code_phase"):
        assert (r0[k] == r1[k]).all(), k
    for k in ("peak", "second"):
        rel = np.abs(w0[k] - w1[k]) / w0["peak"]
        print(f"[unit desc vs generic] {k} max rel diff {rel.max():.3e}")
        assert rel.max() < 1e-9
    assert np.allclose(r0["metric"], r1["metric"], rtol=1e-9)
    # groups 0 and 2 search the same code: where they share a bin the rows agree
    assert w0[0][2].tobytes() == w0[2][0].tobytes()


def _dev_search(gpu, ctx, d_gc, d_gf, d_freqs, G, B):
    d_rows = gpu.DevBuf(G * B * gpu.ACQ_ROW.itemsize)
    d_res = gpu.DevBuf(G * gpu.ACQ_RESULT.itemsize)
    ctx.correlate_dev(2, d_freqs.ptr, G, B, d_gc.ptr, d_gf.ptr)
    ctx.select_dev(G, B, d_freqs.ptr, d_gf.ptr, d_rows.ptr, d_res.ptr)
    ctx.sync()
    return d_res.download(gpu.ACQ_RESULT).tobytes(), d_rows.download(gpu.ACQ_ROW).tobytes()


def test_same_pointers_new_contents(gpu, scene):
    IF, codes = scene
    G, B = 2, 3
    tabs = [(np.array([0, 2], np.int32), np.array([[4, 1, 6], [2, 5, 0]], np.int32)),
            (np.array([2, 1], np.int32), np.array([[1, 7, 3], [6, 0, 4]], np.int32))]
    d_if = gpu.DevBuf.from_array(IF)
    d_freqs = gpu.DevBuf.from_array(FREQS)

    def fresh():
        ctx = gpu.AcqCtx(FS, N, max_freqs=16, max_blocks=2, max_codes=3)
        ctx.set_codes(codes)
        ctx.spectra_dev(d_if.ptr, 2, len(FREQS), d_freqs.ptr)
        return ctx

    ctx = fresh()
    d_gc, d_gf = gpu.DevBuf.from_array(tabs[0][0]), gpu.DevBuf.from_array(tabs[0][1])
    first = _dev_search(gpu, ctx, d_gc, d_gf, d_freqs, G, B)   # ends on a stream sync
    d_gc.upload(tabs[1][0])
    d_gf.upload(tabs[1][1])
    second = _dev_search(gpu, ctx, d_gc, d_gf, d_freqs, G, B)
    ref = _dev_search(gpu, fresh(), gpu.DevBuf.from_array(tabs[1][0]),
                      gpu.DevBuf.from_array(tabs[1][1]), d_freqs, G, B)
    assert second == ref
    assert first != second


def test_records_and_clamped_group_records(gpu, scene):
    _, codes = scene
    recs = [gpu.ifgen(2 * N, [SIGS[r]], fs=FS, seed=0x5EED0091 + r) for r in range(2)]
    gcode, gf = [2, 0], np.array([[6, 1], [5, 2]], np.int32)
    single = gpu.AcqCtx(FS, N, max_freqs=16, max_blocks=2, max_codes=3)
    single.set_codes(codes)
    ref = [single.search(x, 2, FREQS, gcode, gf) for x in recs]

    def batch():
        ctx = gpu.AcqCtx(FS, N, max_freqs=16, max_blocks=4, max_codes=3)
        ctx.set_codes(codes)
        ctx.set_records(2)
        return ctx

    res, rows = batch().search(np.concatenate(recs), 2, FREQS, gcode, gf)
    for r in range(2):
        assert res[r].tobytes() == ref[r][0].tobytes(), f"record {r} results"
        assert rows[r].tobytes() == ref[r][1].tobytes(), f"record {r} rows"
    # per-group records: an entry below 0 and one past the last record are clamped
    out = []
    for tab in ([-3, 7], [0, 1]):
        ctx = batch()
        d_rec = gpu.DevBuf.from_array(np.array(tab, np.int32))
        ctx.set_group_records(d_rec)
        out.append(ctx.search(np.concatenate(recs), 2, FREQS, gcode, gf))
    assert out[0][0].tobytes() == out[1][0].tobytes()
    assert out[0][1].tobytes() == out[1][1].tobytes()
    for g in range(2):   # group g on record g
        assert out[1][1][g].tobytes() == ref[g][1][g].tobytes()


@pytest.mark.parametrize("fs,n,mode", [(16.368e6, 16368, "noncoherent"),
                                       (16.0e6, 16000, "noncoherent"),
                                       (16.0e6, 16000, "best")])
def test_modes_and_plans_vs_oracle(gpu, fs, n, mode):
    """The 16 000 plan runs 400 of its workgroup's threads (the last wave's upper lanes
    have a thread index at or above T)."""
    nc = mode == "noncoherent"
    nb = 3 if nc else 2
    IF = gpu.ifgen(nb * n, SIGS, fs=fs, seed=0x5EED0093)
    codes = np.stack([A.make_ca_table_row(p, fs) for p in (23, 9)])
    freqs = 2.42e6 + 500.0 * np.arange(-3, 4)
    gf = np.array([[1, 6], [6, 3]], np.int32)       # -1000 Hz and +1500 Hz among them
    ctx = gpu.AcqCtx(fs, n, max_freqs=8, max_blocks=nb, max_codes=2)
    ctx.set_codes(codes)
    res, rows = ctx.search(IF, nb, freqs, [0, 1], gf,
                           mode=gpu.ACQ_NONCOHERENT if nc else gpu.ACQ_BEST_OF_BLOCKS)
    ref, ref_rows = A.acquire(IF, fs, codes, freqs, gf, n_blocks=nb, noncoherent=nc,
                              return_rows=True)
    if nc:          # the non-coherent rows carry no block choice
        for rr in ref_rows:
            for r in rr:
                r["block"] = -1
    check_rows(res, rows, ref, ref_rows, True, label=f"unit-desc-{n}-{mode}")


def test_tie_rule_first_index_of_two_equal_maxima(gpu, scene):
    """One row whose two largest powers are exactly equal: a noise-free record at zero
    frequency holding one PRN at code phases p and p + N/2 with equal amplitude.

    The fp64 oracle (numpy's FFT) does not give the two peaks bit-equal: on the CPU they
    come out 120825760000.0 and 120825759999.99995 (printed below).  So the tie is taken
    from the compiled plan's own dumped power row, which must show more than one sample
    at the maximum (the shift N/2 = 8184 is 0 mod 33 and mod 31: it lives in the radix-16
    digit alone, where the twiddles are +-1 and +-i).  Then, as acq_peak.h defines:
    argmax is the smaller index, peak the tied value, and second the other peak, which
    lies outside the window."""
    _, codes = scene
    spc, p = 16, 300
    c = codes[0].astype(np.int64)
    x = np.roll(c, p) + np.roll(c, p + N // 2)
    IF = np.zeros((N, 2), np.int8)
    IF[:, 0] = 20 * x
    IF = IF.reshape(-1)
    ora = A.power_rows(IF, FS, codes[0], 0.0, n_blocks=1)[0]
    print(f"[tie rule] oracle peaks {ora[p]!r} {ora[p + N // 2]!r}, "
          f"bit-equal: {ora[p] == ora[p + N // 2]}")
    ctx = gpu.AcqCtx(FS, N, max_freqs=2, max_blocks=1, max_codes=3)
    ctx.set_codes(codes)
    res, rows = ctx.search(IF, 1, [0.0], [0], [[0]], spc=spc)
    row = ctx.power_row(IF, 1, 0, 0.0, 0)
    tied = np.flatnonzero(row == row.max())
    print(f"[tie rule] dumped row: maximum {row.max()!r} at {tied.tolist()}")
    assert len(tied) > 1, "the dumped row has no exact tie at its maximum"
    assert tied.tolist() == [p, p + N // 2]
    got = rows[0][0]
    assert int(got["argmax"]) == p                          # the first index
    assert got["peak"].tobytes() == row[p].tobytes()
    # the other peak is outside the open window (argmax - spc, argmax + spc)
    d = (np.arange(N) - p) % N
    second = row[(d >= spc) & (d <= N - spc)].max()
    assert second == row[p + N // 2] == row[p]
    assert got["second"].tobytes() == second.tobytes()
