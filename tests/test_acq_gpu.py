"""GPU parity: HIP acquisition vs the fp64 acquisition.sci oracle.

Reference: POSTPROCESSING_SCILAB_RECEIVERS/GPS/L1/acquisition.sci:46-192 and
GLONASS/L1/acquisition.sci:46-198, restated in oracle/acq_oracle.py.

Two precisions (gnsscorr_acq_cfg.precision):
  * F64 -- the reference's own arithmetic (Scilab doubles).  Tolerances are the
    north_star contract, 1e-6 relative, on every power, row peak, second peak
    and metric (observed errors are ~1e-13 and are printed); code phase,
    frequency bin and chosen block must equal the oracle's unconditionally.
  * F32 -- the single-precision fast path: powers within 2e-5 of the row max,
    peaks 1e-4, decisions exact whenever the oracle's winner is clear of the
    runner-up (ties in noise can resolve either way in fp32).
"""
import numpy as np
import pytest

import acq_oracle as A

pytestmark = pytest.mark.gpu
FS = 16.368e6
N = 16368
F64_TOL = 1e-6          # north_star: within 1e-6 relative on floating-point results
F64_CLASS = 1e-9        # and genuinely double precision (fp32 anywhere would show ~1e-6)


def _sig(prn, cp, dop, cn0=50.0, data=0):
    return dict(system=0, prn=prn, code_phase=cp, doppler=dop, cn0=cn0, data_bits=data)


@pytest.fixture(scope="module", params=["f64", "f32"])
def acq(request, gpu):
    prec = gpu.ACQ_F64 if request.param == "f64" else gpu.ACQ_F32
    ctx = gpu.AcqCtx(FS, N, max_freqs=1024, max_blocks=10, max_codes=40, precision=prec)
    codes = np.stack([A.make_ca_table_row(p, FS) for p in range(1, 33)] +
                     [A.make_st_table_row(FS)])
    ctx.set_codes(codes)
    return ctx, codes


def _is64(ctx):
    return ctx.precision == 0


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def check_rows(res, rows, ref, ref_rows, f64, tol=1e-4, label=""):
    """Row statistics and per-group results against the oracle; returns the
    largest relative error seen (peaks, second peaks, metrics)."""
    worst = 0.0
    for g in range(len(ref)):
        for b, rr in enumerate(ref_rows[g]):
            r = rows[g, b]
            if f64:
                e = max(_rel(r["peak"], rr["peak"]), _rel(r["second"], rr["second"]))
                worst = max(worst, e)
                assert e <= F64_TOL, (label, g, b, e)
                assert r["argmax"] == rr["argmax"], (label, g, b)
                assert r["block"] == rr["block"], (label, g, b)
            else:
                assert abs(r["peak"] - rr["peak"]) <= tol * rr["peak"], (g, b)
                assert abs(r["second"] - rr["second"]) <= tol * rr["peak"], (g, b)
        rg = ref[g]
        if f64:
            e = max(_rel(res[g]["peak"], rg["peak"]), _rel(res[g]["second"], rg["second"]),
                    _rel(res[g]["metric"], rg["metric"]))
            worst = max(worst, e)
            assert e <= F64_TOL, (label, g, e)
            assert res[g]["bin"] == rg["bin"], (label, g)
            assert res[g]["code_phase"] == rg["code_phase"], (label, g)
        else:
            assert abs(res[g]["peak"] - rg["peak"]) <= tol * rg["peak"]
            assert abs(res[g]["metric"] - rg["metric"]) <= 10 * tol * rg["metric"]
            pk = np.array([r["peak"] for r in ref_rows[g]])
            srt = np.sort(pk)
            if srt[-1] - srt[-2] > 1e-3 * srt[-1]:
                assert res[g]["bin"] == rg["bin"], g
            if rg["metric"] > 1.01:
                assert res[g]["code_phase"] == rg["code_phase"], g
    if f64:
        print(f"[{label}] max relative error vs fp64 oracle: {worst:.3e}")
        assert worst < F64_CLASS, (label, worst)
    return worst


# backwards-compatible name used by other test modules (fp32 tolerances)
def _check_rows(res, rows, ref, ref_rows, tol=1e-4):
    return check_rows(res, rows, ref, ref_rows, False, tol)


def test_power_rows_match_oracle(gpu, acq):
    ctx, codes = acq
    IF = gpu.ifgen(2 * N, [_sig(7, 100.5, 1234.0), _sig(12, 800.0, -3000.0)], fs=FS, seed=3)
    worst = 0.0
    for code, freq, blk in [(6, 2.42e6 + 1000, 0), (6, 2.42e6 + 1234, 1), (11, 2.42e6 - 3000, 0),
                            (0, 2.42e6, 1), (32, 1.0e6, 0)]:
        got = ctx.power_row(IF, 2, blk, freq, code)
        ref = A.power_rows(IF, FS, codes[code], freq)[blk]
        err = np.abs(got - ref).max() / ref.max()
        if _is64(ctx):
            # every cell, relative to the row maximum, and the peak to itself
            assert err < F64_TOL, (code, freq, blk, err)
            assert _rel(got.max(), ref.max()) < F64_TOL
            worst = max(worst, err)
        else:
            assert err < 2e-5, (code, freq, blk, err)
        assert np.argmax(got) == np.argmax(ref)
    if _is64(ctx):
        print(f"[power rows] max |P - P_ref| / max P_ref = {worst:.3e}")
        assert worst < F64_CLASS


def test_small_search_vs_oracle(gpu, acq):
    ctx, codes = acq
    IF = gpu.ifgen(2 * N, [_sig(3, 200.25, 2500.0), _sig(9, 17.0, -4500.0, data=1)], fs=FS,
                   seed=11)
    freqs = A.gps_bins(2.42e6, 10)                     # 21 bins @ 500 Hz
    gf = np.tile(np.arange(len(freqs)), (4, 1))
    gcode = np.array([2, 8, 0, 31])                    # PRNs 3, 9, 1, 32
    res, rows = ctx.search(IF, 2, freqs, gcode, gf)
    ref, ref_rows = A.acquire(IF, FS, codes, freqs, gf, group_code=gcode, return_rows=True)
    check_rows(res, rows, ref, ref_rows, _is64(ctx), label="small")
    assert res[0]["metric"] > 3 and res[1]["metric"] > 3


def test_cold_start_32x41_config2(gpu, acq):
    """BASELINE config 2: 32 PRN x 41 bins (+-10 kHz @ 500 Hz), 1 ms coherent, 8 planted."""
    ctx, codes = acq
    rng = np.random.default_rng(2)
    planted = [int(p) for p in rng.choice(np.arange(1, 33), 8, replace=False)]
    sigs = [_sig(p, float(rng.uniform(0, 1023)), float(rng.uniform(-5000, 5000)), 46.0, 1)
            for p in planted]
    IF = gpu.ifgen(2 * N, sigs, fs=FS, seed=0x5EED0002)
    freqs = A.gps_bins(2.42e6, 20)                     # 41 bins
    gf = np.tile(np.arange(41), (32, 1))
    res, rows = ctx.search(IF, 2, freqs, np.arange(32), gf)
    ref, ref_rows = A.acquire(IF, FS, codes[:32], freqs, gf, return_rows=True)
    check_rows(res, rows, ref, ref_rows, _is64(ctx), label="config2")
    for p in planted:
        assert res[p - 1]["metric"] > 2.5, p
        assert res[p - 1]["code_phase"] == ref[p - 1]["code_phase"]
        assert res[p - 1]["bin"] == ref[p - 1]["bin"]


def test_noncoherent_10ms(gpu, acq):
    ctx, codes = acq
    IF = gpu.ifgen(10 * N, [_sig(21, 600.0, 700.0, 40.0)], fs=FS, seed=21)
    freqs = A.gps_bins(2.42e6, 4)
    gf = np.tile(np.arange(len(freqs)), (2, 1))
    gcode = np.array([20, 4])
    res, rows = ctx.search(IF, 10, freqs, gcode, gf, mode=gpu.ACQ_NONCOHERENT)
    ref, ref_rows = A.acquire(IF, FS, codes, freqs, gf, group_code=gcode, n_blocks=10,
                              noncoherent=True, return_rows=True)
    for rr in ref_rows:          # the non-coherent rows carry no block choice
        for r in rr:
            r["block"] = -1
    check_rows(res, rows, ref, ref_rows, _is64(ctx), label="noncoherent")


def test_glonass_fch_search(gpu, acq):
    """GLONASS L1OF: one ST code, per-FCH carrier IF + k*562.5 kHz (acquisition.sci:105-108)."""
    ctx, codes = acq
    sigs = [dict(system=1, fch=-3, code_phase=120.0, doppler=1500.0, cn0=50.0),
            dict(system=1, fch=4, code_phase=400.0, doppler=-2000.0, cn0=50.0)]
    IF = gpu.ifgen(2 * N, sigs, fs=FS, if_glo=1.0e6, seed=4)
    fchs = np.arange(-7, 7)
    band = 10
    per = A.gps_bins(0.0, band)                        # relative bins
    freqs = np.concatenate([1.0e6 + k * 0.5625e6 + per for k in fchs])
    B = len(per)
    gf = np.arange(len(fchs) * B).reshape(len(fchs), B)
    gcode = np.full(len(fchs), 32)
    res, rows = ctx.search(IF, 2, freqs, gcode, gf)
    ref, ref_rows = A.acquire(IF, FS, codes, freqs, gf, group_code=gcode, return_rows=True)
    check_rows(res, rows, ref, ref_rows, _is64(ctx), label="glonass")
    best = [int(fchs[i]) for i in np.argsort([-r["metric"] for r in res])[:2]]
    assert sorted(best) == [-3, 4]


def test_search_rejects_bad_tables(gpu, acq):
    ctx, _ = acq
    IF = np.zeros(4 * N, np.int8)
    with pytest.raises(gpu.GnssCorrError):
        ctx.search(IF, 2, np.array([2.42e6]), [99], [[0]])
    with pytest.raises(gpu.GnssCorrError):
        ctx.search(IF, 2, np.array([2.42e6]), [0], [[5]])


def test_zero_if_rows(gpu, acq):
    """An all-zero IF gives all-zero power rows: peak 0, argmax 0 (first index of the
    maximum, as Scilab's max), metric 0/0 = nan like the reference's division."""
    ctx, _ = acq
    IF = np.zeros(4 * N, np.int8)
    res, rows = ctx.search(IF, 2, A.gps_bins(2.42e6, 2), [0], [np.arange(5)])
    assert np.all(rows["peak"] == 0.0) and np.all(rows["argmax"] == 0)
    assert res[0]["code_phase"] == 1 and res[0]["bin"] == 0


def test_two_precisions_in_one_process_do_not_disturb_each_other(gpu):
    """The fp32 and the fp64 engine are separate code objects, each with its own constant
    tables and its own lazy load (acq32_preload / acq64_preload at create).  Whatever order
    the contexts are created in and however their searches interleave, each precision
    returns byte for byte what it returned when it ran alone.  The code is compared with
    itself only; the tests above hold both engines to the oracle."""
    IF = gpu.ifgen(2 * N, [_sig(7, 100.5, 1000.0)], fs=FS, seed=5)
    codes = np.stack([A.make_ca_table_row(p, FS) for p in (7, 9)])
    freqs = 2.42e6 + np.array([0.0, 500.0, 1000.0])    # bins 0 and 2 share a spectrum class
    gf = np.tile(np.arange(3), (2, 1))
    modes = (gpu.ACQ_BEST_OF_BLOCKS, gpu.ACQ_NONCOHERENT)

    def make(prec):
        ctx = gpu.AcqCtx(FS, N, max_freqs=3, max_blocks=2, max_codes=2, precision=prec)
        ctx.set_codes(codes)
        return ctx

    def run(ctx, mode):
        res, rows = ctx.search(IF, 2, freqs, [0, 1], gf, spc=16, mode=mode)
        return rows.tobytes(), res.tobytes()

    c32, c64 = make(gpu.ACQ_F32), make(gpu.ACQ_F64)
    alone = {(ctx.precision, m): run(ctx, m) for ctx in (c32, c64) for m in modes}
    c32.close()
    c64.close()
    assert alone[gpu.ACQ_F32, modes[0]] != alone[gpu.ACQ_F32, modes[1]]   # the modes differ
    c64, c32 = make(gpu.ACQ_F64), make(gpu.ACQ_F32)
    for m in modes:
        for ctx in (c32, c64):
            assert run(ctx, m) == alone[ctx.precision, m], (ctx.precision, m)
    c32.close()
    c64.close()


def test_bad_precision_or_size_rejected(gpu):
    with pytest.raises(gpu.GnssCorrError):
        gpu.AcqCtx(FS, N, precision=7)
    with pytest.raises(gpu.GnssCorrError):
        gpu.AcqCtx(16.0e6, 16000, precision=gpu.ACQ_F32)   # fp32 path: 16368 only
    with pytest.raises(gpu.GnssCorrError):
        gpu.AcqCtx(0.032e6, 32)                             # below the generic fp64 range
    gpu.AcqCtx(16.1e6, 16100).close()                       # any other N: Bluestein (generic)
