"""CPU: the per-row tables of the GPS-SDR int16 acquisition oracle
(sdro_acq_strong_rows / _medium_rows / _weak_rows, oracle/sdr_acq.c).

The GPU tests in test_sdr_acq_rows_gpu.py compare the kernels' whole per-row
tables with these, so the tables themselves are pinned here:
  * scanned with the reference's strict '>' from 0 they give the results of
    sdro_acq_strong / sdro_acq_medium / sdro_acq_weak and the committed results
    of the reference build (tests/golden/sdr_acq.npz, sdr_acq_mw.npz);
  * one lcv at a time (4 rows, 8 for weak) their winner is the compiled
    reference's (oracle/_ref/libsdr_ref.so), at the padding limits lcv = +-100
    and around the sign change -- as fine as the reference's interface allows;
  * the inputs the GPU tests use for the saturating mode do change rows between
    saturate and wrap (and the make_buffer inputs of the older tests do not);
  * the inputs for the tie and column-shift tests have the ties and the
    boundary crossings they are meant to have.

Reference: REALTIME_RECEIVERS/GPS/GPS_SDR_REAL_TIME_GPS_RECEIVER objects/
acquisition.cpp:244-301, :309-425, :433-570.
"""
import os

import numpy as np
import pytest

import sdr_oracle as S
import sdr_rows_cases as K

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
need_ref = pytest.mark.skipif(not S.have_ref(), reason="reference build (oracle/_ref) absent")


@pytest.fixture(scope="module")
def o(oracle):
    return S.OracleSDR()


@pytest.fixture(scope="module")
def codes():
    return np.load(os.path.join(GOLD, "sdr_prn_codes.npz"))["prn_codes"]


def _same(a, b):
    assert a.dtype == b.dtype == S.RESULT and a.tobytes() == b.tobytes(), (a, b)


# ---- the scan of a table is the search ---------------------------------------------
def test_strong_table_scan_is_the_search(o, codes):
    f = np.load(os.path.join(GOLD, "sdr_acq.npz"))
    svs, fif = f["svs"], float(f["fif"])
    for b, res, nar in zip(f["buffers"], f["res"], f["res_narrow"]):
        rows4 = o.prep_if(b, fif)
        for (dmin, dmax), gold in (((-15000, 15000), res), ((-3000, 5000), nar),
                                   ((-999, 1999), None), ((-100000, -99000), None),
                                   ((100000, 101000), None)):
            t = o.strong_rows(rows4, codes, svs, dmin, dmax)
            assert t.shape == (len(svs), S.n_rows("strong", dmin, dmax), 2)
            got = S.scan_rows("strong", t, svs, dmin)
            _same(got, o.acq_strong(b, codes, svs, dmin, dmax, fif))
            if gold is not None:
                _same(got, gold.astype(S.RESULT))


def test_medium_weak_table_scan_is_the_search(o, codes):
    f = np.load(os.path.join(GOLD, "sdr_acq_mw.npz"))
    buf, fif = f["buffer"].astype(np.int16), float(f["fif"])
    svs = np.array([4, 9, 25], np.int32)       # the two planted PRNs and an absent one
    rows = o.new_rows()
    o.prep_rows(rows, buf, 10, fif)
    t = o.search_rows("medium", rows, codes, svs)
    assert t.shape == (3, 124, 2)
    _same(S.scan_rows("medium", t, svs, -15000), f["medium_fresh"][svs].astype(S.RESULT))
    o.prep_rows(rows, buf, 310, fif)
    wsvs = np.array([s for s in f["weak_svs"] if s in (4, 25)], np.int32)
    at = [list(f["weak_svs"]).index(s) for s in wsvs]
    t = o.search_rows("weak", rows, codes, wsvs, -5000, 5000)
    assert t.shape == (len(wsvs), 80, 2)
    _same(S.scan_rows("weak", t, wsvs, -5000), f["weak"][at].astype(S.RESULT))
    for dmin, dmax in ((-2000, 0), (0, 1000), (-999, 1999)):
        t = o.search_rows("weak", rows, codes, wsvs, dmin, dmax)
        _same(S.scan_rows("weak", t, wsvs, dmin),
              o.acq_search("weak", rows, codes, wsvs, dmin, dmax))
    o.prep_rows(rows, buf, 10, fif)
    t = o.search_rows("medium", rows, codes, svs, -7000, 3000)
    _same(S.scan_rows("medium", t, svs, -7000), f["medium_after_weak"][svs].astype(S.RESULT))
    for dmin, dmax in ((-999, 1999), (100000, 100000), (-100000, -99000)):
        t = o.search_rows("medium", rows, codes, svs, dmin, dmax)
        _same(S.scan_rows("medium", t, svs, dmin),
              o.acq_search("medium", rows, codes, svs, dmin, dmax))


def test_scan_keeps_the_first_of_equal_rows():
    t = np.array([[[5, 1], [9, 2], [9, 3], [0, 0], [9, 4]]], np.int32)
    r = S.scan_rows("strong", t, [3], -1000)[0]
    assert (r["row"], r["magnitude"], r["code_phase"], r["doppler"]) == (1, 9, 2046, -750)
    z = S.scan_rows("weak", np.zeros((1, 8, 2), np.int32), [3], 0)[0]
    assert z["success"] == 0 and z["magnitude"] == 0 and z["row"] == 0


# ---- one lcv at a time against the compiled reference -----------------------------
def _level_buffers(ms):
    return (S.make_long_buffer([dict(prn=12, code_phase=321.5, doppler=-600.0, amp=2.0)], ms,
                               seed=61),
            K.uniform(32768, ms, 62))


@need_ref
@pytest.mark.parametrize("lcv", K.LCVS)
def test_strong_rows_vs_reference_build(o, lcv):
    ref = S.RefSDR()
    codes, svs = ref.prn_codes(), [11, 0, 30]
    for buf in _level_buffers(1):
        dmin, dmax = K.one_lcv("strong", lcv)
        t = o.strong_rows(o.prep_if(buf), codes, svs, dmin, dmax)
        assert t.shape == (3, 4, 2)
        _same(S.scan_rows("strong", t, svs, dmin), ref.acq_strong(buf, svs, dmin, dmax))


@need_ref
@pytest.mark.parametrize("lcv", K.LCVS)
def test_medium_weak_rows_vs_reference_build(o, lcv):
    ref = S.RefSDR()
    codes, svs = ref.prn_codes(), [11, 30]
    for buf in _level_buffers(310):
        sess, rows = S.RefAcqSession(ref), o.new_rows()
        sess.prep(buf, 310)
        o.prep_rows(rows, buf, 310)
        for kind, n in (("weak", 8), ("medium", 4)):
            dmin, dmax = K.one_lcv(kind, lcv)
            t = o.search_rows(kind, rows, codes, svs, dmin, dmax)
            assert t.shape == (2, n, 2)
            _same(S.scan_rows(kind, t, svs, dmin), sess.search(kind, svs, dmin, dmax))


# ---- the saturating mode decides something ----------------------------------------
def _sat_counts(o, codes, buf):
    """Differing (saturate vs wrap) prep cells and strong / medium / weak rows."""
    rw, rs = o.new_rows(), o.new_rows()
    o.prep_rows(rw, buf, 310)
    o.prep_rows(rs, buf, 310, saturate=True)
    out = dict(prep=int((rw != rs).any(axis=2).sum()))
    p4w, p4s = o.prep_if(buf[:K.N]), o.prep_if(buf[:K.N], saturate=True)
    out["prep_if"] = int((p4w != p4s).any(axis=2).sum())
    a = o.strong_rows(p4w, codes, [0])
    b = o.strong_rows(p4s, codes, [0], saturate=True)
    out["strong"] = (int((a != b).any(axis=2).sum()), a.shape[1])
    for kind in ("medium", "weak"):
        a = o.search_rows(kind, rw, codes, [0], *K.one_lcv(kind, 0))
        b = o.search_rows(kind, rs, codes, [0], *K.one_lcv(kind, 0), saturate=True)
        out[kind] = (int((a != b).any(axis=2).sum()), a.shape[1])
    return out


def test_saturation_inputs_change_rows(o, codes):
    """Measured: uniform +-12000 and +-20000 leave the prep identical and change
    8 of 8 weak rows (the shift-9 product); full scale changes all 8192 / 2539520
    prep cells, 120 of 120 strong, 4 of 4 medium and 8 of 8 weak rows; int8-level
    inputs change nothing."""
    for amp, seed in ((12000, 1), (20000, 2)):
        c = _sat_counts(o, codes, K.uniform(amp, 310, seed))
        print(amp, c)
        assert c["prep"] == 0 and c["prep_if"] == 0 and c["strong"][0] == 0
        assert 2 * c["weak"][0] >= c["weak"][1] == 8
    c = _sat_counts(o, codes, K.uniform(32768, 310, 3))
    print("full scale", c)
    assert 2 * c["prep_if"] >= 4 * K.N and 2 * c["prep"] >= 1240 * K.N
    for kind, n in (("strong", 120), ("medium", 4), ("weak", 8)):
        assert 2 * c[kind][0] >= c[kind][1] == n
    for name, buf in (("make_buffer amp 60", S.make_long_buffer(
            [dict(prn=3, code_phase=10.0, doppler=500.0, amp=36.0)], 310, seed=3,
            amp_noise=60.0)), ("planted", K.planted()[0])):
        c = _sat_counts(o, codes, buf)
        print(name, c)
        assert c["prep"] == c["prep_if"] == 0
        assert c["strong"][0] == c["medium"][0] == c["weak"][0] == 0


# ---- the column-shift and tie inputs are what they claim to be --------------------
@pytest.mark.parametrize("rec,lcv", [(0, 100), (1, -100)])
def test_planted_peaks_cross_both_column_boundaries(o, codes, rec, lcv):
    rows = o.new_rows()
    o.prep_rows(rows, K.planted()[rec], 310)
    t = o.search_rows("weak", rows, codes, K.PLANT_SVS, *K.one_lcv("weak", lcv))
    for s, boundary in enumerate((0, 1024)):
        row = int(np.argmax(t[s, :, 0]))
        assert t[s, row, 0] > 3 * np.median(t[s, :, 0])          # the planted signal
        col = int(t[s, row, 1]) % K.N
        cols = K.pass_columns(o, lcv, (row >> 1) & 3, col)
        print(rec, lcv, s, row, col, cols)
        assert len(set(cols)) == 15 and K.straddles(cols, boundary)
    sh = [o.weak_shift(14, lcv, j) for j in range(4)]
    assert (max(sh) == 36 and lcv == 100) or (min(sh) == -37 and lcv == -100)


def test_impulse_rows_repeat(o, codes):
    """A record that is (1000, 0) at sample 0 of every 1-ms block has constant
    spectra, so the circular offset lcv changes nothing: strong and medium rows
    are all equal.  A weak row also depends on lcv through its column shifts;
    rows with equal shifts (all 0 for 0 <= Doppler < 2747 Hz) and the k = 0 / 1
    halves are equal, and the maximum over the range lies among those."""
    t = o.strong_rows(o.prep_if(K.impulse(1)), codes, [13])
    assert (t == (2033480, 90)).all() and t.shape == (1, 120, 2)
    rows = o.new_rows()
    o.prep_rows(rows, K.impulse(310), 310)
    t = o.search_rows("medium", rows, codes, [13], -8000, 8000)
    assert t.shape == (1, 68, 2) and (t == t[0, 0]).all() and t[0, 0, 0] > 0
    t = o.search_rows("weak", rows, codes, [13], *K.IMPULSE_WEAK_RANGE)[0]
    assert t.shape == (136, 2)
    top = np.flatnonzero(t[:, 0] == t[:, 0].max())
    print("weak impulse maximum at rows", top)
    assert list(top) == [60, 61, 68, 69, 76, 77]      # lcv 0, 1, 2 at lcv2 = 2, both k
    assert (t[top] == t[top[0]]).all()


def test_tie_search_finds_rows(o, codes):
    """The GPU tie test's rows: >= 3 strong rows with two or more cells at the
    maximum, one with the first cell in a higher thread than a later one; the
    oracle's index is the first such cell."""
    for kind in ("strong", "medium", "weak"):
        ties = K.ties(kind)
        print(kind, [(f["seed"], f["sv"], f["lcv"], f["lcv2"], f["k"], f["mag"], f["cells"][:4],
                      f["inverted"]) for f in ties])
        for f in ties:
            assert len(f["cells"]) >= 2 and f["cells"][0] == min(f["cells"])
    s = K.ties("strong")
    assert len(s) >= 3 and any(f["inverted"] for f in s)
