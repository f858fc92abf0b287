"""CPU tier of GLONASS L3OC: the ranging codes (gnsscorr_l3_code), the host-only entry
points of the tracker (gnsscorr_l3t_*), the second-peak range of
GLONASS/L3/acquisition.sci:134-153 in the 0-based form the library documents against the
1-based restatement (tests/l3_scenarios.py), and the decidability of the closed-loop
scene the GPU tier runs.
"""
import ctypes as C

import numpy as np
import pytest

import l3_scenarios as L3

EINVAL = -1


# ---- codes ----------------------------------------------------------------------------
def test_l3_code_equals_the_restatement_for_all_64_ids(gc):
    for i in range(1, 65):
        got = gc.l3_code(i)
        assert got.shape == (10230,) and got.dtype == np.int8
        assert np.array_equal(got, L3.generate_code(i)), i
    for bad in (0, 65, -1):
        with pytest.raises(gc.GnssCorrError):
            gc.l3_code(bad)


def test_the_tables_three_defects(gc):
    """id 32 is all zero; id 31 carries the state of 32, not the ICD state of 31; id 64
    repeats id 63."""
    assert not gc.l3_code(32).any()
    for i in list(range(1, 32)) + list(range(33, 65)):
        assert set(np.unique(gc.l3_code(i))) == {-1, 1}, i

    def icd(n):
        """The code of the plain 7-bit state of n (no table), register-product form."""
        reg2 = [-1.0 * (1 if (n >> (6 - j)) & 1 else -1) for j in range(7)]
        g2 = np.zeros(10230)
        for k in range(10230):
            g2[k] = reg2[6]
            reg2 = [reg2[5] * reg2[6]] + reg2[:6]
        return -(L3._g1() * g2)
    assert np.array_equal(gc.l3_code(30), icd(30))
    assert not np.array_equal(gc.l3_code(31), icd(31))
    assert np.array_equal(gc.l3_code(31), icd(32))
    assert np.array_equal(gc.l3_code(64), gc.l3_code(63))
    assert np.array_equal(gc.l3_code(63), icd(63))


def test_g2_has_period_127_in_every_code(gc):
    """Independent of both implementations: c = -(g1 g2) and g2 repeats after 127 chips,
    so c(i) c(i + 127) = g1(i) g1(i + 127) is the same sequence for every id."""
    first = None
    for i in range(1, 65):
        if i == 32:
            continue
        c = gc.l3_code(i).astype(np.int64)
        p = c[:-127] * c[127:]
        if first is None:
            first = p
            assert len(set(p)) == 2                 # not a constant: G1 does not repeat there
        assert np.array_equal(p, first), i
    # and the ids differ from each other (63 and 64 aside)
    codes = {gc.l3_code(i).tobytes() for i in range(1, 65)}
    assert len(codes) == 63


# ---- host functions -------------------------------------------------------------------
def test_loop_coefs_and_init_chan_equal_the_restatement(gc):
    for kw in (dict(), dict(dllNoiseBandwidth=2.0, dllDampingRatio=0.9, pllNoiseBandwidth=18.0,
                            fllNoiseBandwidth=100.0)):
        cfg = gc.l3t_cfg(**kw)
        s = L3.settings(**kw)
        want = L3.calc_loop_coef(s["dllNoiseBandwidth"], s["dllDampingRatio"], 1.0) + \
            L3.calc_fll_pll_loop_coef(s["pllNoiseBandwidth"], s["fllNoiseBandwidth"], 0.001)
        assert gc.l3t_loop_coefs(cfg) == want
    cfg = gc.l3t_cfg()
    assert (cfg.samp_rate, cfg.if_freq, cfg.nominal_freq) == (24e6, -2.025e6, 1202.025e6)
    assert (cfg.code_freq_basis, cfg.code_length, cfg.dll_spacing) == (10.23e6, 10230, 0.4)
    f0 = -2.025e6 + 1786.0
    ch = gc.l3t_init_chan(cfg, 30, 3002, f0, stream=1, skip=24000000)[0]
    lp = L3.Loop(L3.settings(), 24000000 + 3002 - 1, f0)
    assert ch["code_id"] == 30 and ch["stream"] == 1 and ch["status"] == 0 and ch["n_epochs"] == 0
    assert ch["pos"] == lp.pos
    assert lp.code_freq == 10.23e6                         # the aiding term is times 0
    for f, v in (("rem_code", lp.rem_code), ("rem_carr", lp.rem_carr),
                 ("code_freq", lp.code_freq), ("carr_freq", lp.carr_freq),
                 ("carr_freq_basis", lp.carr_basis), ("old_code_nco", 0.0),
                 ("old_code_error", 0.0), ("old_carr_nco", 0.0), ("old_carr_error", 0.0),
                 ("i1", lp.I1), ("q1", lp.Q1)):
        assert ch[f] == v, f


def test_refusals_on_the_host(gc):
    """PRN 0, 32 and 33, real-sample records and other code lengths: EINVAL before any
    device call (this tier has no device)."""
    L = gc.lib()
    cfg = gc.l3t_cfg()
    out = np.zeros(1, gc.L3T_CHAN)
    for prn in (0, 32, 33, -1):
        assert L.gnsscorr_l3t_init_chan(C.byref(cfg), prn, 0, 0, 1, -2.025e6,
                                        out.ctypes.data) == EINVAL, prn
        assert b"PRN 1..31" in L.gnsscorr_last_error()
    for prn in (1, 31):
        assert L.gnsscorr_l3t_init_chan(C.byref(cfg), prn, 0, 0, 1, -2.025e6, out.ctypes.data) == 0
    for kw in (dict(fileType=1), dict(fileType=3), dict(codeLength=10229),
               dict(dllCorrelatorSpacing=1.0)):
        bad = gc.l3t_cfg(**kw)
        h = C.c_void_p()
        assert L.gnsscorr_l3t_create(C.byref(h), C.byref(bad)) == EINVAL, kw
        assert b"l3t: bad config" in L.gnsscorr_last_error()
        assert not h.value
        assert L.gnsscorr_l3t_init_chan(C.byref(bad), 1, 0, 0, 1, -2.025e6,
                                        out.ctypes.data) == EINVAL
    assert L.gnsscorr_l3t_track(None, None, 0, 0, 1, None, 1, 1, None) == EINVAL
    assert L.gnsscorr_acq_set_peak_period(None, 5) == EINVAL


def test_bins(gc):
    b = gc.l3_bins(-2.025e6, 5)
    assert len(b) == 51 and b[0] == -2.025e6 - 2500.0 and b[-1] == -2.025e6 + 2500.0
    assert np.array_equal(b, L3.bins(L3.settings()))
    assert np.allclose(np.diff(b), 100.0)


# ---- the window rule ------------------------------------------------------------------
def candidates_0b(a, keep, S, s):
    """The 0-based candidate set as include/gnsscorr.h states it."""
    k = np.arange(keep)
    if a <= s:
        m = (k >= a + s) & (k <= S + a - s)
    elif a >= S - s:
        m = (k >= a + s - S) & (k <= a - s)
    else:
        m = (k <= a - s) | ((k >= a + s) & (k <= S - 1))
    return k[m]


@pytest.mark.parametrize("keep,S,s", [(1000, 200, 2), (1000, 200, 7)])
def test_candidate_set_equals_code_phase_range(keep, S, s):
    for a in range(keep):
        want = L3.code_phase_range_1b(a + 1, S, s) - 1
        want = want[want < keep]
        got = candidates_0b(a, keep, S, s)
        assert np.array_equal(got, want), a
        assert len(got) > 0 and a not in got
    # the argmax values the GPU tier plants
    exp = {s: (2 * s, S), s + 1: None, S - s - 1: None, S - s: (0, S - 2 * s), S: (s, S - s),
           keep - 1: (keep - 1 + s - S, keep - 1 - s)}
    for a, rng in exp.items():
        got = candidates_0b(a, keep, S, s)
        if rng is not None:                                   # a linear range
            assert got[0] == rng[0] and got[-1] == rng[1] and len(got) == rng[1] - rng[0] + 1, a
        else:                                                 # two pieces
            assert got[0] == 0 and got[-1] == S - 1 and len(got) == S - 2 * s + 1, a
    assert S in candidates_0b(s, keep, S, s)                 # index S itself is reachable


@pytest.mark.parametrize("keep,S,s", [(1000, 200, 2), (1000, 200, 7)])
def test_the_kernels_predicate_equals_code_phase_range(gc, keep, S, s):
    """in_period_range of csrc/acq_peak.h itself -- the function the statistics kernel
    evaluates -- through its host export, for every argmax and every lag."""
    f = gc.lib().gnsscorr_acq_second_peak_candidate
    for a in range(keep):
        want = L3.code_phase_range_1b(a + 1, S, s) - 1
        got = np.array([k for k in range(keep) if f(k, a, s, keep, S) == 1])
        assert np.array_equal(got, want[want < keep]), a
    # period 0 is the window circular in the row (e1b_scenarios.second_peak's set)
    for a in (0, s, keep - 1):
        d = (np.arange(keep) - a) % keep
        want = np.flatnonzero((d >= s) & (d <= keep - s))
        got = np.array([k for k in range(keep) if f(k, a, s, keep, 0) == 1])
        assert np.array_equal(got, want), a
    for bad in ((keep, 0, s, keep, S), (0, keep, s, keep, S), (0, 0, 0, keep, S),
                (0, 0, s, keep, keep + 1), (0, 0, S // 2, keep, S), (-1, 0, s, keep, 0)):
        assert f(*bad) == EINVAL, bad


# ---- the closed-loop scene ------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    IF, prn, cp, f0, rate = L3.closed_loop_scene()
    s = L3.settings()
    return IF, prn, cp, f0, rate, s, L3.track(IF, s, prn, cp, f0, L3.SCENE_MS)


def test_restatement_tracks_the_synthetic_signal(scene):
    IF, prn, cp, f0, rate, s, r = scene
    assert r["status"] == 0 and len(r["I_P"]) == L3.SCENE_MS
    assert np.abs(r["blksize"] - 24000).max() <= 1
    assert np.abs(r["codeFreq"] - rate).max() < 30.0
    mp, md = np.hypot(r["I_P"], r["Q_P"]), np.hypot(r["I_P2"], r["Q_P2"])
    for m, tag in ((mp, ""), (md, "2")):
        assert (m > np.hypot(r["I_E" + tag], r["Q_E" + tag])).all()
        assert (m > np.hypot(r["I_L" + tag], r["Q_L" + tag])).all()
        assert (m > 0.5 * 12.0 * 24000).all()                # planted amplitude 12 per code
    # 20 ms is the start of the pull-in: the FLL has taken back half of the planted offset
    err = np.abs(r["carrFreq"] - (s["IF"] + L3.SCENE["doppler"]))
    assert err[-1] < 0.5 * abs(L3.SCENE["acq_err"]) and (np.diff(err) < 0.5).all()


def test_closed_loop_scene_is_decidable(scene):
    """The GPU tier compares a closed-loop run with this restatement at
    |gpu - ref| <= 1e-6 |ref| + 1e-6 and blksize exactly.  Every sum of every epoch is
    offset by 1e-9 relative, signs alternating over the twelve sums (and the opposite
    pattern): the run must keep every blksize and every other field within
    1e-7 |ref| + 1e-7 -- the bound of tests/test_e1t_cpu.py, for the same reason."""
    IF, prn, cp, f0, rate, s, r = scene
    pat = 1e-9 * np.array([1, -1, 1, -1, 1, -1, 1, -1, 1, -1, 1, -1.0])
    for p in (pat, -pat):
        rr = L3.track(IF, s, prn, cp, f0, L3.SCENE_MS, perturb=p)
        assert np.array_equal(rr["blksize"], r["blksize"])
        for f in L3.FIELDS:
            ok = np.abs(rr[f] - r[f]) <= 1e-7 * np.abs(r[f]) + 1e-7
            assert ok.all(), (f, np.flatnonzero(~ok)[:4])


def test_replay_of_recorded_sums_equals_the_tracked_run(scene):
    IF, prn, cp, f0, rate, s, r = scene
    sums = np.stack([r[f] for f in L3.SUMS], axis=1)
    rp = L3.replay(sums, s, cp, f0)
    assert np.array_equal(rp["blksize"], r["blksize"])
    for f in L3.LOOP_FIELDS:
        assert np.array_equal(rp[f], r[f]), f


def test_out_of_data_in_the_restatement():
    s = L3.settings()
    row = L3.padded(L3.generate_code(1))
    IF = np.zeros(2 * 30000, np.int8)
    st, blk, r = L3.correlate(IF, s, row, row, 10000, 0.0, 0.0, 10.23e6, -2.025e6)
    assert (st, blk) == (1, 24000) and r is None
    st, blk, r = L3.correlate(IF, s, row, row, 6000, 0.0, 0.0, 10.23e6, -2.025e6)
    assert st == 0 and r[1] == 30000


def test_restatement_finds_the_planted_prn():
    """acquisition.sci on the search scene: the planted PRN, bin and code phase, with a
    metric above acqThreshold; another PRN stays below it."""
    IF, prn = L3.search_scene()
    s = L3.settings()
    a = L3.acquire(IF, s, prn)
    assert a["metric"] > s["acqThreshold"]
    assert a["code_phase"] == L3.ACQ_START + 2              # 1-based, and the table's one sample
    assert a["carr_freq"] == s["IF"] + L3.ACQ_DOPPLER
    assert L3.acquire(IF, s, 7)["metric"] < s["acqThreshold"]
