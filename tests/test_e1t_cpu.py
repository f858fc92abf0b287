"""CPU tier of the Galileo E1B float tracker (gnsscorr_e1t_*): the restatement of
GALILEO/E1/tracking.sci:95-455 (tests/e1t_scenarios.py), the host-only entry points
of the library, and the decidability of the closed-loop scene the GPU tier runs.
"""
import ctypes as C

import numpy as np
import pytest

import e1t_scenarios as E

EINVAL = -1


def test_subcarrier_table_is_the_parity_of_ceil_t():
    """tracking.sci:164-168: the padded table alternates over all 2050 entries starting
    with +1, so the entry at index ceil(t) + 1 (1-based) is +1 iff ceil(t) is even:
    the identity the kernel uses instead of a table."""
    tab = E.meandr_table()
    assert tab.shape == (2050,)
    m = np.ones(2046)
    m[1::2] = -1
    assert np.array_equal(tab, np.concatenate([[m[-2], m[-1]], m, [m[0], m[1]]]))
    ceil_t = np.arange(2050)                         # index = ceil(t) + 1 = 1..2050
    assert np.array_equal(tab[ceil_t], 1.0 - 2.0 * (ceil_t & 1))
    # and through the same expression the correlator evaluates, over a whole epoch
    k = np.arange(16001, dtype=np.float64)
    for rem in (-0.45, 0.0, 0.06, 1.49):
        idx = np.ceil((rem + 0.1) + k * (2.046e6 / 16e6)).astype(np.int64)
        assert np.array_equal(tab[idx], 1.0 - 2.0 * (idx & 1))


def test_split_rows_wrap_the_whole_code():
    """:157-160: row s is the window [1023 s - 1, 1023 s + 1023] of the circular code, so
    the front pad of row 1 is the last chip and the back pad of row 4 the first."""
    codes, _ = E.fixture_codes()
    c = codes[0].astype(np.float64)
    rows = E.split_code(c)
    assert rows.shape == (4, 1025)
    for s in range(4):
        assert np.array_equal(rows[s], c[(1023 * s - 1 + np.arange(1025)) % 4092])
    assert rows[0, 0] == c[4091] and rows[3, 1024] == c[0]


def test_loop_coefs_and_init_chan_equal_the_restatement(gc):
    for kw in (dict(), dict(dllNoiseBandwidth=2.0, sllNoiseBandwidth=1.5, sllDampingRatio=0.9,
                            pllNoiseBandwidth=18.0, fllNoiseBandwidth=100.0)):
        cfg = gc.e1t_cfg(**kw)
        s = E.settings(**kw)
        want = E.calc_loop_coef(s["dllNoiseBandwidth"], s["dllDampingRatio"], 1.0) + \
            E.calc_loop_coef(s["sllNoiseBandwidth"], s["sllDampingRatio"], 1.0) + \
            E.calc_fll_pll_loop_coef(s["pllNoiseBandwidth"], s["fllNoiseBandwidth"], 0.001)
        assert gc.e1t_loop_coefs(cfg) == want
    cfg = gc.e1t_cfg()
    ch = gc.e1t_init_chan(cfg, 2, 30713, 2.42e6 - 2259.0, stream=1, skip=48000000)[0]
    lp = E.Loop(E.settings(), 48000000 + 30713 - 1, 2.42e6 - 2259.0)
    assert ch["code_id"] == 2 and ch["stream"] == 1 and ch["status"] == 0 and ch["n_epochs"] == 0
    assert ch["pos"] == lp.pos and ch["segment"] == lp.segment == 0
    for f, v in (("rem_code", lp.rem_code), ("rem_meandr", lp.rem_meandr),
                 ("rem_carr", lp.rem_carr), ("code_freq", lp.code_freq),
                 ("meandr_freq", lp.meandr_freq), ("carr_freq", lp.carr_freq),
                 ("carr_freq_basis", lp.carr_basis), ("old_code_nco", 0.0),
                 ("old_code_error", 0.0), ("old_meandr_nco", 0.0), ("old_meandr_error", 0.0),
                 ("old_carr_nco", 0.0), ("old_carr_error", 0.0), ("i1", lp.I1), ("q1", lp.Q1)):
        assert ch[f] == v, f


def test_bad_lengths_and_chips_are_einval_before_any_device_call(gc):
    """Only 4092 / 8184 are accepted, by create and by init_chan; set_codes looks at the
    chips before anything else.  None of these reaches a device call (this tier has no
    device: a device call would answer GNSSCORR_ENODEV or GNSSCORR_EDEVICE instead)."""
    L = gc.lib()
    for kw in (dict(codeLength=1023), dict(codeLength=4091), dict(meandrLength=4092),
               dict(meandrLength=8183), dict(fileType=3), dict(sllCorrelatorSpacing=1.0)):
        cfg = gc.e1t_cfg(**kw)
        h = C.c_void_p()
        assert L.gnsscorr_e1t_create(C.byref(h), C.byref(cfg)) == EINVAL, kw
        assert b"e1t: bad config" in L.gnsscorr_last_error()
        assert not h.value
        out = np.zeros(1, gc.E1T_CHAN)
        assert L.gnsscorr_e1t_init_chan(C.byref(cfg), 0, 0, 0, 1, 2.42e6, out.ctypes.data) == EINVAL
    codes, _ = E.fixture_codes()
    bad = codes.copy()
    bad[1, 77] = 0
    assert L.gnsscorr_e1t_set_codes(None, 3, bad.ctypes.data) == EINVAL
    assert b"chips must be +-1 (code 1, chip 77 is 0)" in L.gnsscorr_last_error()
    bad[1, 77] = 2
    assert L.gnsscorr_e1t_set_codes(None, 3, bad.ctypes.data) == EINVAL
    assert b"chips must be +-1" in L.gnsscorr_last_error()
    # no context: tracking is refused on the host as well
    assert L.gnsscorr_e1t_track(None, None, 0, 0, 1, None, 1, 1, None) == EINVAL


@pytest.fixture(scope="module")
def scene():
    IF, codes, chans = E.closed_loop_scene()
    s = E.settings()
    runs = [E.track(IF, s, codes[row], cp, f0, E.SCENE_MS) for row, cp, f0, _ in chans]
    return IF, codes, chans, s, runs


def test_restatement_tracks_the_synthetic_signal(scene):
    """40 ms on PRN 11 (and the scene's other two): the prompt-prompt arm dominates,
    codeFreq stays within a few Hz of the planted rate, the segment counter wraps."""
    _, _, chans, _, runs = scene
    for (row, cp, f0, rate), r in zip(chans, runs):
        assert r["status"] == 0 and len(r["I_P_P"]) == E.SCENE_MS
        assert np.array_equal(r["segment"], np.arange(E.SCENE_MS) % 4)
        assert np.abs(r["codeFreq"] - rate).max() < 3.0
        mag = {f: np.hypot(r["I" + f], r["Q" + f]) for f in ("_E_P", "_P_E", "_P_P", "_P_L", "_L_P")}
        for f in ("_E_P", "_P_E", "_P_L", "_L_P"):
            assert (mag["_P_P"] > mag[f]).all(), (row, f)
        assert (mag["_P_P"] > 0.5 * 12.0 * 16000).all()       # planted amplitude 12 per sample
        assert np.abs(r["blksize"] - 16000).max() <= 1


def test_closed_loop_scene_is_decidable(scene):
    """The GPU tier compares a closed-loop run with this restatement at
    |gpu - ref| <= 1e-6 |ref| + 1e-6 and blksize exactly.  That is decidable only if the
    rounding of the sums cannot move the loop by that much: here every sum of every
    epoch is offset by 1e-9 relative (signs alternating over the ten sums, so the I/Q
    and early/late ratios the discriminators see all move, and the opposite pattern),
    which is five to six orders above fp64 summation error, and the run must keep every
    blksize and every other field within 1e-7 |ref| + 1e-7: the GPU tier's form, ten
    times tighter.  The scene's seed, phases and acquisition offsets were chosen for
    this (a Q sum that passes through zero amplifies without bound in relative terms)."""
    IF, codes, chans, s, runs = scene
    pat = 1e-9 * np.array([1, -1, 1, -1, 1, -1, 1, -1, 1, -1.0])
    for (row, cp, f0, _), r in zip(chans, runs):
        for p in (pat, -pat):
            rr = E.track(IF, s, codes[row], cp, f0, E.SCENE_MS, perturb=p)
            assert np.array_equal(rr["blksize"], r["blksize"])
            for f in E.FIELDS:
                ok = np.abs(rr[f] - r[f]) <= 1e-7 * np.abs(r[f]) + 1e-7
                assert ok.all(), (row, f, np.flatnonzero(~ok)[:4])


def test_replay_of_recorded_sums_equals_the_tracked_run(scene):
    _, _, chans, s, runs = scene
    row, cp, f0, _ = chans[0]
    r = runs[0]
    sums = np.stack([r[f] for f in E.SUMS], axis=1)
    rp = E.replay(sums, s, cp, f0)
    assert np.array_equal(rp["blksize"], r["blksize"])
    for f in E.LOOP_FIELDS:
        assert np.array_equal(rp[f], r[f]), f


def test_stops_in_the_restatement():
    """Out of data is status 1 with the blksize that did not fit; a subcarrier phase whose
    late index leaves the 2050-entry table is status 2."""
    codes, _ = E.fixture_codes()
    s = E.settings()
    rows, mtab = E.split_code(codes[0]), E.meandr_table()
    IF = np.zeros(2 * 24000, np.int8)
    blk0 = int(np.ceil(1023 / (1.023e6 / 16e6)))              # 16001: the quotient rounds up
    st, blk, r = E.correlate(IF, s, rows, mtab, 10000, 0, 0.0, 0.0, 0.0, 1.023e6, 2.046e6, 2.42e6)
    assert (st, blk) == (1, blk0) and r is None
    st, blk, r = E.correlate(IF, s, rows, mtab, 0, 0, 0.0, 5.0, 0.0, 1.023e6, 2.046e6, 2.42e6)
    assert (st, blk) == (2, blk0)
    st, blk, r = E.correlate(IF, s, rows, mtab, 0, 0, 0.0, -1.0, 0.0, 1.023e6, 2.046e6, 2.42e6)
    assert st == 2
    st, blk, r = E.correlate(IF, s, rows, mtab, 0, 3, 0.0, 1.5, 0.0, 1.023e6, 2.046e6, 2.42e6)
    assert st == 0 and r[2] == 0                              # segment 3 -> 0
