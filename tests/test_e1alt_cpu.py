"""CPU tier of the Galileo E1 tracking alternatives (gnsscorr_e1t_* with epoch_ms / ambiguous):
the tables of the three files of GALILEO/E1/BOC_tracking_alternatives/ as restated in
tests/e1alt_scenarios.py, the host-only entry points of the library in the three new
modes, and the decidability of the closed-loop scene the GPU tier runs in each mode.

Two kinds of test live here.  Those that take the `gc` fixture go through the library
(loop_coefs, init_chan, the mode checks of create) and fail without the feature.  The others
(tables, tracking, decidability, replay, stops) check the restatement alone, the reference
the GPU tier compares the kernels with: the library has no host-only entry point that
returns its code rows, so the rows it builds are checked on the GPU, through the sums of
tests/test_e1alt_gpu.py (segments 0 and 3 for the wrapping pads).
"""
import ctypes as C

import numpy as np
import pytest

import e1alt_scenarios as A
import e1t_scenarios as E

EINVAL = -1
NEW_MODES = ("4ms", "amb1", "amb4")


def test_4ms_code_row():
    """tracking_4ms.sci:159: [c($) c c(1)], 4094 entries."""
    codes, _ = E.fixture_codes()
    c = codes[1].astype(np.float64)
    row = A.code_row_4ms(c)
    assert row.shape == (4094,)
    assert row[0] == c[4091] and row[4093] == c[0]
    assert np.array_equal(row[1:4093], c)
    assert np.array_equal(row, c[(np.arange(4094) - 1) % 4092])


def test_4ms_subcarrier_table_and_its_flipped_parity():
    """tracking_4ms.sci:163-165: [m($) m m(1)] with m = +1 -1 ... (8184) is 8186 entries
    that alternate over the whole table starting with -1, so entry j (1-based) is +1 for
    even j and the entry at index ceil(t) + 1 is -1 iff ceil(t) is even: the opposite sense
    of tracking.sci's table, which the kernel uses instead of a table."""
    tab = A.meandr_table_4ms()
    assert tab.shape == (8186,)
    m = np.ones(8184)
    m[1::2] = -1
    assert np.array_equal(tab, np.concatenate([[m[-1]], m, [m[0]]]))
    assert tab[0] == -1 and tab[1] == 1 and tab[8185] == 1
    ceil_t = np.arange(8186)                        # index = ceil(t) + 1 = 1..8186
    assert np.array_equal(tab[ceil_t], 2.0 * (ceil_t & 1) - 1.0)
    old = E.meandr_table()
    assert np.array_equal(tab[:2050], -old)         # the other sense, entry by entry
    # through the correlator's own index expression, over a whole 4 ms epoch
    k = np.arange(64001, dtype=np.float64)            # blksize at the nominal rates
    for rem in (-0.45, 0.0, 0.06, 0.85):
        for spc in (-0.1, 0.0, 0.1):
            idx = np.ceil((rem + spc) + k * (2.046e6 / 16e6)).astype(np.int64)
            assert idx.min() >= 0 and idx.max() <= 8185
            assert np.array_equal(tab[idx], 2.0 * (idx & 1) - 1.0)


def test_composite_sequence():
    """tracking_ambiguous_1ms.sci:141-145: entry 2i is chip i, entry 2i + 1 its negative."""
    codes, _ = E.fixture_codes()
    c = codes[2].astype(np.float64)
    ca = A.composite(c)
    assert ca.shape == (8184,)
    assert np.array_equal(ca[0::2], c) and np.array_equal(ca[1::2], -c)
    row = A.composite_row_4ms(c)                    # tracking_ambiguous_4ms.sci:146
    assert row.shape == (8186,)
    assert np.array_equal(row, ca[(np.arange(8186) - 1) % 8184])
    assert row[0] == -c[4091] and row[8185] == c[0]


def test_composite_rows_wrap_the_circular_sequence():
    """tracking_ambiguous_1ms.sci:148-151: row s is the window [2046 s - 1, 2046 s + 2046]
    of the circular sequence: the front pad of row 1 is its last entry and the back pad of
    row 4 its first."""
    codes, _ = E.fixture_codes()
    c = codes[0].astype(np.float64)
    ca = A.composite(c)
    rows = A.composite_rows(c)
    assert rows.shape == (4, 2048)
    for s in range(4):
        assert np.array_equal(rows[s], ca[(2046 * s - 1 + np.arange(2048)) % 8184])
    assert rows[0, 0] == ca[8183] and rows[3, 2047] == ca[0]
    assert rows[1, 0] == ca[2045] and rows[1, 2047] == ca[4092]


@pytest.mark.parametrize("mode", NEW_MODES)
def test_loop_coefs_and_init_chan_equal_the_restatement(gc, mode):
    for kw in (dict(), dict(dllNoiseBandwidth=2.0, sllNoiseBandwidth=1.5, sllDampingRatio=0.9,
                            pllNoiseBandwidth=18.0, fllNoiseBandwidth=100.0)):
        cfg = gc.e1t_cfg(**kw, **A.MODES[mode])
        assert gc.e1t_loop_coefs(cfg) == A.loop_coefs(mode, E.settings(**kw))
    # the 0.008 of tracking_ambiguous_4ms.sci:106, and the others, through k3 = T * fll/0.25
    k3 = gc.e1t_loop_coefs(gc.e1t_cfg(**A.MODES[mode]))[6]
    assert k3 == {"4ms": 0.004, "amb1": 0.001, "amb4": 0.008}[mode] * (250.0 / 0.25)
    cfg = gc.e1t_cfg(**A.MODES[mode])
    ch = gc.e1t_init_chan(cfg, 2, 30713, 2.42e6 - 2259.0, stream=1, skip=48000000)[0]
    lp = A.Loop(mode, E.settings(), 48000000 + 30713 - 1, 2.42e6 - 2259.0)
    assert ch["code_id"] == 2 and ch["stream"] == 1 and ch["status"] == 0 and ch["n_epochs"] == 0
    assert ch["pos"] == lp.pos and ch["segment"] == lp.segment == 0
    for f, v in (("rem_code", lp.rem_code), ("rem_meandr", lp.rem_meandr),
                 ("rem_carr", lp.rem_carr), ("code_freq", lp.code_freq),
                 ("meandr_freq", lp.meandr_freq), ("carr_freq", lp.carr_freq),
                 ("carr_freq_basis", lp.carr_basis), ("old_code_nco", 0.0),
                 ("old_code_error", 0.0), ("old_meandr_nco", 0.0), ("old_meandr_error", 0.0),
                 ("old_carr_nco", 0.0), ("old_carr_error", 0.0), ("i1", lp.I1), ("q1", lp.Q1)):
        assert ch[f] == v, f
    assert ch["code_freq"] == (2.046e6 if A.is_amb(mode) else 1.023e6)
    assert ch["meandr_freq"] == (0.0 if A.is_amb(mode) else 2.046e6)


def test_default_and_explicit_1ms_are_todays_mode(gc):
    """epoch_ms 0 and 1 with ambiguous 0 are tracking.sci: its coefficients and channel."""
    want = gc.e1t_loop_coefs(gc.e1t_cfg())
    for ms in (0, 1):
        cfg = gc.e1t_cfg(epochMs=ms, ambiguous=0)
        assert gc.e1t_loop_coefs(cfg) == want
        assert gc.e1t_init_chan(cfg, 0, 7, 2.42e6).tobytes() == \
            gc.e1t_init_chan(gc.e1t_cfg(), 0, 7, 2.42e6).tobytes()
    assert gc.e1t_cfg().epoch_ms == 1 and gc.e1t_cfg().ambiguous == 0


def test_bad_modes_are_einval_before_any_device_call(gc):
    """Only epoch_ms 0 / 1 / 4 and ambiguous 0 / 1, by create and by init_chan; the text keeps
    the configuration message as its prefix.  None reaches a device call (this tier has no
    device: a device call would answer GNSSCORR_ENODEV or GNSSCORR_EDEVICE instead)."""
    L = gc.lib()
    for kw in (dict(epochMs=2), dict(epochMs=3), dict(epochMs=-1), dict(epochMs=8),
               dict(ambiguous=2), dict(ambiguous=-1), dict(epochMs=4, ambiguous=4)):
        cfg = gc.e1t_cfg(**kw)
        h = C.c_void_p()
        assert L.gnsscorr_e1t_create(C.byref(h), C.byref(cfg)) == EINVAL, kw
        text = L.gnsscorr_last_error()
        assert text.startswith(b"e1t: bad config (file_type 1/2, code_length 4092, "
                               b"meandr_length 8184, 0<=dll_spacing<1, 0<=sll_spacing<1, "
                               b"positive rates)"), text
        assert b"epoch_ms" in text and b"ambiguous" in text
        assert not h.value
        out = np.zeros(1, gc.E1T_CHAN)
        assert L.gnsscorr_e1t_init_chan(C.byref(cfg), 0, 0, 0, 1, 2.42e6, out.ctypes.data) == EINVAL
    with pytest.raises(ValueError):
        gc.e1t_cfg(epochMS=4)


@pytest.fixture(scope="module")
def scenes():
    out = {}
    s = E.settings()
    for mode in NEW_MODES:
        IF, codes, chans = A.closed_loop_scene(mode)
        runs = [A.track(mode, IF, s, codes[row], cp, f0, A.SCENE_EPOCHS[mode])
                for row, cp, f0, _ in chans]
        out[mode] = (IF, codes, chans, s, runs)
    return out


@pytest.mark.parametrize("mode", NEW_MODES)
def test_restatement_tracks_the_synthetic_signal(scenes, mode):
    """The prompt arm dominates, codeFreq stays near the planted rate (twice it for the
    composite sequence), the row counter wraps in the ambiguous 1 ms loop only."""
    _, _, chans, _, runs = scenes[mode]
    n, ms = A.SCENE_EPOCHS[mode], A.EPOCH_MS[mode]
    for (row, cp, f0, rate), r in zip(chans, runs):
        assert r["status"] == 0 and len(r["I_P_P"]) == n
        want_seg = np.arange(n) % 4 if mode == "amb1" else np.zeros(n)
        assert np.array_equal(r["segment"], want_seg)
        mult = 2.0 if A.is_amb(mode) else 1.0
        assert np.abs(r["codeFreq"] - mult * rate).max() < 3.0 * mult
        mag = {f: np.hypot(r["I" + f], r["Q" + f]) for f in ("_E_P", "_P_E", "_P_P", "_P_L", "_L_P")}
        for f in ("_P_E", "_P_L") + (() if A.is_amb(mode) else ("_E_P", "_L_P")):
            assert (mag["_P_P"] > mag[f]).all(), (row, f)
        assert (mag["_P_P"] > 0.5 * 12.0 * 16000 * ms).all()   # planted amplitude 12 per sample
        assert np.abs(r["blksize"] - 16000 * ms).max() <= 2
        if A.is_amb(mode):
            for f in ("I_E_P", "I_L_P", "Q_E_P", "Q_L_P", "meandrFreq", "sllDiscr", "sllDiscrFilt"):
                assert not r[f].any(), f


@pytest.mark.parametrize("mode", NEW_MODES)
def test_closed_loop_scene_is_decidable(scenes, mode):
    """As tests/test_e1t_cpu.py::test_closed_loop_scene_is_decidable, for each new mode's
    scene: every sum of every epoch offset by 1e-9 relative, signs alternating over the ten
    sums, and the opposite pattern; every blksize must stay and every other field stay
    within 1e-7 |ref| + 1e-7, ten times inside what the GPU tier asserts."""
    IF, codes, chans, s, runs = scenes[mode]
    pat = 1e-9 * np.array([1, -1, 1, -1, 1, -1, 1, -1, 1, -1.0])
    for (row, cp, f0, _), r in zip(chans, runs):
        for p in (pat, -pat):
            rr = A.track(mode, IF, s, codes[row], cp, f0, A.SCENE_EPOCHS[mode], perturb=p)
            assert np.array_equal(rr["blksize"], r["blksize"])
            for f in E.FIELDS:
                ok = np.abs(rr[f] - r[f]) <= 1e-7 * np.abs(r[f]) + 1e-7
                assert ok.all(), (row, f, np.flatnonzero(~ok)[:4])


@pytest.mark.parametrize("mode", NEW_MODES)
def test_replay_of_recorded_sums_equals_the_tracked_run(scenes, mode):
    _, _, chans, s, runs = scenes[mode]
    row, cp, f0, _ = chans[0]
    r = runs[0]
    sums = np.stack([r[f] for f in E.SUMS], axis=1)
    rp = A.replay(mode, sums, s, cp, f0)
    assert np.array_equal(rp["blksize"], r["blksize"])
    assert np.array_equal(rp["segment"], r["segment"])
    for f in E.LOOP_FIELDS:
        assert np.array_equal(rp[f], r[f]), f


def test_stops_in_the_restatement():
    """Out of data is status 1 with the blksize that did not fit, in every mode; a
    subcarrier phase whose early index is below 1 or whose late index is above 8186 is
    status 2, in the five-arm mode only."""
    codes, _ = E.fixture_codes()
    s = E.settings()
    IF = np.zeros(2 * 70000, np.int8)
    tab = A.tables("4ms", codes[0])
    blk0 = int(np.ceil(4092 / (1.023e6 / 16e6)))
    st, blk, r = A.correlate_4ms(IF, s, tab, 10000, 0.0, 0.0, 0.0, 1.023e6, 2.046e6, 2.42e6)
    assert (st, blk) == (1, blk0) and r is None
    st, blk, r = A.correlate_4ms(IF, s, tab, 0, 0.0, 5.0, 0.0, 1.023e6, 2.046e6, 2.42e6)
    assert (st, blk) == (2, blk0)
    st, blk, r = A.correlate_4ms(IF, s, tab, 0, 0.0, -1.0, 0.0, 1.023e6, 2.046e6, 2.42e6)
    assert st == 2
    # one back pad only: the late arm of a whole epoch ends at ceil(rem + 0.1 + 8184) <= 8185
    st, blk, r = A.correlate_4ms(IF, s, tab, 0, 0.0, 1.5, 0.0, 1.023e6, 2.046e6, 2.42e6)
    assert st == 2
    st, blk, r = A.correlate_4ms(IF, s, tab, 0, 0.0, 0.85, 0.0, 1.023e6, 2.046e6, 2.42e6)
    assert st == 0
    for mode, length in (("amb1", 2046), ("amb4", 8184)):
        tab = A.tables(mode, codes[0])
        n = int(np.ceil(length / (2.046e6 / 16e6)))
        st, blk, r = A.correlate_amb(mode, IF, s, tab, 70000 - n + 1, 3, 0.0, 0.0, 2.046e6, 2.42e6)
        assert (st, blk) == (1, n) and r is None
        st, blk, r = A.correlate_amb(mode, IF, s, tab, 0, 3, 0.0, 0.0, 2.046e6, 2.42e6)
        assert st == 0 and r[2] == (0 if mode == "amb1" else 3)
