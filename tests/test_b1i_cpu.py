"""CPU tier of BeiDou B1I in the float tracker (system 2 of gnsscorr_sgt_*): the ranging
code against the restatement of COMPASS/B1/include/generateCAcode.sci
(tests/b1i_scenarios.py), the host-only entry points of the library, and the
decidability of the closed-loop scene the GPU tier runs.
"""
import ctypes as C

import numpy as np
import pytest

import b1i_scenarios as B

EINVAL, ENODEV = -1, -4


def test_b1i_code_equals_the_restatement(gc):
    for prn in range(1, B.N_PRN + 1):
        got = gc.b1i_code(prn)
        assert got.shape == (2046,) and got.dtype == np.int8
        assert (np.abs(got) == 1).all()
        assert np.array_equal(got, B.generate_code(prn)), prn
    # 37 different codes, balanced as a Gold code is
    assert len({gc.b1i_code(p).tobytes() for p in range(1, 38)}) == 37
    assert abs(int(gc.b1i_code(1).astype(np.int64).sum())) <= 66
    out = np.zeros(2046, np.int8)
    for prn in (0, 38, -1):
        assert gc.lib().gnsscorr_b1i_code(prn, out.ctypes.data) == EINVAL
        with pytest.raises(gc.GnssCorrError):
            gc.b1i_code(prn)


def test_sampled_row_at_16_msps(gc):
    """makeCaTable.sci:62-69: 16 000 samples per period, the last index forced to 2046."""
    chips = gc.b1i_code(7)
    row = gc.sample_code(chips, 2.046e6, 16e6, 16000)
    assert row.shape == (16000,)
    assert np.array_equal(row, B.sample_code(B.generate_code(7), 2.046e6, 16e6, 16000))
    assert row[-1] == chips[2045] and row[0] == chips[0]


def _last(gc):
    return gc.lib().gnsscorr_last_error().decode()


def test_create_accepts_system_2_and_refuses_its_bad_configurations(gc):
    L = gc.lib()
    h = C.c_void_p()
    # a good system-2 configuration passes the configuration check and reaches the
    # device check (no device in this tier)
    cfg = gc.sgt_cfg(2, device=-1)
    assert (cfg.code_length, cfg.code_freq_basis, cfg.if_freq) == (2046, 2.046e6, 0.098e6)
    assert (cfg.dll_spacing, cfg.dll_noise_bw, cfg.dll_damping) == (0.1, 0.5, 0.7)
    assert (cfg.pll_noise_bw, cfg.fll_noise_bw, cfg.file_type, cfg.samp_rate) == (25.0, 250.0, 2, 16e6)
    assert L.gnsscorr_sgt_create(C.byref(h), C.byref(cfg)) == ENODEV
    assert not h.value
    for kw in (dict(codeLength=1023), dict(codeLength=2047), dict(fileType=3),
               dict(dllCorrelatorSpacing=1.0)):
        cfg = gc.sgt_cfg(2, device=-1, **kw)
        assert L.gnsscorr_sgt_create(C.byref(h), C.byref(cfg)) == EINVAL, kw
        assert _last(gc) == ("sgt: bad config (system 2: file_type 1/2, code_length 2046, "
                             "0<=dll_spacing<1, variants 0/1)")
    for system in (3, -1):
        cfg = gc.sgt_cfg(0, device=-1)
        cfg.system = system
        assert L.gnsscorr_sgt_create(C.byref(h), C.byref(cfg)) == EINVAL
        msg = _last(gc)
        assert "GPS" in msg and "GLONASS" in msg and "BeiDou B1I" in msg and str(system) in msg
    # the text of a bad system-0/1 configuration is unchanged
    cfg = gc.sgt_cfg(1, device=-1, codeLength=1023)
    assert L.gnsscorr_sgt_create(C.byref(h), C.byref(cfg)) == EINVAL
    assert _last(gc) == ("sgt: bad config (system 0/1, file_type 1/2, code_length 1023/511, "
                         "0<=dll_spacing<1, variants 0/1)")


def test_init_chan_prn_range(gc):
    L = gc.lib()
    cfg = gc.sgt_cfg(2)
    out = np.zeros(1, gc.SGT_CHAN)
    assert L.gnsscorr_sgt_init_chan(C.byref(cfg), 37, 1, 1000, 4321, 0.098e6 + 250.0,
                                    out.ctypes.data) == 0
    ch = out[0]
    assert ch["code_id"] == 37 and ch["stream"] == 1 and ch["pos"] == 1000 + 4321 - 1
    assert ch["code_freq"] == 2.046e6 and ch["carr_freq"] == ch["carr_freq_basis"] == 0.098e6 + 250.0
    assert ch["i1"] == ch["q1"] == 0.001 and ch["rem_code"] == 0.0
    for prn in (38, 0, -3):
        assert L.gnsscorr_sgt_init_chan(C.byref(cfg), prn, 0, 0, 1, 0.098e6, out.ctypes.data) == EINVAL
        assert "1..37" in _last(gc)
    # GPS keeps its range
    assert L.gnsscorr_sgt_init_chan(C.byref(gc.sgt_cfg(0)), 33, 0, 0, 1, 2.42e6,
                                    out.ctypes.data) == EINVAL


def test_loop_coefs_equal_the_restatement(gc):
    for kw in (dict(), dict(dllNoiseBandwidth=2.0, dllDampingRatio=0.9, pllNoiseBandwidth=18.0,
                            fllNoiseBandwidth=100.0)):
        cfg = gc.sgt_cfg(2, **kw)
        s = B.settings(**kw)
        v = [C.c_double() for _ in range(5)]
        gc.lib().gnsscorr_sgt_loop_coefs(C.byref(cfg), *[C.byref(x) for x in v])
        want = B.S.calc_loop_coef(s["dllNoiseBandwidth"], s["dllDampingRatio"], 1.0) + \
            B.S.calc_fll_pll_loop_coef(s["pllNoiseBandwidth"], s["fllNoiseBandwidth"], 0.001)
        assert tuple(x.value for x in v) == want


@pytest.fixture(scope="module")
def runs():
    IF, chans = B.scene()
    s = B.settings()
    return IF, chans, s, [B.track(IF, s, c[0], c[1], B.scene_acq_freq(c), B.SCENE_MS)
                          for c in chans]


def test_restatement_tracks_the_scene(runs):
    """Seed B.SCENE_SEED at B.SCENE_CN0 dB-Hz: all four channels run 40 epochs, stay within
    a few Hz of the planted code rate, see the Neumann-Hoffman sign changes on I_P and
    keep |I_P| above |Q_P| over the last 10 epochs."""
    _, chans, _, rr = runs
    for c, r in zip(chans, rr):
        assert len(r["I_P"]) == B.SCENE_MS and r["stop_blksize"] is None
        assert np.abs(r["blksize"] - 16000).max() <= 1
        assert np.abs(r["codeFreq"][10:] - c[3]).max() < 3.0
        assert (np.abs(r["I_P"][-10:]) > np.abs(r["Q_P"][-10:])).all()
        sg = np.sign(r["I_P"][10:])
        assert (sg > 0).any() and (sg < 0).any()


def test_closed_loop_scene_is_decidable(runs):
    """The GPU tier compares a closed-loop run with the restatement at 1e-6 relative and
    blksize exactly.  Here every sum of every epoch is offset by 1e-9 relative, signs
    alternating over the six sums (and the opposite pattern): five to six orders above
    fp64 summation error.  Every blksize must stay and every field move by no more than
    1e-7 |ref| + 1e-7.  Scene seed B.SCENE_SEED (= 22), C/N0 50 dB-Hz."""
    IF, chans, s, rr = runs
    pat = 1e-9 * np.array([1, -1, 1, -1, 1, -1.0])
    for c, r in zip(chans, rr):
        for p in (pat, -pat):
            q = B.track(IF, s, c[0], c[1], B.scene_acq_freq(c), B.SCENE_MS, perturb=p)
            assert np.array_equal(q["blksize"], r["blksize"])
            for f in B.FIELDS:
                ok = np.abs(q[f] - r[f]) <= 1e-7 * np.abs(r[f]) + 1e-7
                assert ok.all(), (c[0], f, np.flatnonzero(~ok)[:4])


def test_replay_of_recorded_sums_equals_the_tracked_run(runs):
    _, chans, s, rr = runs
    c, r = chans[0], rr[0]
    sums = np.stack([r[f] for f in B.SUMS], axis=1)
    rp = B.replay(sums, s, c[0], c[1], B.scene_acq_freq(c))
    assert np.array_equal(rp["blksize"], r["blksize"])
    for f in B.FIELDS:
        assert np.array_equal(rp[f], r[f]), f


def test_search_restatement_finds_the_scene(runs):
    """acquisition.sci:86-168 on the first 2 ms: the planted PRNs on their bins and code
    phases, every decision clear of its runner-up by far more than 1e-6, and the channels
    started from these results stay locked for 30 epochs."""
    IF, chans, s, _ = runs
    res = B.acquire(IF, s, [c[0] for c in chans])
    frq = B.bins(s)
    assert len(frq) == 29 and frq[0] == 0.098e6 - 7000 and frq[1] - frq[0] == 500.0
    for c, a in zip(chans, res):
        assert a["metric"] > 2.5
        assert abs(a["carr_freq"] - (0.098e6 + c[2])) <= 250.0
        # the planted start is rounded to a sample, the sampled replica leads by up to one
        # sample (makeCaTable's ceil rule), and the peak is flat over a sample at 7.8 per chip
        assert abs(a["code_phase"] - c[1]) <= 2
        assert min(a["margins"]) > 1e-4
        r = B.track(IF, s, c[0], a["code_phase"], a["carr_freq"], 30)
        assert len(r["I_P"]) == 30
        assert (np.abs(r["I_P"][-10:]) > np.abs(r["Q_P"][-10:])).all()
