"""GPU: GLONASS L1OF ephemeris fields, satellite integration and position fix (csrc/navglo.hip)
against the restatement of the Scilab files (tests/navglo_scenarios.py).  Field values, the
frame time, deltat, the loop counts, ready, clk, rawP, used, n_used, status and n_meas are
exact; the integrated states and the outputs behind transcendental functions are held to
navglo_scenarios.TOL, measured on the CPU from the restatement alone (test_navglo_cpu.py)."""
import numpy as np
import pytest

import navglo_scenarios as S
from nav_fix_gpu_util import check_records, fix_dev, poison as _poison

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ stage 1
@pytest.mark.parametrize("n_ch", [1, 3, 65])
def test_ephemeris_is_byte_equal(gpu, n_ch):
    """every starting string, a repeated string, a missing string 4 and string 1, a 2 inside
    string 2, an almanac string, string 1 and a string number, n_strings 0 / 14 / 15,
    first_mark = -1, poisoned outputs; negative, all-ones and sign-bit-only (-0.0) fields; the
    host twin gives the same"""
    gc = gpu
    assert gc.GLO_EPH.itemsize == S.EPH.itemsize and gc.GLO_EPH.names == S.EPH.names
    nav = gc.NavCtx()
    bits, n_strings, first, _, _ = S.eph_scene(n_ch)
    want = S.eph_literal(bits, n_strings, first)
    d_bits, d_n, d_first = (gc.DevBuf.from_array(a) for a in (bits, n_strings, first))
    d_eph = gc.DevBuf.from_array(_poison(n_ch, gc.GLO_EPH))
    nav.glo_ephemeris_dev(d_bits.ptr, d_n.ptr, d_first.ptr, n_ch, d_eph.ptr)
    nav.sync()
    got = d_eph.download(gc.GLO_EPH)
    for k in S.EPH.names:
        assert got[k].tobytes() == want[k].tobytes(), (k, got[k][:4], want[k][:4])
    assert got.tobytes() == want.tobytes()
    assert nav.glo_ephemeris(bits, n_strings, first).tobytes() == want.tobytes()


# ------------------------------------------------------------------ stage 2
def _check_sat(got, lit, what, tol=None):
    tol = S.TOL if tol is None else tol
    for k in ("n10", "n1", "n001", "ready", "deltat", "clk", "acc"):
        assert got[k].tobytes() == np.ascontiguousarray(lit[k], S.SAT[k].base).tobytes(), (what, k)
    idle = lit["ready"] == 0
    assert not got[idle].view(np.uint8).any(), what             # zeros, every byte
    for g in S.STATE_GROUPS:
        dist = S.state_distance(got, lit, g)
        print(what, g, dist, tol[g])
        assert dist <= tol[g], (what, g, dist, tol[g])


@pytest.mark.parametrize("period", S.SAT_SCENES)
@pytest.mark.parametrize("n_ch", [1, 63, 64, 65])
def test_satpos_equals_the_restatement(gpu, period, n_ch):
    """deltat positive, negative and exactly 0; n10 0, 1 and 90; n1 0 and 9; n001 0, 199 / 200
    and 799 / 800 on either side of the rounding, 999; channels that are not ready"""
    gc = gpu
    nav = gc.NavCtx()
    eph = S.sat_scene(period)[:n_ch]
    lit = {k: v[:n_ch] for k, v in S.sat_literal(period).items()}
    cfg = gc.glo_fix_cfg(navSolPeriod=period)
    d_eph = gc.DevBuf.from_array(eph)
    d_sat = gc.DevBuf.from_array(_poison(n_ch, gc.GLO_SAT))
    nav.glo_satpos_dev(d_eph.ptr, n_ch, cfg, d_sat.ptr)
    nav.sync()
    got = d_sat.download(gc.GLO_SAT)
    _check_sat(got, lit, (period, n_ch))
    assert nav.glo_satpos(eph, cfg).tobytes() == got.tobytes()  # the host twin


# ------------------------------------------------------------------ stage 3
def _fix_dev(gc, nav, s, in_place=False):
    """-> sat, n_meas, sol, chan and the poisoned arrays they started from"""
    n_ch = len(s["eph"])
    d_sat = gc.DevBuf.from_array(_poison(n_ch, gc.GLO_SAT))
    cfg = gc.glo_fix_cfg(**s["cfg"])

    def launch(d_eph, d_first, *series_and_outputs):
        nav.glo_satpos_dev(d_eph, n_ch, cfg, d_sat.ptr)
        nav.glo_fix_dev(d_eph, d_sat.ptr, d_first, *series_and_outputs[:4], s["rx_first"], cfg,
                        *series_and_outputs[4:])
    out = fix_dev(gc, nav, s, launch, in_place)
    return (d_sat.download(gc.GLO_SAT), *out)


def _check_fix(name, s, sat, n_meas, sol, chan, p_sol, p_chan, tol=None):
    _check_sat(sat, S.scene_sat(name), name, tol)
    w_n, Sx, Cx = S.literal_result(name)
    want_sol, want_chan = S.G.as_records(w_n, Sx, Cx, p_sol, p_chan)
    check_records(S, name, (w_n, want_sol, want_chan, Sx["written"]), n_meas, sol, chan, p_sol,
                  tol)
    unwritten = np.repeat(~Sx["written"], np.diff(s["rx_first"]), axis=0)
    assert chan[unwritten].tobytes() == p_chan[unwritten].tobytes(), name


@pytest.mark.parametrize("name", tuple(S.SCENES) + ("many",))
def test_fix_equals_the_restatement(gpu, name):
    """1, 2, 3 and 65 receivers of 4, 5, 12, 64 and unequal numbers of channels; 1, 2, 3 and 7
    measurements and max_meas below n_meas; a satellite on lane 0 that drops below a mask of 10
    degrees after the first fix and stays out, the others keeping their own states; 5 to 3
    active satellites; fewer than 4 ready channels; Bn = 4 and ln = 1 each excluding a channel;
    a rank-deficient receiver; troposphere on and off; masks 0 and 10; padded strides"""
    s = S._scene(name)
    nav = gpu.NavCtx()
    _check_fix(name, s, *_fix_dev(gpu, nav, s))


@pytest.mark.parametrize("name", tuple(S.WORLD_SCENES))
def test_fix_equals_the_restatement_on_the_world_scenes(gpu, name):
    """11 receivers in one launch in every quadrant, south of the equator, on either side of
    the 0 and 180 degree meridians, at the equator and above 80 degrees north and south.  The
    states glo_satpos_dev makes of the scene's ephemerides and the fix are held to TOL_WORLD,
    measured on this scene alone; poisoned outputs, padded strides; the host twins of both
    stages give the device forms' bytes."""
    s = S.fix_scene(name)
    nav = gpu.NavCtx()
    sat, n_meas, sol, chan, p_sol, p_chan = _fix_dev(gpu, nav, s)
    _check_fix(name, s, sat, n_meas, sol, chan, p_sol, p_chan, S.TOL_WORLD)
    assert not sol["status"].any() and chan["used"].all()
    cfg = gpu.glo_fix_cfg(**s["cfg"])
    assert nav.glo_satpos(s["eph"], cfg).tobytes() == sat.tobytes()
    h_n, h_sol, h_chan = nav.glo_fix(s["eph"], sat, s["first"], s["abs_sample"], s["rx_first"],
                                     cfg, sol=p_sol.copy(), chan=p_chan.copy())
    assert h_n.tobytes() == n_meas.tobytes()
    assert h_sol.tobytes() == sol.tobytes() and h_chan.tobytes() == chan.tobytes()


def test_absolute_sample_is_read_in_place_from_epoch_records(gpu):
    nav = gpu.NavCtx()
    for name in ("three_rx", "drop_one"):
        _check_fix(name, S.fix_scene(name), *_fix_dev(gpu, nav, S.fix_scene(name), in_place=True))


def test_strings_to_fix_chain_on_device_buffers(gpu):
    """One receiver of 5 channels over 31 000 epochs: glo_strings_dev -> glo_ephemeris_dev ->
    glo_satpos_dev -> glo_fix_dev on device buffers, queued on the context's stream with no
    host copy in between.  The I_P series carry 15 planted strings with their time marks.  Only
    the final arrays are compared, with the restatements and with what was planted."""
    import navbits_scenarios as NB
    gc = gpu
    s, series = S.chain_scene()
    n_ch, n_ep = series.shape
    mm = s["cfg"]["max_meas"]
    nav = gc.NavCtx()
    d_series, d_x = gc.DevBuf.from_array(series), gc.DevBuf.from_array(s["abs_sample"])
    d_first, d_ns = gc.DevBuf(4 * n_ch), gc.DevBuf(4 * n_ch)
    d_bits = gc.DevBuf(n_ch * 15 * 85)
    d_eph = gc.DevBuf(n_ch * gc.GLO_EPH.itemsize)
    d_sat = gc.DevBuf(n_ch * gc.GLO_SAT.itemsize)
    p_sol, p_chan = _poison(mm, gc.GPS_FIX_SOL), _poison(n_ch * mm, gc.GPS_FIX_CHAN)
    d_n, d_sol, d_fc = gc.DevBuf(4), gc.DevBuf.from_array(p_sol), gc.DevBuf.from_array(p_chan)
    cfg = gc.glo_fix_cfg(**s["cfg"])
    nav.glo_strings_dev(d_series.ptr, 8, 8 * n_ep, n_ep, n_ch, 15, d_first.ptr, d_ns.ptr,
                        d_bits.ptr)
    nav.glo_ephemeris_dev(d_bits.ptr, d_ns.ptr, d_first.ptr, n_ch, d_eph.ptr)
    nav.glo_satpos_dev(d_eph.ptr, n_ch, cfg, d_sat.ptr)
    nav.glo_fix_dev(d_eph.ptr, d_sat.ptr, d_first.ptr, d_x.ptr, 8, 8 * n_ep, n_ep,
                    s["rx_first"], cfg, d_n.ptr, d_sol.ptr, d_fc.ptr)
    nav.sync()
    first, n_str = d_first.download(np.int32), d_ns.download(np.int32)
    bits = d_bits.download(np.uint8).reshape(n_ch, 15, 85)
    eph, sat = d_eph.download(gc.GLO_EPH), d_sat.download(gc.GLO_SAT)
    n_meas = d_n.download(np.int32)
    sol = d_sol.download(gc.GPS_FIX_SOL).reshape(1, mm)
    chan = d_fc.download(gc.GPS_FIX_CHAN).reshape(n_ch, mm)
    for ch in range(n_ch):
        f, b = NB.glo_strings_fast(series[ch])
        assert f == first[ch] == s["first"][ch] and len(b) == n_str[ch] == 15
        assert bits[ch].tobytes() == b.tobytes() == s["bits"][ch].tobytes()
    w_eph = S.eph_literal(bits, n_str, first)
    assert eph.tobytes() == w_eph.tobytes() == s["eph"].tobytes()
    lit_sat = S.satpos_literal(w_eph, s["cfg"]["navSolPeriod"])
    _check_sat(sat, lit_sat, "chain")
    p_sol, p_chan = p_sol.view(gc.GPS_FIX_SOL).reshape(1, mm), p_chan.view(gc.GPS_FIX_CHAN).reshape(n_ch, mm)
    w_n, Sx, Cx = S.fix_literal(w_eph, first, s["abs_sample"], s["rx_first"], s["cfg"], sat=lit_sat)
    want_sol, want_chan = S.G.as_records(w_n, Sx, Cx, p_sol, p_chan)
    assert n_meas.tolist() == [mm] and not sol["status"].any()
    check_records(S, "chain", (w_n, want_sol, want_chan, Sx["written"]), n_meas, sol, chan, p_sol)
    err = np.linalg.norm(np.array([sol["X"][0], sol["Y"][0], sol["Z"][0]]).T - s["planted"][0],
                         axis=1)
    print("chain: distance to the planted receiver", err)
    assert (err < 2000.0).all()


def test_host_twin_equals_the_device_form(gpu):
    nav = gpu.NavCtx()
    for name in ("three_rx", "five_to_three", "few_ready"):
        s = S.fix_scene(name)
        sat, n_meas, sol, chan, p_sol, p_chan = _fix_dev(gpu, nav, s)
        h_n, h_sol, h_chan = nav.glo_fix(s["eph"], sat, s["first"], s["abs_sample"],
                                         s["rx_first"], gpu.glo_fix_cfg(**s["cfg"]),
                                         sol=p_sol.copy(), chan=p_chan.copy())
        assert h_n.tobytes() == n_meas.tobytes()
        assert h_sol.tobytes() == sol.tobytes() and h_chan.tobytes() == chan.tobytes()


def test_a_fix_can_be_repeated_on_the_same_states(gpu):
    """d_sat is read only: the second call gives the first call's bytes"""
    gc, s = gpu, S.fix_scene("drop_one")
    nav = gc.NavCtx()
    sat, n_meas, sol, chan, p_sol, p_chan = _fix_dev(gc, nav, s)
    again = nav.glo_fix(s["eph"], sat, s["first"], s["abs_sample"], s["rx_first"],
                        gc.glo_fix_cfg(**s["cfg"]), sol=p_sol.copy(), chan=p_chan.copy())
    twice = nav.glo_fix(s["eph"], sat, s["first"], s["abs_sample"], s["rx_first"],
                        gc.glo_fix_cfg(**s["cfg"]), sol=p_sol.copy(), chan=p_chan.copy())
    assert again[1].tobytes() == twice[1].tobytes() == sol.tobytes()
    assert again[2].tobytes() == twice[2].tobytes() == chan.tobytes()


def test_bad_arguments_are_refused_and_nothing_is_written(gpu):
    gc, s = gpu, S.fix_scene("three_rx")
    nav = gc.NavCtx()
    n_ch, n_ep = s["abs_sample"].shape
    fill = np.full(1 << 16, 0xAA, np.uint8)
    d_eph, d_first, d_x = (gc.DevBuf.from_array(a) for a in (s["eph"], s["first"], s["abs_sample"]))
    d_sat = gc.DevBuf.from_array(S.sat_records(S.scene_sat("three_rx")))
    d_n, d_sol, d_chan, d_out = (gc.DevBuf.from_array(fill) for _ in range(4))
    good = dict(eph=d_eph.ptr, sat=d_sat.ptr, first=d_first.ptr, x=d_x.ptr, es=8, cs=8 * n_ep,
                n_ep=n_ep, rx_first=s["rx_first"], n=d_n.ptr, sol=d_sol.ptr, chan=d_chan.ptr)

    def fix(cfg_kw=None, cfg=True, **kw):
        a = dict(good, **kw)
        c = gc.glo_fix_cfg(**dict(s["cfg"], **(cfg_kw or {}))) if cfg else None
        nav.glo_fix_dev(a["eph"], a["sat"], a["first"], a["x"], a["es"], a["cs"], a["n_ep"],
                        a["rx_first"], c, a["n"], a["sol"], a["chan"])

    ok = gc.glo_fix_cfg(**s["cfg"])
    bad = [
        lambda: fix(rx_first=[0, 12, 11, 23]),                 # not ascending
        lambda: fix(rx_first=[0, 12, 12, 23]),
        lambda: fix(rx_first=[1, 12, 16, 23]),
        lambda: fix(rx_first=[0, 65, 66, 67]),                 # more than 64 channels
        lambda: fix(cfg_kw=dict(navSolPeriod=0)), lambda: fix(cfg_kw=dict(samplesPerCode=0.0)),
        lambda: fix(cfg_kw=dict(samplesPerCode=-16000.0)), lambda: fix(cfg_kw=dict(max_meas=0)),
        lambda: fix(cfg_kw=dict(dataTypeSizeInBytes=0.0)),
        lambda: fix(cfg_kw=dict(dataTypeSizeInBytes=-1.0)),
        lambda: fix(eph=None), lambda: fix(sat=None), lambda: fix(first=None),
        lambda: fix(x=None), lambda: fix(n=None), lambda: fix(sol=None), lambda: fix(chan=None),
        lambda: fix(cfg=False), lambda: fix(es=4), lambda: fix(n_ep=0),
        lambda: nav.glo_ephemeris_dev(None, d_first.ptr, d_first.ptr, 3, d_out.ptr),
        lambda: nav.glo_ephemeris_dev(d_x.ptr, None, d_first.ptr, 3, d_out.ptr),
        lambda: nav.glo_ephemeris_dev(d_x.ptr, d_first.ptr, d_first.ptr, 3, None),
        lambda: nav.glo_ephemeris_dev(d_x.ptr, d_first.ptr, d_first.ptr, 0, d_out.ptr),
        lambda: nav.glo_satpos_dev(None, 3, ok, d_out.ptr),
        lambda: nav.glo_satpos_dev(d_eph.ptr, 3, ok, None),
        lambda: nav.glo_satpos_dev(d_eph.ptr, 3, None, d_out.ptr),
        lambda: nav.glo_satpos_dev(d_eph.ptr, 0, ok, d_out.ptr),
        lambda: nav.glo_satpos_dev(d_eph.ptr, 3, gc.glo_fix_cfg(navSolPeriod=0), d_out.ptr),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(gc.GnssCorrError):
            call()
            pytest.fail(f"bad call {i} was accepted")
    # the host twins refuse the same and leave their arrays alone
    sol = np.frombuffer(_poison(6, gc.GPS_FIX_SOL), gc.GPS_FIX_SOL).reshape(3, 2).copy()
    chan = np.frombuffer(_poison(n_ch * 2, gc.GPS_FIX_CHAN), gc.GPS_FIX_CHAN).reshape(n_ch, 2).copy()
    with pytest.raises(gc.GnssCorrError):
        nav.glo_fix(s["eph"], S.sat_records(S.scene_sat("three_rx")), s["first"], s["abs_sample"],
                    [0, 12, 11, 23], ok, sol=sol, chan=chan)
    assert (sol.view(np.uint8) == 0xAA).all() and (chan.view(np.uint8) == 0xAA).all()
    eph = np.frombuffer(_poison(3, gc.GLO_EPH), gc.GLO_EPH).copy()
    bits, n_strings, first, _, _ = S.eph_scene(3)
    rc = nav._glo_ephemeris(nav.h, bits.ctypes.data, n_strings.ctypes.data, first.ctypes.data, 0,
                            eph.ctypes.data)
    assert rc == -1 and "n_ch >= 1" in gc.lib().gnsscorr_last_error().decode()
    assert (eph.view(np.uint8) == 0xAA).all()
    nav.sync()
    for d in (d_n, d_sol, d_chan, d_out):
        assert d.download(np.uint8).tobytes() == fill.tobytes()
