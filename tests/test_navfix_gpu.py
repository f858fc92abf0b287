"""GPU: GPS L1 ephemeris fields and position fix (csrc/navfix.hip) against the literal
restatement of the Scilab files (tests/navfix_scenarios.py).  Field values, TOW, rawP, used,
n_used, status and n_meas are exact; the outputs behind transcendental functions are held to
navfix_scenarios.TOL, measured on the CPU from the restatement alone (test_navfix_cpu.py)."""
import numpy as np
import pytest

import navfix_scenarios as S
from nav_fix_gpu_util import check_records, fix_dev, poison as _poison

pytestmark = pytest.mark.gpu


def _eph_dev(gc, nav, bits, n_bits, first):
    n_ch = len(bits)
    d_bits, d_n, d_first = (gc.DevBuf.from_array(a) for a in (bits, n_bits, first))
    d_eph = gc.DevBuf.from_array(np.full(n_ch * gc.GPS_EPH.itemsize, 0xAA, np.uint8))
    nav.gps_ephemeris_dev(d_bits.ptr, d_n.ptr, d_first.ptr, n_ch, d_eph.ptr)
    nav.sync()
    return d_eph.download(gc.GPS_EPH)


@pytest.mark.parametrize("n_ch", [1, 3, 65])
def test_ephemeris_is_byte_equal(gpu, n_ch):
    """every subframe order, a missing subframe, n_bits 0 / 1200 / 1500, a 2 inside and outside
    a decoded field, first_subframe = -1, poisoned outputs; negative, all-ones and sign-bit-only
    signed fields; the host twin gives the same"""
    assert gpu.GPS_EPH.itemsize == S.EPH.itemsize and gpu.GPS_EPH.names == S.EPH.names
    nav = gpu.NavCtx()
    bits, n_bits, first, _ = S.eph_scene(n_ch)
    want = S.eph_literal(bits, n_bits, first)
    got = _eph_dev(gpu, nav, bits, n_bits, first)
    for k in S.EPH.names:
        assert got[k].tobytes() == want[k].tobytes(), (k, got[k][:4], want[k][:4])
    assert got.tobytes() == want.tobytes()
    assert nav.gps_ephemeris(bits, n_bits, first).tobytes() == want.tobytes()


def _fix_dev(gc, nav, s, in_place=False):
    """-> n_meas, sol, chan and the poisoned arrays they started from"""
    def launch(d_eph, d_first, *series_and_outputs):
        nav.gps_fix_dev(d_eph, d_first, *series_and_outputs[:4], s["rx_first"],
                        gc.gps_fix_cfg(**s["cfg"]), *series_and_outputs[4:])
    return fix_dev(gc, nav, s, launch, in_place)


def _check_fix(name, s, n_meas, sol, chan, p_sol, p_chan, tol=None):
    w_n, Sx, Cx = S.literal_result(name)
    want_sol, want_chan = S.as_records(w_n, Sx, Cx, p_sol, p_chan)
    check_records(S, name, (w_n, want_sol, want_chan, Sx["written"]), n_meas, sol, chan, p_sol,
                  tol)


@pytest.mark.parametrize("name", tuple(S.SCENES) + ("many",))
def test_fix_equals_the_literal_restatement(gpu, name):
    """1, 2, 3 and 65 receivers of 4, 5, 12, 64 and unequal numbers of channels; 1, 2, 3 and 7
    measurements and max_meas below n_meas; a satellite that drops below the mask and stays
    out; 5 to 3 active satellites; fewer than 4 ready channels; the TOW seed from an excluded
    channel; a rank-deficient receiver; troposphere on and off; padded strides"""
    s = S.many_rx_scene() if name == "many" else S.fix_scene(name)
    nav = gpu.NavCtx()
    _check_fix(name, s, *_fix_dev(gpu, nav, s))


@pytest.mark.parametrize("name", tuple(S.WORLD_SCENES))
def test_fix_equals_the_literal_restatement_on_the_world_scenes(gpu, name):
    """11 receivers in one launch in every quadrant, south of the equator, on either side of
    the 0 and 180 degree meridians, at the equator and above 80 degrees north and south; TOW
    in the week's last and first minutes with check_t wrapping either way; Kepler loops that
    run all 10 steps at e from 0.1 to 0.3; inclinations from 0.3 to 1.4 rad.  Held to
    TOL_WORLD, measured on these scenes alone; poisoned outputs, padded strides; in the world
    scene the host twin gives the device form's bytes."""
    s = S.fix_scene(name)
    nav = gpu.NavCtx()
    n_meas, sol, chan, p_sol, p_chan = _fix_dev(gpu, nav, s)
    _check_fix(name, s, n_meas, sol, chan, p_sol, p_chan, S.TOL_WORLD)
    assert not sol["status"].any() and chan["used"].all()
    if name == "world":
        h_n, h_sol, h_chan = nav.gps_fix(s["eph"], s["first"], s["abs_sample"], s["rx_first"],
                                         gpu.gps_fix_cfg(**s["cfg"]), sol=p_sol.copy(),
                                         chan=p_chan.copy())
        assert h_n.tobytes() == n_meas.tobytes()
        assert h_sol.tobytes() == sol.tobytes() and h_chan.tobytes() == chan.tobytes()


def test_absolute_sample_is_read_in_place_from_epoch_records(gpu):
    nav = gpu.NavCtx()
    for name in ("three_rx", "drop_one"):
        _check_fix(name, S.fix_scene(name), *_fix_dev(gpu, nav, S.fix_scene(name), in_place=True))


def test_bits_to_fix_on_device_buffers(gpu):
    """gps_ephemeris_dev writes the ephemerides that gps_fix_dev reads, both queued on the
    context's stream with no host copy in between"""
    gc, s = gpu, S.fix_scene("three_rx")
    nav = gc.NavCtx()
    n_ch, n_ep = s["abs_sample"].shape
    n_rx, mm = 3, s["cfg"]["max_meas"]
    d_bits, d_nb, d_first, d_x = (gc.DevBuf.from_array(s[k])
                                  for k in ("bits", "n_bits", "first", "abs_sample"))
    d_eph = gc.DevBuf(n_ch * gc.GPS_EPH.itemsize)
    d_n, d_sol, d_chan = (gc.DevBuf.from_array(_poison(n, t)) for n, t in
                          ((n_rx, np.int32), (n_rx * mm, gc.GPS_FIX_SOL), (n_ch * mm, gc.GPS_FIX_CHAN)))
    nav.gps_ephemeris_dev(d_bits.ptr, d_nb.ptr, d_first.ptr, n_ch, d_eph.ptr)
    nav.gps_fix_dev(d_eph.ptr, d_first.ptr, d_x.ptr, 8, 8 * n_ep, n_ep, s["rx_first"],
                    gc.gps_fix_cfg(**s["cfg"]), d_n.ptr, d_sol.ptr, d_chan.ptr)
    nav.sync()
    sol = d_sol.download(gc.GPS_FIX_SOL).reshape(n_rx, mm)
    chan = d_chan.download(gc.GPS_FIX_CHAN).reshape(n_ch, mm)
    _check_fix("three_rx", s, d_n.download(np.int32), sol, chan, sol, chan)


def test_record_to_position_chain_on_the_device(gpu):
    """One receiver of 8 channels over 31 000 epochs: SgtCtx.replay_dev -> gps_frames_dev ->
    gps_ephemeris_dev -> gps_fix_dev on device buffers, ordered by one event, no host copy in
    between.  The sums carry the planted subframes; absolute_sample is what the tracker's own
    loop makes of the planted start positions, read in place.  Only the final arrays are
    compared, against the restatements fed with the epoch records read back afterwards."""
    import navbits_scenarios as NB
    gc = gpu
    s, sums, pos0 = S.chain_scene()
    n_ch, n_ep, mm = sums.shape[0], sums.shape[1], s["cfg"]["max_meas"]
    trk, nav = gc.SgtCtx(0), gc.NavCtx()
    chans = trk.init_chans([3 + i for i in range(n_ch)], [1] * n_ch, [2.42e6] * n_ch)
    chans["pos"] = pos0
    d_chan, d_sums = gc.DevBuf.from_array(chans), gc.DevBuf.from_array(sums)
    d_ep = gc.DevBuf(n_ch * n_ep * gc.SGT_EPOCH.itemsize)
    d_first, d_nb = gc.DevBuf(4 * n_ch), gc.DevBuf(4 * n_ch)
    d_bits = gc.DevBuf(n_ch * 1500)
    d_eph = gc.DevBuf(n_ch * gc.GPS_EPH.itemsize)
    p_sol, p_chan = _poison(mm, gc.GPS_FIX_SOL), _poison(n_ch * mm, gc.GPS_FIX_CHAN)
    d_n, d_sol, d_fc = gc.DevBuf(4), gc.DevBuf.from_array(p_sol), gc.DevBuf.from_array(p_chan)
    trk.replay_dev(n_ch, d_chan.ptr, n_ep, d_sums.ptr, d_ep.ptr)
    done = gc.Event()
    done.record(trk.stream)
    done.wait_on(nav.stream)
    off_i, es = gc.epoch_field(gc.SGT_EPOCH, "I_P")
    off_a, _ = gc.epoch_field(gc.SGT_EPOCH, "absoluteSample")
    nav.gps_frames_dev(d_ep.ptr + off_i, es, n_ep * es, n_ep, n_ch, 100, 5, d_first.ptr,
                       d_nb.ptr, d_bits.ptr)
    nav.gps_ephemeris_dev(d_bits.ptr, d_nb.ptr, d_first.ptr, n_ch, d_eph.ptr)
    nav.gps_fix_dev(d_eph.ptr, d_first.ptr, d_ep.ptr + off_a, es, n_ep * es, n_ep,
                    s["rx_first"], gc.gps_fix_cfg(**s["cfg"]), d_n.ptr, d_sol.ptr, d_fc.ptr)
    nav.sync()
    # the final arrays, and the records the restatements start from
    first, n_bits = d_first.download(np.int32), d_nb.download(np.int32)
    bits = d_bits.download(np.uint8).reshape(n_ch, 1500)
    eph = d_eph.download(gc.GPS_EPH)
    n_meas = d_n.download(np.int32)
    sol = d_sol.download(gc.GPS_FIX_SOL).reshape(1, mm)
    chan = d_fc.download(gc.GPS_FIX_CHAN).reshape(n_ch, mm)
    ep = d_ep.download(gc.SGT_EPOCH).reshape(n_ch, n_ep)
    w_first, w_bits = np.zeros(n_ch, np.int32), np.zeros((n_ch, 1500), np.uint8)
    w_nb = np.zeros(n_ch, np.int32)
    for ch in range(n_ch):
        f, b = NB.gps_frames_fast(ep["I_P"][ch], search_start=100)
        w_first[ch], w_nb[ch] = f, b.size
        w_bits[ch, :b.size] = b.ravel()
    assert first.tolist() == w_first.tolist() == s["first"].tolist()
    assert n_bits.tolist() == w_nb.tolist() == [1500] * n_ch
    assert bits.tobytes() == w_bits.tobytes()
    w_eph = S.eph_literal(w_bits, w_nb, w_first)
    assert eph.tobytes() == w_eph.tobytes()
    assert eph.tobytes() == s["eph"].tobytes()                  # and what was planted
    want = S.fix_literal_records(w_eph, w_first, np.ascontiguousarray(ep["absoluteSample"]),
                                 s["rx_first"], s["cfg"],
                                 sol=p_sol.view(gc.GPS_FIX_SOL).reshape(1, mm),
                                 chan=p_chan.view(gc.GPS_FIX_CHAN).reshape(n_ch, mm))
    assert n_meas.tolist() == want[0].tolist() == [mm]
    assert np.array_equal(sol["status"], want[1]["status"]) and not sol["status"].any()
    assert np.array_equal(sol["n_used"], want[1]["n_used"])
    assert np.array_equal(chan["used"], want[2]["used"])
    assert chan["rawP"].tobytes() == want[2]["rawP"].tobytes()
    for g in S.GROUPS:
        dist = S.group_distance((sol, chan), want[1:], g)
        print("chain", g, dist, S.TOL[g])
        assert dist <= S.TOL[g], (g, dist, S.TOL[g])
    # the stages' index conventions line up: the fix lands at the planted receiver, to the
    # few samples (19 m each) by which the tracker's loop moves absolute_sample
    err = np.linalg.norm(np.array([sol["X"][0], sol["Y"][0], sol["Z"][0]]).T - s["planted"][0],
                         axis=1)
    print("chain: distance to the planted receiver", err)
    assert (err < 2000.0).all()


def test_host_twin_equals_the_device_form(gpu):
    nav = gpu.NavCtx()
    for name in ("three_rx", "five_to_three", "few_ready"):
        s = S.fix_scene(name)
        n_meas, sol, chan, p_sol, p_chan = _fix_dev(gpu, nav, s)
        h_sol, h_chan = p_sol.copy(), p_chan.copy()
        h_n, h_sol, h_chan = nav.gps_fix(s["eph"], s["first"], s["abs_sample"], s["rx_first"],
                                         gpu.gps_fix_cfg(**s["cfg"]), sol=h_sol, chan=h_chan)
        assert h_n.tobytes() == n_meas.tobytes()
        assert h_sol.tobytes() == sol.tobytes() and h_chan.tobytes() == chan.tobytes()


def test_bad_arguments_are_refused_and_nothing_is_written(gpu):
    gc, s = gpu, S.fix_scene("three_rx")
    nav = gc.NavCtx()
    n_ch, n_ep = s["abs_sample"].shape
    fill = np.full(1 << 16, 0xAA, np.uint8)
    d_eph, d_first, d_x = (gc.DevBuf.from_array(a) for a in (s["eph"], s["first"], s["abs_sample"]))
    d_n, d_sol, d_chan = (gc.DevBuf.from_array(fill) for _ in range(3))
    good = dict(eph=d_eph.ptr, first=d_first.ptr, x=d_x.ptr, es=8, cs=8 * n_ep, n_ep=n_ep,
                rx_first=s["rx_first"], n=d_n.ptr, sol=d_sol.ptr, chan=d_chan.ptr)

    def fix(cfg_kw=None, cfg=True, **kw):
        a = dict(good, **kw)
        c = gc.gps_fix_cfg(**dict(s["cfg"], **(cfg_kw or {}))) if cfg else None
        nav.gps_fix_dev(a["eph"], a["first"], a["x"], a["es"], a["cs"], a["n_ep"], a["rx_first"],
                        c, a["n"], a["sol"], a["chan"])

    bad = [
        lambda: fix(rx_first=[0, 12, 11, 23]),                 # not ascending
        lambda: fix(rx_first=[0, 12, 12, 23]),
        lambda: fix(rx_first=[1, 12, 16, 23]),
        lambda: fix(rx_first=[0, 65, 66, 67]),                 # more than 64 channels
        lambda: fix(cfg_kw=dict(navSolPeriod=0)), lambda: fix(cfg_kw=dict(samplesPerCode=0.0)),
        lambda: fix(cfg_kw=dict(samplesPerCode=-16000.0)), lambda: fix(cfg_kw=dict(max_meas=0)),
        lambda: fix(eph=None), lambda: fix(first=None), lambda: fix(x=None), lambda: fix(n=None),
        lambda: fix(sol=None), lambda: fix(chan=None), lambda: fix(cfg=False),
        lambda: fix(es=4), lambda: fix(n_ep=0),
        lambda: nav.gps_ephemeris_dev(None, d_first.ptr, d_first.ptr, 3, d_sol.ptr),
        lambda: nav.gps_ephemeris_dev(d_x.ptr, d_first.ptr, d_first.ptr, 3, None),
        lambda: nav.gps_ephemeris_dev(d_x.ptr, d_first.ptr, d_first.ptr, 0, d_sol.ptr),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(gc.GnssCorrError):
            call()
            pytest.fail(f"bad call {i} was accepted")
    # the host twin refuses the same and leaves its arrays alone
    sol = np.frombuffer(_poison(6, gc.GPS_FIX_SOL), gc.GPS_FIX_SOL).reshape(3, 2).copy()
    chan = np.frombuffer(_poison(n_ch * 2, gc.GPS_FIX_CHAN), gc.GPS_FIX_CHAN).reshape(n_ch, 2).copy()
    with pytest.raises(gc.GnssCorrError):
        nav.gps_fix(s["eph"], s["first"], s["abs_sample"], [0, 12, 11, 23],
                    gc.gps_fix_cfg(**s["cfg"]), sol=sol, chan=chan)
    assert (sol.view(np.uint8) == 0xAA).all() and (chan.view(np.uint8) == 0xAA).all()
    nav.sync()
    for d in (d_n, d_sol, d_chan):
        assert d.download(np.uint8).tobytes() == fill.tobytes()


def test_refused_ephemeris_twin_leaves_its_array_alone(gpu):
    """gnsscorr_nav_gps_ephemeris with n_ch = 0: refused by the check it shares with the
    device form, and every byte of the host output is still the sentinel."""
    gc = gpu
    nav = gc.NavCtx()
    bits, n_bits, first, _ = S.eph_scene(3)
    bits, n_bits, first = (np.ascontiguousarray(a) for a in (bits, n_bits, first))
    eph = np.frombuffer(_poison(3, gc.GPS_EPH), gc.GPS_EPH).copy()
    rc = nav._gps_ephemeris(nav.h, bits.ctypes.data, n_bits.ctypes.data, first.ctypes.data, 0,
                            eph.ctypes.data)
    assert rc == -1
    assert "n_ch >= 1" in gc.lib().gnsscorr_last_error().decode()
    assert (eph.view(np.uint8) == 0xAA).all()
