"""GPU: BeiDou B1I ephemeris fields and position fix (csrc/navb1.hip) against the literal
restatement of the Scilab files (tests/navb1_scenarios.py).  The ephemeris record, rawP, used,
n_used, status and n_meas are exact; the outputs behind transcendental functions are held to
navb1_scenarios.TOL, measured on the CPU from the restatement alone (test_navb1_cpu.py).  Every
output starts from 0xAA bytes.  The fix tests print every distance next to its tolerance."""
import numpy as np
import pytest

import navb1_scenarios as S
from nav_fix_gpu_util import check_records, fix_dev, poison as _poison

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ stage 1
@pytest.mark.parametrize("n_ch", [1, 3, 65])
def test_ephemeris_is_byte_equal(gpu, n_ch):
    """every rotation of the subframe IDs, a repeated ID, a missing 1, 2 and 3, IDs 0, 6 and 7;
    a 2 inside the slot with ID 2, inside slot 5 outside bits 8..27 (SOW kept) and inside them
    (NO_SOW); n_subframes 0 / 4 / 5, first = -1; all-ones, sign-bit-only and negative fields;
    bit 88 / bit 120 set with alpha3 / beta1 clear; e with its top bit set; the host twin"""
    gc = gpu
    assert gc.B1_EPH.itemsize == S.EPH.itemsize and gc.B1_EPH.names == S.EPH.names
    nav = gc.NavCtx()
    bits, n_sub, first, _, _ = S.eph_scene(n_ch)
    want = S.eph_literal(bits, n_sub, first)
    d_bits, d_n, d_first = (gc.DevBuf.from_array(a) for a in (bits, n_sub, first))
    d_eph = gc.DevBuf.from_array(_poison(n_ch, gc.B1_EPH))
    nav.b1_ephemeris_dev(d_bits.ptr, d_n.ptr, d_first.ptr, n_ch, d_eph.ptr)
    nav.sync()
    got = d_eph.download(gc.B1_EPH)
    for k in S.EPH.names:
        assert got[k].tobytes() == want[k].tobytes(), (k, got[k][:4], want[k][:4])
    assert got.tobytes() == want.tobytes()
    assert nav.b1_ephemeris(bits, n_sub, first).tobytes() == want.tobytes()


# ------------------------------------------------------------------ stage 2
def _fix_dev(gc, nav, s, in_place=False):
    """-> n_meas, sol, chan and the poisoned arrays they started from"""
    def launch(d_eph, d_first, *series_and_outputs):
        nav.b1_fix_dev(d_eph, d_first, *series_and_outputs[:4], s["rx_first"],
                       gc.b1_fix_cfg(**s["cfg"]), *series_and_outputs[4:])
    return fix_dev(gc, nav, s, launch, in_place)


def _check_fix(name, s, n_meas, sol, chan, p_sol, p_chan, tol=None):
    w_n, Sx, Cx = S.literal_result(name)
    want_sol, want_chan = S.as_records(w_n, Sx, Cx, p_sol, p_chan)
    check_records(S, name, (w_n, want_sol, want_chan, Sx["written"]), n_meas, sol, chan, p_sol,
                  tol)
    unwritten = np.repeat(~Sx["written"], np.diff(s["rx_first"]), axis=0)
    assert chan[unwritten].tobytes() == p_chan[unwritten].tobytes(), name


@pytest.mark.parametrize("name", tuple(S.SCENES) + ("many",))
def test_fix_equals_the_restatement(gpu, name):
    """1, 2, 3 and 65 receivers of 4, 5, 12, 64 and unequal numbers of channels; 1, 2, 3 and 7
    measurements and max_meas below n_meas; a receiver with 3 ready channels; a channel with
    have = 5 and one with NO_SOW, each dropped; the lowest-numbered channel not ready and
    carrying another SOW; SOW - t_oc and time - t_oe across the half-week both ways; satellites
    below 10 degrees, used all the same; a rank-deficient receiver; troposphere on and off;
    padded strides; the host twin equal to the device form"""
    s = S._scene(name)
    nav = gpu.NavCtx()
    n_meas, sol, chan, p_sol, p_chan = _fix_dev(gpu, nav, s)
    _check_fix(name, s, n_meas, sol, chan, p_sol, p_chan)
    h_n, h_sol, h_chan = nav.b1_fix(s["eph"], s["first"], s["abs_sample"], s["rx_first"],
                                    gpu.b1_fix_cfg(**s["cfg"]), sol=p_sol.copy(),
                                    chan=p_chan.copy())
    assert h_n.tobytes() == n_meas.tobytes()
    assert h_sol.tobytes() == sol.tobytes() and h_chan.tobytes() == chan.tobytes()


@pytest.mark.parametrize("name", tuple(S.WORLD_SCENES))
def test_fix_equals_the_restatement_on_the_world_scenes(gpu, name):
    """11 receivers in one launch in every quadrant, south of the equator, on either side of
    the 0 and 180 degree meridians, at the equator and above 80 degrees north and south;
    Kepler loops that run all 10 steps at e from 0.1 to 0.24; GEO-like orbits (i_0 below 0.1
    rad, e below 0.001) among MEO and IGSO ones, seen from 20 N 110 E, troposphere on.  Held to
    TOL_WORLD, measured on these scenes alone; poisoned outputs, padded strides; the host twin
    gives the device form's bytes."""
    s = S.fix_scene(name)
    nav = gpu.NavCtx()
    n_meas, sol, chan, p_sol, p_chan = _fix_dev(gpu, nav, s)
    _check_fix(name, s, n_meas, sol, chan, p_sol, p_chan, S.TOL_WORLD)
    assert not sol["status"].any() and chan["used"].all()
    h_n, h_sol, h_chan = nav.b1_fix(s["eph"], s["first"], s["abs_sample"], s["rx_first"],
                                    gpu.b1_fix_cfg(**s["cfg"]), sol=p_sol.copy(),
                                    chan=p_chan.copy())
    assert h_n.tobytes() == n_meas.tobytes()
    assert h_sol.tobytes() == sol.tobytes() and h_chan.tobytes() == chan.tobytes()


def test_absolute_sample_is_read_in_place_from_epoch_records(gpu):
    nav = gpu.NavCtx()
    for name in ("three_rx", "dropped"):
        _check_fix(name, S.fix_scene(name), *_fix_dev(gpu, nav, S.fix_scene(name), in_place=True))


def test_subframes_to_fix_chain_on_device_buffers(gpu):
    """One receiver of 6 channels over 31 000 epochs: b1_subframes_dev -> b1_ephemeris_dev ->
    b1_fix_dev on device buffers, queued on the context's stream with no host copy in between.
    The I_P series carry five planted subframes: interleaved, under the preamble and the
    Neumann-Hoffman code.  The ephemeris comes out as it went in, the position is the
    restatement's and lies within 1 m of the planted receiver."""
    gc = gpu
    s, series = S.chain_scene()
    n_ch, n_ep = series.shape
    mm = s["cfg"]["max_meas"]
    nav = gc.NavCtx()
    d_series, d_x = gc.DevBuf.from_array(series), gc.DevBuf.from_array(s["abs_sample"])
    d_first, d_ns = gc.DevBuf.from_array(_poison(n_ch, np.int32)), \
        gc.DevBuf.from_array(_poison(n_ch, np.int32))
    d_bits = gc.DevBuf.from_array(_poison(n_ch * 5 * 213, np.uint8))
    d_eph = gc.DevBuf.from_array(_poison(n_ch, gc.B1_EPH))
    p_sol, p_chan = _poison(mm, gc.GPS_FIX_SOL), _poison(n_ch * mm, gc.GPS_FIX_CHAN)
    d_n, d_sol, d_fc = gc.DevBuf.from_array(_poison(1, np.int32)), gc.DevBuf.from_array(p_sol), \
        gc.DevBuf.from_array(p_chan)
    cfg = gc.b1_fix_cfg(**s["cfg"])
    nav.b1_subframes_dev(d_series.ptr, 8, 8 * n_ep, n_ep, n_ch, 5, d_first.ptr, d_ns.ptr,
                         d_bits.ptr)
    nav.b1_ephemeris_dev(d_bits.ptr, d_ns.ptr, d_first.ptr, n_ch, d_eph.ptr)
    nav.b1_fix_dev(d_eph.ptr, d_first.ptr, d_x.ptr, 8, 8 * n_ep, n_ep, s["rx_first"], cfg,
                   d_n.ptr, d_sol.ptr, d_fc.ptr)
    nav.sync()
    first, n_sub = d_first.download(np.int32), d_ns.download(np.int32)
    bits = d_bits.download(np.uint8).reshape(n_ch, 5, 213)
    eph, n_meas = d_eph.download(gc.B1_EPH), d_n.download(np.int32)
    sol = d_sol.download(gc.GPS_FIX_SOL).reshape(1, mm)
    chan = d_fc.download(gc.GPS_FIX_CHAN).reshape(n_ch, mm)
    assert first.tolist() == s["first"].tolist() and n_sub.tolist() == [5] * n_ch
    assert bits.tobytes() == s["bits"].tobytes()
    assert eph.tobytes() == s["eph"].tobytes()
    p_sol, p_chan = p_sol.view(gc.GPS_FIX_SOL).reshape(1, mm), p_chan.view(gc.GPS_FIX_CHAN).reshape(n_ch, mm)
    w_n, Sx, Cx = S.fix_literal(s["eph"], first, s["abs_sample"], s["rx_first"], s["cfg"])
    want_sol, want_chan = S.as_records(w_n, Sx, Cx, p_sol, p_chan)
    assert n_meas.tolist() == [mm] and not sol["status"].any()
    check_records(S, "chain", (w_n, want_sol, want_chan, Sx["written"]), n_meas, sol, chan, p_sol)
    err = np.linalg.norm(np.array([sol["X"][0], sol["Y"][0], sol["Z"][0]]).T - s["planted"][0],
                         axis=1)
    print("chain: distance to the planted receiver", err)
    assert (err < 1.0).all()


def test_bad_arguments_are_refused_and_nothing_is_written(gpu):
    gc, s = gpu, S.fix_scene("three_rx")
    nav = gc.NavCtx()
    n_ch, n_ep = s["abs_sample"].shape
    fill = np.full(1 << 16, 0xAA, np.uint8)
    d_eph, d_first, d_x = (gc.DevBuf.from_array(a) for a in (s["eph"], s["first"], s["abs_sample"]))
    d_n, d_sol, d_chan, d_out = (gc.DevBuf.from_array(fill) for _ in range(4))
    good = dict(eph=d_eph.ptr, first=d_first.ptr, x=d_x.ptr, es=8, cs=8 * n_ep, n_ep=n_ep,
                rx_first=s["rx_first"], n=d_n.ptr, sol=d_sol.ptr, chan=d_chan.ptr)

    def fix(cfg_kw=None, cfg=True, **kw):
        a = dict(good, **kw)
        c = gc.b1_fix_cfg(**dict(s["cfg"], **(cfg_kw or {}))) if cfg else None
        nav.b1_fix_dev(a["eph"], a["first"], a["x"], a["es"], a["cs"], a["n_ep"], a["rx_first"],
                       c, a["n"], a["sol"], a["chan"])

    ok = gc.b1_fix_cfg(**s["cfg"])
    bad = [
        lambda: fix(rx_first=[0, 12, 11, 23]),                 # not ascending
        lambda: fix(rx_first=[0, 12, 12, 23]),
        lambda: fix(rx_first=[1, 12, 16, 23]),
        lambda: fix(rx_first=[0, 65, 66, 67]),                 # more than 64 channels
        lambda: fix(cfg_kw=dict(navSolPeriod=0)), lambda: fix(cfg_kw=dict(samplesPerCode=0.0)),
        lambda: fix(cfg_kw=dict(samplesPerCode=-16000.0)), lambda: fix(cfg_kw=dict(max_meas=0)),
        lambda: fix(cfg_kw=dict(dataTypeSizeInBytes=0.0)),
        lambda: fix(cfg_kw=dict(dataTypeSizeInBytes=-1.0)),
        lambda: fix(eph=None), lambda: fix(first=None), lambda: fix(x=None), lambda: fix(n=None),
        lambda: fix(sol=None), lambda: fix(chan=None), lambda: fix(cfg=False),
        lambda: fix(es=4), lambda: fix(cs=12), lambda: fix(n_ep=0),
        lambda: nav.b1_ephemeris_dev(None, d_first.ptr, d_first.ptr, 3, d_out.ptr),
        lambda: nav.b1_ephemeris_dev(d_x.ptr, None, d_first.ptr, 3, d_out.ptr),
        lambda: nav.b1_ephemeris_dev(d_x.ptr, d_first.ptr, None, 3, d_out.ptr),
        lambda: nav.b1_ephemeris_dev(d_x.ptr, d_first.ptr, d_first.ptr, 3, None),
        lambda: nav.b1_ephemeris_dev(d_x.ptr, d_first.ptr, d_first.ptr, 0, d_out.ptr),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(gc.GnssCorrError):
            call()
            pytest.fail(f"bad call {i} was accepted")
    # the host twins refuse the same and leave their arrays alone
    sol = np.frombuffer(_poison(6, gc.GPS_FIX_SOL), gc.GPS_FIX_SOL).reshape(3, 2).copy()
    chan = np.frombuffer(_poison(n_ch * 2, gc.GPS_FIX_CHAN), gc.GPS_FIX_CHAN).reshape(n_ch, 2).copy()
    with pytest.raises(gc.GnssCorrError):
        nav.b1_fix(s["eph"], s["first"], s["abs_sample"], [0, 12, 11, 23], ok, sol=sol, chan=chan)
    assert (sol.view(np.uint8) == 0xAA).all() and (chan.view(np.uint8) == 0xAA).all()
    eph = np.frombuffer(_poison(3, gc.B1_EPH), gc.B1_EPH).copy()
    bits, n_sub, first, _, _ = S.eph_scene(3)
    rc = nav._b1_ephemeris(nav.h, bits.ctypes.data, n_sub.ctypes.data, first.ctypes.data, 0,
                           eph.ctypes.data)
    assert rc == -1 and "n_ch >= 1" in gc.lib().gnsscorr_last_error().decode()
    assert (eph.view(np.uint8) == 0xAA).all()
    nav.sync()
    for d in (d_n, d_sol, d_chan, d_out):
        assert d.download(np.uint8).tobytes() == fill.tobytes()
