"""CPU: the two restatements of the BeiDou B1I field decoding and position fix
(tests/navb1_scenarios.py) against each other and against what the generators planted, the
conditions that keep the scenes away from every decision threshold, and the tolerances of
tests/test_navb1_gpu.py: measured from the literal restatement alone, and shown to tell every
planted mistake from the file's text."""
import ctypes

import numpy as np
import pytest

import navb1_scenarios as S

ALL = tuple(S.SCENES) + ("many",)
WORLD = tuple(S.WORLD_SCENES)
EXACT_SOL, EXACT_CHAN = ("status", "n_used", "written"), ("used", "rawP")


@pytest.mark.parametrize("n_ch", [1, 3, 65])
def test_field_decode_equals_what_was_planted(n_ch):
    bits, n_sub, first, orders, raws = S.eph_scene(n_ch)
    lit = S.eph_literal(bits, n_sub, first)
    for ch in range(n_ch):
        if lit["status"][ch] == S.EPH_SHORT:
            assert not any(lit[k][ch] for k in S.EPH_FIELDS + S.EPH_INTS if k != "status")
            continue
        ids = [0 if (bits[ch, i] > 1).any() else sid for i, sid in enumerate(orders[ch])]
        assert lit["have"][ch] == sum(1 << (i - 1) for i in (1, 2, 3) if i in ids)
        want = S.raw_to_values(raws[ch])
        for k, (sf, *_) in S.FIELDS.items():
            assert lit[k][ch] == (want[k] if sf in ids else 0), (ch, k)
        assert lit["t_oe"][ch] == (want["t_oe"] if 2 in ids and 3 in ids else 0)
        sow = bits[ch, 4, 7:27]
        if (sow > 1).any():
            assert lit["status"][ch] == S.EPH_NO_SOW and lit["SOW"][ch] == 0
        else:
            assert lit["status"][ch] == S.EPH_OK
            assert lit["SOW"][ch] == int("".join(map(str, sow)), 2) - 24
    if n_ch == 65:
        assert lit["status"][[1, 8, 9]].tolist() == [S.EPH_SHORT] * 3
        assert lit["have"][10] == 5 and lit["t_oe"][10] == 0 and lit["t_oe_lsb"][10] != 0
        assert lit["status"][11] == S.EPH_OK and lit["have"][11] == 7      # slot 5 skipped, SOW kept
        assert lit["status"][12] == S.EPH_NO_SOW and lit["have"][12] == 6
        assert lit["alpha3"][13] == -256 * 2.0 ** -24 and lit["beta1"][14] == -256 * 2.0 ** 14
        assert lit["e"][15] < 0
        assert {7, 6, 5, 3} <= set(lit["have"].tolist())
        for k in S.SIGNED:
            assert (lit[k] < 0).any() and (lit[k] > 0).any(), k
        assert (lit["sqrtA"] >= 4096).any()                    # top bit set, read unsigned


@pytest.mark.parametrize("mutant", S.EPH_MUTANTS)
def test_field_mutants_change_the_record(mutant):
    """the quirk cases and the e with its top bit set tell the file's text from the fix"""
    bits, n_sub, first, _, _ = S.eph_scene(65)
    a, b = S.eph_literal(bits, n_sub, first), S.eph_literal(bits, n_sub, first, mutant)
    field = mutant.split("_")[0]
    assert (a[field] != b[field]).any()
    ch = {"alpha3": 13, "beta1": 14, "e": 15}[field]
    assert a[field][ch] != b[field][ch]
    assert all((a[k] == b[k]).all() for k in S.EPH.names if k != field)


@pytest.mark.parametrize("name", ALL + WORLD)
def test_literal_equals_fast(name):
    s = S._scene(name)
    tol = S.TOL_WORLD if name in WORLD else S.TOL
    n_l, Sl, Cl = S.literal_result(name)
    n_f, Sf, Cf = S.fix_fast(s["eph"], s["first"], s["abs_sample"], s["rx_first"], s["cfg"])
    assert n_l.tolist() == n_f.tolist()
    for k in EXACT_SOL:
        assert np.array_equal(Sl[k], Sf[k]), k
    for k in EXACT_CHAN:
        assert np.asarray(Cl[k], np.float64).tobytes() == np.asarray(Cf[k], np.float64).tobytes(), k
    for g in S.GROUPS:
        dist = S.group_distance((Sl, Cl), (Sf, Cf), g)
        assert dist <= tol[g], (name, g, dist, tol[g])


@pytest.mark.parametrize("name", ALL + WORLD)
def test_scene_conditions(name):
    """cond(A) < 1e6 and GDOP < 6 wherever a receiver is solved, on every scene a tolerance is
    measured on; no Kepler or togeod exit within a factor 4 of its threshold"""
    s = S._scene(name)
    full = S.SCENES[name][1] if name in S.SCENES else True     # WORLD_SCENES: all full rank
    d = S.scene_diagnostics(s)
    assert S.conditions_hold(s, full_rank=full), {k: (v.min(), v.max()) for k, v in d.items()
                                                   if len(v)}
    n, Sx, Cx = S.literal_result(name)
    solved = Sx["written"] & (Sx["status"] == S.FIX_OK)
    assert len(d["gdop"]) == solved.sum() and len(d["togeod_all"]) == 6 * solved.sum()
    if not full:                                               # the deficient receiver is no
        assert (Sx["status"] == S.FIX_RANK).any()              # part of any tolerance
        assert (d["cond"] < 1e6).all() and (d["gdop"] < 6).all()


def test_scenes_show_what_they_are_named_for():
    n, Sx, Cx = S.literal_result("three_ready")
    assert n.tolist() == [0, 2] and not Sx["written"][0].any()
    s = S.fix_scene("dropped")
    n, Sx, Cx = S.literal_result("dropped")
    assert s["eph"]["have"][2] == 5 and s["eph"]["status"][10] == S.EPH_NO_SOW
    assert Cx["used"][2].tolist() == [0, 0] and Cx["used"][10].tolist() == [0, 0]
    assert np.isinf(Cx["rawP"][2]).all() and np.isnan(Cx["el"][10]).all()
    assert Sx["n_used"].tolist() == [[5, 5], [5, 5]] and not Sx["status"].any()
    s = S.fix_scene("first_not_ready")
    n, Sx, Cx = S.literal_result("first_not_ready")
    assert s["eph"]["have"][0] == 3 and s["eph"]["SOW"][0] == s["eph"]["SOW"][1] + 600
    assert Sx["n_used"].tolist() == [[4, 4]] and Cx["used"][:, 0].tolist() == [0, 1, 1, 1, 1, 0]
    n, Sx, Cx = S.literal_result("rank")
    assert Sx["status"].tolist() == [[S.FIX_RANK] * 2, [S.FIX_OK] * 2]
    assert not Sx["X"][0].any() and np.isnan(Cx["el"][:5]).all() and Cx["used"][:5].all()
    n, Sx, Cx = S.literal_result("max_meas_below")
    assert n.tolist() == [2]                                   # 300 epochs hold 14 periods of 20
    assert S.literal_result("one_rx_5")[0].tolist() == [7]
    n, Sx, Cx = S.literal_result("low_sats")
    assert (Cx["el"][5:, 0] < 10).all() and Cx["used"].all()   # below a mask, used all the same
    for name, sign in (("week_start", -1), ("week_end", 1)):   # both branches of check_t
        s = S.fix_scene(name)
        assert ((s["sow"] - s["toe"]) * sign > 302400) and s["eph"]["t_oe"][0] == s["toe"]
        assert not S.literal_result(name)[1]["status"].any()
    kinds = {float(v) > 6000 for v in S.many_rx_scene()["eph"]["sqrtA"]}
    assert kinds == {True, False}                              # MEO and IGSO


def test_planted_position_is_recovered():
    """exact geometric ranges, troposphere off: the fix lands on the planted receiver, the
    only error being the solver's.  The bound is 1 m."""
    worst = 0.0
    for name in ALL:
        s = S._scene(name)
        if s["cfg"]["useTropCorr"]:
            continue
        n, Sx, Cx = S.literal_result(name)
        for rx in range(len(n)):
            for m in range(n[rx]):
                if Sx["status"][rx, m] == S.FIX_OK:
                    p = np.array([Sx[k][rx, m] for k in "XYZ"])
                    worst = max(worst, float(np.linalg.norm(p - s["planted"][rx])))
    print("planted position recovered to", worst, "m")
    assert 0 < worst < 1.0


def test_tolerances_are_the_measured_spread_times_16():
    got = S.measure_spread()
    print(got)
    for g, v in got.items():
        assert v <= S.SPREAD[g] * 1.001, (g, v)                # the constants are what is measured
        assert v >= S.SPREAD[g] * 0.5, (g, v)
        assert S.TOL[g] == 16 * S.SPREAD[g]


MUTANT_SCENES = {"gps_consts": ALL[:3], "start_offset": ALL[:3], "obs_sign": ALL[:3],
                 "mask": ("low_sats",)}


def _moves(name, mutant):
    """the groups a mutant moves by more than their tolerance, and the exact outputs it changes"""
    a, b = S.literal_result(name), S.literal_result(name, mutant=mutant)
    moved = set()
    if a[0].tolist() != b[0].tolist():
        moved.add("n_meas")
    for k in EXACT_SOL:
        if not np.array_equal(a[1][k], b[1][k]):
            moved.add(k)
    for k in EXACT_CHAN:
        if np.asarray(a[2][k]).tobytes() != np.asarray(b[2][k]).tobytes():
            moved.add(k)
    if moved & {"n_meas", "status", "written", "used"}:
        return moved                                           # NaN patterns differ from here on
    for g in S.GROUPS:
        if S.group_distance(a[1:], b[1:], g) > S.TOL[g]:
            moved.add(g)
    return moved


@pytest.mark.parametrize("mutant", S.FIX_MUTANTS)
def test_every_fix_mutant_moves_an_output(mutant):
    """each planted mistake moves at least one output of at least one scene by more than its
    tolerance: the GPU comparison can fail for the right reasons"""
    moved = {name: _moves(name, mutant) for name in MUTANT_SCENES[mutant]}
    print(mutant, moved)
    assert any(moved.values()), mutant
    if mutant == "gps_consts":
        assert all("xyz" in m for m in moved.values())
    if mutant == "start_offset":
        assert all("rawP" in m for m in moved.values())
    if mutant == "obs_sign":
        assert all("xyz" in m or "dt" in m for m in moved.values())
    if mutant == "mask":
        assert "used" in moved["low_sats"]


def test_struct_sizes_and_field_names_match_the_library(gc):
    assert gc.B1_EPH.itemsize == S.EPH.itemsize == 280 and gc.B1_EPH.names == S.EPH.names
    assert [gc.B1_EPH.fields[k][1] for k in S.EPH.names] == [S.EPH.fields[k][1] for k in S.EPH.names]
    assert gc.B1_FIX_CFG.itemsize == 40
    assert (gc.B1_EPH_OK, gc.B1_EPH_SHORT, gc.B1_EPH_NO_SOW) == (S.EPH_OK, S.EPH_SHORT, S.EPH_NO_SOW)
    cfg = gc.b1_fix_cfg()
    got = {k: getattr(cfg, k) for k in S.DEFAULTS}
    assert got == S.DEFAULTS
    assert gc.b1_fix_cfg(3, navSolPeriod=20).max_meas == 3
    with pytest.raises(gc.GnssCorrError):
        gc.b1_fix_cfg(elevationMask=10.0)                      # the receiver has no mask
    assert ctypes.sizeof(gc.B1Eph) == 280 and ctypes.sizeof(gc.B1FixCfg) == 40
    for fn in ("ephemeris", "fix"):
        assert hasattr(gc.lib(), f"gnsscorr_nav_b1_{fn}_dev") and hasattr(gc.lib(), f"gnsscorr_nav_b1_{fn}")
    assert hasattr(gc.lib(), "gnsscorr_nav_b1_fix_cfg_init")


# ------------------------------------------------------------------ the scenes of WORLD_SCENES
@pytest.mark.parametrize("name", WORLD)
def test_world_scenes_show_what_they_are_named_for(name):
    """every receiver solved at every measurement and no check_t wrap; world: each receiver's
    solved latitude and longitude in its site's class, both sides of both meridians; eccentric: every Kepler
    loop ran its 10 steps and left by the cap with |dE| > 4e-12; geo: three GEO-like orbits
    (sqrtA near 6493.4, i_0 below 0.1 rad, e below 0.001) beside MEO and IGSO ones, seen from
    near (20 N, 110 E) with GDOP below 5"""
    s = S.fix_scene(name)
    assert S.named_for_missed(name, s) == []
    d = S.scene_diagnostics(s)
    n_calls = int(s["rx_first"][-1]) * s["cfg"]["max_meas"]
    assert len(d["tk"]) == len(d["kepler"]) == n_calls
    if name == "world":
        n, Sx, Cx = S.literal_result(name)
        assert len(n) == len(S.G.SITES) == 11 and s["sizes"] == S.G.WORLD_SIZES
        assert (Sx["Z"] < 0).sum() >= 2 * 5 and (Sx["X"] < 0).any() and (Sx["Y"] > 0).any()
    if name == "eccentric":
        assert d["kepler"][:, 0].sum() == 10 * n_calls and (d["kepler"][:, 1] > 4e-12).all()
        assert (s["eph"]["e"] >= 0.1).all() and (s["eph"]["e"] < 0.25).all()
    if name == "geo":
        n, Sx, Cx = S.literal_result(name)
        assert abs(Sx["lat"][0, 0] - 20) < 2.5 and abs(Sx["lon"][0, 0] - 110) < 2.5
        assert (np.abs(s["eph"]["sqrtA"][:3] - 6493.4) < 0.5).all() and (d["gdop"] < 5).all()
        assert (np.abs(s["eph"]["i_0"][:3]) < 0.1).all() and (s["eph"]["e"][:3] < 0.001).all()
        assert (Cx["el"][:3] > 18).all()                       # high in the sky, and used


def test_world_tolerances_are_the_measured_spread_times_16():
    got = S.measure_spread(WORLD)
    print(got)
    for g, v in got.items():
        assert v <= S.SPREAD_WORLD[g] * 1.001, (g, v)          # the constants are what is measured
        assert v >= S.SPREAD_WORLD[g] * 0.5, (g, v)
        assert S.TOL_WORLD[g] == 16 * S.SPREAD_WORLD[g]


def _xyz_move(name, mutant):
    n0, S0, C0 = S.literal_result(name)
    n1, S1, C1 = S.literal_result(name, mutant=mutant)
    assert not S0["status"].any() and not S1["status"].any() and S0["written"].all()
    return np.max([np.abs(S1[k] - S0[k]) for k in "XYZ"], axis=0)


def test_kepler_cap_mutant_moves_the_eccentric_scene():
    """20 steps in place of 10 move X Y Z of every measurement by more than 100 tolerances"""
    move = _xyz_move("eccentric", "kepler_20")
    print(move, 100 * S.TOL_WORLD["xyz"])
    assert (move > 100 * S.TOL_WORLD["xyz"]).all()


def test_check_t_mutant_moves_the_week_scenes():
    """the week scenes of SCENES catch a check_t that returns its argument: X Y Z of every
    measurement by more than 100 tolerances"""
    for name in ("week_start", "week_end"):
        move = _xyz_move(name, "check_t_identity")
        print(name, move, 100 * S.TOL["xyz"])
        assert (move > 100 * S.TOL["xyz"]).all()


@pytest.mark.parametrize("mutant", ["kepler_20", "check_t_identity"] + list(S.GEO_MUTANTS))
@pytest.mark.parametrize("name", ALL)
def test_world_mutants_leave_every_earlier_scene_as_it_was(name, mutant):
    """bit for bit, but for check_t in the two week scenes: no other scene of SCENES, and not
    many_rx_scene, reaches what these mutants change"""
    if mutant == "check_t_identity" and name.startswith("week"):
        return
    a, b = S.literal_result(name), S.literal_result(name, mutant=mutant)
    assert a[0].tolist() == b[0].tolist()
    ra, rb = S.as_records(*a), S.as_records(*b)
    assert ra[0].tobytes() == rb[0].tobytes() and ra[1].tobytes() == rb[1].tobytes()


# mutant: (the outputs that must move, their tolerance group, which receivers: sign of Z or X)
GEO_MUTANTS = {"togeod_abs_z": (("el", "az"), "elaz", "Z"), "cart2geo_abs_z": (("lat",), "latlon", "Z"),
               "cart2geo_atan_y_over_x": (("lon",), "latlon", "X")}


@pytest.mark.parametrize("mutant", GEO_MUTANTS)
def test_geo_mutants_move_the_world_scene(mutant):
    """fabs(Z) in togeod and in cart2geo and atan(Y / X) for the longitude move the named
    outputs of every measurement of the receivers they concern, the southern ones and those
    with X < 0, by more than 100 tolerances, and no output of any other receiver"""
    keys, group, axis = GEO_MUTANTS[mutant]
    s = S.fix_scene("world")
    n0, S0, C0 = S.literal_result("world")
    n1, S1, C1 = S.literal_result("world", mutant=mutant)
    assert not S0["status"].any() and not S1["status"].any()   # no mask: nothing drops out
    if keys[0] in C0:
        per_ch = np.max([np.abs(C1[k] - C0[k]) for k in keys], axis=0)
        move = np.array([per_ch[a:b].max(axis=0) for a, b in zip(s["rx_first"], s["rx_first"][1:])])
    else:
        move = np.max([np.abs(S1[k] - S0[k]) for k in keys], axis=0)
    hit = S0[axis] < 0
    print(mutant, move[hit].min(), 100 * S.TOL_WORLD[group])
    assert hit.any() and (~hit).any()
    assert (move[hit] > 100 * S.TOL_WORLD[group]).all(), (mutant, move[hit].min())
    assert not move[~hit].any(), (mutant, move[~hit].max())
