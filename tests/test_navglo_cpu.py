"""CPU: the restatement of the GLONASS L1OF field decoding, satellite integration and position
fix (tests/navglo_scenarios.py) against what the generators planted, the conditions that keep
the scenes away from every decision threshold, the file's column bookkeeping against the
library's, and the tolerances of tests/test_navglo_gpu.py: measured from the restatement alone,
and shown to discriminate."""
import ctypes

import numpy as np
import pytest

import navglo_scenarios as S

ALL = tuple(S.SCENES) + ("many",)
WORLD = tuple(S.WORLD_SCENES)
MULTI = tuple(k for k, (_, multi) in S.SCENES.items() if multi)


@pytest.mark.parametrize("n_ch", [1, 3, 65])
def test_field_decode_equals_what_was_planted(n_ch):
    bits, n_strings, first, orders, raws = S.eph_scene(n_ch)
    lit = S.eph_literal(bits, n_strings, first)
    for ch in range(n_ch):
        if lit["status"][ch] != S.EPH_OK:
            assert not any(lit[k][ch] for k in S.EPH_FIELDS + S.EPH_INTS if k != "status")
            continue
        skipped = [i for i in range(15) if (bits[ch, i] > 1).any()]
        assert lit["skipped"][ch] == sum(1 << i for i in skipped)
        nums = [0 if i in skipped else n for i, n in enumerate(orders[ch])]
        if ch == 13:
            nums[skipped[0]] = 0
        want = S.raw_to_values(raws[ch])
        assert lit["have"][ch] == sum(1 << (i - 1) for i in range(1, 6) if i in nums)
        pos1 = max([i + 1 for i, n in enumerate(nums) if n == 1], default=0)
        assert lit["string_1_pos"][ch] == pos1
        for k, (num, *_) in S.FIELDS.items():
            v = want[k] if num in nums else 0
            assert lit[k][ch] == v and np.signbit(lit[k][ch]) == np.signbit(v), (ch, k)
        tk = lit["tk_h"][ch] * 3600 + lit["tk_m"][ch] * 60 + lit["tk_s"][ch]
        assert lit["t"][ch] == (tk - 2 * (pos1 - 1)) - 0.3
    if n_ch == 65:
        assert lit["status"][[1, 8, 9]].tolist() == [S.EPH_SHORT] * 3
        assert lit["skipped"][[10, 11, 12, 13]].all() and lit["have"][10] == 29
        assert lit["have"][21] == 23 and lit["t"][22] == 1.7 and lit["string_1_pos"][22] == 0
        assert sorted(set(lit["string_1_pos"][lit["status"] == 0].tolist())) == list(range(16))
        for k in S.SIGNED:                                     # -0.0, and every sign
            assert (np.signbit(lit[k]) & (lit[k] == 0)).any() and (lit[k] < 0).any(), k


def test_satpos_scenes_cover_the_loop_counts():
    """deltat positive, negative and exactly 0; n10 in {0, 1, 90}; n1 in {0, 9}; n001 0, 199
    and 200, 799 and 800, 999"""
    seen = {"n10": set(), "n1": set(), "n001": set(), "sign": set()}
    for period in S.SAT_SCENES:
        eph = S.sat_scene(period)
        ready, deltat, n10, n1, n001 = S.satpos_decisions(eph, period)
        assert ready.sum() == 61 and not ready[[5, 17, 29, 41]].any()
        seen["n10"] |= set(n10[ready].tolist())
        seen["n1"] |= set(n1[ready].tolist())
        seen["n001"] |= set(n001[ready].tolist())
        seen["sign"] |= set(np.sign(deltat[ready]).tolist())
        whole = np.abs(deltat[ready] - np.round(deltat[ready])) > 0
        print(period, "deltat off a whole ms:", whole.sum(), "of", ready.sum())
    assert {0, 1, 90} <= seen["n10"] and {0, 9} <= seen["n1"]
    assert {0, 199, 200, 799, 800, 999} <= seen["n001"]
    assert seen["sign"] == {-1.0, 0.0, 1.0}


def test_integration_follows_the_orbit():
    """the integrated state stays on the planted orbit: radius within 2 km of 25 510 km after
    up to 15 minutes, and the state at deltat = 0 is the ephemeris itself"""
    for period in S.SAT_SCENES:
        eph, lit = S.sat_scene(period), S.sat_literal(period)
        ok = lit["ready"] == 1
        r = np.linalg.norm(lit["pos"][ok], axis=1)
        assert (np.abs(r - S.ORBIT_R) < 2000.0).all(), np.abs(r - S.ORBIT_R).max()
        still = ok & (lit["deltat"] == 0)
        for ch in np.flatnonzero(still):
            assert lit["pos"][ch].tolist() == [eph[k][ch] * 1000 for k in "xyz"]
    assert (S.sat_literal(700)["deltat"] == 0).any()


@pytest.mark.parametrize("name", ALL + WORLD)
def test_scene_conditions(name):
    """cond(A) < 1e6 and GDOP < 6 where a receiver is full rank; no elevation within 1e-6
    degrees of the mask; no togeod exit within a factor 4 of its threshold"""
    s = S._scene(name)
    d = S.scene_diagnostics(s)
    assert S.conditions_hold(s, full_rank=True), {k: (v.min(), v.max()) for k, v in d.items()
                                                   if len(v)}
    assert len(d["togeod_all"])


def test_frame_times_lie_on_both_sides_of_tb():
    dt = np.concatenate([S.scene_sat(n)["deltat"][S.scene_sat(n)["ready"] == 1] for n in ALL])
    assert (dt > 0).any() and (dt < 0).any() and (np.abs(dt) < 900e3).all()
    tb = np.concatenate([S._scene(n)["eph"]["tb"] for n in ALL])
    assert (tb % 15 == 0).all()
    p1 = np.concatenate([S._scene(n)["eph"]["string_1_pos"] for n in ALL])
    assert set(p1.tolist()) >= set(range(1, 16))


def test_scenes_show_what_they_are_named_for():
    n, Sx, Cx = S.literal_result("drop_one")
    assert Sx["n_used"][0].tolist() == [7, 6, 6] and Cx["used"][0].tolist() == [1, 0, 0]
    assert np.isnan(Cx["el"][0, 1:]).all() and np.isinf(Cx["rawP"][0, 1:]).all()
    assert Cx["el"][0, 0] < 10.0
    n, Sx, Cx = S.literal_result("five_to_three")
    assert Sx["status"][0].tolist() == [S.FIX_OK, S.FIX_FEW, S.FIX_FEW]
    assert np.isnan(Sx["X"][0, 1:]).all() and not Sx["DOP"][0, 1:].any()
    n, Sx, Cx = S.literal_result("few_ready")
    assert n.tolist() == [0, 2] and not Sx["written"][0].any()
    s = S.fix_scene("few_ready")
    assert s["eph"]["status"][1] == S.EPH_SHORT and s["eph"]["have"][3] == 23
    s = S.fix_scene("health")
    n, Sx, Cx = S.literal_result("health")
    assert s["eph"]["Bn"][2] == 4 and s["eph"]["In3"][11] == 1
    assert Cx["used"][2].tolist() == [0, 0] and Cx["used"][11].tolist() == [0, 0]
    assert Sx["n_used"].tolist() == [[5, 5], [5, 5]] and not Sx["status"].any()
    n, Sx, Cx = S.literal_result("rank")
    assert Sx["status"].tolist() == [[S.FIX_RANK] * 2, [S.FIX_OK] * 2]
    assert not Sx["X"][0].any() and np.isnan(Cx["el"][:5]).all()
    n, Sx, Cx = S.literal_result("max_meas_below")
    assert n.tolist() == [2]                                   # 300 epochs hold 14 periods of 20
    n, Sx, Cx = S.literal_result("one_rx_5")
    assert n.tolist() == [7]


def test_planted_position_is_recovered():
    """the fix lands on the planted receiver (PZ-90.02) moved to WGS-84: without troposphere
    to 1 mm over the scene; the bound is 1 m"""
    s = S.fix_scene("notrop")
    n, Sx, Cx = S.literal_result("notrop")
    worst = 0.0
    for rx in range(2):
        want = np.array(S.pz90_to_wgs84(np.float64, list(s["planted"][rx])))
        for m in range(n[rx]):
            p = np.array([Sx["X"][rx, m], Sx["Y"][rx, m], Sx["Z"][rx, m]])
            worst = max(worst, float(np.linalg.norm(p - want)))
    print("planted position recovered to", worst, "m")
    assert worst < 1.0


@pytest.mark.parametrize("name", MULTI)
def test_file_columns_equal_per_channel_states_without_an_exclusion(name):
    a, b = S.literal_result(name), S.literal_result(name, columns="file")
    ra, rb = S.G.as_records(*a), S.G.as_records(*b)
    assert ra[0].tobytes() == rb[0].tobytes() and ra[1].tobytes() == rb[1].tobytes()


def test_file_columns_differ_after_an_exclusion():
    """drop_one: lane 0 of 7 leaves after the first fix.  The first fix is the same; from the
    second on the file's list holds lanes 1..6 while its columns 0..5 still hold the states of
    lanes 0..5, and its position is off by kilometres.  The library keeps each channel's own."""
    a, b = S.literal_result("drop_one"), S.literal_result("drop_one", columns="file")
    ra, rb = S.G.as_records(*a), S.G.as_records(*b)
    assert ra[0][0, 0].tobytes() == rb[0][0, 0].tobytes()
    assert ra[1][:, 0].tobytes() == rb[1][:, 0].tobytes()
    assert a[1]["n_used"][0, 1] == b[1]["n_used"][0, 1] == 6
    move = abs(a[1]["X"][0, 1] - b[1]["X"][0, 1])
    print("the file's second fix is off by", move, "m")
    assert move > 1000.0
    s = S.fix_scene("drop_one")
    want = np.array(S.pz90_to_wgs84(np.float64, list(s["planted"][0])))
    for m in range(3):                                         # the library's stays put
        p = np.array([a[1][k][0, m] for k in "XYZ"])
        assert np.linalg.norm(p - want) < 1.0


def test_tolerances_are_the_measured_spread_times_16():
    got = S.measure_spread()
    print(got)
    for g, v in got.items():
        assert v <= S.SPREAD[g] * 1.001, (g, v)                # the constants are what is measured
        assert v >= S.SPREAD[g] * 0.5, (g, v)
        assert S.TOL[g] == 16 * S.SPREAD[g]


def _xyz_move(name, mutant):
    s = S.fix_scene(name)
    n, Sm, Cm = S.fix_literal(s["eph"], s["first"], s["abs_sample"], s["rx_first"], s["cfg"],
                              mutant=mutant, sat=S.scene_sat(name))
    n0, S0, C0 = S.literal_result(name)
    ok = S0["written"] & (S0["status"] == S.FIX_OK)
    return np.max([np.abs(Sm[k][ok] - S0[k][ok]) for k in ("X", "Y", "Z")], axis=0)


@pytest.mark.parametrize("mutant", ["no_erot", "no_trop"])
def test_tolerances_discriminate(mutant):
    """every mutant of the restatement moves X Y Z of every solved measurement of every
    multi-measurement scene by more than 100 tolerances"""
    for name in MULTI:
        if mutant == "no_trop" and S.fix_scene(name)["cfg"]["useTropCorr"] != 1:
            continue
        move = _xyz_move(name, mutant)
        print(mutant, name, move.min())
        assert (move > 100 * S.TOL["xyz"]).all(), (mutant, name, move.min())


def test_state_tolerance_discriminates():
    """one 1-ms step more or less moves a satellite by metres: 1e5 tolerances"""
    lit = S.sat_literal(500)
    ok = lit["ready"] == 1
    speed = np.linalg.norm(lit["vel"][ok], axis=1)
    assert (speed * 0.001 > 1e5 * S.TOL["state_pos"]).all()


def test_struct_sizes_and_field_names_match_the_library(gc):
    assert gc.GLO_EPH.itemsize == S.EPH.itemsize == 216 and gc.GLO_EPH.names == S.EPH.names
    assert gc.GLO_SAT.itemsize == S.SAT.itemsize == 104 and gc.GLO_SAT.names == S.SAT.names
    assert [gc.GLO_SAT.fields[k][1] for k in S.SAT.names] == [S.SAT.fields[k][1] for k in S.SAT.names]
    assert gc.GLO_FIX_CFG.itemsize == 48
    cfg = gc.glo_fix_cfg()
    got = {k: getattr(cfg, k) for k in S.DEFAULTS}
    assert got == S.DEFAULTS
    assert ctypes.sizeof(gc.GloEph) == 216 and ctypes.sizeof(gc.GloFixCfg) == 48
    for fn in ("ephemeris", "satpos", "fix"):
        assert hasattr(gc.lib(), f"gnsscorr_nav_glo_{fn}_dev") and hasattr(gc.lib(), f"gnsscorr_nav_glo_{fn}")


# ------------------------------------------------------------------ the world scene
def test_world_scene_shows_every_site_class():
    """every receiver solved at both measurements with every channel used, its solved
    latitude and longitude in its site's class; both sides of both meridians"""
    s = S.fix_scene("world")
    assert S.named_for_missed("world", s) == []
    n, Sx, Cx = S.literal_result("world")
    assert len(n) == len(S.G.SITES) == 11 and s["sizes"] == S.G.WORLD_SIZES
    assert (Sx["Z"] < 0).sum() >= 2 * 5 and (Sx["X"] < 0).any() and (Sx["Y"] > 0).any()


def test_world_tolerances_are_the_measured_spread_times_16():
    got = S.measure_spread(WORLD, ())
    print(got)
    for g, v in got.items():
        assert v <= S.SPREAD_WORLD[g] * 1.001, (g, v)          # the constants are what is measured
        assert v >= S.SPREAD_WORLD[g] * 0.5, (g, v)
        assert S.TOL_WORLD[g] == 16 * S.SPREAD_WORLD[g]


# mutant: (the outputs that must move, their tolerance group, which receivers: sign of Z or X)
GEO_MUTANTS = {"togeod_abs_z": (("el", "az"), "elaz", "Z"), "cart2geo_abs_z": (("lat",), "latlon", "Z"),
               "cart2geo_atan_y_over_x": (("lon",), "latlon", "X")}


@pytest.mark.parametrize("mutant", GEO_MUTANTS)
def test_geo_mutants_move_the_world_scene(mutant):
    """fabs(Z) in togeod and in cart2geo and atan(Y / X) for the longitude move the named
    outputs of every measurement of the receivers they concern, the southern ones and those
    with X < 0, by more than 100 tolerances (a satellite that falls below the mask counts as
    moved), and no output of any other receiver"""
    keys, group, axis = GEO_MUTANTS[mutant]
    s = S.fix_scene("world")
    n0, S0, C0 = S.literal_result("world")
    n1, S1, C1 = S.literal_result("world", mutant=mutant)
    assert not S0["status"].any()
    far = lambda x, y: np.nan_to_num(np.abs(x - y), nan=np.inf)
    if keys[0] in C0:
        per_ch = np.max([far(C1[k], C0[k]) for k in keys], axis=0)
        move = np.array([per_ch[a:b].max(axis=0) for a, b in zip(s["rx_first"], s["rx_first"][1:])])
    else:
        move = np.max([far(S1[k], S0[k]) for k in keys], axis=0)
    hit = S0[axis] < 0
    print(mutant, move[hit].min(), 100 * S.TOL_WORLD[group])
    assert hit.any() and (~hit).any()
    assert (move[hit] > 100 * S.TOL_WORLD[group]).all(), (mutant, move[hit].min())
    assert not move[~hit].any(), (mutant, move[~hit].max())


@pytest.mark.parametrize("mutant", GEO_MUTANTS)
@pytest.mark.parametrize("name", ALL)
def test_geo_mutants_leave_every_earlier_scene_as_it_was(name, mutant):
    """bit for bit: no scene of SCENES and not many_rx_scene reaches what they change"""
    a, b = S.literal_result(name), S.literal_result(name, mutant=mutant)
    assert a[0].tolist() == b[0].tolist()
    ra, rb = S.G.as_records(*a), S.G.as_records(*b)
    assert ra[0].tobytes() == rb[0].tobytes() and ra[1].tobytes() == rb[1].tobytes()
