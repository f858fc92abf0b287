"""CPU: the two restatements of the GPS L1 field decoding and position fix
(tests/navfix_scenarios.py) against each other and against what the generators planted, the
conditions that keep the scenes away from every decision threshold, and the tolerances of
tests/test_navfix_gpu.py: measured from the literal restatement alone, and shown to
discriminate."""
import numpy as np
import pytest

import navfix_scenarios as S

ALL = tuple(S.SCENES) + ("many",)
WORLD = tuple(S.WORLD_SCENES)
MULTI = tuple(k for k, (_, multi) in S.SCENES.items() if multi)


def _scene(name):
    return S.many_rx_scene() if name == "many" else S.fix_scene(name)


@pytest.mark.parametrize("n_ch", [1, 3, 65])
def test_field_decode_literal_equals_fast_and_what_was_planted(n_ch):
    bits, n_bits, first, raws = S.eph_scene(n_ch)
    lit = S.eph_literal(bits, n_bits, first)
    assert lit.tobytes() == S.eph_fast(bits, n_bits, first).tobytes()
    for ch in range(n_ch):
        ids = S.ORDERS[ch % len(S.ORDERS)]
        if lit["status"][ch] != S.EPH_OK:
            assert lit["have"][ch] == 0 and not any(lit[k][ch] for k in S.EPH_FIELDS)
            continue
        want = S.raw_to_values(raws[ch])
        assert lit["have"][ch] == sum(1 << (i - 1) for i in (1, 2, 3) if i in ids)
        for k, (sf, *_) in S.FIELDS.items():
            assert lit[k][ch] == (want[k] if sf in ids else 0), (ch, k)
    if n_ch == 65:
        assert lit["status"][[1, 8, 9]].tolist() == [S.EPH_SHORT] * 3
        assert lit["status"][[10, 11, 12]].tolist() == [S.EPH_UNDECIDED] * 3
        neg = [k for k in S.SIGNED if (lit[k] < 0).any()]
        assert set(neg) == set(S.SIGNED)                       # every signed field went negative


@pytest.mark.parametrize("name", ALL + WORLD)
def test_fix_literal_equals_fast(name):
    s = _scene(name)
    n1, S1, C1 = S.literal_result(name)
    n2, S2, C2 = S.fix_fast(s["eph"], s["first"], s["abs_sample"], s["rx_first"], s["cfg"])
    a, b = S.as_records(n1, S1, C1), S.as_records(n2, S2, C2)
    assert np.array_equal(n1, n2)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("name", ALL + WORLD)
def test_scene_conditions(name):
    """cond(A) < 1e6 and GDOP < 6 where a receiver is full rank; no elevation within 1e-6
    degrees of the mask; no Kepler step and no togeod exit within a factor 4 of its threshold"""
    s = _scene(name)
    d = S.scene_diagnostics(s)
    assert S.conditions_hold(s, full_rank=True), {k: (v.min(), v.max()) for k, v in d.items()
                                                   if len(v)}
    assert len(d["dE"]) and len(d["togeod_all"])


def test_scenes_show_what_they_are_named_for():
    n, Sx, Cx = S.literal_result("drop_one")
    assert Sx["n_used"][0].tolist() == [7, 6, 6] and Cx["used"][6].tolist() == [1, 0, 0]
    assert np.isnan(Cx["el"][6, 1:]).all() and np.isinf(Cx["rawP"][6, 1:]).all()
    n, Sx, Cx = S.literal_result("five_to_three")
    assert Sx["status"][0].tolist() == [S.FIX_OK, S.FIX_FEW, S.FIX_FEW]
    assert np.isnan(Sx["X"][0, 1:]).all() and not Sx["DOP"][0, 1:].any()
    n, Sx, Cx = S.literal_result("few_ready")
    assert n.tolist() == [0, 2] and not Sx["written"][0].any()
    s = S.fix_scene("seed_from_excluded")
    n, Sx, Cx = S.literal_result("seed_from_excluded")
    assert s["eph"]["have"][5] == 5 and Cx["used"][5].tolist() == [0, 0]
    assert Sx["status"][0].tolist() == [S.FIX_OK] * 2
    n, Sx, Cx = S.literal_result("rank")
    assert Sx["status"].tolist() == [[S.FIX_RANK] * 2, [S.FIX_OK] * 2]
    assert not Sx["X"][0].any() and np.isnan(Cx["el"][:5]).all()
    n, Sx, Cx = S.literal_result("max_meas_below")
    assert n.tolist() == [2]                                   # 300 epochs hold 12 periods of 20


def test_planted_position_is_recovered_without_troposphere():
    """largest distance over the scene: 1.1e-3 m (seven iterations with rows divided by obs
    instead of the range end a few tenths of a millimetre short); the bound is 1 m"""
    s = S.fix_scene("notrop")
    n, Sx, Cx = S.literal_result("notrop")
    worst = 0.0
    for rx in range(2):
        for m in range(n[rx]):
            p = np.array([Sx["X"][rx, m], Sx["Y"][rx, m], Sx["Z"][rx, m]])
            worst = max(worst, float(np.linalg.norm(p - s["planted"][rx])))
    print("planted position recovered to", worst, "m")
    assert worst < 1.0


def test_tolerances_are_the_measured_spread_times_16():
    got = S.measure_spread()
    print(got)
    for g, v in got.items():
        assert v <= S.SPREAD[g] * 1.001, (g, v)                # the constants are what is measured
        assert v >= S.SPREAD[g] * 0.5, (g, v)
        assert S.TOL[g] == 16 * S.SPREAD[g]


def _xyz_move(name, mutant, n_iter=7, keys=("X", "Y", "Z")):
    s = S.fix_scene(name)
    n, Sm, Cm = S.fix_literal(s["eph"], s["first"], s["abs_sample"], s["rx_first"], s["cfg"],
                              mutant=mutant, n_iter=n_iter)
    n0, S0, C0 = S.fix_literal(s["eph"], s["first"], s["abs_sample"], s["rx_first"], s["cfg"],
                               n_iter=n_iter)
    ok = S0["written"] & (S0["status"] == S.FIX_OK)
    return np.max([np.abs(Sm[k][ok] - S0[k][ok]) for k in keys], axis=0)


@pytest.mark.parametrize("mutant", ["no_erot", "no_trop", "no_dtr", "no_tgd"])
def test_tolerances_discriminate(mutant):
    """every mutant of the literal restatement moves X Y Z of every solved measurement of
    every multi-measurement scene by more than 100 tolerances"""
    for name in MULTI:
        if mutant == "no_trop" and S.fix_scene(name)["cfg"]["useTropCorr"] != 1:
            continue                                           # off only where it should be on
        move = _xyz_move(name, mutant)
        print(mutant, name, move.min())
        assert (move > 100 * S.TOL["xyz"]).all(), (mutant, name, move.min())


def test_first_iteration_troposphere_constant_discriminates():
    """trop = 0 instead of 2 in the first iteration, after one iteration on a one-measurement
    scene.  The constant is common to every row and the fourth column of A is all ones, so it
    moves dt by 2 m and X Y Z by rounding only: the 100 tolerances are asked of dt."""
    move = _xyz_move("one_meas", "trop0_first", n_iter=1, keys=("dt",))
    print(move)
    assert (move > 100 * S.TOL["dt"]).all()
    assert abs(move[0] - 2.0) < 1e-6


# ------------------------------------------------------------------ the scenes of WORLD_SCENES
@pytest.mark.parametrize("name", WORLD)
def test_world_scenes_show_what_they_are_named_for(name):
    """every receiver solved at every measurement; world: each receiver's solved latitude and
    longitude in its site's class; week_end / week_start: check_t moved every used channel's
    time - t_oe by a week, down / up, and nowhere else; eccentric: every Kepler loop ran its 10
    steps and left by the cap with |dE| > 4e-12; inclined: i_0 below 0.6 and above 1.2 rad"""
    s = S.fix_scene(name)
    assert S.named_for_missed(name, s) == []
    d = S.scene_diagnostics(s)
    n_calls = int(s["rx_first"][-1]) * s["cfg"]["max_meas"]
    assert len(d["tk"]) == len(d["kepler"]) == n_calls
    if name == "world":
        n, Sx, Cx = S.literal_result(name)
        assert len(n) == len(S.SITES) == 11 and s["sizes"] == S.WORLD_SIZES
        assert (Sx["Z"] < 0).sum() >= 2 * 5 and (Sx["X"] < 0).any() and (Sx["Y"] > 0).any()
        for k in ("meridian_180", "meridian_0"):               # both sides of both meridians
            i = list(S.SITES).index(k + "_east")
            assert Sx["lon"][i, 0] * Sx["lon"][i - 1 if k == "meridian_0" else i + 1, 0] < 0
    if name.startswith("week"):
        tow = int(s["eph"]["TOW"][0])
        assert (tow > S.WEEK - 900 and tow + 1 < S.WEEK) if name == "week_end" else 0 < tow < 900
        assert (s["eph"]["t_oe"] == (0 if name == "week_end" else 597600)).all()
        assert (s["eph"]["t_oc"] == s["eph"]["t_oe"]).all()
        assert (np.abs(d["tk"][:, 1] - d["tk"][:, 0]) == S.WEEK).all()
    if name == "eccentric":
        assert d["kepler"][:, 0].sum() == 10 * n_calls and (d["kepler"][:, 1] > 4e-12).all()
        assert (s["eph"]["e"] >= 0.1).all() and (s["eph"]["e"] <= 0.3).all()


def test_planted_position_is_recovered_at_the_week_edges():
    """troposphere off in both.  Seven iterations with rows divided by obs stop a geometry's
    own distance short (printed: 2.5e-2 m at the end, 1.1e-3 m at the start), so the check runs
    the same restatement to 14 iterations, where only the planting's rounding is left: 8e-6 m.
    The bound is 1e-4 m, ten times the 1e-5 m a float64 probe of the scene's kind recovered; a
    week lost in tk moves the satellites by thousands of kilometres."""
    for name in ("week_end", "week_start"):
        s = S.fix_scene(name)
        for n_iter in (7, 14):
            n, Sx, Cx = S.fix_literal(s["eph"], s["first"], s["abs_sample"], s["rx_first"],
                                      s["cfg"], n_iter=n_iter)
            err = [float(np.linalg.norm(np.array([Sx[k][0, m] for k in "XYZ"]) - s["planted"][0]))
                   for m in range(n[0])]
            print(name, n_iter, "iterations: planted position recovered to", err, "m")
        assert len(err) == 2 and max(err) < 1e-4


def test_world_tolerances_are_the_measured_spread_times_16():
    got = S.measure_spread(WORLD)
    print(got)
    for g, v in got.items():
        assert v <= S.SPREAD_WORLD[g] * 1.001, (g, v)          # the constants are what is measured
        assert v >= S.SPREAD_WORLD[g] * 0.5, (g, v)
        assert S.TOL_WORLD[g] == 16 * S.SPREAD_WORLD[g]


def _world_move(name, mutant, keys):
    """|mutant - restatement| per receiver and measurement [n_rx, max_meas], the largest over
    keys (sol) or over keys and the receiver's channels (chan); infinite where the mutant has no
    value (fabs(Z) in togeod turns the southern sky over: satellites fall below the mask)"""
    s = S.fix_scene(name)
    n0, S0, C0 = S.literal_result(name)
    n1, S1, C1 = S.literal_result(name, mutant=mutant)
    assert not S0["status"].any()
    far = lambda x, y: np.nan_to_num(np.abs(x - y), nan=np.inf)   # a value gone: moved
    if keys[0] in C0:
        per_ch = np.max([far(C1[k], C0[k]) for k in keys], axis=0)
        return np.array([per_ch[a:b].max(axis=0) for a, b in zip(s["rx_first"], s["rx_first"][1:])])
    return np.max([far(S1[k], S0[k]) for k in keys], axis=0)


# mutant: (its scenes, the outputs that must move, their tolerance group)
WORLD_MUTANTS = {
    "check_t_identity": (("week_end", "week_start"), ("X", "Y", "Z"), "xyz"),
    "kepler_20": (("eccentric",), ("X", "Y", "Z"), "xyz"),
    "togeod_abs_z": (("world",), ("el", "az"), "elaz"),
    "cart2geo_abs_z": (("world",), ("lat",), "latlon"),
    "cart2geo_atan_y_over_x": (("world",), ("lon",), "latlon"),
}


@pytest.mark.parametrize("mutant", WORLD_MUTANTS)
def test_world_mutants_move_the_scene_named_for_them(mutant):
    """each mistake that only the new scenes reach moves the named outputs of every solved
    measurement by more than 100 tolerances; in the world scene of the receivers it concerns,
    the southern ones for fabs(Z) and those with X < 0 for atan(Y / X), and of no other"""
    scenes, keys, group = WORLD_MUTANTS[mutant]
    for name in scenes:
        move = _world_move(name, mutant, keys)
        print(mutant, name, move.min(), move.max(), 100 * S.TOL_WORLD[group])
        if name != "world":
            assert (move > 100 * S.TOL_WORLD[group]).all(), (mutant, name, move.min())
            continue
        n, Sx, Cx = S.literal_result(name)
        hit = (Sx["X"] < 0) if mutant == "cart2geo_atan_y_over_x" else (Sx["Z"] < 0)
        assert hit.any() and (~hit).any()
        assert (move[hit] > 100 * S.TOL_WORLD[group]).all(), (mutant, move[hit].min())
        assert not move[~hit].any(), (mutant, move[~hit].max())


@pytest.mark.parametrize("mutant", WORLD_MUTANTS)
@pytest.mark.parametrize("name", ALL)
def test_world_mutants_leave_every_earlier_scene_as_it_was(name, mutant):
    """bit for bit: what these mutants change, no scene of SCENES and not many_rx_scene reaches"""
    a = S.as_records(*S.literal_result(name))
    b = S.as_records(*S.literal_result(name, mutant=mutant))
    assert S.literal_result(name)[0].tolist() == S.literal_result(name, mutant=mutant)[0].tolist()
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
