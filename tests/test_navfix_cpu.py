"""CPU: the two restatements of the GPS L1 field decoding and position fix
(tests/navfix_scenarios.py) against each other and against what the generators planted, the
conditions that keep the scenes away from every decision threshold, and the tolerances of
tests/test_navfix_gpu.py: measured from the literal restatement alone, and shown to
discriminate."""
import numpy as np
import pytest

import navfix_scenarios as S

ALL = tuple(S.SCENES) + ("many",)
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


@pytest.mark.parametrize("name", ALL)
def test_fix_literal_equals_fast(name):
    s = _scene(name)
    n1, S1, C1 = S.literal_result(name)
    n2, S2, C2 = S.fix_fast(s["eph"], s["first"], s["abs_sample"], s["rx_first"], s["cfg"])
    a, b = S.as_records(n1, S1, C1), S.as_records(n2, S2, C2)
    assert np.array_equal(n1, n2)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("name", ALL)
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
