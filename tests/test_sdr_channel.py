"""CPU: the GPS-SDR Channel fixtures and host code.

The oracle for this row is the reference Channel class itself, compiled from
objects/channel.cpp (oracle/_ref/libsdr_chan_ref.so, oracle/sdr_chan_ref.cpp);
tests/golden/sdr_channel.npz holds its outputs on the synthetic navigation
streams of tests/sdr_nav_scenarios.py (make_sdr_chan_golden.py).
Checked here: the ICD-200 parity encoder against the reference ParityCheck,
the product's host Channel::Start against the reference object byte for byte,
the scenario inputs against their pinned SHA-256, and the fixture against the
reference build.
"""
import hashlib
import os

import numpy as np
import pytest

import sdr_nav_scenarios as N
import sdr_oracle as S

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
need_ref = pytest.mark.skipif(not S.have_ref_chan(), reason="reference build (oracle/_ref) absent")


def _golden():
    return np.load(os.path.join(GOLD, "sdr_channel.npz"))


def test_parity_encoder_roundtrip():
    rng = np.random.default_rng(4)
    prev = 0
    for _ in range(500):
        w = N.encode_word(int(rng.integers(0, 1 << 24)), prev)
        u = w | (prev & 3) << 30                 # bits 31-30: D29*, D30* (BitStuff layout)
        if u & 0x40000000:
            u ^= 0x3FFFFFC0
        assert N.parity_ok(u)
        assert not N.parity_ok(u ^ (1 << int(rng.integers(6, 30))))   # any single data-bit error
        prev = w


@need_ref
def test_parity_against_reference():
    ref = S.RefSdrChannel(0)
    rng = np.random.default_rng(5)
    for _ in range(300):
        w = int(rng.integers(0, 1 << 32, dtype=np.uint64))
        assert ref.parity(w) == N.parity_ok(w)


def test_scenario_inputs_pinned():
    import make_sdr_chan_golden as G
    g = _golden()
    for k, sc in enumerate(N.SCENARIOS):
        corr = G.scenario_corr(sc, int(g["n_ms"]))
        assert hashlib.sha256(corr.tobytes()).hexdigest() == str(g["corr_sha256"][k])


def _branch_golden():
    return np.load(os.path.join(GOLD, "sdr_channel_branches.npz"))


def test_branch_inputs_pinned():
    g = _branch_golden()
    assert list(g["names"]) == [sc["name"] for sc in N.BRANCH_SCENARIOS]
    for k, sc in enumerate(N.BRANCH_SCENARIOS):
        corr = N.branch_corr(sc)
        assert corr.shape == (int(g["n_ms"]), 6)
        assert hashlib.sha256(corr.tobytes()).hexdigest() == str(g["corr_sha256"][k]), sc["name"]


def test_sched_generator_equals_plain():
    """One segment, upright, no slip: correlations_sched is correlations."""
    bits = N.nav_bits(2, seed=9)
    a = N.correlations(3000, bits, 13, 2600.0, 1300.0, seed=3, q_bias=-0.05)
    b = N.correlations_sched(3000, bits, 13, [(0, 2600.0, 1300.0)], seed=3, q_bias=-0.05)
    assert a.tobytes() == b.tobytes()


def test_branch_golden_reaches_branches():
    """The committed arrays themselves show each stream's defining event."""
    import make_sdr_chan_branches_golden as B
    g = _branch_golden()
    rows, words = g["sub_rows"], g["sub_words"]
    subs = [[(int(r[1]), int(r[3]), w) for r, w in zip(rows, words) if r[0] == k]
            for k in range(len(N.BRANCH_SCENARIOS))]
    e = int(g["nco_every"])
    lens = g["snap_state"].view(S.RefSdrChannel.STATE)["len"].reshape(-1)
    for k, sc in enumerate(N.BRANCH_SCENARIOS):
        flags = g["flags"][k]
        nco = np.repeat(g["nco"][k][:, 0], e)[:len(flags)]   # held between the stored calls
        B.reach(sc["name"], flags, nco, subs[k], twin=(g["flags"][0], subs[0]), lens=lens)


@need_ref
def test_branch_golden_matches_reference_build():
    """Re-run the reference on every branch stream: reach, decidability, and the
    fixture's flags, final state and subframes."""
    import make_sdr_chan_branches_golden as B
    g = _branch_golden()
    twin = None
    for k, sc in enumerate(N.BRANCH_SCENARIOS):
        corr, fb, subs, st, tr = B.run_reference(k, sc)
        flags, snaps, _ = B.check_run(sc, fb, subs, tr, twin)
        if sc["name"] == "upright":
            twin = (flags, subs)
        assert (flags == g["flags"][k]).all(), sc["name"]
        assert st.tobytes() == g["state"][k].tobytes(), sc["name"]
        rows = g["sub_rows"][g["sub_rows"][:, 0] == k]
        assert [m for m, _, _ in subs] == list(rows[:, 1])
        assert [s for _, s, _ in subs] == list(rows[:, 3])
        if sc["name"] == "cn0":
            assert list(snaps) == list(g["snap_calls"])
            assert tr[snaps].tobytes() == g["snap_state"].tobytes()


@need_ref
def test_host_start_matches_reference(gc):
    ref = S.RefSdrChannel(3)
    for sv, dop, cl, *_ in N.SCENARIOS + [(31, -14999, 20, 0, 0, 0, 0, 0)]:
        ref.start(sv, dop, cl)
        mine = gc.SdrCorrCtx.channel_start(3, sv, dop, cl)
        assert mine.tobytes()[:580] == ref.state().tobytes()[:580]


@need_ref
def test_golden_matches_reference_build():
    import make_sdr_chan_golden as G
    g = _golden()
    k = 0
    sc = N.SCENARIOS[k]
    corr = G.scenario_corr(sc, int(g["n_ms"]))
    ref = S.RefSdrChannel(k)
    ref.start(int(sc[0]), int(sc[1]), int(sc[2]))
    fb, subs, st = ref.run(corr)
    assert (G.flags_of(fb) == g["flags"][k]).all()
    assert st.tobytes() == g["state"][k].tobytes()
    rows = g["sub_rows"][g["sub_rows"][:, 0] == k]
    assert [m for m, _ in subs] == list(rows[:, 1])
