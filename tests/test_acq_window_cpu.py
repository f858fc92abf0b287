"""The second-peak window scenes (tests/acq_window_scenes.py) set their trap: shown
with the fp64 oracle alone, no GPU.

These are conditions on the inputs of tests/test_acq_window_gpu.py, not on the
kernels: in every row of every case the peak is on sample p; with spc = d the copies
d samples to either side sit on the open window's edges and `second` is the stronger
one (0.25 of the peak); with spc = d + 1 they are inside and `second` falls to the
correlation floor (the non-coherent sum keeps block 0's amplitude-1 copy, 0.03).  So a
kernel that includes or excludes a copy wrongly misses `second` by 0.1 of the peak or
more, far outside any tolerance of check_rows.
"""
import numpy as np
import pytest

import acq_window_scenes as W

# fp32 and fp64 at 16368 search the same scenes: one oracle run serves both (the
# four-step engine shares their d = 16 references and adds its own distances)
ENGINES = [e for e in W.ENGINES if e != "f32-16368"]


def _check(rows, p, edge):
    for r in rows:
        assert r["argmax"] == p
        ratio = r["second"] / r["peak"]
        if edge:
            assert ratio > 0.2, ratio
        else:
            assert ratio < 0.05, ratio


@pytest.mark.parametrize("noncoherent", [False, True], ids=["best", "noncoherent"])
@pytest.mark.parametrize("engine", ENGINES)
def test_window_scenes_set_the_trap(engine, noncoherent):
    e = W.ENGINES[engine]
    assert W.ENGINES["f32-16368"] == W.ENGINES["f64-16368"]
    for p, d, spc, mirror in W.cases(engine):
        ref, ref_rows = W.reference(e["fs"], e["n"], p, d, spc, mirror, noncoherent)
        _check(ref_rows[0], p, spc == d)
        assert ref[0]["bin"] == 1 and ref[0]["code_phase"] == p + 1
        assert all(r["block"] == (-1 if noncoherent else 1) for r in ref_rows[0])
        # the mirror variant gives the same figures from the other edge
        m, m_rows = W.reference(e["fs"], e["n"], p, d, spc, not mirror, noncoherent)
        if spc == d:
            assert abs(m[0]["second"] / m[0]["peak"] - ref[0]["second"] / ref[0]["peak"]) < 0.02


def test_edge_distances_straddle_the_engines_thresholds():
    """The d of every engine is the widest spc its one-pass statistics answer exactly
    (2 spc - 1 samples against the distance between one thread's samples), so spc = d
    and spc = d + 1 run the engine's two branches."""
    for engine, spacing in (("f64-16368", 528), ("f32-16368", 528), ("f64-16000", 400)):
        d = W.ENGINES[engine]["ds"][0]
        assert 2 * d - 1 <= spacing < 2 * (d + 1) - 1
    for engine in ("mixed-5000", "bluestein-4111"):
        e = W.ENGINES[engine]
        assert W.stats1_exact(e["n"], e["ds"][0]) and not W.stats1_exact(e["n"], e["ds"][0] + 1)
    # the four-step plan: the fused column top-2 up to 2 spc - 1 <= N1, then the generic
    # statistics' one pass up to its own threshold, then their two passes
    m4 = W.ENGINES["m4-16368"]
    fused_d, one_pass_d = m4["ds"][:2]
    assert 2 * fused_d - 1 <= m4["n1"] < 2 * (fused_d + 1) - 1
    assert W.stats1_exact(m4["n"], fused_d + 1)
    assert W.stats1_exact(m4["n"], one_pass_d) and not W.stats1_exact(m4["n"], one_pass_d + 1)
    for e in W.ENGINES.values():
        assert 16 in e["ds"] and max(e["ds"]) + 1 <= e["n"] // 2


def test_padded_scenes_set_the_trap():
    for p, dist, mirror in W.padded_cases():
        ref, ref_rows = W.padded_reference(p, dist, mirror)
        _check(ref_rows[0], p, dist == W.PAD_SPC)
        assert ref[0]["bin"] == 1 and ref[0]["code_phase"] == p + 1


@pytest.mark.parametrize("n_blocks", [2, 3])
def test_tied_blocks_report_the_last_block(n_blocks):
    """Bit-identical blocks: a later block replaces the kept one unless the kept
    maximum is strictly larger (acquisition.sci:126-132), so the last block stands."""
    for e in (W.ENGINES["f64-16368"], W.ENGINES["f64-16000"]):
        blocks = W.tied_if(e["n"], n_blocks).reshape(n_blocks, -1)
        assert all(np.array_equal(blocks[0], b) for b in blocks[1:])
        ref, ref_rows = W.tied_reference(e["fs"], e["n"], n_blocks)
        assert all(r["block"] == n_blocks - 1 for r in ref_rows[0])


def test_repeated_frequency_reports_the_first_bin():
    for e in (W.ENGINES["f64-16368"], W.ENGINES["f64-16000"]):
        ref, ref_rows = W.tied_reference(e["fs"], e["n"], 2, group_freq=((1, 1, 0),))
        assert ref_rows[0][0] == ref_rows[0][1]
        assert ref[0]["bin"] == 0 and ref[0]["carr_freq"] == 0.0
