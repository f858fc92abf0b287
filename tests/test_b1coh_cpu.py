"""CPU: the restatement of COMPASS/B1/acquisition_7x3ms.sci and acquisition_4x5ms.sci
(tests/b1coh_scenarios.py) and the small planted scenes of tests/test_b1coh_gpu.py.

These tests exercise the numpy restatement, the scenes and the library's host-side
second-peak predicate, which the parent commit has too: they pass with or without
GNSSCORR_ACQ_CONCAT and gnsscorr_acq_set_block_stride.  The tests that fail without the
feature are the GPU ones.
"""
import numpy as np
import pytest

import b1coh_scenarios as C
import b1i_scenarios as B

# What b1coh_scenarios.acquire printed on b1i_scenarios.scene() (seed 22, 50 dB-Hz, 43 ms)
# over an 8 kHz band: (prn, bin, codePhase, segment, peakMetric, straddles).  Code phases
# reduce mod 16000 to the planted starts plus one sample (makeCaTable.sci:62 samples the
# replica one sample late), PRN 11 at 5 ms plus two.
TABLE = {
    3: [(6, 30, 249931, 5, 26.193739663268016, True),
        (11, 9, 24589, 0, 23.5831701643475, False),
        (23, 15, 158477, 3, 22.66428728544706, True),
        (37, 39, 200329, 4, 35.11640475222386, True)],
    5: [(6, 50, 249931, 3, 49.62530877400352, True),
        (11, 15, 312590, 3, 46.2151717750732, False),
        (23, 25, 126477, 1, 40.44899575955265, False),
        (37, 65, 200329, 2, 50.68219962138471, False)],
}


@pytest.mark.parametrize("mode", [3, 5])
def test_restatement_finds_the_scene(mode):
    """Bins, code phases and segments exact, metrics to 1e-9 of the recorded values, every
    decision margin >= 1e-4 (the smallest is 1.3e-3), at least one second-peak range that
    straddles a segment boundary per mode.  Passes on the parent: numpy only."""
    IF, chans = B.scene()
    s = B.settings()
    prns = [c[0] for c in chans]
    frq = C.bins(s, C.MODES[mode]["coh"], 8.0)
    assert len(frq) == {3: 49, 5: 81}[mode]
    got = C.acquire(IF, s, prns, mode, band_khz=8.0)
    for c, a, (prn, b, cp, seg, metric, strad) in zip(chans, got, TABLE[mode]):
        assert c[0] == prn
        assert (a["bin"], a["code_phase"], a["segment"]) == (b, cp, seg), prn
        assert abs(a["metric"] - metric) <= 1e-9 * metric, (prn, a["metric"])
        assert a["straddles"] == strad, prn
        assert min(a["margins"]) >= 1e-4, (prn, a["margins"])
        assert a["carr_freq"] == frq[b]
        assert (cp - c[1]) % 16000 in (1, 2) and abs(a["carr_freq"] - (s["IF"] + c[2])) < 100
    assert any(a["straddles"] for a in got)


def test_concatenated_row_is_the_linear_correlation():
    """At the small shape index q of the restatement's row is |sum_n x[q + n] r[n]|^2, the
    time-domain linear correlation of the record with the replica (at zero frequency), to
    1e-10 of the peak, across every segment boundary.  Passes on the parent: numpy only."""
    a, s, edge = C.M + C.S - 7, 7, "lo"
    IF = C.scene_if(a, s, edge)
    ref, _ = C.search(IF, C.FS, C.code()[None, :], C.L, C.NB, C.FREQS, C.GF, spc=s, period=C.S)
    row = ref[0]["results"][1]
    x = IF[0::2].astype(np.float64)
    r = C.code().astype(np.float64)
    brute = np.array([np.dot(x[q:q + C.M], r) for q in range(C.NB * C.M)]) ** 2
    assert row.shape == brute.shape == (4200,)
    assert np.abs(row - brute).max() <= 1e-10 * brute.max()
    assert int(np.argmax(brute)) == a   # the weaker copies' sidelobes add to (6 M)^2 there


def test_code_phase_range_is_the_library_predicate(gc):
    """The 1-based codePhaseRange of :159-176 equals gnsscorr_acq_second_peak_candidate(k, a,
    s, n_blocks * keep, S) for every k of the concatenated row, at every peak of the small
    shape's case list.  Passes on the parent: the predicate is the L3 rule's."""
    lib = gc.lib()
    n = C.NB * C.M
    for a, s, _ in C.cases():
        want = np.zeros(n, bool)
        want[C.code_phase_range_1b(a + 1, C.S, s) - 1] = True
        got = np.array([lib.gnsscorr_acq_second_peak_candidate(k, a, s, n, C.S) for k in range(n)])
        assert set(got) <= {0, 1}
        assert np.array_equal(got.astype(bool), want), (a, s)
        assert 0 < want.sum() <= C.S + 1


def test_planted_scenes_are_decidable():
    """Under both rules every row's peak, every row's second peak and the winning bin of
    every planted scene are clear of their runners-up by more than 1e-6 relative; the peak
    is where it was planted, and the two rules answer differently (the decoy, planted at
    1/4 of the peak's power, for the circular window; the edge copy, at 1/9, for the
    period rule).  Passes on the parent: numpy only."""
    for a, s, edge in C.cases():
        on, on_rows = C.reference(a, s, edge, C.S)
        off, off_rows = C.reference(a, s, edge, 0)
        C.assert_decidable(on, on_rows, s, C.S)
        C.assert_decidable(off, off_rows, s, 0)
        assert on[0]["bin"] == 1 and on[0]["code_phase"] == a + 1
        assert on_rows[0][1]["argmax"] == a and on_rows[0][1]["block"] == a // C.M
        # (the copies' sidelobes, some 25 per unit amplitude, move both a little)
        assert on[0]["second"] == on[0]["results"][1][C.edge_lag(a, s, edge)]
        assert off[0]["second"] == off[0]["results"][1][C.decoy_lag(a)]
        assert off[0]["second"] > 1.2 * on[0]["second"], (a, s)


def test_chunk_scene_is_decidable_and_spreads_over_blocks():
    """The chunk-boundary scene of the GPU tier: decidable, and its five groups win in
    three different blocks.  Passes on the parent: numpy only."""
    ref, rows = C.search(C.chunk_if(), C.FS, C.code()[None, :], C.L, C.NB, C.CH_FREQS, C.CH_GF,
                         group_code=np.zeros(5, int), spc=7, period=C.S)
    for g, rg in enumerate(ref):   # groups name one frequency twice: rows, not bins, decide
        for b, rr in enumerate(rows[g]):
            row = rg["results"][b]
            assert rr["peak"] > np.delete(row, rr["argmax"]).max() * (1 + 1e-6)
            v = np.sort(row[C.second_candidates(len(row), rr["argmax"], 7, C.S)])
            assert v[-1] > v[-2] * (1 + 1e-6)
    blocks = [rows[g][ref[g]["bin"]]["block"] for g in range(5)]
    assert blocks == [1, 4, 6, 1, 4]
