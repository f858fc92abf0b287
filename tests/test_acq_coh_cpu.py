"""The coherent-acquisition scenes (tests/acq_coh_scenes.py) set their trap: shown with
the fp64 oracle and numpy alone, no GPU.

These are conditions on the inputs of tests/test_acq_coh_engines_gpu.py, not on the
kernels.  In every scene the oracle finds the planted bin, code phase and block 1; the
N-point fold the kernels compute, restated in numpy, reproduces the oracle's signal row;
and each wrong restatement of that fold (S.folded_signal_row: carrier phase restarted
every period, coh ignored, block b read from b*N, a real record indexed as I, Q, record
r read from r*n_blocks*N) misses the oracle's signal row by more than 1e-2 relative in
`peak`, or decides another block or argmax.  1e-2 is a hundred times the loosest
tolerance of check_rows (fp32 peaks, 1e-4).

Observed margins (relative miss of the signal row's peak; "dec" = another block or
argmax), per scene; the columns are the five restatements in the order above:
  N      scene     coh  mode         restart  ignored  block   real/IQ  record
  4111   IQ        2    best         dec      0.747    0.373   -        -
  4111   IQ        2    noncoherent  dec      0.747    0.452   -        -
  4111   IQ        3    best         0.895    0.893    0.563   -        -
  4111   IQ        3    noncoherent  0.891    0.887    0.588   -        -
  4111   IQ        5    best         0.950    0.953    0.623   -        -
  4111   IQ        5    noncoherent  0.958    0.960    0.652   -        -
  4111   real IF   2    best         dec      0.733    0.398   dec      -
  4111   real IF   2    noncoherent  dec      0.747    0.428   dec      -
  5000   IQ        2    best         dec      0.757    0.440   -        -
  5000   IQ        2    noncoherent  dec      0.746    0.455   -        -
  5000   IQ        3    best         0.880    0.896    0.579   -        -
  5000   IQ        3    noncoherent  0.889    0.891    0.583   -        -
  5000   IQ        5    best         0.952    0.958    0.604   -        -
  5000   IQ        5    noncoherent  0.961    0.959    0.691   -        -
  5000   records   2    best         dec      0.752    0.430   -        dec
  5000   records   2    noncoherent  dec      0.751    0.457   -        dec
  5000   real IF   2    best         dec      0.754    0.405   dec      -
  5000   real IF   2    noncoherent  dec      0.750    0.452   dec      -
  16000  IQ        2    best         dec      0.746    0.408   -        -
  16000  IQ        2    noncoherent  dec      0.752    0.472   -        -
  16000  IQ        3    best         0.891    0.889    0.552   -        -
  16000  IQ        3    noncoherent  0.881    0.891    0.594   -        -
  16000  IQ        5    best         0.959    0.960    0.641   -        -
  16000  IQ        5    noncoherent  0.961    0.961    0.688   -        -
  16368  IQ        2    best         dec      0.741    0.411   -        -
  16368  IQ        2    noncoherent  dec      0.746    0.476   -        -
  16368  IQ        3    best         0.891    0.894    0.574   -        -
  16368  IQ        3    noncoherent  0.886    0.890    0.591   -        -
  16368  IQ        5    best         0.961    0.959    0.623   -        -
  16368  IQ        5    noncoherent  0.959    0.959    0.671   -        -
  16368  records   2    best         dec      0.754    0.440   -        dec
  16368  records   2    noncoherent  dec      0.758    0.463   -        dec
  16368  real IF   2    best         dec      0.749    0.425   dec      -
  16368  real IF   2    noncoherent  dec      0.748    0.425   dec      -
  38192  IQ        2    best         dec      0.756    0.444   -        -
  38192  IQ        2    noncoherent  dec      0.751    0.471   -        -
"""
import numpy as np
import pytest

import acq_coh_scenes as S

# one scene per (length, coh, mode): the engines of one length search the same records
LENGTHS = ["f64-16368", "f64-16000", "mixed-5000", "bluestein-4111", "m4-38192"]
IQ_SCENES = [pytest.param(S.scene(e, coh, mode), mode == "noncoherent", id=f"{e}-coh{coh}-{mode}")
             for e in LENGTHS for coh, mode in S.search_cases(e)]
REAL_SCENES = [pytest.param(S.scene(e, 2, mode, iq=False), mode == "noncoherent",
                            id=f"{e}-real-{mode}")
               for e in S.REAL_IF_ENGINES if e in LENGTHS for mode in S.MODES]
RECORD_SCENES = [pytest.param(S.scene(e, 2, mode, records=S.N_RECORDS), mode == "noncoherent",
                              id=f"{e}-records-{mode}")
                 for e in S.RECORD_ENGINES for mode in S.MODES]
TRAP = 1e-2
CLEAR = 1e-9


def test_every_engine_searches_a_checked_length():
    shown = {(S.ENGINES[e]["fs"], S.ENGINES[e]["n"], S.ENGINES[e]["if0"]) for e in LENGTHS}
    for e in S.ENGINES.values():
        assert (e["fs"], e["n"], e["if0"]) in shown
        assert e["if0"] % 1000.0 == 0.0 and e["if0"] + 3000.0 < e["fs"] / 2


def _records(sc):
    return range(len(sc.phases))


@pytest.mark.parametrize("sc,nc", IQ_SCENES + REAL_SCENES + RECORD_SCENES)
def test_signal_row_is_as_planted(sc, nc):
    f = S.freqs(sc)
    frac = (f[S.SIG_BIN] / 1000.0) % 1.0
    assert frac == (0.5 if sc.coh == 2 else 0.25)
    assert f[5] - f[S.SIG_BIN] == sc.fs / sc.n and f[6] - f[S.SIG_BIN] == 2 * sc.fs / sc.n
    assert len(set(sc.phases)) == len(sc.phases)
    for r in _records(sc):
        ref, ref_rows = S.reference(sc, nc, r)
        g = ref[S.SIG_GROUP]
        assert g["bin"] == S.SIG_BIN and g["code_phase"] == sc.phases[r] + 1
        row = ref_rows[S.SIG_GROUP][S.SIG_BIN]
        assert row["argmax"] == sc.phases[r] and row["block"] == (-1 if nc else 1)
        assert g["metric"] > 2.5 and g["metric"] > ref[1 - S.SIG_GROUP]["metric"]


@pytest.mark.parametrize("sc,nc", IQ_SCENES + REAL_SCENES + RECORD_SCENES)
def test_fold_restates_the_oracle(sc, nc):
    """The kernels' N-point fold, in numpy, gives the oracle's coh*N-point signal row."""
    for r in _records(sc):
        ref_row = S.reference(sc, nc, r)[1][S.SIG_GROUP][S.SIG_BIN]
        assert S.miss(S.folded_signal_row(sc, nc, None, r), ref_row) < 1e-10


@pytest.mark.parametrize("sc,nc", IQ_SCENES + REAL_SCENES + RECORD_SCENES)
def test_wrong_restatements_miss_the_reference(sc, nc):
    # record 0 of a records scene starts at sample 0 under either record stride
    rec = 1 if len(sc.phases) > 1 else 0
    ref_row = S.reference(sc, nc, rec)[1][S.SIG_GROUP][S.SIG_BIN]
    for m in S.mistakes(sc):
        d = S.miss(S.folded_signal_row(sc, nc, m, rec), ref_row)
        print(f"[coh trap n={sc.n} coh={sc.coh} iq={int(sc.iq)} records={len(sc.phases)} "
              f"{'noncoherent' if nc else 'best'}] {m}: {d:.3f}")
        assert d > TRAP, (m, d)


@pytest.mark.parametrize("sc,nc", IQ_SCENES + REAL_SCENES + RECORD_SCENES)
def test_clear_winners(sc, nc):
    """check_rows demands argmax exact in fp64: no row of any scene has a tie that the
    observed ~1e-13 error could turn.  Every row's peak stands more than 1e-9 relative
    above its second peak, and above every other sample of the row."""
    for r in _records(sc):
        ref, ref_rows = S.reference(sc, nc, r)
        for rr in ref_rows:
            for row in rr:
                assert row["peak"] - row["second"] > CLEAR * row["peak"]
        for g in ref:
            assert g["peak"] - g["second"] > CLEAR * g["peak"]
        # the whole rows, from the literal correlation: no second sample within 1e-9 of
        # the maximum, and no two block maxima that close (the block choice is exact too)
        for code in (0, 1):
            for f in S.freqs(sc):
                rows = [S.literal_row(sc, f, code, b, r) for b in range(sc.n_blocks)]
                if nc:
                    rows = [np.sum(rows, axis=0)]
                for row in rows:
                    top = np.sort(row)[-2:]
                    assert top[1] - top[0] > CLEAR * top[1]
                mx = np.sort([row.max() for row in rows])
                assert (np.diff(mx) > CLEAR * mx[-1]).all()
