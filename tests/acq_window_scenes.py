"""Second-peak window scenes: deterministic, noise-free inputs with sharp peaks.

TEST INFRASTRUCTURE ONLY (no GPU).  Every acquisition engine reports, per row,
`second` = the maximum outside the open circular window (argmax - spc, argmax + spc)
(acquisition.sci:147-166, oracle/acq_oracle.py _second_peak), and the acceptance
metric is peak / second.  These scenes put a correlation peak on a chosen sample p
and two weaker copies exactly d samples to either side of it, so that

  spc = d      both copies sit on the open window's edges and count: `second` is the
               stronger copy, (3/6)^2 = 0.25 of the peak;
  spc = d + 1  both copies are inside the window: `second` is the code's correlation
               floor, some 1e-3 of the peak.

An off-by-one at either edge, a window that does not wrap at sample 0 / N - 1, or a
one-pass top-2 that offers an in-window runner-up moves `second` by 0.1 of the peak
or more.

The code row is a seeded random +-1 sequence at sample level: its circular
autocorrelation is a single-sample spike.  The IF is interleaved int8 I, Q with
Q = 0 and

  I = 6 roll(c, p) + a_hi roll(c, (p + d) % N) + a_lo roll(c, (p - d) % N),

(a_hi, a_lo) = (3, 2), or (2, 3) for the `mirror` variant that puts the stronger copy
on the N - spc edge.  The search runs over freqs = [-500, 0, +500] Hz; the peak falls
in the 0 Hz bin at 0-based sample p.  A search is two blocks: block 1 is the scene,
block 0 holds one amplitude-1 copy at (p + N // 2) % N, so best-of-blocks must choose
block 1 and the non-coherent sum keeps that copy at (1/6)^2 = 0.03 of the peak.
"""
import functools

import numpy as np

import acq_oracle as A
import e1b_scenarios as E

FREQS = np.array([-500.0, 0.0, 500.0])
GF = np.arange(3)[None, :]
N_BLOCKS = 2
SEED = 0x5EED0A00

# The edge distance d of every engine straddles that engine's own threshold between
# the one-pass top-2 and the exact pass (2 spc - 1 against the distance between one
# thread's samples); 16 is the default window.
#   compiled fp64 16368 plan  SPACING 528: one pass up to spc = 264
#   compiled fp64 16000 plan  SPACING 400: one pass up to spc = 200
#   fp32 (16368)              a thread's outputs lie 528 apart: as the 16368 plan
#   generic, N = 5000         stats1_exact: 1024 threads, 5000 - 4 * 1024 = 904 across
#                             the wrap -> one pass up to spc = 452
#   generic, N = 4111         4111 - 4 * 1024 = 15 across the wrap -> up to spc = 8
#   generic forced at 16368   the {3, 16, 11, 31} four-step plan, N1 = 48: a column's
#                             samples lie 48 apart, its fused top-2 serves up to
#                             spc = 24; above that the rows go to the generic
#                             statistics, 16368 - 15 * 1024 = 1008 across the wrap ->
#                             one pass up to spc = 504, two passes above
ENGINES = {
    "f64-16368": dict(fs=16.368e6, n=16368, ds=(264, 16)),
    "f64-16000": dict(fs=16.0e6, n=16000, ds=(200, 16)),
    "f32-16368": dict(fs=16.368e6, n=16368, ds=(264, 16)),
    "mixed-5000": dict(fs=5.0e6, n=5000, ds=(452, 16)),
    "bluestein-4111": dict(fs=4.111e6, n=4111, ds=(8, 16)),
    "m4-16368": dict(fs=16.368e6, n=16368, ds=(24, 504, 16),
                     env={"GNSSCORR_ACQ_GENERIC": "1"}, n1=48),
}
STATS_THREADS = 1024     # kStatsThreads of the generic engine's one-pass statistics


def stats1_exact(n, spc):
    """The generic engine's test for its one-pass statistics (csrc/acq64_gen.hip)."""
    r = STATS_THREADS if n <= STATS_THREADS else n - STATS_THREADS * ((n - 1) // STATS_THREADS)
    return 2 * spc - 1 <= min(r, STATS_THREADS)


def positions(n):
    """Peak samples: both ends of the row, a few samples in from each, one interior."""
    return (0, 5, n - 6, n - 1, 4321 % n)


def cases(engine):
    """(p, d, spc, mirror) of every window case of one engine."""
    e = ENGINES[engine]
    return [(p, d, spc, mirror) for d in e["ds"] for p in positions(e["n"])
            for spc in (d, d + 1) for mirror in (False, True)]


def case_id(c):
    p, d, spc, mirror = c
    return f"p{p}-d{d}-spc{spc}{'-mirror' if mirror else ''}"


@functools.lru_cache(maxsize=None)
def code_row(n):
    """(1, n) int8: the seeded random +-1 code of length n."""
    rng = np.random.default_rng(SEED + n)
    return (2 * rng.integers(0, 2, n) - 1).astype(np.int8)[None, :]


def _iq(i_samples):
    out = np.zeros(2 * len(i_samples), np.int8)
    out[0::2] = i_samples
    return out


def scene_block(n, p, d, mirror=False):
    """One block (interleaved int8 I, Q) with the peak at p and copies at p +- d."""
    c = code_row(n)[0].astype(np.int64)
    a_hi, a_lo = (2, 3) if mirror else (3, 2)
    return _iq(6 * np.roll(c, p) + a_hi * np.roll(c, (p + d) % n) + a_lo * np.roll(c, (p - d) % n))


def decoy_block(n, p):
    """Block 0 of a search: one amplitude-1 copy half a row away from p."""
    return _iq(np.roll(code_row(n)[0].astype(np.int64), (p + n // 2) % n))


def scene_if(n, p, d, mirror=False):
    """The two-block IF of a window case: [decoy, scene]."""
    return np.concatenate([decoy_block(n, p), scene_block(n, p, d, mirror)])


def tied_if(n, n_blocks, p=4321, d=16):
    """n_blocks bit-identical scene blocks: every block maximum ties exactly."""
    return np.tile(scene_block(n, p % n, d), n_blocks)


def _blockless(ref_rows):
    for rr in ref_rows:
        for r in rr:
            r["block"] = -1          # the non-coherent rows carry no block choice
    return ref_rows


@functools.lru_cache(maxsize=None)
def reference(fs, n, p, d, spc, mirror, noncoherent):
    """acq_oracle.acquire of a window case, computed once per process."""
    ref, ref_rows = A.acquire(scene_if(n, p, d, mirror), fs, code_row(n), FREQS, GF, spc=spc,
                              n_blocks=N_BLOCKS, noncoherent=noncoherent, return_rows=True)
    return ref, (_blockless(ref_rows) if noncoherent else ref_rows)


@functools.lru_cache(maxsize=None)
def tied_reference(fs, n, n_blocks, group_freq=((0, 1, 2),), spc=16):
    return A.acquire(tied_if(n, n_blocks), fs, code_row(n), FREQS, np.array(group_freq), spc=spc,
                     n_blocks=n_blocks, return_rows=True)


# ---- zero-padded mode (set_zero_padded): the window is circular in keep ---------------
# One block of L = 2 keep samples against [code zeros]: a copy of the keep-chip code
# placed from sample s on correlates at lag s.  The peak copy starts at p, the weaker
# ones at (p +- dist) % keep; the search runs at a fixed spc with dist = spc (on the
# edge: counts) against dist = spc - 1 (inside the window).
PAD_FS = 2.0e6
PAD_L, PAD_KEEP, PAD_SPC = 4000, 2000, 16


def padded_cases():
    return [(p, dist, mirror) for p in (0, PAD_KEEP - 1) for dist in (PAD_SPC, PAD_SPC - 1)
            for mirror in (False, True)]


def padded_if(p, dist, mirror=False):
    c = code_row(PAD_KEEP)[0].astype(np.int64)
    a_hi, a_lo = (2, 3) if mirror else (3, 2)
    x = np.zeros(PAD_L, np.int64)
    for amp, s in ((6, p), (a_hi, (p + dist) % PAD_KEEP), (a_lo, (p - dist) % PAD_KEEP)):
        x[s:s + PAD_KEEP] += amp * c
    return _iq(x)


@functools.lru_cache(maxsize=None)
def padded_reference(p, dist, mirror):
    ref, ref_rows, _ = E.acquire(padded_if(p, dist, mirror), PAD_FS, code_row(PAD_KEEP), PAD_L,
                                 PAD_KEEP, FREQS, GF, spc=PAD_SPC, n_blocks=1)
    return ref, ref_rows
