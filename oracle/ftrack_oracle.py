"""oracle/ftrack_oracle.py -- TEST INFRASTRUCTURE ONLY.

What the fp64 numpy restatements of the float trackers share (oracle/sgt_oracle.py and
tests/{b1i,e1t,e1alt,l3}_scenarios.py): the loop coefficients, the sample reader, the
per-channel drivers around a family's `correlate` and `Loop`, and the second-peak range
two of the Scilab acquisition files write alike.  Each family's correlate, Loop.__init__,
Loop.update and Loop.advance stay in its own file: they are the line-cited restatements,
and their floating-point operation order is the reference.
"""
from __future__ import annotations

import numpy as np


def calc_loop_coef(lbw: float, zeta: float, k: float):
    """calcLoopCoef.sci:39-43 -> (tau1, tau2)."""
    wn = lbw * 8 * zeta / (4 * zeta ** 2 + 1)
    return k / (wn * wn), 2.0 * zeta / wn


def calc_fll_pll_loop_coef(pllbw: float, fllbw: float, T: float):
    """calcFLLPLLLoopCoef.sci:36-38 -> (k1, k2, k3)."""
    k1 = T * ((pllbw / 0.53) ** 2) + 1.414 * (pllbw / 0.53)
    k2 = 1.414 * (pllbw / 0.53)
    k3 = T * (fllbw / 0.25)
    return k1, k2, k3


def _raw(IF, pos, n, s):
    """n samples from sample pos of the record as tracking.sci reads them: real
    (fileType 1) or interleaved I,Q; switchIQ swaps the pair (GLONASS/L1 tracking.sci,
    GLONASS/L3 tracking.sci:276-282; the GPS and COMPASS files, `system` 0 and 2, have no
    such switch).  A key the family's settings do not have counts as fileType 2, switchIQ 0."""
    if s.get("fileType", 2) == 1:
        return IF[pos:pos + n].astype(np.float64)
    v = IF[2 * pos:2 * (pos + n)].astype(np.float64)
    r1, r2 = v[0::2], v[1::2]
    if s.get("switchIQ") and s.get("system", 1) == 1:
        return r2 + 1j * r1
    return r1 + 1j * r2


def _out(fields, segment):
    o = {f: [] for f in fields}
    o["blksize"] = []
    if segment:
        o["segment"] = []
    return o


def track(lp, fields, n_epochs, step, perturb=None, segment=False):
    """A tracking.sci per-channel loop for n_epochs epochs on the family's Loop `lp`.
    step(lp) is one epoch of the family's correlator from lp's state: (status, blksize,
    None) for a stop, else (0, blksize, sums) with lp advanced.  perturb: optional relative
    offsets applied to every epoch's sums before the loop filters.  segment: also record
    lp.segment as each epoch found it.  Returns (dict of `fields` arrays + 'blksize'
    [+ 'segment'], length = epochs processed; stop status or 0; the blksize that stopped)."""
    out = _out(fields, segment)
    status, stop_blk = 0, 0
    for _ in range(n_epochs):
        seg = lp.segment if segment else None
        st, blk, sums = step(lp)
        if st:
            status, stop_blk = st, blk
            break
        if segment:
            out["segment"].append(seg)
        if perturb is not None:
            sums = sums * (1.0 + np.asarray(perturb, np.float64))
        for f, v in zip(fields, lp.update(sums)):
            out[f].append(v)
        out["blksize"].append(blk)
    return {f: np.asarray(v) for f, v in out.items()}, status, stop_blk


def replay(lp, fields, sums, segment=False):
    """The loop half driven by given per-epoch sums [n, len(sums of the family)] instead of
    correlations of a record: lp.blksize() -> (blksize, *steps), lp.advance(blksize,
    *steps), lp.update(row)."""
    out = _out(fields, segment)
    for row in np.asarray(sums, dtype=np.float64):
        blk, *steps = lp.blksize()
        if segment:
            out["segment"].append(lp.segment)
        lp.advance(blk, *steps)
        for f, v in zip(fields, lp.update(row)):
            out[f].append(v)
        out["blksize"].append(blk)
    return {f: np.asarray(v) for f, v in out.items()}


def code_phase_range_1b(code_phase, samples_per_code, samples_per_chip):
    """codePhaseRange, 1-based, exactly as GLONASS/L3/acquisition.sci:137-150 and
    COMPASS/B1/acquisition_7x3ms.sci:162-175 both write it (code_phase: 1-based argmax)."""
    ex1 = code_phase - samples_per_chip                                  # L3 :137, B1 :162
    ex2 = code_phase + samples_per_chip                                  # :138, :163
    if ex1 < 2:                                                          # :142, :167
        return np.arange(ex2, samples_per_code + ex1 + 1)                # :143-144, :168-169
    elif ex2 > samples_per_code:                                         # :145, :170
        return np.arange(ex2 - samples_per_code, ex1 + 1)                # :146-147, :171-172
    return np.concatenate([np.arange(1, ex1 + 1),                        # :149-150, :174-175
                           np.arange(ex2, samples_per_code + 1)])
