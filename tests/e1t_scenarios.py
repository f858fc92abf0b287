"""Galileo E1B float tracking: fp64 numpy restatement and synthetic scenes.

TEST INFRASTRUCTURE ONLY.  Restates GALILEO/E1/tracking.sci:95-455 line by line,
one channel at a time, in the shape of oracle/sgt_oracle.py:

  :157-160  the 4092 chips split into four padded 1025-entry rows
  :164-168  the subcarrier table [m($-1) m($) m m(1) m(2)], m = +1,-1,... (2046);
            read literally here (the kernel uses the parity of ceil(t) instead)
  :263-266  codePhaseStep, meandrPhaseStep, blksize = ceil((1023 - remCode)/step)
  :282-286  out of data stops the channel (status 1)
  :290-315  E/L/P code indices ceil(rem -/+ spc + k*step) + 1, remCodePhase, segment
  :319-338  the same for the subcarrier; an index outside 1..2050, on which Scilab
            aborts, is status 2 (decided on the first early and the last late index:
            the ranges rise with k)
  :341-368  carrier, carry-over with fix, ten sums (first letter: subcarrier arm)
  :371-425  FLL-assisted PLL, DLL on P-E / P-L, SLL on E-P / L-P
  :433-435  absoluteSample, the whole code length in the divisor

Assumptions as in sgt_oracle: `a:step:b` yields a + k*step, complex products and
sums are plain IEEE fp64.
"""
from __future__ import annotations

import math
import os

import numpy as np

import ftrack_oracle as T
from ftrack_oracle import _raw, calc_fll_pll_loop_coef, calc_loop_coef  # noqa: F401

SUMS = ("I_E_P", "I_P_E", "I_P_P", "I_P_L", "I_L_P", "Q_E_P", "Q_P_E", "Q_P_P", "Q_P_L", "Q_L_P")
LOOP_FIELDS = ("carrFreq", "codeFreq", "meandrFreq", "absoluteSample", "dllDiscr", "dllDiscrFilt",
               "sllDiscr", "sllDiscrFilt", "pllDiscr", "pllDiscrFilt")
FIELDS = SUMS + LOOP_FIELDS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "e1b_codes.npz")


def fixture_codes():
    """(codes (3, 4092) int8, prns) of tests/golden/e1b_codes.npz: E1B PRN 11, 12, 19."""
    g = np.load(GOLDEN)
    return g["codes"], [int(p) for p in g["prns"]]


def settings(**kw) -> dict:
    """GALILEO/E1/initSettings.sci:65-107 defaults, overridable."""
    s = dict(fileType=2, samplingFreq=16e6, codeFreqBasis=1.023e6, meandrFreqBasis=2.046e6,
             IF=2.42e6, codeLength=4092, meandrLength=8184, dllDampingRatio=0.7,
             dllNoiseBandwidth=0.5, dllCorrelatorSpacing=0.25, sllDampingRatio=0.7,
             sllNoiseBandwidth=0.5, sllCorrelatorSpacing=0.1, pllNoiseBandwidth=25.0,
             fllNoiseBandwidth=250.0)
    s.update(kw)
    return s


def split_code(chips) -> np.ndarray:
    """tracking.sci:157-160: E1BCodeSplit, (4, 1025)."""
    c = np.asarray(chips, np.float64)
    assert c.shape == (4092,)
    E = lambda i: c[i - 1]                      # 1-based E1BCode(i)
    R = lambda a, b: c[a - 1:b]                 # 1-based E1BCode(a:b)
    return np.stack([
        np.concatenate([[c[-1]], R(1, 1023), [E(1024)]]),
        np.concatenate([[E(1023)], R(1024, 2046), [E(2047)]]),
        np.concatenate([[E(2046)], R(2047, 3069), [E(3070)]]),
        np.concatenate([[E(3069)], R(3070, 4092), [E(1)]]),
    ])


def meandr_table(meandr_length: int = 8184) -> np.ndarray:
    """tracking.sci:164-168, the two-entry front pad as written: 2050 entries."""
    m = np.ones(meandr_length // 4)
    m[1::2] = -1                                # meandr(2:2:$) = -1
    return np.concatenate([m[-2:-1], m[-1:], m, m[0:1], m[1:2]])


def correlate(IF, s, rows, mtab, pos, segment, rem_code, rem_meandr, rem_carr, code_freq,
              meandr_freq, carr_freq):
    """One epoch of the correlator block (:263-368).  segment: 0..3.  Returns
    (status, blksize, None) for a stop (1 out of data, 2 subcarrier index outside
    the table) or (0, blksize, (sums[10], pos', segment', remCode', remMeandr', remCarr'))."""
    fs = s["samplingFreq"]
    dspc, sspc = s["dllCorrelatorSpacing"], s["sllCorrelatorSpacing"]
    cstep = code_freq / fs
    mstep = meandr_freq / fs
    blksize = int(math.ceil((s["codeLength"] / 4 - rem_code) / cstep))
    n_avail = (len(IF) if s["fileType"] == 1 else len(IF) // 2) - pos
    if n_avail < blksize:
        return 1, blksize, None
    raw = _raw(IF, pos, blksize, s)
    k = np.arange(blksize, dtype=np.float64)
    kc = k * cstep
    row = rows[segment]
    early = row[np.ceil((rem_code - dspc) + kc).astype(np.int64)]       # tcode2 - 1 (0-based)
    late = row[np.ceil((rem_code + dspc) + kc).astype(np.int64)]
    tP = rem_code + kc
    prompt = row[np.ceil(tP).astype(np.int64)]
    rem_code_n = (tP[-1] + cstep) - 4092.0 / 4
    segment_n = (segment + 1) % 4
    km = k * mstep
    iE = np.ceil((rem_meandr - sspc) + km).astype(np.int64) + 1          # tmeandr2, 1-based
    iL = np.ceil((rem_meandr + sspc) + km).astype(np.int64) + 1
    tM = rem_meandr + km
    iP = np.ceil(tM).astype(np.int64) + 1
    if min(iE.min(), iP.min(), iL.min()) < 1 or max(iE.max(), iP.max(), iL.max()) > len(mtab):
        return 2, blksize, None
    mE, mL, mP = mtab[iE - 1], mtab[iL - 1], mtab[iP - 1]
    rem_meandr_n = (tM[-1] + mstep) - 8184.0 / 4
    time = np.arange(blksize + 1, dtype=np.float64) / fs
    trig = ((carr_freq * 2.0 * np.pi) * time) + rem_carr
    last = trig[blksize]
    rem_carr_n = last - math.trunc(last / (2 * np.pi)) * (2 * np.pi)
    bb = np.exp(1j * trig[:blksize]) * raw
    qb, ib = bb.real, bb.imag
    sums = np.array([np.sum(mE * prompt * ib), np.sum(mP * early * ib), np.sum(mP * prompt * ib),
                     np.sum(mP * late * ib), np.sum(mL * prompt * ib),
                     np.sum(mE * prompt * qb), np.sum(mP * early * qb), np.sum(mP * prompt * qb),
                     np.sum(mP * late * qb), np.sum(mL * prompt * qb)])
    return 0, blksize, (sums, pos + blksize, segment_n, rem_code_n, rem_meandr_n, rem_carr_n)


class Loop:
    """Per-channel loop state (:170-205) and the update after one epoch's sums (:371-435)."""

    def __init__(self, s, pos, acquired_freq):
        self.s = s
        self.tau1c, self.tau2c = calc_loop_coef(s["dllNoiseBandwidth"], s["dllDampingRatio"], 1.0)
        self.tau1m, self.tau2m = calc_loop_coef(s["sllNoiseBandwidth"], s["sllDampingRatio"], 1.0)
        self.k1, self.k2, self.k3 = calc_fll_pll_loop_coef(s["pllNoiseBandwidth"],
                                                           s["fllNoiseBandwidth"], 0.001)
        self.pos = pos
        self.segment = 0
        self.code_freq = s["codeFreqBasis"]
        self.meandr_freq = s["meandrFreqBasis"]
        self.rem_code = self.rem_meandr = self.rem_carr = 0.0
        self.carr_freq = self.carr_basis = acquired_freq
        self.old_code_nco = self.old_code_err = 0.0
        self.old_meandr_nco = self.old_meandr_err = 0.0
        self.old_carr_nco = self.old_carr_err = 0.0
        self.I1 = self.Q1 = 0.001

    def blksize(self):
        cstep = self.code_freq / self.s["samplingFreq"]
        mstep = self.meandr_freq / self.s["samplingFreq"]
        return int(math.ceil((self.s["codeLength"] / 4 - self.rem_code) / cstep)), cstep, mstep

    def advance(self, blk, cstep, mstep):
        """Carry-over without a record (replay): :310-315, :338, :341-346."""
        self.rem_code = ((self.rem_code + float(blk - 1) * cstep) + cstep) - 4092.0 / 4
        self.segment = (self.segment + 1) % 4
        self.rem_meandr = ((self.rem_meandr + float(blk - 1) * mstep) + mstep) - 8184.0 / 4
        last = ((self.carr_freq * 2.0 * np.pi) * (float(blk) / self.s["samplingFreq"])) + \
            self.rem_carr
        self.rem_carr = last - math.trunc(last / (2 * np.pi)) * (2 * np.pi)
        self.pos += blk

    def update(self, sums):
        """:371-435 on one epoch's sums; returns the record values in FIELDS order."""
        s = self.s
        I_E_P, I_P_E, I_P_P, I_P_L, I_L_P, Q_E_P, Q_P_E, Q_P_P, Q_P_L, Q_L_P = \
            (float(x) for x in sums)
        I2, Q2 = self.I1, self.Q1
        self.I1, self.Q1 = I_P_P, Q_P_P
        cross = self.I1 * Q2 - I2 * self.Q1
        dot = abs(self.I1 * I2 + self.Q1 * Q2)
        freq_err = math.atan2(cross, dot) / math.pi
        carr_err = math.atan(Q_P_P / I_P_P) / (2.0 * math.pi)
        carr_nco = self.old_carr_nco + self.k1 * carr_err - self.k2 * self.old_carr_err - \
            self.k3 * freq_err
        self.old_carr_nco, self.old_carr_err = carr_nco, carr_err
        self.carr_freq = self.carr_basis + carr_nco
        cE = math.sqrt(I_P_E * I_P_E + Q_P_E * Q_P_E)
        cL = math.sqrt(I_P_L * I_P_L + Q_P_L * Q_P_L)
        code_err = (cE - cL) / (cE + cL)
        code_nco = self.old_code_nco + (self.tau2c / self.tau1c) * (code_err - self.old_code_err) + \
            code_err * (0.001 / self.tau1c)
        self.old_code_nco, self.old_code_err = code_nco, code_err
        self.code_freq = s["codeFreqBasis"] - code_nco + ((self.carr_freq - s["IF"]) / 1540)
        mE = math.sqrt(I_E_P * I_E_P + Q_E_P * Q_E_P)
        mL = math.sqrt(I_L_P * I_L_P + Q_L_P * Q_L_P)
        meandr_err = (mE - mL) / (mE + mL)
        meandr_nco = self.old_meandr_nco + \
            (self.tau2m / self.tau1m) * (meandr_err - self.old_meandr_err) + \
            meandr_err * (0.001 / self.tau1m)
        self.old_meandr_nco, self.old_meandr_err = meandr_nco, meandr_err
        self.meandr_freq = s["meandrFreqBasis"] - meandr_nco + ((self.carr_freq - s["IF"]) / 770)
        abs_sample = self.pos - self.rem_code * (s["samplingFreq"] / 1000) / s["codeLength"]
        return (I_E_P, I_P_E, I_P_P, I_P_L, I_L_P, Q_E_P, Q_P_E, Q_P_P, Q_P_L, Q_L_P,
                self.carr_freq, self.code_freq, self.meandr_freq, abs_sample, code_err, code_nco,
                meandr_err, meandr_nco, carr_err, carr_nco)


def track(IF, s, chips, code_phase_1b, acquired_freq, n_ms, skip=0, perturb=None):
    """tracking.sci's per-channel loop for n_ms epochs.  Returns a dict of FIELDS arrays
    (length = epochs processed) + 'blksize', 'segment' (0-based, the quarter each epoch
    used), 'status' (0, or the stop status) and 'stop_blksize'.
    perturb: optional [10] relative offsets applied to every epoch's sums before the loop
    filters (the decidability check of the closed-loop scenes)."""
    rows, mtab = split_code(chips), meandr_table(s["meandrLength"])
    lp = Loop(s, skip + code_phase_1b - 1, acquired_freq)   # mseek, :150-151

    def epoch(lp):
        st, blk, r = correlate(IF, s, rows, mtab, lp.pos, lp.segment, lp.rem_code, lp.rem_meandr,
                               lp.rem_carr, lp.code_freq, lp.meandr_freq, lp.carr_freq)
        if st:
            return st, blk, None
        sums, lp.pos, lp.segment, lp.rem_code, lp.rem_meandr, lp.rem_carr = r
        return 0, blk, sums
    res, res["status"], res["stop_blksize"] = T.track(lp, FIELDS, n_ms, epoch, perturb,
                                                      segment=True)
    return res


def replay(sums, s, code_phase_1b, acquired_freq, skip=0):
    """The loop half driven by given per-epoch sums [n, 10] (SUMS order)."""
    return T.replay(Loop(s, skip + code_phase_1b - 1, acquired_freq), FIELDS, sums, segment=True)


def synth_e1b(n, sats, fs=16e6, IF=2.42e6, noise=6.0, seed=0):
    """int8 interleaved I,Q of n samples: a continuous E1B signal per entry of `sats`
    (dicts: chips [4092], start = the sample (may be fractional) at which the primary
    code begins, doppler [Hz], amp, phase [rad]).  With t the time since `start`: code
    phase t * (1.023e6 + doppler/1540) chips modulo 4092, subcarrier sign from the
    half-chip parity (+ on the first half of a chip), carrier exp(-i (2 pi (IF + doppler)
    t_abs + phase)) so the tracker's wipe-off exp(+i ...) stops it, plus seeded Gaussian
    noise of sigma `noise` per component, rounded and clipped to int8."""
    rng = np.random.default_rng(seed)
    idx = np.arange(n, dtype=np.float64)
    x = noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for sat in sats:
        chips = np.asarray(sat["chips"], np.float64)
        rate = 1.023e6 + sat["doppler"] / 1540.0
        ph = ((idx - sat["start"]) / fs) * rate             # chips since the code began
        half = np.floor(2.0 * ph).astype(np.int64)
        chip = np.floor_divide(half, 2) % 4092
        sub = 1.0 - 2.0 * (half % 2)
        arg = 2.0 * np.pi * (IF + sat["doppler"]) * (idx / fs) + sat.get("phase", 0.0)
        x += sat.get("amp", 12.0) * chips[chip] * sub * np.exp(-1j * arg)
    out = np.empty(2 * n, np.int8)
    out[0::2] = np.clip(np.rint(x.real), -127, 127)
    out[1::2] = np.clip(np.rint(x.imag), -127, 127)
    return out


# The closed-loop scene of the CPU and GPU tiers: PRN 11, 12 and 19 on one 40 ms record
# (ten segment wraps), different Dopplers and code phases.  The seeds are chosen so that
# the decidability condition of tests/test_e1t_cpu.py holds; keep them.
SCENE_MS = 40
SCENE_SEED = 3
SCENE_SATS = (dict(row=0, start=1200.95, doppler=1500.0, acq_err=-12.0, phase=-3.0),
              dict(row=1, start=30711.9, doppler=-2250.0, acq_err=-9.0, phase=0.0),
              dict(row=2, start=51200.97, doppler=310.0, acq_err=-9.0, phase=1.0))


def closed_loop_scene(fs=16e6):
    """(IF int8, codes (3, 4092), chans: list of (row, code_phase_1b, acquired_freq,
    planted code rate)).  Each channel starts on the first whole sample of its code."""
    codes, _ = fixture_codes()
    s = settings(samplingFreq=fs)
    n = int(fs * (SCENE_MS + 5) / 1000)
    sats = [dict(chips=codes[d["row"]], start=d["start"], doppler=d["doppler"], phase=d["phase"])
            for d in SCENE_SATS]
    IF = synth_e1b(n, sats, fs=fs, IF=s["IF"], seed=SCENE_SEED)
    chans = [(d["row"], int(math.ceil(d["start"])) + 1, s["IF"] + d["doppler"] + d["acq_err"],
              1.023e6 + d["doppler"] / 1540.0) for d in SCENE_SATS]
    return IF, codes, chans
