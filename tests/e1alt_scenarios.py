"""Galileo E1 tracking alternatives: fp64 numpy restatements and scenes.

TEST INFRASTRUCTURE ONLY.  Restates, line by line and one channel at a time, the
three loops of GALILEO/E1/BOC_tracking_alternatives/ that differ from
GALILEO/E1/tracking.sci (tests/e1t_scenarios.py restates that one):

  "4ms"   tracking_4ms.sci:95-457, five arms over the whole 4092-chip code
    :107,115,123  PDIcode = PDImeandr = PDIcarr = 0.004
    :159          E1BCode = [E1BCode($) E1BCode E1BCode(1)], 4094 entries
    :163-165      meandr = [meandr($) meandr meandr(1)], 8186 entries, read literally
    :258-261      steps, blksize = ceil((4092 - remCodePhase)/codePhaseStep)
    :277-281      out of data stops the channel (status 1)
    :285-305      E/L/P code indices ceil(rem -/+ spc + k*step) + 1, remCodePhase - 4092.0
    :309-328      the same for the subcarrier, remMeandrPhase - 8184.0; an index outside
                  1..8186, on which Scilab aborts, is status 2
    :331-358      carrier, carry-over with fix, ten sums
    :361-424      FLL-assisted PLL, DLL on P-E / P-L, SLL on E-P / L-P (/1540, /770)
    :433-435      absoluteSample over codeLength
  "amb1"  tracking_ambiguous_1ms.sci:86-375, three arms on the composite sequence
    :91           settings_codeLength = 2*codeLength (the absoluteSample divisor)
    :98,107       PDIcode = PDIcarr = 0.001
    :141-145      caCode = kron(c, [1 1]) .* [+1 -1 ...], 8184 entries
    :148-151      cacCode: four padded rows of 2048, circular
    :157          codeFreq = 2*codeFreqBasis
    :230-232      blksize = ceil((8184/4 - remCodePhase)/codePhaseStep)
    :256-281      E/L/P indices into row remCodePhase2_cnt, remCodePhase - 2046.0, the counter
    :284-306      carrier, six sums
    :309-351      FLL-assisted PLL, DLL; codeFreq = 2*basis - codeNco + (carrFreq - IF)/770
    :360-362      absoluteSample over 2*codeLength, still with fs/1000
  "amb4"  tracking_ambiguous_4ms.sci:85-364, the same over the whole sequence
    :97,106       PDIcode = 0.004, PDIcarr = 0.008 (as written)
    :146          caCode = [caCode($) caCode caCode(1)], 8186 entries
    :222-224      blksize = ceil((8184 - remCodePhase)/codePhaseStep)
    :248-268      indices, remCodePhase - 8184.0
    :340, :349-351  code aiding and absoluteSample as in amb1

Results use the field names of tests/e1t_scenarios.py (the library's record): in the
ambiguous modes I_E, I_P, I_L, Q_E, Q_P, Q_L are I_P_E, I_P_P, I_P_L, Q_P_E, Q_P_P,
Q_P_L, and the fields those loops do not have are 0.

Assumptions as in e1t_scenarios: `a:step:b` yields a + k*step, complex products and
sums are plain IEEE fp64.
"""
from __future__ import annotations

import math

import numpy as np

import e1t_scenarios as E
import ftrack_oracle as T

SUMS, LOOP_FIELDS, FIELDS = E.SUMS, E.LOOP_FIELDS, E.FIELDS
MODES = {"4ms": dict(epochMs=4, ambiguous=0), "amb1": dict(epochMs=1, ambiguous=1),
         "amb4": dict(epochMs=4, ambiguous=1)}
AMB_SLOTS = (1, 2, 3, 6, 7, 8)          # I_E I_P I_L Q_E Q_P Q_L within SUMS
EPOCH_MS = {"4ms": 4, "amb1": 1, "amb4": 4}
PDI_CODE = {"4ms": 0.004, "amb1": 0.001, "amb4": 0.004}
PDI_CARR = {"4ms": 0.004, "amb1": 0.001, "amb4": 0.008}


def is_amb(mode):
    return mode != "4ms"


# ---------------------------------------------------------------- tables
def code_row_4ms(chips) -> np.ndarray:
    """tracking_4ms.sci:159, 4094 entries."""
    c = np.asarray(chips, np.float64)
    assert c.shape == (4092,)
    return np.concatenate([c[-1:], c, c[:1]])


def meandr_table_4ms(meandr_length: int = 8184) -> np.ndarray:
    """tracking_4ms.sci:163-165, the one-entry front pad as written: 8186 entries."""
    m = np.ones(meandr_length)
    m[1::2] = -1                                # meandr(2:2:$) = -1
    return np.concatenate([m[-1:], m, m[:1]])


def composite(chips) -> np.ndarray:
    """tracking_ambiguous_1ms.sci:141-145: each chip twice, times +1 -1 +1 ..., 8184 entries."""
    c = np.asarray(chips, np.float64)
    assert c.shape == (4092,)
    ca = np.kron(c, np.ones(2))
    m = np.ones(2 * 4092)
    m[1::2] = -1
    return ca * m


def composite_rows(chips) -> np.ndarray:
    """tracking_ambiguous_1ms.sci:148-151: cacCode, (4, 2048)."""
    ca = composite(chips)
    A = lambda i: ca[i - 1:i]                   # 1-based caCode(i)
    R = lambda a, b: ca[a - 1:b]                # 1-based caCode(a:b)
    return np.stack([
        np.concatenate([ca[-1:], R(1, 2046), A(2047)]),
        np.concatenate([A(2046), R(2047, 4092), A(4093)]),
        np.concatenate([A(4092), R(4093, 6138), A(6139)]),
        np.concatenate([A(6138), R(6139, 8184), A(1)]),
    ])


def composite_row_4ms(chips) -> np.ndarray:
    """tracking_ambiguous_4ms.sci:146, 8186 entries."""
    ca = composite(chips)
    return np.concatenate([ca[-1:], ca, ca[:1]])


def tables(mode, chips):
    """What correlate() takes as `tab` for one code."""
    if mode == "4ms":
        return code_row_4ms(chips), meandr_table_4ms()
    if mode == "amb1":
        return composite_rows(chips)
    return composite_row_4ms(chips)


# ---------------------------------------------------------------- correlator blocks
def _carrier(blksize, fs, carr_freq, rem_carr, raw):
    time = np.arange(blksize + 1, dtype=np.float64) / fs
    trig = ((carr_freq * 2.0 * np.pi) * time) + rem_carr
    last = trig[blksize]
    rem_carr_n = last - math.trunc(last / (2 * np.pi)) * (2 * np.pi)
    bb = np.exp(1j * trig[:blksize]) * raw
    return bb.real, bb.imag, rem_carr_n         # qBasebandSignal, iBasebandSignal


def _n_avail(IF, s, pos):
    return (len(IF) if s["fileType"] == 1 else len(IF) // 2) - pos


def correlate_4ms(IF, s, tab, pos, rem_code, rem_meandr, rem_carr, code_freq, meandr_freq,
                  carr_freq):
    """tracking_4ms.sci:258-358.  Returns (status, blksize, None) for a stop or
    (0, blksize, (sums[10], pos', remCode', remMeandr', remCarr'))."""
    row, mtab = tab
    fs = s["samplingFreq"]
    dspc, sspc = s["dllCorrelatorSpacing"], s["sllCorrelatorSpacing"]
    cstep = code_freq / fs
    mstep = meandr_freq / fs
    blksize = int(math.ceil((s["codeLength"] - rem_code) / cstep))
    if _n_avail(IF, s, pos) < blksize:
        return 1, blksize, None
    raw = E._raw(IF, pos, blksize, s)
    k = np.arange(blksize, dtype=np.float64)
    kc = k * cstep
    early = row[np.ceil((rem_code - dspc) + kc).astype(np.int64)]       # tcode2 - 1 (0-based)
    late = row[np.ceil((rem_code + dspc) + kc).astype(np.int64)]
    tP = rem_code + kc
    prompt = row[np.ceil(tP).astype(np.int64)]
    rem_code_n = (tP[-1] + cstep) - 4092.0
    km = k * mstep
    iE = np.ceil((rem_meandr - sspc) + km).astype(np.int64) + 1          # tmeandr2, 1-based
    iL = np.ceil((rem_meandr + sspc) + km).astype(np.int64) + 1
    tM = rem_meandr + km
    iP = np.ceil(tM).astype(np.int64) + 1
    if min(iE.min(), iP.min(), iL.min()) < 1 or max(iE.max(), iP.max(), iL.max()) > len(mtab):
        return 2, blksize, None
    mE, mL, mP = mtab[iE - 1], mtab[iL - 1], mtab[iP - 1]
    rem_meandr_n = (tM[-1] + mstep) - 8184.0
    qb, ib, rem_carr_n = _carrier(blksize, fs, carr_freq, rem_carr, raw)
    sums = np.array([np.sum(mE * prompt * ib), np.sum(mP * early * ib), np.sum(mP * prompt * ib),
                     np.sum(mP * late * ib), np.sum(mL * prompt * ib),
                     np.sum(mE * prompt * qb), np.sum(mP * early * qb), np.sum(mP * prompt * qb),
                     np.sum(mP * late * qb), np.sum(mL * prompt * qb)])
    return 0, blksize, (sums, pos + blksize, rem_code_n, rem_meandr_n, rem_carr_n)


def correlate_amb(mode, IF, s, tab, pos, segment, rem_code, rem_carr, code_freq, carr_freq):
    """tracking_ambiguous_1ms.sci:230-306 / tracking_ambiguous_4ms.sci:222-295.  segment:
    remCodePhase2_cnt - 1 (amb1; ignored by amb4).  Returns (1, blksize, None) out of data
    or (0, blksize, (sums[10] with the six sums in AMB_SLOTS, pos', segment', remCode', remCarr'))."""
    fs = s["samplingFreq"]
    dspc = s["dllCorrelatorSpacing"]
    length = 2 * s["codeLength"]                 # loopCnt_codeLength
    cstep = code_freq / fs
    if mode == "amb1":
        blksize = int(math.ceil((length / 4 - rem_code) / cstep))
        row = tab[segment]
    else:
        blksize = int(math.ceil((length - rem_code) / cstep))
        row = tab
    if _n_avail(IF, s, pos) < blksize:
        return 1, blksize, None
    raw = E._raw(IF, pos, blksize, s)
    kc = np.arange(blksize, dtype=np.float64) * cstep
    early = row[np.ceil((rem_code - dspc) + kc).astype(np.int64)]       # tcode2 - 1 (0-based)
    late = row[np.ceil((rem_code + dspc) + kc).astype(np.int64)]
    tP = rem_code + kc
    prompt = row[np.ceil(tP).astype(np.int64)]
    if mode == "amb1":
        rem_code_n = (tP[-1] + cstep) - 2046.0
        segment_n = (segment + 1) % 4            # remCodePhase2_cnt 1..4
    else:
        rem_code_n = (tP[-1] + cstep) - 8184.0
        segment_n = segment
    qb, ib, rem_carr_n = _carrier(blksize, fs, carr_freq, rem_carr, raw)
    sums = np.zeros(10)
    sums[list(AMB_SLOTS)] = [np.sum(early * ib), np.sum(prompt * ib), np.sum(late * ib),
                             np.sum(early * qb), np.sum(prompt * qb), np.sum(late * qb)]
    return 0, blksize, (sums, pos + blksize, segment_n, rem_code_n, rem_carr_n)


# ---------------------------------------------------------------- loops
def loop_coefs(mode, s):
    """(tau1code, tau2code, tau1meandr, tau2meandr, k1, k2, k3) as the file computes them;
    the ambiguous files have no subcarrier loop: 0, 0."""
    tc = E.calc_loop_coef(s["dllNoiseBandwidth"], s["dllDampingRatio"], 1.0)
    tm = (0.0, 0.0) if is_amb(mode) else \
        E.calc_loop_coef(s["sllNoiseBandwidth"], s["sllDampingRatio"], 1.0)
    return tc + tm + E.calc_fll_pll_loop_coef(s["pllNoiseBandwidth"], s["fllNoiseBandwidth"],
                                              PDI_CARR[mode])


class Loop:
    """Per-channel state (4ms:170-200, amb1:157-181, amb4:151-173) and the update after one
    epoch's sums (4ms:361-435, amb1:309-362, amb4:298-351)."""

    def __init__(self, mode, s, pos, acquired_freq):
        self.mode, self.s = mode, s
        (self.tau1c, self.tau2c, self.tau1m, self.tau2m, self.k1, self.k2, self.k3) = \
            loop_coefs(mode, s)
        self.pos = pos
        self.segment = 0
        amb = is_amb(mode)
        self.code_basis = 2 * s["codeFreqBasis"] if amb else s["codeFreqBasis"]
        self.code_freq = self.code_basis
        self.meandr_freq = 0.0 if amb else s["meandrFreqBasis"]
        self.rem_code = self.rem_meandr = self.rem_carr = 0.0
        self.carr_freq = self.carr_basis = acquired_freq
        self.old_code_nco = self.old_code_err = 0.0
        self.old_meandr_nco = self.old_meandr_err = 0.0
        self.old_carr_nco = self.old_carr_err = 0.0
        self.I1 = self.Q1 = 0.001

    def blksize(self):
        fs = self.s["samplingFreq"]
        cstep = self.code_freq / fs
        length = {"4ms": self.s["codeLength"], "amb1": 2 * self.s["codeLength"] / 4,
                  "amb4": 2 * self.s["codeLength"]}[self.mode]
        mstep = self.meandr_freq / fs
        return int(math.ceil((length - self.rem_code) / cstep)), cstep, mstep

    def advance(self, blk, cstep, mstep):
        """Carry-over without a record (replay)."""
        carry = {"4ms": 4092.0, "amb1": 2046.0, "amb4": 8184.0}[self.mode]
        self.rem_code = ((self.rem_code + float(blk - 1) * cstep) + cstep) - carry
        if self.mode == "amb1":
            self.segment = (self.segment + 1) % 4
        if self.mode == "4ms":
            self.rem_meandr = ((self.rem_meandr + float(blk - 1) * mstep) + mstep) - 8184.0
        last = ((self.carr_freq * 2.0 * np.pi) * (float(blk) / self.s["samplingFreq"])) + \
            self.rem_carr
        self.rem_carr = last - math.trunc(last / (2 * np.pi)) * (2 * np.pi)
        self.pos += blk

    def update(self, sums):
        """One epoch's loop filters; returns the record values in FIELDS order."""
        s, amb = self.s, is_amb(self.mode)
        v = [float(x) for x in sums]
        if amb:
            v = [x if j in AMB_SLOTS else 0.0 for j, x in enumerate(v)]
        I_E_P, I_P_E, I_P_P, I_P_L, I_L_P, Q_E_P, Q_P_E, Q_P_P, Q_P_L, Q_L_P = v
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
        pdi = PDI_CODE[self.mode]
        cE = math.sqrt(I_P_E * I_P_E + Q_P_E * Q_P_E)
        cL = math.sqrt(I_P_L * I_P_L + Q_P_L * Q_P_L)
        code_err = (cE - cL) / (cE + cL)
        code_nco = self.old_code_nco + (self.tau2c / self.tau1c) * (code_err - self.old_code_err) + \
            code_err * (pdi / self.tau1c)
        self.old_code_nco, self.old_code_err = code_nco, code_err
        if amb:
            self.code_freq = self.code_basis - code_nco + ((self.carr_freq - s["IF"]) / 770)
            meandr_err = meandr_nco = 0.0
            abs_sample = self.pos - self.rem_code * (s["samplingFreq"] / 1000) / \
                (s["codeLength"] * 2)
        else:
            self.code_freq = s["codeFreqBasis"] - code_nco + ((self.carr_freq - s["IF"]) / 1540)
            mE = math.sqrt(I_E_P * I_E_P + Q_E_P * Q_E_P)
            mL = math.sqrt(I_L_P * I_L_P + Q_L_P * Q_L_P)
            meandr_err = (mE - mL) / (mE + mL)
            meandr_nco = self.old_meandr_nco + \
                (self.tau2m / self.tau1m) * (meandr_err - self.old_meandr_err) + \
                meandr_err * (pdi / self.tau1m)
            self.old_meandr_nco, self.old_meandr_err = meandr_nco, meandr_err
            self.meandr_freq = s["meandrFreqBasis"] - meandr_nco + \
                ((self.carr_freq - s["IF"]) / 770)
            abs_sample = self.pos - self.rem_code * (s["samplingFreq"] / 1000) / s["codeLength"]
        return (I_E_P, I_P_E, I_P_P, I_P_L, I_L_P, Q_E_P, Q_P_E, Q_P_P, Q_P_L, Q_L_P,
                self.carr_freq, self.code_freq, self.meandr_freq, abs_sample, code_err, code_nco,
                meandr_err, meandr_nco, carr_err, carr_nco)


def correlate(mode, IF, s, tab, lp):
    """One epoch from the state of Loop `lp`, which is advanced on success.  Returns
    (status, blksize, sums[10] or None)."""
    if mode == "4ms":
        st, blk, r = correlate_4ms(IF, s, tab, lp.pos, lp.rem_code, lp.rem_meandr, lp.rem_carr,
                                   lp.code_freq, lp.meandr_freq, lp.carr_freq)
        if st:
            return st, blk, None
        sums, lp.pos, lp.rem_code, lp.rem_meandr, lp.rem_carr = r
    else:
        st, blk, r = correlate_amb(mode, IF, s, tab, lp.pos, lp.segment, lp.rem_code,
                                   lp.rem_carr, lp.code_freq, lp.carr_freq)
        if st:
            return st, blk, None
        sums, lp.pos, lp.segment, lp.rem_code, lp.rem_carr = r
    return 0, blk, sums


def track(mode, IF, s, chips, code_phase_1b, acquired_freq, n_epochs, skip=0, perturb=None):
    """The file's per-channel loop for n_epochs epochs: a dict of FIELDS arrays + 'blksize',
    'segment' (the row each epoch used), 'status', 'stop_blksize'.  perturb: optional [10]
    relative offsets applied to every epoch's sums before the loop filters."""
    tab = tables(mode, chips)
    lp = Loop(mode, s, skip + code_phase_1b - 1, acquired_freq)   # mseek
    res, res["status"], res["stop_blksize"] = T.track(
        lp, FIELDS, n_epochs, lambda lp: correlate(mode, IF, s, tab, lp), perturb, segment=True)
    return res


def replay(mode, sums, s, code_phase_1b, acquired_freq, skip=0):
    """The loop half driven by given per-epoch sums [n, 10] (SUMS order)."""
    return T.replay(Loop(mode, s, skip + code_phase_1b - 1, acquired_freq), FIELDS, sums,
                    segment=True)


# ---------------------------------------------------------------- closed-loop scenes
# Each mode runs the 40 ms three-PRN scene of e1t_scenarios (its record, seed 3, its
# Dopplers and code phases): 10 epochs at 4 ms, 40 at 1 ms.  "4ms" and "amb1" keep its
# acquisition errors (-12, -9, -9 Hz).  "amb4" does not pass the decidability check of
# tests/test_e1alt_cpu.py with them: PRN 12's Q sums pass through zero in epoch 9 (Q_P
# 5e3 beside I_P 7e5), which moves three fields by 1.1 to 1.7 times the bound.  Its
# channels start 20 Hz below the planted carrier instead (worst field 0.09 of the
# bound).  Keep these.
SCENE_EPOCHS = {"4ms": E.SCENE_MS // 4, "amb1": E.SCENE_MS, "amb4": E.SCENE_MS // 4}
SCENE_SEED = {"4ms": E.SCENE_SEED, "amb1": E.SCENE_SEED, "amb4": E.SCENE_SEED}
SCENE_ACQ_ERR = {"4ms": None, "amb1": None, "amb4": (-20.0, -20.0, -20.0)}


def closed_loop_scene(mode):
    """(IF int8, codes (3, 4092), chans) as e1t_scenarios.closed_loop_scene, with the
    mode's acquisition errors."""
    assert SCENE_SEED[mode] == E.SCENE_SEED
    IF, codes, chans = E.closed_loop_scene()
    errs = SCENE_ACQ_ERR[mode]
    if errs is not None:
        IFc = E.settings()["IF"]
        chans = [(row, cp, IFc + d["doppler"] + e, rate)
                 for (row, cp, _, rate), d, e in zip(chans, E.SCENE_SATS, errs)]
    return IF, codes, chans
