"""GLONASS L3OC: fp64 numpy restatement of the Scilab receiver and synthetic scenes.

TEST INFRASTRUCTURE ONLY (no GPU).  Restates POSTPROCESSING_SCILAB_RECEIVERS/GLONASS/L3:

  include/generateCAcode.sci:40-139  the code generator in register-product form with
                the literal G2 initial-state table, its three defects included: the
                line commented #32 assigns row 31 again, row 32 is never assigned (Scilab
                zero-fills it: the code is all zero), row 64 repeats row 63
  include/makeCaTable.sci:41-69      the data-channel code (id PRN + 32) sampled by
                ceil(ts*n/tc), the last index forced to codeLength
  acquisition.sci:53-166             10 ms of signal against five code periods signed by
                the overlay [-1 -1 -1 1 -1] and zero-padded, the first 5*samplesPerCode
                lags kept, and the three-branch codePhaseRange written on samplesPerCode
                in its 1-based form exactly as the file has it
  tracking.sci:123-423               the per-channel loop: one code NCO, the pilot
                (id PRN) and data (id PRN + 32) codes on its three index sequences,
                twelve sums, FLL and DLL on the data sums, PLL on the pilot prompt

Assumptions as in oracle/sgt_oracle.py: `a:step:b` yields a + k*step, complex products
and sums are plain IEEE fp64.  An index of codePhaseRange past the row's end, on which
Scilab would abort (only for samplesPerCode equal to the row length), is dropped.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import e1b_scenarios as E1B
import ftrack_oracle as T
from ftrack_oracle import (_raw, calc_fll_pll_loop_coef, calc_loop_coef,  # noqa: F401
                           code_phase_range_1b)

SUMS = ("I_E", "I_P", "I_L", "Q_E", "Q_P", "Q_L", "I_E2", "I_P2", "I_L2", "Q_E2", "Q_P2", "Q_L2")
LOOP_FIELDS = ("carrFreq", "codeFreq", "absoluteSample", "dllDiscr", "dllDiscrFilt", "pllDiscr",
               "pllDiscrFilt")
FIELDS = SUMS + LOOP_FIELDS
BARKER = np.array([-1, -1, -1, 1, -1])                       # acquisition.sci:94-96
NH = np.array([-1, -1, -1, -1, 1, 1, -1, 1, -1, 1])


# ---- generateCAcode.sci ---------------------------------------------------------------
def _g2s_table():
    """g2s(1:64, 1:7) as the file builds it: rows are 1-based here too (row 0 unused)."""
    g2s = np.zeros((65, 7))

    def binary(n):                                # the listed +-1 pattern of number n
        return np.array([1 if (n >> (6 - j)) & 1 else -1 for j in range(7)])
    for n in range(1, 32):
        g2s[n] = -1 * binary(n)                   # :40-70
    g2s[31] = -1 * binary(32)                     # :72, commented #32, assigns row 31
    for n in range(33, 64):
        g2s[n] = -1 * binary(n)                   # :74-104
    g2s[64] = -1 * binary(63)                     # :105, "#63 Some dirty tricks"
    return g2s                                    # row 32 stays zero


G2S = _g2s_table()


@functools.lru_cache(maxsize=None)
def _g1():
    reg = [-1 * v for v in (-1, -1, 1, 1, -1, 1, -1, -1, 1, 1, 1, -1, -1, -1)]   # :112
    g1 = np.zeros(10230)
    for i in range(10230):
        g1[i] = reg[13]
        save = reg[3] * reg[7] * reg[12] * reg[13]                                # :117
        reg = [save] + reg[:13]
    return g1


@functools.lru_cache(maxsize=None)
def generate_code(code_id: int) -> np.ndarray:
    """generateCAcode(PRN), float64 [10230] of +-1 (all zero for id 32)."""
    reg2 = [float(v) for v in G2S[code_id]]                                      # :127
    g2 = np.zeros(10230)
    for i in range(10230):
        g2[i] = reg2[6]
        save = reg2[5] * reg2[6]                                                  # :133
        reg2 = [save] + reg2[:6]
    out = -(_g1() * g2) + 0.0                                                     # :139 (-0 -> 0)
    out.setflags(write=False)
    return out


# ---- settings -------------------------------------------------------------------------
def settings(**kw) -> dict:
    """GLONASS/L3/initSettings.sci:64-96 defaults, overridable."""
    s = dict(fileType=2, switchIQ=0, IF=-2.025e6, GLONASS_nominal_freq=1202.025e6,
             samplingFreq=24e6, codeFreqBasis=10.23e6, codeLength=10230, acqSearchBand=5,
             acqThreshold=3.0, dllDampingRatio=0.7, dllNoiseBandwidth=1.0,
             dllCorrelatorSpacing=0.4, pllNoiseBandwidth=25.0, fllNoiseBandwidth=250.0)
    s.update(kw)
    return s


# ---- makeCaTable.sci and the replica --------------------------------------------------
def samples_per_code(s):
    return int(round(s["samplingFreq"] / (s["codeFreqBasis"] / s["codeLength"])))


def ca_table_row(s, prn):
    """caCodesTable(PRN, :) (makeCaTable.sci:54-69): the data-channel code, sampled."""
    spc_ = samples_per_code(s)
    ts, tc = 1 / s["samplingFreq"], 1 / s["codeFreqBasis"]
    idx = np.ceil((ts * np.arange(1, spc_ + 1)) / tc).astype(np.int64)
    idx[-1] = s["codeLength"]
    return generate_code(prn + 32)[idx - 1]


def overlay_replica(s, prn):
    """The five signed code periods of acquisition.sci:94-96 (without the zeros)."""
    row = ca_table_row(s, prn)
    return np.concatenate([b * row for b in BARKER])


def bins(s):
    """acquisition.sci:66, :103-105."""
    nb = int(round(s["acqSearchBand"] * 2 * 5)) + 1
    k = np.arange(1, nb + 1)
    return s["IF"] - (s["acqSearchBand"] / 2) * 1000 + (1000 / (2 * 5)) * (k - 1)


# ---- the second-peak range of acquisition.sci:134-153 ---------------------------------
def period_second(row, argmax0, spc, period):
    """secondPeakSize (:153) of one kept row; argmax0 0-based."""
    rng = code_phase_range_1b(argmax0 + 1, period, spc)
    rng = rng[rng <= len(row)]
    return float(row[rng - 1].max())


def apply_period_rule(ref, ref_rows, spc, period):
    """Re-state `second` / `metric` of an e1b_scenarios.acquire result by the L3 rule."""
    for g, rg in enumerate(ref):
        for b, rr in enumerate(ref_rows[g]):
            rr["second"] = period_second(rg["results"][b], rr["argmax"], spc, period)
        rg["second"] = period_second(rg["results"][rg["bin"]], rg["code_phase"] - 1, spc, period)
        rg["metric"] = rg["peak"] / rg["second"]
    return ref, ref_rows


def acquire(IF, s, prn):
    """acquisition.sci:53-166 for one PRN on the first 10 ms of IF (int8 interleaved I,Q;
    switchIQ 0).  Returns dict(peak, second, metric, bin, code_phase, carr_freq, results)."""
    spc_ = samples_per_code(s)
    fs = s["samplingFreq"]
    x = np.asarray(IF[:2 * 10 * spc_], np.float64)
    signal1 = x[0::2] + 1j * x[1::2]                                             # :57
    phase_points = np.arange(10 * spc_) * 2 * np.pi * (1 / fs)                    # :63
    frq = bins(s)
    cf = np.conj(np.fft.fft(np.concatenate([overlay_replica(s, prn), np.zeros(5 * spc_)])))
    results = np.zeros((len(frq), 5 * spc_))
    for i, f in enumerate(frq):
        X = np.fft.fft(np.exp(1j * f * phase_points) * signal1)                   # :107-111
        results[i] = (np.abs(np.fft.ifft(X * cf)) ** 2)[:5 * spc_]                # :114-121
    bin_idx = int(np.argmax(results.max(axis=1)))                                 # :129
    code_phase = int(np.argmax(results.max(axis=0))) + 1                          # :132
    chip = int(round(fs / s["codeFreqBasis"]))                                    # :135
    second = period_second(results[bin_idx], code_phase - 1, chip, spc_)
    peak = results.max()
    return dict(peak=peak, second=second, metric=peak / second, bin=bin_idx,
                code_phase=code_phase, carr_freq=float(frq[bin_idx]), results=results)


# ---- tracking.sci ---------------------------------------------------------------------
def padded(code):
    """[caCode($) caCode caCode(1)] (:174, :179)."""
    return np.concatenate([code[-1:], code, code[:1]])


def correlate(IF, s, prow, drow, pos, rem_code, rem_carr, code_freq, carr_freq):
    """One epoch of the correlator block (:265-351); prow / drow the padded pilot / data
    rows.  Returns (1, blksize, None) out of data, else
    (0, blksize, (sums[12], pos', remCode', remCarr'))."""
    fs, spc = s["samplingFreq"], s["dllCorrelatorSpacing"]
    step = code_freq / fs                                                         # :265
    blksize = int(math.ceil((s["codeLength"] - rem_code) / step))                 # :267
    if len(IF) // 2 - pos < blksize:
        return 1, blksize, None
    raw = _raw(IF, pos, blksize, s)
    kc = np.arange(blksize, dtype=np.float64) * step
    iE = np.ceil((rem_code - spc) + kc).astype(np.int64)                          # tcode2 - 1
    iL = np.ceil((rem_code + spc) + kc).astype(np.int64)
    tP = rem_code + kc
    iP = np.ceil(tP).astype(np.int64)
    rem_code_n = (tP[-1] + step) - s["codeLength"]                                # :319
    time = np.arange(blksize + 1, dtype=np.float64) / fs                          # :322
    trig = ((carr_freq * 2.0 * np.pi) * time) + rem_carr                          # :325
    last = trig[blksize]
    rem_carr_n = last - math.trunc(last / (2 * np.pi)) * (2 * np.pi)              # :326-327
    bb = np.exp(1j * trig[:blksize]) * raw
    qb, ib = bb.real, bb.imag                                                     # :335-336
    sums = np.array([np.sum(prow[iE] * ib), np.sum(prow[iP] * ib), np.sum(prow[iL] * ib),
                     np.sum(prow[iE] * qb), np.sum(prow[iP] * qb), np.sum(prow[iL] * qb),
                     np.sum(drow[iE] * ib), np.sum(drow[iP] * ib), np.sum(drow[iL] * ib),
                     np.sum(drow[iE] * qb), np.sum(drow[iP] * qb), np.sum(drow[iL] * qb)])
    return 0, blksize, (sums, pos + blksize, rem_code_n, rem_carr_n)


class Loop:
    """Per-channel loop state (:184-208) and the update after one epoch's sums (:353-408)."""

    def __init__(self, s, pos, acquired_freq):
        self.s = s
        self.tau1, self.tau2 = calc_loop_coef(s["dllNoiseBandwidth"], s["dllDampingRatio"], 1.0)
        self.k1, self.k2, self.k3 = calc_fll_pll_loop_coef(s["pllNoiseBandwidth"],
                                                           s["fllNoiseBandwidth"], 0.001)
        self.pos = pos
        self.code_freq = s["codeFreqBasis"] + \
            ((acquired_freq - s["IF"]) / (s["GLONASS_nominal_freq"] / s["codeFreqBasis"])) * 0
        self.rem_code = self.rem_carr = 0.0
        self.carr_freq = self.carr_basis = acquired_freq
        self.old_code_nco = self.old_code_err = 0.0
        self.old_carr_nco = self.old_carr_err = 0.0
        self.I1 = self.Q1 = 0.001

    def blksize(self):
        step = self.code_freq / self.s["samplingFreq"]
        return int(math.ceil((self.s["codeLength"] - self.rem_code) / step)), step

    def advance(self, blk, step):
        """Carry-over without a record (replay): :319, :322-327."""
        self.rem_code = ((self.rem_code + float(blk - 1) * step) + step) - self.s["codeLength"]
        last = ((self.carr_freq * 2.0 * np.pi) * (float(blk) / self.s["samplingFreq"])) + \
            self.rem_carr
        self.rem_carr = last - math.trunc(last / (2 * np.pi)) * (2 * np.pi)
        self.pos += blk

    def update(self, sums):
        """:353-408 on one epoch's sums; returns the record values in FIELDS order."""
        s = self.s
        v = [float(x) for x in sums]
        I_P, Q_P = v[1], v[4]
        I_E2, I_P2, I_L2, Q_E2, Q_P2, Q_L2 = v[6:]
        I2, Q2 = self.I1, self.Q1                                                 # :354
        self.I1, self.Q1 = I_P2, Q_P2                                             # :355
        cross = self.I1 * Q2 - I2 * self.Q1
        dot = abs(self.I1 * I2 + self.Q1 * Q2)
        freq_err = math.atan2(cross, dot) / math.pi                               # :362
        carr_err = math.atan(Q_P / I_P) / (2.0 * math.pi)                         # :365
        carr_nco = self.old_carr_nco + self.k1 * carr_err - self.k2 * self.old_carr_err + \
            self.k3 * freq_err                                                    # :368
        self.old_carr_nco, self.old_carr_err = carr_nco, carr_err
        self.carr_freq = self.carr_basis + carr_nco
        cE = math.sqrt(I_E2 * I_E2 + Q_E2 * Q_E2)
        cL = math.sqrt(I_L2 * I_L2 + Q_L2 * Q_L2)
        code_err = (cE - cL) / (cE + cL)                                          # :378-381
        code_nco = self.old_code_nco + (self.tau2 / self.tau1) * (code_err - self.old_code_err) + \
            code_err * (0.001 / self.tau1)                                        # :384-385
        self.old_code_nco, self.old_code_err = code_nco, code_err
        self.code_freq = s["codeFreqBasis"] - code_nco + \
            ((self.carr_freq - s["IF"]) / (s["GLONASS_nominal_freq"] / s["codeFreqBasis"]))
        abs_sample = self.pos - self.rem_code * (s["samplingFreq"] / 1000) / s["codeLength"]
        return tuple(v) + (self.carr_freq, self.code_freq, abs_sample, code_err, code_nco,
                           carr_err, carr_nco)


def track(IF, s, prn, code_phase_1b, acquired_freq, n_ms, skip=0, perturb=None):
    """tracking.sci's per-channel loop for n_ms epochs.  Returns a dict of FIELDS arrays
    (length = epochs processed) + 'blksize', 'status' (0 or 1) and 'stop_blksize'.
    perturb: optional [12] relative offsets applied to every epoch's sums before the loop
    filters (the decidability check of the closed-loop scene)."""
    prow, drow = padded(generate_code(prn)), padded(generate_code(prn + 32))
    lp = Loop(s, skip + code_phase_1b - 1, acquired_freq)

    def epoch(lp):
        st, blk, r = correlate(IF, s, prow, drow, lp.pos, lp.rem_code, lp.rem_carr, lp.code_freq,
                               lp.carr_freq)
        if st:
            return st, blk, None
        sums, lp.pos, lp.rem_code, lp.rem_carr = r
        return 0, blk, sums
    res, res["status"], res["stop_blksize"] = T.track(lp, FIELDS, n_ms, epoch, perturb)
    return res


def replay(sums, s, code_phase_1b, acquired_freq, skip=0):
    """The loop half driven by given per-epoch sums [n, 12] (SUMS order)."""
    return T.replay(Loop(s, skip + code_phase_1b - 1, acquired_freq), FIELDS, sums)


# ---- scenes ---------------------------------------------------------------------------
def synth_l3(n, prn, start, doppler, fs=24e6, IF=-2.025e6, amp=12.0, phase=0.0, noise=6.0,
             seed=0, pilot=True, data=True, symbols_seed=1):
    """int8 interleaved I,Q of n samples of a continuous L3OC signal in the manner of the
    reference's simulator (glonass_l3_generator.sce): with t the time since `start` (a
    sample position, may be fractional) the code phase is t * (10.23e6 + doppler/117.5)
    chips, the pilot is code(prn) times the 10-symbol 1 kHz overlay NH, the data channel
    code(prn + 32) times the 5-symbol 1 kHz Barker overlay times seeded +-1 symbols of
    5 ms; the two ride in quadrature on one carrier,
      x = amp * exp(-i (2 pi (IF + doppler) t_abs + phase)) * ((-1 + i) pilot + (1 + i) data)/sqrt 2
    (the simulator's I/Q formula, so the tracker's wipe-off exp(+i ...) stops it), plus
    seeded Gaussian noise of sigma `noise` per component, rounded and clipped to int8."""
    rng = np.random.default_rng(seed)
    idx = np.arange(n, dtype=np.float64)
    x = noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    rate = 10.23e6 + doppler / 117.5
    ph = ((idx - start) / fs) * rate                        # chips since the code began
    chip = np.floor(ph).astype(np.int64)
    ms = np.floor_divide(chip, 10230)
    chip = chip % 10230
    sym = 2 * np.random.default_rng(symbols_seed).integers(0, 2, 64) - 1
    sI = generate_code(prn)[chip] * NH[ms % 10] if pilot else 0.0
    sQ = generate_code(prn + 32)[chip] * BARKER[ms % 5] * sym[np.floor_divide(ms, 5) % 64] \
        if data else 0.0
    arg = 2.0 * np.pi * (IF + doppler) * (idx / fs) + phase
    x += amp * np.exp(-1j * arg) * ((-1 + 1j) * sI + (1 + 1j) * sQ) / math.sqrt(2)
    out = np.empty(2 * n, np.int8)
    out[0::2] = np.clip(np.rint(x.real), -127, 127)
    out[1::2] = np.clip(np.rint(x.imag), -127, 127)
    return out


# The closed-loop scene of the CPU and GPU tiers: PRN 30 (the simulator's and
# initSettings.sci's satellite) on a 26 ms record.  Seed, phase and acquisition offset are
# chosen so that the decidability condition of tests/test_l3_cpu.py holds; keep them.
SCENE_PRN = 30
SCENE_MS = 20
SCENE = dict(start=3000.6, doppler=1800.0, acq_err=-14.0, phase=0.7, seed=4)


@functools.lru_cache(maxsize=None)
def closed_loop_scene(fs=24e6):
    """(IF int8, prn, code_phase_1b, acquired_freq, planted code rate).  The channel starts
    on the first whole sample of a code period."""
    s = settings(samplingFreq=fs)
    n = int(fs * (SCENE_MS + 6) / 1000)
    IF = synth_l3(n, SCENE_PRN, SCENE["start"], SCENE["doppler"], fs=fs, IF=s["IF"],
                  phase=SCENE["phase"], seed=SCENE["seed"])
    IF.setflags(write=False)
    return (IF, SCENE_PRN, int(math.ceil(SCENE["start"])) + 1,
            s["IF"] + SCENE["doppler"] + SCENE["acq_err"], 10.23e6 + SCENE["doppler"] / 117.5)


# The search scene: the same satellite with the data-channel overlay period (5 ms, one data
# symbol) starting at sample ACQ_START, Doppler on a bin of the 100 Hz grid.
ACQ_START = 31234
ACQ_DOPPLER = 1300.0


@functools.lru_cache(maxsize=None)
def search_scene(fs=24e6):
    """(IF int8 of 22 ms, prn): 10 ms for the search and 10 closed-loop epochs after it.
    The search answers one sample late, 0-based lag ACQ_START + 1: makeCaTable.sci:62
    takes sample n (1-based) of the replica at time n * ts, not (n - 1) * ts.  The carrier
    phase at that sample is pi/4, which puts the pilot on the I arm of a channel that
    starts there with remCarrPhase 0 on the true frequency: the loop starts in lock (its
    pull-in from elsewhere takes some 60 ms)."""
    s = settings(samplingFreq=fs)
    n = int(fs * 0.022)
    phase = math.pi / 4 - 2.0 * math.pi * (s["IF"] + ACQ_DOPPLER) * ((ACQ_START + 1) / fs)
    IF = synth_l3(n, SCENE_PRN, float(ACQ_START), ACQ_DOPPLER, fs=fs, IF=s["IF"], phase=phase,
                  seed=9)
    IF.setflags(write=False)
    return IF, SCENE_PRN


synth_if = E1B.synth_if
