"""BeiDou B1I in the float tracker (system 2 of gnsscorr_sgt_*): restatements of the
COMPASS/B1 Scilab receiver and the synthetic scene the CPU and GPU tiers share.

  generate_code   COMPASS/B1/include/generateCAcode.sci:38-146, in the file's own +-1
                  register-product form (the library uses a bit form)
  settings        COMPASS/B1/initSettings.sci:64-101
  Loop / track    COMPASS/B1/tracking.sci:123-357: the correlator block is the generic
                  oracle/sgt_oracle.correlate; the loop update restates :291-344, which
                  differs from the GPS file in two places: the previous prompt pair is
                  negated when sign(I_P) changed (:295-298) and the carrier aiding of the
                  code NCO divides by 763 (:336)
  acquire         COMPASS/B1/acquisition.sci:86-168 (2 S samples against [code zeros],
                  the first S lags, second peak outside one chip of the peak)
  scene           continuous B1I signals with the 20-bit Neumann-Hoffman sequence of
                  acquisition.sci:89 on the code periods, AWGN, int8 I,Q
"""
import math

import numpy as np

import ftrack_oracle as T
import sgt_oracle as S

FIELDS = S.FIELDS
SUMS = FIELDS[:6]
N_PRN = 37
L_CODE = 2046
# acquisition.sci:89
NH = 1.0 - 2.0 * np.array([0, 0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 1, 0, 1, 0, 0, 1, 1, 1, 0], np.float64)
# generateCAcode.sci:63-136: the two G2 stages whose product is the G2 output
G2_TAPS = [(1, 3), (1, 4), (1, 5), (1, 6), (1, 8), (1, 9), (1, 10), (1, 11), (2, 7), (3, 4),
           (3, 5), (3, 6), (3, 8), (3, 9), (3, 10), (3, 11), (4, 5), (4, 6), (4, 8), (4, 9),
           (4, 10), (4, 11), (5, 6), (5, 8), (5, 9), (5, 10), (5, 11), (6, 8), (6, 9), (6, 10),
           (6, 11), (8, 9), (8, 10), (8, 11), (9, 10), (9, 11), (10, 11)]

_codes = {}


def generate_code(prn: int) -> np.ndarray:
    """generateCAcode.sci:38-146 as written: 1-based register entries, products."""
    if prn in _codes:
        return _codes[prn]
    a, b = G2_TAPS[prn - 1]
    g1 = np.zeros(L_CODE)
    reg = -1 * np.array([0, -1, 1, -1, 1, -1, 1, -1, 1, -1, 1, -1], np.int64)   # reg[1..11]
    for i in range(L_CODE):
        g1[i] = reg[11]
        save = reg[1] * reg[7] * reg[8] * reg[9] * reg[10] * reg[11]
        reg[2:12] = reg[1:11].copy()
        reg[1] = save
    g2 = np.zeros(L_CODE)
    reg2 = -1 * np.array([0, -1, 1, -1, 1, -1, 1, -1, 1, -1, 1, -1], np.int64)
    for i in range(L_CODE):
        g2[i] = reg2[a] * reg2[b]
        save = reg2[1] * reg2[2] * reg2[3] * reg2[4] * reg2[5] * reg2[8] * reg2[9] * reg2[11]
        reg2[2:12] = reg2[1:11].copy()
        reg2[1] = save
    _codes[prn] = -(g1 * g2)
    return _codes[prn]


def padded_code(prn: int) -> np.ndarray:
    """tracking.sci:140-142: [c(2046) c c(1)]."""
    c = generate_code(prn)
    return np.concatenate([c[-1:], c, c[:1]])


def sample_code(chips, code_rate, fs, n):
    """makeCaTable.sci:62-69."""
    ts, tc = 1.0 / fs, 1.0 / code_rate
    idx = np.ceil((ts * np.arange(1, n + 1)) / tc).astype(np.int64)
    idx[-1] = len(chips)
    return np.asarray(chips)[idx - 1]


def settings(**kw) -> dict:
    """initSettings.sci:64-101 in the key set sgt_oracle.correlate reads."""
    s = dict(system=2, samplingFreq=16e6, codeFreqBasis=2.046e6, codeLength=L_CODE, IF=0.098e6,
             L1_IF_step=0.0, GLONASS_zero_channel=0.0, dllCorrelatorSpacing=0.1,
             dllNoiseBandwidth=0.5, dllDampingRatio=0.7, pllNoiseBandwidth=25.0,
             fllNoiseBandwidth=250.0, fileType=2, switchIQ=0, codeNcoVariant=0,
             absSampleVariant=0)
    s.update(kw)
    return s


def _sign(x):
    return (x > 0) - (x < 0)


class Loop(S.Loop):
    """tracking.sci:144-169 initial values (those of the GPS file) and :291-344."""

    def update(self, sums):
        s = self.s
        I_E, I_P, I_L, Q_E, Q_P, Q_L = (float(x) for x in sums)
        I2, Q2 = self.I1, self.Q1                                    # :292-293
        self.I1, self.Q1 = I_P, Q_P
        if _sign(I2) != _sign(self.I1):                              # :295-298
            I2, Q2 = -I2, -Q2
        cross = self.I1 * Q2 - I2 * self.Q1
        dot = abs(self.I1 * I2 + self.Q1 * Q2)
        freq_err = math.atan2(cross, dot) / math.pi
        carr_err = math.atan(Q_P / I_P) / (2.0 * math.pi)
        carr_nco = self.old_carr_nco + self.k1 * carr_err - self.k2 * self.old_carr_err - \
            self.k3 * freq_err
        self.old_carr_nco, self.old_carr_err = carr_nco, carr_err
        self.carr_freq = self.carr_basis + carr_nco
        aE = math.sqrt(I_E * I_E + Q_E * Q_E)
        aL = math.sqrt(I_L * I_L + Q_L * Q_L)
        code_err = (aE - aL) / (aE + aL)
        code_nco = self.old_code_nco + (self.tau2 / self.tau1) * (code_err - self.old_code_err) + \
            code_err * (0.001 / self.tau1)
        self.old_code_nco, self.old_code_err = code_nco, code_err
        if s["codeNcoVariant"] == 1:
            self.code_freq = s["codeFreqBasis"] - code_nco
        else:
            self.code_freq = s["codeFreqBasis"] - code_nco + ((self.carr_freq - s["IF"]) / 763)   # :336
        if s["absSampleVariant"] == 1:
            abs_sample = float(self.pos)
        else:                                                        # :342-344
            abs_sample = self.pos - self.rem_code * (s["samplingFreq"] / 1000) / s["codeLength"]
        return (I_E, I_P, I_L, Q_E, Q_P, Q_L, self.carr_freq, self.code_freq, abs_sample,
                code_err, code_nco, carr_err, carr_nco)


def track(IF, s, prn, code_phase_1b, acquired_freq, n_ms, skip=0, perturb=None):
    """The per-channel loop for n_ms epochs; stops as tracking.sci:236-240 when the
    record runs out (`stop_blksize` then holds the blksize that did not fit).  perturb:
    six relative offsets applied to the sums before the loop sees them."""
    pad = padded_code(prn)
    lp = Loop(s, prn, skip + code_phase_1b - 1, acquired_freq)
    res, status, stop = T.track(lp, FIELDS, n_ms, lambda lp: S.epoch(IF, s, pad, lp), perturb)
    res["stop_blksize"] = stop if status else None
    return res


def replay(sums, s, prn, code_phase_1b, acquired_freq, skip=0):
    """The loop half on given sums [n, 6] (as sgt_oracle.replay, with this file's Loop)."""
    return T.replay(Loop(s, prn, skip + code_phase_1b - 1, acquired_freq), FIELDS, sums)


# ---- acquisition.sci:86-168 ------------------------------------------------------------
def bins(s, band_khz=14.0):
    """:62, :96-98: round(band * 2) + 1 bins of 500 Hz from IF - band/2 kHz."""
    nb = int(round(band_khz * 2 * 1)) + 1
    k = np.arange(1, nb + 1)
    return s["IF"] - (band_khz / 2) * 1000 + (1000 / (2 * 1)) * (k - 1)


def acquire(IF, s, prns, band_khz=14.0):
    """One dict per PRN: bin (0-based), code_phase (1-based), peak, second, metric,
    carr_freq, and margins (how far the peak / bin / second-peak decisions are from
    their runners-up, relative)."""
    fs = s["samplingFreq"]
    spc_n = int(round(fs / (s["codeFreqBasis"] / s["codeLength"])))          # :48
    x = np.asarray(IF[:4 * spc_n], np.float64)
    signal1 = x[0::2] + 1j * x[1::2]
    phase_points = np.arange(2 * spc_n) * 2 * np.pi * (1.0 / fs)
    frq = bins(s, band_khz)
    spectra = [np.fft.fft(np.exp(1j * f * phase_points) * signal1) for f in frq]
    chip = int(round(fs / s["codeFreqBasis"]))                               # :131
    out = []
    for prn in prns:
        row = sample_code(generate_code(prn), s["codeFreqBasis"], fs, spc_n)
        cf = np.conj(np.fft.fft(np.concatenate([row, np.zeros(spc_n)])))
        results = np.stack([(np.abs(np.fft.ifft(X * cf)) ** 2)[:spc_n] for X in spectra])
        row_max = results.max(axis=1)
        b = int(np.argmax(row_max))                                          # :125
        cp = int(np.argmax(results.max(axis=0))) + 1                         # :128
        i1, i2 = cp - chip, cp + chip                                        # :133-147, 1-based
        if i1 < 2:
            rng = np.arange(i2, spc_n + i1 + 1)
        elif i2 > spc_n:
            rng = np.arange(i2 - spc_n, i1 + 1)
        else:
            rng = np.concatenate([np.arange(1, i1 + 1), np.arange(i2, spc_n + 1)])
        outside = np.sort(results[b, rng - 1])
        peak = float(row_max[b])
        others = np.sort(results.ravel())
        rm = np.sort(row_max)
        out.append(dict(bin=b, code_phase=cp, peak=peak, second=float(outside[-1]),
                        metric=peak / float(outside[-1]), carr_freq=float(frq[b]),
                        margins=(peak / others[-2] - 1.0, rm[-1] / rm[-2] - 1.0,
                                 outside[-1] / outside[-2] - 1.0)))
    return out


# ---- the scene -------------------------------------------------------------------------
SCENE_SEED = 22
SCENE_MS = 40
SCENE_CN0 = 50.0
RF = 1561.098e6


def scene(fs=16e6, n_ms=SCENE_MS + 3, seed=SCENE_SEED, cn0=SCENE_CN0, if_freq=0.098e6):
    """(IF int8 interleaved I,Q, chans): four continuous B1I signals.  chans: one
    (prn, start_1b, doppler, code_rate) per signal; start_1b is the 1-based sample of
    the first whole code period.  Code rate 2.046e6 (1 + fd / 1561.098e6), carrier at
    -(IF + fd) (the receiver's wipe-off is exp(+i 2 pi f t)), every code period times
    the Neumann-Hoffman sequence, complex unit-variance noise per component, the sum
    scaled by 24 and rounded to int8."""
    rng = np.random.default_rng(seed)
    prns = [6, 11, 23, 37]
    n = int(fs * n_ms / 1000)
    t = np.arange(n) / fs
    x = np.zeros(n, np.complex128)
    chans = []
    for prn in prns:
        cp = rng.uniform(100, L_CODE - 100)          # code phase [chips] at sample 0
        fd = 500.0 * int(rng.integers(-6, 7)) + rng.uniform(-8, 8)   # near a search bin
        ph0 = rng.uniform(0, 2 * np.pi)
        nh0 = int(rng.integers(0, 20))
        rate = 2.046e6 * (1 + fd / RF)
        chips = cp + t * rate
        per = np.floor(chips / L_CODE)
        ci = (chips - per * L_CODE).astype(np.int64) % L_CODE
        v = generate_code(prn)[ci] * NH[(per.astype(np.int64) + nh0) % 20]
        amp = math.sqrt(10.0 ** (cn0 / 10.0) * 2.0 / fs)
        x += amp * v * np.exp(-1j * (2 * np.pi * (if_freq + fd) * t + ph0))
        start = int(round((L_CODE - cp) / rate * fs)) + 1
        chans.append((prn, start, fd, rate))
    x += rng.standard_normal(n) + 1j * rng.standard_normal(n)
    IF = np.empty(2 * n, np.int8)
    IF[0::2] = np.clip(np.rint(24 * x.real), -127, 127)
    IF[1::2] = np.clip(np.rint(24 * x.imag), -127, 127)
    return IF, chans


def scene_acq_freq(chan, if_freq=0.098e6):
    """The acquired frequency handed to the closed-loop tests: the planted carrier plus a
    fixed 9 Hz acquisition error."""
    return if_freq + chan[2] + 9.0
