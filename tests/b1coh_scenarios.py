"""COMPASS B1 coherent searches: fp64 numpy restatement of acquisition_7x3ms.sci and
acquisition_4x5ms.sci, and the small planted scenes of the CPU and GPU tiers.

TEST INFRASTRUCTURE ONLY (no GPU).  Restates COMPASS/B1/acquisition_7x3ms.sci:45-199
(acquisition_4x5ms.sci differs in its constants only: 5 code periods per segment, 4
segments, bins of 100 Hz); S = samplesPerCode, c = 3 or 5, M = c S:

  :52-58    segment k (0-based) is longSignal(k M + 1 : (k + 2) M): 2 M samples, M after
            the previous one
  :64       phasePoints over 2 M samples: the carrier restarts at 0 in every segment
  :67       round(band * 2 * c) + 1 bins, :103-105 in steps of 1000 / (2 c) Hz
  :95-97    conj(fft([-code ... -code (c times) zeros(1, M)])): the first c
            Neumann-Hoffman bits are 0, so every period carries the sign -1
  :112-136  |ifft(fft(exp(i f phasePoints) .* segment) .* replica)|^2
  :139-145  the row of one bin is [acqRes1(1:M) ... acqResK(1:M)]
  :154      frequencyBinIndex: the first maximum of the row maxima
  :157      codePhase: the first maximum of the column maxima, 1-based in 1 .. K M
  :159-176  codePhaseRange written on samplesPerCode, 1-based, as the file has it
  :179      secondPeakSize over results(frequencyBinIndex, codePhaseRange)
  :188      codePhase stored as found, not reduced to one code period

`search` is that computation at any shape (the small scenes, group tables as the
library takes them, either second-peak rule) in the result layout of
test_acq_gpu.check_rows; `acquire` is the receiver's call on b1i_scenarios.scene() with
the decision margins of b1i_scenarios.acquire.  Assumptions as in oracle/sgt_oracle.py;
an index of codePhaseRange past the row's end is dropped (it cannot occur: S <= K M).
"""
import functools

import numpy as np

import b1i_scenarios as B
import e1b_scenarios as E
from ftrack_oracle import code_phase_range_1b

MODES = {3: dict(coh=3, segments=7), 5: dict(coh=5, segments=4)}


# ---- acquisition_7x3ms.sci:159-176 (codePhaseRange: ftrack_oracle.code_phase_range_1b) --
def second_candidates(row_len, argmax0, spc, period):
    """0-based candidate lags of `second` in a row of row_len lags: the range of :159-176
    written on `period`, or (period 0) outside the open window circular in the row."""
    if period:
        rng = code_phase_range_1b(argmax0 + 1, period, spc)
        return rng[rng <= row_len] - 1
    d = (np.arange(row_len) - argmax0) % row_len
    return np.flatnonzero((d >= spc) & (d <= row_len - spc))


def straddles(argmax0, spc, period, M):
    """The :159-176 range of this peak holds lags of two segments."""
    rng = code_phase_range_1b(argmax0 + 1, period, spc) - 1
    return bool(rng.min() // M != rng.max() // M)


# ---- :52-145 ---------------------------------------------------------------------------
def concat_rows(sig, fs, freqs, cfs, M, segments):
    """results(frqBinIndex, :) of every replica for every frequency:
    [n_replicas, n_freqs, segments * M].  sig: the complex record, cfs: the replicas'
    conjugate spectra (2 M points each).  The segments' spectra do not depend on the PRN
    (:112-118 sit inside the PRN loop), so each is formed once."""
    L = 2 * M
    phase_points = np.arange(L) * 2 * np.pi * (1.0 / fs)                         # :64
    segs = np.stack([sig[k * M:k * M + L] for k in range(segments)])              # :52-58
    out = np.empty((len(cfs), len(freqs), segments * M))
    for i, f in enumerate(freqs):
        X = np.fft.fft(np.exp(1j * f * phase_points) * segs, axis=1)              # :107-118
        for j, cf in enumerate(cfs):
            acq = np.abs(np.fft.ifft(X * cf, axis=1)) ** 2                        # :121-136
            out[j, i] = acq[:, :M].reshape(-1)                                    # :139-145
    return out


def search(IF, fs, codes, L, n_blocks, freqs, group_freq, group_code=None, spc=8, period=0):
    """codes: (n_codes, M = L / 2) replicas as uploaded (signs included).  Returns
    (results, rows) shaped like acq_oracle.acquire(..., return_rows=True): per group
    dict(peak, second, metric, bin, code_phase, carr_freq, results) and per (group, bin)
    dict(peak, argmax, block, second), all on the concatenated row of n_blocks * M lags."""
    codes = np.asarray(codes, np.float64)
    M = L // 2
    assert codes.shape[1] == M
    group_freq = np.asarray(group_freq)
    G, nb = group_freq.shape
    if group_code is None:
        group_code = np.arange(G)
    x = np.asarray(IF, np.float64)
    sig = x[0::2] + 1j * x[1::2]
    n = n_blocks * M
    used = sorted(set(int(v) for v in group_freq.ravel()))
    ucodes = sorted(set(int(v) for v in group_code))
    cfs = [np.conj(np.fft.fft(np.concatenate([codes[k], np.zeros(M)]))) for k in ucodes]   # :95-97
    allrows = concat_rows(sig, fs, [freqs[i] for i in used], cfs, M, n_blocks)
    out, rows_out = [], []
    for g in range(G):
        mine = allrows[ucodes.index(int(group_code[g]))]
        results = mine[[used.index(int(fi)) for fi in group_freq[g]]]
        rows = []
        for b in range(nb):
            am = int(np.argmax(results[b]))
            rows.append(dict(peak=results[b].max(), argmax=am, block=am // M,
                             second=float(results[b][second_candidates(n, am, spc, period)].max())))
        row_max = results.max(axis=1)
        bin_idx = int(np.argmax(row_max))                                         # :154
        code_phase = int(np.argmax(results.max(axis=0))) + 1                      # :157
        second = float(results[bin_idx][second_candidates(n, code_phase - 1, spc, period)].max())
        out.append(dict(peak=row_max.max(), second=second, metric=row_max.max() / second,
                        bin=bin_idx, code_phase=code_phase,
                        carr_freq=float(freqs[group_freq[g, bin_idx]]), results=results))
        rows_out.append(rows)
    return out, rows_out


def assert_decidable(ref, ref_rows, spc, period, margin=1e-6):
    """Every row's peak is clear of every other lag, its `second` of every other candidate,
    and the winning bin of the others, by more than `margin` relative."""
    for g, rg in enumerate(ref):
        for b, rr in enumerate(ref_rows[g]):
            row = rg["results"][b]
            assert rr["peak"] > np.delete(row, rr["argmax"]).max() * (1 + margin), ("peak", g, b)
            v = np.sort(row[second_candidates(len(row), rr["argmax"], spc, period)])
            assert v[-1] == rr["second"] and v[-1] > v[-2] * (1 + margin), ("second", g, b)
        pk = np.sort(rg["results"].max(axis=1))
        if len(pk) > 1:
            assert pk[-1] > pk[-2] * (1 + margin), ("bin", g)


# ---- the receiver's call ---------------------------------------------------------------
def bins(s, coh, band_khz=14.0):
    """:67, :103-105."""
    nb = int(round(band_khz * 2 * coh)) + 1
    k = np.arange(1, nb + 1)
    return s["IF"] - (band_khz / 2) * 1000 + (1000 / (2 * coh)) * (k - 1)


def replica(s, prn, coh):
    """The coh code periods of :95-97, each times -1 (without the zeros)."""
    fs = s["samplingFreq"]
    spc_n = int(round(fs / (s["codeFreqBasis"] / s["codeLength"])))              # :48
    row = B.sample_code(B.generate_code(prn), s["codeFreqBasis"], fs, spc_n)
    return -np.tile(row, coh)


def _top2(v):
    p = np.partition(np.asarray(v).ravel(), -2)
    return float(p[-1]), float(p[-2])


def acquire(IF, s, prns, mode, band_khz=14.0):
    """acquisition_7x3ms.sci (mode 3) or acquisition_4x5ms.sci (mode 5) per PRN: bin
    (0-based), code_phase (1-based, concatenated), segment, peak, second, metric,
    carr_freq, margins (peak / bin / second-peak decisions against their runners-up,
    relative, as b1i_scenarios.acquire) and whether the second-peak range straddles a
    segment boundary."""
    coh, segments = MODES[mode]["coh"], MODES[mode]["segments"]
    fs = s["samplingFreq"]
    S = int(round(fs / (s["codeFreqBasis"] / s["codeLength"])))
    M = coh * S
    chip = int(round(fs / s["codeFreqBasis"]))                                   # :160-161
    frq = bins(s, coh, band_khz)
    gf = np.tile(np.arange(len(frq)), (len(prns), 1))
    ref, _ = search(IF, fs, np.stack([replica(s, p, coh) for p in prns]), 2 * M, segments, frq,
                    gf, spc=chip, period=S)
    out = []
    for r in ref:
        results = r.pop("results")
        a = r["code_phase"] - 1
        cand = results[r["bin"]][second_candidates(segments * M, a, chip, S)]
        pk, pk2 = _top2(results)
        rm, rm2 = _top2(results.max(axis=1))
        sc, sc2 = _top2(cand)
        assert pk == r["peak"] and sc == r["second"]
        r.update(segment=a // M, straddles=straddles(a, chip, S, M),
                 margins=(pk / pk2 - 1.0, rm / rm2 - 1.0, sc / sc2 - 1.0))
        out.append(r)
    return out


# ---- the small shape -------------------------------------------------------------------
FS = 2.0e6
S, M, L, NB = 200, 600, 1200, 7          # L = 2^4 * 3 * 5^2; the row is NB * M = 4200 lags
FREQS = np.array([-500.0, 0.0, 500.0])
GF = np.arange(3)[None, :]
N_REC = (NB - 1) * M + L                  # samples of the record


@functools.lru_cache(maxsize=None)
def code():
    """An aperiodic random +-1 code of M samples."""
    rng = np.random.default_rng(0xB1C0DE)
    c = (2 * rng.integers(0, 2, M) - 1).astype(np.int8)
    c.setflags(write=False)
    return c


def cases():
    """(a, s, edge): the peak's concatenated lag, spc, and the edge of the admitted range
    that carries the weakest copy ('lo' / 'hi'; alternating, and as the case is named:
    M + s puts the top edge a - s on the first lag of block 1, M + S - s - 1 and M + S - s
    the bottom edge a + s - S on the last lag of block 0 / the first of block 1)."""
    out = []
    for s in (2, 7):
        out += [(s, s, "lo"), (s + 1, s, "hi"), (S - s - 1, s, "lo"), (S - s, s, "hi"),
                (M - 1, s, "lo"), (M, s, "hi"), (M + s, s, "hi"), (M + S - s - 1, s, "lo"),
                (M + S - s, s, "lo"), (6 * M, s, "hi"), (7 * M - 1, s, "lo")]
    return out


def edge_lag(a, s, edge):
    """The named edge of the :159-176 range of peak a (0-based): its first / last lag; in
    the two-piece branch the lags next to the excluded chip, a + s and a - s."""
    rng = code_phase_range_1b(a + 1, S, s) - 1
    if s < a < S - s:
        return a + s if edge == "lo" else a - s
    return int(rng.min() if edge == "lo" else rng.max())


def decoy_lag(a):
    """One period from the peak: never in the :159-176 range, always outside the circular
    window."""
    return a - S if a >= S else a + S


def planted_if(parts):
    """Noise-free int8 I,Q record of N_REC samples: amp * code placed from sample p for
    every (amp, p); a copy placed from p correlates at concatenated lag p."""
    c = code().astype(np.int64)
    x = np.zeros(N_REC, np.int64)
    for amp, p in parts:
        assert 0 <= p and p + M <= N_REC
        x[p:p + M] += amp * c
    out = np.zeros(2 * N_REC, np.int8)
    out[0::2] = x
    return out


def scene_if(a, s, edge):
    """The peak (6) at a, the decoy (3) one period away, the weakest copy (2) on the edge."""
    return planted_if([(6, a), (3, decoy_lag(a)), (2, edge_lag(a, s, edge))])


_ref = {}


def reference(a, s, edge, period):
    """search() of one case under one rule, computed once."""
    key = (a, s, edge, period)
    if key not in _ref:
        _ref[key] = search(scene_if(a, s, edge), FS, code()[None, :], L, NB, FREQS, GF, spc=s,
                           period=period)
    return _ref[key]


# chunk scene: three copies on three frequencies a null of the 0.3 ms correlation apart
# (fs / M), in three different blocks; five groups of one code name them differently
CH_FREQS = np.array([-FS / M, 0.0, FS / M])
CH_PARTS = ((40.0, 700, 0), (30.0, 2500, 1), (20.0, 3700, 2))       # (amp, lag, frequency)
CH_GF = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [0, 1, 1], [1, 2, 2]])


def chunk_if():
    return E.synth_if(N_REC, [(code().astype(np.float64), amp, p, CH_FREQS[fi])
                              for amp, p, fi in CH_PARTS], FS, noise=0.0)
