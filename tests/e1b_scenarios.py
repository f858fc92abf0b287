"""Zero-padded long-code acquisition: fp64 numpy restatement and synthetic scenes.

TEST INFRASTRUCTURE ONLY.  Restates GALILEO/E1/acquisition.sci:45-165 line by line:

  :52,58   a block is L = 2 * samplesPerCode samples, phase points over L
  :88      E1BCodeFreqDom = conj(fft([code zeros(1, samplesPerCode)]))
  :99-109  |ifft(fft(exp(i f phasePoints) .* signal) .* E1BCodeFreqDom)|^2
  :112     the row keeps the first samplesPerCode lags (`keep` here)
  :121-124 peak / bin / code phase over the kept lags
  :129-145 second peak outside (codePhase - spc, codePhase + spc), the range wrapping
           at samplesPerCode; stated as the open circular window the project uses
           for the GPS / GLONASS searches (oracle/acq_oracle.py _second_peak),
           circular in keep

The reference searches one block; several blocks (best of blocks by the kept lags'
maximum, or the non-coherent sum of the kept lags) follow acq_oracle.acquire's rule.
Results and rows have the shape of acq_oracle.acquire(..., return_rows=True), so
test_acq_gpu.check_rows applies.  `full` holds the chosen block's complete L-lag
row of every (group, bin), for tests about the discarded lags.
"""
import numpy as np


def second_peak(row, argmax, spc):
    """Max outside the open window (argmax - spc, argmax + spc), circular in len(row)."""
    n = len(row)
    d = (np.arange(n) - argmax) % n
    return float(row[(d >= spc) & (d <= n - spc)].max())


def acquire(IF, fs, codes, L, keep, freqs, group_freq, group_code=None, spc=16, n_blocks=1,
            noncoherent=False):
    """codes: (n_codes, code_len <= L) +-1.  Returns (results, rows, full)."""
    codes = np.asarray(codes, np.float64)
    group_freq = np.asarray(group_freq)
    G, B = group_freq.shape
    if group_code is None:
        group_code = np.arange(G)
    x = np.asarray(IF, np.float64)
    sig = x[0::2] + 1j * x[1::2]
    phase_points = np.arange(L) * 2 * np.pi * (1.0 / fs)
    blocks = [sig[b * L:(b + 1) * L] for b in range(n_blocks)]
    spec = {}
    out, rows_out, full_out = [], [], []
    for g in range(G):
        padded = np.zeros(L)
        padded[:codes.shape[1]] = codes[group_code[g]]
        cf = np.conj(np.fft.fft(padded))
        results = np.zeros((B, keep))
        rows, fulls = [], []
        for b in range(B):
            fi = int(group_freq[g, b])
            if fi not in spec:
                sc = np.exp(1j * freqs[fi] * phase_points)
                spec[fi] = [np.fft.fft(sc * blk) for blk in blocks]
            full = [np.abs(np.fft.ifft(X * cf)) ** 2 for X in spec[fi]]
            acq = [a[:keep] for a in full]
            if noncoherent:
                results[b] = np.sum(acq, axis=0)
                chosen = 0
                fulls.append(np.sum(full, axis=0))
            else:
                chosen = 0
                for k in range(1, n_blocks):
                    if not (acq[chosen].max() > acq[k].max()):
                        chosen = k
                results[b] = acq[chosen]
                fulls.append(full[chosen])
            am = int(np.argmax(results[b]))
            rows.append(dict(peak=results[b].max(), argmax=am,
                             block=-1 if noncoherent else chosen,
                             second=second_peak(results[b], am, spc)))
        row_max = results.max(axis=1)
        bin_idx = int(np.argmax(row_max))
        code_phase = int(np.argmax(results.max(axis=0))) + 1
        second = second_peak(results[bin_idx], code_phase - 1, spc)
        out.append(dict(peak=row_max.max(), second=second, metric=row_max.max() / second,
                        bin=bin_idx, code_phase=code_phase,
                        carr_freq=float(freqs[group_freq[g, bin_idx]]), results=results))
        rows_out.append(rows)
        full_out.append(fulls)
    return out, rows_out, full_out


def assert_decidable(ref, ref_rows, spc, margin=1e-6):
    """Every row's peak exceeds every other kept lag, and its second peak every other
    value outside the exclusion window, by more than `margin` relative: neither the
    argmax nor `second` of a correct fp64 implementation can turn on rounding."""
    for g, rg in enumerate(ref):
        for b, rr in enumerate(ref_rows[g]):
            row = rg["results"][b]
            n = len(row)
            others = np.delete(row, rr["argmax"])
            assert rr["peak"] > others.max() * (1 + margin), ("peak", g, b)
            d = (np.arange(n) - rr["argmax"]) % n
            outside = np.sort(row[(d >= spc) & (d <= n - spc)])
            assert outside[-1] == rr["second"]
            assert outside[-1] > outside[-2] * (1 + margin), ("second", g, b)
        pk = np.sort(rg["results"].max(axis=1))
        if len(pk) > 1:
            assert pk[-1] > pk[-2] * (1 + margin), ("bin", g)


def synth_if(L_total, parts, fs, noise=3.0, seed=0):
    """int8 interleaved I,Q: the sum of parts (samples, amplitude, start, freq) --
    `samples` (+-1 array) placed from sample `start`, times amplitude *
    exp(-i 2 pi freq n / fs) (so the search's wipe-off exp(+i 2 pi f t) stops it at
    f = freq) -- plus seeded Gaussian noise of the given sigma per component, rounded
    and clipped to int8."""
    rng = np.random.default_rng(seed)
    n = np.arange(L_total)
    x = np.zeros(L_total, np.complex128)
    for samples, amp, start, freq in parts:
        s = np.zeros(L_total)
        m = min(len(samples), L_total - start)
        s[start:start + m] = samples[:m]
        x += amp * s * np.exp(-2j * np.pi * freq * n / fs)
    x += noise * (rng.standard_normal(L_total) + 1j * rng.standard_normal(L_total))
    out = np.empty(2 * L_total, np.int8)
    out[0::2] = np.clip(np.rint(x.real), -127, 127)
    out[1::2] = np.clip(np.rint(x.imag), -127, 127)
    return out


def sample_boc(chips, code_rate, fs, n):
    """makeE1BCodesTable.sci:56-78 in numpy (the test of gnsscorr_sample_boc_code)."""
    chips = np.asarray(chips)
    half = np.kron(chips, np.ones(2, chips.dtype))
    half[1::2] *= -1                                   # meandr(2:2:$) = -1
    ts, tc = 1.0 / fs, 1.0 / code_rate
    idx = np.ceil((ts * np.arange(1, n + 1)) / tc * 2).astype(np.int64)
    idx[-1] = len(chips)                               # codeValueIndex($) = codeLength
    return half[idx - 1]
