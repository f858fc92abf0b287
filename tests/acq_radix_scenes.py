"""The per-radix tier of the generic fp64 acquisition engine (csrc/acq64_gen.hip mx_pass):
the lengths, the scenes and the references that tests/test_acq_mixplan_cpu.py and
tests/test_acq_radix_gpu.py share.

TEST INFRASTRUCTURE ONLY.  The lengths are chosen so that every compiled radix runs as a
first, a middle and a last pass; TABLE records the pass orders the lengths were picked
for.  It is only what the test ids are made of and what the coverage is counted over:
test_acq_mixplan_cpu.py holds it to the library's own gnsscorr_acq_mix_plan, and no test
restates the ordering rule.

A scene at length N: fs = 1000 N Hz (a 1 ms code period), two seeded +-1 codes of N
chips, two blocks of int8 IQ noise with code 0 planted periodically (block 1 stronger),
and the seven bins 4000 + 500 k Hz, k = -3 .. 3.  The bins are N-independent multiples
(8 + k) / 2 of the 1000 Hz spectral line spacing: two residue classes, spectrum shifts
2 .. 5, and a wipe-off argument 2 pi (8 + k) n / (2 N) below 35 rad, whose own fp64
rounding stays near 1e-15.
"""
import functools

import numpy as np

import acq_oracle as A
import e1b_scenarios as E

# N -> (unpadded pass order, zero-padded pass order)
TABLE = {
    77: ((7, 11), (7, 11)),
    88: ((8, 11), (11, 8)),
    171: ((3, 19, 3), (3, 19, 3)),
    221: ((13, 17), (13, 17)),
    256: ((16, 16), (16, 16)),
    264: ((3, 11, 8), (3, 11, 8)),
    276: ((3, 23, 4), (3, 23, 4)),
    280: ((5, 8, 7), (5, 7, 8)),
    323: ((17, 19), (17, 19)),
    435: ((3, 29, 5), (3, 29, 5)),
    437: ((19, 23), (19, 23)),
    540: ((3, 3, 4, 5, 3), (3, 3, 3, 5, 4)),
    651: ((3, 31, 7), (3, 31, 7)),
    667: ((23, 29), (23, 29)),
    770: ((2, 7, 11, 5), (5, 7, 11, 2)),
    899: ((29, 31), (29, 31)),
    961: ((31, 31), (31, 31)),
    1088: ((4, 17, 16), (16, 17, 4)),
    1232: ((7, 16, 11), (7, 11, 16)),
    1859: ((11, 13, 13), (11, 13, 13)),
}
LENGTHS = tuple(TABLE)
RADICES = (2, 3, 4, 5, 7, 8, 11, 13, 16, 17, 19, 23, 29, 31)   # mx_pass is compiled for these

K_BINS = np.arange(-3, 4)
BINS = 4000.0 + 500.0 * K_BINS
PLANTED = 4                       # bin index of the planted code: k = +1, 4500 Hz
ROW_BINS = (1, 6, PLANTED)        # power rows: 3000 Hz (class 0), 5500 Hz (class 500), planted


def case_id(n):
    return f"{n}-" + "x".join(str(r) for r in TABLE[n][0])


def padded_id(n):
    return f"{n}-" + "x".join(str(r) for r in TABLE[n][1])


def fs_of(n):
    return 1000.0 * n


def codes_of(n, count=2):
    rng = np.random.default_rng(0xC0DE00 + n)
    return rng.choice(np.array([-1, 1], np.int8), (count, n))


@functools.lru_cache(maxsize=None)
def scene(n):
    """(codes (2, N) int8, IF of two blocks, int8 interleaved I,Q): code 0 periodic with
    its period starting at lag N // 3, on the planted bin, 4/3 as strong in block 1."""
    codes = codes_of(n)
    lag = n // 3
    x = np.tile(codes[0], 3)[n - lag:3 * n - lag].astype(np.float64)
    x[n:] *= 4.0 / 3.0
    IF = E.synth_if(2 * n, [(x, 3.0, 0, BINS[PLANTED])], fs_of(n), noise=3.0, seed=0x5CE0 + n)
    IF.setflags(write=False)
    codes.setflags(write=False)
    return codes, IF


@functools.lru_cache(maxsize=None)
def oracle_rows(n, code, bin_idx):
    """acq_oracle.power_rows of the scene: (2 blocks, N), read-only."""
    codes, IF = scene(n)
    ref = A.power_rows(IF, fs_of(n), codes[code], BINS[bin_idx])
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def padded_scene(n, keep):
    """(codes (2, keep), IF of two blocks) of a zero-padded search at L = N: code 0 at lag
    keep // 3 of both blocks (stronger in the second) on the planted bin, code 1 at lag
    keep - 3 of the first block on bin 2 (tests/test_acq_padded_gpu.py test_parity_small)."""
    codes = codes_of(n)[:, :keep].copy()
    lag = keep // 3
    parts = [(codes[0], 3.0, lag, BINS[PLANTED]), (codes[0], 4.0, n + lag, BINS[PLANTED]),
             (codes[1], 3.5, keep - 3, BINS[2])]
    IF = E.synth_if(2 * n, parts, fs_of(n), noise=3.0, seed=0x9AD0 + n + keep)
    IF.setflags(write=False)
    codes.setflags(write=False)
    return codes, IF


def keeps_of(n):
    """The kept lags of the zero-padded cases: N/2 for an even N (the half last pass where
    the padded order ends on an even radix), and the odd floor(3N/8) | 1 (the bounded one)."""
    odd = (3 * n // 8) | 1
    return ([n // 2] if n % 2 == 0 else []) + [odd]


# ---- the long-double reference of the power rows (the floor of acq_oracle.power_rows) ----
def _unit_roots(m, sign):
    """exp(sign 2 pi i j / m), j < m, in long double."""
    ld = np.longdouble
    a = (8 * np.arctan(ld(1))) * np.arange(m, dtype=ld) / ld(m)
    return np.cos(a) + sign * 1j * np.sin(a)


def power_rows_longdouble(n, code, bins):
    """The chain of acq_oracle.power_rows in long double with direct O(N^2) DFTs:
    |idft(dft(exp(i 2 pi f t) sig) conj(dft(code)))|^2 for the bins (indices into BINS)
    and both blocks of scene(n): (len(bins), 2, N).  The wipe-off phase is exact:
    f / fs = (8 + k) / (2 N), so sample t turns by the ((8 + k) t mod 2 N)-th of the
    2 N-th roots of unity."""
    codes, IF = scene(n)
    x = IF.astype(np.longdouble)
    sig = (x[0::2] + 1j * x[1::2]).reshape(2, n)
    t = np.arange(n, dtype=np.int64)
    w2 = _unit_roots(2 * n, +1)
    rows = np.concatenate([sig * w2[((8 + int(K_BINS[b])) * t) % (2 * n)] for b in bins])
    W = _unit_roots(n, -1)[np.outer(t, t) % n]              # W[k, t] = exp(-2 pi i k t / N)
    cf = np.conj(codes[code].astype(np.longdouble) @ W)     # W is symmetric
    y = (((rows @ W) * cf) @ np.conj(W)) / np.longdouble(n)
    return (y.real * y.real + y.imag * y.imag).reshape(len(bins), 2, n)
