"""Multi-ms coherent acquisition scenes (gnsscorr_acq_set_coherent), pure numpy.

TEST INFRASTRUCTURE ONLY (no GPU).  Every engine folds `coh` code periods of a block
into one N-point row, x[n] = sum_{p<coh} IF[b*coh*N + n + p*N] exp(i f (n + p*N) 2 pi ts)
(GLONASS/L1/acquisition.sci:52-72, 113-135 through oracle/acq_oracle.py acquire(coh=)).
The scenes are built so that each way of getting that fold wrong changes the signal row:

  carrier   the planted signal lies exactly on searched bin SIG_BIN, whose frequency is
            a whole kHz plus 500 Hz (coh = 2) or 250 Hz (coh = 3, 5): a phase ramp
            restarted every code period then adds the periods with phases
            exp(2 pi i p frac) and cancels (coh = 2) or keeps 1 / coh^2 of the power;
  blocks    the blocks carry the signal at amplitudes 1 : 2 (: 3), so best-of-blocks
            must report block 1 and a block read from b*N instead of b*coh*N mixes
            periods of two amplitudes;
  periods   one code phase and no data-bit flip inside a record;
  bins      the table also holds SIG_BIN + fs/N and + 2 fs/N, the same wipe-off class
            as the signal bin, so the class shift runs; the other four bins step by
            the receiver's 1000 / (2 coh) Hz;
  codes     group 0 searches a PRN that is absent, group 1 the planted one;
  records   the records scene plants one code phase per record.

The IF is replica x carrier + seeded Gaussian noise (sigma = 2 per component), quantised
to the four levels of the 2-bit packing (+-1, +-3; threshold 2), so one scene serves the
int8 and the gpu.pack2 searches.  The real-IF variant is the same with cos for exp, at
an IF inside Nyquist.
"""
import functools
from typing import NamedTuple

import numpy as np

import acq_oracle as A

SEED = 0x5EED0C00
PRN_ABSENT, PRN_SIGNAL = 11, 19
SIG_GROUP = 1            # group 0 is the absent code
SIG_BIN = 2
N_BINS = 7
AMP = 0.5                # block 0; noise sigma 2 per component
BLOCK_AMPS = (1.0, 2.0, 3.0)
SIGMA = 2.0
COHS = (2, 3, 5)
MODES = ("best", "noncoherent")

# if0: a whole kHz, inside Nyquist of the real-IF variant too
ENGINES = {
    "f64-16368": dict(fs=16.368e6, n=16368, if0=2.42e6),
    "f32-16368": dict(fs=16.368e6, n=16368, if0=2.42e6, f32=True),
    "f64-16000": dict(fs=16.0e6, n=16000, if0=2.42e6),
    "mixed-5000": dict(fs=5.0e6, n=5000, if0=1.25e6),
    "bluestein-5000": dict(fs=5.0e6, n=5000, if0=1.25e6, env={"GNSSCORR_ACQ_BLUESTEIN": "1"}),
    "bluestein-4111": dict(fs=4.111e6, n=4111, if0=1.0e6),
    "m4-16368": dict(fs=16.368e6, n=16368, if0=2.42e6, env={"GNSSCORR_ACQ_GENERIC": "1"}),
    "passes-16368": dict(fs=16.368e6, n=16368, if0=2.42e6,
                         env={"GNSSCORR_ACQ_GENERIC": "1", "GNSSCORR_ACQ_MIX4": "0"}),
    "m4-38192": dict(fs=38.192e6, n=38192, if0=9.548e6, cohs=(2,)),
}
GENERIC = [e for e in ENGINES if not e.startswith("f")]
REAL_IF_ENGINES = ("f64-16368", "f32-16368", "mixed-5000", "bluestein-4111")
RECORD_ENGINES = ("mixed-5000", "m4-16368")
N_RECORDS = 3


class Scene(NamedTuple):
    fs: float
    n: int
    if0: float
    coh: int
    n_blocks: int
    iq: bool
    phases: tuple        # planted 0-based code phase (the row's argmax) of every record

    @property
    def spc(self):
        return int(round(self.fs / 1.023e6))

    @property
    def rec_samples(self):
        return self.n_blocks * self.coh * self.n


def n_blocks_of(mode):
    return 2 if mode == "best" else 3


def cohs(engine):
    return ENGINES[engine].get("cohs", COHS)


def scene(engine, coh, mode, iq=True, records=1):
    e = ENGINES[engine]
    n = e["n"]
    phases = tuple((3 * n // 7 + 1 + r * (n // 3 + 5)) % n for r in range(records))
    return Scene(e["fs"], n, e["if0"], coh, n_blocks_of(mode), iq, phases)


def search_cases(engine):
    return [(coh, mode) for coh in cohs(engine) for mode in MODES]


def sig_freq(sc):
    return sc.if0 + (500.0 if sc.coh == 2 else 250.0)


def freqs(sc):
    d = 1000.0 / (2 * sc.coh)
    delta = sc.fs / sc.n
    return sig_freq(sc) + np.array([-2 * d, -d, 0.0, d, 2 * d, delta, 2 * delta])


GF = np.tile(np.arange(N_BINS), (2, 1))
GCODE = np.arange(2)


@functools.lru_cache(maxsize=None)
def codes(fs):
    """(2, N) int8: the absent PRN's replica, then the planted one's."""
    c = np.stack([A.make_ca_table_row(p, fs) for p in (PRN_ABSENT, PRN_SIGNAL)])
    c.setflags(write=False)
    return c


def _quantise(x):
    return (np.where(x < 0, -1, 1) * np.where(np.abs(x) < 2.0, 1, 3)).astype(np.int8)


@functools.lru_cache(maxsize=None)
def if_records(sc):
    """The scene's records end to end: int8 levels +-1, +-3; I, Q interleaved when iq."""
    rng = np.random.default_rng([SEED, sc.n, sc.coh, sc.n_blocks, int(sc.iq), len(sc.phases)])
    L = sc.rec_samples
    t = np.arange(L) / sc.fs
    amp = AMP * np.repeat(np.array(BLOCK_AMPS[:sc.n_blocks]), sc.coh * sc.n)
    # the wipe-off multiplies by exp(+i f 2 pi t) (acquisition.sci:107)
    arg = 2 * np.pi * sig_freq(sc) * t + 0.3
    out = []
    for p in sc.phases:
        chips = np.tile(np.roll(codes(sc.fs)[1].astype(np.float64), p), sc.n_blocks * sc.coh)
        if sc.iq:
            s = amp * chips * np.exp(-1j * arg)
            x = np.empty(2 * L)
            x[0::2] = s.real + SIGMA * rng.standard_normal(L)
            x[1::2] = s.imag + SIGMA * rng.standard_normal(L)
        else:
            x = 2 * amp * chips * np.cos(arg) + SIGMA * rng.standard_normal(L)
        out.append(_quantise(x))
    rec = np.concatenate(out)
    rec.setflags(write=False)
    return rec


def record(sc, r=0):
    ne = (2 if sc.iq else 1) * sc.rec_samples
    return if_records(sc)[r * ne:(r + 1) * ne]


@functools.lru_cache(maxsize=None)
def reference(sc, noncoherent, rec=0):
    """acq_oracle.acquire of one record of the scene, computed once per process."""
    ref, ref_rows = A.acquire(record(sc, rec), sc.fs, codes(sc.fs), freqs(sc), GF, spc=sc.spc,
                              n_blocks=sc.n_blocks, iq=sc.iq, noncoherent=noncoherent,
                              coh=sc.coh, return_rows=True)
    if noncoherent:
        for rr in ref_rows:
            for r in rr:
                r["block"] = -1          # the non-coherent rows carry no block choice
    return ref, ref_rows


def literal_row(sc, freq, code, blk, rec=0):
    """The coh*N-point correlation of one block, first code period
    (acquisition.sci:113-135), with nothing folded."""
    sig = A._signal(record(sc, rec), sc.iq)
    L = sc.coh * sc.n
    pp = np.arange(L) * 2 * np.pi / sc.fs
    X = np.fft.fft(np.exp(1j * freq * pp) * sig[blk * L:(blk + 1) * L])
    cf = np.conj(np.fft.fft(np.tile(codes(sc.fs)[code].astype(np.float64), sc.coh)))
    return (np.abs(np.fft.ifft(X * cf)) ** 2)[:sc.n]


# ---- the fold as the kernels do it, and the ways of getting it wrong --------------------
MISTAKES = ("phase_restart", "coh_ignored", "block_stride", "real_as_iq", "record_stride")


def mistakes(sc):
    m = ["phase_restart", "coh_ignored", "block_stride"]
    if not sc.iq:
        m.append("real_as_iq")
    if len(sc.phases) > 1:
        m.append("record_stride")
    return m


def folded_signal_row(sc, noncoherent, mistake=None, rec=0):
    """The signal row (SIG_GROUP, SIG_BIN) from the N-point fold the kernels compute;
    `mistake` names one wrong restatement of it:
      phase_restart  carrier phase n instead of n + p*N
      coh_ignored    the first period of every block only
      block_stride   block b read from b*N instead of b*coh*N
      real_as_iq     a real record indexed as interleaved I, Q (zero past its end)
      record_stride  record r read from r*n_blocks*N instead of r*n_blocks*coh*N"""
    assert mistake is None or mistake in MISTAKES
    N, coh = sc.n, sc.coh
    x = if_records(sc).astype(np.float64)
    as_iq = sc.iq or mistake == "real_as_iq"

    def sample(idx):
        def elem(e):
            return np.where(e < len(x), x[np.minimum(e, len(x) - 1)], 0.0)
        return elem(2 * idx) + 1j * elem(2 * idx + 1) if as_iq else elem(idx)

    rec0 = rec * sc.n_blocks * (1 if mistake == "record_stride" else coh) * N
    bstride = (1 if mistake == "block_stride" else coh) * N
    f = freqs(sc)[SIG_BIN]
    cf = np.conj(np.fft.fft(codes(sc.fs)[SIG_GROUP].astype(np.float64)))
    n = np.arange(N)
    rows = []
    for b in range(sc.n_blocks):
        acc = np.zeros(N, complex)
        for p in range(1 if mistake == "coh_ignored" else coh):
            m = n + p * N
            ph = n if mistake == "phase_restart" else m
            acc += sample(rec0 + b * bstride + m) * np.exp(1j * f * (ph * 2 * np.pi / sc.fs))
        rows.append(np.abs(np.fft.ifft(np.fft.fft(acc) * cf)) ** 2)
    if noncoherent:
        row, chosen = np.sum(rows, axis=0), -1
    else:
        chosen = 0
        for k in range(1, sc.n_blocks):      # acquisition.sci:126-132
            if not (rows[chosen].max() > rows[k].max()):
                chosen = k
        row = rows[chosen]
    return dict(peak=float(row.max()), argmax=int(np.argmax(row)), block=chosen)


def miss(row, ref_row):
    """How far a restated signal row is from the reference's: the relative peak
    difference, or inf where it decides another block or argmax."""
    if row["block"] != ref_row["block"] or row["argmax"] != ref_row["argmax"]:
        return float("inf")
    return abs(row["peak"] - ref_row["peak"]) / ref_row["peak"]
