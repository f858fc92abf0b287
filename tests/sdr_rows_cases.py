"""Inputs shared by the per-row tests of the GPS-SDR int16 acquisition
(test_sdr_acq_rows_cpu.py, test_sdr_acq_rows_gpu.py): buffers that make the
saturating arm, the weak search's column shift and the first-index tie rules
decide something, and the CPU searches that pick them.  Everything here runs on
the C oracle (oracle/sdr_acq.c); nothing is taken from the GPU.
"""
import functools

import numpy as np

import sdr_oracle as S

N = S.N
LCVS = (-100, -1, 0, 100)          # one-lcv ranges: the padding limits and the sign change


def one_lcv(kind, lcv):
    """(doppmin, doppmax) that search lcv alone: medium's upper bound is
    inclusive (acquisition.cpp:324), strong and weak exclusive (:258, :452)."""
    return (lcv * 1000, lcv * 1000 + (0 if kind == "medium" else 1000))


def uniform(amp, ms, seed):
    """ms x 2048 CPX uniform in +-amp; amp 32768 = the whole int16 range."""
    rng = np.random.default_rng(seed)
    hi = min(amp, 32767)
    return rng.integers(-amp, hi + 1, (ms * N, 2)).astype(np.int16)


def sparse(seed, ms=1):
    """+-1 samples at density 1/64, the rest 0: row maxima of a few hundred,
    so that equal maxima within a row are common."""
    rng = np.random.default_rng(seed)
    on = rng.random((ms * N, 2)) < 1.0 / 64
    sign = rng.integers(0, 2, (ms * N, 2)) * 2 - 1
    return (on * sign).astype(np.int16)


def impulse(ms):
    """(1000, 0) at sample 0 of every 1-ms block: every spectrum is constant."""
    b = np.zeros((ms, N, 2), np.int16)
    b[:, 0] = (1000, 0)
    return b.reshape(-1, 2)


# ---- the weak search's column shift --------------------------------------------
# Signals at +-100 kHz Doppler drift by +-20 chips (40 samples) over 310 ms; the
# search follows them with shifts 0..+36 (lcv = 100) and 0..-37 (lcv = -100).
# code_phase is chosen so that the summed peak lies a few columns past column 0
# / 1024 in the direction of the drift: the 15 passes' own peaks then lie on
# both sides of the boundary.  Record 0 carries the +100 kHz pair, record 1 the
# -100 kHz pair; svs are the two PRNs.
PLANT_SVS = (4, 25)                # PRN 5, PRN 26


def _cp_for_column(col):
    """code_phase [chips] whose correlation peak lies at column col of the
    medium / weak search (code_phase = column there, acquisition.cpp:397-405):
    a code that starts col samples into the buffer."""
    return (1023.0 - col * 1023.0 / N) % 1023.0


@functools.lru_cache(maxsize=None)
def planted():
    """[2, 310*2048, 2] int16."""
    recs = []
    for r, (dop, c0, c1) in enumerate(((100300.0, 12, 1024 + 14), (-99700.0, N - 12, 1024 - 14))):
        sigs = [dict(prn=PLANT_SVS[0] + 1, code_phase=_cp_for_column(c0), doppler=dop, amp=3.0),
                dict(prn=PLANT_SVS[1] + 1, code_phase=_cp_for_column(c1), doppler=dop + 150.0,
                     amp=3.0)]
        recs.append(S.make_long_buffer(sigs, 310, seed=40 + r))
    return np.stack(recs)


def pass_columns(o, lcv, lcv2, column):
    """The 15 columns whose powers the weak search sums into `column`."""
    return [(column - o.weak_shift(i, lcv, lcv2)) % N for i in range(15)]


def straddles(cols, boundary, reach=40):
    """cols lie within reach of boundary (0 or 1024, circular) on both sides."""
    d = [((c - boundary + N // 2) % N) - N // 2 for c in cols]
    return all(abs(x) <= reach for x in d) and min(d) < 0 <= max(d)


# ---- equal maxima within a row --------------------------------------------------
def tid_of(kind, index):
    """The kernel thread that owns cell `index` of a row: the strong kernel's
    256 threads hold outputs g + 512 q, g = tid + 256 u; the medium / weak
    kernel's 1024 threads hold columns tid and tid + 1024 of every DFT row."""
    return index % 256 if kind == "strong" else index % 1024


def find_ties(o, codes, kind, seeds, svs, lcvs, max_rows=6):
    """Search sparse(seed) buffers for rows whose maximum occurs at two or more
    cells.  Returns a list of dict(seed, sv, lcv, lcv2, k, mag, cells) with
    cells = the tied flat indices, ascending; rows in which the first cell's
    thread is above a later cell's come first (the reduction then has to carry
    the index, not the lane order)."""
    ms = {"strong": 1, "medium": 10, "weak": 310}[kind]
    found = []
    for seed in seeds:
        buf = sparse(seed, ms)
        if kind == "strong":
            rows = o.prep_if(buf)
        else:
            rows = o.new_rows()
            o.prep_rows(rows, buf, ms)
        for sv in svs:
            for lcv in lcvs:
                for lcv2 in range(4):
                    for k in range(2 if kind == "weak" else 1):
                        p = o.row_powers(kind, rows, codes[sv], lcv, lcv2, k).reshape(-1)
                        m = int(p.max())
                        cells = np.flatnonzero(p == m)
                        if m > 0 and len(cells) >= 2:
                            t = [tid_of(kind, int(c)) for c in cells]
                            found.append(dict(seed=seed, sv=sv, lcv=lcv, lcv2=lcv2, k=k, mag=m,
                                              cells=[int(c) for c in cells],
                                              inverted=t[0] > min(t[1:])))
        if sum(f["inverted"] for f in found) >= 1 and len(found) >= max_rows:
            break
    found.sort(key=lambda f: not f["inverted"])
    return found[:max_rows]


# Seed windows of the bounded searches (svs 7 and 19, lcv -1 and 0).  A scan of
# seeds 1..199 (medium) and 1..99 (weak) found 23 and 3 tied rows; the windows
# below hold the first few of them so that the search stays within a second or
# two.  No weak row with the first cell in the higher thread turned up.
TIE_SEARCH = {"strong": (range(1, 40), range(-2, 2)), "medium": (range(19, 29), range(-1, 1)),
              "weak": (range(27, 30), range(0, 1))}
TIE_SVS = (7, 19)


@functools.lru_cache(maxsize=None)
def ties(kind):
    o = S.OracleSDR()
    seeds, lcvs = TIE_SEARCH[kind]
    return find_ties(o, o.prn_codes(), kind, seeds, TIE_SVS, lcvs)


# the weak search over the impulse record: lcv -7..9, 136 rows; the rows with
# all-zero shifts at lcv2 = 2 (lcv 0, 1, 2) hold the maximum: rows 60/61, 68/69,
# 76/77, on both sides of the 64-row stride of the row scan
IMPULSE_WEAK_RANGE = (-7000, 10000)
