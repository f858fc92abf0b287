"""Navigation symbols of Galileo E1B and GLONASS L3OC: numpy restatement of the Scilab
receiver's symbol chain, and seeded generators.

TEST INFRASTRUCTURE ONLY (no GPU).  Restates, from POSTPROCESSING_SCILAB_RECEIVERS:

  GALILEO/E1/convolution_decoding/convol_decoder.sci       viterbi_literal(code, False)
  GALILEO/E1/convolution_decoding/convol_decoder_soft.sci  viterbi_literal(code, True)
                (GLONASS/L3/convolution_decoding/ holds the same three files)
  GALILEO/E1/convolution_decoding/convol_encoder.sci:50-57 conv_encode
  GALILEO/E1/findPageStart.sci:39-63                       find_page_start
  GALILEO/E1/include/decode_gll_data.sci:16-39             decode_gll_data
  GLONASS/L3/test_data_decode.sce:19-83                    l3_data_decode

viterbi_literal keeps the files' matrices (Dist, P, M, the shifted identities Jd / Jp,
the predecessor table I, the Z list) and their 1-based state numbers; only the loops over
states inside one column are numpy expressions.  One departure: the files pad the code word
to f*L entries, which is fewer than the (f + L - 1) pairs they then read when L < 3 (Scilab
stops with an index error); here the padding goes on with zeros as far as it is read.

viterbi_fast is an independent implementation of the same decision rule on index arrays;
tests/test_navsym_cpu.py holds the two equal.  The E1 and L3 restatements take the decoder
as an argument.

Three things a textbook Viterbi decoder does differently:
  1. the decision is not a best-path traceback: every state at the window's end is walked
     back, and of the start states that survive the one with the smallest metric after the
     window's first step gives the bit, the lowest state on ties;
  2. the trellis is not flushed: the code word is padded with zero pairs, so the last six
     bits of a message that does not end in six zeros can come out wrong on clean input;
  3. test_data_decode.sce:29 compares a sum of ten +-1 products with -20, so an inverted
     L3 stream is never turned round.
"""
from __future__ import annotations

import numpy as np

GEN = np.array([[1, 0, 1, 1, 0, 1, 1], [1, 1, 1, 1, 0, 0, 1]])     # decode_gll_data.sci:37
N_OUT, M_REG = 2, 7
WINDOW = 6 * M_REG                                                   # f
E1_SYNC = np.array([-1, 1, -1, 1, 1, -1, -1, -1, -1, -1])            # decode_gll_data.sci:18
NH = np.array([-1, -1, -1, -1, 1, 1, -1, 1, -1, 1])                  # test_data_decode.sce:19
BARKER = np.array([-1, -1, -1, 1, -1])                               # :20
TIME_MARK = np.array([-1, -1, -1, -1, -1, 1, -1, -1, 1, -1, -1, 1, -1, 1, -1, -1, 1, 1, 1, -1])


# ---- convol_encoder.sci ----------------------------------------------------------------
def conv_encode(msg):
    """code = W(:)' with W(i, :) = modulo(convol(mess, X(i, :)), 2): (len + 6) * 2 symbols,
    the two outputs of one step next to each other."""
    msg = np.asarray(msg, np.int64).ravel()
    W = np.zeros((N_OUT, len(msg) + M_REG - 1), np.int64)
    for i in range(N_OUT):
        W[i, :] = np.round(np.convolve(msg, GEN[i])).astype(np.int64) % 2
    return W.flatten(order="F").astype(np.uint8)


# ---- convol_decoder.sci / convol_decoder_soft.sci --------------------------------------
def _db(x, p):
    """:1-16, x on p binary digits, most significant first"""
    b = np.zeros(p)
    for i in range(1, p + 1):
        d = x - 2 ** (p - i)
        b[i - 1] = (d >= 0) * 1
        x = x - 2 ** (p - i) * b[i - 1]
    return b


def _table(n, m, x):
    """:19-39, the outputs of every state for input 0 (columns 1..n) and 1 (n+1..2n)"""
    table = np.zeros((2 ** (m - 1), 2 * n))
    E = np.zeros((2 ** (m - 1), m - 1))
    for i in range(table.shape[0]):
        E[i, :] = _db(i, m - 1)
    for i in range(table.shape[0]):
        for j in range(n):
            table[i, j] = np.concatenate([[0], E[i, :]]) @ x[j, :] % 2
            table[i, n + j] = np.concatenate([[1], E[i, :]]) @ x[j, :] % 2
    return table


def viterbi_literal(code, soft=False):
    """mess, survivors, ties: the decoded bits, and per decision the number of window-start
    states that survive the elimination and how many of them share the smallest metric."""
    n, m, x = N_OUT, M_REG, GEN
    code = np.asarray(code, np.float64).ravel()
    f = 6 * m
    L = len(code) // n
    S = 2 ** (m - 1)
    d = np.zeros((S, 2))
    Dist = np.zeros((S, f + 1))
    Dist[:, 0] = np.concatenate([[0], 10000 * np.ones(S - 1)])
    P = np.zeros((S, f), np.int64)         # predecessor state numbers, 1-based; 0 = eliminated
    M = np.zeros((S, f - 1), np.int64)
    mess = np.zeros(L, np.uint8)
    survivors, ties = np.zeros(L, np.int64), np.zeros(L, np.int64)
    Jd = np.hstack([np.zeros((f + 1, 1)), np.eye(f + 1)])[:, :f + 1]
    Jp = np.hstack([np.zeros((f, 1), np.int64), np.eye(f, dtype=np.int64)])[:, :f]
    I = np.arange(1, S + 1).reshape((2, S // 2), order="F")
    I = np.hstack([I, I])
    table = _table(n, m, x)
    code_etat = np.concatenate([np.zeros(S // 2), np.ones(S // 2)])
    code = np.concatenate([code, np.zeros(max(f * L - len(code), 0))])
    code = np.concatenate([code, np.zeros(max((f + L - 1) * n - len(code), 0))])   # see above
    cols = np.arange(S)

    def column(pair, dist):
        """d(k, j), the smaller of each pair with the first on ties, and the P column"""
        for j in range(2):
            out = table[:, j * n:(j + 1) * n]
            if soft:
                diff = pair[None, :] - out
                d[:, j] = (diff[:, 0] ** 2 + diff[:, 1] ** 2) + dist
            else:
                d[:, j] = np.sum(np.round(pair[None, :] + out) % 2, axis=1) + dist
        dbis = d.flatten(order="F").reshape((2, S), order="F")
        ind = np.argmin(dbis, axis=0)
        return dbis[ind, cols], I[ind, cols]

    def eliminate():
        for i in range(1, f):
            src = P[:, f - i]
            M[src[src != 0] - 1, f - i - 1] = 1
            P[:, f - i - 1] = P[:, f - i - 1] * M[:, f - i - 1]

    def decide(c):
        Z = [(j + 1, Dist[j, 1]) for j in range(S) if P[j, 0] != 0]
        w = np.array([z[1] for z in Z])
        p = int(np.argmin(w))
        mess[c] = code_etat[Z[p][0] - 1]
        survivors[c], ties[c] = len(Z), int(np.sum(w == w[p]))

    if L < 1:
        return mess, survivors, ties
    for i in range(f):
        Dist[:, i + 1], P[:, i] = column(code[i * n:(i + 1) * n], Dist[:, i])
    eliminate()
    decide(0)
    compteur = 1
    while compteur < L:
        M[:] = 0
        Dist = Dist @ Jd.T
        P = P @ Jp.T
        Dist[:, f], P[:, f - 1] = column(code[(f + compteur - 1) * n:(f + compteur) * n],
                                         Dist[:, f - 1])
        eliminate()
        decide(compteur)
        compteur += 1
    return mess, survivors, ties


_P0 = 2 * (np.arange(64) % 32)
_U = np.arange(64) // 32


def _branch_outputs():
    """out[p, u, j]: output j of the register [u, digits of p]"""
    out = np.zeros((64, 2, 2), np.int64)
    for p in range(64):
        for u in range(2):
            reg = np.array([u] + [(p >> (5 - k)) & 1 for k in range(6)])
            out[p, u] = GEN @ reg % 2
    return out


_OUT = _branch_outputs()


def viterbi_fast(code, soft=False):
    """The decision rule on index arrays: a forward pass that keeps every step's decisions
    and metrics, then all L walks side by side."""
    code = np.asarray(code, np.float64 if soft else np.int64).ravel()
    L = len(code) // 2
    if L < 1:
        return np.zeros(0, np.uint8)
    T = L + WINDOW - 1
    rx = np.zeros((T, 2), code.dtype)
    rx[:L] = code[:2 * L].reshape(L, 2)
    metric = np.full(64, 10000, np.float64 if soft else np.int64)
    metric[0] = 0
    after = np.zeros((T, 64), metric.dtype)
    dec = np.zeros((T, 64), np.int64)
    o0, o1 = _OUT[_P0, _U], _OUT[_P0 + 1, _U]
    for t in range(T):
        r = rx[t]
        if soft:
            c0 = ((r[0] - o0[:, 0]) ** 2 + (r[1] - o0[:, 1]) ** 2) + metric[_P0]
            c1 = ((r[0] - o1[:, 0]) ** 2 + (r[1] - o1[:, 1]) ** 2) + metric[_P0 + 1]
        else:
            c0 = ((r[0] ^ o0[:, 0]) & 1) + ((r[1] ^ o0[:, 1]) & 1) + metric[_P0]
            c1 = ((r[0] ^ o1[:, 0]) & 1) + ((r[1] ^ o1[:, 1]) & 1) + metric[_P0 + 1]
        dec[t] = c1 < c0
        metric = np.where(c1 < c0, c1, c0)
        after[t] = metric
    alive = np.ones((L, 64), bool)
    c = np.arange(L)
    for k in range(WINDOW - 1):
        pred = _P0[None, :] + dec[c + WINDOW - 1 - k]
        rows, states = np.nonzero(alive)
        prev = np.zeros((L, 64), bool)
        prev[rows, pred[rows, states]] = True
        alive = prev
    w = np.where(alive, after[:L].astype(np.float64), np.inf)
    return (np.argmin(w, axis=1) // 32).astype(np.uint8)


# ---- findPageStart.sci, decode_gll_data.sci --------------------------------------------
def find_page_start(i_p):
    """firstPage of one channel, 0-based, or -1 (:39-63)"""
    nav_bits = np.sign(np.asarray(i_p, np.float64))
    sync_pattern = np.array([-1, -1, -1, -1, -1, 1, 1, -1, 1, -1])
    sync_pattern_long = np.kron(sync_pattern, np.ones(4))
    corr = np.convolve(sync_pattern_long, nav_bits)
    corr = corr[39:]
    index = np.nonzero(np.abs(corr) > 38)[0]
    for i in range(len(index)):
        index2 = index - index[i]
        if np.any(index2 == 1000):
            return int(index[i])
    return -1


def decode_gll_data(data, decoder=viterbi_fast):
    """One page part of 1000 prompt sums -> 120 bits"""
    ndata = np.sign(np.asarray(data[:1000], np.float64))
    ndata = np.sign(ndata.reshape((4, 250), order="F").sum(axis=0))
    if np.sign(np.sum(ndata[:10] * E1_SYNC)) == -1:
        ndata = -ndata
    ndata = ndata[10:].reshape((30, 8), order="F").T
    ndata = ndata.flatten(order="F")
    return decoder(np.floor((ndata + 1) / 2).astype(np.uint8))


def e1_pages(series, decoder=viterbi_fast):
    """first_page and the bits of every whole page part from it on, [n_pages, 120]"""
    series = np.asarray(series, np.float64)
    first = find_page_start(series)
    pages = []
    if first >= 0:
        for p in range(first, len(series) - 999, 1000):
            pages.append(decode_gll_data(series[p:p + 1000], decoder))
    return first, np.array(pages, np.uint8).reshape(len(pages), 120)


# ---- test_data_decode.sce --------------------------------------------------------------
def _xcorr_lags(x, pattern):
    """xcorr(x, pattern) from lag 0 on: sum_j x[k + j] * pattern[j], zeros past the end"""
    xp = np.concatenate([x, np.zeros(len(pattern))])
    return np.array([np.sum(xp[k:k + len(pattern)] * pattern) for k in range(len(x))])


def l3_data_decode(pilot, data, decoder=viterbi_fast):
    """start (0-based, -1 if the overlay is never met), bits, time mark positions"""
    I = np.sign(np.asarray(pilot, np.float64))
    Q = np.sign(np.asarray(data, np.float64))
    starts = np.nonzero(np.abs(_xcorr_lags(I, NH)) == 10)[0]
    if len(starts) == 0:
        return -1, np.zeros(0, np.uint8), np.zeros(0, np.int64)
    start = int(starts[0])
    I, Q = I[start:], Q[start:]
    if np.sum(NH * I[:len(NH)]) == -20:        # :29, never true
        I, Q = -I, -Q
    n10 = len(I) // 10
    Q = Q[:10 * n10] * np.tile(BARKER, 2 * n10)
    ndata = np.sign(Q.reshape((5, 2 * n10), order="F").sum(axis=0))
    bits = decoder(np.floor((ndata + 1) / 2).astype(np.uint8))
    marks = np.nonzero(np.abs(_xcorr_lags(bits * 2.0 - 1, TIME_MARK)) == 20)[0]
    return start, bits, marks


# ---- generators ------------------------------------------------------------------------
def noisy_code(rng, L, flip_rate=0.0, random=False, zero_tail=False):
    """msg (L bits) and a hard code word of L pairs: the encoder's first 2L symbols with
    flips at flip_rate, or L random pairs."""
    msg = rng.integers(0, 2, L).astype(np.uint8)
    if zero_tail:
        msg[max(L - 6, 0):] = 0
    if random:
        return msg, rng.integers(0, 2, 2 * L).astype(np.uint8)
    code = conv_encode(msg)[:2 * L]
    return msg, code ^ (rng.random(2 * L) < flip_rate).astype(np.uint8)


def soft_code(rng, L, grid=False, sigma=0.7):
    """msg and soft pairs: the code word plus noise, on a 1/8 grid (exact arithmetic, many
    ties) or as plain doubles."""
    msg = rng.integers(0, 2, L).astype(np.uint8)
    code = conv_encode(msg)[:2 * L].astype(np.float64)
    if grid:
        return msg, code + rng.integers(-6, 7, 2 * L) / 8.0
    return msg, code + sigma * rng.standard_normal(2 * L)


def _disturb(rng, x, flip_rate, n_zeros, keep):
    """sign flips at flip_rate and n_zeros exact zeros, outside the samples marked `keep`"""
    free = np.nonzero(~keep)[0]
    x = x.copy()
    x[free[rng.random(len(free)) < flip_rate]] *= -1
    if n_zeros:
        x[rng.choice(free, n_zeros, replace=False)] = 0.0
    return x


def e1_series(rng, n_epochs, start, polarity=1, amplitude=1500.0, flip_rate=0.0, n_zeros=0,
              zero_in_sync=False):
    """I_P_P of one channel: `start` random epochs, then page parts of 1000 epochs (sync
    pattern, 240 interleaved symbols of a 114-bit message with six zero tail bits, each
    symbol four epochs) up to n_epochs.  Returns the series and the messages [n, 120]."""
    out = list(rng.choice([-1.0, 1.0], start))
    keep = [False] * start
    msgs = []
    while len(out) < n_epochs:
        msg = rng.integers(0, 2, 120).astype(np.uint8)
        msg[114:] = 0
        sym = conv_encode(msg[:114]) * 2.0 - 1              # 240 symbols
        z = np.zeros(240)
        for c in range(8):
            for r in range(30):
                z[r + 30 * c] = sym[c + 8 * r]
        y = np.concatenate([E1_SYNC, z])
        out += list(np.repeat(y, 4))
        keep += [True] * 40 + [False] * 960
        msgs.append(msg)
    x = polarity * amplitude * np.array(out[:n_epochs])
    x = _disturb(rng, x, flip_rate, n_zeros, np.array(keep[:n_epochs]))
    if zero_in_sync and start + 40 <= n_epochs:
        x[start + 17] = 0.0         # 39 of 40 still passes the > 38 test
    return x, np.array(msgs, np.uint8)


def l3_series(rng, n_epochs, start, polarity=1, amplitude=900.0, flip_rate=0.0, n_zeros=0,
              mark_at=None, constant_pilot=False):
    """pilot I_P and data Q_P2 of one channel: `start` random epochs, then the overlay on
    the pilot and Barker-coded symbols (five epochs each) of a random message on the data
    channel, the time mark written into the message at bit mark_at.  Returns pilot, data
    and the message."""
    n_bits = n_epochs // 10 + 2
    msg = rng.integers(0, 2, n_bits).astype(np.uint8)
    if mark_at is not None:
        msg[mark_at:mark_at + 20] = (TIME_MARK + 1) // 2
    sym = conv_encode(msg) * 2.0 - 1
    data = np.concatenate([rng.choice([-1.0, 1.0], start),
                           (sym[:, None] * BARKER[None, :]).ravel()])[:n_epochs]
    pilot = np.concatenate([rng.choice([-1.0, 1.0], start),
                            np.tile(NH.astype(np.float64), n_bits + 6)])[:n_epochs]
    if constant_pilot:
        pilot = np.ones(n_epochs)
    keep = np.zeros(n_epochs, bool)
    data = _disturb(rng, polarity * amplitude * data, flip_rate, n_zeros, keep)
    keep[start:start + 10] = True
    pilot = _disturb(rng, polarity * amplitude * pilot, 0.0, n_zeros, keep)
    return pilot, data, msg
