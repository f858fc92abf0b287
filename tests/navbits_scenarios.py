"""Frame synchronisation and data bits of GPS L1 C/A, GLONASS L1OF and BeiDou B1I as the
Scilab receiver computes them, restated twice, and the series the tests run them on.

*_literal: a transcription of the six files, line by line, with their 1-based indices kept
in the comments: convol as a full convolution and then the slice, the 20-sample sums as an
explicit left-to-right loop (np.sum adds pairwise), navPartyChk and checkPhase on the
values the files hand them ({-1, 0, 1} and {0, 0.5, 1}).
  GPS/L1/findPreambles.sci, include/navPartyChk.sci, include/checkPhase.sci,
  postNavigation.sci:91-106, include/ephemeris.sci:68-80
  GLONASS/L1/findTimeMarks.sci, postNavigation.sci:89-99, include/ephemeris.sci:30-36,
  include/decode_gl_data.sci
  COMPASS/B1/findSubframeStart.sci, postNavigation.sci:81-92, include/ephemeris.sci:28-34,
  include/decode_bd_data.sci
*_fast: an independent restatement (prefix sums over the pattern's runs, vectorised sums in
the same add order, the D30* chain without a loop); tests/test_navbits_cpu.py holds the two
equal, tests/test_navbits_gpu.py holds the device to the literal one.

Positions are 0-based epoch indices, -1 for none; bits are uint8 0 / 1, 2 for the files' 0.5.
The one widening (gnsscorr.h): GPS returns the whole subframes that fit, where the file
takes five or stops with an index error.
"""
import numpy as np

# ---- the files' vectors, as written there ------------------------------------------------
GPS_PREAMBLE_BITS = np.array([1, 1, -1, 1, -1, -1, -1, 1])             # findPreambles.sci:56
GLO_TM_BITS = np.array([-1, 1, 1, -1, 1, -1, -1, 1, -1, -1, -1, -1, 1, -1, 1, -1, 1, 1, 1, -1,
                        1, 1, -1, -1, -1, 1, 1, 1, 1, 1])              # findTimeMarks.sci:45
B1_SEARCH_PREAMBLE = np.array([-1, 1, -1, -1, 1, -1, -1, -1, 1, 1, 1])  # findSubframeStart.sci:42
B1_SEARCH_SECONDARY = np.array([-1, 1, 1, 1, -1, -1, 1, -1, 1, -1, 1, 1, -1, -1, 1, -1, -1, -1,
                                -1, -1])                               # :43
B1_PREAMBLE = np.array([1, 1, 1, -1, -1, -1, 1, -1, -1, 1, -1])        # decode_bd_data.sci:18
B1_SECONDARY = np.array([-1, -1, -1, -1, -1, 1, -1, -1, 1, 1, -1, 1, -1, 1, -1, -1, 1, 1, 1,
                         -1])                                          # :19

GPS_PREAMBLE_MS = np.kron(GPS_PREAMBLE_BITS, np.ones(20, int))         # findPreambles.sci:60
GLO_TM_LONG = np.kron(-GLO_TM_BITS, np.ones(10, int))                  # findTimeMarks.sci:46
B1_PREAMBLE_LONG = np.kron(B1_SEARCH_PREAMBLE, -B1_SEARCH_SECONDARY)   # findSubframeStart.sci:44

# the device's patterns, in correlation order: the convol vectors reversed
GPS_PATTERN = np.kron([1, -1, -1, -1, 1, -1, 1, 1], np.ones(20, int)).astype(np.int8)
GLO_PATTERN = GLO_TM_LONG[::-1].astype(np.int8)
B1_PATTERN = B1_PREAMBLE_LONG[::-1].astype(np.int8)
GPS_THRESHOLD, GLO_THRESHOLD, B1_THRESHOLD = 153, 290, 200

# navPartyChk.sci:68-91, 1-based
PARITY_TERMS = [
    [1, 3, 4, 5, 7, 8, 12, 13, 14, 15, 16, 19, 20, 22, 25],
    [2, 4, 5, 6, 8, 9, 13, 14, 15, 16, 17, 20, 21, 23, 26],
    [1, 3, 5, 6, 7, 9, 10, 14, 15, 16, 17, 18, 21, 22, 24],
    [2, 4, 6, 7, 8, 10, 11, 15, 16, 17, 18, 19, 22, 23, 25],
    [2, 3, 5, 7, 8, 9, 11, 12, 16, 17, 18, 19, 20, 23, 24, 26],
    [1, 5, 7, 8, 10, 11, 12, 13, 15, 17, 21, 24, 25, 26]]


def sign(x):
    """Scilab's sign for reals: -1, 0, 1"""
    x = np.asarray(x)
    return (x > 0).astype(int) - (x < 0).astype(int)


def half_bits(v, signed=False):
    """{0, 0.5, 1}, or {-1, 0, 1} with signed, -> uint8 0 / 1 with 2 for the undecided value"""
    v = np.asarray(v, float)
    if signed:
        v = (v + 1) / 2
    return np.where(v == 0.5, 2, v).astype(np.uint8)


# =========================================================================== literal ====
def sums20_literal(seg):
    """matrix(seg, 20, n / 20) and sum(.., 'r'): each column added from its first row down"""
    seg = np.asarray(seg, float)
    out = np.zeros(len(seg) // 20)
    for j in range(len(out)):
        acc = float(seg[20 * j])
        for t in range(1, 20):
            acc = acc + float(seg[20 * j + t])
        out[j] = acc
    return out


def convol_hits_literal(vec, x, first_k, threshold):
    """convol(vec, sign(x(1 + off : $))), result(T : $), find(abs(..) > threshold) + off:
    the hits as 0-based epochs, ascending"""
    T = len(vec)
    bits = sign(np.asarray(x)[first_k:])                       # x(1 + off : $)
    if bits.size == 0:
        return np.zeros(0, int)
    r = np.convolve(np.asarray(vec, float), bits.astype(float))  # length T + L - 1
    r = r[T - 1:]                                              # r(T : $)
    return np.flatnonzero(np.abs(r) > threshold) + first_k     # 1-based find + off, minus 1


def nav_party_chk_literal(ndat32):
    """navPartyChk.sci:56-103 on 32 values in {-1, 0, 1}"""
    ndat = np.concatenate([[0], np.asarray(ndat32, int)])      # ndat[i] is the file's ndat(i)
    if ndat[2] != 1:                                           # :56
        ndat[3:27] = -1 * ndat[3:27]                           # :57 ndat(3:26)
    parity = [int(np.prod(ndat[terms])) for terms in PARITY_TERMS]
    if sum(int(parity[i] == ndat[27 + i]) for i in range(6)) == 6:   # :94
        return -1 * ndat[2]                                    # :99
    return 0


def gps_first_subframe_literal(x, search_start=5000):
    """findPreambles.sci:84-153 for one channel"""
    x = np.asarray(x, float)
    index = convol_hits_literal(GPS_PREAMBLE_MS, x, search_start, 153) + 1   # 1-based, :106
    for i in range(len(index)):                                # :109
        index2 = index - index[i]                              # :116
        if np.any(index2 == 6000):                             # :118
            seg = x[index[i] - 40 - 1: index[i] + 20 * 60 - 1]  # (index - 40 : index + 1199)
            bits = sign(sums20_literal(seg))                   # :133-139
            if nav_party_chk_literal(bits[0:32]) != 0 and \
                    nav_party_chk_literal(bits[30:62]) != 0:   # bits(1:32), bits(31:62)
                return int(index[i]) - 1
    return -1


def check_phase_literal(word, d30star):
    """checkPhase.sci:45-52 on values in {0, 0.5, 1}"""
    rslt = np.array(word, float)
    if d30star == 1:
        rslt[0:24] = word[0:24] - 1
        rslt[0:24] = rslt[0:24] * (-1)
    return rslt


def gps_bits_literal(x, p, n_sub=5):
    """postNavigation.sci:91-106 and ephemeris.sci:68-80 for n_sub subframes from the 0-based
    first subframe p: 300 n_sub bits"""
    x = np.asarray(x, float)
    sfs = p + 1                                                # 1-based
    seg = x[sfs - 20 - 1: sfs + 300 * n_sub * 20 - 1]          # (sfs - 20 : sfs + 1500 * 20 - 1)
    nav = (sign(sums20_literal(seg)) + 1) / 2                  # :99-106
    bits, d30star = nav[1:].copy(), nav[0]                     # ephemeris(navBits(2:$), navBits(1))
    for i in range(n_sub):                                     # ephemeris.sci:68
        sub = bits[300 * i: 300 * (i + 1)]                     # a view: written back in place
        for j in range(10):                                    # :74
            sub[30 * j: 30 * (j + 1)] = check_phase_literal(sub[30 * j: 30 * (j + 1)], d30star)
            d30star = sub[30 * j + 29]                         # :79
    return half_bits(bits)


def gps_frames_literal(x, search_start=5000, max_subframes=5):
    """(first_subframe, bits of the whole subframes that fit)"""
    p = gps_first_subframe_literal(x, search_start)
    if p < 0:
        return -1, np.zeros(0, np.uint8)
    n_sub = min(max_subframes, 5, (len(x) - p) // 6000)
    return p, gps_bits_literal(x, p, n_sub)


def decode_gl_data_literal(data):
    """decode_gl_data.sci:17-34 on 1700 signs"""
    ndata = np.asarray(data[0:1700], int)
    meandr = np.ones(170, int)
    meandr[1::2] = -1                                          # meandr(2:2:$)
    meandr = np.kron(-meandr, np.ones(10, int))
    ndata = ndata * meandr
    ndata = sign(ndata.reshape(-1, 20).sum(axis=1))            # integers: any order
    dec = np.zeros(85, int)
    for j in range(1, 85):                                     # j = 1:84
        dec[85 - j - 1] = -ndata[j - 1] * ndata[j]             # decoded(85 - j) = -n(j) n(j + 1)
    dec[84] = -1
    return dec


def glo_strings_literal(x, max_strings=15):
    """findTimeMarks.sci:42-65, then per string what postNavigation.sci:96-99 and
    ephemeris.sci:30-36 hand decode_gl_data: (first_mark, [n_strings, 85] bits)"""
    x = np.asarray(x, float)
    index = convol_hits_literal(GLO_TM_LONG, x, 0, 290) + 1    # 1-based
    if len(index) == 0:
        return -1, np.zeros((0, 85), np.uint8)
    start = int(index[0])
    out = []
    for i in range(1, min(max_strings, 15) + 1):               # i = 1:15
        lo = start + 300 + 2000 * (i - 1)                      # 1-based first sample
        if lo + 1700 - 1 > len(x):
            break
        out.append(half_bits(decode_gl_data_literal(sign(x[lo - 1: lo - 1 + 1700])), True))
    return start - 1, np.array(out, np.uint8).reshape(-1, 85)


def decode_bd_data_literal(data):
    """decode_bd_data.sci:16-38 on 6000 signs"""
    ndata = np.asarray(data[0:6000], int)
    ndata = ndata * np.kron(np.ones(300, int), B1_SECONDARY)
    ndata = sign(ndata.reshape(-1, 20).sum(axis=1))
    if sign(np.sum(ndata[0:11] * B1_PREAMBLE)) == -1:          # :29
        ndata = -ndata
    dec = list(ndata[11:26])                                   # ndata(12:26)
    for i in range(1, 10):                                     # i = 1:9
        word = ndata[i * 30: i * 30 + 30]                      # ndata(i*30+1 : i*30+30)
        dec += list(word[0:21:2]) + list(word[1:22:2])         # (1:2:21), (2:2:22)
    return np.array(dec, int)


def b1_subframes_literal(x, max_subframes=5):
    x = np.asarray(x, float)
    index = convol_hits_literal(B1_PREAMBLE_LONG, x, 0, 200) + 1
    if len(index) == 0:
        return -1, np.zeros((0, 213), np.uint8)
    start = int(index[0])
    out = []
    for i in range(1, min(max_subframes, 5) + 1):
        lo = start + 6000 * (i - 1)
        if lo + 6000 - 1 > len(x):
            break
        out.append(half_bits(decode_bd_data_literal(sign(x[lo - 1: lo - 1 + 6000])), True))
    return start - 1, np.array(out, np.uint8).reshape(-1, 213)


# ============================================================================== fast ====
def pattern_r_fast(x, pattern):
    """r[k] = sum_i pattern[i] sign(x[k + i]) for every k < len(x), samples past the end 0:
    one prefix sum of the signs, one difference per run of equal taps"""
    pattern = np.asarray(pattern, int)
    n, T = len(x), len(pattern)
    c = np.concatenate([[0], np.cumsum(np.concatenate([sign(x), np.zeros(T, int)]))])
    edges = np.flatnonzero(np.diff(pattern)) + 1
    r = np.zeros(n, int)
    for a, b in zip(np.concatenate([[0], edges]), np.concatenate([edges, [T]])):
        r += pattern[a] * (c[b:b + n] - c[a:a + n])
    return r


def pattern_hits_fast(x, pattern, threshold, first_k=0):
    r = pattern_r_fast(x, pattern)
    k = np.flatnonzero(np.abs(r) > threshold)
    return k[k >= first_k]


def sums20_fast(seg):
    cols = np.asarray(seg, float).reshape(-1, 20)
    acc = cols[:, 0].copy()
    for t in range(1, 20):
        acc = acc + cols[:, t]                                 # the same order, all bits at once
    return acc


def _parity_ok_fast(b32):
    """navPartyChk as bit arithmetic; zeros make it fail unless the file's products agree,
    so undecided bits fall back to the literal function"""
    b32 = np.asarray(b32, int)
    if np.any(b32 == 0):
        return nav_party_chk_literal(b32) != 0
    s = b32.copy()
    if s[1] != 1:
        s[2:26] = -s[2:26]
    neg = (s < 0).astype(int)
    return all((sum(neg[t - 1] for t in terms) & 1) == neg[26 + i]
               for i, terms in enumerate(PARITY_TERMS))


def gps_frames_fast(x, search_start=5000, max_subframes=5):
    x = np.asarray(x, float)
    hits = pattern_hits_fast(x, GPS_PATTERN, 153, search_start)
    hitset = set(hits.tolist())
    for p in hits:
        if p + 6000 not in hitset:
            continue
        b = sign(sums20_fast(x[p - 40: p + 1200]))
        if _parity_ok_fast(b[0:32]) and _parity_ok_fast(b[30:62]):
            break
    else:
        return -1, np.zeros(0, np.uint8)
    p = int(p)
    n_sub = min(max_subframes, 5, (len(x) - p) // 6000)
    raw = half_bits((sign(sums20_fast(x[p - 20: p + 6000 * n_sub])) + 1) / 2)
    bits = raw[1:].copy()
    d30 = np.repeat(raw[0:-1:30], 30)                          # the bit before each word
    inv = (d30 == 1) & (np.arange(len(bits)) % 30 < 24) & (bits != 2)
    bits[inv] = 1 - bits[inv]
    return p, bits


def glo_strings_fast(x, max_strings=15):
    x = np.asarray(x, float)
    hits = pattern_hits_fast(x, GLO_PATTERN, 290)
    if len(hits) == 0:
        return -1, np.zeros((0, 85), np.uint8)
    first = int(hits[0])
    m = np.concatenate([-np.ones(10, int), np.ones(10, int)])
    out = []
    for i in range(min(max_strings, 15)):
        s = first + 300 + 2000 * i
        if s + 1700 > len(x):
            break
        y = sign((sign(x[s:s + 1700]).reshape(85, 20) * m).sum(axis=1))
        dec = np.concatenate([(-y[:-1] * y[1:])[::-1], [-1]])
        out.append(half_bits(dec, True))
    return first, np.array(out, np.uint8).reshape(-1, 85)


_B1_ORDER = np.concatenate([np.arange(11, 26)] + [
    30 * w + np.concatenate([np.arange(0, 22, 2), np.arange(1, 22, 2)]) for w in range(1, 10)])


def b1_subframes_fast(x, max_subframes=5):
    x = np.asarray(x, float)
    hits = pattern_hits_fast(x, B1_PATTERN, 200)
    if len(hits) == 0:
        return -1, np.zeros((0, 213), np.uint8)
    first = int(hits[0])
    out = []
    for i in range(min(max_subframes, 5)):
        s = first + 6000 * i
        if s + 6000 > len(x):
            break
        y = sign((sign(x[s:s + 6000]).reshape(300, 20) * B1_SECONDARY).sum(axis=1))
        if np.sum(y[:11] * B1_PREAMBLE) < 0:
            y = -y
        out.append(half_bits(y[_B1_ORDER], True))
    return first, np.array(out, np.uint8).reshape(-1, 213)


# ======================================================================== generators ====
def _finish(rng, x, flip_rate, n_zeros, protect=()):
    """flipped epochs and exact zeros, outside the protected (start, stop) ranges"""
    free = np.ones(len(x), bool)
    for a, b in protect:
        free[max(a, 0):max(b, 0)] = False
    idx = np.flatnonzero(free)
    if flip_rate:
        f = idx[rng.random(len(idx)) < flip_rate]
        x[f] = -x[f]
    if n_zeros:
        x[rng.choice(idx, n_zeros, replace=False)] = 0.0
    return x


def gps_encode_word(d24, d29s, d30s):
    """IS-GPS-200 table 20-XIV: the 30 transmitted bits of 24 source bits"""
    d = np.concatenate([[d29s, d30s], np.asarray(d24, int)])   # d[i - 1] is navPartyChk's ndat(i)
    par = [int(sum(d[t - 1] for t in terms) & 1) for terms in PARITY_TERMS]
    return np.concatenate([np.asarray(d24, int) ^ d30s, par])


def gps_series(rng, n_epochs, start, polarity=1, flip_rate=0.0, n_zeros=0, amp=1000.0,
               decoys=(), lone=(), lone_valid=()):
    """Random 20-ms bits up to `start`, then subframes of ten words with valid parity whose
    first word opens with the preamble 10001011.  decoys: epochs q < start that get the
    preamble at q and at q + 6000 inside the random part (parity fails there); lone: epochs
    that get one preamble without a partner; lone_valid: epochs that get two whole words with
    the preamble and valid parity, and no partner.  Returns (series, bits 0/1 per 20 ms from the
    epoch start % 20)."""
    lead = start % 20
    n_bits = (n_epochs - lead) // 20 + 1
    bits = rng.integers(0, 2, n_bits)
    pre = np.array([1, 0, 0, 0, 1, 0, 1, 1])
    for q in list(decoys) + [q + 6000 for q in decoys] + list(lone):
        assert (q - lead) % 20 == 0
        bits[(q - lead) // 20:(q - lead) // 20 + 8] = pre
    for q in lone_valid:
        assert (q - lead) % 20 == 0 and q >= 40 and q + 1200 <= start
        for w in range(2):
            at = (q - lead) // 20 + 30 * w
            d24 = rng.integers(0, 2, 24)
            if w == 0:
                d24[:8] = pre ^ bits[at - 1]
            bits[at:at + 30] = gps_encode_word(d24, bits[at - 2], bits[at - 1])
    b0 = (start - lead) // 20
    for w in range((n_bits - b0) // 30):
        at = b0 + 30 * w
        d29s, d30s = (bits[at - 2], bits[at - 1]) if at >= 2 else (0, 0)
        d24 = rng.integers(0, 2, 24)
        if w % 10 == 0:
            d24[:8] = pre ^ d30s
        bits[at:at + 30] = gps_encode_word(d24, d29s, d30s)
    for q in [q + 6000 for q in decoys if q + 6000 >= start]:   # over the words written there
        bits[(q - lead) // 20:(q - lead) // 20 + 8] = pre
    x = np.repeat(2.0 * bits - 1, 20)
    x = np.concatenate([2.0 * rng.integers(0, 2, lead) - 1, x])[:n_epochs]
    x = polarity * amp * x * (1.0 + 0.2 * rng.random(n_epochs))
    marks = list(decoys) + [q + 6000 for q in decoys] + list(lone) + list(lone_valid)
    return _finish(rng, x, flip_rate, n_zeros, [(q, q + 160) for q in marks]), bits


def glo_series(rng, n_epochs, first, polarity=1, flip_rate=0.0, n_zeros=0, amp=800.0):
    """Random 10-ms chips up to `first`, then [time mark 300][85 meander symbols 1700]
    repeated.  Returns (series, y [n_strings_generated, 85])."""
    x = 2.0 * np.repeat(rng.integers(0, 2, first // 10 + 1), 10)[:first] - 1
    m = np.concatenate([-np.ones(10), np.ones(10)])
    ys = []
    while len(x) < n_epochs:
        y = 2 * rng.integers(0, 2, 85) - 1
        ys.append(y)
        x = np.concatenate([x, GLO_PATTERN.astype(float), np.kron(y, m)])
    x = polarity * amp * x[:n_epochs] * (1.0 + 0.2 * rng.random(n_epochs))
    return _finish(rng, x, flip_rate, n_zeros), np.array(ys)


def b1_series(rng, n_epochs, first, polarity=1, flip_rate=0.0, n_zeros=0, amp=800.0):
    """Random epochs up to `first`, then subframes of 300 symbols under the Neumann-Hoffman
    code, each opening with the 11-symbol preamble."""
    x = 2.0 * rng.integers(0, 2, first) - 1
    ys = []
    while len(x) < n_epochs:
        y = 2 * rng.integers(0, 2, 300) - 1
        y[:11] = B1_PREAMBLE
        ys.append(y)
        x = np.concatenate([x, np.kron(y, B1_SECONDARY).astype(float)])
    x = polarity * amp * x[:n_epochs] * (1.0 + 0.2 * rng.random(n_epochs))
    return _finish(rng, x, flip_rate, n_zeros), np.array(ys)


def planted(rng, n_epochs, pattern, starts, amp=500.0):
    """Noise-like +-amp epochs (no hit of their own at the thresholds the tests use) with
    `pattern` written at each start, cut off at the end of the series"""
    x = amp * (2.0 * rng.integers(0, 2, n_epochs) - 1)
    for k in starts:
        seg = np.asarray(pattern, float)[:max(n_epochs - k, 0)]
        x[k:k + len(seg)] = amp * seg
    return x


# ============================================================================ scenes ====
# Built once and shared by tests/test_navbits_cpu.py (literal == fast, planted == found)
# and tests/test_navbits_gpu.py (device == literal).  Arrays are read-only.
import functools  # noqa: E402

PRIM_T = (1, 64, 65, 160, 220, 300, 512)
PRIM_CH = (1, 3, 65)


def prim_epochs(T):
    return (T - 1, T, 63 + T, 64 + T, 1000, 4099)


def prim_threshold(T):
    return T - 1 - T // 8 if T > 1 else 0


@functools.lru_cache(maxsize=None)
def prim_case(T, n_epochs, n_ch):
    """(pattern, series [n_ch, n_epochs]): a random pattern (a few zero taps), planted at
    starts with k mod 64 in {0, 1, 63} where they fit, also cut off by the end; the last
    channel of several is noise only; a few exact zeros"""
    rng = np.random.default_rng(100000 + 1000 * T + 7 * n_epochs + n_ch)
    pattern = (2 * rng.integers(0, 2, T) - 1).astype(np.int8)
    if T >= 64:
        pattern[rng.choice(T, 3, replace=False)] = 0
    x = np.zeros((n_ch, max(n_epochs, 0)))
    for ch in range(n_ch):
        starts = [k + 64 * (ch % 3) for k in (0, 65, 127 + 64 * (T // 64 + 1))]
        starts.append(n_epochs - T + T // 16)                   # cut off, still above threshold
        if n_ch > 1 and ch == n_ch - 1:
            starts = []
        x[ch] = planted(rng, n_epochs, pattern, [k for k in starts if 0 <= k < n_epochs])
        if n_epochs > 8:
            x[ch, rng.choice(n_epochs, 2, replace=False)] = 0.0
    pattern.setflags(write=False)
    x.setflags(write=False)
    return pattern, x


@functools.lru_cache(maxsize=None)
def edge_scene():
    """Threshold edges: T = 160 at 153 with 3 / 7 zeros and 3 / 4 flips inside the planted
    pattern (r = 157, 153, 154, 152); T = 300 at 290 with 295 and 290 taps before the end."""
    rng = np.random.default_rng(31)
    x = np.stack([planted(rng, 1000, GPS_PATTERN, [321]) for _ in range(4)])
    x[0, 321 + np.array([5, 70, 159])] = 0.0
    x[1, 321 + np.array([0, 5, 64, 70, 100, 128, 159])] = 0.0
    x[2, 321 + np.array([5, 70, 159])] *= -1
    x[3, 321 + np.array([0, 5, 70, 159])] *= -1
    y = np.stack([planted(rng, 1000, GLO_PATTERN, [1000 - 295]),
                  planted(rng, 1000, GLO_PATTERN, [1000 - 290])])
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def _bit_span(start, word, bit):
    """epochs of bit `bit` (0-based) of word `word` counted from the first subframe"""
    a = start + 20 * (30 * word + bit)
    return slice(a, a + 20)


GPS_START = 100      # search_start of the short scene


@functools.lru_cache(maxsize=None)
def gps_scene():
    """4 channels x 14 000 epochs: [0] subframes from 1900 (two whole ones), exact zeros, at
    300 a preamble with two words of valid parity but no partner 6000 later; [1] from 2500 (one whole subframe), inverted, 1 % flips, a decoy
    pair at 400 / 6400 whose parity fails; [2] from 700 with a bit of ten +a and ten -a
    (sum exactly 0 -> 2), one in a word's D30, the group [1e16, 1, -1e16, 0, ...], which is 0
    when added in order and 1 when the large pair meets first, and [1e16, 1, -1e16, 1, 0, ...],
    which is 1 in order and 0 when neighbours are added in pairs first; [3] random bits and one lone preamble: no frame."""
    rng = np.random.default_rng(2024)
    n = 14000
    x = np.zeros((4, n))
    x[0], b0 = gps_series(rng, n, 1900, n_zeros=30, lone_valid=[300])
    x[1], _ = gps_series(rng, n, 2500, polarity=-1, flip_rate=0.01, decoys=[400])
    x[2], b2 = gps_series(rng, n, 700)
    tie = np.tile([1000.0, -1000.0], 10)
    x[2, _bit_span(700, 3, 7)] = tie
    x[2, _bit_span(700, 5, 29)] = tie
    order = np.zeros(20)
    order[:3] = [1e16, 1.0, -1e16]
    x[2, _bit_span(700, 12, 3)] = order
    order[3] = 1.0                                              # in order 1; added in pairs 0
    x[2, _bit_span(700, 13, 3)] = order
    x[3], _ = gps_series(rng, n, 13990, lone=[5010])
    x[3, 13980:] = 1000.0
    # words that follow a D30 = 1 are there, in both kinds of channel
    assert any(b0[(1900 // 20) + 30 * w - 1] == 1 for w in range(1, 20))
    assert any(b2[(700 // 20) + 30 * w - 1] == 0 for w in range(1, 20))
    x.setflags(write=False)
    return x, [1900, 2500, 700, -1], [600, 300, 600, 0]


@functools.lru_cache(maxsize=None)
def gps_long_scene():
    """one channel of 36 000 epochs, inverted, subframes from 5200: five whole ones with the
    file's search offset of 5000"""
    rng = np.random.default_rng(36)
    x, _ = gps_series(rng, 36000, 5200, polarity=-1, n_zeros=40)
    x = x.reshape(1, -1)
    x.setflags(write=False)
    return x, [5200], [1500]


@functools.lru_cache(maxsize=None)
def glo_scene():
    """30 100 epochs: [0] mark at 0, 15 strings, one symbol split 10 / 10 (two decoded 2s);
    [1] mark at 37, flips and zeros; [2] = -[1]: the same bits"""
    rng = np.random.default_rng(77)
    n = 30100
    x = np.zeros((3, n))
    x[0], _ = glo_series(rng, n, 0)
    a = 300 + 2000 * 2 + 20 * 40                                # string 2, symbol 40
    x[0, a:a + 10] = x[0, a + 10:a + 20]                        # meander removed: 10 against 10
    x[1], _ = glo_series(rng, n, 37, flip_rate=0.01, n_zeros=25)
    x[2] = -x[1]
    x.setflags(write=False)
    return x, [0, 37, 37], [15, 15, 15]


@functools.lru_cache(maxsize=None)
def glo_short_scene():
    """2400 epochs: one string, a mark but no room for a string, no mark"""
    rng = np.random.default_rng(78)
    n = 2400
    x = np.stack([glo_series(rng, n, 37)[0], glo_series(rng, n, 500, polarity=-1)[0],
                  800.0 * (2.0 * rng.integers(0, 2, n) - 1)])
    x.setflags(write=False)
    return x, [37, 500, -1], [1, 0, 0]


@functools.lru_cache(maxsize=None)
def b1_scene():
    """30 100 epochs: [0] from 0, five subframes, the second with a preamble sum of exactly 0
    (one symbol split 10 / 10, five of the other ten negated): not negated; [1] from 37,
    inverted, flips and zeros"""
    rng = np.random.default_rng(88)
    n = 30100
    x = np.zeros((2, n))
    x[0], _ = b1_series(rng, n, 0)
    s = 6000
    x[0, s:s + 10] *= -1
    for j in (1, 3, 5, 7, 9):
        x[0, s + 20 * j:s + 20 * j + 20] *= -1
    x[1], _ = b1_series(rng, n, 37, polarity=-1, flip_rate=0.01, n_zeros=25)
    x.setflags(write=False)
    return x, [0, 37], [5, 5]


@functools.lru_cache(maxsize=None)
def b1_short_scene():
    """7000 epochs: one subframe, a preamble without a whole subframe, no preamble"""
    rng = np.random.default_rng(89)
    n = 7000
    x = np.stack([b1_series(rng, n, 100)[0], b1_series(rng, n, 2000, polarity=-1)[0],
                  800.0 * (2.0 * rng.integers(0, 2, n) - 1)])
    x.setflags(write=False)
    return x, [100, 2000, -1], [1, 0, 0]


@functools.lru_cache(maxsize=None)
def literal_results(name):
    """the literal chain's (first, bits) per channel of a scene"""
    scene, fn, kw = {
        "gps": (gps_scene, gps_frames_literal, dict(search_start=GPS_START)),
        "gps_long": (gps_long_scene, gps_frames_literal, {}),
        "glo": (glo_scene, glo_strings_literal, {}),
        "glo_short": (glo_short_scene, glo_strings_literal, {}),
        "b1": (b1_scene, b1_subframes_literal, {}),
        "b1_short": (b1_short_scene, b1_subframes_literal, {}),
    }[name]
    return [fn(x, **kw) for x in scene()[0]]
