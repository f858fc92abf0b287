"""GPS L1 after the data bits: a literal restatement of the Scilab receiver's field decoding
and position fix, a fast restatement vectorised over receivers, and seeded scene generators
(tests/test_navfix_cpu.py holds the two restatements equal; tests/test_navfix_gpu.py holds
csrc/navfix.hip to the literal one).

    GPS/L1/include/ephemeris.sci:82-226          eph_literal, eph_fast
    GPS/L1/postNavigation.sci:117-282            fix_literal, fix_fast
    GPS/L1/calculatePseudoranges.sci:55-72, geoFunctions/satpos.sci:49-147, check_t.sci,
    leastSquarePos.sci:32-111, e_r_corr.sci, topocent.sci, togeod.sci, tropo.sci, cart2geo.sci

Comments carry the files' 1-based indices.  The literal restatement takes the scalar type T
(numpy.float64 or numpy.longdouble): constants are the files' float64 literals in both, only
the operations change.  A \\ omc and inv(A'A) are written in elementary operations: the
normal equations by an LDL' factorisation in column order, with the library's rank rule
(include/gnsscorr.h).  Scilab's two-argument atand is read as (180 / %pi) * atan(y, x).

Tolerances (fp64 outputs behind transcendental functions).  SPREAD is the largest
|literal in float64 - literal in longdouble| per output group over every scene and
measurement of SCENES and of many_rx_scene(); TOL = 16 * SPREAD.  Produced by
    python tests/navfix_scenarios.py
and copied here; test_navfix_cpu.py asserts that a fresh measurement does not exceed them.
SPREAD_WORLD and TOL_WORLD are the same over the scenes of WORLD_SCENES alone
(`python tests/navfix_scenarios.py world`): other sites, the week's edges, other orbit shapes.
"""
import functools

import numpy as np

GPS_PI = 3.1415926535898                    # ephemeris.sci:65, satpos.sci:34
PI = float(np.pi)                           # %pi

EPH_FIELDS = ("T_GD", "t_oc", "a_f2", "a_f1", "a_f0", "C_rs", "deltan", "M_0", "C_uc", "e",
              "C_us", "sqrtA", "t_oe", "C_ic", "omega_0", "C_is", "i_0", "C_rc", "omega",
              "omegaDot", "iDot")
EPH_INTS = ("weekNumber", "accuracy", "health", "IODC", "IODE_sf2", "IODE_sf3", "TOW", "have",
            "status", "reserved")
EPH = np.dtype([(f, "<f8") for f in EPH_FIELDS] + [(f, "<i4") for f in EPH_INTS])
SOL = np.dtype([("X", "<f8"), ("Y", "<f8"), ("Z", "<f8"), ("dt", "<f8"), ("DOP", "<f8", (5,)),
                ("lat", "<f8"), ("lon", "<f8"), ("height", "<f8"), ("status", "<i4"),
                ("n_used", "<i4")])
CHAN = np.dtype([("el", "<f8"), ("az", "<f8"), ("rawP", "<f8"), ("corrP", "<f8"),
                 ("used", "<i4"), ("reserved", "<i4")])
EPH_OK, EPH_SHORT, EPH_UNDECIDED = 0, 1, 2
FIX_OK, FIX_FEW, FIX_RANK = 0, 1, 2

# name: (subframe, ranges (first, last) 1-based, signed, exponent of 2, times gpsPi, added)
FIELDS = {
    "weekNumber": (1, ((61, 70),), 0, 0, 0, 1024), "accuracy": (1, ((73, 76),), 0, 0, 0, 0),
    "health": (1, ((77, 82),), 0, 0, 0, 0), "T_GD": (1, ((197, 204),), 1, -31, 0, 0),
    "IODC": (1, ((83, 84), (197, 204)), 0, 0, 0, 0), "t_oc": (1, ((219, 234),), 0, 4, 0, 0),
    "a_f2": (1, ((241, 248),), 1, -55, 0, 0), "a_f1": (1, ((249, 264),), 1, -43, 0, 0),
    "a_f0": (1, ((271, 292),), 1, -31, 0, 0),
    "IODE_sf2": (2, ((61, 68),), 0, 0, 0, 0), "C_rs": (2, ((69, 84),), 1, -5, 0, 0),
    "deltan": (2, ((91, 106),), 1, -43, 1, 0), "M_0": (2, ((107, 114), (121, 144)), 1, -31, 1, 0),
    "C_uc": (2, ((151, 166),), 1, -29, 0, 0), "e": (2, ((167, 174), (181, 204)), 0, -33, 0, 0),
    "C_us": (2, ((211, 226),), 1, -29, 0, 0),
    "sqrtA": (2, ((227, 234), (241, 264)), 0, -19, 0, 0), "t_oe": (2, ((271, 286),), 0, 4, 0, 0),
    "C_ic": (3, ((61, 76),), 1, -29, 0, 0), "omega_0": (3, ((77, 84), (91, 114)), 1, -31, 1, 0),
    "C_is": (3, ((121, 136),), 1, -29, 0, 0), "i_0": (3, ((137, 144), (151, 174)), 1, -31, 1, 0),
    "C_rc": (3, ((181, 196),), 1, -5, 0, 0), "omega": (3, ((197, 204), (211, 234)), 1, -31, 1, 0),
    "omegaDot": (3, ((241, 264),), 1, -43, 1, 0), "IODE_sf3": (3, ((271, 278),), 0, 0, 0, 0),
    "iDot": (3, ((279, 292),), 1, -43, 1, 0),
}
SIGNED = tuple(k for k, v in FIELDS.items() if v[2])


def field_len(name):
    return sum(b - a + 1 for a, b in FIELDS[name][1])


# ------------------------------------------------------------------ ephemeris.sci, literal
def _bin2dec(v):
    n = 0
    for b in v:
        n = 2 * n + int(b)
    return n


def eph_literal_one(bits, n_bits, first):
    """one channel -> a dict of the EPH record's values"""
    out = {k: 0 for k in EPH_FIELDS + EPH_INTS}
    out.update({k: 0.0 for k in EPH_FIELDS})
    bits = np.asarray(bits)
    if n_bits < 1500 or first < 0:
        out["status"] = EPH_SHORT
        return out
    if (bits[:1500] > 1).any():
        out["status"] = EPH_UNDECIDED
        return out
    gpsPi = GPS_PI
    for i in range(1, 6):                                      # :68
        subframe = bits[300 * (i - 1):300 * i]                 # :71; subframe(k) = subframe[k - 1]
        sub = lambda a, b: subframe[a - 1:b]
        subframeID = _bin2dec(sub(50, 52))                     # :85
        if subframeID == 1:                                    # :92-119
            out["weekNumber"] = _bin2dec(sub(61, 70)) + 1024
            out["accuracy"] = _bin2dec(sub(73, 76))
            out["health"] = _bin2dec(sub(77, 82))
            out["T_GD"] = (_bin2dec(sub(197, 204)) - int(subframe[196]) * 2 ** 8) * 2.0 ** (-31)
            out["IODC"] = _bin2dec(np.r_[sub(83, 84), sub(197, 204)])
            out["t_oc"] = _bin2dec(sub(219, 234)) * 2.0 ** 4
            out["a_f2"] = (_bin2dec(sub(241, 248)) - int(subframe[240]) * 2 ** 8) * 2.0 ** (-55)
            out["a_f1"] = (_bin2dec(sub(249, 264)) - int(subframe[248]) * 2 ** 16) * 2.0 ** (-43)
            out["a_f0"] = (_bin2dec(sub(271, 292)) - int(subframe[270]) * 2 ** 22) * 2.0 ** (-31)
            out["have"] |= 1
        elif subframeID == 2:                                  # :121-159
            out["IODE_sf2"] = _bin2dec(sub(61, 68))
            out["C_rs"] = (_bin2dec(sub(69, 84)) - int(subframe[68]) * 2 ** 16) * 2.0 ** (-5)
            out["deltan"] = (_bin2dec(sub(91, 106)) - int(subframe[90]) * 2 ** 16) \
                * 2.0 ** (-43) * gpsPi
            out["M_0"] = (_bin2dec(np.r_[sub(107, 114), sub(121, 144)])
                          - int(subframe[106]) * 2 ** 32) * 2.0 ** (-31) * gpsPi
            out["C_uc"] = (_bin2dec(sub(151, 166)) - int(subframe[150]) * 2 ** 16) * 2.0 ** (-29)
            out["e"] = _bin2dec(np.r_[sub(167, 174), sub(181, 204)]) * 2.0 ** (-33)
            out["C_us"] = (_bin2dec(sub(211, 226)) - int(subframe[210]) * 2 ** 16) * 2.0 ** (-29)
            out["sqrtA"] = _bin2dec(np.r_[sub(227, 234), sub(241, 264)]) * 2.0 ** (-19)
            out["t_oe"] = _bin2dec(sub(271, 286)) * 2.0 ** 4
            out["have"] |= 2
        elif subframeID == 3:                                  # :161-205
            out["C_ic"] = (_bin2dec(sub(61, 76)) - int(subframe[60]) * 2 ** 16) * 2.0 ** (-29)
            out["omega_0"] = (_bin2dec(np.r_[sub(77, 84), sub(91, 114)])
                              - int(subframe[76]) * 2 ** 32) * 2.0 ** (-31) * gpsPi
            out["C_is"] = (_bin2dec(sub(121, 136)) - int(subframe[120]) * 2 ** 16) * 2.0 ** (-29)
            out["i_0"] = (_bin2dec(np.r_[sub(137, 144), sub(151, 174)])
                          - int(subframe[136]) * 2 ** 32) * 2.0 ** (-31) * gpsPi
            out["C_rc"] = (_bin2dec(sub(181, 196)) - int(subframe[180]) * 2 ** 16) * 2.0 ** (-5)
            out["omega"] = (_bin2dec(np.r_[sub(197, 204), sub(211, 234)])
                            - int(subframe[196]) * 2 ** 32) * 2.0 ** (-31) * gpsPi
            out["omegaDot"] = (_bin2dec(sub(241, 264)) - int(subframe[240]) * 2 ** 24) \
                * 2.0 ** (-43) * gpsPi
            out["IODE_sf3"] = _bin2dec(sub(271, 278))
            out["iDot"] = (_bin2dec(sub(279, 292)) - int(subframe[278]) * 2 ** 14) \
                * 2.0 ** (-43) * gpsPi
            out["have"] |= 4
    out["TOW"] = _bin2dec(subframe[30:47]) * 6 - 30            # :226, the last subframe
    return out


def eph_literal(bits, n_bits, first):
    rec = np.zeros(len(bits), EPH)
    for ch in range(len(bits)):
        for k, v in eph_literal_one(bits[ch], n_bits[ch], first[ch]).items():
            rec[k][ch] = v
    return rec


def eph_fast(bits, n_bits, first):
    """vectorised over channels"""
    bits = np.asarray(bits, np.uint8).reshape(-1, 1500)
    n_ch = len(bits)
    rec = np.zeros(n_ch, EPH)
    short = (np.asarray(n_bits) < 1500) | (np.asarray(first) < 0)
    undec = ~short & (bits > 1).any(axis=1)
    rec["status"] = np.where(short, EPH_SHORT, np.where(undec, EPH_UNDECIDED, EPH_OK))
    ok = ~(short | undec)
    sf = bits.reshape(n_ch, 5, 300).astype(np.int64)

    def value(s, ranges):
        idx = np.concatenate([np.arange(a - 1, b) for a, b in ranges])
        w = 1 << np.arange(len(idx) - 1, -1, -1, dtype=np.int64)
        return s[:, idx] @ w, s[:, idx[0]], len(idx)

    for i in range(5):
        s = sf[:, i]
        sid = s[:, 49] * 4 + s[:, 50] * 2 + s[:, 51]
        for name, (fid, ranges, sgn, ex, pi, add) in FIELDS.items():
            v, firstbit, n = value(s, ranges)
            if sgn:
                v = v - firstbit * (1 << n)
            sel = ok & (sid == fid)
            if name in EPH_INTS:
                rec[name][sel] = (v + add)[sel]
            else:
                x = v.astype(np.float64) * 2.0 ** ex
                if pi:
                    x = x * GPS_PI
                rec[name][sel] = x[sel]
        for fid in (1, 2, 3):
            rec["have"][ok & (sid == fid)] |= 1 << (fid - 1)
    tow, _, _ = value(sf[:, 4], ((31, 47),))
    rec["TOW"][ok] = (tow * 6 - 30)[ok]
    return rec


# ------------------------------------------------------------------ the fix, literal
DEFAULTS = dict(samplesPerCode=16000.0, startOffset=68.802, c=299792458.0, navSolPeriod=500,
                elevationMask=10.0, useTropCorr=1, max_meas=1)   # initSettings.sci:103-125


def settings(**kw):
    s = dict(DEFAULTS)
    s.update(kw)
    return s


def check_t(T, time):                                          # check_t.sci:19-27
    half_week = T(302400)
    if time > half_week:
        return time - 2 * half_week
    if time < -half_week:
        return time + 2 * half_week
    return time


def _rem(T, x, y):                                             # x - fix(x ./ y) .* y
    return x - np.trunc(x / y) * y


def _atand(T, y, x):
    return (T(180) / T(PI)) * np.arctan2(y, x)


def satpos_literal(T, transmitTime, e, mutant=None, trace=None):
    """satpos.sci:56-145 for one satellite; e: a mapping of float64 fields.
    Returns (x, y, z, satClkCorr) and the |dE| of every step of the Kepler loop.  trace: a
    list that receives (time - t_oe, tk), the argument and the value of check_t at :71."""
    gpsPi = T(GPS_PI)
    chk = (lambda T, t: t) if mutant == "check_t_identity" else check_t
    Omegae_dot, GM, F = T(7.2921151467e-5), T(3.986005e14), T(-4.442807633e-10)
    g = lambda k: T(e[k])
    T_GD = T(0) if mutant == "no_tgd" else g("T_GD")
    dt = chk(T, transmitTime - g("t_oc"))                      # :56
    satClkCorr = (g("a_f2") * dt + g("a_f1")) * dt + g("a_f0") - T_GD   # :59-61
    time = transmitTime - satClkCorr                           # :63
    a = g("sqrtA") * g("sqrtA")                                # :68
    tk = chk(T, time - g("t_oe"))                              # :71
    if trace is not None:
        trace.append((time - g("t_oe"), tk))
    n0 = np.sqrt(GM / (a * a * a))                             # :74
    n = n0 + g("deltan")                                       # :76
    M = g("M_0") + n * tk                                      # :79
    M = _rem(T, M + 2 * gpsPi, 2 * gpsPi)                      # :82
    E = M                                                      # :85
    steps = []
    for ii in range(20 if mutant == "kepler_20" else 10):      # :88-97
        E_old = E
        E = M + g("e") * np.sin(E)
        dE = _rem(T, E - E_old, 2 * gpsPi)
        steps.append(abs(dE))
        if abs(dE) < T(1.e-12):
            break
    E = _rem(T, E + 2 * gpsPi, 2 * gpsPi)                      # :101
    dtr = F * g("e") * g("sqrtA") * np.sin(E)                  # :104
    nu = _atand(T, np.sqrt(1 - g("e") * g("e")) * np.sin(E), np.cos(E) - g("e")) / 180 * T(PI)
    phi = nu + g("omega")                                      # :111
    phi = _rem(T, phi, 2 * gpsPi)                              # :114
    u = phi + g("C_uc") * np.cos(2 * phi) + g("C_us") * np.sin(2 * phi)          # :117-119
    r = a * (1 - g("e") * np.cos(E)) + g("C_rc") * np.cos(2 * phi) + g("C_rs") * np.sin(2 * phi)
    i = g("i_0") + g("iDot") * tk + g("C_ic") * np.cos(2 * phi) + g("C_is") * np.sin(2 * phi)
    Omega = g("omega_0") + (g("omegaDot") - Omegae_dot) * tk - Omegae_dot * g("t_oe")   # :130
    Omega = _rem(T, Omega + 2 * gpsPi, 2 * gpsPi)              # :134
    x = np.cos(u) * r * np.cos(Omega) - np.sin(u) * r * np.cos(i) * np.sin(Omega)   # :137-139
    y = np.cos(u) * r * np.sin(Omega) + np.sin(u) * r * np.cos(i) * np.cos(Omega)
    z = np.sin(u) * r * np.sin(i)
    if mutant == "no_dtr":
        dtr = T(0)
    satClkCorr = (g("a_f2") * dt + g("a_f1")) * dt + g("a_f0") - T_GD + dtr      # :143-145
    return (x, y, z, satClkCorr), steps


def togeod_literal(T, X, Y, Z, mutant=None):
    """togeod.sci:32-113 with a = 6378137, finv = 298.257223563 -> (dphi, dlambda) in degrees
    and the residual dP^2 + dZ^2 at the loop's exit"""
    a, finv, tolsq = T(6378137), T(298.257223563), T(1.e-10)
    if mutant == "togeod_abs_z":
        Z = abs(Z)
    rtd = T(180) / T(PI)                                       # :37
    esq = (2 - 1 / finv) / finv                                # :43
    oneesq = 1 - esq
    P = np.sqrt(X * X + Y * Y)                                 # :50
    dlambda = (_atand(T, Y, X) / 180 * T(PI)) * rtd if P > T(1.e-20) else T(0)   # :53-58
    if dlambda < 0:
        dlambda = dlambda + 360
    r = np.sqrt(P * P + Z * Z)                                 # :65
    sinphi = Z / r if r > T(1.e-20) else T(0)
    dphi = np.arcsin(sinphi)                                   # :73
    if r < T(1.e-20):
        return dphi, dlambda, T(0)
    h = r - a * (1 - sinphi * sinphi / finv)                   # :82
    res = T(np.inf)
    for i in range(10):                                        # :85-111
        sinphi = np.sin(dphi)
        cosphi = np.cos(dphi)
        N_phi = a / np.sqrt(1 - esq * sinphi * sinphi)
        dP = P - (N_phi + h) * cosphi
        dZ = Z - (N_phi * oneesq + h) * sinphi
        h = h + (sinphi * dZ + cosphi * dP)
        dphi = dphi + (cosphi * dZ - sinphi * dP) / (N_phi + h)
        res = dP * dP + dZ * dZ
        if res < tolsq:
            break
    return dphi * rtd, dlambda, res


@functools.lru_cache(None)
def tropo_consts(T):
    """tropo.sci:34-56,94-96 for (hsta, p, tkel, hum, hp, htkel, hhum) = (0, 1013, 293, 50, 0, 0, 0):
    ((htop, ref) of the first pass, (htop, ref) of the second)"""
    hsta, p, tkel, hum, hp, htkel, hhum = T(0), T(1013), T(293), T(50), T(0), T(0), T(0)
    tlapse = T(-6.5)
    tkhum = tkel + tlapse * (hhum - htkel)
    atkel = T(7.5) * (tkhum - T(273.15)) / (T(237.3) + tkhum - T(273.15))
    e0 = T(0.0611) * hum * T(10) ** atkel
    tksea = tkel - tlapse * htkel
    em = T(-978.77) / (T(2.8704e6) * tlapse * T(1.0e-5))
    tkelh = tksea + tlapse * hhum
    e0sea = e0 * (tksea / tkelh) ** (4 * em)
    tkelp = tksea + tlapse * hp
    psea = p * (tksea / tkelp) ** em
    refsea = T(77.624e-6) / tksea
    htop1 = T(1.1385e-5) / refsea
    refsea = refsea * psea
    ref1 = refsea * ((htop1 - hsta) / htop1) ** 4
    refsea = (T(371900.0e-6) / tksea - T(12.92e-6)) / tksea
    htop2 = T(1.1385e-5) * (1255 / tksea + T(0.05)) / refsea
    ref2 = refsea * e0sea * ((htop2 - hsta) / htop2) ** 4
    return (htop1, ref1), (htop2, ref2)


def tropo_literal(T, sinel):
    """tropo.sci:47-97 with hsta = 0 and the constants above"""
    a_e, b0, hsta = T(6378.137), T(7.839257e-5), T(0)
    if sinel < 0:
        sinel = T(0)
    tropo = T(0)
    for htop, ref in tropo_consts(T):                          # the two passes of `while 1`
        rtop = (a_e + htop) * (a_e + htop) - (a_e + hsta) * (a_e + hsta) * (1 - sinel * sinel)
        if rtop < 0:
            rtop = T(0)
        rtop = np.sqrt(rtop) - (a_e + hsta) * sinel
        a = -sinel / (htop - hsta)
        b = -b0 * (1 - sinel * sinel) / (htop - hsta)
        rn = [rtop ** (i + 1) for i in range(1, 9)]            # :71-73
        alpha = [2 * a, 2 * a ** 2 + 4 * b / 3, a * (a ** 2 + 3 * b),
                 a ** 4 / 5 + T(2.4) * a ** 2 * b + T(1.2) * b ** 2,
                 2 * a * b * (a ** 2 + 3 * b) / 3,
                 b ** 2 * (6 * a ** 2 + 4 * b) * T(1.428571e-1), T(0), T(0)]
        if b ** 2 > T(1.0e-35):
            alpha[6] = a * b ** 3 / 2
            alpha[7] = b ** 4 / 9
        dot = T(0)
        for k in range(8):
            dot = dot + alpha[k] * rn[k]
        dr = rtop + dot                                        # :84-85
        tropo = tropo + dr * ref * 1000                        # :86
    return tropo


def ldl_factor(T, N):
    """LDL' of the symmetric 4 x 4 N in column order; None when a pivot is not above 1e-12 of
    its column's diagonal entry (the library's rank rule)"""
    tol = T(1.e-12)
    L = [[T(0)] * 4 for _ in range(4)]
    d = [T(0)] * 4
    for j in range(4):
        dj = N[j][j]
        for k in range(j):
            dj = dj - L[j][k] * L[j][k] * d[k]
        if not dj > tol * N[j][j]:
            return None
        d[j] = dj
        for i in range(j + 1, 4):
            v = N[i][j]
            for k in range(j):
                v = v - L[i][k] * L[j][k] * d[k]
            L[i][j] = v / dj
    return L, d


def ldl_solve(T, f, g):
    L, d = f
    z = [T(0)] * 4
    for i in range(4):
        v = g[i]
        for k in range(i):
            v = v - L[i][k] * z[k]
        z[i] = v
    x = [T(0)] * 4
    for i in range(3, -1, -1):
        v = z[i] / d[i]
        for k in range(i + 1, 4):
            v = v - L[k][i] * x[k]
        x[i] = v
    return x


def one_argument_atan(T, Y, X):
    """(Y, X) as the "cart2geo_atan_y_over_x" mutant passes them on to the two-argument form:
    the quadrant-blind angle atan(Y / X), written as atan(-Y, -X) where X < 0 so that where
    X > 0 it is the file's own operation, bit for bit"""
    return (-Y, -X) if X < 0 else (Y, X)


def cart2geo_literal(T, X, Y, Z, mutant=None):
    """cart2geo.sci:22-53 with i = 5"""
    a, f = T(6378137), 1 / T(298.257223563)
    if mutant == "cart2geo_abs_z":
        Z = abs(Z)
    ly, lx = one_argument_atan(T, Y, X) if mutant == "cart2geo_atan_y_over_x" else (Y, X)
    lam = _atand(T, ly, lx) / 180 * T(PI)                      # :26
    ex2 = (2 - f) * f / ((1 - f) * (1 - f))
    c = a * np.sqrt(1 + ex2)
    p = np.sqrt(X * X + Y * Y)
    phi = np.arctan(Z / (p * (1 - (2 - f)) * f))               # :29
    h, oldh = T(0.1), T(0)
    iterations = 0
    while abs(h - oldh) > T(1.e-12):                           # :33-45
        oldh = h
        cp = np.cos(phi)
        N = c / np.sqrt(1 + ex2 * (cp * cp))
        phi = np.arctan(Z / (p * (1 - (2 - f) * f * N / (N + h))))
        h = p / np.cos(phi) - N
        iterations = iterations + 1
        if iterations > 100:
            break
    return phi * 180 / T(PI), lam * 180 / T(PI), h


def lsq_literal(T, satpos, obs, c, useTropCorr, mutant=None, n_iter=7, diag=None):
    """leastSquarePos.sci:32-111.  Returns None for rank(A) ~= 4, else (pos, el, az, dop)."""
    dtr = T(PI) / 180
    pos = [T(0)] * 4
    n = len(obs)
    az, el = [T(0)] * n, [T(0)] * n
    f = None
    for it in range(1, n_iter + 1):                            # :45
        A = [None] * n
        omc = [T(0)] * n
        if it > 1:
            phi, lam, res = togeod_literal(T, pos[0], pos[1], pos[2], mutant)   # topocent.sci:26
            if diag is not None:
                diag["togeod"].append(res)
        for i in range(n):                                     # :47
            X = satpos[i]
            if it == 1:
                Rot_X = [X[0], X[1], X[2]]
                trop = T(0) if mutant == "trop0_first" else T(2)
            else:
                rho2 = (X[0] - pos[0]) * (X[0] - pos[0]) + (X[1] - pos[1]) * (X[1] - pos[1]) + \
                    (X[2] - pos[2]) * (X[2] - pos[2])          # :54-55
                traveltime = np.sqrt(rho2) / c
                if mutant == "no_erot":
                    Rot_X = [X[0], X[1], X[2]]
                else:                                          # e_r_corr.sci:21-32
                    omegatau = T(7.292115147e-5) * traveltime
                    co, so = np.cos(omegatau), np.sin(omegatau)
                    Rot_X = [co * X[0] + so * X[1], -so * X[0] + co * X[1], X[2]]
                dx = [Rot_X[0] - pos[0], Rot_X[1] - pos[1], Rot_X[2] - pos[2]]
                cl, sl = np.cos(lam * dtr), np.sin(lam * dtr)  # topocent.sci:28-31
                cb, sb = np.cos(phi * dtr), np.sin(phi * dtr)
                E = -sl * dx[0] + cl * dx[1] + 0 * dx[2]       # F' * dx, :33-40
                Nn = -sb * cl * dx[0] + -sb * sl * dx[1] + cb * dx[2]
                U = cb * cl * dx[0] + cb * sl * dx[1] + sb * dx[2]
                hor_dis = np.sqrt(E * E + Nn * Nn)
                if hor_dis < T(1.e-20):
                    az[i], el[i] = T(0), T(90)
                else:
                    az[i] = (_atand(T, E, Nn) / 180 * T(PI)) / dtr
                    el[i] = (_atand(T, U, hor_dis) / 180 * T(PI)) / dtr
                if az[i] < 0:
                    az[i] = az[i] + 360
                if useTropCorr == 1 and mutant != "no_trop":   # :64-71
                    trop = tropo_literal(T, np.sin(el[i] * dtr))
                else:
                    trop = T(0)
            d = [Rot_X[0] - pos[0], Rot_X[1] - pos[1], Rot_X[2] - pos[2]]
            omc[i] = obs[i] - np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) - pos[3] - trop
            A[i] = [-d[0] / obs[i], -d[1] / obs[i], -d[2] / obs[i], T(1)]          # :78-81
        N = [[T(0)] * 4 for _ in range(4)]
        g = [T(0)] * 4
        for i in range(n):                                     # A'A and A'omc, row after row
            for r in range(4):
                for s in range(r + 1):
                    N[r][s] = N[r][s] + A[i][r] * A[i][s]
                g[r] = g[r] + A[i][r] * omc[i]
        if diag is not None:
            diag["A"] = np.array(A, np.float64)
        f = ldl_factor(T, N)
        if f is None:                                          # :85-88
            return None
        x = ldl_solve(T, f, g)                                 # :91
        pos = [pos[k] + x[k] for k in range(4)]                # :94
    Q = [ldl_solve(T, f, [T(k == j) for k in range(4)])[j] for j in range(4)]      # :105
    dop = [np.sqrt(Q[0] + Q[1] + Q[2] + Q[3]), np.sqrt(Q[0] + Q[1] + Q[2]), np.sqrt(Q[0] + Q[1]),
           np.sqrt(Q[2]), np.sqrt(Q[3])]
    return pos, el, az, dop


def fix_literal(eph, first, abs_sample, rx_first, cfg, T=np.float64, mutant=None, n_iter=7,
                n_meas_out=None, sol=None, chan=None, diag=None):
    """postNavigation.sci:117-282 per receiver.  abs_sample [n_ch, n_epochs].  Returns n_meas,
    sol [n_rx, max_meas], chan [n_ch, max_meas] as dicts of T arrays (see as_records)."""
    n_rx, n_ch, mm = len(rx_first) - 1, len(eph), cfg["max_meas"]
    n_epochs = abs_sample.shape[1]
    nan, inf = T(np.nan), T(np.inf)
    S = {k: np.zeros((n_rx, mm), T) for k in ("X", "Y", "Z", "dt", "lat", "lon", "height")}
    S["DOP"] = np.zeros((n_rx, mm, 5), T)
    S["status"] = np.zeros((n_rx, mm), np.int32)
    S["n_used"] = np.zeros((n_rx, mm), np.int32)
    S["written"] = np.zeros((n_rx, mm), bool)
    Cn = {k: np.zeros((n_ch, mm), T) for k in ("el", "az", "rawP", "corrP")}
    Cn["used"] = np.zeros((n_ch, mm), np.int32)
    n_meas = np.zeros(n_rx, np.int32)
    c = T(cfg["c"])
    period = int(cfg["navSolPeriod"])
    with np.errstate(all="ignore"):
        for rx in range(n_rx):
            chs = list(range(rx_first[rx], rx_first[rx + 1]))
            decodable = [ch for ch in chs if first[ch] >= 0 and eph["status"][ch] == EPH_OK]
            ready = [ch for ch in decodable if eph["have"][ch] == 7]           # :120-126
            if len(ready) < 4:                                 # :130
                continue
            pmax = max(first[ch] for ch in chs if first[ch] >= 0)
            n_meas[rx] = max(0, min(mm, int((n_epochs - (pmax + 1)) / period)))   # :163
            transmitTime = T(int(eph["TOW"][decodable[-1]]))   # :117,152
            satElev = {ch: inf for ch in chs}                  # :144
            for m in range(n_meas[rx]):
                active = [ch for ch in ready if satElev[ch] >= T(cfg["elevationMask"])]   # :167
                for ch in chs:                                 # :176-177
                    Cn["el"][ch, m] = nan
                    Cn["az"][ch, m] = nan
                    Cn["used"][ch, m] = ch in active
                    Cn["corrP"][ch, m] = 0
                # calculatePseudoranges.sci:55-72
                travelTime = {ch: inf for ch in chs}
                for ch in active:
                    travelTime[ch] = T(abs_sample[ch, first[ch] + period * m]) / \
                        T(cfg["samplesPerCode"])
                minimum = np.floor(min(travelTime.values()))
                for ch in chs:
                    Cn["rawP"][ch, m] = (travelTime[ch] - minimum + T(cfg["startOffset"])) * \
                        (c / 1000)
                sp = []
                for ch in active:                              # :189-191
                    e = {k: eph[k][ch] for k in EPH_FIELDS}
                    s, dE = satpos_literal(T, transmitTime, e, mutant,
                                           None if diag is None else diag.setdefault("tk", []))
                    sp.append(s)
                    if diag is not None:
                        diag["dE"].extend(dE)
                        diag.setdefault("kepler", []).append((len(dE), float(dE[-1])))
                S["written"][rx, m] = True
                S["n_used"][rx, m] = len(active)
                if len(active) > 3:                            # :197
                    obs = [Cn["rawP"][ch, m] + s[3] * c for ch, s in zip(active, sp)]
                    if diag is not None:
                        diag["togeod"] = []
                    r = lsq_literal(T, sp, obs, c, cfg["useTropCorr"], mutant, n_iter, diag)
                    if r is None:                              # the library's widening
                        S["status"][rx, m] = FIX_RANK
                        for k in ("X", "Y", "Z", "dt", "lat", "lon", "height"):
                            S[k][rx, m] = 0
                        S["DOP"][rx, m] = 0
                    else:
                        pos, el, az, dop = r
                        S["X"][rx, m], S["Y"][rx, m], S["Z"][rx, m], S["dt"][rx, m] = pos
                        S["DOP"][rx, m] = dop
                        for i, ch in enumerate(active):        # :205-206
                            Cn["el"][ch, m] = el[i]
                            Cn["az"][ch, m] = az[i]
                        satElev = {ch: Cn["el"][ch, m] for ch in chs}          # :217
                        for ch, s in zip(active, sp):          # :220-222
                            Cn["corrP"][ch, m] = Cn["rawP"][ch, m] + s[3] * c + pos[3]
                        S["lat"][rx, m], S["lon"][rx, m], S["height"][rx, m] = \
                            cart2geo_literal(T, pos[0], pos[1], pos[2], mutant)   # :227-233
                        if diag is not None:
                            diag.setdefault("elev", []).extend(el)
                            diag.setdefault("togeod_all", []).extend(diag["togeod"])
                            diag.setdefault("cond", []).append(np.linalg.cond(diag["A"]))
                            diag.setdefault("gdop", []).append(float(dop[0]))
                else:                                          # :245-269
                    S["status"][rx, m] = FIX_FEW
                    for k in ("X", "Y", "Z", "dt", "lat", "lon", "height"):
                        S[k][rx, m] = nan
                    S["DOP"][rx, m] = 0
                transmitTime = transmitTime + T(period) / 1000 # :280
    return n_meas, S, Cn


def as_records(n_meas, S, Cn, sol=None, chan=None):
    """the literal or fast results as SOL / CHAN records; rows past n_meas keep what `sol`
    and `chan` hold (zeros without them)"""
    n_rx, mm = S["X"].shape
    sol = np.zeros((n_rx, mm), SOL) if sol is None else sol.copy()
    chan = np.zeros(Cn["el"].shape, CHAN) if chan is None else chan.copy()
    w = S["written"]
    for k in ("X", "Y", "Z", "dt", "DOP", "lat", "lon", "height", "status", "n_used"):
        sol[k][w] = S[k][w]
    wc = np.zeros(chan.shape, bool)
    for rx in range(n_rx):
        wc[S["rx_first"][rx]:S["rx_first"][rx + 1]] = w[rx]
    for k in ("el", "az", "rawP", "corrP", "used"):
        chan[k][wc] = Cn[k][wc]
    chan["reserved"][wc] = 0
    return sol, chan


def fix_literal_records(eph, first, abs_sample, rx_first, cfg, sol=None, chan=None, **kw):
    n_meas, S, Cn = fix_literal(eph, first, abs_sample, rx_first, cfg, **kw)
    S["rx_first"] = rx_first
    return (n_meas,) + as_records(n_meas, S, Cn, sol, chan)


# ------------------------------------------------------------------ the fix, fast
def _satpos_fast(t, e):
    """satpos.sci over arrays: t and every field of e of one shape"""
    two_pi = 2 * GPS_PI
    Oe, GM, F = 7.2921151467e-5, 3.986005e14, -4.442807633e-10
    chk = lambda x: np.where(x > 302400.0, x - 604800.0, np.where(x < -302400.0, x + 604800.0, x))
    rem = lambda x, y: x - np.trunc(x / y) * y
    dt = chk(t - e["t_oc"])
    clk = (e["a_f2"] * dt + e["a_f1"]) * dt + e["a_f0"] - e["T_GD"]
    time = t - clk
    a = e["sqrtA"] * e["sqrtA"]
    tk = chk(time - e["t_oe"])
    n = np.sqrt(GM / (a * a * a)) + e["deltan"]
    M = e["M_0"] + n * tk
    M = rem(M + two_pi, two_pi)
    E = M.copy()
    done = np.zeros(E.shape, bool)
    for ii in range(10):
        En = M + e["e"] * np.sin(E)
        dE = rem(En - E, two_pi)
        E = np.where(done, E, En)
        done = done | (np.abs(dE) < 1.e-12)
    E = rem(E + two_pi, two_pi)
    dtr = F * e["e"] * e["sqrtA"] * np.sin(E)
    nu = (180.0 / PI) * np.arctan2(np.sqrt(1 - e["e"] * e["e"]) * np.sin(E),
                                   np.cos(E) - e["e"]) / 180 * PI
    phi = rem(nu + e["omega"], two_pi)
    c2, s2 = np.cos(2 * phi), np.sin(2 * phi)
    u = phi + e["C_uc"] * c2 + e["C_us"] * s2
    r = a * (1 - e["e"] * np.cos(E)) + e["C_rc"] * c2 + e["C_rs"] * s2
    i = e["i_0"] + e["iDot"] * tk + e["C_ic"] * c2 + e["C_is"] * s2
    Om = e["omega_0"] + (e["omegaDot"] - Oe) * tk - Oe * e["t_oe"]
    Om = rem(Om + two_pi, two_pi)
    x = np.cos(u) * r * np.cos(Om) - np.sin(u) * r * np.cos(i) * np.sin(Om)
    y = np.cos(u) * r * np.sin(Om) + np.sin(u) * r * np.cos(i) * np.cos(Om)
    z = np.sin(u) * r * np.sin(i)
    return x, y, z, clk + dtr


def _togeod_fast(X, Y, Z):
    a, finv, tolsq, rtd = 6378137.0, 298.257223563, 1.e-10, 180.0 / PI
    esq = (2 - 1 / finv) / finv
    oneesq = 1 - esq
    P = np.sqrt(X * X + Y * Y)
    lam = np.where(P > 1.e-20, ((180.0 / PI) * np.arctan2(Y, X) / 180 * PI) * rtd, 0.0)
    lam = np.where(lam < 0, lam + 360, lam)
    r = np.sqrt(P * P + Z * Z)
    sinphi = np.where(r > 1.e-20, Z / np.where(r > 1.e-20, r, 1.0), 0.0)
    dphi = np.arcsin(sinphi)
    h = r - a * (1 - sinphi * sinphi / finv)
    done = r < 1.e-20
    small = done.copy()
    for i in range(10):
        sp, cp = np.sin(dphi), np.cos(dphi)
        Np = a / np.sqrt(1 - esq * sp * sp)
        dP = P - (Np + h) * cp
        dZ = Z - (Np * oneesq + h) * sp
        hn = h + (sp * dZ + cp * dP)
        pn = dphi + (cp * dZ - sp * dP) / (Np + hn)
        h = np.where(done, h, hn)
        dphi = np.where(done, dphi, pn)
        done = done | (dP * dP + dZ * dZ < tolsq)
    return np.where(small, dphi, dphi * rtd), lam


def _tropo_fast(sinel):
    a_e, b0 = 6378.137, 7.839257e-5
    sinel = np.where(sinel < 0, 0.0, sinel)
    tropo = np.zeros_like(sinel)
    for htop, ref in tropo_consts(np.float64):
        rtop = (a_e + htop) * (a_e + htop) - (a_e + 0.0) * (a_e + 0.0) * (1 - sinel * sinel)
        rtop = np.where(rtop < 0, 0.0, rtop)
        rtop = np.sqrt(rtop) - (a_e + 0.0) * sinel
        a = -sinel / (htop - 0.0)
        b = -b0 * (1 - sinel * sinel) / (htop - 0.0)
        alpha = [2 * a, 2 * a ** 2 + 4 * b / 3, a * (a ** 2 + 3 * b),
                 a ** 4 / 5 + 2.4 * a ** 2 * b + 1.2 * b ** 2, 2 * a * b * (a ** 2 + 3 * b) / 3,
                 b ** 2 * (6 * a ** 2 + 4 * b) * 1.428571e-1,
                 np.where(b ** 2 > 1.0e-35, a * b ** 3 / 2, 0.0),
                 np.where(b ** 2 > 1.0e-35, b ** 4 / 9, 0.0)]
        dot = np.zeros_like(sinel)
        for k in range(8):
            dot = dot + alpha[k] * rtop ** (k + 2)
        tropo = tropo + (rtop + dot) * ref * 1000
    return tropo


def _ldl_fast(N):
    """N [4][4] of arrays -> L, d, ok (arrays)"""
    L = [[None] * 4 for _ in range(4)]
    d = [None] * 4
    ok = np.ones(N[0][0].shape, bool)
    for j in range(4):
        dj = N[j][j]
        for k in range(j):
            dj = dj - L[j][k] * L[j][k] * d[k]
        ok = ok & (dj > 1.e-12 * N[j][j])
        d[j] = dj
        for i in range(j + 1, 4):
            v = N[i][j]
            for k in range(j):
                v = v - L[i][k] * L[j][k] * d[k]
            L[i][j] = v / dj
    return L, d, ok


def _ldl_solve_fast(L, d, g):
    z = [None] * 4
    for i in range(4):
        v = g[i]
        for k in range(i):
            v = v - L[i][k] * z[k]
        z[i] = v
    x = [None] * 4
    for i in range(3, -1, -1):
        v = z[i] / d[i]
        for k in range(i + 1, 4):
            v = v - L[k][i] * x[k]
        x[i] = v
    return x


def _cart2geo_fast(X, Y, Z):
    a, f = 6378137.0, 1 / 298.257223563
    lam = (180.0 / PI) * np.arctan2(Y, X) / 180 * PI
    ex2 = (2 - f) * f / ((1 - f) * (1 - f))
    c = a * np.sqrt(1 + ex2)
    p = np.sqrt(X * X + Y * Y)
    phi = np.arctan(Z / (p * (1 - (2 - f)) * f))
    h, oldh = np.full(X.shape, 0.1), np.zeros(X.shape)
    it = np.zeros(X.shape, int)
    run = np.abs(h - oldh) > 1.e-12
    while run.any():
        cp = np.cos(phi)
        N = c / np.sqrt(1 + ex2 * (cp * cp))
        pn = np.arctan(Z / (p * (1 - (2 - f) * f * N / (N + h))))
        hn = p / np.cos(pn) - N
        oldh = np.where(run, h, oldh)
        phi = np.where(run, pn, phi)
        h = np.where(run, hn, h)
        it = it + run
        run = run & (it <= 100) & (np.abs(h - oldh) > 1.e-12)
    return phi * 180 / PI, lam * 180 / PI, h


def fix_fast(eph, first, abs_sample, rx_first, cfg):
    """fix_literal in float64, vectorised over receivers: arrays [n_rx, W], W the largest
    receiver; sums over a receiver's channels run in channel order with zeros for the
    channels outside the active set, which is the literal sum."""
    rx_first = np.asarray(rx_first)
    first = np.asarray(first)
    n_rx, n_ch, mm = len(rx_first) - 1, len(eph), cfg["max_meas"]
    n_epochs = abs_sample.shape[1]
    size = np.diff(rx_first)
    W = int(size.max())
    lane = np.arange(W)
    valid = lane[None, :] < size[:, None]
    chi = np.where(valid, rx_first[:-1, None] + lane[None, :], 0)
    e = {k: eph[k][chi] for k in EPH_FIELDS}
    fs = np.where(valid, first[chi], -1)
    decodable = valid & (fs >= 0) & (eph["status"][chi] == EPH_OK)
    ready = decodable & (eph["have"][chi] == 7)
    period, c = int(cfg["navSolPeriod"]), cfg["c"]
    pmax = fs.max(axis=1)
    n_meas = np.where(ready.sum(axis=1) >= 4,
                      np.clip(np.trunc((n_epochs - (pmax + 1)) / period).astype(int), 0, mm), 0)
    seed = np.where(decodable.any(axis=1), W - 1 - np.argmax(decodable[:, ::-1], axis=1), 0)
    t = eph["TOW"][chi][np.arange(n_rx), seed].astype(np.float64)
    S = {k: np.zeros((n_rx, mm)) for k in ("X", "Y", "Z", "dt", "lat", "lon", "height")}
    S["DOP"] = np.zeros((n_rx, mm, 5))
    S["status"] = np.zeros((n_rx, mm), np.int32)
    S["n_used"] = np.zeros((n_rx, mm), np.int32)
    S["written"] = np.zeros((n_rx, mm), bool)
    Cn = {k: np.zeros((n_ch, mm)) for k in ("el", "az", "rawP", "corrP")}
    Cn["used"] = np.zeros((n_ch, mm), np.int32)
    satElev = np.full((n_rx, W), np.inf)
    dtr = PI / 180
    with np.errstate(all="ignore"):
        for m in range(int(n_meas.max(initial=0))):
            live = n_meas > m
            active = ready & (satElev >= cfg["elevationMask"]) & live[:, None]
            n_act = active.sum(axis=1)
            idx = np.clip(fs + period * m, 0, n_epochs - 1)
            travel = np.where(active, abs_sample[chi, idx] / cfg["samplesPerCode"], np.inf)
            minimum = np.floor(travel.min(axis=1))
            rawP = (travel - minimum[:, None] + cfg["startOffset"]) * (c / 1000)
            sx, sy, sz, clk = _satpos_fast(t[:, None] + np.zeros((1, W)), e)
            obs = rawP + clk * c
            full = live & (n_act > 3)
            pos = np.zeros((4, n_rx))
            el = np.full((n_rx, W), np.nan)
            az = np.full((n_rx, W), np.nan)
            rank_ok = np.ones(n_rx, bool)
            L = d = None
            for it in range(7):
                if it == 0:
                    r0, r1, r2 = sx, sy, sz
                    trop = np.full((n_rx, W), 2.0)
                else:
                    P0, P1, P2 = pos[0][:, None], pos[1][:, None], pos[2][:, None]
                    rho2 = (sx - P0) * (sx - P0) + (sy - P1) * (sy - P1) + (sz - P2) * (sz - P2)
                    omegatau = 7.292115147e-5 * (np.sqrt(rho2) / c)
                    co, so = np.cos(omegatau), np.sin(omegatau)
                    r0, r1, r2 = co * sx + so * sy, -so * sx + co * sy, sz
                    phi, lam = _togeod_fast(pos[0], pos[1], pos[2])
                    cl, sl = np.cos(lam * dtr)[:, None], np.sin(lam * dtr)[:, None]
                    cb, sb = np.cos(phi * dtr)[:, None], np.sin(phi * dtr)[:, None]
                    d0, d1, d2 = r0 - P0, r1 - P1, r2 - P2
                    E = -sl * d0 + cl * d1 + 0 * d2
                    Nn = -sb * cl * d0 + -sb * sl * d1 + cb * d2
                    U = cb * cl * d0 + cb * sl * d1 + sb * d2
                    hd = np.sqrt(E * E + Nn * Nn)
                    az_n = np.where(hd < 1.e-20, 0.0, ((180.0 / PI) * np.arctan2(E, Nn) / 180 * PI) / dtr)
                    el_n = np.where(hd < 1.e-20, 90.0, ((180.0 / PI) * np.arctan2(U, hd) / 180 * PI) / dtr)
                    az_n = np.where(az_n < 0, az_n + 360, az_n)
                    upd = (full & rank_ok)[:, None]
                    az, el = np.where(upd, az_n, az), np.where(upd, el_n, el)
                    trop = _tropo_fast(np.sin(el_n * dtr)) if cfg["useTropCorr"] == 1 \
                        else np.zeros((n_rx, W))
                P0, P1, P2 = pos[0][:, None], pos[1][:, None], pos[2][:, None]
                d0, d1, d2 = r0 - P0, r1 - P1, r2 - P2
                omc = obs - np.sqrt(d0 * d0 + d1 * d1 + d2 * d2) - pos[3][:, None] - trop
                A = [np.where(active, -d0 / obs, 0.0), np.where(active, -d1 / obs, 0.0),
                     np.where(active, -d2 / obs, 0.0), np.where(active, 1.0, 0.0)]
                omc = np.where(active, omc, 0.0)
                N = [[np.zeros(n_rx) for _ in range(4)] for _ in range(4)]
                g = [np.zeros(n_rx) for _ in range(4)]
                for w in range(W):
                    for r in range(4):
                        for s in range(r + 1):
                            N[r][s] = N[r][s] + A[r][:, w] * A[s][:, w]
                        g[r] = g[r] + A[r][:, w] * omc[:, w]
                Ln, dn, ok = _ldl_fast(N)
                step = full & rank_ok & ok
                x = _ldl_solve_fast(Ln, dn, g)
                if L is None:
                    L, d = Ln, dn
                else:
                    L = [[None if Ln[i][j] is None else np.where(step, Ln[i][j], L[i][j])
                          for j in range(4)] for i in range(4)]
                    d = [np.where(step, dn[j], d[j]) for j in range(4)]
                pos = np.where(step[None, :], pos + np.array(x), pos)
                rank_ok = rank_ok & (ok | ~full)
            good = full & rank_ok
            bad = full & ~rank_ok
            few = live & ~full
            Q = [_ldl_solve_fast(L, d, [np.full(n_rx, float(k == j)) for k in range(4)])[j]
                 for j in range(4)]
            dop = np.stack([np.sqrt(Q[0] + Q[1] + Q[2] + Q[3]), np.sqrt(Q[0] + Q[1] + Q[2]),
                            np.sqrt(Q[0] + Q[1]), np.sqrt(Q[2]), np.sqrt(Q[3])], axis=1)
            lat, lon, hgt = _cart2geo_fast(np.where(good, pos[0], 1.0), np.where(good, pos[1], 1.0),
                                           np.where(good, pos[2], 1.0))
            for k, v in (("X", pos[0]), ("Y", pos[1]), ("Z", pos[2]), ("dt", pos[3]),
                         ("lat", lat), ("lon", lon), ("height", hgt)):
                S[k][:, m] = np.where(good, v, np.where(few, np.nan, 0.0))
            S["DOP"][:, m] = np.where(good[:, None], dop, 0.0)
            S["status"][:, m] = np.where(good, FIX_OK, np.where(bad, FIX_RANK, FIX_FEW))
            S["n_used"][:, m] = n_act
            S["written"][:, m] = live
            el_out = np.where(good[:, None] & active, el, np.nan)
            az_out = np.where(good[:, None] & active, az, np.nan)
            satElev = np.where(good[:, None], el_out, satElev)
            corrP = np.where(good[:, None] & active, rawP + clk * c + pos[3][:, None], 0.0)
            sel = valid & live[:, None]
            for k, v in (("el", el_out), ("az", az_out), ("rawP", rawP), ("corrP", corrP),
                         ("used", active)):
                Cn[k][chi[sel], m] = v[sel]
            t = t + period / 1000
    S["rx_first"] = rx_first
    return n_meas.astype(np.int32), S, Cn


# ------------------------------------------------------------------ scene generators
def eph_ints(rng, kind="random"):
    """the raw field integers of one ephemeris on the ICD grid (unsigned bit patterns)"""
    raw = {k: int(rng.integers(0, 1 << field_len(k))) for k in FIELDS}
    if kind == "ones":
        raw.update({k: (1 << field_len(k)) - 1 for k in SIGNED})
    elif kind == "signbit":
        raw.update({k: 1 << (field_len(k) - 1) for k in SIGNED})
    elif kind == "negative":
        raw.update({k: raw[k] | 1 << (field_len(k) - 1) for k in SIGNED})
    # IODC's low 8 bits are T_GD's bits in this file (ephemeris.sci:105 reads 197:204 again)
    raw["IODC"] = (raw["IODC"] >> 8 << 8) | raw["T_GD"]
    return raw


def raw_to_values(raw):
    out = {}
    for k, (sf, ranges, sgn, ex, pi, add) in FIELDS.items():
        n = field_len(k)
        v = raw[k] - (raw[k] >> (n - 1)) * (1 << n) if sgn else raw[k]
        if k in EPH_INTS:
            out[k] = v + add
        else:
            x = float(v) * 2.0 ** ex
            out[k] = x * GPS_PI if pi else x
    return out


def values_to_raw(vals):
    """the nearest grid integers of physical values (the orbit generator)"""
    raw = {}
    for k, (sf, ranges, sgn, ex, pi, add) in FIELDS.items():
        n = field_len(k)
        if k in EPH_INTS:
            v = int(vals.get(k, add)) - add
        else:
            v = int(round(vals.get(k, 0.0) / (2.0 ** ex * (GPS_PI if pi else 1.0))))
        lo, hi = (-(1 << (n - 1)), (1 << (n - 1)) - 1) if sgn else (0, (1 << n) - 1)
        raw[k] = min(max(v, lo), hi) & ((1 << n) - 1)
    raw["IODC"] = (raw["IODC"] >> 8 << 8) | raw["T_GD"]
    return raw


def subframe_bits(rng, sid, raw, tow_count):
    """300 bits of a subframe with ID sid as they stand after checkPhase: the fields of `raw`
    that belong to it, the TOW count in 31:47, everything else random"""
    b = rng.integers(0, 2, 300).astype(np.uint8)
    put = lambda a, v, n: b.__setitem__(slice(a - 1, a - 1 + n),
                                        [(v >> (n - 1 - i)) & 1 for i in range(n)])
    put(1, 0b10001011, 8)                                      # the preamble
    put(31, tow_count, 17)
    put(50, sid, 3)
    order = [k for k in FIELDS if k != "IODC"] + []            # IODC's tail is T_GD's
    for k in order:
        sf, ranges, *_ = FIELDS[k]
        if sf != sid:
            continue
        n, v = field_len(k), raw[k]
        for a, z in ranges:
            ln = z - a + 1
            n -= ln
            put(a, (v >> n) & ((1 << ln) - 1), ln)
    if sid == 1:
        put(83, raw["IODC"] >> 8, 2)
    return b


def frame_bits(rng, ids, raw, tow_count=1000):
    """[1500] bits: five subframes with the IDs `ids`; a repeated ID carries other field values
    the first time, so the later one must win"""
    out = []
    for j, sid in enumerate(ids):
        r = raw
        if sid in ids[j + 1:]:
            r = eph_ints(rng)
        out.append(subframe_bits(rng, sid, r, tow_count + j))
    return np.concatenate(out)


ORDERS = ((1, 2, 3, 4, 5), (3, 4, 5, 1, 2), (1, 1, 2, 3, 4), (4, 2, 3, 4, 5), (1, 5, 3, 4, 5),
          (1, 2, 4, 5, 6), (0, 7, 1, 2, 3))


@functools.lru_cache(None)
def eph_scene(n_ch, seed=11):
    """bits [n_ch, 1500], n_bits, first, planted raw integers per channel: every order of ORDERS
    in turn, the four kinds of field patterns in turn; refusals spread over the channels when
    there are enough of them"""
    rng = np.random.default_rng(seed)
    kinds = ("random", "negative", "ones", "signbit")
    bits = np.zeros((n_ch, 1500), np.uint8)
    raws = []
    n_bits = np.full(n_ch, 1500, np.int32)
    first = rng.integers(40, 9000, n_ch).astype(np.int32)
    for ch in range(n_ch):
        raw = eph_ints(rng, kinds[ch % 4])
        raws.append(raw)
        bits[ch] = frame_bits(rng, ORDERS[ch % len(ORDERS)], raw, int(rng.integers(0, 100000)))
    if n_ch >= 3:
        n_bits[1] = 1200
        bits[1, 1200:] = 0
    if n_ch >= 16:
        n_bits[8] = 0
        bits[8] = 0
        first[9] = -1
        bits[10, 60 + 3] = 2                                   # inside weekNumber
        bits[11, 299] = 2                                      # a parity bit: outside every field
        bits[12, 1499] = 2
    return bits, n_bits, first, tuple(raws)


# orbit and geometry ---------------------------------------------------------
# near 60 N: there togeod's residual passes its 1e-10 exit by a factor of 70 and more
RX_ECEF = (1911300.0, -2548400.0, 5517448.0)


def _elevation(pos, sat):
    phi, lam, _ = togeod_literal(np.float64, *map(np.float64, pos))
    d2r = PI / 180
    cl, sl, cb, sb = np.cos(lam * d2r), np.sin(lam * d2r), np.cos(phi * d2r), np.sin(phi * d2r)
    dx = np.asarray(sat[:3], np.float64) - np.asarray(pos, np.float64)
    E = -sl * dx[0] + cl * dx[1]
    N = -sb * cl * dx[0] - sb * sl * dx[1] + cb * dx[2]
    U = cb * cl * dx[0] + cb * sl * dx[1] + sb * dx[2]
    return np.degrees(np.arctan2(U, np.hypot(E, N)))


def _near(v, t):
    v = np.asarray(v, np.float64)
    return bool(((v > t / 4) & (v < t * 4)).any())


def _gdop(pos, sats):
    A = np.array([np.r_[-(np.array(s[:3], float) - pos) / np.linalg.norm(np.array(s[:3], float) - pos),
                        1.0] for s in sats])
    return float(np.sqrt(np.trace(np.linalg.inv(A.T @ A))))


def site_ecef(site):
    """(latitude, longitude) in degrees -> the point of the 6371 km sphere there"""
    lat, lon = np.radians(site[0]), np.radians(site[1])
    return 6371000.0 * np.array([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon),
                                 np.sin(lat)])


def full_kepler_loop(steps):
    """the loop ran its 10 steps and left by the cap, its last |dE| a factor 4 above the exit"""
    return len(steps) == 10 and steps[-1] > 4e-12


def draw_satellite(rng, tow, pos, el_lo, el_hi, span=4.0, e=(0.001, 0.02), i_0=None, toe=None):
    """a GPS-like orbit on the ICD grid whose elevation from pos at tow lies in [el_lo, el_hi]
    and whose Kepler loop, at tow and `span` seconds on, takes no step with |dE| within a
    factor 4 of its 1e-12 exit.  e, i_0: the ranges the eccentricity and the inclination [rad]
    are drawn from (i_0 None: 0.96 +- 0.03); from e = 0.1 on only orbits whose loop runs all
    10 steps are kept.  toe: t_oe = t_oc (None: the next 2-hour boundary).  Returns the raw
    integers and the position at tow."""
    toe = tow - tow % 7200 + 7200 if toe is None else toe
    while True:
        vals = dict(sqrtA=5153.6 + rng.uniform(-0.5, 0.5), e=rng.uniform(*e),
                    i_0=0.96 + rng.uniform(-0.03, 0.03) if i_0 is None else rng.uniform(*i_0),
                    omega_0=rng.uniform(-PI, PI),
                    omega=rng.uniform(-PI, PI), M_0=rng.uniform(-PI, PI),
                    deltan=rng.uniform(3e-9, 6e-9), omegaDot=rng.uniform(-9e-9, -7e-9),
                    iDot=rng.uniform(-5e-10, 5e-10), t_oe=toe,
                    t_oc=toe, a_f0=rng.uniform(-5e-4, 5e-4),
                    a_f1=rng.uniform(-1e-11, 1e-11), a_f2=0.0, T_GD=rng.uniform(-2e-8, 2e-8),
                    weekNumber=1024 + int(rng.integers(0, 1024)), IODC=int(rng.integers(0, 1024)),
                    IODE_sf2=int(rng.integers(0, 256)), IODE_sf3=int(rng.integers(0, 256)),
                    **{k: rng.uniform(-1e-6, 1e-6) for k in ("C_uc", "C_us", "C_ic", "C_is")},
                    **{k: rng.uniform(-100, 100) for k in ("C_rc", "C_rs")})
        raw = values_to_raw(vals)
        s, dE = satpos_literal(np.float64, np.float64(tow), raw_to_values(raw))
        dE2 = satpos_literal(np.float64, np.float64(tow + span), raw_to_values(raw))[1]
        if e[0] >= 0.1 and not (full_kepler_loop(dE) and full_kepler_loop(dE2)):
            continue
        if el_lo <= _elevation(pos, s) <= el_hi and not _near(dE + dE2, 1e-12):
            return raw, s


def plant_abs_samples(eph, first, chans, tow, pos, cfg, n_epochs, n_meas, trop, offset_ms=0.3):
    """absoluteSample rows [len(chans), n_epochs] for one receiver at `pos`: at measurement m
    every channel's pseudorange is range + troposphere + a common clock term chosen so that the
    smallest travel time sits offset_ms above a whole millisecond.  Other epochs hold NaN."""
    T = np.float64
    c, spc, period = T(cfg["c"]), cfg["samplesPerCode"], cfg["navSolPeriod"]
    out = np.full((len(chans), n_epochs), np.nan)
    for m in range(n_meas):
        t = T(tow) + m * (T(period) / 1000)
        rawp = []
        for ch in chans:
            e = {k: eph[k][ch] for k in EPH_FIELDS}
            (x, y, z, clk), _ = satpos_literal(T, t, e)
            rho = T(2.2e7)
            for _ in range(8):                                 # fixed point of the rotation
                w = T(7.292115147e-5) * (rho / c)
                rx = [np.cos(w) * x + np.sin(w) * y, -np.sin(w) * x + np.cos(w) * y, z]
                rho = np.sqrt(sum((rx[k] - pos[k]) ** 2 for k in range(3)))
            tr = tropo_literal(T, np.sin(np.radians(_elevation(pos, rx)))) if trop else T(0)
            rawp.append(rho + tr - clk * c)
        rawp = np.array(rawp) / (c / 1000)                     # ms, up to the clock term
        ms = rawp - rawp.min() + offset_ms                     # abs / spc - K
        for i, ch in enumerate(chans):
            out[i, first[ch] + period * m] = (ms[i] + (1000 + period * m)) * spc
    return out


WEEK = 604800


def make_fix_scene(seed, sizes, n_epochs=200, period=20, max_meas=7, trop=1, low=(), no_sf2=(),
                   not_ready=(), clone=(), first_lo=40, first_hi=55, sites=None, week=None,
                   e=(0.001, 0.02), i_0=None):
    """sizes: channels per receiver.  low: {receiver: number of satellites between 3 and 7
    degrees}: in the first fix, then out.  no_sf2 / not_ready: (receiver, lane) pairs whose
    frame has no subframe 2 / whose first_subframe is -1.  clone: receivers in which every
    channel carries channel 0's ephemeris and absoluteSample (rank 1).  sites: (latitude,
    longitude) in degrees per receiver, in place of RX_ECEF; the 200 km of jitter and the
    rescaling to 6371 km stay.  week: "end" puts TOW into the last 15 minutes of the week with
    t_oe = t_oc = 0 (check_t subtracts a week), "start" into the first 15 minutes with
    t_oe = t_oc = 597600 (check_t adds one).  e, i_0: draw_satellite's ranges."""
    rng = np.random.default_rng(seed)
    cfg = settings(navSolPeriod=period, max_meas=max_meas, useTropCorr=trop)
    rx_first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n_ch = int(rx_first[-1])
    bits = np.zeros((n_ch, 1500), np.uint8)
    first = rng.integers(first_lo, first_hi, n_ch).astype(np.int32)
    planted = []
    toe = None
    if week == "end":                                          # TOW = 6 count - 6 below
        tow_count, toe = WEEK // 6 + 1 - int(rng.integers(10, 150)), 0
    elif week == "start":
        tow_count, toe = 1 + int(rng.integers(10, 150)), WEEK - 7200
    else:
        tow_count = int(rng.integers(1000, 90000))
    tow = tow_count * 6 - 30 + 24                              # the fifth subframe's count is + 4
    for rx, size in enumerate(sizes):
        pos = (np.array(RX_ECEF) if sites is None else site_ecef(sites[rx])) + \
            rng.uniform(-2e5, 2e5, 3)
        pos *= 6371000.0 / np.linalg.norm(pos)
        planted.append(pos)
        n_low = dict(low).get(rx, 0)
        while True:                                            # a geometry with GDOP < 5
            drawn = [draw_satellite(rng, tow, pos, *((3.0, 7.0) if lane >= size - n_low
                                                     else (18.0, 85.0)), e=e, i_0=i_0, toe=toe)
                     for lane in range(size)]
            use = [lane for lane in range(size)
                   if (rx, lane) not in no_sf2 and (rx, lane) not in not_ready]
            high = [lane for lane in use if lane < size - n_low]
            if len(use) < 4 or rx in clone:
                break
            if _gdop(pos, [drawn[l][1] for l in use]) < 5 and \
                    (len(high) < 4 or _gdop(pos, [drawn[l][1] for l in high]) < 5):
                break
        for lane in range(size):
            ch = rx_first[rx] + lane
            raw = drawn[lane][0]
            ids = (1, 4, 3, 4, 5) if (rx, lane) in no_sf2 else ORDERS[ch % 3]
            bits[ch] = frame_bits(rng, ids, raw, tow_count)
            if (rx, lane) in not_ready:
                first[ch] = -1
        if rx in clone:
            for lane in range(1, size):
                bits[rx_first[rx] + lane] = bits[rx_first[rx]]
                first[rx_first[rx] + lane] = first[rx_first[rx]]
    n_bits = np.full(n_ch, 1500, np.int32)
    eph = eph_fast(bits, n_bits, first)
    abs_sample = np.full((n_ch, n_epochs), np.nan)
    for rx, size in enumerate(sizes):
        chans = [ch for ch in range(rx_first[rx], rx_first[rx + 1])
                 if first[ch] >= 0 and eph["have"][ch] == 7]
        pm = max([first[ch] for ch in range(rx_first[rx], rx_first[rx + 1]) if first[ch] >= 0],
                 default=0)
        nm = max(0, min(max_meas, (n_epochs - (pm + 1)) // period))
        if chans:
            abs_sample[chans] = plant_abs_samples(eph, first, chans, tow, planted[rx], cfg,
                                                  n_epochs, nm, trop)
        if rx in clone:
            for ch in range(rx_first[rx] + 1, rx_first[rx + 1]):
                abs_sample[ch] = abs_sample[rx_first[rx]]
    return dict(bits=bits, n_bits=n_bits, first=first, eph=eph, abs_sample=abs_sample,
                rx_first=rx_first, cfg=cfg, planted=np.array(planted), sizes=tuple(sizes))


SCENES = {
    # name: (arguments of make_fix_scene, multi-measurement full-rank scene)
    "one_rx_4": (dict(seed=1, sizes=(4,), max_meas=2), True),
    "one_rx_5": (dict(seed=2, sizes=(5,), max_meas=7), True),
    "three_rx": (dict(seed=3, sizes=(12, 4, 7), max_meas=2), True),
    "wave64": (dict(seed=4, sizes=(64,), max_meas=1, n_epochs=120), False),
    "notrop": (dict(seed=5, sizes=(6, 9), max_meas=2, trop=0), True),
    "drop_one": (dict(seed=6, sizes=(7,), max_meas=3, low={0: 1}), True),
    "five_to_three": (dict(seed=7, sizes=(5, 5), max_meas=3, low={0: 2}), False),
    "few_ready": (dict(seed=8, sizes=(5, 6), max_meas=2, not_ready=((0, 1), (0, 3))), False),
    "seed_from_excluded": (dict(seed=9, sizes=(6,), max_meas=2, no_sf2=((0, 5),)), True),
    "rank": (dict(seed=10, sizes=(5, 6), max_meas=2, clone=(0,)), False),
    "max_meas_below": (dict(seed=12, sizes=(5,), max_meas=2, n_epochs=300), True),
    "one_meas": (dict(seed=13, sizes=(8,), max_meas=1, n_epochs=80), False),
}


# name: (latitude, longitude) the receiver starts from, what its solved latitude and longitude
# must show.  The two meridians hold two receivers each, and the seed is one whose jitter puts
# them on either side.  The southern sites stand at 17 S: between 33 S and 37 S togeod's exit
# residual lies at 0.5 to 1 times its 1e-10 threshold, so one last bit of sin / cos decides
# the number of its steps there, in the reference itself.
SITES = {
    "north_east": ((48.0, 11.0), lambda lat, lon: lat > 0 and lon > 0),
    "south_east": ((-17.0, 150.0), lambda lat, lon: lat < 0 and lon > 0),
    "south_west": ((-17.0, -70.0), lambda lat, lon: lat < 0 and lon < 0),
    "meridian_180_east": ((-17.0, 179.2), lambda lat, lon: lat < 0 and lon > 177),
    "meridian_180_west": ((-17.0, 179.2), lambda lat, lon: lat < 0 and lon < -177),
    "meridian_0_west": ((51.0, -0.3), lambda lat, lon: lat > 0 and -3 < lon < 0),
    "meridian_0_east": ((51.0, -0.3), lambda lat, lon: lat > 0 and 0 < lon < 3),
    "equator": ((0.4, 101.0), lambda lat, lon: abs(lat) < 2.5 and lon > 0),
    "arctic": ((84.0, -30.0), lambda lat, lon: lat > 80 and lon < 0),
    "antarctic": ((-82.0, 70.0), lambda lat, lon: lat < -80 and lon > 0),
    "control": ((60.0, -53.0), lambda lat, lon: lat > 0 and lon < 0),
}
WORLD_SIZES = (6, 5, 7, 4, 5, 8, 5, 6, 4, 7, 5)                # one receiver per site, in order


def world_sites(moved=None):
    """the (latitude, longitude) of SITES in order, with those of `moved` in their place"""
    return tuple(dict(moved or {}).get(k, v[0]) for k, v in SITES.items())


# the scenes that reach what SCENES does not: sites in every quadrant in one launch, the
# week's two edges, Kepler loops that leave by the cap, inclinations from 0.3 to 1.4 rad.  Every
# seed is the first, counting up from the hundred it starts with, at which the scene passes
# conditions_hold and shows what it is named for (search_seed: world took 36 seeds, most of them
# for the jitter to put the meridians' receivers on either side; inclined 2); no site was moved.
# useTropCorr is one setting per launch: the troposphere is on for all eleven receivers, and
# SCENES' "notrop" stays the case without it.
WORLD_SCENES = {
    "world": (dict(seed=135, sizes=WORLD_SIZES, max_meas=2, sites=world_sites()), True),
    "week_end": (dict(seed=200, sizes=(6,), max_meas=2, trop=0, week="end"), True),
    "week_start": (dict(seed=300, sizes=(5,), max_meas=2, trop=0, week="start"), True),
    "eccentric": (dict(seed=400, sizes=(6,), max_meas=2, e=(0.1, 0.3)), True),
    "inclined": (dict(seed=501, sizes=(8,), max_meas=2, i_0=(0.3, 1.4)), True),
}


@functools.lru_cache(None)
def fix_scene(name):
    return make_fix_scene(**(SCENES.get(name) or WORLD_SCENES[name])[0])


def site_classes_missed(lat, lon):
    """the sites of SITES whose class a solved (lat, lon) [n_rx, max_meas] of a world scene
    does not show"""
    return [k for (k, (_, rule)), las, los in zip(SITES.items(), lat, lon)
            if not all(rule(la, lo) for la, lo in zip(las, los))]


@functools.lru_cache(None)
def many_rx_scene(n_rx=65, seed=21):
    """n_rx receivers of unequal size (4 .. 9 channels) in one launch"""
    sizes = tuple(4 + (i * 5) % 6 for i in range(n_rx))
    return make_fix_scene(seed, sizes, max_meas=2)


@functools.lru_cache(None)
def literal_result(name, T=np.float64, mutant=None):
    s = many_rx_scene() if name == "many" else fix_scene(name)
    n_meas, S, Cn = fix_literal(s["eph"], s["first"], s["abs_sample"], s["rx_first"], s["cfg"], T,
                                mutant)
    S["rx_first"] = s["rx_first"]
    return n_meas, S, Cn


def scene_diagnostics(s):
    """what the scene conditions are asserted on, from the literal restatement in float64:
    cond(A) and GDOP of every solved measurement, every elevation, the |dE| at every exit of
    the Kepler loop and the residual at every exit of togeod's loop"""
    diag = {"dE": []}
    fix_literal(s["eph"], s["first"], s["abs_sample"], s["rx_first"], s["cfg"], diag=diag)
    return {k: np.array(diag.get(k, []), np.float64)
            for k in ("cond", "gdop", "elev", "dE", "togeod_all", "tk", "kepler")}


def conditions_hold(s, full_rank=True, mask=10.0):
    d = scene_diagnostics(s)
    ok = not _near(d["dE"][np.isfinite(d["dE"])], 1e-12) and not _near(d["togeod_all"], 1e-10)
    ok = ok and not (np.abs(d["elev"] - mask) < 1e-6).any()
    if full_rank:
        ok = ok and (d["cond"] < 1e6).all() and (d["gdop"] < 6).all()
    return bool(ok)


@functools.lru_cache(None)
def chain_scene(seed=41, n_ch=8, n_epochs=31000, max_meas=3):
    """One receiver for the whole device chain: the six sums per epoch whose I_P carries each
    channel's five subframes as transmitted words with valid parity (the frame's bits 1-24 of
    every word are the source bits, navbits_scenarios.gps_encode_word), starting at the
    channel's first_subframe, and the tracker start positions that put absoluteSample at the
    first measurement near the planted geometry (to the tracker loop's own fraction of a
    sample).  Returns the fix scene, sums [n_ch, n_epochs, 6] and pos0 [n_ch]."""
    import navbits_scenarios as NB
    s = make_fix_scene(seed, (n_ch,), n_epochs=n_epochs, period=20, max_meas=max_meas,
                       first_lo=120, first_hi=400)
    rng = np.random.default_rng(seed + 1)
    sums = np.zeros((n_ch, n_epochs, 6))
    pos0 = np.zeros(n_ch, np.int64)
    for ch in range(n_ch):
        start = int(s["first"][ch])
        lead = start % 20
        n_bits = (n_epochs - lead) // 20 + 1
        tx = rng.integers(0, 2, n_bits)
        b0 = (start - lead) // 20
        for w in range((n_bits - b0) // 30):
            at = b0 + 30 * w
            d24 = s["bits"][ch, 30 * w:30 * w + 24].astype(int) if w < 50 \
                else rng.integers(0, 2, 24)
            tx[at:at + 30] = NB.gps_encode_word(d24, tx[at - 2], tx[at - 1])
        x = np.repeat(2.0 * tx - 1, 20)
        x = np.concatenate([2.0 * rng.integers(0, 2, lead) - 1, x])[:n_epochs]
        x = 1000.0 * x * (1.0 + 0.2 * rng.random(n_epochs))
        q = 10.0 * rng.standard_normal(n_epochs)
        sums[ch] = np.stack([0.5 * x, x, 0.5 * x, 0.5 * q, q, 0.5 * q], axis=1)
        pos0[ch] = int(round(s["abs_sample"][ch, start])) - 16000 * (start + 1)
    return s, sums, pos0


GROUPS = {"xyz": ("sol", ("X", "Y", "Z")), "dt": ("sol", ("dt",)), "dop": ("sol", ("DOP",)),
          "latlon": ("sol", ("lat", "lon")), "height": ("sol", ("height",)),
          "elaz": ("chan", ("el", "az")), "corrP": ("chan", ("corrP",))}

# the largest |float64 - longdouble| of the literal restatement over SCENES and many_rx_scene(), per group
# (metres, metres, -, degrees, metres, degrees, metres), from `python tests/navfix_scenarios.py`
SPREAD = {"xyz": 2.882e-07, "dt": 1.476e-07, "dop": 1.518e-13, "latlon": 1.843e-12,
          "height": 2.517e-07, "elaz": 5.777e-12, "corrP": 1.691e-07}
TOL = {k: 16 * v for k, v in SPREAD.items()}

# the same over WORLD_SCENES alone, from `python tests/navfix_scenarios.py world`
SPREAD_WORLD = {"xyz": 8.624e-08, "dt": 6.939e-08, "dop": 4.391e-14, "latlon": 1.467e-12,
                "height": 9.391e-08, "elaz": 2.247e-12, "corrP": 9.004e-08}
TOL_WORLD = {k: 16 * v for k, v in SPREAD_WORLD.items()}


def group_distance(a, b, group):
    """largest |a - b| over a group's fields, NaN and inf patterns required equal; a and b are
    (S, Cn) pairs of dicts or (sol, chan) pairs of records"""
    which, names = GROUPS[group]
    worst = 0.0
    for k in names:
        x = np.asarray(a[which == "chan"][k], np.longdouble)
        y = np.asarray(b[which == "chan"][k], np.longdouble)
        assert np.array_equal(np.isnan(x), np.isnan(y)), (group, k)
        assert np.array_equal(np.isinf(x), np.isinf(y)), (group, k)
        fin = np.isfinite(x)
        if fin.any():
            worst = max(worst, float(np.abs(x[fin] - y[fin]).max()))
    return worst


def measure_spread(names=tuple(SCENES) + ("many",)):
    out = {g: 0.0 for g in GROUPS}
    for name in names:
        _, S64, C64 = literal_result(name, np.float64)
        _, SL, CL = literal_result(name, np.longdouble)
        for g in GROUPS:
            out[g] = max(out[g], group_distance((S64, C64), (SL, CL), g))
    return out


def named_for_missed(name, s):
    """what the scene `name` of WORLD_SCENES is named for and s does not show, from the literal
    restatement in float64 (an empty list: it shows all of it).  Every receiver is solved at
    every measurement; world: site_classes_missed; week_end / week_start: check_t took every
    used channel's time - t_oe down / up by a week; eccentric: every Kepler loop ran 10 steps
    and left by the cap with |dE| > 4e-12; inclined: inclinations below 0.6 and above 1.2 rad"""
    diag = {"dE": []}
    n, Sx, Cx = fix_literal(s["eph"], s["first"], s["abs_sample"], s["rx_first"], s["cfg"],
                            diag=diag)
    missed = []
    if not (n == s["cfg"]["max_meas"]).all() or Sx["status"].any() or not Cx["used"].all():
        missed.append("solved")
    tk = np.array(diag["tk"], np.float64)
    wrap = {"week_end": -WEEK, "week_start": WEEK}.get(name, 0)
    if not (tk[:, 1] - tk[:, 0] == wrap).all():
        missed.append("check_t")
    kep = np.array(diag["kepler"], np.float64)
    if name == "eccentric" and not ((kep[:, 0] == 10) & (kep[:, 1] > 4e-12)).all():
        missed.append("kepler")
    if name == "inclined" and not (s["eph"]["i_0"].min() < 0.6 and s["eph"]["i_0"].max() > 1.2):
        missed.append("i_0")
    if name == "world":
        missed += site_classes_missed(Sx["lat"], Sx["lon"])
    return missed


def search_seed(S, name, start, tries=400, **kw):
    """S: a scenario module.  The first seed from `start` on at which the scene `name` of
    S.WORLD_SCENES, with kw in place of its arguments, passes S.conditions_hold and
    S.named_for_missed is empty"""
    for seed in range(start, start + tries):
        s = S.make_fix_scene(**dict(S.WORLD_SCENES[name][0], seed=seed, **kw))
        if S.conditions_hold(s, full_rank=True) and not S.named_for_missed(name, s):
            return seed
    return None


def receiver_scene(s, rx):
    """the scene s cut down to its receiver rx: receivers do not see each other"""
    a, b = s["rx_first"][rx], s["rx_first"][rx + 1]
    return dict(s, eph=s["eph"][a:b], first=s["first"][a:b], abs_sample=s["abs_sample"][a:b],
                rx_first=np.array([0, b - a], np.int32), sizes=(int(b - a),))


def search_rx_seeds(S, tries=200, **kw):
    """for the world scene of a module whose builder takes rx_seeds: per receiver rx the first
    seed 1000 rx + t, t = 0, 1, .., at which that receiver alone passes S.conditions_hold, is
    solved at every measurement with every channel used and shows its site's class.  A
    receiver's draw depends on the scene's seed and its own only, so the seeds found together
    give the receivers found one by one."""
    rules = [rule for _, rule in SITES.values()]
    found = [None] * len(rules)
    for t in range(tries):
        s = S.make_fix_scene(**dict(S.WORLD_SCENES["world"][0], **kw,
                                    rx_seeds=tuple(1000 * rx + t for rx in range(len(rules)))))
        for rx in (rx for rx in range(len(rules)) if found[rx] is None):
            sub = receiver_scene(s, rx)
            n, Sx, Cx = S.fix_literal(sub["eph"], sub["first"], sub["abs_sample"],
                                      sub["rx_first"], sub["cfg"])
            if (n == sub["cfg"]["max_meas"]).all() and not Sx["status"].any() and \
                    Cx["used"].all() and S.conditions_hold(sub, full_rank=True) and \
                    all(rules[rx](la, lo) for la, lo in zip(Sx["lat"][0], Sx["lon"][0])):
                found[rx] = 1000 * rx + t
        if None not in found:
            break
    return tuple(found)


if __name__ == "__main__":
    import sys
    world = sys.argv[1:] == ["world"]
    for g, v in (measure_spread(tuple(WORLD_SCENES)) if world else measure_spread()).items():
        print(f'"{g}": {v:.3e},')
