"""GLONASS L1OF after the data bits: a literal restatement of the Scilab receiver's field
decoding, satellite integration and position fix, and seeded scene generators
(tests/test_navglo_cpu.py holds the restatement to what the generators planted;
tests/test_navglo_gpu.py holds csrc/navglo.hip to the restatement).

    GLONASS/L1/include/ephemeris.sci:25-98                    eph_literal
    GLONASS/L1/geoFunctions/satposg.sci:38-132,299-310        satpos_literal, rk4_literal
    GLONASS/L1/postNavigation.sci:89-123,142-284              fix_literal
    calculatePseudoranges.sci:55-72, geoFunctions/deltasatposg.sci:66-137,
    leastSquarePos.sci:45-100, e_r_corr.sci, topocent.sci, togeod.sci, tropo.sci, cart2geo.sci

Comments carry the files' 1-based indices.  The restatement takes the scalar type T
(numpy.float64 or numpy.longdouble) as navfix_scenarios does: constants are the files'
float64 literals in both, only the operations change.  The frame time t, deltat and the three
loop counts are decisions: they are always computed in float64, and the longdouble run takes
them from there.  The Runge-Kutta step is written once (satposg.sci:67-132 and
deltasatposg.sci:67-126 are the same text) on arrays over satellites: every element sees the
file's operations in the file's order.  tropo, the LDL' solve with the library's rank rule and
the record types of the solution are navfix_scenarios'.  topocent, togeod and cart2geo of this
receiver call atan(y, x) directly.

columns="file" reproduces the file's bookkeeping of satellite states: columns ordered by
position in the active list, so that after an exclusion the remaining satellites take their
neighbours' states.  columns="channel" is the library's: every channel keeps its own.

Tolerances.  SPREAD is the largest |literal in float64 - literal in longdouble| per output
group over every scene and measurement of SCENES, of many_rx_scene() and, for the state
groups, of SAT_SCENES; TOL = 16 * SPREAD.  Produced by
    python tests/navglo_scenarios.py
and copied here; test_navglo_cpu.py asserts that a fresh measurement does not exceed them.
"""
import functools

import numpy as np

import navfix_scenarios as G

PI = G.PI
EPH_FIELDS = ("x", "y", "z", "xdot", "ydot", "zdot", "xdotdot", "ydotdot", "zdotdot", "gamman",
              "taun", "deltataun", "tauc", "tauGPS", "t")
EPH_INTS = ("P1", "tk_h", "tk_m", "tk_s", "Bn", "P2", "tb", "P3", "P", "In3", "En", "P4", "Ft",
            "Nt", "n", "M", "NA", "N4", "In5", "string_1_pos", "have", "skipped", "status",
            "reserved")
EPH = np.dtype([(f, "<f8") for f in EPH_FIELDS] + [(f, "<i4") for f in EPH_INTS])
SAT = np.dtype([("pos", "<f8", (3,)), ("vel", "<f8", (3,)), ("acc", "<f8", (3,)), ("clk", "<f8"),
                ("deltat", "<f8"), ("n10", "<i4"), ("n1", "<i4"), ("n001", "<i4"),
                ("ready", "<i4")])
SOL, CHAN = G.SOL, G.CHAN
EPH_OK, EPH_SHORT = 0, 1
FIX_OK, FIX_FEW, FIX_RANK = G.FIX_OK, G.FIX_FEW, G.FIX_RANK

# name: (string number, hi, lo (decoded_str(hi:-1:lo), 1-based), sign position or 0,
#        exponent of 2, integer factor)
FIELDS = {
    "P1": (1, 78, 77, 0, 0, 1), "tk_h": (1, 76, 72, 0, 0, 1), "tk_m": (1, 71, 66, 0, 0, 1),
    "tk_s": (1, 65, 65, 0, 0, 30), "xdot": (1, 63, 41, 64, -20, 0),
    "xdotdot": (1, 39, 36, 40, -30, 0), "x": (1, 34, 9, 35, -11, 0),
    "Bn": (2, 80, 80, 0, 0, 4), "P2": (2, 65, 65, 0, 0, 1), "tb": (2, 76, 70, 0, 0, 15),
    "ydot": (2, 63, 41, 64, -20, 0), "ydotdot": (2, 39, 36, 40, -30, 0),
    "y": (2, 34, 9, 35, -11, 0),
    "P3": (3, 80, 80, 0, 0, 1), "gamman": (3, 78, 69, 79, -40, 0), "P": (3, 67, 66, 0, 0, 1),
    "In3": (3, 65, 65, 0, 0, 1), "zdot": (3, 63, 41, 64, -20, 0),
    "zdotdot": (3, 39, 36, 40, -30, 0), "z": (3, 34, 9, 35, -11, 0),
    "taun": (4, 79, 59, 80, -30, 0), "deltataun": (4, 57, 54, 58, -30, 0),
    "En": (4, 53, 49, 0, 0, 1), "P4": (4, 34, 34, 0, 0, 1), "Ft": (4, 33, 30, 0, 0, 1),
    "Nt": (4, 26, 16, 0, 0, 1), "n": (4, 15, 11, 0, 0, 1), "M": (4, 10, 9, 0, 0, 1),
    "NA": (5, 80, 70, 0, 0, 1), "tauc": (5, 68, 38, 69, -31, 0), "N4": (5, 36, 32, 0, 0, 1),
    "tauGPS": (5, 30, 10, 31, -30, 0), "In5": (5, 9, 9, 0, 0, 1),
}
SIGNED = tuple(k for k, v in FIELDS.items() if v[3])


def field_len(name):
    return FIELDS[name][1] - FIELDS[name][2] + 1


# ------------------------------------------------------------------ ephemeris.sci, literal
def _bin2dec(v):
    n = 0
    for b in v:
        n = 2 * n + int(b)
    return n


def eph_literal_one(bits, n_strings, first):
    """one channel: bits [15, 85] -> a dict of the EPH record's values"""
    out = {k: 0 for k in EPH_INTS}
    out.update({k: 0.0 for k in EPH_FIELDS})
    bits = np.asarray(bits).reshape(15, 85)
    if n_strings < 15 or first < 0:                            # postNavigation.sci:89-93
        out["status"] = EPH_SHORT
        return out
    string_1_pos = 0                                           # :25
    for i in range(1, 16):                                     # :30
        decoded_str = bits[i - 1]                              # decoded_str(k) = decoded_str[k - 1]
        if (decoded_str > 1).any():                            # :38-41
            out["skipped"] |= 1 << (i - 1)
            continue
        rng = lambda hi, lo: decoded_str[lo - 1:hi][::-1]      # decoded_str(hi:-1:lo)
        val = lambda hi, lo: _bin2dec(rng(hi, lo))
        sgn = lambda k: (-1.0) ** int(decoded_str[k - 1])
        str_num = val(84, 81)                                  # :43
        if 1 <= str_num <= 5:
            out["have"] |= 1 << (str_num - 1)
        if str_num == 1:                                       # :49-56
            out["P1"] = val(78, 77)
            out["tk_h"] = val(76, 72)
            out["tk_m"] = val(71, 66)
            out["tk_s"] = val(65, 65) * 30
            out["xdot"] = val(63, 41) * sgn(64) * 2.0 ** -20
            out["xdotdot"] = val(39, 36) * sgn(40) * 2.0 ** -30
            out["x"] = val(34, 9) * sgn(35) * 2.0 ** -11
            string_1_pos = i
        elif str_num == 2:                                     # :60-65
            out["Bn"] = val(80, 80) * 4
            out["P2"] = val(65, 65)
            out["tb"] = val(76, 70) * 15
            out["ydot"] = val(63, 41) * sgn(64) * 2.0 ** -20
            out["ydotdot"] = val(39, 36) * sgn(40) * 2.0 ** -30
            out["y"] = val(34, 9) * sgn(35) * 2.0 ** -11
        elif str_num == 3:                                     # :68-74
            out["P3"] = val(80, 80)
            out["gamman"] = val(78, 69) * sgn(79) * 2.0 ** -40
            out["P"] = val(67, 66)
            out["In3"] = val(65, 65)
            out["zdot"] = val(63, 41) * sgn(64) * 2.0 ** -20
            out["zdotdot"] = val(39, 36) * sgn(40) * 2.0 ** -30
            out["z"] = val(34, 9) * sgn(35) * 2.0 ** -11
        elif str_num == 4:                                     # :77-84
            out["taun"] = val(79, 59) * sgn(80) * 2.0 ** -30
            out["deltataun"] = val(57, 54) * sgn(58) * 2.0 ** -30
            out["En"] = val(53, 49)
            out["P4"] = val(34, 34)
            out["Ft"] = val(33, 30)
            out["Nt"] = val(26, 16)
            out["n"] = val(15, 11)
            out["M"] = val(10, 9)
        elif str_num == 5:                                     # :86-90
            out["NA"] = val(80, 70)
            out["tauc"] = val(68, 38) * sgn(69) * 2.0 ** -31
            out["N4"] = val(36, 32)
            out["tauGPS"] = val(30, 10) * sgn(31) * 2.0 ** -30
            out["In5"] = val(9, 9)
    out["string_1_pos"] = string_1_pos
    t = float(out["tk_h"] * 60 * 60 + out["tk_m"] * 60 + out["tk_s"])          # :95
    out["t"] = t - float((string_1_pos - 1) * 2) - 0.3         # :98
    return out


def eph_literal(bits, n_strings, first):
    rec = np.zeros(len(bits), EPH)
    for ch in range(len(bits)):
        for k, v in eph_literal_one(bits[ch], n_strings[ch], first[ch]).items():
            rec[k][ch] = v
    return rec


# ------------------------------------------------------------------ satposg.sci, literal
DEFAULTS = dict(samplesPerCode=16000.0, dataTypeSizeInBytes=1.0, c=299792458.0,
                navSolPeriod=500, elevationMask=0.0, useTropCorr=1, max_meas=1)
MAX_DELTAT = 2.0 ** 27     # the library's widening: beyond it a record is not ready


def settings(**kw):
    s = dict(DEFAULTS)
    s.update(kw)
    return s


def rk4_literal(T, w, acc, h):
    """satposg.sci:67-132 (= deltasatposg.sci:67-126) on arrays over satellites.  w: six
    arrays (w10 .. w60), acc: three, h: an array or a scalar.  Returns the six new arrays."""
    mu, c20, ae, we = T(398600.44e9), T(-1082.63e-6), T(6378.136e3), T(0.7292115e-4)
    w10, w20, w30, w40, w50, w60 = w
    xdotdot, ydotdot, zdotdot = acc
    half = T(0.5)
    r = np.sqrt((w10 ** 2) + (w20 ** 2) + (w30 ** 2))

    def fx(x, z, vy):
        return -mu / (r ** 3) * x + T(3) / 2 * c20 * mu * (ae ** 2) / (r ** 5) * x * \
            (1 - 5 / (r ** 2) * (z ** 2)) + (we ** 2) * x + 2 * we * vy + xdotdot

    def fy(y, z, vx):
        return -mu / (r ** 3) * y + T(3) / 2 * c20 * mu * (ae ** 2) / (r ** 5) * y * \
            (1 - 5 / (r ** 2) * (z ** 2)) + (we ** 2) * y - 2 * we * vx + ydotdot

    def fz(z):
        return -mu / (r ** 3) * z + T(3) / 2 * c20 * mu * (ae ** 2) / (r ** 5) * z * \
            (3 - 5 / (r ** 2) * (z ** 2)) + zdotdot

    k11, k12, k13 = h * w40, h * w50, h * w60
    k14, k15, k16 = h * fx(w10, w30, w50), h * fy(w20, w30, w40), h * fz(w30)
    k21, k22, k23 = h * (w40 + half * k14), h * (w50 + half * k15), h * (w60 + half * k16)
    k24 = h * fx(w10 + half * k11, w30 + half * k13, w50 + half * k15)
    k25 = h * fy(w20 + half * k12, w30 + half * k13, w40 + half * k14)
    k26 = h * fz(w30 + half * k13)
    k31, k32, k33 = h * (w40 + half * k24), h * (w50 + half * k25), h * (w60 + half * k26)
    k34 = h * fx(w10 + half * k21, w30 + half * k23, w50 + half * k25)
    k35 = h * fy(w20 + half * k22, w30 + half * k23, w40 + half * k24)
    k36 = h * fz(w30 + half * k23)
    k41, k42, k43 = h * (w40 + k34), h * (w50 + k35), h * (w60 + k36)
    k44 = h * fx(w10 + k31, w30 + k33, w50 + k35)
    k45 = h * fy(w20 + k32, w30 + k33, w40 + k34)
    k46 = h * fz(w30 + k33)
    sixth = T(1) / 6
    return [w10 + sixth * (k11 + 2 * k21 + 2 * k31 + k41),
            w20 + sixth * (k12 + 2 * k22 + 2 * k32 + k42),
            w30 + sixth * (k13 + 2 * k23 + 2 * k33 + k43),
            w40 + sixth * (k14 + 2 * k24 + 2 * k34 + k44),
            w50 + sixth * (k15 + 2 * k25 + 2 * k35 + k45),
            w60 + sixth * (k16 + 2 * k26 + 2 * k36 + k46)]


def satpos_decisions(eph, period):
    """float64: ready, deltat [ms], n10, n1, n001 per channel (postNavigation.sci:107-123,160,
    satposg.sci:38-44; Scilab runs 1:abs(x) floor(abs(x)) times)"""
    step = np.float64(period) / 1000
    t = eph["t"].astype(np.float64)
    deltat = ((t - step) * 1000) - (eph["tb"].astype(np.float64) * 60 * 1000)
    ready = (eph["status"] == EPH_OK) & ((eph["have"] & 15) == 15) & (eph["Bn"] != 4) & \
        (eph["In3"] != 1) & (np.abs(deltat) < MAX_DELTAT)
    deltat10 = np.trunc(deltat / 10000)
    remdeltat10 = deltat - np.trunc(deltat / 10000) * 10000
    deltat1 = np.trunc(remdeltat10 / 1000)
    deltat001 = remdeltat10 - np.trunc(remdeltat10 / 1000) * 1000
    z = lambda v: np.where(ready, v, 0)
    return (ready, z(deltat), z(np.abs(deltat10)).astype(np.int32),
            z(np.abs(deltat1)).astype(np.int32),
            z(np.floor(np.abs(deltat001))).astype(np.int32))


def satpos_literal(eph, period, T=np.float64):
    """satposg.sci for every channel at once -> a dict: pos, vel, acc [n_ch, 3] and clk [n_ch]
    in T; deltat, n10, n1, n001, ready from satpos_decisions.  Channels that are not ready
    hold zeros."""
    n_ch = len(eph)
    ready, deltat, n10, n1, n001 = satpos_decisions(eph, period)
    out = dict(pos=np.zeros((n_ch, 3), T), vel=np.zeros((n_ch, 3), T), acc=np.zeros((n_ch, 3), T),
               clk=np.zeros(n_ch, T), deltat=deltat, n10=n10, n1=n1, n001=n001,
               ready=ready.astype(np.int32))
    idx = np.flatnonzero(ready)
    if len(idx) == 0:
        return out
    g = lambda k: eph[k][idx].astype(T)
    w = [g(k) * 1000 for k in ("x", "y", "z", "xdot", "ydot", "zdot")]        # :54-59
    acc = [g(k) * 1000 for k in ("xdotdot", "ydotdot", "zdotdot")]            # :60-62
    sign = np.sign(deltat[idx]).astype(T)
    a, b, c = n10[idx], n1[idx], n001[idx]
    total = a + b + c
    with np.errstate(all="ignore"):
        for i in range(int(total.max(initial=0))):             # :64, :142, :223
            h = np.where(i < a, T(10), np.where(i < a + b, T(1), T(0.001))) * sign
            new = rk4_literal(T, w, acc, h)
            run = i < total
            w = [np.where(run, n, o) for n, o in zip(new, w)]
    out["pos"][idx] = np.stack(w[:3], axis=1)
    out["vel"][idx] = np.stack(w[3:], axis=1)
    out["acc"][idx] = np.stack(acc, axis=1)
    out["clk"][idx] = g("taun") - g("gamman") * (deltat[idx].astype(T) / 1000)   # :310
    return out


def sat_records(lit):
    rec = np.zeros(len(lit["clk"]), SAT)
    for k in SAT.names:
        rec[k] = lit[k]
    return rec


# ------------------------------------------------------------------ the fix, literal
def togeod_literal(T, X, Y, Z, mutant=None):
    """togeod.sci:31-110 with a = 6378137, finv = 298.257223563 -> (dphi, dlambda) in degrees
    and the residual dP^2 + dZ^2 at the loop's exit"""
    a, finv, tolsq = T(6378137), T(298.257223563), T(1.e-10)
    if mutant == "togeod_abs_z":
        Z = abs(Z)
    rtd = T(180) / T(PI)
    esq = (2 - 1 / finv) / finv
    oneesq = 1 - esq
    P = np.sqrt(X * X + Y * Y)
    dlambda = np.arctan2(Y, X) * rtd if P > T(1.e-20) else T(0)               # :52-56
    if dlambda < 0:
        dlambda = dlambda + 360
    r = np.sqrt(P * P + Z * Z)
    sinphi = Z / r if r > T(1.e-20) else T(0)
    dphi = np.arcsin(sinphi)
    if r < T(1.e-20):
        return dphi, dlambda, T(0)
    h = r - a * (1 - sinphi * sinphi / finv)
    res = T(np.inf)
    for i in range(10):
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


def cart2geo_literal(T, X, Y, Z, mutant=None):
    """cart2geo.sci:20-45 with i = 5"""
    a, f = T(6378137), 1 / T(298.257223563)
    if mutant == "cart2geo_abs_z":
        Z = abs(Z)
    ly, lx = G.one_argument_atan(T, Y, X) if mutant == "cart2geo_atan_y_over_x" else (Y, X)
    lam = np.arctan2(ly, lx)                                   # :23
    ex2 = (2 - f) * f / ((1 - f) * (1 - f))
    c = a * np.sqrt(1 + ex2)
    p = np.sqrt(X * X + Y * Y)
    phi = np.arctan(Z / (p * (1 - (2 - f)) * f))
    h, oldh = T(0.1), T(0)
    iterations = 0
    while abs(h - oldh) > T(1.e-12):
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
    """leastSquarePos.sci:45-100.  Returns None for a rank-deficient A (the library's rule),
    else (pos, el, az, dop)."""
    dtr = T(PI) / 180
    pos = [T(0)] * 4
    n = len(obs)
    az, el = [T(0)] * n, [T(0)] * n
    f = None
    for it in range(1, n_iter + 1):                            # :45
        A = [None] * n
        F = [T(0)] * n
        if it > 1:
            phi, lam, res = togeod_literal(T, pos[0], pos[1], pos[2], mutant)   # topocent.sci:24
            if diag is not None:
                diag["togeod"].append(res)
        for i in range(n):                                     # :47
            X = satpos[i]
            if it == 1:                                        # :49-54
                Rot_X = [X[0], X[1], X[2]]
                dist = np.sqrt((X[0] - pos[0]) ** 2 + (X[1] - pos[1]) ** 2 + (X[2] - pos[2]) ** 2)
                trop = T(0)
            else:
                rho2 = (X[0] - pos[0]) ** 2 + (X[1] - pos[1]) ** 2 + (X[2] - pos[2]) ** 2
                traveltime = np.sqrt(rho2) / c
                if mutant == "no_erot":
                    Rot_X = [X[0], X[1], X[2]]
                else:                                          # e_r_corr.sci:20-31
                    omegatau = T(7.292115147e-5) * traveltime
                    co, so = np.cos(omegatau), np.sin(omegatau)
                    Rot_X = [co * X[0] + so * X[1], -so * X[0] + co * X[1], X[2]]
                dx = [Rot_X[0] - pos[0], Rot_X[1] - pos[1], Rot_X[2] - pos[2]]
                cl, sl = np.cos(lam * dtr), np.sin(lam * dtr)  # topocent.sci:26-29
                cb, sb = np.cos(phi * dtr), np.sin(phi * dtr)
                E = -sl * dx[0] + cl * dx[1] + 0 * dx[2]       # F' * dx, :31-38
                Nn = -sb * cl * dx[0] + -sb * sl * dx[1] + cb * dx[2]
                U = cb * cl * dx[0] + cb * sl * dx[1] + sb * dx[2]
                hor_dis = np.sqrt(E * E + Nn * Nn)
                if hor_dis < T(1.e-20):
                    az[i], el[i] = T(0), T(90)
                else:                                          # :46-47
                    az[i] = np.arctan2(E, Nn) / dtr
                    el[i] = np.arctan2(U, hor_dis) / dtr
                if az[i] < 0:
                    az[i] = az[i] + 360
                dist = np.sqrt(dx[0] ** 2 + dx[1] ** 2 + dx[2] ** 2)           # :54
                if useTropCorr == 1 and mutant != "no_trop":   # :63-69
                    trop = G.tropo_literal(T, np.sin(el[i] * dtr))
                else:
                    trop = T(0)
            F[i] = obs[i] - pos[3] - dist - trop               # :71
            A[i] = [(-(Rot_X[0] - pos[0])) / dist, (-(Rot_X[1] - pos[1])) / dist,
                    (-(Rot_X[2] - pos[2])) / dist, T(1)]       # :72-75
        N = [[T(0)] * 4 for _ in range(4)]
        g = [T(0)] * 4
        for i in range(n):                                     # A'A and A'F, row after row
            for r in range(4):
                for s in range(r + 1):
                    N[r][s] = N[r][s] + A[i][r] * A[i][s]
                g[r] = g[r] + A[i][r] * F[i]
        if diag is not None:
            diag["A"] = np.array(A, np.float64)
        f = G.ldl_factor(T, N)
        if f is None:
            return None
        x = G.ldl_solve(T, f, g)                               # :81
        pos = [pos[k] + x[k] for k in range(4)]
    Q = [G.ldl_solve(T, f, [T(k == j) for k in range(4)])[j] for j in range(4)]   # :92
    dop = [np.sqrt(Q[0] + Q[1] + Q[2] + Q[3]), np.sqrt(Q[0] + Q[1] + Q[2]), np.sqrt(Q[0] + Q[1]),
           np.sqrt(Q[2]), np.sqrt(Q[3])]
    return pos, el, az, dop


def pz90_to_wgs84(T, xyz):
    """postNavigation.sci:206-208"""
    x, y, z = xyz
    r = [1 * x + T(-0.82e-6) * y + 0 * z, T(0.82e-6) * x + 1 * y + 0 * z, 0 * x + 0 * y + 1 * z]
    k = 1 - T(0.12e-6)
    return [T(-1.1) + k * r[0], T(-0.3) + k * r[1], T(-0.9) + k * r[2]]


def fix_literal(eph, first, abs_sample, rx_first, cfg, T=np.float64, columns="channel",
                mutant=None, n_iter=7, diag=None, sat=None):
    """postNavigation.sci:142-284 per receiver.  abs_sample [n_ch, n_epochs].  Returns n_meas,
    sol [n_rx, max_meas], chan [n_ch, max_meas] as dicts of T arrays (navfix_scenarios.
    as_records).  sat: satpos_literal's result for (eph, navSolPeriod, T), computed when None."""
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
    step = T(np.float64(period) / 1000)                        # set_navSolPeriod/1000
    if sat is None:
        sat = satpos_literal(eph, period, T)
    with np.errstate(all="ignore"):
        for rx in range(n_rx):
            chs = list(range(rx_first[rx], rx_first[rx + 1]))
            ready = [ch for ch in chs if first[ch] >= 0 and sat["ready"][ch]]  # :107-123
            if len(ready) < 4:                                 # :128
                continue
            pmax = max(first[ch] for ch in chs if first[ch] >= 0)
            n_meas[rx] = max(0, min(mm, int((n_epochs - (pmax + 1)) / period)))   # :167
            # satposg's outputs: one column per ready channel (:159-160)
            colP = [[sat["pos"][ch][k] for k in range(3)] for ch in ready]
            colV = [[sat["vel"][ch][k] for k in range(3)] for ch in ready]
            colA = [[sat["acc"][ch][k] for k in range(3)] for ch in ready]
            colC = [sat["clk"][ch] for ch in ready]
            col_of = {ch: j for j, ch in enumerate(ready)}     # columns="channel"
            satElev = {ch: inf for ch in chs}                  # :142
            for m in range(n_meas[rx]):
                active = [ch for ch in ready if satElev[ch] >= T(cfg["elevationMask"])]   # :170
                for ch in chs:                                 # :179-180
                    Cn["el"][ch, m] = nan
                    Cn["az"][ch, m] = nan
                    Cn["used"][ch, m] = ch in active
                    Cn["corrP"][ch, m] = 0
                # calculatePseudoranges.sci:55-72
                travelTime = {ch: inf for ch in chs}
                for ch in active:
                    travelTime[ch] = T(abs_sample[ch, first[ch] + period * m]) / \
                        T(cfg["samplesPerCode"]) / T(cfg["dataTypeSizeInBytes"])
                minimum = np.floor(min(travelTime.values()))
                for ch in chs:
                    Cn["rawP"][ch, m] = (travelTime[ch] - minimum) * (c / 1000)
                # deltasatposg.sci:40-137: column satNr of the old arrays, gamman of the prn
                cols = list(range(len(active))) if columns == "file" else \
                    [col_of[ch] for ch in active]
                if active:
                    w = [np.array([colP[j][k] for j in cols], T) for k in range(3)] + \
                        [np.array([colV[j][k] for j in cols], T) for k in range(3)]
                    a = [np.array([colA[j][k] for j in cols], T) for k in range(3)]
                    new = rk4_literal(T, w, a, step)
                    clk = [colC[j] - T(eph["gamman"][ch]) * step for j, ch in zip(cols, active)]
                    if columns == "file":                      # the outputs replace the arrays
                        colP = [[new[k][i] for k in range(3)] for i in range(len(active))]
                        colV = [[new[3 + k][i] for k in range(3)] for i in range(len(active))]
                        colC = clk
                    else:
                        for i, j in enumerate(cols):
                            colP[j] = [new[k][i] for k in range(3)]
                            colV[j] = [new[3 + k][i] for k in range(3)]
                            colC[j] = clk[i]
                    sp = [[new[k][i] for k in range(3)] for i in range(len(active))]
                else:
                    sp, clk = [], []
                    if columns == "file":
                        colP, colV, colC = [], [], []
                if diag is not None:
                    diag.setdefault("states", []).append((rx, m, list(active), sp))
                S["written"][rx, m] = True
                S["n_used"][rx, m] = len(active)
                if len(active) > 3:                            # :198
                    obs = [Cn["rawP"][ch, m] - k * c for ch, k in zip(active, clk)]   # :202-203
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
                        xyz = pz90_to_wgs84(T, pos[:3])        # :206-208
                        S["X"][rx, m], S["Y"][rx, m], S["Z"][rx, m] = xyz
                        S["dt"][rx, m] = pos[3]
                        S["DOP"][rx, m] = dop
                        for i, ch in enumerate(active):        # :210-211
                            Cn["el"][ch, m] = el[i]
                            Cn["az"][ch, m] = az[i]
                        satElev = {ch: Cn["el"][ch, m] for ch in chs}          # :221
                        for ch, k in zip(active, clk):         # :224-226
                            Cn["corrP"][ch, m] = Cn["rawP"][ch, m] - k * c + pos[3]
                        S["lat"][rx, m], S["lon"][rx, m], S["height"][rx, m] = \
                            cart2geo_literal(T, xyz[0], xyz[1], xyz[2], mutant)   # :231-237
                        if diag is not None:
                            diag.setdefault("elev", []).extend(el)
                            diag.setdefault("togeod_all", []).extend(diag["togeod"])
                            diag.setdefault("cond", []).append(np.linalg.cond(diag["A"]))
                            diag.setdefault("gdop", []).append(float(dop[0]))
                else:                                          # :249-271
                    S["status"][rx, m] = FIX_FEW
                    for k in ("X", "Y", "Z", "dt", "lat", "lon", "height"):
                        S[k][rx, m] = nan
                    S["DOP"][rx, m] = 0
    S["rx_first"] = np.asarray(rx_first)
    return n_meas, S, Cn


def fix_literal_records(eph, first, abs_sample, rx_first, cfg, sol=None, chan=None, **kw):
    n_meas, S, Cn = fix_literal(eph, first, abs_sample, rx_first, cfg, **kw)
    return (n_meas,) + G.as_records(n_meas, S, Cn, sol, chan)


# ------------------------------------------------------------------ scene generators
def eph_ints(rng, kind="random"):
    """the raw field integers of one ephemeris: name -> (magnitude, sign bit)"""
    raw = {k: (int(rng.integers(0, 1 << field_len(k))), int(rng.integers(0, 2)) if v[3] else 0)
           for k, v in FIELDS.items()}
    if kind == "ones":
        raw.update({k: ((1 << field_len(k)) - 1, 1 if FIELDS[k][3] else 0) for k in FIELDS})
    elif kind == "signbit":
        raw.update({k: (0, 1) for k in SIGNED})
    elif kind == "negative":
        raw.update({k: (raw[k][0] | 1, 1) for k in SIGNED})
    return raw


def raw_to_values(raw):
    out = {}
    for k, (num, hi, lo, sg, ex, mul) in FIELDS.items():
        mag, s = raw[k]
        out[k] = mag * mul if mul else float(mag) * (-1.0 if s else 1.0) * 2.0 ** ex
    return out


def values_to_raw(vals, rng):
    """the nearest grid integers of physical values; fields not in vals are random"""
    raw = eph_ints(rng)
    for k, v in vals.items():
        num, hi, lo, sg, ex, mul = FIELDS[k]
        top = (1 << field_len(k)) - 1
        if mul:
            assert v % mul == 0 and 0 <= v // mul <= top, (k, v)
            raw[k] = (int(v) // mul, 0)
        else:
            mag = int(round(abs(v) / 2.0 ** ex))
            assert mag <= top, (k, v)
            raw[k] = (mag, 1 if v < 0 else 0)
    return raw


def string_bits(rng, num, raw):
    """85 bits of a string with number num (decoded_str(k) = bits[k - 1]): the fields of `raw`
    that belong to it, everything else random, decoded_str(85) = 0 as decode_gl_data leaves it"""
    b = rng.integers(0, 2, 85).astype(np.uint8)
    b[84] = 0
    put = lambda hi, lo, v: b.__setitem__(slice(lo - 1, hi), [(v >> i) & 1 for i in range(hi - lo + 1)])
    put(84, 81, num)
    for k, (sn, hi, lo, sg, ex, mul) in FIELDS.items():
        if sn == num:
            put(hi, lo, raw[k][0])
            if sg:
                b[sg - 1] = raw[k][1]
    return b


def wrap_order(start):
    """the 15 string numbers of a frame read from string `start` on"""
    return tuple((start - 1 + i) % 15 + 1 for i in range(15))


def frame_bits(rng, nums, raw):
    """[15, 85] bits: strings with the numbers `nums`; a repeated number carries other field
    values the first time, so the later one must win"""
    out = []
    for j, num in enumerate(nums):
        r = eph_ints(rng) if num in nums[j + 1:] else raw
        out.append(string_bits(rng, num, r))
    return np.array(out, np.uint8)


REPEATED = (1, 2, 3, 4, 5, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10)
NO_STRING_4 = (1, 2, 3, 0, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
NO_STRING_1 = (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 0)


@functools.lru_cache(None)
def eph_scene(n_ch, seed=11):
    """bits [n_ch, 15, 85], n_strings, first, the string numbers and planted raw integers per
    channel: every starting string in turn, the four kinds of field patterns in turn; the
    special frames and refusals spread over the channels when there are enough of them"""
    rng = np.random.default_rng(seed)
    kinds = ("random", "negative", "ones", "signbit")
    bits = np.zeros((n_ch, 15, 85), np.uint8)
    raws, orders = [], []
    n_strings = np.full(n_ch, 15, np.int32)
    first = rng.integers(0, 900, n_ch).astype(np.int32)
    for ch in range(n_ch):
        raw = eph_ints(rng, kinds[ch % 4])
        nums = wrap_order(ch % 15 + 1)
        if n_ch >= 32:
            nums = {20: REPEATED, 21: NO_STRING_4, 22: NO_STRING_1, 23: REPEATED}.get(ch, nums)
        raws.append(raw)
        orders.append(nums)
        bits[ch] = frame_bits(rng, nums, raw)
    if n_ch >= 3:
        n_strings[1] = 14
        bits[1, 14] = 0
    if n_ch >= 32:
        n_strings[8] = 0
        bits[8] = 0
        first[9] = -1
        bits[10, orders[10].index(2), 40] = 2                  # inside string 2
        bits[11, orders[11].index(9), 3] = 2                   # inside an almanac string
        bits[12, orders[12].index(1), 84] = 2                  # string 1, outside every field
        bits[13, orders[13].index(3), 82] = 2                  # inside string 3's number
    return bits, n_strings, first, tuple(orders), tuple(raws)


# orbits and geometry --------------------------------------------------------
MU, WE = 398600.44e9, 0.7292115e-4
ORBIT_R, ORBIT_INC = 25510.0e3, np.radians(64.8)
RX_ECEF = G.RX_ECEF


def _enu(pos):
    phi, lam, _ = togeod_literal(np.float64, *map(np.float64, pos))
    d2r = PI / 180
    cl, sl, cb, sb = np.cos(lam * d2r), np.sin(lam * d2r), np.cos(phi * d2r), np.sin(phi * d2r)
    return np.array([[-sl, cl, 0.0], [-sb * cl, -sb * sl, cb], [cb * cl, cb * sl, sb]])


def _elevation(pos, sat):
    e, n, u = _enu(pos) @ (np.asarray(sat[:3], np.float64) - np.asarray(pos, np.float64))
    return np.degrees(np.arctan2(u, np.hypot(e, n)))


def _orbit_velocity(rng, P):
    """ECEF velocity at P of a circular orbit of inclination 64.8 degrees: the inertial
    velocity minus the Earth's rotation"""
    r = P / np.linalg.norm(P)
    hz = np.cos(ORBIT_INC)
    # h . r = 0, h_z = hz, |h| = 1: h_xy = a r_xy + b perp(r_xy)
    rxy = np.array([r[0], r[1]])
    n2 = rxy @ rxy
    a = -hz * r[2] / n2
    b2 = (1 - hz * hz) / n2 - a * a
    if b2 <= 0:
        return None                                            # latitude above the inclination
    b = np.sqrt(b2) * (1 if rng.integers(0, 2) else -1)
    h = np.array([a * rxy[0] - b * rxy[1], a * rxy[1] + b * rxy[0], hz])
    v = np.sqrt(MU / np.linalg.norm(P)) * np.cross(h, r)
    return v - np.cross([0.0, 0.0, WE], P)


def _propagate(P, V, dt, n=12):
    w = [np.array([v]) for v in (*P, *V)]
    z = [np.zeros(1)] * 3
    for _ in range(n):
        w = rk4_literal(np.float64, w, z, np.float64(dt / n))
    return np.array([v[0] for v in w[:3]]), np.array([v[0] for v in w[3:]])


def draw_satellite(rng, pos, el_lo, el_hi, dt):
    """a GLONASS-like state at t_b, on the ICD grid, of a satellite that `dt` seconds later
    stands at an elevation in [el_lo, el_hi] from pos.  Returns the field values (km, km/s,
    km/s^2) and the position at t_b + dt."""
    while True:
        az, el = rng.uniform(0, 2 * PI), np.radians(rng.uniform(el_lo, el_hi))
        d = _enu(pos).T @ np.array([np.sin(az) * np.cos(el), np.cos(az) * np.cos(el), np.sin(el)])
        pb = pos @ d
        P = pos + d * (-pb + np.sqrt(pb * pb - pos @ pos + ORBIT_R ** 2))
        V = _orbit_velocity(rng, P)
        if V is None:
            continue
        P0, V0 = _propagate(P, V, -dt)
        vals = dict(zip(("x", "y", "z"), P0 / 1000))
        vals.update(zip(("xdot", "ydot", "zdot"), V0 / 1000))
        return vals, P


def _gdop(pos, sats):
    A = np.array([np.r_[-(np.asarray(s, float) - pos) / np.linalg.norm(np.asarray(s, float) - pos),
                        1.0] for s in sats])
    return float(np.sqrt(np.trace(np.linalg.inv(A.T @ A))))


def frame_time(tb, offset_s, pos1):
    """(tk_h, tk_m, tk_s) for which t = tb*60 + offset_s - 0.3 with string 1 at position pos1;
    offset_s + 2 (pos1 - 1) must be a multiple of 30"""
    tk = tb * 60 + offset_s + 2 * (pos1 - 1)
    assert tk % 30 == 0 and 0 <= tk < 32 * 3600, (tb, offset_s, pos1)
    return tk // 3600, tk % 3600 // 60, tk % 60


def plant_abs_samples(eph, first, chans, pos, cfg, n_epochs, n_meas, trop, offset_ms=0.3):
    """absoluteSample rows [len(chans), n_epochs] for one receiver at `pos` (PZ-90.02), from the
    restatement itself: at measurement m every channel's pseudorange is range + troposphere +
    clk c + a common clock term chosen so that the smallest travel time sits offset_ms above a
    whole millisecond.  Other epochs hold NaN."""
    T = np.float64
    c, spc, period = T(cfg["c"]), cfg["samplesPerCode"] * cfg["dataTypeSizeInBytes"], \
        cfg["navSolPeriod"]
    step = T(period) / 1000
    out = np.full((len(chans), n_epochs), np.nan)
    sat = satpos_literal(eph[chans], period)
    w = [sat["pos"][:, k].copy() for k in range(3)] + [sat["vel"][:, k].copy() for k in range(3)]
    a = [sat["acc"][:, k] for k in range(3)]
    clk = sat["clk"].copy()
    for m in range(n_meas):
        w = rk4_literal(T, w, a, step)
        clk = clk - eph["gamman"][chans] * step
        rawp = []
        for i, ch in enumerate(chans):
            x, y, z = w[0][i], w[1][i], w[2][i]
            rho = T(2.2e7)
            for _ in range(8):                                 # fixed point of the rotation
                om = T(7.292115147e-5) * (rho / c)
                rx = [np.cos(om) * x + np.sin(om) * y, -np.sin(om) * x + np.cos(om) * y, z]
                rho = np.sqrt(sum((rx[k] - pos[k]) ** 2 for k in range(3)))
            tr = G.tropo_literal(T, np.sin(np.radians(_elevation(pos, rx)))) if trop else T(0)
            rawp.append(rho + tr + clk[i] * c)
        rawp = np.array(rawp) / (c / 1000)                     # ms, up to the clock term
        ms = rawp - rawp.min() + offset_ms
        for i, ch in enumerate(chans):
            out[i, first[ch] + period * m] = (ms[i] + (1000 + period * m)) * spc
    return out


def make_fix_scene(seed, sizes, n_epochs=200, period=20, max_meas=7, trop=1, mask=10.0, low=(),
                   no_str4=(), not_ready=(), bn4=(), in3=(), clone=(), first_lo=0, first_hi=15,
                   low_first=False, sites=None, rx_seeds=None):
    """sizes: channels per receiver.  low: {receiver: number of satellites between 3 and 7
    degrees}: in the first fix, then out (mask 10); they are the receiver's last lanes, its first
    with low_first.  no_str4 / not_ready / bn4 / in3: (receiver,
    lane) pairs whose frame has no string 4 / whose first_mark is -1 / whose Bn is 4 / whose ln
    flag of string 3 is 1.  clone: receivers in which every channel carries channel 0's frame
    and absoluteSample (rank 1).  t_b is a multiple of 15 minutes, every channel's frame time
    lies within 15 minutes of it on either side, and the frames start at every string number in
    turn.  sites: (latitude, longitude) in degrees per receiver, in place of RX_ECEF; the 200 km of
    jitter and the rescaling to 6371 km stay.  rx_seeds: a seed per receiver for its own
    generator (jitter, satellites, frame filler) in place of the scene's, so that one
    receiver's draw can be searched with the others kept."""
    rng = np.random.default_rng(seed)
    cfg = settings(navSolPeriod=period, max_meas=max_meas, useTropCorr=trop, elevationMask=mask)
    rx_first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n_ch = int(rx_first[-1])
    bits = np.zeros((n_ch, 15, 85), np.uint8)
    first = rng.integers(first_lo, first_hi, n_ch).astype(np.int32)
    planted = []
    scene_rng = rng
    for rx, size in enumerate(sizes):
        rng = scene_rng if rx_seeds is None else np.random.default_rng(rx_seeds[rx])
        pos = (np.array(RX_ECEF) if sites is None else G.site_ecef(sites[rx])) + \
            rng.uniform(-2e5, 2e5, 3)
        pos *= 6371000.0 / np.linalg.norm(pos)
        planted.append(pos)
        n_low = dict(low).get(rx, 0)
        is_low = lambda lane: lane < n_low if low_first else lane >= size - n_low
        tb = 15 * int(rng.integers(4, 90))
        base = 30 * int(rng.integers(-28, 29))                 # the frame's t_k - t_b [s]
        bad = [p for p in (*no_str4, *not_ready, *bn4, *in3) if p[0] == rx]
        while True:                                            # a geometry with GDOP < 5
            drawn = []
            for lane in range(size):
                start = (rx_first[rx] + lane) % 15 + 1
                pos1 = (16 - start) % 15 + 1                   # where string 1 stands
                dt = base - 2 * (pos1 - 1) - 0.3               # t - t_b [s]
                drawn.append(draw_satellite(rng, pos, *((3.0, 7.0) if is_low(lane)
                                                        else (18.0, 85.0)), dt) + (start, pos1))
            use = [lane for lane in range(size) if (rx, lane) not in bad]
            high = [lane for lane in use if not is_low(lane)]
            if len(use) < 4 or rx in clone:
                break
            if _gdop(pos, [drawn[l][1] for l in use]) < 5 and \
                    (len(high) < 4 or _gdop(pos, [drawn[l][1] for l in high]) < 5):
                break
        for lane in range(size):
            ch = rx_first[rx] + lane
            vals, _, start, pos1 = drawn[lane]
            h, mi, s = frame_time(tb, base - 2 * (pos1 - 1), pos1)
            vals.update(tk_h=h, tk_m=mi, tk_s=s, tb=tb, Bn=4 if (rx, lane) in bn4 else 0,
                        In3=1 if (rx, lane) in in3 else 0,
                        gamman=rng.uniform(-1e-11, 1e-11), taun=rng.uniform(-2e-4, 2e-4),
                        **{k: rng.uniform(-1e-8, 1e-8) for k in ("xdotdot", "ydotdot", "zdotdot")})
            nums = wrap_order(start)
            if (rx, lane) in no_str4:
                nums = tuple(0 if n == 4 else n for n in nums)
            bits[ch] = frame_bits(rng, nums, values_to_raw(vals, rng))
            if (rx, lane) in not_ready:
                first[ch] = -1
        if rx in clone:
            for lane in range(1, size):
                bits[rx_first[rx] + lane] = bits[rx_first[rx]]
                first[rx_first[rx] + lane] = first[rx_first[rx]]
    n_strings = np.full(n_ch, 15, np.int32)
    eph = eph_literal(bits, n_strings, first)
    ready = satpos_decisions(eph, period)[0]
    abs_sample = np.full((n_ch, n_epochs), np.nan)
    for rx, size in enumerate(sizes):
        chans = [ch for ch in range(rx_first[rx], rx_first[rx + 1]) if first[ch] >= 0 and ready[ch]]
        pm = max([first[ch] for ch in range(rx_first[rx], rx_first[rx + 1]) if first[ch] >= 0],
                 default=0)
        nm = max(0, min(max_meas, (n_epochs - (pm + 1)) // period))
        if chans:
            abs_sample[chans] = plant_abs_samples(eph, first, chans, planted[rx], cfg, n_epochs,
                                                  nm, trop)
        if rx in clone:
            for ch in range(rx_first[rx] + 1, rx_first[rx + 1]):
                abs_sample[ch] = abs_sample[rx_first[rx]]
    return dict(bits=bits, n_strings=n_strings, first=first, eph=eph, abs_sample=abs_sample,
                rx_first=rx_first, cfg=cfg, planted=np.array(planted), sizes=tuple(sizes))


SCENES = {
    # name: (arguments of make_fix_scene, multi-measurement full-rank scene with no exclusion)
    "one_rx_4": (dict(seed=1, sizes=(4,), max_meas=2), True),
    "one_rx_5": (dict(seed=2, sizes=(5,), max_meas=7), True),
    "three_rx": (dict(seed=3, sizes=(12, 4, 7), max_meas=2), True),
    "wave64": (dict(seed=4, sizes=(64,), max_meas=1, n_epochs=120), False),
    "notrop": (dict(seed=5, sizes=(6, 9), max_meas=2, trop=0, mask=0.0), True),
    "drop_one": (dict(seed=6, sizes=(7,), max_meas=3, low={0: 1}, low_first=True), False),
    "five_to_three": (dict(seed=7, sizes=(5, 5), max_meas=3, low={0: 2}), False),
    "few_ready": (dict(seed=8, sizes=(5, 6), max_meas=2, not_ready=((0, 1),), no_str4=((0, 3),)),
                  False),
    "health": (dict(seed=9, sizes=(6, 6), max_meas=2, bn4=((0, 2),), in3=((1, 5),)), True),
    "rank": (dict(seed=10, sizes=(5, 6), max_meas=2, clone=(0,)), False),
    "max_meas_below": (dict(seed=12, sizes=(5,), max_meas=2, n_epochs=300), True),
    "one_meas": (dict(seed=13, sizes=(8,), max_meas=1, n_epochs=80), False),
}


# one receiver at every site of navfix_scenarios.SITES in one launch, troposphere on for all
# (useTropCorr is one setting per launch).  Every receiver has a seed of its own, the first of
# 1000 rx + 0, 1, .. at which it passes conditions_hold alone and shows its site's class
# (navfix_scenarios.search_rx_seeds).
# MOVED, and further than the 5 degrees a site was meant to move: the four sites at 17 S stand
# at 8 S.  In this least-squares text the first togeod call of a fix, on the position after one
# step from the origin (hundreds of kilometres off, and much the same for every geometry of
# satellites on one orbit radius), leaves its loop with a residual of 3e-11 to 6e-11 at every
# latitude from 12 to 22 degrees, north or south: within conditions_hold's factor 4 of the
# 1e-10 exit.  None of 384 draws at 17 S passed (96 seeds, four receivers), none of 160 at
# 12 S, nor with one to four satellites low in the sky (7e-11 to 1e-10).  At 8 S each of the
# four passes within 14 seeds.  Hemisphere, quadrant and class are the sites' own.
WORLD_MOVED = {k: (-8.0, G.SITES[k][0][1])
               for k in ("south_east", "south_west", "meridian_180_east", "meridian_180_west")}
WORLD_SCENES = {
    "world": (dict(seed=100, sizes=G.WORLD_SIZES, max_meas=2, sites=G.world_sites(WORLD_MOVED),
                   rx_seeds=(0, 1000, 2001, 3013, 4003, 5000, 6000, 7000, 8001, 9000, 10000)),
              True),
}


@functools.lru_cache(None)
def fix_scene(name):
    return make_fix_scene(**(SCENES.get(name) or WORLD_SCENES[name])[0])


@functools.lru_cache(None)
def many_rx_scene(n_rx=65, seed=21):
    """n_rx receivers of unequal size (4 .. 9 channels) in one launch"""
    sizes = tuple(4 + (i * 5) % 6 for i in range(n_rx))
    return make_fix_scene(seed, sizes, max_meas=2)


def _scene(name):
    return many_rx_scene() if name == "many" else fix_scene(name)


@functools.lru_cache(None)
def scene_sat(name, T=np.float64):
    s = _scene(name)
    return satpos_literal(s["eph"], s["cfg"]["navSolPeriod"], T)


@functools.lru_cache(None)
def literal_result(name, T=np.float64, columns="channel", mutant=None):
    s = _scene(name)
    return fix_literal(s["eph"], s["first"], s["abs_sample"], s["rx_first"], s["cfg"], T,
                       columns=columns, mutant=mutant, sat=scene_sat(name, T))


def scene_diagnostics(s):
    """what the scene conditions are asserted on, from the restatement in float64: cond(A) and
    GDOP of every solved measurement, every elevation, the residual at every exit of togeod"""
    diag = {}
    fix_literal(s["eph"], s["first"], s["abs_sample"], s["rx_first"], s["cfg"], diag=diag)
    return {k: np.array(diag.get(k, []), np.float64) for k in ("cond", "gdop", "elev", "togeod_all")}


def conditions_hold(s, full_rank=True):
    d = scene_diagnostics(s)
    ok = not G._near(d["togeod_all"], 1e-10)
    ok = ok and not (np.abs(d["elev"] - s["cfg"]["elevationMask"]) < 1e-6).any()
    if full_rank:
        ok = ok and (d["cond"] < 1e6).all() and (d["gdop"] < 6).all()
    return bool(ok)


# satpos scenes ----------------------------------------------------------------
# (offset of t + 0.3 from t_b in seconds, position of string 1) per channel, in turn; with
# navSolPeriod 500 deltat sits 200 ms above a whole second (n001 199 or 200 by the last bit,
# 799 or 800 for a negative deltat), with 700 it sits at a whole second (n001 0 or 999, and
# deltat exactly 0 for the offset 1)
SAT_OFFSETS = (900, -898, 902, 10, -8, 2, 0, 12, -10, 92, -88, 480, -478, 30, -30, 1, 9, 11,
               -9, 20, 100, -100, 450, -450, 898, -900, 901, -899, 31, -29)


def _offset_frame(tb, off):
    """string 1's position and t_k for which t + 0.3 = tb*60 + off"""
    for pos1 in range(1, 16):
        if (off + 2 * (pos1 - 1)) % 30 == 0:
            return (pos1,) + frame_time(tb, off, pos1)
    raise AssertionError(off)


# channel: (t_b [min], offset): t = 32768.7 sits just above 2^15, where t - step rounds the
# other way: n001 199 instead of 200 with navSolPeriod 500, 999 instead of 0 with 700; and a
# negative deltat whose remainder is 799 instead of 800
SAT_SPECIAL = {50: (540, 370), 51: (540, 369), 52: (150, -806)}


@functools.lru_cache(None)
def sat_scene(period, n_ch=65, seed=31):
    """GLO_EPH records [n_ch] made directly (no bits): orbit states on the ICD grid, frame
    times from SAT_OFFSETS; odd offsets are not reachable from tk and string_1_pos, so t is
    written as stage 1 would for the even part and 1 s is added through tk_s (a record the
    caller made).  Channels 5, 17, 29, 41 are not ready: status SHORT, string 4 missing, Bn 4,
    ln 1."""
    rng = np.random.default_rng(seed)
    eph = np.zeros(n_ch, EPH)
    pos = np.array(RX_ECEF)
    for ch in range(n_ch):
        off = SAT_OFFSETS[ch % len(SAT_OFFSETS)]
        tb = 15 * int(rng.integers(4, 90))
        tb, off = SAT_SPECIAL.get(ch, (tb, off))
        vals, _ = draw_satellite(rng, pos, -90.0, 90.0, float(off))
        odd = off % 2
        pos1, h, mi, s = _offset_frame(tb, off - odd)
        vals.update(tk_h=h, tk_m=mi, tk_s=s, tb=tb, Bn=0, In3=0,
                    gamman=rng.uniform(-1e-11, 1e-11), taun=rng.uniform(-2e-4, 2e-4),
                    **{k: rng.uniform(-1e-8, 1e-8) for k in ("xdotdot", "ydotdot", "zdotdot")})
        for k, v in raw_to_values(values_to_raw(vals, rng)).items():
            eph[k][ch] = v
        eph["tk_s"][ch] += odd
        eph["string_1_pos"][ch] = pos1
        eph["have"][ch] = 31
        eph["t"][ch] = float(h * 3600 + mi * 60 + s + odd) - float((pos1 - 1) * 2) - 0.3
    for ch, (k, v) in zip((5, 17, 29, 41), (("status", EPH_SHORT), ("have", 23), ("Bn", 4),
                                            ("In3", 1))):
        if ch < n_ch:
            eph[k][ch] = v
    return eph


SAT_SCENES = (500, 700)


@functools.lru_cache(None)
def sat_literal(period, T=np.float64):
    return satpos_literal(sat_scene(period), period, T)


# the chain ---------------------------------------------------------------------
def strings_to_series(rng, bits, first, n_epochs, amp=800.0):
    """the prompt sums of one channel whose 15 strings decode to bits [15, 85]: random 10-ms
    chips up to `first`, then [time mark 300][85 relative-coded meander symbols 1700] per string
    (decode_gl_data.sci:19-34 inverted: dec[83 - i] = -y[i] y[i + 1])"""
    import navbits_scenarios as NB
    x = 2.0 * np.repeat(rng.integers(0, 2, first // 10 + 1), 10)[:first] - 1
    m = np.concatenate([-np.ones(10), np.ones(10)])
    for i in range(15):
        dec = 2 * bits[i].astype(int) - 1
        y = np.ones(85, int)
        for j in range(84):
            y[j + 1] = -dec[83 - j] * y[j]
        x = np.concatenate([x, NB.GLO_PATTERN.astype(float), np.kron(y, m)])
    tail = 2.0 * rng.integers(0, 2, max(n_epochs - len(x), 0)) - 1
    x = np.concatenate([x, tail])[:n_epochs]
    return amp * x * (1.0 + 0.2 * rng.random(n_epochs))


@functools.lru_cache(None)
def chain_scene(seed=41, n_ch=5, n_epochs=31000, max_meas=3):
    """One receiver for the device chain: a fix scene whose first marks leave room for 15
    strings, and the I_P series [n_ch, n_epochs] that carry its frames"""
    s = make_fix_scene(seed, (n_ch,), n_epochs=n_epochs, period=20, max_meas=max_meas,
                       first_lo=100, first_hi=900)
    rng = np.random.default_rng(seed + 1)
    series = np.stack([strings_to_series(rng, s["bits"][ch], int(s["first"][ch]), n_epochs)
                       for ch in range(n_ch)])
    return s, series


# tolerances ----------------------------------------------------------------------
GROUPS = dict(G.GROUPS)
STATE_GROUPS = {"state_pos": "pos", "state_vel": "vel"}

# the largest |float64 - longdouble| of the restatement per group (metres, metres, -, degrees,
# metres, degrees, metres; metres, metres per second), from `python tests/navglo_scenarios.py`
SPREAD = {"xyz": 2.660e-07, "dt": 2.955e-07, "dop": 8.634e-14, "latlon": 3.294e-12,
          "height": 3.024e-07, "elaz": 7.712e-12, "corrP": 3.108e-07, "state_pos": 3.279e-07,
          "state_vel": 4.208e-11}
TOL = {k: 16 * v for k, v in SPREAD.items()}

# the same over WORLD_SCENES alone (the states: their ephemerides'), from
# `python tests/navglo_scenarios.py world`
SPREAD_WORLD = {"xyz": 3.130e-07, "dt": 1.980e-07, "dop": 6.543e-14, "latlon": 1.466e-12,
                "height": 3.151e-07, "elaz": 7.168e-12, "corrP": 2.100e-07,
                "state_pos": 2.761e-07, "state_vel": 7.082e-12}
TOL_WORLD = {k: 16 * v for k, v in SPREAD_WORLD.items()}

group_distance = G.group_distance


def state_distance(a, b, group):
    """largest |a - b| over pos or vel; a and b are satpos_literal results or SAT records"""
    k = STATE_GROUPS[group]
    x, y = np.asarray(a[k], np.longdouble), np.asarray(b[k], np.longdouble)
    assert np.isfinite(x).all() and np.isfinite(y).all()
    return float(np.abs(x - y).max(initial=0.0))


def measure_spread(names=tuple(SCENES) + ("many",), sat_scenes=SAT_SCENES):
    out = {g: 0.0 for g in SPREAD}
    for name in names:
        _, S64, C64 = literal_result(name, np.float64)
        _, SL, CL = literal_result(name, np.longdouble)
        for g in GROUPS:
            out[g] = max(out[g], group_distance((S64, C64), (SL, CL), g))
        for g in STATE_GROUPS:
            out[g] = max(out[g], state_distance(scene_sat(name), scene_sat(name, np.longdouble), g))
    for period in sat_scenes:
        for g in STATE_GROUPS:
            out[g] = max(out[g], state_distance(sat_literal(period),
                                                sat_literal(period, np.longdouble), g))
    return out


def named_for_missed(name, s):
    """what the world scene is named for and s does not show, from the restatement in float64
    (an empty list: all of it): every receiver solved at every measurement with every channel
    used, and navfix_scenarios.site_classes_missed"""
    n, Sx, Cx = fix_literal(s["eph"], s["first"], s["abs_sample"], s["rx_first"], s["cfg"])
    missed = []
    if not (n == s["cfg"]["max_meas"]).all() or Sx["status"].any() or not Cx["used"].all():
        missed.append("solved")
    return missed + G.site_classes_missed(Sx["lat"], Sx["lon"])


if __name__ == "__main__":
    import sys
    world = sys.argv[1:] == ["world"]
    for g, v in (measure_spread(tuple(WORLD_SCENES), ()) if world else measure_spread()).items():
        print(f'"{g}": {v:.3e},')
