"""BeiDou B1I after the data bits: a literal restatement of the Scilab receiver's field decoding
and position fix, a fast restatement vectorised over receivers, seeded scene generators and
the encoder that turns subframes back into prompt sums (tests/test_navb1_cpu.py holds the two
restatements equal and the tolerances to what they are measured from; tests/test_navb1_gpu.py
holds csrc/navb1.hip to the literal one).

    COMPASS/B1/include/ephemeris.sci:28-123                   eph_literal
    COMPASS/B1/postNavigation.sci:129-272                     fix_literal, fix_fast
    calculatePseudoranges.sci, geoFunctions/satpos.sci:45-137 satpos_literal
    leastSquarePos.sci, e_r_corr.sci, topocent.sci, togeod.sci, tropo.sci, cart2geo.sci: the
    same text as GLONASS/L1 (only whitespace differs), taken from navglo_scenarios; check_t,
    tropo and the LDL' solve with the library's rank rule from navfix_scenarios
    COMPASS/B1/include/decode_bd_data.sci:16-38               encode_subframe (its inverse)

Comments carry the files' 1-based indices.  The restatement takes the scalar type T
(numpy.float64 or numpy.longdouble) as navfix_scenarios does: constants are the files' float64
literals in both, only the operations change.  Scilab's two-argument atand is read as
(180 / %pi) * atan(y, x), and the file's 10^-9 as the double 1e-9.

mutant= switches plant one mistake each, a mistake a kernel could plausibly make:
    "gps_consts"   GM and Omegae_dot of the GPS satpos.sci
    "start_offset" the GPS receiver's startOffset of 68.802 ms added to the travel time
    "obs_sign"     obs = rawP - satClkCorr c, the sign corrP has
    "mask"         the elevation mask of 10 degrees applied as the GPS receiver does
    "alpha3_own_sign", "beta1_own_sign"   the fields' own sign bits instead of bits 88 / 120
    "e_unsigned"   e read without the subtraction
    "togeod_abs_z", "cart2geo_abs_z", "cart2geo_atan_y_over_x"   fabs(Z) for Z, and atan(Y / X)
                   for atan(Y, X) in the longitude (the world scene)
    "check_t_identity"   check_t returning its argument (the week scenes)
    "kepler_20"    the Kepler loop capped at 20 steps in place of 10 (the eccentric scene)

Tolerances.  SPREAD is the largest |literal in float64 - literal in longdouble| per output
group over every scene and measurement of SCENES and of many_rx_scene(); TOL = 16 * SPREAD.
Produced by
    python tests/navb1_scenarios.py
and copied here; test_navb1_cpu.py asserts that a fresh measurement does not exceed them, and
that every scene they are measured on has full rank and a GDOP below 6 where it is solved.
"""
import functools

import numpy as np

import navbits_scenarios as NB
import navfix_scenarios as G
import navglo_scenarios as GL

BD_PI = 3.1415926535898                     # ephemeris.sci:25, satpos.sci:30
PI = G.PI

EPH_FIELDS = ("T_GD_1", "t_oc", "a2", "a0", "a1", "alpha0", "alpha1", "alpha2", "alpha3", "beta0",
              "beta1", "beta2", "beta3", "deltan", "C_uc", "M_0", "e", "C_us", "C_rc", "C_rs",
              "sqrtA", "t_oe_msb", "t_oe_lsb", "i_0", "C_ic", "omegaDot", "C_is", "iDot",
              "omega_0", "omega", "t_oe")
EPH_INTS = ("SatH1", "IODC", "URAI", "WN", "IODE", "SOW", "have", "status")
EPH = np.dtype([(f, "<f8") for f in EPH_FIELDS] + [(f, "<i4") for f in EPH_INTS])
SOL, CHAN = G.SOL, G.CHAN
EPH_OK, EPH_SHORT, EPH_NO_SOW = 0, 1, 2
FIX_OK, FIX_FEW, FIX_RANK = G.FIX_OK, G.FIX_FEW, G.FIX_RANK

# name: (subframe, first, last (1-based), the bit whose value * 2^length is subtracted or 0,
#        exponent of 2, "" | "pi" | "tgd" | "int")
FIELDS = {
    "SatH1": (1, 28, 28, 0, 0, "int"), "IODC": (1, 29, 33, 0, 0, "int"),
    "URAI": (1, 34, 37, 0, 0, "int"), "WN": (1, 38, 50, 0, 0, "int"),
    "t_oc": (1, 51, 67, 0, 3, ""), "T_GD_1": (1, 68, 77, 68, 0, "tgd"),
    "alpha0": (1, 88, 95, 88, -30, ""), "alpha1": (1, 96, 103, 96, -27, ""),
    "alpha2": (1, 104, 111, 104, -24, ""), "alpha3": (1, 112, 119, 88, -24, ""),
    "beta0": (1, 120, 127, 120, 11, ""), "beta1": (1, 128, 135, 120, 14, ""),
    "beta2": (1, 136, 143, 136, 16, ""), "beta3": (1, 144, 151, 144, 16, ""),
    "a2": (1, 152, 162, 152, -66, ""), "a0": (1, 163, 186, 163, -33, ""),
    "a1": (1, 187, 208, 187, -50, ""), "IODE": (1, 209, 213, 0, 0, "int"),
    "deltan": (2, 28, 43, 28, -43, "pi"), "C_uc": (2, 44, 61, 44, -31, ""),
    "M_0": (2, 62, 93, 62, -31, "pi"), "e": (2, 94, 125, 94, -33, ""),
    "C_us": (2, 126, 143, 126, -31, ""), "C_rc": (2, 144, 161, 144, -6, ""),
    "C_rs": (2, 162, 179, 162, -6, ""), "sqrtA": (2, 180, 211, 0, -19, ""),
    "t_oe_msb": (2, 212, 213, 0, 18, ""),
    "t_oe_lsb": (3, 28, 42, 0, 3, ""), "i_0": (3, 43, 74, 43, -31, "pi"),
    "C_ic": (3, 75, 92, 75, -31, ""), "omegaDot": (3, 93, 116, 93, -43, "pi"),
    "C_is": (3, 117, 134, 117, -31, ""), "iDot": (3, 135, 148, 135, -43, "pi"),
    "omega_0": (3, 149, 180, 149, -31, "pi"), "omega": (3, 181, 212, 181, -31, "pi"),
}
SIGNED = tuple(k for k, v in FIELDS.items() if v[3])
EPH_MUTANTS = ("alpha3_own_sign", "beta1_own_sign", "e_unsigned")
FIX_MUTANTS = ("gps_consts", "start_offset", "obs_sign", "mask")
GEO_MUTANTS = ("togeod_abs_z", "cart2geo_abs_z", "cart2geo_atan_y_over_x")


def field_len(name):
    return FIELDS[name][2] - FIELDS[name][1] + 1


# ------------------------------------------------------------------ ephemeris.sci, literal
_bin2dec = G._bin2dec


def eph_literal_one(bits, n_subframes, first, mutant=None):
    """one channel: bits [5, 213] -> a dict of the EPH record's values"""
    out = {k: 0 for k in EPH_INTS}
    out.update({k: 0.0 for k in EPH_FIELDS})
    bits = np.asarray(bits).reshape(5, 213)
    if n_subframes < 5 or first < 0:                           # :20-22, postNavigation.sci:81
        out["status"] = EPH_SHORT
        return out
    BDPi = BD_PI                                               # :25
    decoded_sbfrm = None
    for i in range(1, 6):                                      # :28
        decoded_sbfrm = bits[i - 1]                            # decoded_sbfrm(k) = [k - 1]
        if (decoded_sbfrm > 1).any():                          # :36-39
            continue
        d = decoded_sbfrm
        val = lambda a, b: _bin2dec(d[a - 1:b])                # bin2dec(..(a:b))
        sgn = lambda a, b, s=None: val(a, b) - int(d[(s or a) - 1]) * 2 ** (b - a + 1)
        sbfrm_num = val(5, 7)                                  # :41
        if sbfrm_num == 1:                                     # :45-74
            out["SatH1"] = int(d[27])
            out["IODC"] = val(29, 33)
            out["URAI"] = val(34, 37)
            out["WN"] = val(38, 50)
            out["t_oc"] = val(51, 67) * 2.0 ** 3
            out["T_GD_1"] = sgn(68, 77) * 0.1 * 1e-9
            out["alpha0"] = sgn(88, 95) * 2.0 ** (-30)
            out["alpha1"] = sgn(96, 103) * 2.0 ** (-27)
            out["alpha2"] = sgn(104, 111) * 2.0 ** (-24)
            out["alpha3"] = sgn(112, 119, 112 if mutant == "alpha3_own_sign" else 88) \
                * 2.0 ** (-24)                                 # :58-59: decoded_sbfrm(88)
            out["beta0"] = sgn(120, 127) * 2.0 ** 11
            out["beta1"] = sgn(128, 135, 128 if mutant == "beta1_own_sign" else 120) \
                * 2.0 ** 14                                    # :62-63: decoded_sbfrm(120)
            out["beta2"] = sgn(136, 143) * 2.0 ** 16
            out["beta3"] = sgn(144, 151) * 2.0 ** 16
            out["a2"] = sgn(152, 162) * 2.0 ** (-66)
            out["a0"] = sgn(163, 186) * 2.0 ** (-33)
            out["a1"] = sgn(187, 208) * 2.0 ** (-50)
            out["IODE"] = val(209, 213)
            out["have"] |= 1
        elif sbfrm_num == 2:                                   # :76-91
            out["deltan"] = sgn(28, 43) * 2.0 ** (-43) * BDPi
            out["C_uc"] = sgn(44, 61) * 2.0 ** (-31)
            out["M_0"] = sgn(62, 93) * 2.0 ** (-31) * BDPi
            out["e"] = (val(94, 125) if mutant == "e_unsigned" else sgn(94, 125)) * 2.0 ** (-33)
            out["C_us"] = sgn(126, 143) * 2.0 ** (-31)
            out["C_rc"] = sgn(144, 161) * 2.0 ** (-6)
            out["C_rs"] = sgn(162, 179) * 2.0 ** (-6)
            out["sqrtA"] = val(180, 211) * 2.0 ** (-19)
            out["t_oe_msb"] = val(212, 213) * 2.0 ** 15 * 2.0 ** 3
            out["have"] |= 2
        elif sbfrm_num == 3:                                   # :93-107
            out["t_oe_lsb"] = val(28, 42) * 2.0 ** 3
            out["i_0"] = sgn(43, 74) * 2.0 ** (-31) * BDPi
            out["C_ic"] = sgn(75, 92) * 2.0 ** (-31)
            out["omegaDot"] = sgn(93, 116) * 2.0 ** (-43) * BDPi
            out["C_is"] = sgn(117, 134) * 2.0 ** (-31)
            out["iDot"] = sgn(135, 148) * 2.0 ** (-43) * BDPi
            out["omega_0"] = sgn(149, 180) * 2.0 ** (-31) * BDPi
            out["omega"] = sgn(181, 212) * 2.0 ** (-31) * BDPi
            out["have"] |= 4
    if out["have"] & 6 == 6:                                   # :118, both set in the file
        out["t_oe"] = out["t_oe_msb"] + out["t_oe_lsb"]
    if (decoded_sbfrm[7:27] > 1).any():                        # :123 on a 0.5: the widening
        out["status"] = EPH_NO_SOW
    else:
        out["SOW"] = _bin2dec(decoded_sbfrm[7:27]) - 24        # :123, the last slot
    return out


def eph_literal(bits, n_subframes, first, mutant=None):
    rec = np.zeros(len(bits), EPH)
    for ch in range(len(bits)):
        for k, v in eph_literal_one(bits[ch], n_subframes[ch], first[ch], mutant).items():
            rec[k][ch] = v
    return rec


# ------------------------------------------------------------------ the fix, literal
DEFAULTS = dict(samplesPerCode=16000.0, dataTypeSizeInBytes=1.0, c=299792458.0,
                navSolPeriod=500, useTropCorr=0, max_meas=1)   # initSettings.sci:59-129


def settings(**kw):
    s = dict(DEFAULTS)
    s.update(kw)
    return s


check_t, _rem, _atand = G.check_t, G._rem, G._atand


def satpos_literal(T, transmitTime, e, mutant=None, trace=None):
    """satpos.sci:53-136 for one satellite; e: a mapping of float64 fields.
    Returns (x, y, z, satClkCorr) and the |dE| of every step of the Kepler loop.  trace: a
    list that receives (time - t_oe, tk), the argument and the value of check_t at :69."""
    BDPi = T(BD_PI)
    chk = (lambda T, t: t) if mutant == "check_t_identity" else check_t
    Omegae_dot, GM, F = T(7.2921150e-5), T(3.986004418e14), T(-4.442807633e-10)   # :34-37
    if mutant == "gps_consts":
        Omegae_dot, GM = T(7.2921151467e-5), T(3.986005e14)
    g = lambda k: T(e[k])
    dt = chk(T, transmitTime - g("t_oc"))                      # :53
    satClkCorr = (g("a2") * dt + g("a1")) * dt + g("a0") - g("T_GD_1")   # :56-58
    time = transmitTime - satClkCorr                           # :61
    a = g("sqrtA") * g("sqrtA")                                # :66
    tk = chk(T, time - g("t_oe"))                              # :69
    if trace is not None:
        trace.append((time - g("t_oe"), tk))
    n0 = np.sqrt(GM / (a * a * a))                             # :72
    n = n0 + g("deltan")                                       # :74
    M = g("M_0") + n * tk                                      # :77
    M = _rem(T, M + 2 * BDPi, 2 * BDPi)                        # :79
    E = M                                                      # :82
    steps = []
    for ii in range(20 if mutant == "kepler_20" else 10):      # :85-93
        E_old = E
        E = M + g("e") * np.sin(E)
        dE = _rem(T, E - E_old, 2 * BDPi)
        steps.append(abs(dE))
        if abs(dE) < T(1.e-12):
            break
    E = _rem(T, E + 2 * BDPi, 2 * BDPi)                        # :96
    dtr = F * g("e") * g("sqrtA") * np.sin(E)                  # :99
    nu = _atand(T, np.sqrt(1 - g("e") * g("e")) * np.sin(E), np.cos(E) - g("e")) / 180 * T(PI)
    phi = nu + g("omega")                                      # :105
    phi = _rem(T, phi, 2 * BDPi)                               # :107
    u = phi + g("C_uc") * np.cos(2 * phi) + g("C_us") * np.sin(2 * phi)          # :110-112
    r = a * (1 - g("e") * np.cos(E)) + g("C_rc") * np.cos(2 * phi) + g("C_rs") * np.sin(2 * phi)
    i = g("i_0") + g("iDot") * tk + g("C_ic") * np.cos(2 * phi) + g("C_is") * np.sin(2 * phi)
    Omega = g("omega_0") + (g("omegaDot") - Omegae_dot) * tk - Omegae_dot * g("t_oe")   # :123
    Omega = _rem(T, Omega + 2 * BDPi, 2 * BDPi)                # :126
    x = np.cos(u) * r * np.cos(Omega) - np.sin(u) * r * np.cos(i) * np.sin(Omega)   # :129-131
    y = np.cos(u) * r * np.sin(Omega) + np.sin(u) * r * np.cos(i) * np.cos(Omega)
    z = np.sin(u) * r * np.sin(i)
    satClkCorr = (g("a2") * dt + g("a1")) * dt + g("a0") - g("T_GD_1") + dtr     # :134-136
    return (x, y, z, satClkCorr), steps


SAT_FIELDS = ("T_GD_1", "t_oc", "a2", "a0", "a1", "deltan", "C_uc", "M_0", "e", "C_us", "C_rc",
              "C_rs", "sqrtA", "i_0", "C_ic", "omegaDot", "C_is", "iDot", "omega_0", "omega", "t_oe")
MUTANT_MASK, MUTANT_START_OFFSET = 10.0, 68.802


def is_ready(eph, first, ch):
    return first[ch] >= 0 and eph["status"][ch] == EPH_OK and eph["have"][ch] == 7


def fix_literal(eph, first, abs_sample, rx_first, cfg, T=np.float64, mutant=None, diag=None):
    """postNavigation.sci:129-272 per receiver.  abs_sample [n_ch, n_epochs].  Returns n_meas,
    sol [n_rx, max_meas], chan [n_ch, max_meas] as dicts of T arrays (see as_records)."""
    n_rx, n_ch, mm = len(rx_first) - 1, len(eph), cfg["max_meas"]
    n_epochs = abs_sample.shape[1]
    nan, inf = T(np.nan), T(np.inf)
    S = {k: np.zeros((n_rx, mm), T) for k in ("X", "Y", "Z", "dt", "lat", "lon", "height")}
    S["DOP"] = np.zeros((n_rx, mm, 5), T)
    S["status"] = np.zeros((n_rx, mm), np.int32)
    S["n_used"] = np.zeros((n_rx, mm), np.int32)
    S["written"] = np.zeros((n_rx, mm), bool)
    S["rx_first"] = np.asarray(rx_first)
    Cn = {k: np.zeros((n_ch, mm), T) for k in ("el", "az", "rawP", "corrP")}
    Cn["used"] = np.zeros((n_ch, mm), np.int32)
    n_meas = np.zeros(n_rx, np.int32)
    c = T(cfg["c"])
    period = int(cfg["navSolPeriod"])
    with np.errstate(all="ignore"):
        for rx in range(n_rx):
            chs = list(range(rx_first[rx], rx_first[rx + 1]))
            # :117-118 are disabled in the file; the library drops what has no ephemeris
            ready = [ch for ch in chs if is_ready(eph, first, ch)]
            if len(ready) < 4:                                 # :121
                continue
            pmax = max(first[ch] for ch in chs if first[ch] >= 0)
            n_meas[rx] = max(0, min(mm, int((n_epochs - (pmax + 1)) / period)))   # :152
            transmitTime = T(int(eph["SOW"][ready[0]]))        # :145
            satElev = {ch: inf for ch in chs}                  # :135
            for m in range(n_meas[rx]):
                active = ready                                 # :156-157 are commented out
                if mutant == "mask":
                    active = [ch for ch in ready if satElev[ch] >= T(MUTANT_MASK)]
                for ch in chs:                                 # :165-166
                    Cn["el"][ch, m] = nan
                    Cn["az"][ch, m] = nan
                    Cn["used"][ch, m] = ch in active
                    Cn["corrP"][ch, m] = 0
                # calculatePseudoranges.sci
                travelTime = {ch: inf for ch in chs}
                for ch in active:
                    travelTime[ch] = T(abs_sample[ch, first[ch] + period * m]) / \
                        T(cfg["samplesPerCode"]) / T(cfg["dataTypeSizeInBytes"])
                minimum = np.floor(min(travelTime.values()))
                for ch in chs:
                    tt = travelTime[ch] - minimum
                    if mutant == "start_offset":
                        tt = tt + T(MUTANT_START_OFFSET)
                    Cn["rawP"][ch, m] = tt * (c / 1000)
                sp = []
                for ch in active:                              # :175-177
                    s, dE = satpos_literal(T, transmitTime, {k: eph[k][ch] for k in SAT_FIELDS},
                                           mutant,
                                           None if diag is None else diag.setdefault("tk", []))
                    sp.append(s)
                    if diag is not None:
                        diag["dE"].extend(dE)
                        diag.setdefault("kepler", []).append((len(dE), float(dE[-1])))
                S["written"][rx, m] = True
                S["n_used"][rx, m] = len(active)
                if len(active) > 3:                            # :183
                    sign = -1 if mutant == "obs_sign" else 1
                    obs = [Cn["rawP"][ch, m] + sign * (s[3] * c) for ch, s in zip(active, sp)]
                    if diag is not None:
                        diag["togeod"] = []
                    geo = mutant if mutant in GEO_MUTANTS else None
                    r = GL.lsq_literal(T, sp, obs, c, cfg["useTropCorr"], geo, 7, diag)   # :186
                    if r is None:                              # the library's widening
                        S["status"][rx, m] = FIX_RANK
                        for k in ("X", "Y", "Z", "dt", "lat", "lon", "height"):
                            S[k][rx, m] = 0
                        S["DOP"][rx, m] = 0
                    else:
                        pos, el, az, dop = r
                        S["X"][rx, m], S["Y"][rx, m], S["Z"][rx, m], S["dt"][rx, m] = pos
                        S["DOP"][rx, m] = dop
                        for i, ch in enumerate(active):        # :190-191
                            Cn["el"][ch, m] = el[i]
                            Cn["az"][ch, m] = az[i]
                        satElev = {ch: Cn["el"][ch, m] for ch in chs}          # :209
                        for ch, s in zip(active, sp):          # :212-214
                            Cn["corrP"][ch, m] = Cn["rawP"][ch, m] - s[3] * c + pos[3]
                        S["lat"][rx, m], S["lon"][rx, m], S["height"][rx, m] = \
                            GL.cart2geo_literal(T, pos[0], pos[1], pos[2], geo)   # :219-225
                        if diag is not None:
                            diag.setdefault("elev", []).extend(el)
                            diag.setdefault("togeod_all", []).extend(diag["togeod"])
                            diag.setdefault("cond", []).append(np.linalg.cond(diag["A"]))
                            diag.setdefault("gdop", []).append(float(dop[0]))
                else:                                          # :237-259, only under "mask"
                    S["status"][rx, m] = FIX_FEW
                    for k in ("X", "Y", "Z", "dt", "lat", "lon", "height"):
                        S[k][rx, m] = nan
                    S["DOP"][rx, m] = 0
                transmitTime = transmitTime + T(period) / 1000 # :270
    return n_meas, S, Cn


def as_records(n_meas, S, Cn, sol=None, chan=None):
    """the literal or fast results as SOL / CHAN records; rows past n_meas keep what `sol` and
    `chan` hold (zeros without them)"""
    return G.as_records(n_meas, S, Cn, sol, chan)


def fix_literal_records(eph, first, abs_sample, rx_first, cfg, sol=None, chan=None, **kw):
    n_meas, S, Cn = fix_literal(eph, first, abs_sample, rx_first, cfg, **kw)
    return (n_meas,) + as_records(n_meas, S, Cn, sol, chan)


# ------------------------------------------------------------------ the fix, fast
def _satpos_fast(t, e):
    """satpos.sci over arrays: t and every field of e of one shape"""
    two_pi = 2 * BD_PI
    Oe, GM, F = 7.2921150e-5, 3.986004418e14, -4.442807633e-10
    chk = lambda x: np.where(x > 302400.0, x - 604800.0, np.where(x < -302400.0, x + 604800.0, x))
    rem = lambda x, y: x - np.trunc(x / y) * y
    dt = chk(t - e["t_oc"])
    clk = (e["a2"] * dt + e["a1"]) * dt + e["a0"] - e["T_GD_1"]
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


def fix_fast(eph, first, abs_sample, rx_first, cfg):
    """fix_literal in float64, vectorised over receivers: arrays [n_rx, W], W the largest
    receiver; sums over a receiver's channels run in channel order with zeros for the channels
    outside the used set, which is the literal sum.  togeod, tropo, the LDL' solve and cart2geo
    are navfix_scenarios' array forms; its togeod and cart2geo take the angle through atand and
    back, a few last bits that the tolerance covers."""
    rx_first = np.asarray(rx_first)
    first = np.asarray(first)
    n_rx, n_ch, mm = len(rx_first) - 1, len(eph), cfg["max_meas"]
    n_epochs = abs_sample.shape[1]
    size = np.diff(rx_first)
    W = int(size.max())
    lane = np.arange(W)
    valid = lane[None, :] < size[:, None]
    chi = np.where(valid, rx_first[:-1, None] + lane[None, :], 0)
    e = {k: eph[k][chi] for k in SAT_FIELDS}
    fs = np.where(valid, first[chi], -1)
    used = valid & (fs >= 0) & (eph["status"][chi] == EPH_OK) & (eph["have"][chi] == 7)
    period, c = int(cfg["navSolPeriod"]), cfg["c"]
    pmax = fs.max(axis=1)
    n_used = used.sum(axis=1)
    n_meas = np.where(n_used >= 4,
                      np.clip(np.trunc((n_epochs - (pmax + 1)) / period).astype(int), 0, mm), 0)
    t = eph["SOW"][chi][np.arange(n_rx), np.argmax(used, axis=1)].astype(np.float64)
    S = {k: np.zeros((n_rx, mm)) for k in ("X", "Y", "Z", "dt", "lat", "lon", "height")}
    S["DOP"] = np.zeros((n_rx, mm, 5))
    S["status"] = np.zeros((n_rx, mm), np.int32)
    S["n_used"] = np.zeros((n_rx, mm), np.int32)
    S["written"] = np.zeros((n_rx, mm), bool)
    S["rx_first"] = rx_first
    Cn = {k: np.zeros((n_ch, mm)) for k in ("el", "az", "rawP", "corrP")}
    Cn["used"] = np.zeros((n_ch, mm), np.int32)
    dtr = PI / 180
    with np.errstate(all="ignore"):
        for m in range(int(n_meas.max(initial=0))):
            live = n_meas > m
            act = used & live[:, None]
            idx = np.clip(fs + period * m, 0, n_epochs - 1)
            travel = np.where(act, abs_sample[chi, idx] / cfg["samplesPerCode"] /
                              cfg["dataTypeSizeInBytes"], np.inf)
            minimum = np.floor(travel.min(axis=1))
            rawP = (travel - minimum[:, None]) * (c / 1000)
            sx, sy, sz, clk = _satpos_fast(t[:, None] + np.zeros((1, W)), e)
            obs = rawP + clk * c
            pos = np.zeros((4, n_rx))
            el = np.full((n_rx, W), np.nan)
            az = np.full((n_rx, W), np.nan)
            rank_ok = np.ones(n_rx, bool)
            L = d = None
            for it in range(7):
                if it == 0:
                    r0, r1, r2 = sx, sy, sz
                    trop = np.zeros((n_rx, W))
                else:
                    P0, P1, P2 = pos[0][:, None], pos[1][:, None], pos[2][:, None]
                    rho2 = (sx - P0) ** 2 + (sy - P1) ** 2 + (sz - P2) ** 2
                    omegatau = 7.292115147e-5 * (np.sqrt(rho2) / c)
                    co, so = np.cos(omegatau), np.sin(omegatau)
                    r0, r1, r2 = co * sx + so * sy, -so * sx + co * sy, sz
                    phi, lam = G._togeod_fast(pos[0], pos[1], pos[2])
                    cl, sl = np.cos(lam * dtr)[:, None], np.sin(lam * dtr)[:, None]
                    cb, sb = np.cos(phi * dtr)[:, None], np.sin(phi * dtr)[:, None]
                    d0, d1, d2 = r0 - P0, r1 - P1, r2 - P2
                    E = -sl * d0 + cl * d1 + 0 * d2
                    Nn = -sb * cl * d0 + -sb * sl * d1 + cb * d2
                    U = cb * cl * d0 + cb * sl * d1 + sb * d2
                    hd = np.sqrt(E * E + Nn * Nn)
                    az_n = np.where(hd < 1.e-20, 0.0, np.arctan2(E, Nn) / dtr)
                    el_n = np.where(hd < 1.e-20, 90.0, np.arctan2(U, hd) / dtr)
                    az_n = np.where(az_n < 0, az_n + 360, az_n)
                    upd = (live & rank_ok)[:, None]
                    az, el = np.where(upd, az_n, az), np.where(upd, el_n, el)
                    trop = G._tropo_fast(np.sin(el_n * dtr)) if cfg["useTropCorr"] == 1 \
                        else np.zeros((n_rx, W))
                P0, P1, P2 = pos[0][:, None], pos[1][:, None], pos[2][:, None]
                d0, d1, d2 = r0 - P0, r1 - P1, r2 - P2
                dist = np.sqrt(d0 ** 2 + d1 ** 2 + d2 ** 2)
                F = np.where(act, obs - pos[3][:, None] - dist - trop, 0.0)
                A = [np.where(act, (-d0) / dist, 0.0), np.where(act, (-d1) / dist, 0.0),
                     np.where(act, (-d2) / dist, 0.0), np.where(act, 1.0, 0.0)]
                N = [[np.zeros(n_rx) for _ in range(4)] for _ in range(4)]
                g = [np.zeros(n_rx) for _ in range(4)]
                for w in range(W):
                    for r in range(4):
                        for s in range(r + 1):
                            N[r][s] = N[r][s] + A[r][:, w] * A[s][:, w]
                        g[r] = g[r] + A[r][:, w] * F[:, w]
                Ln, dn, ok = G._ldl_fast(N)
                step = live & rank_ok & ok
                x = G._ldl_solve_fast(Ln, dn, g)
                if L is None:
                    L, d = Ln, dn
                else:
                    L = [[None if Ln[i][j] is None else np.where(step, Ln[i][j], L[i][j])
                          for j in range(4)] for i in range(4)]
                    d = [np.where(step, dn[j], d[j]) for j in range(4)]
                pos = np.where(step[None, :], pos + np.array(x), pos)
                rank_ok = rank_ok & (ok | ~live)
            good = live & rank_ok
            bad = live & ~rank_ok
            Q = [G._ldl_solve_fast(L, d, [np.full(n_rx, float(k == j)) for k in range(4)])[j]
                 for j in range(4)]
            dop = np.stack([np.sqrt(Q[0] + Q[1] + Q[2] + Q[3]), np.sqrt(Q[0] + Q[1] + Q[2]),
                            np.sqrt(Q[0] + Q[1]), np.sqrt(Q[2]), np.sqrt(Q[3])], axis=1)
            lat, lon, hgt = G._cart2geo_fast(np.where(good, pos[0], 1.0), np.where(good, pos[1], 1.0),
                                             np.where(good, pos[2], 1.0))
            for k, v in (("X", pos[0]), ("Y", pos[1]), ("Z", pos[2]), ("dt", pos[3]),
                         ("lat", lat), ("lon", lon), ("height", hgt)):
                S[k][:, m] = np.where(good, v, 0.0)
            S["DOP"][:, m] = np.where(good[:, None], dop, 0.0)
            S["status"][:, m] = np.where(bad, FIX_RANK, FIX_OK)
            S["n_used"][:, m] = np.where(live, n_used, 0)
            S["written"][:, m] = live
            el_out = np.where(good[:, None] & act, el, np.nan)
            az_out = np.where(good[:, None] & act, az, np.nan)
            corrP = np.where(good[:, None] & act, rawP - clk * c + pos[3][:, None], 0.0)
            sel = valid & live[:, None]
            for k, v in (("el", el_out), ("az", az_out), ("rawP", rawP), ("corrP", corrP),
                         ("used", act)):
                Cn[k][chi[sel], m] = v[sel]
            t = t + period / 1000
    return n_meas.astype(np.int32), S, Cn


# ------------------------------------------------------------------ scene generators
def eph_ints(rng, kind="random"):
    """the raw field integers of one ephemeris (unsigned bit patterns)"""
    raw = {k: int(rng.integers(0, 1 << field_len(k))) for k in FIELDS}
    if kind == "ones":
        raw.update({k: (1 << field_len(k)) - 1 for k in FIELDS})
    elif kind == "signbit":
        raw.update({k: 1 << (field_len(k) - 1) for k in SIGNED})
    elif kind == "negative":
        raw.update({k: raw[k] | 1 << (field_len(k) - 1) for k in SIGNED})
    elif kind == "quirk88":                                    # bit 88 set, alpha3 clear
        raw.update(alpha0=0x80 | raw["alpha0"], alpha3=0)
    elif kind == "quirk120":                                   # bit 120 set, beta1 clear
        raw.update(beta0=0x80 | raw["beta0"], beta1=0)
    elif kind == "e_top":
        raw.update(e=raw["e"] | 1 << 31)
    return raw


def raw_to_values(raw):
    """what the file makes of the raw integers, field by field"""
    out = {}
    for k, (sf, a, b, sg, ex, kind) in FIELDS.items():
        n = b - a + 1
        v = raw[k]
        if sg:
            owner = next(o for o, f in FIELDS.items() if f[:2] == (sf, sg))   # whose top bit
            v -= (raw[owner] >> (field_len(owner) - 1)) << n
        if kind == "int":
            out[k] = v
        elif kind == "tgd":
            out[k] = v * 0.1 * 1e-9
        else:
            x = float(v) * 2.0 ** ex
            out[k] = x * BD_PI if kind == "pi" else x
    out["t_oe"] = out["t_oe_msb"] + out["t_oe_lsb"]
    return out


def values_to_raw(vals, rng):
    """the nearest grid integers of physical values; fields not in vals are random, with
    bits 88 and 120 clear so that alpha3 and beta1 stay what they are.  t_oe is split."""
    raw = eph_ints(rng)
    raw["alpha0"] &= 0x7f
    raw["beta0"] &= 0x7f
    vals = dict(vals)
    if "t_oe" in vals:
        t = int(vals.pop("t_oe"))
        assert t % 8 == 0 and 0 <= t < 1 << 20
        raw["t_oe_msb"], raw["t_oe_lsb"] = t >> 18, (t >> 3) & 0x7fff
    for k, v in vals.items():
        sf, a, b, sg, ex, kind = FIELDS[k]
        n = b - a + 1
        if kind == "int":
            q = int(v)
        elif kind == "tgd":
            q = int(round(v / 1e-10))
        else:
            q = int(round(v / (2.0 ** ex * (BD_PI if kind == "pi" else 1.0))))
        lo, hi = (-(1 << (n - 1)), (1 << (n - 1)) - 1) if sg else (0, (1 << n) - 1)
        assert lo <= q <= hi, (k, v)
        raw[k] = q & ((1 << n) - 1)
    return raw


def subframe_bits(rng, sid, raw, sow):
    """213 deinterleaved bits of a subframe with ID sid: bits 5..7 the ID, 8..27 the SOW, the
    fields of `raw` that belong to it, everything else random"""
    b = rng.integers(0, 2, 213).astype(np.uint8)
    put = lambda a, v, n: b.__setitem__(slice(a - 1, a - 1 + n),
                                        [(v >> (n - 1 - i)) & 1 for i in range(n)])
    put(5, sid, 3)
    put(8, sow, 20)
    for k, (sf, a, z, sg, ex, kind) in FIELDS.items():
        if sf == sid:
            put(a, raw[k], z - a + 1)
    return b


def frame_bits(rng, ids, raw, sow=1000):
    """[5, 213] bits: slots with the IDs `ids` and SOW sow, sow + 6, ..; a repeated ID carries
    other field values the first time, so the later one must win"""
    out = []
    for j, sid in enumerate(ids):
        r = eph_ints(rng) if sid in ids[j + 1:] else raw
        out.append(subframe_bits(rng, sid, r, sow + 6 * j))
    return np.array(out, np.uint8)


ROTATIONS = ((1, 2, 3, 4, 5), (2, 3, 4, 5, 1), (3, 4, 5, 1, 2), (4, 5, 1, 2, 3), (5, 1, 2, 3, 4))
ORDERS = ROTATIONS + ((1, 1, 2, 3, 4), (4, 2, 3, 4, 5), (1, 5, 3, 4, 5), (1, 2, 4, 5, 5),
                      (0, 7, 1, 2, 3), (3, 2, 1, 6, 3))
KINDS = ("random", "negative", "ones", "signbit")
SPECIAL_KINDS = {13: "quirk88", 14: "quirk120", 15: "e_top"}


@functools.lru_cache(None)
def eph_scene(n_ch, seed=11):
    """bits [n_ch, 5, 213], n_subframes, first, the slot IDs and planted raw integers per
    channel: every order of ORDERS and the four kinds of field patterns in turn; the refusals,
    the undecided values and the quirk cases spread over the channels of the large scene"""
    rng = np.random.default_rng(seed)
    bits = np.zeros((n_ch, 5, 213), np.uint8)
    raws, orders = [], []
    n_sub = np.full(n_ch, 5, np.int32)
    first = rng.integers(0, 900, n_ch).astype(np.int32)
    for ch in range(n_ch):
        kind = SPECIAL_KINDS.get(ch, KINDS[ch % 4]) if n_ch >= 32 else KINDS[ch % 4]
        raw = eph_ints(rng, kind)
        ids = ORDERS[ch % len(ORDERS)]
        if n_ch >= 32 and ch in SPECIAL_KINDS:
            ids = ROTATIONS[ch % 5]
        raws.append(raw)
        orders.append(ids)
        bits[ch] = frame_bits(rng, ids, raw, int(rng.integers(24, 100000)))
    if n_ch >= 3:
        n_sub[1] = 4
        bits[1, 4] = 0
    if n_ch >= 32:
        n_sub[8] = 0
        bits[8] = 0
        first[9] = -1
        bits[10, orders[10].index(2), 99] = 2                  # inside e: the slot with ID 2 goes
        bits[11, 4, 150] = 2                                   # slot 5, outside bits 8..27
        bits[12, 4, 12] = 2                                    # slot 5, inside bits 8..27
        bits[16, 0, 2] = 2                                     # slot 1, a reserved bit
    return bits, n_sub, first, tuple(orders), tuple(raws)


# orbits and geometry --------------------------------------------------------
RX_ECEF = G.RX_ECEF
_elevation, _near, _gdop = G._elevation, G._near, G._gdop
WEEK = 604800


def draw_satellite(rng, tow, toe, pos, el_lo, el_hi, span=4.0, e=(0.001, 0.01), i_0=None,
                   geo=False):
    """a BeiDou-like orbit, MEO (sqrtA near 5282) or IGSO (near 6493), on the message's grid,
    whose elevation from pos at tow lies in [el_lo, el_hi] and whose Kepler loop, at tow and
    `span` seconds on, takes no step with |dE| within a factor 4 of its 1e-12 exit.  e, i_0:
    the ranges the eccentricity and the inclination [rad] are drawn from (i_0 None: 0.96 +-
    0.03); from e = 0.1 on only orbits whose loop runs all 10 steps are kept.  geo: a GEO-like
    orbit, sqrtA near 6493.4 with i_0 in 0 .. 0.1 rad and e below 0.001.  Returns the raw
    integers and the position at tow."""
    if geo:
        e, i_0 = (0.0001, 0.001), (0.0, 0.1)
    while True:
        igso = bool(rng.integers(0, 2)) or geo
        vals = dict(sqrtA=(6493.4 if igso else 5282.6) + rng.uniform(-0.5, 0.5),
                    e=rng.uniform(*e),
                    i_0=0.96 + rng.uniform(-0.03, 0.03) if i_0 is None else rng.uniform(*i_0),
                    omega_0=rng.uniform(-PI, PI), omega=rng.uniform(-PI, PI),
                    M_0=rng.uniform(-PI, PI), deltan=rng.uniform(1e-9, 4e-9),
                    omegaDot=rng.uniform(-8e-9, -2e-9), iDot=rng.uniform(-5e-10, 5e-10),
                    t_oe=toe, t_oc=toe, a0=rng.uniform(-5e-4, 5e-4),
                    a1=rng.uniform(-1e-11, 1e-11), a2=0.0, T_GD_1=rng.uniform(-2e-8, 2e-8),
                    **{k: rng.uniform(-1e-6, 1e-6) for k in ("C_uc", "C_us", "C_ic", "C_is")},
                    **{k: rng.uniform(-100, 100) for k in ("C_rc", "C_rs")})
        raw = values_to_raw(vals, rng)
        v = raw_to_values(raw)
        s, dE = satpos_literal(np.float64, np.float64(tow), v)
        dE2 = satpos_literal(np.float64, np.float64(tow + span), v)[1]
        if e[0] >= 0.1 and not (G.full_kepler_loop(dE) and G.full_kepler_loop(dE2)):
            continue
        if el_lo <= _elevation(pos, s) <= el_hi and not _near(dE + dE2, 1e-12):
            return raw, s


def plant_abs_samples(eph, first, chans, tow, pos, cfg, n_epochs, n_meas, trop, offset_ms=0.3):
    """absoluteSample rows [len(chans), n_epochs] for one receiver at `pos`: at measurement m
    every channel's pseudorange is the geometric range (to the satellite turned by the Earth's
    rotation over the travel time) + troposphere - satClkCorr c + a common clock term chosen so
    that the smallest travel time sits offset_ms above a whole millisecond.  Other epochs hold
    NaN."""
    T = np.float64
    c, period = T(cfg["c"]), cfg["navSolPeriod"]
    spc = cfg["samplesPerCode"] * cfg["dataTypeSizeInBytes"]
    out = np.full((len(chans), n_epochs), np.nan)
    t = T(tow)
    for m in range(n_meas):
        rawp = []
        for ch in chans:
            (x, y, z, clk), _ = satpos_literal(T, t, {k: eph[k][ch] for k in SAT_FIELDS})
            rho = T(2.2e7)
            for _ in range(8):                                 # fixed point of the rotation
                w = T(7.292115147e-5) * (rho / c)
                rx = [np.cos(w) * x + np.sin(w) * y, -np.sin(w) * x + np.cos(w) * y, z]
                rho = np.sqrt(sum((rx[k] - pos[k]) ** 2 for k in range(3)))
            tr = G.tropo_literal(T, np.sin(np.radians(_elevation(pos, rx)))) if trop else T(0)
            rawp.append(rho + tr - clk * c)
        rawp = np.array(rawp) / (c / 1000)                     # ms, up to the clock term
        ms = rawp - rawp.min() + offset_ms
        for i, ch in enumerate(chans):
            out[i, first[ch] + period * m] = (ms[i] + (1000 + period * m)) * spc
        t = t + T(period) / 1000
    return out


def make_fix_scene(seed, sizes, n_epochs=200, period=20, max_meas=7, trop=0, low=(), no_sf=(),
                   no_sow=(), not_ready=(), odd_sow=(), clone=(), first_lo=0, first_hi=15,
                   week=None, sites=None, e=(0.001, 0.01), i_0=None, geo=(), rx_seeds=None):
    """sizes: channels per receiver.  low: {receiver: number of satellites between 3 and 7
    degrees} (its last lanes; used all the same, the receiver has no mask).  no_sf: (receiver,
    lane, ID) whose frame lacks the subframe with that ID; no_sow / not_ready: (receiver, lane)
    pairs with a 2 inside bits 8..27 of slot 5 / with first = -1; odd_sow: pairs whose SOW is
    600 s off the others'; clone: receivers in which every channel carries channel 0's
    ephemeris and absoluteSample (rank 1).  week: "start" puts SOW near the start of the week
    with t_oe and t_oc at the end of the week before (check_t adds a week), "end" the other way
    round (check_t subtracts one).  sites: (latitude, longitude) in degrees per receiver, in
    place of RX_ECEF; the 200 km of jitter and the rescaling to 6371 km stay.  e, i_0:
    draw_satellite's ranges.  geo: {receiver: number of GEO-like satellites}, its first lanes.  rx_seeds: a seed per receiver for its own
    generator (jitter, satellites, frame filler) in place of the scene's, so that one
    receiver's draw can be searched with the others kept."""
    rng = np.random.default_rng(seed)
    cfg = settings(navSolPeriod=period, max_meas=max_meas, useTropCorr=trop)
    rx_first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n_ch = int(rx_first[-1])
    bits = np.zeros((n_ch, 5, 213), np.uint8)
    first = rng.integers(first_lo, first_hi, n_ch).astype(np.int32)
    planted = []
    if week == "start":
        sow, toe = 6 * int(rng.integers(20, 200)), WEEK - 3600
    elif week == "end":
        sow, toe = WEEK - 6 * int(rng.integers(20, 200)), 1800
    else:
        sow = 6 * int(rng.integers(2000, 90000))
        toe = sow - sow % 3600 + (3600 if rng.integers(0, 2) else 0)
    missing = {(r, l): i for r, l, i in no_sf}
    scene_rng = rng
    for rx, size in enumerate(sizes):
        rng = scene_rng if rx_seeds is None else np.random.default_rng(rx_seeds[rx])
        pos = (np.array(RX_ECEF) if sites is None else G.site_ecef(sites[rx])) + \
            rng.uniform(-2e5, 2e5, 3)
        pos *= 6371000.0 / np.linalg.norm(pos)
        planted.append(pos)
        n_low, n_geo = dict(low).get(rx, 0), dict(geo).get(rx, 0)
        bad = [(r, l) for r, l in (*missing, *no_sow, *not_ready) if r == rx]
        while True:                                            # a geometry with GDOP < 5
            drawn = [draw_satellite(rng, sow, toe, pos, *((3.0, 7.0) if lane >= size - n_low
                                                          else (18.0, 85.0)), e=e, i_0=i_0,
                                    geo=lane < n_geo) for lane in range(size)]
            use = [lane for lane in range(size) if (rx, lane) not in bad]
            if len(use) < 4 or rx in clone:
                break
            if _gdop(pos, [drawn[l][1] for l in use]) < 5:
                break
        for lane in range(size):
            ch = rx_first[rx] + lane
            ids = ROTATIONS[ch % 5]
            if (rx, lane) in missing:
                ids = tuple(4 if i == missing[rx, lane] else i for i in ids)
            bits[ch] = frame_bits(rng, ids, drawn[lane][0], sow + (600 if (rx, lane) in odd_sow else 0))
            if (rx, lane) in no_sow:
                bits[ch, 4, 20] = 2
            if (rx, lane) in not_ready:
                first[ch] = -1
        if rx in clone:
            for lane in range(1, size):
                bits[rx_first[rx] + lane] = bits[rx_first[rx]]
                first[rx_first[rx] + lane] = first[rx_first[rx]]
    n_sub = np.full(n_ch, 5, np.int32)
    eph = eph_literal(bits, n_sub, first)
    abs_sample = np.full((n_ch, n_epochs), np.nan)
    for rx, size in enumerate(sizes):
        every = range(rx_first[rx], rx_first[rx + 1])
        chans = [ch for ch in every if is_ready(eph, first, ch)]
        pm = max([first[ch] for ch in every if first[ch] >= 0], default=0)
        nm = max(0, min(max_meas, (n_epochs - (pm + 1)) // period))
        if chans:
            abs_sample[chans] = plant_abs_samples(eph, first, chans, sow, planted[rx], cfg,
                                                  n_epochs, nm, trop)
        if rx in clone:
            for ch in range(rx_first[rx] + 1, rx_first[rx + 1]):
                abs_sample[ch] = abs_sample[rx_first[rx]]
    return dict(bits=bits, n_subframes=n_sub, first=first, eph=eph, abs_sample=abs_sample,
                rx_first=rx_first, cfg=cfg, planted=np.array(planted), sizes=tuple(sizes),
                sow=sow, toe=toe)


SCENES = {
    # name: (arguments of make_fix_scene, every receiver solved at full rank)
    "one_rx_4": (dict(seed=1, sizes=(4,), max_meas=2), True),
    "one_rx_5": (dict(seed=2, sizes=(5,), max_meas=7), True),
    "three_rx": (dict(seed=3, sizes=(12, 4, 7), max_meas=3), True),
    "wave64": (dict(seed=4, sizes=(64,), max_meas=1, n_epochs=120), True),
    "trop": (dict(seed=5, sizes=(6, 9), max_meas=2, trop=1), True),
    "low_sats": (dict(seed=6, sizes=(7,), max_meas=3, trop=1, low={0: 2}), True),
    "three_ready": (dict(seed=7, sizes=(5, 6), max_meas=2, not_ready=((0, 1), (0, 3))), True),
    "dropped": (dict(seed=8, sizes=(6, 6), max_meas=2, no_sf=((0, 2, 2),), no_sow=((1, 4),)), True),
    "first_not_ready": (dict(seed=9, sizes=(6,), max_meas=2, no_sf=((0, 0, 3),), no_sow=((0, 5),),
                             odd_sow=((0, 0), (0, 5))), True),
    "rank": (dict(seed=10, sizes=(5, 6), max_meas=2, clone=(0,)), False),
    "week_start": (dict(seed=11, sizes=(5,), max_meas=2, week="start"), True),
    "week_end": (dict(seed=12, sizes=(6,), max_meas=2, week="end"), True),
    "max_meas_below": (dict(seed=13, sizes=(5,), max_meas=2, n_epochs=300), True),
}


# the scenes that reach what SCENES does not: one receiver at every site of
# navfix_scenarios.SITES in one launch, Kepler loops that leave by the cap, and GEO-like orbits
# among MEO and IGSO ones seen from (20 N, 110 E).  eccentric and geo: the seed is the first
# tried; the scene passes conditions_hold and shows what it is named for
# (navfix_scenarios.search_seed).  world: in this least-squares text the first togeod call of a
# fix, on the position after one step from the origin, leaves its loop at 3e-11 to 1e-10 at
# sites between 12 and 22 degrees of latitude unless the geometry makes it take one step more,
# about one draw in three; so every receiver has a seed of its own, the first of 1000 rx + 0,
# 1, .. at which it passes alone (navfix_scenarios.search_rx_seeds: the second for S-E, the
# fourth for the western side of the 180 degree meridian, the first for the rest).  No site
# was moved.  useTropCorr is one setting per launch: on for all eleven.  e stops at 0.24
# where the GPS scene goes to 0.3: the file reads the 32-bit field as signed, which ends at 0.25.
WORLD_SCENES = {
    "world": (dict(seed=100, sizes=G.WORLD_SIZES, max_meas=2, trop=1, sites=G.world_sites(),
                   rx_seeds=(0, 1001, 2000, 3000, 4003, 5000, 6000, 7000, 8000, 9000, 10000)),
              True),
    "eccentric": (dict(seed=400, sizes=(6,), max_meas=2, e=(0.1, 0.24)), True),
    "geo": (dict(seed=600, sizes=(8,), max_meas=2, trop=1, sites=((20.0, 110.0),), geo={0: 3}),
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
def literal_result(name, T=np.float64, mutant=None):
    s = _scene(name)
    eph = s["eph"]
    if mutant in EPH_MUTANTS:
        eph = eph_literal(s["bits"], s["n_subframes"], s["first"], mutant)
    return fix_literal(eph, s["first"], s["abs_sample"], s["rx_first"], s["cfg"], T, mutant)


def scene_diagnostics(s):
    """what the scene conditions are asserted on, from the literal restatement in float64:
    cond(A) and GDOP of every solved measurement, every elevation, the |dE| at every exit of
    the Kepler loop and the residual at every exit of togeod's loop"""
    diag = {"dE": []}
    fix_literal(s["eph"], s["first"], s["abs_sample"], s["rx_first"], s["cfg"], diag=diag)
    return {k: np.array(diag.get(k, []), np.float64)
            for k in ("cond", "gdop", "elev", "dE", "togeod_all", "tk", "kepler")}


def conditions_hold(s, full_rank=True):
    """navfix_scenarios.conditions_hold without the mask: no Kepler or togeod exit within a
    factor 4 of its threshold; cond(A) < 1e6 and GDOP < 6 wherever a receiver is solved"""
    d = scene_diagnostics(s)
    ok = not _near(d["dE"][np.isfinite(d["dE"])], 1e-12) and not _near(d["togeod_all"], 1e-10)
    if full_rank:
        ok = ok and (d["cond"] < 1e6).all() and (d["gdop"] < 6).all()
    return bool(ok)


# the chain ---------------------------------------------------------------------
def encode_subframe(rng, dec):
    """decode_bd_data.sci:29-38 inverted: 213 deinterleaved bits -> the 300 symbols +-1 of a
    subframe.  Symbols 1..11 are the preamble, 12..26 the first 15 bits; word w = 1..9 carries
    its 22 bits as 11 at the odd positions then 11 at the even ones; the parity symbols the
    file never reads are random."""
    y = 2 * rng.integers(0, 2, 300) - 1
    d = 2 * np.asarray(dec, int) - 1
    y[:11] = NB.B1_PREAMBLE
    y[11:26] = d[:15]
    for w in range(1, 10):
        word = d[15 + 22 * (w - 1):15 + 22 * w]
        y[30 * w:30 * w + 22:2] = word[:11]                    # current_word(1:2:21)
        y[30 * w + 1:30 * w + 22:2] = word[11:]                # current_word(2:2:22)
    return y


def subframes_to_series(rng, bits, first, n_epochs, amp=800.0):
    """the prompt sums of one channel whose five subframes decode to bits [5, 213]: random
    epochs up to `first`, then the symbols under the Neumann-Hoffman code (:19-22 inverted),
    then random symbols"""
    x = 2.0 * rng.integers(0, 2, first) - 1
    for i in range(5):
        x = np.concatenate([x, np.kron(encode_subframe(rng, bits[i]), NB.B1_SECONDARY).astype(float)])
    tail = np.kron(2 * rng.integers(0, 2, max(n_epochs - len(x), 0) // 20 + 1) - 1,
                   NB.B1_SECONDARY).astype(float)
    x = np.concatenate([x, tail])[:n_epochs]
    return amp * x * (1.0 + 0.2 * rng.random(n_epochs))


@functools.lru_cache(None)
def chain_scene(seed=41, n_ch=6, n_epochs=31000, max_meas=3):
    """One receiver for the device chain: a fix scene without troposphere whose first positions
    leave room for five subframes, and the I_P series [n_ch, n_epochs] that carry them"""
    s = make_fix_scene(seed, (n_ch,), n_epochs=n_epochs, period=20, max_meas=max_meas,
                       first_lo=100, first_hi=900)
    rng = np.random.default_rng(seed + 1)
    series = np.stack([subframes_to_series(rng, s["bits"][ch], int(s["first"][ch]), n_epochs)
                       for ch in range(n_ch)])
    return s, series


# tolerances ----------------------------------------------------------------------
GROUPS = dict(G.GROUPS)

# the largest |float64 - longdouble| of the literal restatement over SCENES and many_rx_scene(),
# per group (metres, metres, -, degrees, metres, degrees, metres), from
# `python tests/navb1_scenarios.py`
SPREAD = {"xyz": 2.044e-07, "dt": 1.258e-07, "dop": 1.332e-13, "latlon": 1.561e-12,
          "height": 1.932e-07, "elaz": 4.399e-12, "corrP": 1.570e-07}
TOL = {k: 16 * v for k, v in SPREAD.items()}

# the same over WORLD_SCENES alone, from `python tests/navb1_scenarios.py world`
SPREAD_WORLD = {"xyz": 1.001e-07, "dt": 6.779e-08, "dop": 4.881e-14, "latlon": 1.813e-12,
                "height": 9.244e-08, "elaz": 1.820e-12, "corrP": 1.033e-07}
TOL_WORLD = {k: 16 * v for k, v in SPREAD_WORLD.items()}

group_distance = G.group_distance


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
    every measurement; no check_t wraps; world: navfix_scenarios.site_classes_missed;
    eccentric: every Kepler loop ran 10 steps and left by the cap with |dE| > 4e-12; geo: three
    orbits with sqrtA above 6000, i_0 below 0.1 rad and e below 0.001, a MEO and an IGSO one"""
    diag = {"dE": []}
    n, Sx, Cx = fix_literal(s["eph"], s["first"], s["abs_sample"], s["rx_first"], s["cfg"],
                            diag=diag)
    missed = []
    if not (n == s["cfg"]["max_meas"]).all() or Sx["status"].any() or not Cx["used"].all():
        missed.append("solved")
    tk = np.array(diag["tk"], np.float64)
    if not (tk[:, 1] == tk[:, 0]).all():
        missed.append("check_t")
    kep = np.array(diag["kepler"], np.float64)
    if name == "eccentric" and not ((kep[:, 0] == 10) & (kep[:, 1] > 4e-12)).all():
        missed.append("kepler")
    if name == "geo":
        e = s["eph"]
        is_geo = (e["sqrtA"] > 6000) & (np.abs(e["i_0"]) < 0.1) & (e["e"] < 0.001)
        igso = (e["sqrtA"] > 6000) & (e["i_0"] > 0.9)
        if not (is_geo.sum() == 3 and igso.any() and (e["sqrtA"] < 6000).any()):
            missed.append("orbits")
    if name == "world":
        missed += G.site_classes_missed(Sx["lat"], Sx["lon"])
    return missed


if __name__ == "__main__":
    import sys
    world = sys.argv[1:] == ["world"]
    for g, v in (measure_spread(tuple(WORLD_SCENES)) if world else measure_spread()).items():
        print(f'"{g}": {v:.3e},')
