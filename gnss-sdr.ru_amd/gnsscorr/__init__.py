"""gnsscorr -- Python (ctypes) view of libgnsscorr.so, the MI355X GNSS correlator.

This module is plumbing for tests and benchmarks: every computation happens in
the HIP kernels behind the C ABI declared in include/gnsscorr.h.  There is no
CPU fallback -- if the shared library (or a GPU, for compute calls) is
missing, the calls raise.

Two views are provided:

* ``TrackCtx`` / ``AcqCtx``: the batched API (explicit state, many channels).
* ``OSG``: the reference's GP2021 register interface (correlator_init,
  Sim_GP2021_int, REG_read/REG_write + the gp2021.c accessors ch_carrier,
  ch_code, ch_code_slew, ch_cntl, ch_epoch_load, ch_{i,q}_{early,prompt,late},
  accum_status), so host-loop tests read like the reference's own
  osgnss_next_step.c main loop.
"""
from __future__ import annotations

import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# GNSSCORR_LIB: an alternative build of the same library (A/B timing in tools/)
LIB_PATH = os.environ.get("GNSSCORR_LIB") or os.path.join(_HERE, "libgnsscorr.so")

# ---------------------------------------------------------------- structs
NCO_CMD = np.dtype([("prn", "<i4"), ("carrier_incr", "<u4"), ("code_incr", "<u4"),
                    ("slew", "<u4"), ("epoch_load", "<i4"), ("stream", "<i4")])
CHAN_STATE = np.dtype([("carrier_phase", "<u4"), ("carrier_cycle", "<u4"),
                       ("code_phase", "<u4"), ("half_chip", "<u4"), ("acc", "<i4", (6,)),
                       ("ms_counter", "<i4"), ("bit_counter", "<i4"), ("msbit_reg", "<i4"),
                       ("pad", "<i4")])
TRACK_RESULT = np.dtype([("n_dumps", "<i4"), ("dump", "<i4", (6,)), ("msbit_reg", "<i4"),
                         ("tic", "<i4"), ("tic_regs", "<i4", (6,)), ("pad", "<i4")])
ACQ_ROW = np.dtype([("peak", "<f8"), ("second", "<f8"), ("argmax", "<i4"), ("block", "<i4")])
ACQ_RESULT = np.dtype([("peak", "<f8"), ("second", "<f8"), ("metric", "<f8"), ("bin", "<i4"),
                       ("code_phase", "<i4"), ("pad", "<i4"), ("pad2", "<i4"),
                       ("carr_freq", "<f8")])
SIG = np.dtype([("system", "<i4"), ("prn", "<i4"), ("fch", "<i4"), ("data_bits", "<i4"),
                ("code_phase", "<f8"), ("doppler", "<f8"), ("cn0", "<f8"),
                ("carr_phase", "<f8")])
assert NCO_CMD.itemsize == 24 and CHAN_STATE.itemsize == 56 and TRACK_RESULT.itemsize == 64
assert ACQ_ROW.itemsize == 24 and ACQ_RESULT.itemsize == 48 and SIG.itemsize == 48

OSG_LOOP = np.dtype([("state", "<i4"), ("n_freq", "<i4"), ("i_confirm", "<i4"),
                     ("n_thresh", "<i4"), ("codes", "<i4"), ("del_freq", "<i4"),
                     ("sign_pos", "<i4"), ("prev_sign_pos", "<i4"), ("sign_count", "<i4"),
                     ("ms_count", "<i4"), ("ms_set", "<i4"), ("search_max_prn_delay", "<i4"),
                     ("search_max_f", "<i4"), ("cn0", "<i4"), ("bit", "<i4"), ("exited", "<i4"),
                     ("accum", "<i2", (6,)), ("prev_accum", "<i2", (6,)),
                     ("early_mag", "<i8"), ("prompt_mag", "<i8"), ("late_mag", "<i8"),
                     ("cross", "<i8"), ("dot", "<i8"), ("carr_error", "<i8"),
                     ("old_carr_error", "<i8"), ("freq_error", "<i8"), ("carr_nco", "<i8"),
                     ("old_carr_nco", "<i8"), ("carr_freq", "<i8"), ("carr_freq_basis", "<i8"),
                     ("code_error", "<i8"), ("old_code_error", "<i8"), ("code_freq", "<i8"),
                     ("code_freq_basis", "<i8"), ("code_nco", "<i8"), ("old_code_nco", "<i8"),
                     ("ch_time", "<i8"), ("carrier_freq", "<i8"), ("carrier_cold_corr", "<i8"),
                     ("ms_sign", "<u8")])
assert OSG_LOOP.itemsize == 264

SGT_CHAN = np.dtype([("code_id", "<i4"), ("stream", "<i4"), ("status", "<i4"),
                     ("n_epochs", "<i4"), ("pos", "<i8"), ("pad", "<i8"),
                     ("rem_code", "<f8"), ("rem_carr", "<f8"), ("code_freq", "<f8"),
                     ("carr_freq", "<f8"), ("carr_freq_basis", "<f8"), ("old_code_nco", "<f8"),
                     ("old_code_error", "<f8"), ("old_carr_nco", "<f8"),
                     ("old_carr_error", "<f8"), ("i1", "<f8"), ("q1", "<f8"), ("pad2", "<f8")])
SGT_EPOCH = np.dtype([("I_E", "<f8"), ("I_P", "<f8"), ("I_L", "<f8"), ("Q_E", "<f8"),
                      ("Q_P", "<f8"), ("Q_L", "<f8"), ("carrFreq", "<f8"), ("codeFreq", "<f8"),
                      ("absoluteSample", "<f8"), ("dllDiscr", "<f8"), ("dllDiscrFilt", "<f8"),
                      ("pllDiscr", "<f8"), ("pllDiscrFilt", "<f8"), ("blksize", "<i4"),
                      ("status", "<i4")])
assert SGT_CHAN.itemsize == 128 and SGT_EPOCH.itemsize == 112
E1T_SUMS = ("I_E_P", "I_P_E", "I_P_P", "I_P_L", "I_L_P", "Q_E_P", "Q_P_E", "Q_P_P", "Q_P_L",
            "Q_L_P")   # first letter: subcarrier arm, second: code arm
E1T_CHAN = np.dtype([("code_id", "<i4"), ("stream", "<i4"), ("status", "<i4"),
                     ("n_epochs", "<i4"), ("segment", "<i4"), ("pad", "<i4"), ("pos", "<i8"),
                     ("rem_code", "<f8"), ("rem_meandr", "<f8"), ("rem_carr", "<f8"),
                     ("code_freq", "<f8"), ("meandr_freq", "<f8"), ("carr_freq", "<f8"),
                     ("carr_freq_basis", "<f8"), ("old_code_nco", "<f8"),
                     ("old_code_error", "<f8"), ("old_meandr_nco", "<f8"),
                     ("old_meandr_error", "<f8"), ("old_carr_nco", "<f8"),
                     ("old_carr_error", "<f8"), ("i1", "<f8"), ("q1", "<f8"), ("pad2", "<f8")])
E1T_EPOCH = np.dtype([(f, "<f8") for f in E1T_SUMS] +
                     [("carrFreq", "<f8"), ("codeFreq", "<f8"), ("meandrFreq", "<f8"),
                      ("absoluteSample", "<f8"), ("dllDiscr", "<f8"), ("dllDiscrFilt", "<f8"),
                      ("sllDiscr", "<f8"), ("sllDiscrFilt", "<f8"), ("pllDiscr", "<f8"),
                      ("pllDiscrFilt", "<f8"), ("blksize", "<i4"), ("status", "<i4"),
                      ("segment", "<i4"), ("pad", "<i4")])
assert E1T_CHAN.itemsize == 160 and E1T_EPOCH.itemsize == 176
L3T_SUMS = ("I_E", "I_P", "I_L", "Q_E", "Q_P", "Q_L",          # pilot channel
            "I_E2", "I_P2", "I_L2", "Q_E2", "Q_P2", "Q_L2")    # data channel
L3T_CHAN = np.dtype([("code_id", "<i4"), ("stream", "<i4"), ("status", "<i4"),
                     ("n_epochs", "<i4"), ("pos", "<i8"), ("pad", "<i8"),
                     ("rem_code", "<f8"), ("rem_carr", "<f8"), ("code_freq", "<f8"),
                     ("carr_freq", "<f8"), ("carr_freq_basis", "<f8"), ("old_code_nco", "<f8"),
                     ("old_code_error", "<f8"), ("old_carr_nco", "<f8"),
                     ("old_carr_error", "<f8"), ("i1", "<f8"), ("q1", "<f8"), ("pad2", "<f8")])
L3T_EPOCH = np.dtype([(f, "<f8") for f in L3T_SUMS] +
                     [("carrFreq", "<f8"), ("codeFreq", "<f8"), ("absoluteSample", "<f8"),
                      ("dllDiscr", "<f8"), ("dllDiscrFilt", "<f8"), ("pllDiscr", "<f8"),
                      ("pllDiscrFilt", "<f8"), ("blksize", "<i4"), ("status", "<i4")])
assert L3T_CHAN.itemsize == 128 and L3T_EPOCH.itemsize == 160
GPS_EPH_FIELDS = ("T_GD", "t_oc", "a_f2", "a_f1", "a_f0", "C_rs", "deltan", "M_0", "C_uc", "e",
                  "C_us", "sqrtA", "t_oe", "C_ic", "omega_0", "C_is", "i_0", "C_rc", "omega",
                  "omegaDot", "iDot")   # ephemeris.sci:92-205, the file's order
GPS_EPH_INTS = ("weekNumber", "accuracy", "health", "IODC", "IODE_sf2", "IODE_sf3", "TOW",
                "have", "status", "reserved")
GPS_EPH_OK, GPS_EPH_SHORT, GPS_EPH_UNDECIDED = 0, 1, 2
GPS_FIX_OK, GPS_FIX_FEW, GPS_FIX_RANK = 0, 1, 2


class GpsEph(C.Structure):
    """gnsscorr_gps_eph"""
    _fields_ = [(f, C.c_double) for f in GPS_EPH_FIELDS] + [(f, C.c_int32) for f in GPS_EPH_INTS]


class GpsFixCfg(C.Structure):
    """gnsscorr_gps_fix_cfg"""
    _fields_ = [("samplesPerCode", C.c_double), ("startOffset", C.c_double), ("c", C.c_double),
                ("elevationMask", C.c_double), ("navSolPeriod", C.c_int32),
                ("useTropCorr", C.c_int32), ("max_meas", C.c_int32), ("reserved", C.c_int32)]


GPS_EPH = np.dtype(GpsEph)
GPS_FIX_SOL = np.dtype([("X", "<f8"), ("Y", "<f8"), ("Z", "<f8"), ("dt", "<f8"),
                        ("DOP", "<f8", (5,)), ("lat", "<f8"), ("lon", "<f8"), ("height", "<f8"),
                        ("status", "<i4"), ("n_used", "<i4")])
GPS_FIX_CHAN = np.dtype([("el", "<f8"), ("az", "<f8"), ("rawP", "<f8"), ("corrP", "<f8"),
                         ("used", "<i4"), ("reserved", "<i4")])
assert GPS_EPH.itemsize == 208 and GPS_FIX_SOL.itemsize == 104 and GPS_FIX_CHAN.itemsize == 40
GLO_EPH_FIELDS = ("x", "y", "z", "xdot", "ydot", "zdot", "xdotdot", "ydotdot", "zdotdot",
                  "gamman", "taun", "deltataun", "tauc", "tauGPS", "t")   # km, km/s, km/s^2; s
GLO_EPH_INTS = ("P1", "tk_h", "tk_m", "tk_s", "Bn", "P2", "tb", "P3", "P", "In3", "En", "P4",
                "Ft", "Nt", "n", "M", "NA", "N4", "In5", "string_1_pos", "have", "skipped",
                "status", "reserved")
GLO_EPH_OK, GLO_EPH_SHORT = 0, 1


class GloEph(C.Structure):
    """gnsscorr_glo_eph"""
    _fields_ = [(f, C.c_double) for f in GLO_EPH_FIELDS] + [(f, C.c_int32) for f in GLO_EPH_INTS]


class GloSat(C.Structure):
    """gnsscorr_glo_sat"""
    _fields_ = [("pos", C.c_double * 3), ("vel", C.c_double * 3), ("acc", C.c_double * 3),
                ("clk", C.c_double), ("deltat", C.c_double), ("n10", C.c_int32),
                ("n1", C.c_int32), ("n001", C.c_int32), ("ready", C.c_int32)]


class GloFixCfg(C.Structure):
    """gnsscorr_glo_fix_cfg"""
    _fields_ = [("samplesPerCode", C.c_double), ("dataTypeSizeInBytes", C.c_double),
                ("c", C.c_double), ("elevationMask", C.c_double), ("navSolPeriod", C.c_int32),
                ("useTropCorr", C.c_int32), ("max_meas", C.c_int32), ("reserved", C.c_int32)]


GLO_EPH = np.dtype(GloEph)
GLO_SAT = np.dtype(GloSat)
GLO_FIX_CFG = np.dtype(GloFixCfg)
assert GLO_EPH.itemsize == 216 and GLO_SAT.itemsize == 104 and GLO_FIX_CFG.itemsize == 48
B1_EPH_FIELDS = ("T_GD_1", "t_oc", "a2", "a0", "a1", "alpha0", "alpha1", "alpha2", "alpha3",
                 "beta0", "beta1", "beta2", "beta3", "deltan", "C_uc", "M_0", "e", "C_us", "C_rc",
                 "C_rs", "sqrtA", "t_oe_msb", "t_oe_lsb", "i_0", "C_ic", "omegaDot", "C_is",
                 "iDot", "omega_0", "omega", "t_oe")   # ephemeris.sci:45-118
B1_EPH_INTS = ("SatH1", "IODC", "URAI", "WN", "IODE", "SOW", "have", "status")
B1_EPH_OK, B1_EPH_SHORT, B1_EPH_NO_SOW = 0, 1, 2


class B1Eph(C.Structure):
    """gnsscorr_b1_eph"""
    _fields_ = [(f, C.c_double) for f in B1_EPH_FIELDS] + [(f, C.c_int32) for f in B1_EPH_INTS]


class B1FixCfg(C.Structure):
    """gnsscorr_b1_fix_cfg"""
    _fields_ = [("samplesPerCode", C.c_double), ("dataTypeSizeInBytes", C.c_double),
                ("c", C.c_double), ("navSolPeriod", C.c_int32), ("useTropCorr", C.c_int32),
                ("max_meas", C.c_int32), ("reserved", C.c_int32)]


B1_EPH = np.dtype(B1Eph)
B1_FIX_CFG = np.dtype(B1FixCfg)
assert B1_EPH.itemsize == 280 and B1_FIX_CFG.itemsize == 40
SDR_CHAN = np.dtype([("code_phase", "<f8"), ("carrier_phase", "<f8"),
                     ("carrier_phase_prev", "<f8"), ("code_phase_mod", "<f8"),
                     ("carrier_phase_mod", "<f8"), ("code_nco", "<f8"), ("carrier_nco", "<f8"),
                     ("chan", "<u4"), ("sv", "<u4"), ("navigate", "<u4"), ("active", "<u4"),
                     ("count", "<u4"), ("scount", "<u4"), ("epoch_1ms", "<u4"),
                     ("epoch_20ms", "<u4"), ("z_count", "<u4"), ("rollover", "<u4"),
                     ("cbin", "<u4", (3,)), ("sbin", "<u4"), ("coff", "<i4", (3,)),
                     ("soff", "<i4")])
SDR_CORR = np.dtype([("i", "<i4", (3,)), ("q", "<i4", (3,))])
SDR_JOB = np.dtype([("packet", "<i4"), ("data_off", "<i4"), ("samps", "<i4"), ("sv", "<i4"),
                    ("sbin", "<i4"), ("soff", "<i4"), ("cbin", "<i4", (3,)),
                    ("coff", "<i4", (3,))])
assert SDR_CHAN.itemsize == 128 and SDR_CORR.itemsize == 24 and SDR_JOB.itemsize == 48
# gnsscorr_sdr_channel: the Channel object's state (objects/channel.h:53-132)
_CH_CORE = [("carrier_nco", "<f8"), ("code_nco", "<f8"), ("len", "<i4"), ("count", "<i4"),
            ("state", "<i4"), ("sv", "<i4"), ("chan", "<i4"), ("I", "<i4", (3,)),
            ("Q", "<i4", (3,)), ("P", "<i4", (3,)), ("I_prev", "<i4"), ("Q_prev", "<i4"),
            ("I_avg", "<f4"), ("Q_var", "<f4"), ("P_avg", "<f4"), ("cn0", "<f4"),
            ("bit_lock", "<i4"), ("bit_lock_pend", "<i4"), ("bit_lock_ticks", "<i4"),
            ("I_sum20", "<i4"), ("Q_sum20", "<i4"), ("I_buff", "<i4", (20,)),
            ("Q_buff", "<i4", (20,)), ("P_buff", "<i4", (20,)), ("epoch_20ms", "<i4"),
            ("epoch_1ms", "<i4"), ("best_epoch", "<i4"), ("valid_frame", "<i4", (5,)),
            ("navigate", "<i4"), ("z_lock", "<i4"), ("converged", "<i4"), ("frame_z", "<i4"),
            ("z_count", "<i4"), ("z_count_pend", "<i4"), ("word_buff", "<u4", (12,)),
            ("frame_lock", "<i4"), ("frame_lock_pend", "<i4"), ("bit_number", "<i4"),
            ("subframe", "<i4"), ("freq_lock", "<i4"), ("freq_lock_ticks", "<i4"),
            ("pll", "<f4", (17,)), ("dll", "<f4", (7,))]
# the C structs' trailing alignment padding as named fields: numpy copies
# (copy(), element assignment) skip unnamed padding bytes, which then hold
# whatever np.empty left there and make byte comparisons of copies flaky
SDR_CHANNEL_CORE = np.dtype(_CH_CORE + [("_pad", "<u4")], align=True)
SDR_CHANNEL = np.dtype(_CH_CORE + [("fft_buff", "<u4", (512,)), ("_pad", "<u4")], align=True)
SDR_SUBFRAME = np.dtype([("sv", "<i4"), ("subframe", "<i4"), ("word_buff", "<u4", (12,)),
                         ("chan", "<i4"), ("ms", "<i4")])
SDR_FEEDBACK = np.dtype([("carrier_nco", "<f8"), ("code_nco", "<f8"), ("kill", "<u4"),
                         ("reset_1ms", "<u4"), ("reset_20ms", "<u4"), ("set_z_count", "<u4"),
                         ("z_count", "<u4"), ("length", "<u4"), ("navigate", "<u4"),
                         ("pad", "<u4")])
SDR_DUMP_REC = np.dtype([("packet", "<i4"), ("phase", "<i4"), ("corr", SDR_CORR),
                         ("fb", SDR_FEEDBACK)])
assert SDR_DUMP_REC.itemsize == 80
assert SDR_CHANNEL_CORE.itemsize == 584 and SDR_CHANNEL.itemsize == 2632
assert SDR_SUBFRAME.itemsize == 64 and SDR_FEEDBACK.itemsize == 48
SDR_ACQ_STRONG, SDR_ACQ_MEDIUM, SDR_ACQ_WEAK = 0, 1, 2   # ACQ_TYPE_* (acquisition.cpp:584-599)
SDR_ACQ_MS = {0: 1, 1: 10, 2: 310}                       # ms per request (acquisition.cpp:628-641)
SDR_RESULT = np.dtype([("sv", "<i4"), ("code_phase", "<i4"), ("doppler", "<i4"),
                       ("magnitude", "<u4"), ("success", "<i4"), ("row", "<i4")])

IF_IQ = 1        # GNSSCORR_IF_IQ: interleaved I,Q
IF_PACKED2 = 2   # GNSSCORR_IF_PACKED2: 2-bit codes, 4 elements per byte (GN3S LUT {-3,-1,1,3})
IF_INT16 = 4     # GNSSCORR_IF_INT16: little-endian int16 elements (fp64 acquisition)
ACQ_BEST_OF_BLOCKS = 0
ACQ_NONCOHERENT = 1
ACQ_CONCAT = 2   # GNSSCORR_ACQ_CONCAT: the blocks' kept lags end to end (set_block_stride)
ACQ_F64 = 0      # reference precision (acquisition.sci evaluates in doubles)
ACQ_F32 = 1      # single-precision fast path (n_samples 16368 only)
CODE_GLO_ST = 0  # GNSSCORR_CODE_GLO_ST: the GLONASS ST code id of set_prn_codes


class TrackCfg(C.Structure):
    _fields_ = [("n_channels", C.c_int), ("iq", C.c_int), ("device", C.c_int),
                ("max_nsamp", C.c_int), ("samp_rate", C.c_double), ("tic_period", C.c_double)]


class AcqCfg(C.Structure):
    _fields_ = [("samp_rate", C.c_double), ("n_samples", C.c_int), ("device", C.c_int),
                ("max_freqs", C.c_int), ("max_blocks", C.c_int), ("max_codes", C.c_int),
                ("precision", C.c_int)]


class SgtCfg(C.Structure):
    _fields_ = [("system", C.c_int32), ("file_type", C.c_int32), ("switch_iq", C.c_int32),
                ("code_length", C.c_int32), ("device", C.c_int32), ("max_channels", C.c_int32),
                ("samp_rate", C.c_double), ("code_freq_basis", C.c_double),
                ("if_freq", C.c_double), ("l1_if_step", C.c_double),
                ("glonass_zero_channel", C.c_double), ("dll_spacing", C.c_double),
                ("dll_noise_bw", C.c_double), ("dll_damping", C.c_double),
                ("pll_noise_bw", C.c_double), ("fll_noise_bw", C.c_double),
                ("code_nco_variant", C.c_int32), ("abs_sample_variant", C.c_int32)]


class E1tCfg(C.Structure):
    _fields_ = [("file_type", C.c_int32), ("device", C.c_int32), ("max_channels", C.c_int32),
                ("max_codes", C.c_int32), ("code_length", C.c_int32),
                ("meandr_length", C.c_int32), ("samp_rate", C.c_double),
                ("code_freq_basis", C.c_double), ("meandr_freq_basis", C.c_double),
                ("if_freq", C.c_double), ("dll_spacing", C.c_double),
                ("dll_noise_bw", C.c_double), ("dll_damping", C.c_double),
                ("sll_spacing", C.c_double), ("sll_noise_bw", C.c_double),
                ("sll_damping", C.c_double), ("pll_noise_bw", C.c_double),
                ("fll_noise_bw", C.c_double), ("epoch_ms", C.c_int32),
                ("ambiguous", C.c_int32)]


class L3tCfg(C.Structure):
    _fields_ = [("file_type", C.c_int32), ("switch_iq", C.c_int32), ("code_length", C.c_int32),
                ("device", C.c_int32), ("max_channels", C.c_int32), ("pad", C.c_int32),
                ("samp_rate", C.c_double), ("code_freq_basis", C.c_double),
                ("if_freq", C.c_double), ("nominal_freq", C.c_double),
                ("dll_spacing", C.c_double), ("dll_noise_bw", C.c_double),
                ("dll_damping", C.c_double), ("pll_noise_bw", C.c_double),
                ("fll_noise_bw", C.c_double)]


class SdrCorrCfg(C.Structure):
    _fields_ = [("device", C.c_int32), ("saturate", C.c_int32)]


class SdrAcqCfg(C.Structure):
    _fields_ = [("fif", C.c_double), ("device", C.c_int32), ("saturate", C.c_int32)]


_P, _I, _I64, _D, _U64 = C.c_void_p, C.c_int, C.c_int64, C.c_double, C.c_uint64


def _ctx_sig(prefix, *create_args):
    """The rows every context family has: create, destroy, sync, stream."""
    return {prefix + "_create": (_I, [C.POINTER(_P), *create_args]),
            prefix + "_destroy": (_I, [_P]), prefix + "_sync": (_I, [_P]),
            prefix + "_stream": (_P, [_P])}


def _tracker_sig(prefix, Cfg, n_coefs):
    """The rows of a float tracker family (csrc/ftrack.h), alike up to prefix and cfg."""
    cfg = C.POINTER(Cfg)
    run = (_I, [_P, _P, _I64, _I64, _I, _P, _I, _I, _P])
    rep = (_I, [_P, _I, _P, _I, _P, _P])
    return {prefix + "_loop_coefs": (None, [cfg] + [C.POINTER(_D)] * n_coefs),
            prefix + "_init_chan": (_I, [cfg, _I, _I, _I64, _I64, _D, _P]),
            **_ctx_sig(prefix, cfg),
            prefix + "_track_dev": run, prefix + "_track": run,
            prefix + "_set_packed": (_I, [_P, _I]),
            prefix + "_set_record_format": (_I, [_P, _I]),
            prefix + "_replay": rep, prefix + "_replay_dev": rep}


def _sig_table():
    P, I, I64, D, U64 = _P, _I, _I64, _D, _U64
    return {
        "gnsscorr_last_error": (C.c_char_p, []),
        "gnsscorr_version": (C.c_char_p, []),
        "gnsscorr_device_count": (I, []),
        "gnsscorr_device_pci_bus_id": (I, [I, P, I]),
        "gnsscorr_device_lds_bytes": (I, [I]),
        "gnsscorr_hip_runtime": (I, [P, I, P]),
        **_ctx_sig("gnsscorr_track", C.POINTER(TrackCfg)),
        "gnsscorr_track_set_layout": (I, [P, I]),
        "gnsscorr_track_max_dumps": (I, [P]),
        "gnsscorr_track": (I, [P, P, I64, I, I64, P, P, P, C.POINTER(I)]),
        "gnsscorr_track_dev": (I, [P, P, I64, I64, P, P, P, I64]),
        "gnsscorr_track_next_tic": (I64, [P, I64]),
        "gnsscorr_track_if_bytes": (I64, [P, I64]),
        "gnsscorr_pack2": (I, [P, I64, P]),
        "gnsscorr_unpack2": (I, [P, I64, P]),
        "gnsscorr_track_replay_dev": (I, [P, P, I64, I64, I, P, P]),
        "gnsscorr_track_get_state": (I, [P, P]),
        "gnsscorr_track_set_state": (I, [P, P]),
        **_ctx_sig("gnsscorr_acq", C.POINTER(AcqCfg)),
        "gnsscorr_acq_set_codes": (I, [P, I, P]),
        "gnsscorr_acq_search": (I, [P, P, I, I, I, I, P, I, I, P, P, I, P, P]),
        "gnsscorr_acq_search_dev": (I, [P, P, I, I, I, I, P, I, I, P, P, I, P, P]),
        "gnsscorr_acq_power_row": (I, [P, P, I, I, I, D, I, P]),
        "gnsscorr_acq_spectra_dev": (I, [P, P, I, I, I, P]),
        "gnsscorr_acq_correlate_dev": (I, [P, I, I, P, I, I, P, P, I, P, P]),
        "gnsscorr_acq_select_dev": (I, [P, I, I, P, P, P, P]),
        "gnsscorr_acq_set_coherent": (I, [P, I]),
        "gnsscorr_acq_set_records": (I, [P, I]),
        "gnsscorr_acq_set_group_records": (I, [P, P]),
        "gnsscorr_acq_set_prn_codes": (I, [P, I, P]),
        "gnsscorr_acq_set_zero_padded": (I, [P, I]),
        "gnsscorr_acq_set_codes_padded": (I, [P, I, P, I]),
        "gnsscorr_acq_set_peak_period": (I, [P, I]),
        "gnsscorr_acq_second_peak_candidate": (I, [I, I, I, I, I]),
        "gnsscorr_acq_set_block_stride": (I, [P, I]),
        "gnsscorr_acq_mix_plan": (I, [I, P, P, I]),
        **_tracker_sig("gnsscorr_sgt", SgtCfg, 5),
        **_tracker_sig("gnsscorr_e1t", E1tCfg, 7),
        "gnsscorr_e1t_set_codes": (I, [P, I, P]),
        "gnsscorr_l3_code": (I, [I, P]),
        **_tracker_sig("gnsscorr_l3t", L3tCfg, 5),
        **_ctx_sig("gnsscorr_nav", I),
        "gnsscorr_nav_conv_encode": (I, [P, I, P]),
        "gnsscorr_nav_viterbi_dev": (I, [P, P, I64, I, I, I, P]),
        "gnsscorr_nav_viterbi": (I, [P, P, I64, I, I, I, P]),
        "gnsscorr_nav_e1_pages_dev": (I, [P, P, I64, I64, I, I, I, P, P, P]),
        "gnsscorr_nav_e1_pages": (I, [P, P, I64, I64, I, I, I, P, P, P]),
        "gnsscorr_nav_l3_decode_dev": (I, [P, P, P, I64, I64, I, I, I, P, P, P, P, P]),
        "gnsscorr_nav_l3_decode": (I, [P, P, P, I64, I64, I, I, I, P, P, P, P, P]),
        "gnsscorr_nav_pattern_hits_dev": (I, [P, P, I64, I64, I, I, P, I, I, I, I, P, P, P]),
        "gnsscorr_nav_pattern_hits": (I, [P, P, I64, I64, I, I, P, I, I, I, I, P, P, P]),
        "gnsscorr_nav_gps_frames_dev": (I, [P, P, I64, I64, I, I, I, I, P, P, P]),
        "gnsscorr_nav_gps_frames": (I, [P, P, I64, I64, I, I, I, I, P, P, P]),
        "gnsscorr_nav_glo_strings_dev": (I, [P, P, I64, I64, I, I, I, P, P, P]),
        "gnsscorr_nav_glo_strings": (I, [P, P, I64, I64, I, I, I, P, P, P]),
        "gnsscorr_nav_b1_subframes_dev": (I, [P, P, I64, I64, I, I, I, P, P, P]),
        "gnsscorr_nav_b1_subframes": (I, [P, P, I64, I64, I, I, I, P, P, P]),
        "gnsscorr_nav_gps_ephemeris_dev": (I, [P, P, P, P, I, P]),
        "gnsscorr_nav_gps_ephemeris": (I, [P, P, P, P, I, P]),
        "gnsscorr_nav_gps_fix_cfg_init": (None, [P]),
        "gnsscorr_nav_gps_fix_dev": (I, [P, P, P, P, I64, I64, I, I, P, P, P, P, P]),
        "gnsscorr_nav_gps_fix": (I, [P, P, P, P, I64, I64, I, I, P, P, P, P, P]),
        "gnsscorr_nav_glo_ephemeris_dev": (I, [P, P, P, P, I, P]),
        "gnsscorr_nav_glo_ephemeris": (I, [P, P, P, P, I, P]),
        "gnsscorr_nav_glo_fix_cfg_init": (None, [P]),
        "gnsscorr_nav_glo_satpos_dev": (I, [P, P, I, P, P]),
        "gnsscorr_nav_glo_satpos": (I, [P, P, I, P, P]),
        "gnsscorr_nav_glo_fix_dev": (I, [P, P, P, P, P, I64, I64, I, I, P, P, P, P, P]),
        "gnsscorr_nav_glo_fix": (I, [P, P, P, P, P, I64, I64, I, I, P, P, P, P, P]),
        "gnsscorr_nav_b1_ephemeris_dev": (I, [P, P, P, P, I, P]),
        "gnsscorr_nav_b1_ephemeris": (I, [P, P, P, P, I, P]),
        "gnsscorr_nav_b1_fix_cfg_init": (None, [P]),
        "gnsscorr_nav_b1_fix_dev": (I, [P, P, P, P, I64, I64, I, I, P, P, P, P, P]),
        "gnsscorr_nav_b1_fix": (I, [P, P, P, P, I64, I64, I, I, P, P, P, P, P]),
        "gnsscorr_sdr_prn_codes": (I, [P]),
        "gnsscorr_sdr_sine_gen": (None, [P, D, D, I]),
        **_ctx_sig("gnsscorr_sdr_acq", C.POINTER(SdrAcqCfg)),
        "gnsscorr_sdr_acq_strong": (I, [P, P, I, I, P, I, I, P]),
        "gnsscorr_sdr_acq_strong_dev": (I, [P, P, I, I, P, I, I, P]),
        "gnsscorr_sdr_acq_prep_dev": (I, [P, I, P, I]),
        "gnsscorr_sdr_channel_start": (I, [P, I, I, I, I]),
        "gnsscorr_sdr_channel_accum_dev": (I, [P, I, I, P, P, P, P, P, I, P]),
        "gnsscorr_sdr_track_dev": (I, [P, P, I, I, I, P, P, P, P, P, P, I, P, P, P, I, P]),
        "gnsscorr_sdr_acq_search_dev": (I, [P, I, I, I, P, I, I, P]),
        "gnsscorr_sdr_acq_acquire": (I, [P, I, P, I, I, P, I, I, P]),
        "gnsscorr_sdr_acq_read_rows": (I, [P, P, C.c_size_t]),
        "gnsscorr_sdr_acq_read_spectra": (I, [P, I, I, I, I, P]),
        **_ctx_sig("gnsscorr_sdr_corr", C.POINTER(SdrCorrCfg)),
        "gnsscorr_sdr_init_chan": (I, [P, I, I, I, D]),
        "gnsscorr_sdr_accum_dev": (I, [P, P, I, P, P]),
        "gnsscorr_sdr_correlate": (I, [P, P, I, I, P, P, P, P, P]),
        "gnsscorr_sdr_corr_device": (I, [P]),
        "gnsscorr_sdr_gn3s_products": (None, [P]),
        "gnsscorr_osg_loop_cfg_init": (None, [P, D, D, D, I, I, D, C.c_long, C.c_long, C.c_long,
                                              C.c_long, C.c_long, I]),
        "gnsscorr_osg_loop_reset": (None, [P, I, P, P, P]),
        "gnsscorr_osg_isr_dev": (I, [P, P, I, P, P, P]),
        "gnsscorr_osg_closed_loop_dev": (I, [P, P, P, I64, I64, I, I, P, P, P, P]),
        **_ctx_sig("gnsscorr_sdr_fe", I),
        "gnsscorr_sdr_gn3s_dev": (I, [P, P, I, I, C.POINTER(C.c_uint32), C.c_uint32, P]),
        "gnsscorr_sdr_gn3s": (I, [P, P, I, I, C.POINTER(C.c_uint32), C.c_uint32, P]),
        "gnsscorr_sdr_downsample_count": (I, [I, D, D, P]),
        "gnsscorr_sdr_downsample_dev": (I, [P, P, I, D, D, P, C.POINTER(C.c_int)]),
        "gnsscorr_dev_alloc": (I, [I, C.c_size_t, C.POINTER(P)]),
        "gnsscorr_dev_free": (I, [I, P]),
        "gnsscorr_memcpy_htod": (I, [I, P, P, C.c_size_t]),
        "gnsscorr_memcpy_dtoh": (I, [I, P, P, C.c_size_t]),
        "gnsscorr_dev_synchronize": (I, [I]),
        "gnsscorr_event_create": (I, [I, C.POINTER(P)]),
        "gnsscorr_event_record": (I, [P, P]),
        "gnsscorr_stream_wait_event": (I, [P, P]),
        "gnsscorr_event_elapsed_ms": (I, [P, P, C.POINTER(C.c_float)]),
        "gnsscorr_event_destroy": (I, [P]),
        "gnsscorr_dev_fill_if2": (I, [I, P, C.c_size_t, U64]),
        "gnsscorr_ifgen": (I, [P, I64, I, D, D, D, I, P, U64]),
        "gnsscorr_ca_code": (I, [I, P]),
        "gnsscorr_b1i_code": (I, [I, P]),
        "gnsscorr_st_code": (I, [P]),
        "gnsscorr_sample_code": (I, [P, I, D, D, I, P]),
        "gnsscorr_sample_boc_code": (I, [P, I, D, D, I, P]),
        "correlator_init": (None, [D]),
        "Sim_GP2021_int": (None, [P, C.c_long]),
        "gnsscorr_osg_configure": (I, [D, D, D, D, I, I, I, I, D, I]),
        "gnsscorr_osg_get_state": (I, [P]),
    }


# name -> (restype, argtypes) of every function include/gnsscorr.h and
# include/gnsscorr_osg.h declare; lib() sets them on the loaded library
_SIG = _sig_table()
EXPORTED_FUNCTIONS = list(_SIG)
EXPORTED_DATA = ["REG_read", "REG_write", "Carrier_DCO_Delta", "Code_DCO_Delta",
                 "gps_code_ref", "gps_carrier_ref", "glonass_code_ref",
                 "glonass_carrier_ref", "d_freq"]

_lib = None


class GnssCorrError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Load libgnsscorr.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GnssCorrError(f"{LIB_PATH} not built (run `make -C gnss-sdr.ru_amd`)")
    L = C.CDLL(LIB_PATH)  # RTLD_LOCAL: never interpose REG_read etc. into other libraries
    for name, (res, args) in _SIG.items():
        if not hasattr(L, name):
            continue  # reported by tests/test_abi.py
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def _check(rc: int, what) -> None:
    """what: the symbol's name, or its ctypes function (named only when the call failed)."""
    if rc != 0:
        msg = lib().gnsscorr_last_error().decode(errors="replace")
        raise GnssCorrError(f"{getattr(what, '__name__', what)} failed ({rc}): {msg}")


class _Handle:
    """What the context classes share: a handle `h` made by <prefix>_create and freed by
    <prefix>_destroy, sync() and the stream property.  The family's ctypes functions are
    looked up once, at creation: sync and stream sit inside timed loops."""

    _prefix = None   # "gnsscorr_track", ...

    def _create(self, *args, ops=()):
        """<prefix>_create(&h, *args); binds <prefix>_<op> as self._<op> for `ops` too."""
        L = lib()
        for op in ("destroy", "sync", "stream") + ops:
            setattr(self, "_" + op, getattr(L, f"{self._prefix}_{op}"))
        h = C.c_void_p()
        _check(getattr(L, self._prefix + "_create")(C.byref(h), *args),
               self._prefix + "_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):   # also after a constructor that failed before h existed
            self._destroy(self.h)
            self.h = None

    __del__ = close

    def sync(self):
        _check(self._sync(self.h), self._sync)

    @property
    def stream(self) -> int:
        return self._stream(self.h)


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def _if_bytes(a, iq=0) -> np.ndarray:
    """IF samples as the C ABI's int8 byte buffer (packed data may come as uint8).  With
    GNSSCORR_IF_INT16 in iq the record is an int16 array, handed over as its little-endian
    bytes, or those bytes as uint8; an array of another type holds no 16-bit elements (an
    int8 array is int8 samples, whatever its size) and is refused."""
    a = np.ascontiguousarray(a)
    if int(iq) & IF_INT16:
        if a.dtype.kind == "i" and a.dtype.itemsize == 2:
            return a.astype("<i2", copy=False).reshape(-1).view(np.int8)
        if a.dtype != np.uint8:
            raise GnssCorrError(f"GNSSCORR_IF_INT16 needs an int16 array (or its bytes as "
                                f"uint8), got {a.dtype}")
    return a.view(np.int8) if a.dtype == np.uint8 else np.ascontiguousarray(a, np.int8)


def iq_flags(iq, packed=False, int16=False) -> int:
    """The `iq` argument of the C ABI: GNSSCORR_IF_* flags (iq may already be flags)."""
    f = int(iq)
    f = f | IF_PACKED2 if packed else f
    return f | IF_INT16 if int16 else f


def pack2(levels) -> np.ndarray:
    """int8 levels in {-3,-1,1,3} -> GNSSCORR_IF_PACKED2 bytes (gnsscorr_pack2)."""
    lv = np.ascontiguousarray(levels, np.int8).ravel()
    out = np.empty((lv.size + 3) // 4, np.uint8)
    _check(lib().gnsscorr_pack2(_ptr(lv), lv.size, _ptr(out)), "gnsscorr_pack2")
    return out


def unpack2(packed, n) -> np.ndarray:
    """The first n int8 levels of GNSSCORR_IF_PACKED2 bytes (gnsscorr_unpack2)."""
    b = np.ascontiguousarray(packed).view(np.uint8).ravel()
    n = int(n)
    if n > 4 * b.size:
        raise ValueError(f"{b.size} packed bytes hold fewer than {n} elements")
    out = np.empty(max(n, 0), np.int8)
    _check(lib().gnsscorr_unpack2(_ptr(b), n, _ptr(out)), "gnsscorr_unpack2")
    return out


def device_count() -> int:
    return int(lib().gnsscorr_device_count())


def device_lds_bytes(device: int = 0) -> int:
    """LDS bytes a workgroup may allocate on the device (gnsscorr_device_lds_bytes)."""
    return int(lib().gnsscorr_device_lds_bytes(device))


def pci_bus_id(device: int = 0) -> str:
    buf = C.create_string_buffer(64)
    _check(lib().gnsscorr_device_pci_bus_id(device, buf, 64), "gnsscorr_device_pci_bus_id")
    return buf.value.decode()


def hip_runtime() -> dict:
    """The libamdhip64 libgnsscorr's HIP calls bind to (gnsscorr_hip_runtime), its
    hipRuntimeGetVersion, and every libamdhip64 the process has mapped."""
    buf = C.create_string_buffer(4096)
    ver = C.c_int(0)
    _check(lib().gnsscorr_hip_runtime(buf, 4096, C.byref(ver)), "gnsscorr_hip_runtime")
    mapped = []
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line and line.split()[-1] not in mapped:
                    mapped.append(line.split()[-1])
    except OSError:
        pass
    return dict(bound=os.path.realpath(buf.value.decode()), version=ver.value, mapped=mapped)


# ---------------------------------------------------------------- device memory
class DevBuf:
    """A HIP device allocation owned by libgnsscorr (no other GPU runtime)."""

    def __init__(self, nbytes: int, device: int = 0):
        self.device = device
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        _check(lib().gnsscorr_dev_alloc(device, self.nbytes, C.byref(p)), "gnsscorr_dev_alloc")
        self.ptr = p.value

    @classmethod
    def from_array(cls, a: np.ndarray, device: int = 0) -> "DevBuf":
        a = np.ascontiguousarray(a)
        b = cls(max(a.nbytes, 1), device)
        b.upload(a)
        return b

    def upload(self, a: np.ndarray, offset: int = 0):
        a = np.ascontiguousarray(a)
        assert offset + a.nbytes <= self.nbytes
        _check(lib().gnsscorr_memcpy_htod(self.device, self.ptr + offset, _ptr(a), a.nbytes),
               "gnsscorr_memcpy_htod")

    def download(self, dtype, count: int = -1, offset: int = 0) -> np.ndarray:
        dt = np.dtype(dtype)
        if count < 0:
            count = (self.nbytes - offset) // dt.itemsize
        out = np.empty(count, dt)
        _check(lib().gnsscorr_memcpy_dtoh(self.device, _ptr(out), self.ptr + offset, out.nbytes),
               "gnsscorr_memcpy_dtoh")
        return out

    def fill_if2(self, seed: int):
        _check(lib().gnsscorr_dev_fill_if2(self.device, self.ptr, self.nbytes, seed),
               "gnsscorr_dev_fill_if2")

    def free(self):
        if getattr(self, "ptr", None):
            lib().gnsscorr_dev_free(self.device, self.ptr)
            self.ptr = None

    __del__ = free


def dev_synchronize(device: int = 0):
    _check(lib().gnsscorr_dev_synchronize(device), "gnsscorr_dev_synchronize")


class Event:
    """hipEvent_t wrapper for timing on a specific HIP stream."""

    def __init__(self, device: int = 0):
        p = C.c_void_p()
        _check(lib().gnsscorr_event_create(device, C.byref(p)), "gnsscorr_event_create")
        self.h = p

    def record(self, stream: int):
        _check(lib().gnsscorr_event_record(self.h, stream), "gnsscorr_event_record")

    def wait_on(self, stream: int):
        """Work queued on `stream` from now on waits for this event."""
        _check(lib().gnsscorr_stream_wait_event(stream, self.h), "gnsscorr_stream_wait_event")

    def elapsed_ms(self, end: "Event") -> float:
        ms = C.c_float()
        _check(lib().gnsscorr_event_elapsed_ms(self.h, end.h, C.byref(ms)),
               "gnsscorr_event_elapsed_ms")
        return float(ms.value)

    def __del__(self):
        if getattr(self, "h", None):
            lib().gnsscorr_event_destroy(self.h)
            self.h = None


# ---------------------------------------------------------------- host utils
def ca_code(prn: int) -> np.ndarray:
    out = np.empty(1023, np.int8)
    _check(lib().gnsscorr_ca_code(prn, _ptr(out)), "gnsscorr_ca_code")
    return out


def b1i_code(prn: int) -> np.ndarray:
    """BeiDou B1I ranging code of prn 1..37 as +-1 chips
    (COMPASS/B1/include/generateCAcode.sci:38-146)."""
    out = np.empty(2046, np.int8)
    _check(lib().gnsscorr_b1i_code(prn, _ptr(out)), "gnsscorr_b1i_code")
    return out


def l3_code(code_id: int) -> np.ndarray:
    """GLONASS L3OC code of table row 1..64 as 10230 chips (GLONASS/L3/include/
    generateCAcode.sci:40-139, its table as it stands: id 31 has 32's G2 state, id 32 is
    all zero, id 64 equals 63).  Ids 1..31: pilot codes; 33..63: data codes of PRN id - 32."""
    out = np.empty(10230, np.int8)
    _check(lib().gnsscorr_l3_code(code_id, _ptr(out)), "gnsscorr_l3_code")
    return out


def st_code() -> np.ndarray:
    out = np.empty(511, np.int8)
    _check(lib().gnsscorr_st_code(_ptr(out)), "gnsscorr_st_code")
    return out


def sample_code(chips: np.ndarray, code_rate: float, fs: float, n: int) -> np.ndarray:
    chips = np.ascontiguousarray(chips, np.int8)
    out = np.empty(n, np.int8)
    _check(lib().gnsscorr_sample_code(_ptr(chips), len(chips), code_rate, fs, n, _ptr(out)),
           "gnsscorr_sample_code")
    return out


def sample_boc_code(chips: np.ndarray, code_rate: float, fs: float, n: int) -> np.ndarray:
    """gnsscorr_sample_boc_code: +-1 chips sampled as BOC(1,1) by the
    makeE1BCodesTable.sci:56-78 rule (the last sample takes half-chip index code_len)."""
    chips = np.ascontiguousarray(chips, np.int8)
    out = np.empty(n, np.int8)
    _check(lib().gnsscorr_sample_boc_code(_ptr(chips), len(chips), code_rate, fs, n, _ptr(out)),
           "gnsscorr_sample_boc_code")
    return out


def e1b_bins(if_freq: float, band_khz: float, ms_code_len: int) -> np.ndarray:
    """The frequency grid of GALILEO/E1/acquisition.sci:61, 94-96: round(band * 2 * ms) + 1
    bins from IF - band/2 kHz in steps of 1000 / (2 * ms) Hz."""
    nb = int(round(band_khz * 2 * ms_code_len)) + 1
    k = np.arange(1, nb + 1)
    return if_freq - (band_khz / 2) * 1000 + (1000 / (2 * ms_code_len)) * (k - 1)


def l3_bins(if_freq: float, band_khz: float) -> np.ndarray:
    """The frequency grid of GLONASS/L3/acquisition.sci:66, 103-105: round(band * 2 * 5) + 1
    bins from IF - band/2 kHz in steps of 1000 / (2 * 5) Hz."""
    nb = int(round(band_khz * 2 * 5)) + 1
    k = np.arange(1, nb + 1)
    return if_freq - (band_khz / 2) * 1000 + (1000 / (2 * 5)) * (k - 1)


def acq_mix_plan(n_samples: int):
    """gnsscorr_acq_mix_plan: the radices of the generic fp64 engine's mixed-radix passes
    at n_samples, as (unpadded order, zero-padded order); two empty lists where the
    chirp-z engine serves the length (a prime factor above 31) or it is out of range."""
    r, rp = np.zeros(24, np.int32), np.zeros(24, np.int32)
    n = lib().gnsscorr_acq_mix_plan(int(n_samples), _ptr(r), _ptr(rp), 24)
    return [int(x) for x in r[:n]], [int(x) for x in rp[:n]]


def b1_coh_bins(if_freq: float, band_khz: float, coh: int) -> np.ndarray:
    """The frequency grid of COMPASS/B1/acquisition_7x3ms.sci:67, 103-105 (coh = 3) and
    acquisition_4x5ms.sci (coh = 5): round(band * 2 * coh) + 1 bins from IF - band/2 kHz in
    steps of 1000 / (2 * coh) Hz."""
    nb = int(round(band_khz * 2 * coh)) + 1
    k = np.arange(1, nb + 1)
    return if_freq - (band_khz / 2) * 1000 + (1000 / (2 * coh)) * (k - 1)


def make_sigs(sigs) -> np.ndarray:
    """sigs: list of dicts with keys of SIG (missing keys default to 0)."""
    a = np.zeros(len(sigs), SIG)
    for i, s in enumerate(sigs):
        for k, v in s.items():
            a[i][k] = v
    return a


def ifgen(nsamp: int, sigs=(), fs=16.368e6, if_gps=2.42e6, if_glo=1.0e6, iq=True,
          seed=0x5EED0000) -> np.ndarray:
    """Deterministic synthetic 2-bit IF as int8 (interleaved I,Q when iq)."""
    sa = make_sigs(sigs) if not isinstance(sigs, np.ndarray) else sigs
    out = np.empty(nsamp * (2 if iq else 1), np.int8)
    _check(lib().gnsscorr_ifgen(_ptr(out), nsamp, int(iq), fs, if_gps, if_glo, len(sa),
                                _ptr(sa) if len(sa) else None, seed), "gnsscorr_ifgen")
    return out


# ---------------------------------------------------------------- tracking
class TrackCtx(_Handle):
    """Batched GP2021-semantics tracking correlator context (one per GPU)."""

    _prefix = "gnsscorr_track"

    def __init__(self, n_channels: int, iq: bool = True, device: int = 0,
                 max_nsamp: int = 65536, samp_rate: float = 16.368e6,
                 tic_period: float = 0.0, packed: bool = False):
        self.n_channels = n_channels
        self.iq = bool(int(iq) & IF_IQ)
        self.packed = bool(packed or int(iq) & IF_PACKED2)
        cfg = TrackCfg(n_channels, iq_flags(self.iq, self.packed), device, max_nsamp, samp_rate,
                       tic_period)
        self._create(C.byref(cfg))
        self.max_dumps = lib().gnsscorr_track_max_dumps(self.h)

    def set_layout(self, one_stream_per_channel: bool):
        """gnsscorr_track_set_layout: per-channel LDS staging of int8 C_s = 1 streams."""
        _check(lib().gnsscorr_track_set_layout(self.h, int(bool(one_stream_per_channel))),
               "gnsscorr_track_set_layout")

    def track(self, if_samples: np.ndarray, nsamp: int, cmds: np.ndarray, n_streams: int = 1,
              stream_stride: int = 0, all_dumps: bool = False):
        if_samples = _if_bytes(if_samples)
        cmds = np.ascontiguousarray(cmds, NCO_CMD)
        assert len(cmds) == self.n_channels
        res = np.zeros(self.n_channels, TRACK_RESULT)
        dumps = np.zeros((self.n_channels, self.max_dumps, 6), np.int32) if all_dumps else None
        tic = C.c_int(0)
        _check(lib().gnsscorr_track(self.h, _ptr(if_samples), stream_stride, n_streams, nsamp,
                                    _ptr(cmds), _ptr(res),
                                    _ptr(dumps) if dumps is not None else None, C.byref(tic)),
               "gnsscorr_track")
        return (res, bool(tic.value), dumps) if all_dumps else (res, bool(tic.value))

    def track_dev(self, d_if: int, stream_stride: int, nsamp: int, d_cmds: int, d_res: int,
                  d_dumps: int = 0, tic_count: int = -1):
        _check(lib().gnsscorr_track_dev(self.h, d_if, stream_stride, nsamp, d_cmds, d_res,
                                        d_dumps or None, tic_count), "gnsscorr_track_dev")

    def replay_dev(self, d_if: int, stream_stride: int, nsamp: int, n_steps: int, d_cmds: int,
                   d_res: int):
        _check(lib().gnsscorr_track_replay_dev(self.h, d_if, stream_stride, nsamp, n_steps,
                                               d_cmds, d_res), "gnsscorr_track_replay_dev")

    def if_bytes(self, samples: int) -> int:
        """Bytes of `samples` samples of one stream in this context's format."""
        return int(lib().gnsscorr_track_if_bytes(self.h, samples))

    def next_tic(self, nsamp: int) -> int:
        return int(lib().gnsscorr_track_next_tic(self.h, nsamp))

    def get_state(self) -> np.ndarray:
        st = np.zeros(self.n_channels, CHAN_STATE)
        _check(lib().gnsscorr_track_get_state(self.h, _ptr(st)), "gnsscorr_track_get_state")
        return st

    def set_state(self, st: np.ndarray):
        st = np.ascontiguousarray(st, CHAN_STATE)
        _check(lib().gnsscorr_track_set_state(self.h, _ptr(st)), "gnsscorr_track_set_state")


# ---------------------------------------------------------------- acquisition
class AcqCtx(_Handle):
    """Parallel code-phase acquisition context (SoftGNSS acquisition.sci semantics)."""

    _prefix = "gnsscorr_acq"

    def __init__(self, samp_rate: float = 16.368e6, n_samples: int = 16368, device: int = 0,
                 max_freqs: int = 1024, max_blocks: int = 16, max_codes: int = 64,
                 precision: int = ACQ_F64):
        cfg = AcqCfg(samp_rate, n_samples, device, max_freqs, max_blocks, max_codes, precision)
        self.precision = precision
        self._create(C.byref(cfg))
        self.n = n_samples
        self.fs = samp_rate
        self.records = 1

    def set_codes(self, codes: np.ndarray):
        codes = np.ascontiguousarray(codes, np.int8).reshape(-1, self.n)
        _check(lib().gnsscorr_acq_set_codes(self.h, codes.shape[0], _ptr(codes)),
               "gnsscorr_acq_set_codes")

    def set_codes_padded(self, codes: np.ndarray):
        """gnsscorr_acq_set_codes_padded: (n_codes, code_len) +-1 chips with code_len <=
        n_samples, zero-extended to n_samples on the device ([code zeros],
        E1/acquisition.sci:88)."""
        codes = np.ascontiguousarray(codes, np.int8)
        codes = codes.reshape(1, -1) if codes.ndim == 1 else codes
        _check(lib().gnsscorr_acq_set_codes_padded(self.h, codes.shape[0], _ptr(codes),
                                                   codes.shape[1]),
               "gnsscorr_acq_set_codes_padded")

    def set_zero_padded(self, keep: int):
        """gnsscorr_acq_set_zero_padded: row statistics over the first `keep` lags only,
        the second-peak window circular in keep (E1/acquisition.sci:112-145); 0: off."""
        _check(lib().gnsscorr_acq_set_zero_padded(self.h, int(keep)),
               "gnsscorr_acq_set_zero_padded")
        if not int(keep):
            self.block_stride = 0   # the library clears it with the mode

    def set_block_stride(self, stride: int):
        """gnsscorr_acq_set_block_stride: block b of a zero-padded search starts at sample
        b * stride of the record (COMPASS/B1/acquisition_7x3ms.sci:52-58: overlapping
        segments), which then holds (n_blocks - 1) * stride + n_samples samples; 0: blocks
        end to end.  mode=ACQ_CONCAT needs stride == keep."""
        _check(lib().gnsscorr_acq_set_block_stride(self.h, int(stride)),
               "gnsscorr_acq_set_block_stride")
        self.block_stride = int(stride)

    def set_peak_period(self, period: int):
        """gnsscorr_acq_set_peak_period: the second-peak range of GLONASS/L3/
        acquisition.sci:134-153, written on `period` samples inside a zero-padded search's
        keep lags (2 spc < period <= keep); 0: off, the window circular in keep."""
        _check(lib().gnsscorr_acq_set_peak_period(self.h, int(period)),
               "gnsscorr_acq_set_peak_period")

    def set_prn_codes(self, code_ids):
        """gnsscorr_acq_set_prn_codes: replicas generated on the device from code ids
        (1..32: GPS C/A PRN; CODE_GLO_ST: the GLONASS ST code), then their spectra
        (acquisition.sci:91-95).  Asynchronous on the context stream."""
        ids = np.ascontiguousarray(code_ids, np.int32)
        _check(lib().gnsscorr_acq_set_prn_codes(self.h, len(ids), _ptr(ids)),
               "gnsscorr_acq_set_prn_codes")

    def search(self, if_samples, n_blocks, freqs, group_code, group_freq, spc=16, iq=True,
               mode=ACQ_BEST_OF_BLOCKS):
        if_samples = _if_bytes(if_samples, iq)
        freqs = np.ascontiguousarray(freqs, np.float64)
        group_code = np.ascontiguousarray(group_code, np.int32)
        group_freq = np.ascontiguousarray(group_freq, np.int32).reshape(len(group_code), -1)
        G, B = group_freq.shape
        stride = getattr(self, "block_stride", 0)
        if stride and n_blocks >= 1:
            # the library copies the strided record's length: refuse a shorter host array
            n_el = ((n_blocks - 1) * stride + self.n) * (2 if int(iq) & IF_IQ else 1)
            need = (n_el + 3) // 4 if int(iq) & IF_PACKED2 else n_el
            need = 2 * n_el if int(iq) & IF_INT16 else need
            if if_samples.size < need:
                raise GnssCorrError(f"gnsscorr_acq_search: {n_blocks} blocks at stride {stride} "
                                    f"need {need} bytes of IF, got {if_samples.size}")
        R = 1 if getattr(self, "_group_rec", None) is not None else self.records
        rows = np.zeros(R * G * B, ACQ_ROW)
        res = np.zeros(R * G, ACQ_RESULT)
        _check(lib().gnsscorr_acq_search(self.h, _ptr(if_samples), int(iq), n_blocks, mode,
                                         len(freqs), _ptr(freqs), G, B, _ptr(group_code),
                                         _ptr(group_freq), spc, _ptr(rows), _ptr(res)),
               "gnsscorr_acq_search")
        if R == 1:
            return res, rows.reshape(G, B)
        return res.reshape(R, G), rows.reshape(R, G, B)

    def set_records(self, n_records: int):
        """Records per search (fp64): n_records IF records end to end, searched
        in one launch; search() then returns (R, G) results and (R, G, B) rows."""
        _check(lib().gnsscorr_acq_set_records(self.h, int(n_records)), "gnsscorr_acq_set_records")
        if int(n_records) != getattr(self, "records", 1):
            self._group_rec = None   # the library drops a per-group table on a count change
        self.records = int(n_records)

    def set_group_records(self, d_group_rec):
        """Per-group IF records (gnsscorr_acq_set_group_records): a device int32 array
        (DevBuf or pointer), group g searched on record d_group_rec[g] only; None: off."""
        ptr = None if d_group_rec is None else getattr(d_group_rec, "ptr", d_group_rec)
        _check(lib().gnsscorr_acq_set_group_records(self.h, ptr),
               "gnsscorr_acq_set_group_records")
        self._group_rec = d_group_rec   # keep the device array alive

    def set_coherent(self, coh_ms: int):
        """settings.acqCohIntegration: code periods per coherent block (default 1)."""
        _check(lib().gnsscorr_acq_set_coherent(self.h, int(coh_ms)), "gnsscorr_acq_set_coherent")

    def search_dev(self, d_if, n_blocks, n_freqs, d_freqs, n_groups, n_bins, d_group_code,
                   d_group_freq, d_rows, d_res, spc=16, iq=True, mode=ACQ_BEST_OF_BLOCKS):
        _check(lib().gnsscorr_acq_search_dev(self.h, d_if, int(iq), n_blocks, mode, n_freqs,
                                             d_freqs, n_groups, n_bins, d_group_code,
                                             d_group_freq, spc, d_rows, d_res),
               "gnsscorr_acq_search_dev")

    def spectra_dev(self, d_if, n_blocks, n_freqs, d_freqs, iq=True):
        _check(lib().gnsscorr_acq_spectra_dev(self.h, d_if, int(iq), n_blocks, n_freqs, d_freqs),
               "gnsscorr_acq_spectra_dev")

    def correlate_dev(self, n_blocks, d_freqs, n_groups, n_bins, d_group_code, d_group_freq,
                      d_rows=None, d_res=None, spc=16, mode=ACQ_BEST_OF_BLOCKS):
        _check(lib().gnsscorr_acq_correlate_dev(self.h, n_blocks, mode, d_freqs, n_groups, n_bins,
                                                d_group_code, d_group_freq, spc, d_rows or None,
                                                d_res or None), "gnsscorr_acq_correlate_dev")

    def select_dev(self, n_groups, n_bins, d_freqs, d_group_freq, d_rows, d_res):
        _check(lib().gnsscorr_acq_select_dev(self.h, n_groups, n_bins, d_freqs, d_group_freq,
                                             d_rows, d_res), "gnsscorr_acq_select_dev")

    def power_row(self, if_samples, n_blocks, block, freq, code, iq=True) -> np.ndarray:
        if_samples = _if_bytes(if_samples, iq)
        out = np.empty(self.n, np.float64)
        _check(lib().gnsscorr_acq_power_row(self.h, _ptr(if_samples), int(iq), n_blocks, block,
                                            freq, code, _ptr(out)), "gnsscorr_acq_power_row")
        return out


# ---------------------------------------------------------------- float trackers
def _settings(defaults: dict, kw: dict, also=()) -> dict:
    """The defaults overridden by kw; a key that is neither a default nor in `also` is refused."""
    unknown = set(kw) - set(defaults) - set(also)
    if unknown:
        raise ValueError(f"unknown settings {sorted(unknown)}")
    defaults.update(kw)
    return defaults


def _loop_coefs(prefix, cfg, n):
    v = [C.c_double() for _ in range(n)]
    getattr(lib(), prefix + "_loop_coefs")(C.byref(cfg), *[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def _init_chan(prefix, chan_dtype, cfg, code_id, code_phase_1b, acq_freq, stream, skip):
    out = np.zeros(1, chan_dtype)
    _check(getattr(lib(), prefix + "_init_chan")(C.byref(cfg), int(code_id), int(stream),
                                                 int(skip), int(code_phase_1b), float(acq_freq),
                                                 out.ctypes.data), prefix + "_init_chan")
    return out


class _FloatTracker(_Handle):
    """What SgtCtx, E1tCtx and L3tCtx share (csrc/ftrack.h on the C side).  A subclass
    states _prefix, _make_cfg (its *_cfg builder), its CHAN and EPOCH dtypes, the number of
    sums per epoch and the number of loop coefficients."""

    _make_cfg = _CHAN = _EPOCH = _n_sums = _n_coefs = None

    def __init__(self, device: int = 0, **settings):
        self._open(self._make_cfg(device, **settings))

    def _open(self, cfg):
        self.cfg = cfg
        self._create(C.byref(cfg), ops=("track", "track_dev", "replay", "replay_dev"))

    def set_packed(self, packed=True):
        """<prefix>_set_packed: the records of later track / track_dev calls are 2-bit
        packed (pack2 of the int8 levels; 16-byte-aligned d_if, strides multiples of 16
        bytes, counts and positions still in samples) instead of int8."""
        fn = getattr(lib(), self._prefix + "_set_packed")
        _check(fn(self.h, int(packed)), fn)

    RECORD_FORMATS = {"int8": 0, "packed2": 1, "int16": 2}

    def set_format(self, fmt):
        """<prefix>_set_record_format: the records of later track / track_dev calls are
        "int8", "packed2" (what set_packed selects) or "int16" (little-endian int16
        elements, 2 * elements bytes; 16-byte-aligned d_if, strides multiples of 16 bytes,
        counts and positions still in samples)."""
        if fmt not in self.RECORD_FORMATS:
            raise ValueError(f"record format {fmt!r}: one of {sorted(self.RECORD_FORMATS)}")
        fn = getattr(lib(), self._prefix + "_set_record_format")
        _check(fn(self.h, self.RECORD_FORMATS[fmt]), fn)

    def loop_coefs(self):
        """sgt, l3t: (tau1code, tau2code, k1, k2, k3); e1t: *_loop_coefs' seven."""
        return _loop_coefs(self._prefix, self.cfg, self._n_coefs)

    def init_chans(self, code_ids, code_phases_1b, acq_freqs, streams=None, skip=0):
        n = len(code_ids)
        streams = np.zeros(n, np.int64) if streams is None else np.asarray(streams)
        out = np.zeros(n, self._CHAN)
        for i in range(n):
            out[i] = _init_chan(self._prefix, self._CHAN, self.cfg, code_ids[i],
                                code_phases_1b[i], acq_freqs[i], streams[i], skip)[0]
        return out

    def track(self, d_if, stride, n_samples, chans, n_epochs, closed_loop=True):
        """Host channel array in/out; returns epochs [n_ch, n_epochs]."""
        assert chans.dtype == self._CHAN and chans.flags.c_contiguous
        ep = np.zeros((len(chans), n_epochs), self._EPOCH)
        _check(self._track(self.h, d_if, stride, n_samples, len(chans), _ptr(chans), n_epochs,
                           int(closed_loop), _ptr(ep)), self._track)
        return ep

    def track_dev(self, d_if, stride, n_samples, n_ch, d_chan, n_epochs, d_epochs,
                  closed_loop=True):
        _check(self._track_dev(self.h, d_if, stride, n_samples, n_ch, d_chan, n_epochs,
                               int(closed_loop), d_epochs), self._track_dev)

    def replay(self, chans, sums):
        """The loop half on given sums [n_ch, n_epochs, n_sums] (sgt: I_E, I_P, I_L, Q_E,
        Q_P, Q_L; e1t: E1T_SUMS order; l3t: L3T_SUMS order); host channel array in/out;
        returns epochs [n_ch, n_epochs]."""
        assert chans.dtype == self._CHAN and chans.flags.c_contiguous
        sums = np.ascontiguousarray(sums, dtype=np.float64)
        n_ch, n_ep = sums.shape[0], sums.shape[1]
        assert sums.shape == (len(chans), n_ep, self._n_sums)
        ep = np.zeros((n_ch, n_ep), self._EPOCH)
        _check(self._replay(self.h, n_ch, _ptr(chans), n_ep, _ptr(sums), _ptr(ep)),
               self._replay)
        return ep

    def replay_dev(self, n_ch, d_chan, n_epochs, d_sums, d_epochs):
        """replay on device arrays: channels in/out at d_chan, sums [n_ch, n_epochs, n_sums]
        at d_sums, epochs [n_ch, n_epochs] to d_epochs; queued on the context's stream."""
        _check(self._replay_dev(self.h, n_ch, d_chan, n_epochs, d_sums, d_epochs),
               self._replay_dev)


# ---------------------------------------------------------------- SoftGNSS float tracking
def sgt_cfg(system: int, device: int = 0, **kw) -> SgtCfg:
    """initSettings.sci defaults (GLONASS/L1:41-107, GPS/L1:41-95, system 2:
    COMPASS/B1:64-101); keyword overrides use the Scilab names (samplingFreq, IF,
    dllCorrelatorSpacing, fileType, ...)."""
    glo = system == 1
    d = dict(samplingFreq=16e6, codeFreqBasis=0.511e6 if glo else 1.023e6,
             codeLength=511 if glo else 1023, IF=1e6 if glo else 2.42e6,
             L1_IF_step=0.5625e6 if glo else 0.0, GLONASS_zero_channel=1602e6 if glo else 0.0,
             dllCorrelatorSpacing=0.05 if glo else 0.2, dllNoiseBandwidth=0.5 if glo else 0.1,
             dllDampingRatio=0.7, pllNoiseBandwidth=25.0, fllNoiseBandwidth=250.0, fileType=2,
             switchIQ=0, codeNcoVariant=0, absSampleVariant=0)
    if system == 2:
        d.update(codeFreqBasis=2.046e6, codeLength=2046, IF=0.098e6, dllCorrelatorSpacing=0.1,
                 dllNoiseBandwidth=0.5)
    d = _settings(d, kw, also=("system",))
    return SgtCfg(system, d["fileType"], d["switchIQ"], d["codeLength"], device, 0,
                  d["samplingFreq"], d["codeFreqBasis"], d["IF"], d["L1_IF_step"],
                  d["GLONASS_zero_channel"], d["dllCorrelatorSpacing"], d["dllNoiseBandwidth"],
                  d["dllDampingRatio"], d["pllNoiseBandwidth"], d["fllNoiseBandwidth"],
                  d["codeNcoVariant"], d["absSampleVariant"])


class SgtCtx(_FloatTracker):
    """SoftGNSS float tracking (tracking.sci) for many channels over HBM-resident records."""

    _prefix, _CHAN, _EPOCH, _n_sums, _n_coefs = "gnsscorr_sgt", SGT_CHAN, SGT_EPOCH, 6, 5

    def __init__(self, system: int, device: int = 0, **settings):
        self._open(sgt_cfg(system, device, **settings))


# ---------------------------------------------------------------- Galileo E1B float tracking
def e1t_cfg(device: int = 0, **kw) -> E1tCfg:
    """GALILEO/E1/initSettings.sci:65-107 defaults; keyword overrides use the Scilab
    names (samplingFreq, IF, sllCorrelatorSpacing, fileType, ...) plus maxCodes and the
    loop of GALILEO/E1/BOC_tracking_alternatives/ to run: epochMs 1 (tracking.sci) or 4
    (tracking_4ms.sci), ambiguous 1 for the three-arm tracking_ambiguous_{1,4}ms.sci."""
    d = _settings(dict(
        fileType=2, samplingFreq=16e6, codeFreqBasis=1.023e6, meandrFreqBasis=2.046e6,
        IF=2.42e6, codeLength=4092, meandrLength=8184, dllDampingRatio=0.7,
        dllNoiseBandwidth=0.5, dllCorrelatorSpacing=0.25, sllDampingRatio=0.7,
        sllNoiseBandwidth=0.5, sllCorrelatorSpacing=0.1, pllNoiseBandwidth=25.0,
        fllNoiseBandwidth=250.0, maxCodes=50, epochMs=1, ambiguous=0), kw)
    return E1tCfg(d["fileType"], device, 0, d["maxCodes"], d["codeLength"], d["meandrLength"],
                  d["samplingFreq"], d["codeFreqBasis"], d["meandrFreqBasis"], d["IF"],
                  d["dllCorrelatorSpacing"], d["dllNoiseBandwidth"], d["dllDampingRatio"],
                  d["sllCorrelatorSpacing"], d["sllNoiseBandwidth"], d["sllDampingRatio"],
                  d["pllNoiseBandwidth"], d["fllNoiseBandwidth"], d["epochMs"], d["ambiguous"])


def e1t_loop_coefs(cfg: E1tCfg):
    """(tau1code, tau2code, tau1meandr, tau2meandr, k1, k2, k3) of a configuration (host only)."""
    return _loop_coefs("gnsscorr_e1t", cfg, 7)


def e1t_init_chan(cfg: E1tCfg, code_id, code_phase_1b, acq_freq, stream=0, skip=0) -> np.ndarray:
    """One E1T_CHAN (shape (1,)) from an acquisition result (host only)."""
    return _init_chan("gnsscorr_e1t", E1T_CHAN, cfg, code_id, code_phase_1b, acq_freq, stream,
                      skip)


class E1tCtx(_FloatTracker):
    """Galileo E1B float tracking (GALILEO/E1/tracking.sci) for many channels over
    HBM-resident records: code and subcarrier NCOs, five arms, PLL/FLL + DLL + SLL.
    epochMs=4 and / or ambiguous=1 select the loops of BOC_tracking_alternatives/ (e1t_cfg);
    in the ambiguous modes I_E .. Q_L are the I_P_E, I_P_P, I_P_L, Q_P_E, Q_P_P, Q_P_L fields."""

    _prefix, _CHAN, _EPOCH, _n_sums, _n_coefs = "gnsscorr_e1t", E1T_CHAN, E1T_EPOCH, 10, 7
    _make_cfg = staticmethod(e1t_cfg)

    def set_codes(self, chips):
        """chips: (n_codes, 4092) of +-1; channel code_id is the row."""
        chips = np.ascontiguousarray(chips, np.int8)
        assert chips.ndim == 2 and chips.shape[1] == 4092
        _check(lib().gnsscorr_e1t_set_codes(self.h, chips.shape[0], _ptr(chips)),
               "gnsscorr_e1t_set_codes")

    def init_chan(self, code_id, code_phase_1b, acq_freq, stream=0, skip=0):
        return e1t_init_chan(self.cfg, code_id, code_phase_1b, acq_freq, stream, skip)


# ---------------------------------------------------------------- GLONASS L3OC float tracking
def l3t_cfg(device: int = 0, **kw) -> L3tCfg:
    """GLONASS/L3/initSettings.sci:64-96 defaults; keyword overrides use the Scilab names
    (samplingFreq, IF, GLONASS_nominal_freq, dllCorrelatorSpacing, switchIQ, ...)."""
    d = _settings(dict(
        fileType=2, switchIQ=0, samplingFreq=24e6, codeFreqBasis=10.23e6, codeLength=10230,
        IF=-2.025e6, GLONASS_nominal_freq=1202.025e6, dllDampingRatio=0.7,
        dllNoiseBandwidth=1.0, dllCorrelatorSpacing=0.4, pllNoiseBandwidth=25.0,
        fllNoiseBandwidth=250.0), kw)
    return L3tCfg(d["fileType"], d["switchIQ"], d["codeLength"], device, 0, 0, d["samplingFreq"],
                  d["codeFreqBasis"], d["IF"], d["GLONASS_nominal_freq"],
                  d["dllCorrelatorSpacing"], d["dllNoiseBandwidth"], d["dllDampingRatio"],
                  d["pllNoiseBandwidth"], d["fllNoiseBandwidth"])


def l3t_loop_coefs(cfg: L3tCfg):
    """(tau1code, tau2code, k1, k2, k3) of a configuration (host only)."""
    return _loop_coefs("gnsscorr_l3t", cfg, 5)


def l3t_init_chan(cfg: L3tCfg, prn, code_phase_1b, acq_freq, stream=0, skip=0) -> np.ndarray:
    """One L3T_CHAN (shape (1,)) from an acquisition result (host only); PRN 1..31."""
    return _init_chan("gnsscorr_l3t", L3T_CHAN, cfg, prn, code_phase_1b, acq_freq, stream, skip)


class L3tCtx(_FloatTracker):
    """GLONASS L3OC float tracking (GLONASS/L3/tracking.sci) for many channels over
    HBM-resident IQ records: pilot and data code on one code NCO, twelve sums, FLL and DLL
    on the data channel, PLL on the pilot."""

    _prefix, _CHAN, _EPOCH, _n_sums, _n_coefs = "gnsscorr_l3t", L3T_CHAN, L3T_EPOCH, 12, 5
    _make_cfg = staticmethod(l3t_cfg)

    def init_chan(self, prn, code_phase_1b, acq_freq, stream=0, skip=0):
        return l3t_init_chan(self.cfg, prn, code_phase_1b, acq_freq, stream, skip)

    def init_chans(self, prns, code_phases_1b, acq_freqs, streams=None, skip=0):
        return super().init_chans(prns, code_phases_1b, acq_freqs, streams, skip)


# ---------------------------------------------------------------- E1B / L3OC navigation symbols
def epoch_field(epoch_dtype, name):
    """(byte offset, epoch stride in bytes) of an fp64 field of E1T_EPOCH, L3T_EPOCH or
    SGT_EPOCH, e.g. epoch_field(E1T_EPOCH, "I_P_P"): d_epochs + offset with that stride is
    the series argument of NavCtx.e1_pages_dev, read in place."""
    dt = np.dtype(epoch_dtype)
    if name not in (dt.names or ()) or dt.fields[name][0] != np.dtype("<f8"):
        raise ValueError(f"{name!r} is not an fp64 field of the epoch record")
    return dt.fields[name][1], dt.itemsize


def nav_conv_encode(msg) -> np.ndarray:
    """convol_encoder.sci for the K = 7 code: (len(msg) + 6) * 2 symbols 0/1 (host only)."""
    msg = np.ascontiguousarray(msg, np.uint8).ravel()
    out = np.zeros((msg.size + 6) * 2, np.uint8)
    _check(lib().gnsscorr_nav_conv_encode(_ptr(msg), msg.size, _ptr(out)),
           "gnsscorr_nav_conv_encode")
    return out


class NavCtx(_Handle):
    """Navigation symbols of Galileo E1B and GLONASS L3OC on the device (csrc/navsym.hip):
    page and overlay synchronisation, deinterleaving and the Scilab receiver's K = 7
    Viterbi decoder, one wave per stream; and frame synchronisation and data bits of GPS
    L1 C/A, GLONASS L1OF and BeiDou B1I (csrc/navbits.hip) from SgtCtx epoch records; and
    the rest of the GPS L1 receiver (csrc/navfix.hip): ephemeris fields and TOW from those
    bits, then pseudoranges, satellite positions and least-squares positions; and the rest
    of the GLONASS L1OF receiver (csrc/navglo.hip): ephemeris fields and frame time from the
    15 strings, the satellite states by Runge-Kutta integration, then the same loop with
    one integration step per fix and PZ-90.02 -> WGS-84; and the rest of the BeiDou B1I
    receiver (csrc/navb1.hip): ephemeris fields and SOW from the five subframes, then the
    loop with Kepler satellite positions and no elevation mask.  The
    *_dev calls are queued on the context's stream and read the trackers' epoch records in
    place (epoch_field)."""

    _prefix = "gnsscorr_nav"

    def __init__(self, device: int = 0):
        self.device = device
        self._create(device, ops=("viterbi", "viterbi_dev", "e1_pages", "e1_pages_dev",
                                  "l3_decode", "l3_decode_dev", "pattern_hits",
                                  "pattern_hits_dev", "gps_frames", "gps_frames_dev",
                                  "glo_strings", "glo_strings_dev", "b1_subframes",
                                  "b1_subframes_dev", "gps_ephemeris", "gps_ephemeris_dev",
                                  "gps_fix", "gps_fix_dev", "glo_ephemeris",
                                  "glo_ephemeris_dev", "glo_satpos", "glo_satpos_dev",
                                  "glo_fix", "glo_fix_dev", "b1_ephemeris", "b1_ephemeris_dev",
                                  "b1_fix", "b1_fix_dev"))

    conv_encode = staticmethod(nav_conv_encode)

    def viterbi(self, code, soft=False) -> np.ndarray:
        """code [n_streams, 2 L] (or [2 L]): uint8 0/1 symbols, or fp64 with soft=True;
        returns bits [n_streams, L] uint8."""
        code = np.ascontiguousarray(code, np.float64 if soft else np.uint8)
        code = code.reshape(1, -1) if code.ndim == 1 else code
        assert code.ndim == 2 and code.shape[1] % 2 == 0
        n, L = code.shape[0], code.shape[1] // 2
        bits = np.zeros((n, L), np.uint8)
        _check(self._viterbi(self.h, _ptr(code), code.strides[0], n, L, int(soft), _ptr(bits)),
               self._viterbi)
        return bits

    def viterbi_dev(self, d_code, stream_stride_bytes, n_streams, L, soft, d_bits):
        _check(self._viterbi_dev(self.h, d_code, stream_stride_bytes, n_streams, L, int(soft),
                                 d_bits), self._viterbi_dev)

    def e1_pages(self, series, max_pages=None):
        """series [n_ch, n_epochs] fp64 (I_P_P); returns first_page [n_ch], n_pages [n_ch]
        and bits [n_ch, max_pages, 120] (max_pages: every whole page part by default)."""
        series = np.ascontiguousarray(series, np.float64)
        series = series.reshape(1, -1) if series.ndim == 1 else series
        n_ch, n_ep = series.shape
        max_pages = max(n_ep // 1000, 1) if max_pages is None else int(max_pages)
        first, n_pages = np.zeros(n_ch, np.int32), np.zeros(n_ch, np.int32)
        bits = np.zeros((n_ch, max_pages, 120), np.uint8)
        _check(self._e1_pages(self.h, _ptr(series), 8, max(series.strides[0], 8), n_ep, n_ch,
                              max_pages, _ptr(first), _ptr(n_pages), _ptr(bits)), self._e1_pages)
        return first, n_pages, bits

    def e1_pages_dev(self, d_series, epoch_stride_bytes, chan_stride_bytes, n_epochs, n_ch,
                     max_pages, d_first_page, d_n_pages, d_bits):
        _check(self._e1_pages_dev(self.h, d_series, epoch_stride_bytes, chan_stride_bytes,
                                  n_epochs, n_ch, max_pages, d_first_page, d_n_pages, d_bits),
               self._e1_pages_dev)

    def l3_decode(self, pilot, data, max_marks=64):
        """pilot (I_P), data (Q_P2): [n_ch, n_epochs] fp64; returns start [n_ch], n_bits
        [n_ch], bits [n_ch, n_epochs // 10], n_marks [n_ch], marks [n_ch, max_marks]."""
        pilot = np.ascontiguousarray(pilot, np.float64)
        data = np.ascontiguousarray(data, np.float64)
        pilot = pilot.reshape(1, -1) if pilot.ndim == 1 else pilot
        data = data.reshape(pilot.shape)
        n_ch, n_ep = pilot.shape
        start, n_bits = np.zeros(n_ch, np.int32), np.zeros(n_ch, np.int32)
        bits = np.zeros((n_ch, n_ep // 10), np.uint8)
        n_marks = np.zeros(n_ch, np.int32)
        marks = np.full((n_ch, int(max_marks)), -1, np.int32)
        _check(self._l3_decode(self.h, _ptr(pilot), _ptr(data), 8, max(pilot.strides[0], 8),
                               n_ep, n_ch, int(max_marks), _ptr(start), _ptr(n_bits),
                               _ptr(bits), _ptr(n_marks), _ptr(marks)),
               self._l3_decode)
        return start, n_bits, bits, n_marks, marks

    def l3_decode_dev(self, d_pilot, d_data, epoch_stride_bytes, chan_stride_bytes, n_epochs,
                      n_ch, max_marks, d_start, d_n_bits, d_bits, d_n_marks, d_marks):
        _check(self._l3_decode_dev(self.h, d_pilot, d_data, epoch_stride_bytes,
                                   chan_stride_bytes, n_epochs, n_ch, max_marks, d_start,
                                   d_n_bits, d_bits, d_n_marks, d_marks), self._l3_decode_dev)

    @staticmethod
    def _series(series):
        """[n_ch, n_epochs] fp64 (or one channel), its channel stride, n_epochs, n_ch"""
        series = np.ascontiguousarray(series, np.float64)
        series = series.reshape(1, -1) if series.ndim == 1 else series
        return series, max(series.strides[0], 8), series.shape[1], series.shape[0]

    def pattern_hits(self, series, pattern, threshold, first_k=0, max_hits=16):
        """series [n_ch, n_epochs] fp64, pattern int8 [T] in {-1, 0, 1}: the k >= first_k with
        |sum_i pattern[i] sign(x[k + i])| > threshold.  Returns first [n_ch], n_hits [n_ch]
        and hits [n_ch, max_hits] (ascending, -1 after the last)."""
        series, cs, n_ep, n_ch = self._series(series)
        pattern = np.ascontiguousarray(pattern, np.int8).ravel()
        first, n_hits = np.zeros(n_ch, np.int32), np.zeros(n_ch, np.int32)
        hits = np.full((n_ch, max(int(max_hits), 1)), -1, np.int32)
        _check(self._pattern_hits(self.h, _ptr(series), 8, cs, n_ep, n_ch, _ptr(pattern),
                                  pattern.size, int(threshold), int(first_k), int(max_hits),
                                  _ptr(first), _ptr(n_hits), _ptr(hits)), self._pattern_hits)
        return first, n_hits, hits

    def pattern_hits_dev(self, d_series, epoch_stride_bytes, chan_stride_bytes, n_epochs, n_ch,
                         pattern, threshold, first_k, max_hits, d_first, d_n_hits, d_hits):
        """pattern: a host int8 array (it reaches the kernel as two masks in its arguments)."""
        pattern = np.ascontiguousarray(pattern, np.int8).ravel()
        _check(self._pattern_hits_dev(self.h, d_series, epoch_stride_bytes, chan_stride_bytes,
                                      n_epochs, n_ch, _ptr(pattern), pattern.size,
                                      int(threshold), int(first_k), int(max_hits), d_first,
                                      d_n_hits, d_hits), self._pattern_hits_dev)

    def gps_frames(self, series, search_start=5000, max_subframes=5):
        """GPS L1 C/A: series [n_ch, n_epochs] fp64 (SGT_EPOCH I_P); returns first_subframe
        [n_ch], n_bits [n_ch] and bits [n_ch, 1500] (0 / 1, 2 for an undecided bit)."""
        series, cs, n_ep, n_ch = self._series(series)
        first, n_bits = np.zeros(n_ch, np.int32), np.zeros(n_ch, np.int32)
        bits = np.zeros((n_ch, 1500), np.uint8)
        _check(self._gps_frames(self.h, _ptr(series), 8, cs, n_ep, n_ch, int(search_start),
                                int(max_subframes), _ptr(first), _ptr(n_bits), _ptr(bits)),
               self._gps_frames)
        return first, n_bits, bits

    def gps_frames_dev(self, d_series, epoch_stride_bytes, chan_stride_bytes, n_epochs, n_ch,
                       search_start, max_subframes, d_first_subframe, d_n_bits, d_bits):
        _check(self._gps_frames_dev(self.h, d_series, epoch_stride_bytes, chan_stride_bytes,
                                    n_epochs, n_ch, search_start, max_subframes,
                                    d_first_subframe, d_n_bits, d_bits), self._gps_frames_dev)

    def glo_strings(self, series, max_strings=15):
        """GLONASS L1OF: returns first_mark [n_ch], n_strings [n_ch] and bits
        [n_ch, 15, 85]."""
        series, cs, n_ep, n_ch = self._series(series)
        first, n_str = np.zeros(n_ch, np.int32), np.zeros(n_ch, np.int32)
        bits = np.zeros((n_ch, 15, 85), np.uint8)
        _check(self._glo_strings(self.h, _ptr(series), 8, cs, n_ep, n_ch, int(max_strings),
                                 _ptr(first), _ptr(n_str), _ptr(bits)), self._glo_strings)
        return first, n_str, bits

    def glo_strings_dev(self, d_series, epoch_stride_bytes, chan_stride_bytes, n_epochs, n_ch,
                        max_strings, d_first_mark, d_n_strings, d_bits):
        _check(self._glo_strings_dev(self.h, d_series, epoch_stride_bytes, chan_stride_bytes,
                                     n_epochs, n_ch, max_strings, d_first_mark, d_n_strings,
                                     d_bits), self._glo_strings_dev)

    def b1_subframes(self, series, max_subframes=5):
        """BeiDou B1I: returns first [n_ch], n_subframes [n_ch] and bits [n_ch, 5, 213]."""
        series, cs, n_ep, n_ch = self._series(series)
        first, n_sub = np.zeros(n_ch, np.int32), np.zeros(n_ch, np.int32)
        bits = np.zeros((n_ch, 5, 213), np.uint8)
        _check(self._b1_subframes(self.h, _ptr(series), 8, cs, n_ep, n_ch, int(max_subframes),
                                  _ptr(first), _ptr(n_sub), _ptr(bits)), self._b1_subframes)
        return first, n_sub, bits

    def b1_subframes_dev(self, d_series, epoch_stride_bytes, chan_stride_bytes, n_epochs, n_ch,
                         max_subframes, d_first, d_n_subframes, d_bits):
        _check(self._b1_subframes_dev(self.h, d_series, epoch_stride_bytes, chan_stride_bytes,
                                      n_epochs, n_ch, max_subframes, d_first, d_n_subframes,
                                      d_bits), self._b1_subframes_dev)

    def _ephemeris(self, fn, shape, dtype, bits, n_units, first) -> np.ndarray:
        bits = np.ascontiguousarray(bits, np.uint8).reshape(-1, *shape)
        n_ch = bits.shape[0]
        n_units = np.ascontiguousarray(n_units, np.int32).reshape(n_ch)
        first = np.ascontiguousarray(first, np.int32).reshape(n_ch)
        eph = np.zeros(n_ch, dtype)
        _check(fn(self.h, _ptr(bits), _ptr(n_units), _ptr(first), n_ch, _ptr(eph)), fn)
        return eph

    def _fix_host(self, fn, eph_dtype, eph, extra_inputs, first, abs_sample, rx_first, cfg,
                  n_meas, sol, chan):
        """extra_inputs: (array, dtype) of each per-channel input between eph and first"""
        eph = np.ascontiguousarray(eph, eph_dtype).ravel()
        n_ch = eph.size
        extra = [np.ascontiguousarray(x, dt).reshape(n_ch) for x, dt in extra_inputs]
        first = np.ascontiguousarray(first, np.int32).reshape(n_ch)
        series, cs, n_ep, _ = self._series(abs_sample)
        assert series.shape[0] == n_ch
        rx_first = np.ascontiguousarray(rx_first, np.int32).ravel()
        n_rx = rx_first.size - 1
        n_meas = np.zeros(n_rx, np.int32) if n_meas is None else n_meas
        sol = np.zeros((n_rx, cfg.max_meas), GPS_FIX_SOL) if sol is None else sol
        chan = np.zeros((n_ch, cfg.max_meas), GPS_FIX_CHAN) if chan is None else chan
        _check(fn(self.h, _ptr(eph), *[_ptr(x) for x in extra], _ptr(first), _ptr(series), 8, cs,
                  n_ep, n_rx, _ptr(rx_first), C.addressof(cfg), _ptr(n_meas), _ptr(sol),
                  _ptr(chan)), fn)
        return n_meas, sol, chan

    def _fix_dev(self, fn, d_inputs, d_abs_sample, epoch_stride_bytes, chan_stride_bytes,
                 n_epochs, rx_first, cfg, d_n_meas, d_sol, d_chan):
        rx_first = np.ascontiguousarray(rx_first, np.int32).ravel()
        _check(fn(self.h, *d_inputs, d_abs_sample, epoch_stride_bytes, chan_stride_bytes,
                  n_epochs, rx_first.size - 1, _ptr(rx_first),
                  C.addressof(cfg) if cfg is not None else None, d_n_meas, d_sol, d_chan), fn)

    def gps_ephemeris(self, bits, n_bits, first_subframe) -> np.ndarray:
        """GPS L1: bits [n_ch, 1500], n_bits [n_ch] and first_subframe [n_ch] as gps_frames
        returns them -> GPS_EPH [n_ch] (ephemeris.sci:82-226; status GPS_EPH_*)."""
        return self._ephemeris(self._gps_ephemeris, (1500,), GPS_EPH, bits, n_bits,
                               first_subframe)

    def gps_ephemeris_dev(self, d_bits, d_n_bits, d_first_subframe, n_ch, d_eph):
        _check(self._gps_ephemeris_dev(self.h, d_bits, d_n_bits, d_first_subframe, n_ch, d_eph),
               self._gps_ephemeris_dev)

    def gps_fix(self, eph, first_subframe, abs_sample, rx_first, cfg, n_meas=None, sol=None,
                chan=None):
        """GPS L1: eph GPS_EPH [n_ch], first_subframe [n_ch], abs_sample [n_ch, n_epochs] fp64
        (SGT_EPOCH absoluteSample), rx_first [n_rx + 1] channel offsets, cfg from gps_fix_cfg.
        Returns n_meas [n_rx], sol GPS_FIX_SOL [n_rx, max_meas] and chan GPS_FIX_CHAN
        [n_ch, max_meas]; rows past n_meas keep what sol and chan held (zeros by default)."""
        return self._fix_host(self._gps_fix, GPS_EPH, eph, (), first_subframe, abs_sample,
                              rx_first, cfg, n_meas, sol, chan)

    def gps_fix_dev(self, d_eph, d_first_subframe, d_abs_sample, epoch_stride_bytes,
                    chan_stride_bytes, n_epochs, rx_first, cfg, d_n_meas, d_sol, d_chan):
        """rx_first: a host int32 array of n_rx + 1 offsets (checked before the launch)."""
        self._fix_dev(self._gps_fix_dev, (d_eph, d_first_subframe), d_abs_sample,
                      epoch_stride_bytes, chan_stride_bytes, n_epochs, rx_first, cfg, d_n_meas,
                      d_sol, d_chan)

    def glo_ephemeris(self, bits, n_strings, first_mark) -> np.ndarray:
        """GLONASS L1OF: bits [n_ch, 15, 85], n_strings [n_ch] and first_mark [n_ch] as
        glo_strings returns them -> GLO_EPH [n_ch] (ephemeris.sci:25-98; status GLO_EPH_*)."""
        return self._ephemeris(self._glo_ephemeris, (15, 85), GLO_EPH, bits, n_strings,
                               first_mark)

    def glo_ephemeris_dev(self, d_bits, d_n_strings, d_first_mark, n_ch, d_eph):
        _check(self._glo_ephemeris_dev(self.h, d_bits, d_n_strings, d_first_mark, n_ch, d_eph),
               self._glo_ephemeris_dev)

    def glo_satpos(self, eph, cfg) -> np.ndarray:
        """GLONASS L1OF: eph GLO_EPH [n_ch], cfg from glo_fix_cfg (its navSolPeriod) ->
        GLO_SAT [n_ch]: the satellite states one navSolPeriod before each channel's frame
        time (satposg.sci); zeros for a channel that is not ready."""
        eph = np.ascontiguousarray(eph, GLO_EPH).ravel()
        sat = np.zeros(eph.size, GLO_SAT)
        _check(self._glo_satpos(self.h, _ptr(eph), eph.size, C.addressof(cfg), _ptr(sat)),
               self._glo_satpos)
        return sat

    def glo_satpos_dev(self, d_eph, n_ch, cfg, d_sat):
        _check(self._glo_satpos_dev(self.h, d_eph, n_ch,
                                    C.addressof(cfg) if cfg is not None else None, d_sat),
               self._glo_satpos_dev)

    def glo_fix(self, eph, sat, first_mark, abs_sample, rx_first, cfg, n_meas=None, sol=None,
                chan=None):
        """GLONASS L1OF: eph GLO_EPH [n_ch], sat GLO_SAT [n_ch] from glo_satpos with the same
        cfg, first_mark [n_ch], abs_sample [n_ch, n_epochs] fp64 (SGT_EPOCH absoluteSample),
        rx_first [n_rx + 1] channel offsets.  Returns n_meas [n_rx], sol GPS_FIX_SOL
        [n_rx, max_meas] and chan GPS_FIX_CHAN [n_ch, max_meas]; rows past n_meas keep what
        sol and chan held (zeros by default)."""
        return self._fix_host(self._glo_fix, GLO_EPH, eph, ((sat, GLO_SAT),), first_mark,
                              abs_sample, rx_first, cfg, n_meas, sol, chan)

    def glo_fix_dev(self, d_eph, d_sat, d_first_mark, d_abs_sample, epoch_stride_bytes,
                    chan_stride_bytes, n_epochs, rx_first, cfg, d_n_meas, d_sol, d_chan):
        """rx_first: a host int32 array of n_rx + 1 offsets (checked before the launch)."""
        self._fix_dev(self._glo_fix_dev, (d_eph, d_sat, d_first_mark), d_abs_sample,
                      epoch_stride_bytes, chan_stride_bytes, n_epochs, rx_first, cfg, d_n_meas,
                      d_sol, d_chan)

    def b1_ephemeris(self, bits, n_subframes, first) -> np.ndarray:
        """BeiDou B1I: bits [n_ch, 5, 213], n_subframes [n_ch] and first [n_ch] as
        b1_subframes returns them -> B1_EPH [n_ch] (ephemeris.sci:28-123; status B1_EPH_*)."""
        return self._ephemeris(self._b1_ephemeris, (5, 213), B1_EPH, bits, n_subframes, first)

    def b1_ephemeris_dev(self, d_bits, d_n_subframes, d_first, n_ch, d_eph):
        _check(self._b1_ephemeris_dev(self.h, d_bits, d_n_subframes, d_first, n_ch, d_eph),
               self._b1_ephemeris_dev)

    def b1_fix(self, eph, first, abs_sample, rx_first, cfg, n_meas=None, sol=None, chan=None):
        """BeiDou B1I: eph B1_EPH [n_ch], first [n_ch], abs_sample [n_ch, n_epochs] fp64
        (SGT_EPOCH absoluteSample), rx_first [n_rx + 1] channel offsets, cfg from b1_fix_cfg.
        Returns n_meas [n_rx], sol GPS_FIX_SOL [n_rx, max_meas] and chan GPS_FIX_CHAN
        [n_ch, max_meas]; rows past n_meas keep what sol and chan held (zeros by default)."""
        return self._fix_host(self._b1_fix, B1_EPH, eph, (), first, abs_sample, rx_first, cfg,
                              n_meas, sol, chan)

    def b1_fix_dev(self, d_eph, d_first, d_abs_sample, epoch_stride_bytes, chan_stride_bytes,
                   n_epochs, rx_first, cfg, d_n_meas, d_sol, d_chan):
        """rx_first: a host int32 array of n_rx + 1 offsets (checked before the launch)."""
        self._fix_dev(self._b1_fix_dev, (d_eph, d_first), d_abs_sample, epoch_stride_bytes,
                      chan_stride_bytes, n_epochs, rx_first, cfg, d_n_meas, d_sol, d_chan)


def _fix_cfg(name, struct, allowed, max_meas, kw):
    cfg = struct()
    getattr(lib(), f"gnsscorr_nav_{name}_init")(C.byref(cfg))
    cfg.max_meas = int(max_meas)
    for k, v in kw.items():
        if k not in allowed:
            raise GnssCorrError(f"{name}: unknown setting {k!r}")
        setattr(cfg, k, v)
    return cfg


def gps_fix_cfg(max_meas=1, **kw) -> GpsFixCfg:
    """GPS/L1/initSettings.sci:103-125 defaults (samplesPerCode 16000, startOffset 68.802,
    c 299792458, navSolPeriod 500, elevationMask 10, useTropCorr 1); keyword overrides use
    the Scilab names."""
    return _fix_cfg("gps_fix_cfg", GpsFixCfg, ("samplesPerCode", "startOffset", "c",
                                               "elevationMask", "navSolPeriod", "useTropCorr"),
                    max_meas, kw)


def glo_fix_cfg(max_meas=1, **kw) -> GloFixCfg:
    """GLONASS/L1/initSettings.sci:59-136 defaults (samplesPerCode 16000, dataTypeSizeInBytes
    1, c 299792458, navSolPeriod 500, elevationMask 0, useTropCorr 1); keyword overrides use
    the Scilab names."""
    return _fix_cfg("glo_fix_cfg", GloFixCfg, ("samplesPerCode", "dataTypeSizeInBytes", "c",
                                               "elevationMask", "navSolPeriod", "useTropCorr"),
                    max_meas, kw)


def b1_fix_cfg(max_meas=1, **kw) -> B1FixCfg:
    """COMPASS/B1/initSettings.sci defaults (samplesPerCode 16000, dataTypeSizeInBytes 1,
    c 299792458, navSolPeriod 500, useTropCorr 0; the receiver has no elevation mask);
    keyword overrides use the Scilab names."""
    return _fix_cfg("b1_fix_cfg", B1FixCfg, ("samplesPerCode", "dataTypeSizeInBytes", "c",
                                             "navSolPeriod", "useTropCorr"), max_meas, kw)


# ---------------------------------------------------------------- GPS-SDR integer acquisition
def sdr_prn_codes() -> np.ndarray:
    """PRN_Codes (51, 2048, 2) int16 as gen_fft_codes.m builds them."""
    out = np.zeros((51, 2048, 2), np.int16)
    _check(lib().gnsscorr_sdr_prn_codes(_ptr(out)), "gnsscorr_sdr_prn_codes")
    return out


def sdr_sine_gen(f: float, n: int = 2048, fs: float = 2048000.0) -> np.ndarray:
    out = np.zeros((n, 2), np.int16)
    lib().gnsscorr_sdr_sine_gen(_ptr(out), f, fs, n)
    return out


class SdrAcqCtx(_Handle):
    """GPS-SDR strong (1 ms, int16 FFT) acquisition, bit-exact with the reference."""

    _prefix = "gnsscorr_sdr_acq"

    def __init__(self, fif: float = 38400.0, device: int = 0, saturate: bool = False):
        self._create(C.byref(SdrAcqCfg(fif, device, int(saturate))))

    def strong(self, buffers, svs, doppmin=-15000, doppmax=15000) -> np.ndarray:
        """buffers: (n_rec, 2048, 2) or (2048, 2) int16; returns SDR_RESULT [n_rec, n_sv]."""
        b = np.ascontiguousarray(buffers, np.int16).reshape(-1, 2048, 2)
        svs = np.ascontiguousarray(svs, np.int32)
        res = np.zeros((b.shape[0], len(svs)), SDR_RESULT)
        _check(lib().gnsscorr_sdr_acq_strong(self.h, _ptr(b), b.shape[0], len(svs), _ptr(svs),
                                             doppmin, doppmax, _ptr(res)),
               "gnsscorr_sdr_acq_strong")
        return res

    def acquire(self, acq_type, buffers, svs, doppmin=-15000, doppmax=15000) -> np.ndarray:
        """Acquisition::Acquire for one request type (doPrepIF + doAcqStrong /
        doAcqMedium / doAcqWeak).  buffers: (n_rec, ms*2048, 2) int16 with ms =
        1 / 10 / 310; returns SDR_RESULT [n_rec, n_sv].  Medium and weak preps
        update the context's persistent per-record row store."""
        ms = SDR_ACQ_MS[acq_type]
        b = np.ascontiguousarray(buffers, np.int16).reshape(-1, ms * 2048, 2)
        svs = np.ascontiguousarray(svs, np.int32)
        res = np.zeros((b.shape[0], len(svs)), SDR_RESULT)
        _check(lib().gnsscorr_sdr_acq_acquire(self.h, acq_type, _ptr(b), b.shape[0], len(svs),
                                              _ptr(svs), doppmin, doppmax, _ptr(res)),
               "gnsscorr_sdr_acq_acquire")
        return res

    def prep_dev(self, acq_type, d_buff, n_rec):
        _check(lib().gnsscorr_sdr_acq_prep_dev(self.h, acq_type, d_buff, n_rec),
               "gnsscorr_sdr_acq_prep_dev")

    def search_dev(self, acq_type, n_rec, n_sv, d_svs, d_res, doppmin=-15000, doppmax=15000):
        _check(lib().gnsscorr_sdr_acq_search_dev(self.h, acq_type, n_rec, n_sv, d_svs, doppmin,
                                                 doppmax, d_res), "gnsscorr_sdr_acq_search_dev")

    def strong_dev(self, d_buff, n_rec, n_sv, d_svs, d_res, doppmin=-15000, doppmax=15000):
        _check(lib().gnsscorr_sdr_acq_strong_dev(self.h, d_buff, n_rec, n_sv, d_svs, doppmin,
                                                 doppmax, d_res), "gnsscorr_sdr_acq_strong_dev")

    def read_rows(self, n_rec, n_sv, n_rows) -> np.ndarray:
        """The last search's per-row (magnitude, index) table, int32
        [n_rec, n_sv, n_rows, 2]; the three counts are that search's."""
        out = np.zeros((n_rec, n_sv, n_rows, 2), np.int32)
        _check(lib().gnsscorr_sdr_acq_read_rows(self.h, _ptr(out), n_rec * n_sv * n_rows),
               "gnsscorr_sdr_acq_read_rows")
        return out

    def read_spectra(self, acq_type, rec, row0, n_rows) -> np.ndarray:
        """Prepared spectra, int16 [n_rows, 2048, 2]: rows of the last strong
        search's four (SDR_ACQ_STRONG) or of the persistent 1240-row store
        (SDR_ACQ_MEDIUM / SDR_ACQ_WEAK) of record rec, as last written."""
        out = np.zeros((max(int(n_rows), 1), 2048, 2), np.int16)
        _check(lib().gnsscorr_sdr_acq_read_spectra(self.h, acq_type, rec, row0, n_rows,
                                                   _ptr(out)), "gnsscorr_sdr_acq_read_spectra")
        return out


class OsgLoopCfg(C.Structure):
    _fields_ = [("carrier_ref", C.c_int64), ("code_ref", C.c_int64), ("d_freq", C.c_int64),
                ("fll_i1", C.c_int32), ("fll_i2", C.c_int32), ("fll_i3", C.c_int32),
                ("dll_i1", C.c_int32), ("dll_i2", C.c_int32), ("acq_thresh", C.c_int32),
                ("confirm_m", C.c_int32), ("n_of_m_thresh", C.c_int32),
                ("carrier_shift", C.c_int32), ("code_shift", C.c_int32),
                ("clock_mult", C.c_double)]


def osg_loop_cfg(samp_rate=16.0e6, gps_if=2.42e6, clock_mult=5.0, carrier_bits=30, code_bits=29,
                 bin_width=1000.0, bnp=25, bnf=1400, bnd=2, fll_t_ms=1, dll_t_ms=1,
                 acq_thresh=1800) -> OsgLoopCfg:
    """Receiver loop constants as the reference derives them (globals.h defaults)."""
    cfg = OsgLoopCfg()
    lib().gnsscorr_osg_loop_cfg_init(C.byref(cfg), samp_rate, gps_if, clock_mult, carrier_bits,
                                     code_bits, bin_width, bnp, bnf, bnd, fll_t_ms, dll_t_ms,
                                     acq_thresh)
    return cfg


def osg_loop_reset(cfg: OsgLoopCfg, prns):
    """Start state of every channel (reset_all_correlator_channles) -> (loops, cmds)."""
    prns = np.ascontiguousarray(prns, np.int32)
    loops = np.zeros(len(prns), OSG_LOOP)
    cmds = np.zeros(len(prns), NCO_CMD)
    lib().gnsscorr_osg_loop_reset(C.byref(cfg), len(prns), _ptr(prns), _ptr(loops), _ptr(cmds))
    return loops, cmds


def osg_isr_dev(track: "TrackCtx", cfg: OsgLoopCfg, n_ch, d_loops, d_cmds, d_res):
    _check(lib().gnsscorr_osg_isr_dev(track.h, C.byref(cfg), n_ch, d_loops, d_cmds, d_res),
           "gnsscorr_osg_isr_dev")


def osg_closed_loop_dev(track: "TrackCtx", cfg: OsgLoopCfg, d_if, stream_stride, nsamp, n_calls,
                        n_ch, d_loops, d_cmds, d_res_hist, d_loop_hist=None):
    _check(lib().gnsscorr_osg_closed_loop_dev(track.h, C.byref(cfg), d_if, stream_stride, nsamp,
                                              n_calls, n_ch, d_loops, d_cmds, d_res_hist,
                                              d_loop_hist), "gnsscorr_osg_closed_loop_dev")


GN3S_BLOCK_IN, GN3S_BLOCK_OUT, GN3S_STEP = 20000, 10240, 2557223528


def gn3s_products() -> np.ndarray:
    """The GN3S front end's int16 product table [4 codes, 1024 phases, 2]."""
    out = np.zeros((4, 1024, 2), np.int16)
    lib().gnsscorr_sdr_gn3s_products(_ptr(out))
    return out


def pack_2bit(samples) -> np.ndarray:
    """One-sample-per-byte 2-bit codes -> packed bytes (sample j in bits 2j..2j+1)."""
    s = np.ascontiguousarray(samples, np.uint8).reshape(-1, 4) & 3
    return (s[:, 0] | (s[:, 1] << 2) | (s[:, 2] << 4) | (s[:, 3] << 6)).astype(np.uint8)


class SdrFeCtx(_Handle):
    """GPS-SDR sample front end: GN3S 2-bit unpack + NCO mix + resample, downsample."""

    _prefix = "gnsscorr_sdr_fe"

    def __init__(self, device: int = 0):
        self._create(device)

    def gn3s(self, data, packed=False, phase=0, step=GN3S_STEP):
        """data: n_blocks * 20000 bytes (or / 4 when packed); returns (CPX [n*10240, 2], phase)."""
        d = np.ascontiguousarray(data, np.uint8).ravel()
        per = GN3S_BLOCK_IN // 4 if packed else GN3S_BLOCK_IN
        nb = d.size // per
        out = np.zeros((nb * GN3S_BLOCK_OUT, 2), np.int16)
        ph = C.c_uint32(phase)
        _check(lib().gnsscorr_sdr_gn3s(self.h, _ptr(d), int(packed), nb, C.byref(ph),
                                       C.c_uint32(step), _ptr(out)), "gnsscorr_sdr_gn3s")
        return out, ph.value

    def gn3s_dev(self, d_in, packed, n_blocks, phase, d_out, step=GN3S_STEP) -> int:
        ph = C.c_uint32(phase)
        _check(lib().gnsscorr_sdr_gn3s_dev(self.h, d_in, int(packed), n_blocks, C.byref(ph),
                                           C.c_uint32(step), d_out), "gnsscorr_sdr_gn3s_dev")
        return ph.value

    def downsample_dev(self, d_src, n_src, fdest, fsource, d_dest) -> int:
        n = C.c_int()
        _check(lib().gnsscorr_sdr_downsample_dev(self.h, d_src, n_src, C.c_double(fdest),
                                                 C.c_double(fsource), d_dest, C.byref(n)),
               "gnsscorr_sdr_downsample_dev")
        return n.value

    @staticmethod
    def downsample_count(n_src, fdest, fsource) -> int:
        return lib().gnsscorr_sdr_downsample_count(n_src, C.c_double(fdest), C.c_double(fsource),
                                                   None)


class SdrCorrCtx(_Handle):
    """GPS-SDR tracking correlator (Correlator class): batched Accum on the GPU,
    Correlate schedule + UpdateState/DumpAccum on the host, channel loop by callback."""

    _prefix = "gnsscorr_sdr_corr"

    def __init__(self, device: int = 0, saturate: bool = False):
        self._create(C.byref(SdrCorrCfg(device, int(saturate))))
        self.device = device

    @staticmethod
    def init_chan(sv, acq_code_phase, acq_doppler, packets_since_acq=0.0) -> np.ndarray:
        out = np.zeros(1, SDR_CHAN)
        _check(lib().gnsscorr_sdr_init_chan(_ptr(out), int(sv), int(acq_code_phase),
                                            int(acq_doppler), float(packets_since_acq)),
               "gnsscorr_sdr_init_chan")
        return out[0]

    @staticmethod
    def channel_start(chan, sv, acq_doppler, corr_len=1) -> np.ndarray:
        """Channel::Clear + Channel::Start (objects/channel.cpp:71-170)."""
        out = np.zeros(1, SDR_CHANNEL)
        _check(lib().gnsscorr_sdr_channel_start(_ptr(out), int(chan), int(sv), int(acq_doppler),
                                                int(corr_len)), "gnsscorr_sdr_channel_start")
        return out[0]

    def channel_accum_dev(self, n_ch, n_ms, d_corr, d_chans, d_fb, d_fb_last, d_events,
                          max_events, d_n_events):
        _check(lib().gnsscorr_sdr_channel_accum_dev(self.h, n_ch, n_ms, d_corr, d_chans, d_fb,
                                                    d_fb_last, d_events, max_events, d_n_events),
               "gnsscorr_sdr_channel_accum_dev")

    def channel_accum(self, corr, chans, max_events=4096, all_feedback=True):
        """n_ms Channel::Accum calls per channel: corr (n_ms, n_ch, 6) int32 rows
        (I_E, I_P, I_L, Q_E, Q_P, Q_L); chans SDR_CHANNEL[n_ch] updated in place.
        Returns (feedback SDR_FEEDBACK[n_ms, n_ch] or [n_ch], subframes sorted by (ms, chan))."""
        corr = np.ascontiguousarray(corr, np.int32)
        n_ms, n_ch = corr.shape[0], corr.shape[1]
        assert chans.dtype == SDR_CHANNEL and len(chans) == n_ch
        dev = self.device
        d_c = DevBuf.from_array(corr, dev)
        d_s = DevBuf.from_array(chans, dev)
        d_fb = DevBuf(max(n_ms, 1) * n_ch * SDR_FEEDBACK.itemsize, dev) if all_feedback else None
        d_last = DevBuf(n_ch * SDR_FEEDBACK.itemsize, dev)
        d_ev = DevBuf(max(max_events, 1) * SDR_SUBFRAME.itemsize, dev)
        d_n = DevBuf.from_array(np.zeros(1, np.int32), dev)
        self.channel_accum_dev(n_ch, n_ms, d_c.ptr, d_s.ptr, d_fb.ptr if d_fb else None,
                               d_last.ptr, d_ev.ptr, max_events, d_n.ptr)
        self.sync()
        chans[:] = d_s.download(np.uint8).view(SDR_CHANNEL)
        n = int(d_n.download(np.int32)[0])
        if n > max_events:
            # the kernel keeps whichever max_events subframes won the append race
            raise GnssCorrError(f"channel_accum: {n} subframes exceed max_events={max_events}; "
                                "the kept set would be arbitrary -- raise max_events")
        ev = d_ev.download(np.uint8).view(SDR_SUBFRAME)[:n]
        ev = ev[np.lexsort((ev["chan"], ev["ms"]))]
        if all_feedback:
            fb = d_fb.download(np.uint8).view(SDR_FEEDBACK)[:n_ms * n_ch].reshape(n_ms, n_ch)
        else:
            fb = d_last.download(np.uint8).view(SDR_FEEDBACK)
        return fb, ev, n

    def track_dev(self, d_packets, n_packets, n_rx, n_ch, d_rx, d_states, d_corr, d_chans,
                  d_fb_last, d_log, log_per_ch, d_n_log, d_status, d_events, max_events,
                  d_n_events):
        _check(lib().gnsscorr_sdr_track_dev(self.h, d_packets, n_packets, n_rx, n_ch, d_rx,
                                            d_states, d_corr, d_chans, d_fb_last, d_log,
                                            log_per_ch, d_n_log, d_status, d_events, max_events,
                                            d_n_events), "gnsscorr_sdr_track_dev")

    def track(self, packets, states, corr, chans, rx=None, log_per_ch=0, max_events=4096):
        """The closed loop on the device: packets (n_packets, n_rx, 2048, 2) int16;
        states SDR_CHAN[n_ch], corr SDR_CORR[n_ch], chans SDR_CHANNEL[n_ch] updated in
        place (chans[c] steers states[c]).  Returns dict(fb_last, log SDR_DUMP_REC
        [n_ch, log_per_ch], n_log, status, events sorted by (ms = packet, chan)).
        Raises when a channel's state left the tables (status != 0)."""
        pk = np.ascontiguousarray(packets, np.int16)
        n_packets, n_rx = pk.shape[0], pk.shape[1]
        assert pk.shape[2:] == (2048, 2), pk.shape
        n_ch = len(states)
        assert states.dtype == SDR_CHAN and corr.dtype == SDR_CORR and chans.dtype == SDR_CHANNEL
        assert len(corr) == n_ch and len(chans) == n_ch
        dev = self.device
        d_pk = DevBuf.from_array(pk, dev)
        d_rx = None if rx is None else DevBuf.from_array(np.ascontiguousarray(rx, np.int32), dev)
        d_st, d_c, d_ch = (DevBuf.from_array(a, dev) for a in (states, corr, chans))
        d_last = DevBuf.from_array(np.zeros(n_ch, SDR_FEEDBACK), dev)
        d_log = DevBuf(max(n_ch * log_per_ch, 1) * SDR_DUMP_REC.itemsize, dev)
        d_nlog = DevBuf.from_array(np.zeros(n_ch, np.int32), dev)
        d_stat = DevBuf.from_array(np.zeros(n_ch, np.int32), dev)
        d_ev = DevBuf(max(max_events, 1) * SDR_SUBFRAME.itemsize, dev)
        d_n = DevBuf.from_array(np.zeros(1, np.int32), dev)
        self.track_dev(d_pk.ptr, n_packets, n_rx, n_ch, None if d_rx is None else d_rx.ptr,
                       d_st.ptr, d_c.ptr, d_ch.ptr, d_last.ptr, d_log.ptr, log_per_ch,
                       d_nlog.ptr, d_stat.ptr, d_ev.ptr, max_events, d_n.ptr)
        self.sync()
        status = d_stat.download(np.int32)[:n_ch]
        states[:] = d_st.download(np.uint8).view(SDR_CHAN)
        corr[:] = d_c.download(np.uint8).view(SDR_CORR)
        chans[:] = d_ch.download(np.uint8).view(SDR_CHANNEL)
        if np.any(status != 0):
            c = int(np.flatnonzero(status)[0])
            raise GnssCorrError(f"sdr track: channel {c} stopped (status {int(status[c])}: "
                                "-1 bad receiver index, 1+p state out of the tables at packet p)")
        n = int(d_n.download(np.int32)[0])
        if n > max_events:
            raise GnssCorrError(f"sdr track: {n} subframes exceed max_events={max_events}")
        ev = d_ev.download(np.uint8).view(SDR_SUBFRAME)[:n]
        ev = ev[np.lexsort((ev["chan"], ev["ms"]))]
        log = d_log.download(np.uint8).view(SDR_DUMP_REC)[:n_ch * log_per_ch]
        return dict(fb_last=d_last.download(np.uint8).view(SDR_FEEDBACK),
                    log=log.reshape(n_ch, log_per_ch), n_log=d_nlog.download(np.int32)[:n_ch],
                    status=status, events=ev)

    def accum_dev(self, d_packets, n_jobs, d_jobs, d_out):
        _check(lib().gnsscorr_sdr_accum_dev(self.h, d_packets, n_jobs, d_jobs, d_out),
               "gnsscorr_sdr_accum_dev")

    def correlate(self, packets, states, corr, cb, user=None, rx=None):
        """packets: (n, 2048, 2) int16; states SDR_CHAN[n_ch], corr SDR_CORR[n_ch] in place;
        cb: a C function pointer (int) of gnsscorr_sdr_dump_fn type; user: pointer or None."""
        pk = np.ascontiguousarray(packets, np.int16).reshape(-1, 2048, 2)
        assert states.dtype == SDR_CHAN and corr.dtype == SDR_CORR
        rxa = None if rx is None else np.ascontiguousarray(rx, np.int32)
        _check(lib().gnsscorr_sdr_correlate(self.h, _ptr(pk), pk.shape[0], len(states),
                                            None if rxa is None else _ptr(rxa), _ptr(states),
                                            _ptr(corr), cb, user),
               "gnsscorr_sdr_correlate")


# ---------------------------------------------------------------- legacy OSG view
class OSG:
    """The reference's GP2021 register interface, backed by libgnsscorr.

    Accessors mirror osgnss_next_step/src/gp2021/gp2021.c:11-130 (same
    arithmetic, including the NCO word scaling and the `short` truncation of
    from_gps)."""

    MAX_DIGIT = 32

    def __init__(self, samp_rate=16.0e6, gps_if=2.42e6, glonass_if=0.0, sys_clock_mult=5.0,
                 carrier_bits=30, code_bits=29, n_channels=12, use_iq=True,
                 freq_bin_width=1000.0, device=0):
        L = lib()
        _check(L.gnsscorr_osg_configure(samp_rate, gps_if, glonass_if, sys_clock_mult,
                                        carrier_bits, code_bits, n_channels, int(use_iq),
                                        freq_bin_width, device), "gnsscorr_osg_configure")
        self.mult = sys_clock_mult
        self.n_channels = n_channels
        self.carrier_bits = carrier_bits
        self.code_bits = code_bits
        self.REG_read = (C.c_int * 256).in_dll(L, "REG_read")
        self.REG_write = (C.c_int * 256).in_dll(L, "REG_write")

    def get_state(self, n_channels: int = 12) -> np.ndarray:
        st = np.zeros(n_channels, CHAN_STATE)
        _check(lib().gnsscorr_osg_get_state(_ptr(st)), "gnsscorr_osg_get_state")
        return st

    def chan_state(self):
        st = self.get_state(self.n_channels)
        return dict(carrier_phase=st["carrier_phase"].copy(),
                    carrier_cycle=st["carrier_cycle"].copy(),
                    code_phase=st["code_phase"].copy(), half_chip=st["half_chip"].copy(),
                    acc=st["acc"].copy())

    def correlator_init(self, tic_period: float = 0.0):
        lib().correlator_init(tic_period)

    def sim(self, IF: np.ndarray, nsamp: int):
        IF = np.ascontiguousarray(IF, np.int8)
        lib().Sim_GP2021_int(_ptr(IF), nsamp)

    @property
    def gps_carrier_ref(self):
        return C.c_long.in_dll(lib(), "gps_carrier_ref").value

    @property
    def gps_code_ref(self):
        return C.c_long.in_dll(lib(), "gps_code_ref").value

    @property
    def d_freq(self):
        return C.c_long.in_dll(lib(), "d_freq").value

    # --- gp2021.c accessors ---
    def _outpwd(self, add, data):
        self.REG_write[add & 0xFF] = int(data) & 0xFFFF

    def _from_gps(self, add):
        v = self.REG_read[add] & 0xFFFF
        return v - 0x10000 if v >= 0x8000 else v

    def ch_cntl(self, ch, data):
        self._outpwd(ch << 3, data)

    def ch_code_slew(self, ch, data):
        self._outpwd((ch << 3) + 0x84, data)

    def ch_epoch_load(self, ch, data):
        self._outpwd((ch << 3) + 7, data)

    def ch_carrier(self, ch, freq):
        f = int(float(freq << (self.MAX_DIGIT - self.carrier_bits)) * self.mult)
        self._outpwd((ch << 3) + 3, (f >> 16) & 0xFFFF)
        self._outpwd((ch << 3) + 4, f & 0xFFFF)

    def ch_code(self, ch, freq):
        f = int(float(freq << (self.MAX_DIGIT - self.code_bits)) * self.mult)
        self._outpwd((ch << 3) + 5, (f >> 16) & 0xFFFF)
        self._outpwd((ch << 3) + 6, f & 0xFFFF)

    def accum_status(self):
        return self._from_gps(0x82)

    def ch_i_late(self, ch):
        return self._from_gps((ch << 3) + 0x84)

    def ch_q_late(self, ch):
        return self._from_gps((ch << 3) + 0x85)

    def ch_i_prompt(self, ch):
        return self._from_gps((ch << 3) + 0x86)

    def ch_q_prompt(self, ch):
        return self._from_gps((ch << 3) + 0x87)

    def ch_i_early(self, ch):
        return self._from_gps((ch << 3) + 0x88)

    def ch_q_early(self, ch):
        return self._from_gps((ch << 3) + 0x89)
