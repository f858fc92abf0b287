"""The error contract of the seven create functions on a machine without a HIP device:
a bad configuration is refused with its own text before any device call, and a valid one
answers GNSSCORR_ENODEV with "<function>: no HIP device".  The texts are the library's
public behaviour (callers match on them), so they hold for any build of it: the module
also passes against another build named by GNSSCORR_LIB.
"""
import ctypes as C

import pytest

EINVAL, ENODEV = -1, -4


@pytest.fixture(scope="module")
def L(gc):
    if gc.device_count() > 0:
        pytest.skip("a HIP device is visible: create succeeds (tests/test_hostctx_gpu.py)")
    return gc.lib()


def _last(L):
    return L.gnsscorr_last_error().decode()


def _good(gc):
    """name -> call(handle) with a valid configuration"""
    L = gc.lib()
    track = gc.TrackCfg(1, gc.IF_IQ, 0, 4096, 16.368e6, 0.0)
    acq = gc.AcqCfg(16.368e6, 64, 0, 1, 1, 1, gc.ACQ_F64)
    acq32 = gc.AcqCfg(16.368e6, 16368, 0, 1, 1, 1, gc.ACQ_F32)
    sgt, e1t = gc.sgt_cfg(0), gc.e1t_cfg()
    sdr_acq, sdr_corr = gc.SdrAcqCfg(38400.0, 0, 0), gc.SdrCorrCfg(0, 0)
    return [
        ("gnsscorr_track_create", lambda h: L.gnsscorr_track_create(C.byref(h), C.byref(track))),
        ("gnsscorr_acq_create", lambda h: L.gnsscorr_acq_create(C.byref(h), C.byref(acq))),
        ("gnsscorr_acq_create", lambda h: L.gnsscorr_acq_create(C.byref(h), C.byref(acq32))),
        ("gnsscorr_sgt_create", lambda h: L.gnsscorr_sgt_create(C.byref(h), C.byref(sgt))),
        ("gnsscorr_e1t_create", lambda h: L.gnsscorr_e1t_create(C.byref(h), C.byref(e1t))),
        ("gnsscorr_sdr_acq_create",
         lambda h: L.gnsscorr_sdr_acq_create(C.byref(h), C.byref(sdr_acq))),
        ("gnsscorr_sdr_corr_create",
         lambda h: L.gnsscorr_sdr_corr_create(C.byref(h), C.byref(sdr_corr))),
        ("gnsscorr_sdr_fe_create", lambda h: L.gnsscorr_sdr_fe_create(C.byref(h), 0)),
    ]


def test_valid_configuration_answers_no_hip_device(gc, L):
    for name, create in _good(gc):
        h = C.c_void_p(0xdead)
        assert create(h) == ENODEV, name
        assert _last(L) == name + ": no HIP device"
        assert not h.value, name                       # *out is cleared before the device checks


def test_bad_configuration_is_refused_before_the_device_checks(gc, L):
    """Each answers GNSSCORR_EINVAL, not GNSSCORR_ENODEV, and leaves its own text."""
    h = C.c_void_p()

    def refused(rc, text):
        assert rc == EINVAL, text
        assert _last(L) == text

    cfg = gc.TrackCfg(0, gc.IF_IQ, 0, 4096, 16.368e6, 0.0)
    assert L.gnsscorr_track_create(C.byref(h), C.byref(cfg)) == EINVAL
    assert _last(L).startswith("gnsscorr_track_create: bad config (n_channels>=1, 1<=max_nsamp<=")
    assert _last(L).endswith(", iq = GNSSCORR_IF_* flags)")
    cfg = gc.TrackCfg(1, 4, 0, 4096, 16.368e6, 0.0)     # a flag bit the library does not know
    assert L.gnsscorr_track_create(C.byref(h), C.byref(cfg)) == EINVAL
    assert _last(L).startswith("gnsscorr_track_create: bad config")

    cfg = gc.AcqCfg(16.368e6, 64, 0, 0, 1, 1, gc.ACQ_F64)
    refused(L.gnsscorr_acq_create(C.byref(h), C.byref(cfg)), "gnsscorr_acq_create: bad config")
    cfg = gc.AcqCfg(16.368e6, 64, 0, 1, 1, 1, 7)
    refused(L.gnsscorr_acq_create(C.byref(h), C.byref(cfg)), "gnsscorr_acq_create: bad config")
    cfg = gc.AcqCfg(16.368e6, 64, 0, 1, 1, 1, gc.ACQ_F32)
    refused(L.gnsscorr_acq_create(C.byref(h), C.byref(cfg)),
            "gnsscorr_acq_create: the fp32 path needs n_samples 16368 (got 64)")
    cfg = gc.AcqCfg(16.368e6, 63, 0, 1, 1, 1, gc.ACQ_F64)
    refused(L.gnsscorr_acq_create(C.byref(h), C.byref(cfg)),
            "gnsscorr_acq_create: n_samples 63 outside the fp64 range [64, 524288]")

    cfg = gc.sgt_cfg(0, codeLength=511)
    refused(L.gnsscorr_sgt_create(C.byref(h), C.byref(cfg)),
            "sgt: bad config (system 0/1, file_type 1/2, code_length 1023/511, "
            "0<=dll_spacing<1, variants 0/1)")
    cfg = gc.e1t_cfg(codeLength=1023)
    refused(L.gnsscorr_e1t_create(C.byref(h), C.byref(cfg)),
            "e1t: bad config (file_type 1/2, code_length 4092, meandr_length 8184, "
            "0<=dll_spacing<1, 0<=sll_spacing<1, positive rates)")
    refused(L.gnsscorr_sdr_fe_create(None, 0), "gnsscorr_sdr_fe_create: null out")

    # the two GPS-SDR creates refuse a null configuration without a text of their own:
    # the last error stays what it was
    before = _last(L)
    assert L.gnsscorr_sdr_acq_create(C.byref(h), None) == EINVAL
    assert L.gnsscorr_sdr_corr_create(C.byref(h), None) == EINVAL
    assert L.gnsscorr_sdr_acq_create(None, C.byref(gc.SdrAcqCfg(38400.0, 0, 0))) == EINVAL
    assert L.gnsscorr_sdr_corr_create(None, C.byref(gc.SdrCorrCfg(0, 0))) == EINVAL
    assert _last(L) == before


def test_a_bad_device_index_is_seen_after_the_configuration(gc, L):
    """device = -1 with a valid configuration reaches the device checks (no device here),
    with a bad configuration it does not."""
    h = C.c_void_p()
    cfg = gc.sgt_cfg(0, device=-1)
    assert L.gnsscorr_sgt_create(C.byref(h), C.byref(cfg)) == ENODEV
    cfg = gc.sgt_cfg(0, device=-1, codeLength=511)
    assert L.gnsscorr_sgt_create(C.byref(h), C.byref(cfg)) == EINVAL
    assert _last(L).startswith("sgt: bad config")
