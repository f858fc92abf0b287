"""CPU: the host side of int16 IF records: the GNSSCORR_IF_INT16 flag and iq_flags, the
byte view of an int16 array, the three *_set_record_format setters in the library, the
header and the Python binding, and what they refuse without a device.  The checks that
need a context (a bad fmt on a live context, INT16 | PACKED2, INT16 on an F32 context,
misaligned records) are made before any launch but after create, which needs a device:
they are in tests/test_if16_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTERS = tuple(f"gnsscorr_{fam}_set_record_format" for fam in ("sgt", "e1t", "l3t"))
EINVAL = -1


def test_iq_flags_values(gc):
    assert (gc.IF_IQ, gc.IF_PACKED2, gc.IF_INT16) == (1, 2, 4)
    assert gc.iq_flags(False) == 0 and gc.iq_flags(True) == 1
    assert gc.iq_flags(True, packed=True) == 3 and gc.iq_flags(False, True) == 2
    assert gc.iq_flags(True, int16=True) == 5 and gc.iq_flags(False, int16=True) == 4
    assert gc.iq_flags(True, False, True) == 5
    assert gc.iq_flags(5) == 5 and gc.iq_flags(1, int16=True) == 5
    hdr = open(os.path.join(ROOT, "include", "gnsscorr.h")).read()
    assert re.search(r"^#define GNSSCORR_IF_INT16\s+4$", hdr, flags=re.M)


def test_if_bytes_views_an_int16_record_as_its_little_endian_bytes(gc):
    a = np.array([0x00FF, -256, 0x7FFF, -32768, 1, -1], np.int16)
    b = gc._if_bytes(a, gc.IF_INT16)
    assert b.dtype == np.int8 and b.size == 2 * a.size
    assert b.view(np.uint8).tolist() == [0xFF, 0x00, 0x00, 0xFF, 0xFF, 0x7F, 0x00, 0x80,
                                          0x01, 0x00, 0xFF, 0xFF]
    assert np.array_equal(b.view("<i2"), a)
    # a 2-d (samples, 2) array, as SdrFeCtx.gn3s returns, and a big-endian one
    assert np.array_equal(gc._if_bytes(a.reshape(3, 2), gc.IF_IQ | gc.IF_INT16), b)
    assert np.array_equal(gc._if_bytes(a.astype(">i2"), gc.IF_INT16), b)
    assert np.array_equal(gc._if_bytes(b.view(np.uint8), gc.IF_INT16), b)   # its raw bytes
    # an array of another type holds no int16 elements: refused, not reinterpreted
    for other in (b, np.zeros(4, np.int32), np.zeros(4, np.float64)):
        with pytest.raises(gc.GnssCorrError, match="int16"):
            gc._if_bytes(other, gc.IF_IQ | gc.IF_INT16)
    # without the flag, int8 and uint8 arrays as before
    i8 = np.array([-3, 1, 127, -128], np.int8)
    assert np.array_equal(gc._if_bytes(i8), i8)
    assert np.array_equal(gc._if_bytes(i8.view(np.uint8)), i8)


def test_record_format_setters_are_exported_declared_and_bound(gc):
    L = C.CDLL(gc.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "gnsscorr.h")).read()
    table = gc._sig_table()
    for name in SETTERS:
        assert hasattr(L, name), name
        assert re.search(r"^int %s\(" % name, hdr, flags=re.M), name
        assert name in table and name in gc.EXPORTED_FUNCTIONS, name
        res, args = table[name]
        assert res is C.c_int and args == [C.c_void_p, C.c_int]
    for cls in (gc.SgtCtx, gc.E1tCtx, gc.L3tCtx):
        assert callable(getattr(cls, "set_format")) and callable(getattr(cls, "set_packed"))
        assert cls.RECORD_FORMATS == {"int8": 0, "packed2": 1, "int16": 2}


def test_a_null_context_is_refused_without_a_device(gc):
    for name in SETTERS:
        fn = getattr(gc.lib(), name)
        for fmt in (0, 1, 2, 3, -1):
            assert fn(None, fmt) == EINVAL
        assert b"set_record_format" in gc.lib().gnsscorr_last_error()
