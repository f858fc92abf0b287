"""CPU: the host side of packed records in the float trackers: gnsscorr_unpack2 (the
inverse of gnsscorr_pack2) and the presence of the three *_set_packed setters in the
library, the header and the Python binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnsscorr_sgt_set_packed", "gnsscorr_e1t_set_packed", "gnsscorr_l3t_set_packed",
       "gnsscorr_unpack2")
EINVAL = -1


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 4097])
def test_unpack2_inverts_pack2(gc, n):
    lv = np.random.default_rng(n).choice(np.array([-3, -1, 1, 3], np.int8), n)
    packed = gc.pack2(lv)
    assert packed.size == (n + 3) // 4
    got = gc.unpack2(packed, n)
    assert got.dtype == np.int8 and np.array_equal(got, lv)
    # the layout: element e in bits 2(e%4)..2(e%4)+1 of byte e/4, code c is level 2c-3
    e = np.arange(n)
    assert np.array_equal(2 * ((packed[e // 4].astype(np.int16) >> (2 * (e % 4))) & 3) - 3, lv)


def test_unpack2_refuses_bad_arguments(gc):
    L = gc.lib()
    src, dst = np.zeros(4, np.uint8), np.zeros(16, np.int8)
    assert L.gnsscorr_unpack2(None, 4, dst.ctypes.data) == EINVAL
    assert b"gnsscorr_unpack2" in L.gnsscorr_last_error()
    assert L.gnsscorr_unpack2(src.ctypes.data, 4, None) == EINVAL
    assert L.gnsscorr_unpack2(src.ctypes.data, -1, dst.ctypes.data) == EINVAL
    assert L.gnsscorr_unpack2(src.ctypes.data, 0, dst.ctypes.data) == 0
    with pytest.raises(ValueError):
        gc.unpack2(src, 17)                       # 4 bytes hold 16 elements


def test_setters_are_exported_declared_and_bound(gc):
    L = C.CDLL(gc.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "gnsscorr.h")).read()
    table = gc._sig_table()
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(r"^int %s\(" % name, hdr, flags=re.M), name
        assert name in table and name in gc.EXPORTED_FUNCTIONS, name
    for fam in ("sgt", "e1t", "l3t"):
        res, args = table[f"gnsscorr_{fam}_set_packed"]
        assert res is C.c_int and args == [C.c_void_p, C.c_int]
    for cls in (gc.SgtCtx, gc.E1tCtx, gc.L3tCtx):
        assert callable(getattr(cls, "set_packed"))
    # a null context is refused without a device
    assert gc.lib().gnsscorr_sgt_set_packed(None, 1) == EINVAL
    assert gc.lib().gnsscorr_e1t_set_packed(None, 0) == EINVAL
    assert gc.lib().gnsscorr_l3t_set_packed(None, 1) == EINVAL
