"""CPU: the Galileo E1B host pieces -- gnsscorr_sample_boc_code against a numpy
restatement of GALILEO/E1/include/makeE1BCodesTable.sci:56-78, the E1B chip fixture,
the E1 frequency grid, and the new acquisition entry points in the header, the
library and the ctypes mirror."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import e1b_scenarios as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnsscorr_acq_set_zero_padded", "gnsscorr_acq_set_codes_padded",
       "gnsscorr_sample_boc_code")


@pytest.fixture(scope="module")
def e1b():
    return np.load(os.path.join(ROOT, "tests", "golden", "e1b_codes.npz"))


def test_fixture_shape(e1b):
    codes = e1b["codes"]
    assert codes.shape == (3, 4092) and codes.dtype == np.int8
    assert set(np.unique(codes)) == {-1, 1}
    assert list(e1b["prns"]) == [11, 12, 19]
    assert len({c.tobytes() for c in codes}) == 3


@pytest.mark.parametrize("fs,n", [(16.0e6, 64000), (4.092e6, 16368)])
def test_sample_boc_code_matches_restatement(gc, e1b, fs, n):
    for chips in e1b["codes"]:
        got = gc.sample_boc_code(chips, 1.023e6, fs, n)
        want = E.sample_boc(chips, 1.023e6, fs, n)
        assert got.dtype == np.int8 and np.array_equal(got, want)
        # the last-index quirk (makeE1BCodesTable.sci:73): half-chip index codeLength,
        # i.e. the second half of chip 2046, not the end of the code
        assert got[-1] == -chips[4092 // 2 - 1]
    # it is a quirk: on a code whose last chip differs from chip 2046, the natural last
    # index, 2 * codeLength (the second half of the last chip), gives the other sample
    c = e1b["codes"][0].copy()
    c[-1] = -c[4092 // 2 - 1]
    got = gc.sample_boc_code(c, 1.023e6, fs, n)
    assert got[-1] == -c[4092 // 2 - 1] and got[-1] != -c[-1]
    assert np.array_equal(got, E.sample_boc(c, 1.023e6, fs, n))


def test_sample_boc_code_is_meandered_chips(gc, e1b):
    """At 16 Msps a chip is 15.6 samples: away from the half-chip edges (where the
    rule's fp64 ceil decides) sample k is +chip in the first half of its chip and
    -chip in the second."""
    chips = e1b["codes"][1]
    got = gc.sample_boc_code(chips, 1.023e6, 16.0e6, 64000)
    pos = (np.arange(1, 64000) * 1.023e6 / 16.0e6) * 2          # in half chips, k = 1..n-1
    clear = np.abs(pos - np.rint(pos)) > 1e-6
    hc = np.ceil(pos).astype(np.int64) - 1
    want = chips[hc // 2] * np.where(hc % 2 == 0, 1, -1)
    assert np.array_equal(got[:-1][clear], want[clear]) and clear.sum() > 63000


def test_sample_boc_code_rejects_bad_arguments(gc):
    out = np.empty(8, np.int8)
    chips = np.ones(4, np.int8)
    L = gc.lib()
    assert L.gnsscorr_sample_boc_code(None, 4, 1.0, 2.0, 8, out.ctypes.data) == -1
    assert L.gnsscorr_sample_boc_code(chips.ctypes.data, 0, 1.0, 2.0, 8, out.ctypes.data) == -1
    assert L.gnsscorr_sample_boc_code(chips.ctypes.data, 4, 1.0, 2.0, 0, out.ctypes.data) == -1


def test_e1b_bins(gc):
    """acquisition.sci:61, 94-96 with initSettings.sci's IF 2.42 MHz, 14 kHz, 4 ms."""
    f = gc.e1b_bins(2.42e6, 14, 4)
    assert len(f) == 113
    assert f[0] == 2.42e6 - 7000.0 and f[-1] == 2.42e6 + 7000.0
    assert np.allclose(np.diff(f), 125.0, rtol=0, atol=1e-9)


def test_new_symbols_in_header_library_and_mirror(gc):
    hdr = open(os.path.join(ROOT, "include", "gnsscorr.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = C.CDLL(gc.LIB_PATH)
    gc.lib()
    for name in NEW:
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, flags=re.M), name
        assert hasattr(L, name), name
        assert name in gc.EXPORTED_FUNCTIONS, name
        assert getattr(gc.lib(), name).argtypes is not None, name
    assert gc.lib().gnsscorr_acq_set_zero_padded.argtypes == [C.c_void_p, C.c_int]
    assert gc.lib().gnsscorr_acq_set_codes_padded.argtypes == [C.c_void_p, C.c_int, C.c_void_p,
                                                              C.c_int]
    for meth in ("set_zero_padded", "set_codes_padded"):
        assert callable(getattr(gc.AcqCtx, meth))
