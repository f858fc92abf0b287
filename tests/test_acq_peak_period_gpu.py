"""GPU: the second-peak rule of GLONASS/L3/acquisition.sci:134-153 in a zero-padded search
(gnsscorr_acq_set_peak_period) against the restatement's 1-based codePhaseRange
(tests/l3_scenarios.py), on both generic engines and in both search modes.

Smallest shape: L = 2000, keep = 1000, period S = 200, 2 Msps, noise-free planted copies
of a random +-1 code (a copy placed from sample k correlates at lag k, as in
tests/acq_window_scenes.py).  Each case plants the peak (amplitude 6) on one argmax value
a at which the rule changes branch or reaches an edge -- s, s + 1, S - s - 1, S - s, S,
keep - 1, for s = spc = 2 and 7 -- and two weaker copies:
  amplitude 3 at (a + S) % keep, a candidate of the window circular in keep and not of
              the L3 range: with the period off it is `second`;
  amplitude 2 inside both sets (for a = s on index S, the top edge of the reference's own
              range): with the period on it is `second`.
Held to the project's fp64 bar (test_acq_gpu.check_rows).
"""
import numpy as np
import pytest

import e1b_scenarios as E
import l3_scenarios as L3
from test_acq_gpu import check_rows

pytestmark = pytest.mark.gpu
FS = 2.0e6
L, KEEP, S = 2000, 1000, 200
FREQS = np.array([-500.0, 0.0, 500.0])
GF = np.arange(3)[None, :]
EINVAL = -1


def _code():
    rng = np.random.default_rng(0x13C0DE)
    return (2 * rng.integers(0, 2, KEEP) - 1).astype(np.int8)[None, :]


def cases():
    return [(a, s) for s in (2, 7) for a in (s, s + 1, S - s - 1, S - s, S, KEEP - 1)]


def agree_lag(a, s):
    if a == s:
        return S
    return a - s - 10 if a - s - 10 >= 0 else a + s + 10


def scene_if(a, s):
    c = _code()[0].astype(np.int64)
    x = np.zeros(L, np.int64)
    for amp, k in ((6, a), (3, (a + S) % KEEP), (2, agree_lag(a, s))):
        x[k:k + KEEP] += amp * c
    out = np.zeros(2 * L, np.int8)
    out[0::2] = x
    return out


_ref = {}


def reference(a, s, nc):
    """(period rule, circular rule) restatements of one case, computed once."""
    if (a, s, nc) not in _ref:
        IF = scene_if(a, s)
        off = E.acquire(IF, FS, _code(), L, KEEP, FREQS, GF, spc=s, n_blocks=1, noncoherent=nc)[:2]
        on = E.acquire(IF, FS, _code(), L, KEEP, FREQS, GF, spc=s, n_blocks=1, noncoherent=nc)[:2]
        on = L3.apply_period_rule(on[0], on[1], s, S)
        # decidable: the L3 candidates' maximum clear of their runner-up, in every row
        for b, rr in enumerate(on[1][0]):
            rng = L3.code_phase_range_1b(rr["argmax"] + 1, S, s)
            v = np.sort(on[0][0]["results"][b][rng[rng <= KEEP] - 1])
            assert v[-1] == rr["second"] and v[-1] > v[-2] * (1 + 1e-6), (a, s, b)
        _ref[(a, s, nc)] = (on, off)
    return _ref[(a, s, nc)]


def _ctx(gpu):
    ctx = gpu.AcqCtx(FS, L, max_freqs=4, max_blocks=1, max_codes=1)
    ctx.set_zero_padded(KEEP)
    ctx.set_codes_padded(_code())
    return ctx


@pytest.mark.parametrize("nc", [False, True], ids=["best", "noncoherent"])
@pytest.mark.parametrize("engine", ["mixed", "bluestein"])
def test_second_peak_follows_the_period_rule(gpu, engine, nc, monkeypatch):
    monkeypatch.setenv("GNSSCORR_ACQ_BLUESTEIN", "1" if engine == "bluestein" else "0")
    mode = gpu.ACQ_NONCOHERENT if nc else gpu.ACQ_BEST_OF_BLOCKS
    ctx = _ctx(gpu)
    for a, s in cases():
        (ref, ref_rows), (off, off_rows) = reference(a, s, nc)
        IF = scene_if(a, s)
        assert ref_rows[0][1]["argmax"] == a and ref[0]["bin"] == 1
        # the restatements themselves disagree where the test says they do
        pk = ref[0]["peak"]
        assert abs(off[0]["second"] / pk - 0.25) < 0.05 and abs(ref[0]["second"] / pk - 1 / 9) < 0.05
        ctx.set_peak_period(S)
        res, rows = ctx.search(IF, 1, FREQS, [0], GF, spc=s, mode=mode)
        check_rows(res, rows, ref, ref_rows, True, label=f"period-{engine}-{a}-{s}")
        assert res[0]["code_phase"] == a + 1 and rows[0, 1]["argmax"] == a
        ctx.set_peak_period(0)
        res0, rows0 = ctx.search(IF, 1, FREQS, [0], GF, spc=s, mode=mode)
        check_rows(res0, rows0, off, off_rows, True, label=f"period-off-{engine}-{a}-{s}")
        assert res0[0]["second"] > 1.5 * res[0]["second"]          # fails without the feature
        assert rows0[0, 1]["second"] != rows[0, 1]["second"]
        assert res0[0]["peak"] == res[0]["peak"] and res0[0]["code_phase"] == res[0]["code_phase"]


@pytest.mark.parametrize("engine", ["mixed", "bluestein"])
def test_period_off_again_is_a_fresh_padded_context(gpu, engine, monkeypatch):
    monkeypatch.setenv("GNSSCORR_ACQ_BLUESTEIN", "1" if engine == "bluestein" else "0")
    used, fresh = _ctx(gpu), _ctx(gpu)
    IF = scene_if(S, 7)
    used.set_peak_period(S)
    used.search(IF, 1, FREQS, [0], GF, spc=7)
    used.set_peak_period(0)
    for mode in (gpu.ACQ_BEST_OF_BLOCKS, gpu.ACQ_NONCOHERENT):
        a = used.search(IF, 1, FREQS, [0], GF, spc=7, mode=mode)
        b = fresh.search(IF, 1, FREQS, [0], GF, spc=7, mode=mode)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    # set_zero_padded(0) clears the period: on again, the window is circular in keep
    used.set_peak_period(S)
    used.set_zero_padded(0)
    used.set_zero_padded(KEEP)
    a = used.search(IF, 1, FREQS, [0], GF, spc=7)
    b = fresh.search(IF, 1, FREQS, [0], GF, spc=7)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_refusals(gpu):
    lib = gpu.lib()

    def refused(rc, word):
        assert rc == EINVAL
        assert word in lib.gnsscorr_last_error().decode()

    c = gpu.AcqCtx(FS, L, max_freqs=4, max_blocks=1, max_codes=1)
    refused(lib.gnsscorr_acq_set_peak_period(c.h, S), "zero-padded")      # mode off
    assert lib.gnsscorr_acq_set_peak_period(c.h, 0) == 0
    c.set_zero_padded(KEEP)
    refused(lib.gnsscorr_acq_set_peak_period(c.h, KEEP + 1), "keep")
    refused(lib.gnsscorr_acq_set_peak_period(c.h, -1), "period")
    c.set_peak_period(KEEP)                                             # period == keep is fine
    refused(lib.gnsscorr_acq_set_zero_padded(c.h, KEEP - 1), "peak period")  # keep below it
    c.set_peak_period(S)
    c.set_zero_padded(KEEP - 1)                                         # above the period: fine
    c.set_zero_padded(KEEP)
    c.set_codes_padded(_code())
    IF = scene_if(S, 7)
    for spc in (S // 2, S // 2 + 1):                                    # period <= 2 spc
        with pytest.raises(gpu.GnssCorrError, match="2 spc < period"):
            c.search(IF, 1, FREQS, [0], GF, spc=spc)
    res, _ = c.search(IF, 1, FREQS, [0], GF, spc=S // 2 - 1)            # 2 spc < period
    assert res[0]["code_phase"] == S + 1
