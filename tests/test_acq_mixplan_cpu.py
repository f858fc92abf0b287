"""CPU: the pass plan of the generic fp64 acquisition engine (csrc/acq64_gen.hip mix_factor /
mix_order_padded, read through gnsscorr_acq_mix_plan) and the reference floor of the
per-radix GPU tier (tests/test_acq_radix_gpu.py).

1. The plan at every length of acq_radix_scenes.TABLE and at the lengths the other
   acquisition tests run: the radices multiply to N and are compiled ones, the unpadded
   order has the smallest first and the second smallest last, the padded order ends on the
   smallest even radix.  The ordering rule is not restated here: the orders come from the
   library.
2. Coverage, the point of the table: over its lengths every compiled radix runs as the
   first pass (mx_pass MODE 1 of a search, MODE 5 of zero-extended codes), as a middle
   pass (MODE 0), as the last pass (MODE 2) and as the last pass of the padded order
   (MODE 3; every even one with an even N: MODE 4 at keep = N/2).
3. The floor: acq_oracle.power_rows against a long-double direct DFT of the same chain
   (acq_radix_scenes.power_rows_longdouble) at the rows the GPU tier compares.  Measured
   1.4e-15 .. 2.8e-15 of the row maximum over the 20 lengths; held below 1e-14, so of the
   GPU tier's 1e-12 bar at most a hundredth is the reference's own error.
"""
import math

import numpy as np
import pytest

import acq_radix_scenes as S

OTHER_LENGTHS = (5000, 38192, 16368, 16100, 64, 1 << 19)


@pytest.mark.parametrize("n", S.LENGTHS + OTHER_LENGTHS)
def test_plan_properties(gc, n):
    r, rp = gc.acq_mix_plan(n)
    assert len(r) >= 2 and len(rp) == len(r)
    assert math.prod(r) == n and math.prod(rp) == n
    assert set(r) <= set(S.RADICES) and sorted(rp) == sorted(r)
    s = sorted(r)
    assert r[0] == s[0] and r[-1] == s[1]                  # the two fused passes: fewest registers
    assert sorted(r[1:-1]) == s[2:]
    if n % 2 == 0:
        assert rp[-1] == min(x for x in r if x % 2 == 0)
    else:
        assert rp == r
    if n in S.TABLE:
        assert (tuple(r), tuple(rp)) == S.TABLE[n], "re-pick the length: the table row is stale"


@pytest.mark.parametrize("n", [4111, 2018, 524287])
def test_no_plan_above_31(gc, n):
    """A prime factor above 31 remains (4111 and 524287 are prime, 2018 = 2 x 1009)."""
    assert gc.acq_mix_plan(n) == ([], [])
    assert gc.lib().gnsscorr_acq_mix_plan(n, None, None, 0) == 0


def test_plan_is_a_pure_host_function(gc, monkeypatch):
    """No environment variable changes the answer (a context's engine switches do not
    reach it), the arrays are optional and cap bounds what is written."""
    want = gc.acq_mix_plan(38192)
    for var in ("GNSSCORR_ACQ_BLUESTEIN", "GNSSCORR_ACQ_GENERIC"):
        monkeypatch.setenv(var, "1")
    monkeypatch.setenv("GNSSCORR_ACQ_MIX4", "0")
    assert gc.acq_mix_plan(38192) == want and len(want[0]) == 4
    L = gc.lib()
    assert L.gnsscorr_acq_mix_plan(38192, None, None, 24) == 4
    r = np.full(4, -1, np.int32)
    assert L.gnsscorr_acq_mix_plan(38192, r.ctypes.data, None, 2) == 4
    assert list(r) == want[0][:2] + [-1, -1]
    for n in (63, 0, -8, (1 << 19) + 16):                  # outside the engine's range
        assert L.gnsscorr_acq_mix_plan(n, None, None, 0) == 0


def test_table_covers_every_radix_in_every_position(gc):
    plans = {n: gc.acq_mix_plan(n) for n in S.LENGTHS}
    first = {r[0] for r, _ in plans.values()}
    middle = {x for r, _ in plans.values() for x in r[1:-1]}
    last = {r[-1] for r, _ in plans.values()}
    last_padded = {rp[-1] for _, rp in plans.values()}
    last_padded_even_n = {rp[-1] for n, (_, rp) in plans.items() if n % 2 == 0}
    every = set(S.RADICES)
    # a plan holds at most one radix 2 and it is the smallest radix: first in the
    # unpadded order, last in the padded one, never a middle pass of either
    assert first == every
    assert middle == every - {2}
    assert last == every - {2}
    assert last_padded == every
    assert last_padded_even_n == {2, 4, 8, 16}
    # the padded order's own first and middle passes (MODE 1 / MODE 0 of a padded search)
    assert {rp[0] for _, rp in plans.values()} >= every - {2, 4, 8}
    assert all(2 not in rp[:-1] for _, rp in plans.values())


@pytest.mark.parametrize("n", S.LENGTHS, ids=S.case_id)
def test_reference_floor(n):
    """acq_oracle.power_rows (numpy fp64 FFTs, fp64 wipe-off argument) against the
    long-double direct DFT with the exact rational phase, at the rows of the GPU tier."""
    worst = 0.0
    exact = S.power_rows_longdouble(n, 0, S.ROW_BINS)
    for ld, b in zip(exact, S.ROW_BINS):
        ref = S.oracle_rows(n, 0, b)
        for blk in range(2):
            err = float(np.abs(ref[blk] - ld[blk]).max() / ld[blk].max())
            worst = max(worst, err)
            assert int(np.argmax(ref[blk])) == int(np.argmax(ld[blk]))
    print(f"[reference floor N={n}] {worst:.3e}")
    assert worst < 1e-14
