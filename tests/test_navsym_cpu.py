"""CPU: the restated symbol chain of Galileo E1B and GLONASS L3OC (tests/navsym_scenarios.py)
and the host-only encoder of the library.

The literal transcription of the Scilab decoder is the oracle of tests/test_navsym_gpu.py;
here it is held equal, bit for bit, to the independent index-array implementation, on cases
that are shown not to be vacuous: the literal decoder itself reports, per decision, how many
window-start states survive the elimination and how many of them share the smallest metric.

Where the non-vacuity bound (>= 8 decisions with more than one survivor, >= 4 with a tied
minimum) is asserted: the noisy cases with L >= 43.  With L <= 8 the walk back through 41
steps, most of them zero padding, always ends in a single state, so no seed can meet it
there; and on random doubles two path metrics are never equal, so the soft "doubles" cases
assert the survivors alone.
"""
import numpy as np
import pytest

import navsym_scenarios as S

LENGTHS = (1, 2, 8, 43, 60, 120)
RATES = {"clean": 0.0, "flip03": 0.03, "flip15": 0.15, "random": 0.0}
# seeds (of default_rng([L, seed])) at which the literal decoder meets the bound above
HARD_SEEDS = {(43, "flip03"): 2, (43, "flip15"): 0, (43, "random"): 1,
              (60, "flip03"): 65, (60, "flip15"): 0, (60, "random"): 0,
              (120, "flip03"): 55, (120, "flip15"): 0, (120, "random"): 0}
SOFT_SEEDS = {(43, True): 1, (43, False): 0, (60, True): 5, (60, False): 0,
              (120, True): 0, (120, False): 0}


def _counts(survivors, ties):
    return int((survivors > 1).sum()), int((ties > 1).sum())


@pytest.mark.parametrize("kind", list(RATES))
@pytest.mark.parametrize("L", LENGTHS)
def test_hard_literal_equals_fast(L, kind):
    rng = np.random.default_rng([L, HARD_SEEDS.get((L, kind), 0)])
    _, code = S.noisy_code(rng, L, RATES[kind], kind == "random")
    bits, survivors, ties = S.viterbi_literal(code, False)
    assert bits.tobytes() == S.viterbi_fast(code, False).tobytes()
    if (L, kind) in HARD_SEEDS:
        multi, tied = _counts(survivors, ties)
        print(f"L {L} {kind}: {multi} decisions with several survivors, {tied} with a tie")
        assert multi >= 8 and tied >= 4


@pytest.mark.parametrize("grid", [True, False], ids=["grid8", "doubles"])
@pytest.mark.parametrize("L", LENGTHS)
def test_soft_literal_equals_fast(L, grid):
    rng = np.random.default_rng([L, SOFT_SEEDS.get((L, grid), 0), 7])
    _, code = S.soft_code(rng, L, grid)
    bits, survivors, ties = S.viterbi_literal(code, True)
    assert bits.tobytes() == S.viterbi_fast(code, True).tobytes()
    if (L, grid) in SOFT_SEEDS:
        multi, tied = _counts(survivors, ties)
        print(f"L {L} grid {grid}: {multi} with several survivors, {tied} with a tie")
        assert multi >= 8 and (tied >= 4 or not grid)


def test_hard_symbols_as_soft_input_decode_alike():
    rng = np.random.default_rng([60, 0])
    _, code = S.noisy_code(rng, 60, 0.15)
    assert (S.viterbi_literal(code.astype(np.float64), True)[0].tobytes()
            == S.viterbi_literal(code, False)[0].tobytes())


def test_the_trellis_is_not_flushed():
    """Quirk 2: with six zero tail bits a clean message decodes exactly; without them the last
    six bits can be wrong (the seed is pinned: bits 56, 58 and 59 of 60)."""
    for seed in range(5):
        rng = np.random.default_rng([120, seed, 2])
        msg, code = S.noisy_code(rng, 120, zero_tail=True)
        assert S.viterbi_literal(code)[0].tobytes() == msg.tobytes()
    msg = np.random.default_rng([60, 1, 1]).integers(0, 2, 60).astype(np.uint8)
    bits = S.viterbi_literal(S.conv_encode(msg)[:120])[0]
    wrong = np.nonzero(bits != msg)[0]
    assert wrong.tolist() == [56, 58, 59]
    flushed = S.viterbi_literal(S.conv_encode(msg))[0]       # the encoder's own six tail steps
    assert flushed[:60].tobytes() == msg.tobytes()


@pytest.mark.parametrize("n", [1, 7, 120])
def test_library_encoder_equals_the_restated_encoder(gc, n):
    msg = np.random.default_rng(n).integers(0, 2, n).astype(np.uint8)
    want = S.conv_encode(msg)
    assert want.size == (n + 6) * 2
    assert gc.nav_conv_encode(msg).tobytes() == want.tobytes()
    assert gc.NavCtx.conv_encode(msg).tobytes() == want.tobytes()


def test_encoder_and_field_helper_refuse_bad_arguments(gc):
    with pytest.raises(gc.GnssCorrError):
        gc.nav_conv_encode(np.zeros(0, np.uint8))
    assert gc.epoch_field(gc.E1T_EPOCH, "I_P_P") == (16, 176)
    assert gc.epoch_field(gc.L3T_EPOCH, "I_P") == (8, 160)
    assert gc.epoch_field(gc.L3T_EPOCH, "Q_P2") == (80, 160)
    with pytest.raises(ValueError):
        gc.epoch_field(gc.L3T_EPOCH, "blksize")
    with pytest.raises(ValueError):
        gc.epoch_field(gc.L3T_EPOCH, "I_P_P")


@pytest.mark.parametrize("polarity", [1, -1])
@pytest.mark.parametrize("start", [0, 37, 999])
def test_e1_restatement_recovers_the_planted_pages(start, polarity):
    rng = np.random.default_rng([start, polarity + 1])
    series, msgs = S.e1_series(rng, 3200, start, polarity=polarity, n_zeros=12,
                               zero_in_sync=True)
    assert (series == 0).sum() >= 12
    first, pages = S.e1_pages(series)
    assert first == start
    assert len(pages) == (3200 - start) // 1000
    assert pages.tobytes() == msgs[:len(pages)].tobytes()     # the messages end in six zeros
    lit = S.decode_gll_data(series[start:start + 1000], lambda c: S.viterbi_literal(c)[0])
    assert lit.tobytes() == pages[0].tobytes()


def test_e1_restatement_without_a_second_sync_finds_nothing():
    rng = np.random.default_rng(8)
    series, _ = S.e1_series(rng, 1030, 0)                      # one pattern, the next one cut
    assert S.e1_pages(series)[0] == -1
    assert S.e1_pages(1500.0 * rng.standard_normal(3200))[0] == -1


@pytest.mark.parametrize("start", [0, 7])
def test_l3_restatement_recovers_start_message_and_mark(start):
    rng = np.random.default_rng([start, 3])
    pilot, data, msg = S.l3_series(rng, 2500, start, mark_at=100, n_zeros=10)
    assert (data == 0).sum() == 10
    got_start, bits, marks = S.l3_data_decode(pilot, data)
    assert got_start == start
    assert len(bits) == (2500 - start) // 10
    # the stream is cut, not flushed: an error event of the unflushed tail can begin a few
    # bits before the last six (seen: bit 243 of 250), so the tail is left out generously
    assert bits[:-16].tobytes() == msg[:len(bits) - 16].tobytes()
    assert 100 in marks
    assert S.l3_data_decode(np.ones(2500), data)[0] == -1      # the overlay is never met


def test_an_inverted_l3_stream_stays_inverted():
    """Quirk 3: the -20 comparison never fires, so the decoder sees the complemented code
    word; both generators have odd weight, so once six true bits are in the register that is
    the code word of the complemented message."""
    rng = np.random.default_rng(21)
    pilot, data, msg = S.l3_series(rng, 2500, 7, mark_at=100)
    start, bits, marks = S.l3_data_decode(-pilot, -data)
    upright = S.l3_data_decode(pilot, data)
    assert start == upright[0] == 7
    assert bits[8:-16].tobytes() == (1 - msg[8:len(bits) - 16]).tobytes()
    assert bits[8:-16].tobytes() == (1 - upright[1][8:-16]).tobytes()
    assert 100 in marks                                        # |.| == 20 either way
