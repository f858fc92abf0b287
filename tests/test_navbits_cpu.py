"""CPU: the two restatements of the Scilab receiver's frame synchronisation and bit
extraction for GPS L1 C/A, GLONASS L1OF and BeiDou B1I (tests/navbits_scenarios.py) agree on
every scene tests/test_navbits_gpu.py runs on the device, the planted positions are what the
literal transcription finds, and the device's patterns are the files' vectors reversed."""
import numpy as np
import pytest

import navbits_scenarios as S

FAST = {"gps": (S.gps_frames_fast, dict(search_start=S.GPS_START)),
        "gps_long": (S.gps_frames_fast, {}),
        "glo": (S.glo_strings_fast, {}), "glo_short": (S.glo_strings_fast, {}),
        "b1": (S.b1_subframes_fast, {}), "b1_short": (S.b1_subframes_fast, {})}
SCENES = {"gps": S.gps_scene, "gps_long": S.gps_long_scene, "glo": S.glo_scene,
          "glo_short": S.glo_short_scene, "b1": S.b1_scene, "b1_short": S.b1_short_scene}


def test_patterns_are_the_files_vectors_reversed():
    assert S.GPS_PATTERN.tolist() == S.GPS_PREAMBLE_MS[::-1].tolist() and len(S.GPS_PATTERN) == 160
    assert S.GLO_PATTERN.tolist() == S.GLO_TM_LONG[::-1].tolist() and len(S.GLO_PATTERN) == 300
    assert S.B1_PATTERN.tolist() == S.B1_PREAMBLE_LONG[::-1].tolist() and len(S.B1_PATTERN) == 220
    # the search's preamble and secondary code are the decoder's, written backwards
    assert S.B1_SEARCH_PREAMBLE[::-1].tolist() == S.B1_PREAMBLE.tolist()
    assert S.B1_SEARCH_SECONDARY[::-1].tolist() == S.B1_SECONDARY.tolist()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_literal_equals_fast_and_finds_what_was_planted(name):
    x, firsts, counts = SCENES[name]()
    want = S.literal_results(name)
    fast, kw = FAST[name]
    per = 1 if name.startswith("gps") else None
    for ch in range(len(x)):
        first, bits = want[ch]
        assert first == firsts[ch], (name, ch)
        assert (bits.size if per else len(bits)) == counts[ch], (name, ch)
        f_first, f_bits = fast(x[ch], **kw)
        assert f_first == first and f_bits.tobytes() == bits.tobytes(), (name, ch)


def test_scene_properties():
    """what the scenes are built to show is in the literal results"""
    gps = S.literal_results("gps")
    b = gps[2][1]
    assert b[30 * 3 + 7] == 2 and b[30 * 5 + 29] == 2          # the two ties
    assert b[30 * 12 + 3] == 2                                 # [1e16, 1, -1e16]: 0 in order
    x = S.gps_scene()[0][2]
    g = x[S._bit_span(700, 12, 3)]
    assert (g[0] + g[2]) + g[1] == 1.0                         # ... and 1 in another order
    g = x[S._bit_span(700, 13, 3)]
    pairs = g[0::2] + g[1::2]                                  # neighbours first: 0
    assert S.sums20_literal(np.concatenate([pairs, np.zeros(10)]))[0] == 0.0
    assert S.sums20_literal(g)[0] == 1.0 and b[30 * 13 + 3] != 2
    hits = S.convol_hits_literal(S.GPS_PREAMBLE_MS, S.gps_scene()[0][0], S.GPS_START, 153)
    assert 300 in hits and 6300 not in hits                    # the lone preamble ...
    b = S.sign(S.sums20_literal(S.gps_scene()[0][0][260:1500]))  # ... whose two words pass parity
    assert S.nav_party_chk_literal(b[0:32]) != 0 and S.nav_party_chk_literal(b[30:62]) != 0
    hits = S.convol_hits_literal(S.GPS_PREAMBLE_MS, S.gps_scene()[0][1], S.GPS_START, 153)
    assert 400 in hits and 6400 in hits                        # the decoy pair, refused by parity
    glo = S.literal_results("glo")
    assert np.flatnonzero(glo[0][1][2] == 2).tolist() == [83 - 40, 84 - 40]
    assert glo[1][1].tobytes() == glo[2][1].tobytes()          # inverted: the same bits
    assert (glo[1][1] <= 1).all()
    b1 = S.literal_results("b1")
    x = S.b1_scene()[0][0]
    y = S.sign((S.sign(x[6000:12000]).reshape(300, 20) * S.B1_SECONDARY).sum(axis=1))
    assert np.sum(y[:11] * S.B1_PREAMBLE) == 0 and y[0] == 0
    assert b1[0][1][1][:15].tolist() == S.half_bits(y[11:26], True).tolist()   # not negated


def test_threshold_edges_literal():
    x, y = S.edge_scene()
    r = [S.pattern_r_fast(c, S.GPS_PATTERN)[321] for c in x]
    assert r == [157, 153, 154, 152]
    got = [321 in S.convol_hits_literal(S.GPS_PREAMBLE_MS, c, 0, 153) for c in x]
    assert got == [True, False, True, False]
    assert S.pattern_r_fast(y[0], S.GLO_PATTERN)[705] == 295
    assert S.pattern_r_fast(y[1], S.GLO_PATTERN)[710] == 290
    assert 705 in S.convol_hits_literal(S.GLO_TM_LONG, y[0], 0, 290)
    assert 710 not in S.convol_hits_literal(S.GLO_TM_LONG, y[1], 0, 290)


@pytest.mark.parametrize("T", [1, 65, 300])
def test_primitive_literal_equals_fast(T):
    for n in S.prim_epochs(T):
        if n < 1:
            continue
        pattern, x = S.prim_case(T, n, 3)
        for c in x:
            a = S.convol_hits_literal(pattern[::-1], c, 0, S.prim_threshold(T))
            b = S.pattern_hits_fast(c, pattern, S.prim_threshold(T))
            assert a.tolist() == b.tolist(), (T, n)


def test_parity_encoder_round_trip():
    """words made by gps_encode_word pass navPartyChk in either polarity, for both D30*"""
    rng = np.random.default_rng(5)
    for d29s in (0, 1):
        for d30s in (0, 1):
            w = S.gps_encode_word(rng.integers(0, 2, 24), d29s, d30s)
            s = 2 * np.concatenate([[d29s, d30s], w]) - 1
            assert S.nav_party_chk_literal(s) != 0 and S.nav_party_chk_literal(-s) != 0
            s[9] = -s[9]
            assert S.nav_party_chk_literal(s) == 0
