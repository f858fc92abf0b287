"""GPU: frame synchronisation and data bits of GPS L1 C/A, GLONASS L1OF and BeiDou B1I
(csrc/navbits.hip) against the literal transcription of the Scilab files
(tests/navbits_scenarios.py).  Every comparison is exact: positions and bits have no
tolerance.  The scenes and their literal results are built once and shared with
tests/test_navbits_cpu.py, which holds the literal and the fast restatement equal on them.
"""
import numpy as np
import pytest

import nav_twin as T
import navbits_scenarios as S

pytestmark = pytest.mark.gpu

PAD = 5              # epochs of padding after every channel: large values, never to be read
MAX_HITS = 4


def _upload_padded(gc, x):
    """the series with PAD epochs of 9e9 after each channel -> (DevBuf, channel stride)"""
    padded = np.full((x.shape[0], x.shape[1] + PAD), 9e9)
    padded[:, :x.shape[1]] = x
    return gc.DevBuf.from_array(padded), padded.strides[0]


def _hits_dev(gc, nav, x, pattern, threshold, first_k=0, max_hits=MAX_HITS):
    n_ch, n_ep = x.shape
    d_x, cs = _upload_padded(gc, x)
    d_first, d_n = (gc.DevBuf.from_array(np.full(n_ch, -7, np.int32)) for _ in range(2))
    d_hits = gc.DevBuf.from_array(np.full(n_ch * max_hits, -7, np.int32))
    nav.pattern_hits_dev(d_x.ptr, 8, cs, n_ep, n_ch, pattern, threshold, first_k, max_hits,
                         d_first.ptr, d_n.ptr, d_hits.ptr)
    nav.sync()
    return (d_first.download(np.int32), d_n.download(np.int32),
            d_hits.download(np.int32).reshape(n_ch, max_hits))


def _check_hits(got, x, vec, threshold, first_k, max_hits, what):
    first, n_hits, hits = got
    for ch in range(len(x)):
        want = S.convol_hits_literal(vec, x[ch], first_k, threshold)
        assert n_hits[ch] == len(want), (what, ch)
        assert first[ch] == (want[0] if len(want) else -1), (what, ch)
        k = min(len(want), max_hits)
        assert hits[ch, :k].tolist() == want[:k].tolist(), (what, ch)
        assert (hits[ch, k:] == -1).all(), (what, ch)
    return n_hits


@pytest.mark.parametrize("T", S.PRIM_T)
def test_pattern_hits_equal_the_files_convol(gpu, T):
    """Every tap count at every series length (shorter than the pattern, one window, a word
    boundary either side, one tile, more than one word of tail) for 1, 3 and 65 channels with
    a padded channel stride; hits start at k mod 64 = 0, 1 and 63 and one is cut off by the
    end; the noise channel gives -1; T = 1 has more hits than max_hits."""
    nav = gpu.NavCtx()
    thr = S.prim_threshold(T)
    seen_many = seen_none = False
    for n_ep in S.prim_epochs(T):
        for n_ch in S.PRIM_CH:
            pattern, x = S.prim_case(T, n_ep, n_ch)
            if n_ep < 1:                                       # T = 1: an empty series is refused
                with pytest.raises(gpu.GnssCorrError):
                    nav.pattern_hits(np.zeros((n_ch, 0)), pattern, thr)
                continue
            got = _hits_dev(gpu, nav, x, pattern, thr)
            n_hits = _check_hits(got, x, pattern[::-1], thr, 0, MAX_HITS, (T, n_ep, n_ch))
            seen_many |= bool((n_hits > MAX_HITS).any())
            seen_none |= bool((n_hits == 0).any())
    assert seen_none or T == 1
    assert seen_many or T > 1


def test_pattern_hits_across_tiles_and_first_k(gpu):
    """20 000 epochs are three tiles of 8192: hits in each tile, one whose window spans a tile
    boundary, and first_k inside the series"""
    rng = np.random.default_rng(8)
    n = 20000
    starts = [[63, 7800, 8191, 8600, 16383, 19705], [5000, 16300], []]
    x = np.stack([S.planted(rng, n, S.GLO_PATTERN, s) for s in starts])
    nav = gpu.NavCtx()
    for first_k in (0, 64, 8101):
        got = _hits_dev(gpu, nav, x, S.GLO_PATTERN, 290, first_k, 8)
        _check_hits(got, x, S.GLO_TM_LONG, 290, first_k, 8, first_k)
    assert got[0].tolist() == [8191, 16300, -1]


def test_threshold_edges_and_a_pattern_cut_off_by_the_end(gpu):
    x, y = S.edge_scene()
    nav = gpu.NavCtx()
    first, n_hits, _ = _hits_dev(gpu, nav, x, S.GPS_PATTERN, 153)
    _check_hits((first, n_hits, _), x, S.GPS_PREAMBLE_MS, 153, 0, MAX_HITS, "gps")
    assert first.tolist() == [321, -1, 321, -1]                # 157, 153, 154, 152
    got = _hits_dev(gpu, nav, y, S.GLO_PATTERN, 290)
    _check_hits(got, y, S.GLO_TM_LONG, 290, 0, MAX_HITS, "glo")
    assert got[0].tolist() == [705, -1]                        # 295 taps there, 290 taps there


def _check_chain(name, first, count, bits, per):
    """per: bits per counted unit (GPS counts bits: 1)"""
    want = S.literal_results(name)
    flat = bits.reshape(len(want), -1)
    for ch, (w_first, w_bits) in enumerate(want):
        assert first[ch] == w_first, (name, ch)
        assert count[ch] * per == w_bits.size, (name, ch)
        assert flat[ch, :w_bits.size].tobytes() == w_bits.tobytes(), \
            (name, ch, np.flatnonzero(flat[ch, :w_bits.size] != w_bits.ravel())[:8])
        assert not flat[ch, w_bits.size:].any(), (name, ch)


def _chain_dev(gc, nav, call, x, shape, *args):
    n_ch, n_ep = x.shape
    d_x, cs = _upload_padded(gc, x)
    d_first, d_n = (gc.DevBuf.from_array(np.full(n_ch, -7, np.int32)) for _ in range(2))
    d_bits = gc.DevBuf.from_array(np.full(n_ch * int(np.prod(shape)), 0xAA, np.uint8))
    call(d_x.ptr, 8, cs, n_ep, n_ch, *args, d_first.ptr, d_n.ptr, d_bits.ptr)
    nav.sync()
    return (d_first.download(np.int32), d_n.download(np.int32),
            d_bits.download(np.uint8).reshape((n_ch,) + shape))


def test_gps_frames(gpu):
    """Both polarities, a lone preamble with valid parity and no partner, a decoy pair refused by parity, words after D30* = 1,
    bits whose 20 samples sum to exactly 0, the groups that pin the add order, and records
    with no frame, one and two whole subframes; the host twin gives the same."""
    nav = gpu.NavCtx()
    x, firsts, n_bits = S.gps_scene()
    got = _chain_dev(gpu, nav, nav.gps_frames_dev, x, (1500,), S.GPS_START, 5)
    assert got[0].tolist() == firsts and got[1].tolist() == n_bits
    _check_chain("gps", *got, 1)
    assert got[2][2, 30 * 3 + 7] == 2 and got[2][2, 30 * 12 + 3] == 2
    twin = nav.gps_frames(x, search_start=S.GPS_START)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, twin))
    # fewer subframes asked for than there are
    one = nav.gps_frames(x, search_start=S.GPS_START, max_subframes=1)
    assert one[1].tolist() == [300, 300, 300, 0]
    assert one[2][:, :300].tobytes() == got[2][:, :300].tobytes() and not one[2][:, 300:].any()


def test_gps_five_subframes_with_the_files_search_offset(gpu):
    nav = gpu.NavCtx()
    x, firsts, n_bits = S.gps_long_scene()
    got = _chain_dev(gpu, nav, nav.gps_frames_dev, x, (1500,), 5000, 5)
    assert got[0].tolist() == firsts and got[1].tolist() == n_bits
    _check_chain("gps_long", *got, 1)


@pytest.mark.parametrize("name", ["glo", "glo_short"])
def test_glo_strings(gpu, name):
    """Marks at 0 and 37, a symbol split 10 / 10 (2 in two decoded places), an inverted copy
    with the same bits; 15, one and no string, and no mark."""
    nav = gpu.NavCtx()
    x, firsts, counts = (S.glo_scene if name == "glo" else S.glo_short_scene)()
    got = _chain_dev(gpu, nav, nav.glo_strings_dev, x, (15, 85), 15)
    assert got[0].tolist() == firsts and got[1].tolist() == counts
    _check_chain(name, *got, 85)
    if name == "glo":
        assert np.flatnonzero(got[2][0, 2] == 2).tolist() == [43, 44]
        assert got[2][1].tobytes() == got[2][2].tobytes()
        two = nav.glo_strings(x, max_strings=2)
        assert two[1].tolist() == [2, 2, 2] and not two[2][:, 2:].any()
        assert two[2][:, :2].tobytes() == got[2][:, :2].tobytes()
    twin = nav.glo_strings(x)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, twin))


@pytest.mark.parametrize("name", ["b1", "b1_short"])
def test_b1_subframes(gpu, name):
    """Both polarities, a preamble sum of exactly 0 (not negated); five, one and no whole
    subframe, and no preamble."""
    nav = gpu.NavCtx()
    x, firsts, counts = (S.b1_scene if name == "b1" else S.b1_short_scene)()
    got = _chain_dev(gpu, nav, nav.b1_subframes_dev, x, (5, 213), 5)
    assert got[0].tolist() == firsts and got[1].tolist() == counts
    _check_chain(name, *got, 213)
    twin = nav.b1_subframes(x)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, twin))


def test_in_place_read_of_tracker_epoch_records(gpu):
    """gnsscorr_sgt_epoch records with NaN in every field but I_P, strides 112 and
    n_epochs * 112: the results of the packed series."""
    gc = gpu
    nav = gc.NavCtx()
    off, stride = gc.epoch_field(gc.SGT_EPOCH, "I_P")
    assert stride == 112
    for name, scene, call, shape, args, per in (
            ("gps", S.gps_scene, nav.gps_frames_dev, (1500,), (S.GPS_START, 5), 1),
            ("glo_short", S.glo_short_scene, nav.glo_strings_dev, (15, 85), (15,), 85),
            ("b1_short", S.b1_short_scene, nav.b1_subframes_dev, (5, 213), (5,), 213)):
        x = scene()[0]
        n_ch, n_ep = x.shape
        ep = np.zeros((n_ch, n_ep), gc.SGT_EPOCH)
        for f in gc.SGT_EPOCH.names:
            if gc.SGT_EPOCH[f].kind == "f":
                ep[f] = np.nan
        ep["I_P"] = x
        d_ep = gc.DevBuf.from_array(ep)
        d_first, d_n = gc.DevBuf(4 * n_ch), gc.DevBuf(4 * n_ch)
        d_bits = gc.DevBuf.from_array(np.full(n_ch * int(np.prod(shape)), 0xAA, np.uint8))
        call(d_ep.ptr + off, stride, n_ep * stride, n_ep, n_ch, *args, d_first.ptr, d_n.ptr,
             d_bits.ptr)
        nav.sync()
        _check_chain(name, d_first.download(np.int32), d_n.download(np.int32),
                     d_bits.download(np.uint8).reshape((n_ch,) + shape), per)
    # the primitive, in place
    x = S.edge_scene()[0]
    ep = np.zeros(x.shape, gc.SGT_EPOCH)
    ep["I_E"], ep["I_L"], ep["I_P"] = np.nan, np.nan, x
    d_ep = gc.DevBuf.from_array(ep)
    d_first, d_n, d_hits = gc.DevBuf(16), gc.DevBuf(16), gc.DevBuf(16 * MAX_HITS)
    nav.pattern_hits_dev(d_ep.ptr + off, stride, x.shape[1] * stride, x.shape[1], 4,
                         S.GPS_PATTERN, 153, 0, MAX_HITS, d_first.ptr, d_n.ptr, d_hits.ptr)
    nav.sync()
    assert d_first.download(np.int32).tolist() == [321, -1, 321, -1]


def test_host_twin_of_the_primitive(gpu):
    nav = gpu.NavCtx()
    pattern, x = S.prim_case(220, 4099, 3)
    thr = S.prim_threshold(220)
    dev = _hits_dev(gpu, nav, x, pattern, thr, 0, 3)
    twin = nav.pattern_hits(x, pattern, thr, 0, 3)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(dev, twin))


@pytest.mark.parametrize("name", ["glo_strings", "b1_subframes"])
def test_first_hit_chain_twins_equal_the_device_forms(gpu, name):
    """The short scenes through the exported host twin and through the device form, both on
    sentinel-filled outputs: the same bytes in first, count and bits, none past them."""
    scene, units, per = {"glo_strings": (S.glo_short_scene, 15, 85),
                         "b1_subframes": (S.b1_short_scene, 5, 213)}[name]
    x, firsts, counts = scene()
    n_ch = len(x)
    first, count, bits = T.twin_and_dev(
        gpu, gpu.NavCtx(), name, [x], [units],
        [(np.int32, n_ch), (np.int32, n_ch), (np.uint8, n_ch * units * per)])
    assert first.tolist() == firsts and count.tolist() == counts


def test_sgt_replay_epochs_feed_the_gps_chain_on_the_device(gpu):
    """SgtCtx.replay_dev writes d_epochs from sums whose I_P carries generated subframes;
    NavCtx.gps_frames_dev reads that array in place, ordered after the replay by an event."""
    gc = gpu
    if not hasattr(gc.SgtCtx, "replay_dev"):
        pytest.fail("SgtCtx.replay_dev is missing")
    x = S.gps_scene()[0][:2]
    n_ch, n_ep = x.shape
    trk = gc.SgtCtx(0)
    rng = np.random.default_rng(3)
    sums = 200.0 + 50.0 * rng.standard_normal((n_ch, n_ep, 6))
    sums[:, :, 1] = x                                          # I_E, I_P, I_L, Q_E, Q_P, Q_L
    chans = trk.init_chans([3, 7], [1, 1], [2.42e6, 2.42e6])
    d_chan, d_sums = gc.DevBuf.from_array(chans), gc.DevBuf.from_array(sums)
    d_ep = gc.DevBuf(n_ch * n_ep * gc.SGT_EPOCH.itemsize)
    d_first, d_n, d_bits = gc.DevBuf(4 * n_ch), gc.DevBuf(4 * n_ch), gc.DevBuf(n_ch * 1500)
    nav = gc.NavCtx()
    trk.replay_dev(n_ch, d_chan.ptr, n_ep, d_sums.ptr, d_ep.ptr)
    done = gc.Event()
    done.record(trk.stream)
    done.wait_on(nav.stream)
    off, stride = gc.epoch_field(gc.SGT_EPOCH, "I_P")
    nav.gps_frames_dev(d_ep.ptr + off, stride, n_ep * stride, n_ep, n_ch, S.GPS_START, 5,
                       d_first.ptr, d_n.ptr, d_bits.ptr)
    nav.sync()
    want = S.literal_results("gps")[:2]
    bits = d_bits.download(np.uint8).reshape(n_ch, 1500)
    assert d_first.download(np.int32).tolist() == [w[0] for w in want]
    for ch in range(n_ch):
        assert bits[ch, :want[ch][1].size].tobytes() == want[ch][1].tobytes()


def test_bad_arguments_are_refused_before_any_launch(gpu):
    gc = gpu
    nav = gc.NavCtx()
    d_in = gc.DevBuf.from_array(np.ones(4096, np.float64))
    fill = np.full(8192, 0xAA, np.uint8)
    d_a, d_b, d_c = (gc.DevBuf.from_array(fill) for _ in range(3))
    pat = np.ones(160, np.int8)
    two = pat.copy()
    two[5] = 2

    def hits(series=d_in.ptr, es=8, cs=8000, n_ep=1000, n_ch=1, pattern=pat, thr=153, first_k=0,
             max_hits=4, a=d_a.ptr, b=d_b.ptr, c=d_c.ptr):
        nav.pattern_hits_dev(series, es, cs, n_ep, n_ch, pattern, thr, first_k, max_hits, a, b, c)

    def chain(call, *mid, series=d_in.ptr, es=8, cs=8000, n_ep=1000, n_ch=1, a=d_a.ptr,
              b=d_b.ptr, c=d_c.ptr):
        call(series, es, cs, n_ep, n_ch, *mid, a, b, c)

    bad = [
        lambda: hits(series=None), lambda: hits(a=None), lambda: hits(b=None),
        lambda: hits(c=None), lambda: hits(n_ep=0), lambda: hits(n_ch=0), lambda: hits(es=4),
        lambda: hits(es=12), lambda: hits(cs=0), lambda: hits(series=d_in.ptr + 4),
        lambda: hits(pattern=np.ones(513, np.int8), thr=10),   # T > 512
        lambda: hits(pattern=np.ones(0, np.int8), thr=0),      # T < 1
        lambda: hits(thr=160), lambda: hits(thr=-1), lambda: hits(first_k=-1),
        lambda: hits(max_hits=0), lambda: hits(pattern=two),
        lambda: chain(nav.gps_frames_dev, 39, 5),              # search_start < 40
        lambda: chain(nav.gps_frames_dev, 100, 0), lambda: chain(nav.gps_frames_dev, 100, 5, a=None),
        lambda: chain(nav.gps_frames_dev, 100, 5, es=7),
        lambda: chain(nav.gps_frames_dev, 100, 5, series=None),
        lambda: chain(nav.glo_strings_dev, 0), lambda: chain(nav.glo_strings_dev, 15, c=None),
        lambda: chain(nav.glo_strings_dev, 15, n_ep=0),
        lambda: chain(nav.b1_subframes_dev, 0), lambda: chain(nav.b1_subframes_dev, 5, b=None),
        lambda: chain(nav.b1_subframes_dev, 5, cs=4),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(gc.GnssCorrError):
            call()
            pytest.fail(f"bad call {i} was accepted")
    h_first, h_n, h_hits = (np.full(4, -7, np.int32) for _ in range(3))
    for thr, p in ((160, pat), (10, two)):                     # the host twins refuse the same
        rc = gc.lib().gnsscorr_nav_pattern_hits(nav.h, d_in.ptr, 8, 8000, 1000, 1, p.ctypes.data,
                                                160, thr, 0, 4, h_first.ctypes.data,
                                                h_n.ctypes.data, h_hits.ctypes.data)
        assert rc == -1
    with pytest.raises(gc.GnssCorrError):
        nav.gps_frames(np.ones((1, 1000)), search_start=10)
    nav.sync()
    assert (h_first == -7).all() and (h_n == -7).all() and (h_hits == -7).all()
    for d in (d_a, d_b, d_c):                                  # nothing ran: nothing was written
        assert d.download(np.uint8).tobytes() == fill.tobytes()
