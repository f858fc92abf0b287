"""GPU: the navigation-symbol kernels (csrc/navsym.hip) against the literal restatement of
the Scilab receiver's symbol chain (tests/navsym_scenarios.py).  Every comparison is exact:
bits and positions have no tolerance.

The Viterbi cases take their expected bits from viterbi_literal, the transcription that keeps
the files' matrices; the E1 and L3 chains use the restatements with viterbi_fast, which
tests/test_navsym_cpu.py holds equal to the literal decoder.  References are computed once per
case and shared.
"""
import functools

import numpy as np
import pytest

import nav_twin as T
import navsym_scenarios as S

pytestmark = pytest.mark.gpu

# (L, streams): one step, the window edge 42 / 43, more than one block of 64 output bits
# (257 = 4 blocks + 1); 1, 3 and 65 streams
SHAPES = [(1, 3), (2, 3), (8, 3), (43, 3), (120, 3), (257, 3), (42, 1), (257, 1), (43, 65)]
KINDS = ("clean", "flip03", "flip15", "random")


@functools.lru_cache(maxsize=None)
def _hard_case(L, n):
    rng = np.random.default_rng(7000 + 10 * L + n)
    code = np.zeros((n, 2 * L), np.uint8)
    for i in range(n):
        kind = KINDS[(i + L) % 4]
        _, code[i] = S.noisy_code(rng, L, {"flip03": 0.03, "flip15": 0.15}.get(kind, 0.0),
                                  kind == "random")
    want = np.array([S.viterbi_literal(c, False)[0] for c in code])
    code.setflags(write=False)
    want.setflags(write=False)
    return code, want


@functools.lru_cache(maxsize=None)
def _soft_case(L, n, grid):
    rng = np.random.default_rng(9000 + 10 * L + n + int(grid))
    code = np.array([S.soft_code(rng, L, grid)[1] for _ in range(n)])
    want = np.array([S.viterbi_literal(c, True)[0] for c in code])
    code.setflags(write=False)
    want.setflags(write=False)
    return code, want


def _decode_dev(gc, nav, code, soft, pad):
    """viterbi_dev on an uploaded copy whose rows are `pad` elements longer than a stream"""
    n, L = code.shape[0], code.shape[1] // 2
    padded = np.full((n, code.shape[1] + pad), 1, code.dtype)     # padding of ones: never read
    padded[:, :code.shape[1]] = code
    d_code = gc.DevBuf.from_array(padded)
    d_bits = gc.DevBuf.from_array(np.full(n * L, 0xAA, np.uint8))
    nav.viterbi_dev(d_code.ptr, padded.strides[0], n, L, soft, d_bits.ptr)
    nav.sync()
    return d_bits.download(np.uint8).reshape(n, L)


@pytest.mark.parametrize("L,n", SHAPES)
def test_hard_viterbi_equals_the_literal_decoder(gpu, L, n):
    nav = gpu.NavCtx()
    code, want = _hard_case(L, n)
    got = _decode_dev(gpu, nav, code, False, pad=3 if L % 2 else 0)
    assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:8]


@pytest.mark.parametrize("grid", [True, False], ids=["grid8", "doubles"])
@pytest.mark.parametrize("L,n", SHAPES)
def test_soft_viterbi_equals_the_literal_decoder(gpu, L, n, grid):
    """Soft input once on a 1/8 grid (exact arithmetic, many tied costs) and once as random
    doubles (every rounding of (r1 - o1)^2 + (r2 - o2)^2 + metric counts)."""
    nav = gpu.NavCtx()
    code, want = _soft_case(L, n, grid)
    got = _decode_dev(gpu, nav, code, True, pad=1 if L % 2 else 0)
    assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:8]


def test_host_twin_and_hard_input_as_soft(gpu):
    """NavCtx.viterbi (host arrays) gives the device call's bits; hard 0/1 symbols given as
    doubles decode to the hard decoder's bits (the squared distance of 0/1 values is the
    Hamming distance)."""
    nav = gpu.NavCtx()
    code, want = _hard_case(120, 3)
    assert nav.viterbi(code).tobytes() == want.tobytes()
    assert nav.viterbi(code[0])[0].tobytes() == want[0].tobytes()
    assert nav.viterbi(code.astype(np.float64), soft=True).tobytes() == want.tobytes()


# ---- E1B pages -------------------------------------------------------------------------
E1_EPOCHS = 3200


@functools.lru_cache(maxsize=None)
def _e1_scene():
    """Three channels with page starts 0, 37 and 999 (both polarities, exact zeros, a zero
    inside a sync pattern, a few flipped epochs) and a fourth of noise, which must give -1:
    the three page starts and the noise channel in one launch of 4 x 3200 epochs."""
    rng = np.random.default_rng(4242)
    series = np.zeros((4, E1_EPOCHS))
    series[0], _ = S.e1_series(rng, E1_EPOCHS, 0, polarity=1, n_zeros=20)
    series[1], _ = S.e1_series(rng, E1_EPOCHS, 37, polarity=-1, flip_rate=0.02)
    series[2], _ = S.e1_series(rng, E1_EPOCHS, 999, polarity=1, zero_in_sync=True, n_zeros=5)
    series[3] = 1500.0 * rng.standard_normal(E1_EPOCHS)
    want = [S.e1_pages(x) for x in series]
    assert [w[0] for w in want] == [0, 37, 999, -1]        # the planted starts are what is found
    assert [len(w[1]) for w in want] == [3, 3, 2, 0]
    series.setflags(write=False)
    return series, want


def _check_e1(first, n_pages, bits, want):
    for ch, (w_first, w_bits) in enumerate(want):
        assert first[ch] == w_first, ch
        assert n_pages[ch] == len(w_bits), ch
        assert bits[ch, :len(w_bits)].tobytes() == w_bits.tobytes(), ch
        assert not bits[ch, len(w_bits):].any(), ch


def test_e1_pages_from_a_plain_array(gpu):
    series, want = _e1_scene()
    first, n_pages, bits = gpu.NavCtx().e1_pages(series)
    assert bits.shape == (4, 3, 120)
    _check_e1(first, n_pages, bits, want)


def test_e1_pages_in_place_from_epoch_records(gpu):
    """The series read at stride 176 out of an uploaded gnsscorr_e1t_epoch array."""
    gc = gpu
    series, want = _e1_scene()
    n_ch, n_ep = series.shape
    ep = np.zeros((n_ch, n_ep), gc.E1T_EPOCH)
    for f in gc.E1T_SUMS:
        ep[f] = -series[:, ::-1]                           # the neighbours hold other values
    ep["I_P_P"] = series
    off, stride = gc.epoch_field(gc.E1T_EPOCH, "I_P_P")
    assert stride == 176
    d_ep = gc.DevBuf.from_array(ep)
    d_first, d_np = gc.DevBuf(4 * n_ch), gc.DevBuf(4 * n_ch)
    d_bits = gc.DevBuf.from_array(np.full(n_ch * 3 * 120, 0xAA, np.uint8))
    nav = gc.NavCtx()
    nav.e1_pages_dev(d_ep.ptr + off, stride, n_ep * stride, n_ep, n_ch, 3, d_first.ptr, d_np.ptr,
                     d_bits.ptr)
    nav.sync()
    _check_e1(d_first.download(np.int32), d_np.download(np.int32),
              d_bits.download(np.uint8).reshape(n_ch, 3, 120), want)
    # fewer pages asked for than there are
    nav.e1_pages_dev(d_ep.ptr + off, stride, n_ep * stride, n_ep, n_ch, 1, d_first.ptr, d_np.ptr,
                     d_bits.ptr)
    nav.sync()
    assert d_np.download(np.int32).tolist() == [1, 1, 1, 0]
    got = d_bits.download(np.uint8)[:n_ch * 120].reshape(n_ch, 120)
    for ch in range(3):
        assert got[ch].tobytes() == want[ch][1][0].tobytes()


# ---- L3OC ------------------------------------------------------------------------------
L3_EPOCHS = 2500
MAX_MARKS = 8


@functools.lru_cache(maxsize=None)
def _l3_scene():
    """Overlay starts 0 and 7 (the second channel inverted, with zeros and flips), a time
    mark in each message, and a channel whose pilot never reaches 10."""
    rng = np.random.default_rng(777)
    pilot, data = np.zeros((3, L3_EPOCHS)), np.zeros((3, L3_EPOCHS))
    pilot[0], data[0], _ = S.l3_series(rng, L3_EPOCHS, 0, mark_at=100, n_zeros=10)
    pilot[1], data[1], _ = S.l3_series(rng, L3_EPOCHS, 7, polarity=-1, mark_at=31,
                                       flip_rate=0.01, n_zeros=10)
    pilot[2], data[2], _ = S.l3_series(rng, L3_EPOCHS, 3, constant_pilot=True)
    want = [S.l3_data_decode(p, d) for p, d in zip(pilot, data)]
    assert [w[0] for w in want] == [0, 7, -1]
    assert [len(w[1]) for w in want] == [250, 249, 0]
    assert 100 in want[0][2] and 31 in want[1][2]          # the planted marks are found
    return pilot, data, want


def _check_l3(start, n_bits, bits, n_marks, marks, want):
    for ch, (w_start, w_bits, w_marks) in enumerate(want):
        assert start[ch] == w_start, ch
        assert n_bits[ch] == len(w_bits), ch
        assert bits[ch, :len(w_bits)].tobytes() == w_bits.tobytes(), ch
        assert not bits[ch, len(w_bits):].any(), ch
        assert n_marks[ch] == len(w_marks), ch
        k = min(len(w_marks), MAX_MARKS)
        assert marks[ch, :k].tolist() == w_marks[:k].tolist(), ch
        assert (marks[ch, k:] == -1).all(), ch


def test_l3_decode_in_place_from_epoch_records(gpu):
    """Pilot i_p and data q_p2 read at stride 160 out of an uploaded gnsscorr_l3t_epoch
    array; the host-array twin gives the same."""
    gc = gpu
    pilot, data, want = _l3_scene()
    n_ch, n_ep = pilot.shape
    ep = np.zeros((n_ch, n_ep), gc.L3T_EPOCH)
    for f in gc.L3T_SUMS:
        ep[f] = -pilot[:, ::-1]
    ep["I_P"], ep["Q_P2"] = pilot, data
    (off_i, stride), (off_q, _) = (gc.epoch_field(gc.L3T_EPOCH, f) for f in ("I_P", "Q_P2"))
    assert stride == 160
    d_ep = gc.DevBuf.from_array(ep)
    d_start, d_nb, d_nm = (gc.DevBuf(4 * n_ch) for _ in range(3))
    d_marks = gc.DevBuf(4 * n_ch * MAX_MARKS)
    d_bits = gc.DevBuf.from_array(np.full(n_ch * (n_ep // 10), 0xAA, np.uint8))
    nav = gc.NavCtx()
    nav.l3_decode_dev(d_ep.ptr + off_i, d_ep.ptr + off_q, stride, n_ep * stride, n_ep, n_ch,
                      MAX_MARKS, d_start.ptr, d_nb.ptr, d_bits.ptr, d_nm.ptr, d_marks.ptr)
    nav.sync()
    _check_l3(d_start.download(np.int32), d_nb.download(np.int32),
              d_bits.download(np.uint8).reshape(n_ch, n_ep // 10), d_nm.download(np.int32),
              d_marks.download(np.int32).reshape(n_ch, MAX_MARKS), want)
    _check_l3(*nav.l3_decode(pilot, data, max_marks=MAX_MARKS), want)


def test_l3_more_marks_than_room(gpu):
    """A message of repeated time marks: the count is of all of them, the list holds the
    first max_marks in ascending order."""
    n_ep = 1300
    msg = np.tile((S.TIME_MARK + 1) // 2, 7)[:n_ep // 10].astype(np.uint8)
    sym = S.conv_encode(msg)[:2 * len(msg)] * 2.0 - 1
    data = (sym[:, None] * S.BARKER[None, :]).ravel() * 300.0
    pilot = np.tile(S.NH, n_ep // 10) * 300.0
    want = S.l3_data_decode(pilot, data)
    assert len(want[2]) >= 5
    start, n_bits, bits, n_marks, marks = gpu.NavCtx().l3_decode(pilot, data, max_marks=3)
    assert start[0] == 0 and n_bits[0] == len(want[1])
    assert bits[0].tobytes() == want[1].tobytes()
    assert n_marks[0] == len(want[2]) and marks[0].tolist() == want[2][:3].tolist()


# ---- hand-off --------------------------------------------------------------------------
def test_e1t_replay_epochs_feed_the_page_decoder_on_the_device(gpu):
    """E1tCtx.replay_dev writes d_epochs from sums whose I_P_P carries generated pages;
    NavCtx.e1_pages_dev reads that array in place, ordered after the replay by an event."""
    gc = gpu
    rng = np.random.default_rng(99)
    n_ep, starts = 2200, (37, 5)
    series = np.stack([S.e1_series(rng, n_ep, starts[0])[0],
                       S.e1_series(rng, n_ep, starts[1], polarity=-1, n_zeros=8)[0]])
    want = [S.e1_pages(x) for x in series]
    assert [w[0] for w in want] == list(starts) and [len(w[1]) for w in want] == [2, 2]
    n_ch = len(series)
    sums = 200.0 + 50.0 * rng.standard_normal((n_ch, n_ep, len(gc.E1T_SUMS)))
    sums[:, :, gc.E1T_SUMS.index("I_P_P")] = series
    trk = gc.E1tCtx()
    chans = np.concatenate([trk.init_chan(0, 1, 2.42e6) for _ in range(n_ch)])
    d_chan, d_sums = gc.DevBuf.from_array(chans), gc.DevBuf.from_array(sums)
    d_ep = gc.DevBuf(n_ch * n_ep * gc.E1T_EPOCH.itemsize)
    d_first, d_np = gc.DevBuf(4 * n_ch), gc.DevBuf(4 * n_ch)
    d_bits = gc.DevBuf(n_ch * 2 * 120)
    nav = gc.NavCtx()
    trk.replay_dev(n_ch, d_chan.ptr, n_ep, d_sums.ptr, d_ep.ptr)
    done = gc.Event()
    done.record(trk.stream)
    done.wait_on(nav.stream)
    off, stride = gc.epoch_field(gc.E1T_EPOCH, "I_P_P")
    nav.e1_pages_dev(d_ep.ptr + off, stride, n_ep * stride, n_ep, n_ch, 2, d_first.ptr, d_np.ptr,
                     d_bits.ptr)
    nav.sync()
    _check_e1(d_first.download(np.int32), d_np.download(np.int32),
              d_bits.download(np.uint8).reshape(n_ch, 2, 120), want)
    ep = d_ep.download(gc.E1T_EPOCH).reshape(n_ch, n_ep)
    assert ep["I_P_P"].tobytes() == series.tobytes()


# ---- host-array twins against the device forms -------------------------------------------
def _l3_outs(n_ch, n_ep, max_marks):
    """start, n_bits, bits, n_marks, marks"""
    return [(np.int32, n_ch), (np.int32, n_ch), (np.uint8, n_ch * (n_ep // 10)),
            (np.int32, n_ch), (np.int32, n_ch * max_marks)]


def test_l3_host_twin_equals_the_device_form(gpu):
    """Two channels, overlay starts 0 and 7 (the second inverted, with zeros), a time mark in
    each message: every output of the twin is the device form's, byte for byte, and nothing
    past it is written."""
    rng = np.random.default_rng(31)
    a = S.l3_series(rng, 600, 0, mark_at=10)
    b = S.l3_series(rng, 600, 7, polarity=-1, mark_at=25, n_zeros=4)
    pilot, data = np.stack([a[0], b[0]]), np.stack([a[1], b[1]])
    start, n_bits, bits, n_marks, marks = T.twin_and_dev(
        gpu, gpu.NavCtx(), "l3_decode", [pilot, data], [4], _l3_outs(2, 600, 4))
    assert start.tolist() == [0, 7] and n_bits.tolist() == [60, 59]
    assert n_marks.tolist() == [1, 1] and marks.reshape(2, 4)[:, 0].tolist() == [10, 25]


def test_l3_host_twin_with_fewer_than_ten_epochs(gpu):
    """n_epochs = 9: n_epochs // 10 == 0, the bits output has no element and its host array is
    left alone; start, n_bits, n_marks and marks still come back (nine epochs cannot reach the
    overlay's |sum| = 10: no start, no bits, no marks)."""
    rng = np.random.default_rng(32)
    a, b = S.l3_series(rng, 9, 0), S.l3_series(rng, 9, 2)
    pilot, data = np.stack([a[0], b[0]]), np.stack([a[1], b[1]])
    start, n_bits, bits, n_marks, marks = T.twin_and_dev(
        gpu, gpu.NavCtx(), "l3_decode", [pilot, data], [3], _l3_outs(2, 9, 3))
    assert bits.size == 0
    assert start.tolist() == [-1, -1] and n_bits.tolist() == [0, 0]
    assert n_marks.tolist() == [0, 0] and marks.tolist() == [-1] * 6


def test_e1_host_twin_equals_the_device_form(gpu):
    """Two channels, max_pages = 2: page start 37 (inverted, with zeros) and a channel of
    noise, which has no page start."""
    rng = np.random.default_rng(33)
    series = np.stack([S.e1_series(rng, 2200, 37, polarity=-1, n_zeros=6)[0],
                       1500.0 * rng.standard_normal(2200)])
    first, n_pages, bits = T.twin_and_dev(
        gpu, gpu.NavCtx(), "e1_pages", [series], [2],
        [(np.int32, 2), (np.int32, 2), (np.uint8, 2 * 2 * 120)])
    assert first.tolist() == [37, -1] and n_pages.tolist() == [2, 0]
    assert not bits.reshape(2, 240)[1].any()


def test_refused_host_twins_leave_their_arrays_alone(gpu):
    """l3_decode and e1_pages with n_ch = 0 and with an odd epoch stride: the shared series
    check refuses both before anything is staged, and every output byte is still the
    sentinel."""
    gc = gpu
    nav = gc.NavCtx()
    x = np.ones((2, 1200))
    p = x.ctypes.data
    for es, n_ch in ((8, 0), (9, 2)):
        outs = [T.sentinel(n, dt) for dt, n in _l3_outs(2, 1200, 4)]
        rc = nav._l3_decode(nav.h, p, p, es, 8 * 1200, 1200, n_ch, 4,
                            *[o.ctypes.data for o in outs])
        assert rc == -1, (es, n_ch)
        assert all(T.intact(o) for o in outs), (es, n_ch)
        outs = [T.sentinel(n, dt) for dt, n in ((np.int32, 2), (np.int32, 2), (np.uint8, 240))]
        rc = nav._e1_pages(nav.h, p, es, 8 * 1200, 1200, n_ch, 1, *[o.ctypes.data for o in outs])
        assert rc == -1, (es, n_ch)
        assert all(T.intact(o) for o in outs), (es, n_ch)


# ---- bad arguments ---------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(gpu):
    gc = gpu
    nav = gc.NavCtx()
    d_in = gc.DevBuf.from_array(np.zeros(4096, np.float64))
    fill = np.full(4096, 0xAA, np.uint8)
    d_out, d_a, d_b, d_c, d_d = (gc.DevBuf.from_array(fill) for _ in range(5))
    big = (2 ** 31 - 1 - 10000) // 2 - 42 + 1               # the first L past the int32 bound
    bad = [
        lambda: nav.viterbi_dev(None, 16, 1, 8, False, d_out.ptr),
        lambda: nav.viterbi_dev(d_in.ptr, 16, 1, 8, False, None),
        lambda: nav.viterbi_dev(d_in.ptr, 16, 1, 0, False, d_out.ptr),
        lambda: nav.viterbi_dev(d_in.ptr, 16, 0, 8, False, d_out.ptr),
        lambda: nav.viterbi_dev(d_in.ptr, 2 * big, 1, big, False, d_out.ptr),
        lambda: nav.viterbi_dev(d_in.ptr, 8, 2, 8, False, d_out.ptr),       # streams overlap
        lambda: nav.viterbi_dev(d_in.ptr + 4, 128, 1, 8, True, d_out.ptr),  # fp64 misaligned
        lambda: nav.e1_pages_dev(None, 8, 8000, 1000, 1, 1, d_a.ptr, d_b.ptr, d_out.ptr),
        lambda: nav.e1_pages_dev(d_in.ptr, 8, 8000, 1000, 1, 1, None, d_b.ptr, d_out.ptr),
        lambda: nav.e1_pages_dev(d_in.ptr, 8, 8000, 0, 1, 1, d_a.ptr, d_b.ptr, d_out.ptr),
        lambda: nav.e1_pages_dev(d_in.ptr, 4, 8000, 1000, 1, 1, d_a.ptr, d_b.ptr, d_out.ptr),
        lambda: nav.e1_pages_dev(d_in.ptr, 8, 0, 1000, 1, 1, d_a.ptr, d_b.ptr, d_out.ptr),
        lambda: nav.e1_pages_dev(d_in.ptr, 8, 8000, 1000, 1, 0, d_a.ptr, d_b.ptr, d_out.ptr),
        lambda: nav.l3_decode_dev(d_in.ptr, None, 8, 8000, 1000, 1, 4, d_a.ptr, d_b.ptr,
                                  d_out.ptr, d_c.ptr, d_d.ptr),
        lambda: nav.l3_decode_dev(d_in.ptr, d_in.ptr, 8, 8000, 0, 1, 4, d_a.ptr, d_b.ptr,
                                  d_out.ptr, d_c.ptr, d_d.ptr),
        lambda: nav.l3_decode_dev(d_in.ptr, d_in.ptr, 7, 8000, 1000, 1, 4, d_a.ptr, d_b.ptr,
                                  d_out.ptr, d_c.ptr, d_d.ptr),
        lambda: nav.l3_decode_dev(d_in.ptr, d_in.ptr, 8, 8000, 1000, 1, 4, d_a.ptr, d_b.ptr,
                                  d_out.ptr, d_c.ptr, None),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(gc.GnssCorrError):
            call()
            pytest.fail(f"bad call {i} was accepted")
    with pytest.raises(gc.GnssCorrError):
        nav.viterbi(np.zeros((2, 0), np.uint8))
    nav.sync()
    for d in (d_out, d_a, d_b, d_c, d_d):                  # nothing ran: nothing was written
        assert d.download(np.uint8).tobytes() == fill.tobytes()
