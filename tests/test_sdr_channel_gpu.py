"""GPU parity: the GPS-SDR Channel object batched on the GPU (sdr_channel.hip),
SURVEY 8(f) ranks 2 and 4: bit lock, bit stuffing, frame sync, ICD-200 parity,
subframe validation, C/N0, FrequencyLock / PLL / DLL, Error / Kill, and the
NCO_Command_S feedback of every Channel::Accum call (objects/channel.cpp:182-993).

Against the reference Channel itself: its committed outputs
(tests/golden/sdr_channel.npz, sdr_channel_branches.npz) and, where the
reference build travelled with the tree (oracle/_ref/libsdr_chan_ref.so), a
live run on other streams.
Integers, flags, bit decisions, word buffers and subframes exact; float /
double loop state within rtol 1e-6 (atan / log10 may differ in the last bit).

The launch shape (64 channels per workgroup, a partial last workgroup, the
fb == NULL / fb_last form the benchmark uses, the subframe array overflowing)
is held to the one-workgroup launch byte for byte, with poisoned guard regions
behind every output array.
"""
import os

import numpy as np
import pytest

import make_sdr_chan_branches_golden as B
import make_sdr_chan_golden as G
import sdr_nav_scenarios as N
import sdr_oracle as S

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLOATS = ("carrier_nco", "code_nco", "I_avg", "Q_var", "P_avg", "cn0", "pll", "dll")
POISON = 0xA5
N_MANY = 200          # three full workgroups of 64 and one of 8


def _start(gpu, scen):
    ch = np.zeros(len(scen), gpu.SDR_CHANNEL)
    for k, sc in enumerate(scen):
        ch[k] = gpu.SdrCorrCtx.channel_start(k, int(sc[0]), int(sc[1]), int(sc[2]))
    return ch


def _cmp_state(got, want_bytes, gpu):
    want = np.frombuffer(want_bytes.tobytes()[:gpu.SDR_CHANNEL_CORE.itemsize],
                         gpu.SDR_CHANNEL_CORE)[0]
    for f in gpu.SDR_CHANNEL_CORE.names:
        if f == "_pad":   # alignment padding (in the full struct: fft_buff[0])
            continue
        a, b = np.asarray(got[f]), np.asarray(want[f])
        if f in FLOATS:
            if f == "pll":   # [15] fll_lock reads an uninitialised local in the reference
                a, b = np.delete(a, 15), np.delete(b, 15)
            assert np.allclose(a, b, rtol=1e-6, atol=1e-9), (f, a, b)
        else:
            assert (a == b).all(), (f, a, b)


def _cmp_golden(gpu, g, fb, ch, ev, n_ev):
    """One launch's outputs (channel k = stream k of the fixture g) against g."""
    e = int(g["nco_every"])
    for k in range(len(ch)):
        assert (G.flags_of(fb[:, k]) == g["flags"][k]).all(), k
        zc = np.where(fb[:, k]["set_z_count"] != 0, fb[:, k]["z_count"], 0)
        assert (zc == g["z_count"][k]).all()
        assert np.allclose(fb[::e, k]["carrier_nco"], g["nco"][k][:, 0], rtol=1e-9)
        assert np.allclose(fb[::e, k]["code_nco"], g["nco"][k][:, 1], rtol=1e-9)
        _cmp_state(ch[k], g["state"][k], gpu)
    rows, words = g["sub_rows"], g["sub_words"]
    order = np.lexsort((rows[:, 0], rows[:, 1]))
    assert n_ev == len(rows)
    assert (ev["chan"] == rows[order, 0]).all() and (ev["ms"] == rows[order, 1]).all()
    assert (ev["sv"] == rows[order, 2]).all() and (ev["subframe"] == rows[order, 3]).all()
    assert (ev["word_buff"] == words[order]).all()


def test_golden_scenarios(gpu):
    g = np.load(os.path.join(GOLD, "sdr_channel.npz"))
    n_ms = int(g["n_ms"])
    corr = np.stack([G.scenario_corr(sc, n_ms) for sc in N.SCENARIOS], 1)   # (n_ms, n_ch, 6)
    ch = _start(gpu, N.SCENARIOS)
    ctx = gpu.SdrCorrCtx()
    fb, ev, n_ev = ctx.channel_accum(corr, ch)
    _cmp_golden(gpu, g, fb, ch, ev, n_ev)


def _subs_of(ev, k):
    return [(int(e["ms"]), int(e["subframe"]), e["word_buff"]) for e in ev[ev["chan"] == k]]


def test_branch_goldens(gpu):
    """The eight branch streams in one launch against the reference's outputs,
    then each stream's defining event on the GPU's own output."""
    g = np.load(os.path.join(GOLD, "sdr_channel_branches.npz"))
    scen = N.BRANCH_SCENARIOS
    corr = np.stack([N.branch_corr(sc) for sc in scen], 1)
    ch = _start(gpu, [N.branch_start(sc) for sc in scen])
    ctx = gpu.SdrCorrCtx()
    fb, ev, n_ev = ctx.channel_accum(corr, ch)
    _cmp_golden(gpu, g, fb, ch, ev, n_ev)
    # the C/N0 stream alone, launch by launch up to each snapshot call: len 1, 20, 20, 1
    k = int(g["snap_stream"])
    one = _start(gpu, [N.branch_start(sc) for sc in scen])[k:k + 1]
    lens, m0 = [], 0
    for call, want in zip(g["snap_calls"], g["snap_state"]):
        ctx.channel_accum(corr[m0:call + 1, k:k + 1], one)
        m0 = int(call) + 1
        _cmp_state(one[0], want, gpu)
        lens.append(int(one[0]["len"]))
    assert lens == [1, 20, 20, 1]
    ctx.channel_accum(corr[m0:, k:k + 1], one)
    assert one.tobytes() == ch[k:k + 1].tobytes()
    for j, sc in enumerate(scen):
        B.reach(sc["name"], G.flags_of(fb[:, j]), fb[:, j]["carrier_nco"], _subs_of(ev, j),
                twin=(G.flags_of(fb[:, 0]), _subs_of(ev, 0)), lens=lens)


def test_split_launches_equal_one(gpu):
    """State carries across launches: 3 launches of 5000 calls == one of 15000."""
    corr = np.stack([G.scenario_corr(sc, 15000) for sc in N.SCENARIOS], 1)
    ctx = gpu.SdrCorrCtx()
    a = _start(gpu, N.SCENARIOS)
    fa, ea, _ = ctx.channel_accum(corr, a)
    b = _start(gpu, N.SCENARIOS)
    parts = [ctx.channel_accum(corr[i:i + 5000], b) for i in range(0, 15000, 5000)]
    assert a.tobytes() == b.tobytes()
    assert np.concatenate([p[0] for p in parts]).tobytes() == fa.tobytes()
    assert sum(p[2] for p in parts) == len(ea)


# ---------------------------------------------------------------- launch shape
class _Guarded:
    """A device array of exactly the payload's size followed by a poisoned guard."""

    def __init__(self, gpu, payload, guard, poison_payload=False):
        self.n = payload if isinstance(payload, int) else payload.nbytes
        self.guard = guard
        self.buf = gpu.DevBuf(self.n + guard)
        self.buf.upload(np.full(guard, POISON, np.uint8), self.n)
        if not isinstance(payload, int):
            self.buf.upload(payload)
        elif poison_payload:
            self.buf.upload(np.full(self.n, POISON, np.uint8))
        self.ptr = self.buf.ptr

    def get(self, dtype):
        return self.buf.download(np.uint8, self.n).view(dtype)

    def intact(self):
        return bool((self.buf.download(np.uint8, self.guard, self.n) == POISON).all())


def _launch(gpu, ctx, corr, chans, ends=None, all_fb=True, max_ev=4096):
    """channel_accum_dev over corr (n_ms, n_ch, 6) in len(ends) launches (ends: the
    launches' end calls) on arrays exactly n_ch long, each followed by 64 poisoned
    records.  Events come back in slot order with ms counted from the first
    launch; slots past n_ev (and past max_ev) keep the poison."""
    n_ms, n_ch = corr.shape[:2]
    fbsz, evsz = gpu.SDR_FEEDBACK.itemsize, gpu.SDR_SUBFRAME.itemsize
    d_c = gpu.DevBuf.from_array(corr)
    d_s = _Guarded(gpu, chans, 64 * gpu.SDR_CHANNEL.itemsize)
    d_fb = _Guarded(gpu, n_ms * n_ch * fbsz, 64 * fbsz) if all_fb else None
    d_last = _Guarded(gpu, n_ch * fbsz, 64 * fbsz, poison_payload=True)
    d_ev = _Guarded(gpu, max_ev * evsz, 64 * evsz, poison_payload=True)
    d_n = gpu.DevBuf.from_array(np.zeros(1, np.int32))
    m0, marks = 0, []
    for m1 in ends or [n_ms]:
        ctx.channel_accum_dev(n_ch, m1 - m0, d_c.ptr + m0 * n_ch * corr.itemsize * 6, d_s.ptr,
                              d_fb.ptr + m0 * n_ch * fbsz if all_fb else None, d_last.ptr,
                              d_ev.ptr, max_ev, d_n.ptr)
        ctx.sync()
        marks.append((m0, int(d_n.download(np.int32)[0])))
        m0 = m1
    assert m0 == n_ms
    ev = d_ev.get(gpu.SDR_SUBFRAME).copy()
    n0 = 0
    for start, n1 in marks:
        ev["ms"][n0:min(n1, max_ev)] += start
        n0 = min(n1, max_ev)
    guards = [d_s, d_last, d_ev] + ([d_fb] if all_fb else [])
    return dict(chans=d_s.get(gpu.SDR_CHANNEL).copy(), last=d_last.get(gpu.SDR_FEEDBACK),
                fb=d_fb.get(gpu.SDR_FEEDBACK).reshape(n_ms, n_ch) if all_fb else None,
                ev=ev, n_ev=marks[-1][1], intact=all(d.intact() for d in guards))


def _by_ms_chan(ev):
    return ev[np.lexsort((ev["chan"], ev["ms"]))]


@pytest.fixture(scope="module")
def many(gpu):
    """The four golden and the eight branch streams, once as 12 channels of one
    workgroup and once as N_MANY channels (channel c runs stream perm[c] % 12, so
    neighbouring threads diverge) with every call's feedback."""
    n_ms = N.BRANCH_MS
    corr12 = np.stack([G.scenario_corr(sc, n_ms) for sc in N.SCENARIOS] +
                      [N.branch_corr(sc) for sc in N.BRANCH_SCENARIOS], 1)
    start = [sc[:3] for sc in N.SCENARIOS] + [N.branch_start(sc) for sc in N.BRANCH_SCENARIOS]
    ctx = gpu.SdrCorrCtx()
    ch12 = _start(gpu, start)
    fb12, ev12, _ = ctx.channel_accum(corr12, ch12)
    stream = np.random.default_rng(200).permutation(N_MANY) % len(start)
    corr = np.ascontiguousarray(corr12[:, stream])
    ch0 = _start(gpu, [start[s] for s in stream])
    out = _launch(gpu, ctx, corr, ch0)
    # what the one-workgroup run says each of the N_MANY channels must give
    want_ch = ch12[stream].copy()
    want_ch["chan"] = np.arange(N_MANY)
    want_ev = []
    for c, s in enumerate(stream):
        e = ev12[ev12["chan"] == s].copy()
        e["chan"] = c
        want_ev.append(e)
    return dict(ctx=ctx, corr=corr, ch0=ch0, stream=stream, out=out, fb12=fb12, want_ch=want_ch,
                want_ev=_by_ms_chan(np.concatenate(want_ev)))


def test_many_workgroups_equal_one(gpu, many):
    out, stream = many["out"], many["stream"]
    assert out["intact"], "a write past the n_ch-long channel, feedback or event array"
    assert np.bincount(stream, minlength=12).min() >= 16
    assert out["chans"].tobytes() == many["want_ch"].tobytes()
    want_fb = np.ascontiguousarray(many["fb12"][:, stream])
    same = (out["fb"].view(np.uint8).reshape(len(want_fb), N_MANY, -1) ==
            want_fb.view(np.uint8).reshape(len(want_fb), N_MANY, -1)).all(axis=(0, 2))
    assert same.all(), ("channels whose feedback differs", np.flatnonzero(~same)[:8])
    assert (out["last"].tobytes() == want_fb[-1].tobytes())
    n = out["n_ev"]
    assert n == len(many["want_ev"]) and n > 64
    assert _by_ms_chan(out["ev"][:n]).tobytes() == many["want_ev"].tobytes()
    assert (out["ev"][n:].view(np.uint8) == POISON).all()


def test_bench_argument_shape(gpu, many):
    """fb == NULL, fb_last only, three launches: the benchmark's call."""
    n_ms = many["corr"].shape[0]
    out = _launch(gpu, many["ctx"], many["corr"], many["ch0"].copy(),
                  ends=[10667, 21334, n_ms], all_fb=False)
    assert out["intact"]
    assert out["chans"].tobytes() == many["out"]["chans"].tobytes()
    assert out["last"].tobytes() == many["out"]["fb"][-1].tobytes()
    n = out["n_ev"]
    assert n == many["out"]["n_ev"]
    assert _by_ms_chan(out["ev"][:n]).tobytes() == many["want_ev"].tobytes()


def test_event_overflow(gpu, many):
    """max_ev below the number of subframes: n_ev counts them all, the records
    kept are distinct members of the full set, nothing lies past max_ev, and the
    channels do not notice."""
    max_ev = 37
    out = _launch(gpu, many["ctx"], many["corr"], many["ch0"].copy(), all_fb=False,
                  max_ev=max_ev)
    assert out["n_ev"] == many["out"]["n_ev"] > 4 * max_ev
    assert out["intact"], "a record written past max_ev"
    full = {e.tobytes() for e in many["want_ev"]}
    kept = {e.tobytes() for e in out["ev"]}
    assert len(out["ev"]) == max_ev and len(kept) == max_ev and kept <= full
    assert out["chans"].tobytes() == many["out"]["chans"].tobytes()
    assert out["last"].tobytes() == many["out"]["fb"][-1].tobytes()


@pytest.mark.skipif(not S.have_ref_chan(), reason="reference build (oracle/_ref) absent")
def test_live_reference_random_streams(gpu):
    rng = np.random.default_rng(17)
    scen = [(int(rng.integers(0, 32)), int(rng.integers(-9000, 9000)), int(rng.choice([1, 20])),
             int(rng.integers(0, 20)), float(rng.uniform(2500, 5000)),
             float(rng.uniform(300, 1500)), float(rng.uniform(-0.1, 0.1)), -1)
            for _ in range(6)]
    n_ms = 22000
    plain = [N.correlations(n_ms, N.nav_bits(8, seed=100 + k), sc[3], sc[4], sc[5],
                            seed=200 + k, q_bias=sc[6]) for k, sc in enumerate(scen)]
    # the same six again with random polarity, first subframe, one flipped bit, one slip
    rng = np.random.default_rng(18)
    varied = []
    for k, sc in enumerate(scen):
        bits = N.nav_bits(8, seed=100 + k, sid0=int(rng.integers(1, 6)))
        bits[int(rng.integers(300, 900))] ^= 1
        slip = (int(rng.integers(4000, 9000)), int(rng.integers(0, 20)))
        varied.append(N.correlations_sched(n_ms, bits, sc[3], [(0, sc[4], sc[5])], seed=300 + k,
                                           q_bias=sc[6], sign=int(rng.choice([-1, 1])),
                                           slip=slip))
    scen = scen + scen
    corr = np.stack(plain + varied, 1)
    ch = _start(gpu, scen)
    fb, ev, _ = gpu.SdrCorrCtx().channel_accum(corr, ch)
    for k, sc in enumerate(scen):
        ref = S.RefSdrChannel(k)
        ref.start(sc[0], sc[1], sc[2])
        rfb, subs, st = ref.run(corr[:, k])
        assert (G.flags_of(fb[:, k]) == G.flags_of(rfb)).all()
        assert np.allclose(fb[:, k]["carrier_nco"], rfb["carrier_nco"], rtol=1e-9)
        assert np.allclose(fb[:, k]["code_nco"], rfb["code_nco"], rtol=1e-9)
        _cmp_state(ch[k], st, gpu)
        mine = ev[ev["chan"] == k]
        assert list(mine["ms"]) == [m for m, _ in subs]
        for (m, s), e in zip(subs, mine):
            assert (e["word_buff"] == s["word_buff"]).all() and e["subframe"] == s["subframe"]


def test_bad_args(gpu):
    ctx = gpu.SdrCorrCtx()
    with pytest.raises(gpu.GnssCorrError):
        ctx.channel_accum_dev(0, 10, None, None, None, None, None, 0, None)
