"""Generate tests/golden/sdr_channel_branches.npz from the REFERENCE GPS-SDR Channel.

Same recipe and stored quantities as make_sdr_chan_golden.py (the reference
Channel class compiled by `make -C oracle ref`, driven by oracle/sdr_chan_ref.cpp),
on the streams of sdr_nav_scenarios.BRANCH_SCENARIOS: one stream per Channel
branch that the four SCENARIOS never take.  Stored per stream: the
NCO_Command_S flags of every call, z_count where set, carrier / code NCO every
50th call, the final Channel state, the subframes sent to the ephemeris pipe,
the SHA-256 of the input, and for the C/N0 stream the state after the calls
around each change of the integration length.

Before anything is written the reference's own output must show that each
stream takes its branch (reach) and that no float threshold is decided within
the float bar of the GPU comparison (decidable).
Usage:  python tests/golden/make_sdr_chan_branches_golden.py
"""
import hashlib
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), HERE]
import sdr_nav_scenarios as N  # noqa: E402
import sdr_oracle as S  # noqa: E402
from make_sdr_chan_golden import NCO_EVERY, flags_of  # noqa: E402

IF, CARRIER_LIMIT = 38400, 15000          # IF_FREQUENCY, CARRIER_BINS * CARRIER_SPACING
KILL, RESET_1MS, RESET_20MS = 1, 2, 4     # bits of flags_of()
DATA_BITS = 0x3FFFFFC0                    # d1..d24 of a word as ValidFrameFormat leaves it
MARGIN = 1e-4


def reach(name, flags, carrier_nco, subs, twin=None, lens=None):
    """The defining event of branch stream `name` in one run's output; raises
    AssertionError naming the branch.  flags: flags_of() per call; carrier_nco:
    per call; subs: [(ms, subframe id, word_buff[12])]; twin: (flags, subs) of
    the upright run for "inverted"; lens: `len` in the state snapshots for "cn0".
    Returns the call numbers at which the branch was taken."""
    ms = [m for m, _, _ in subs]
    sid = [s for _, s, _ in subs]
    r1 = np.flatnonzero(flags & RESET_1MS)
    r20 = np.flatnonzero(flags & RESET_20MS)
    kills = np.flatnonzero(flags & KILL)
    if name in ("upright", "inverted"):
        assert len(r1) == 1 and len(subs) >= 2 and len(kills) == 0, (name, r1, ms)
        if name == "inverted":
            tf, ts = twin
            assert (flags == tf).all(), "inverted: flags differ from the upright twin"
            assert ms == [m for m, _, _ in ts] and sid == [s for _, s, _ in ts], (name, ms, sid)
            for (_, _, w), (_, _, tw) in zip(subs, ts):
                # D29*, D30* and the parity bits arrive complemented and stay so
                assert ((np.asarray(w) ^ np.asarray(tw)) & DATA_BITS == 0).all(), name
        return dict(bit_lock=int(r1[0]), subframes=ms)
    if name == "wrap":
        hit = [ms[i] for i in range(len(subs) - 1)
               if sid[i] == 5 and sid[i + 1] == 1 and ms[i + 1] - ms[i] == 6000]
        assert hit, ("wrap: no subframe 5 followed by 1 after 6000 ms", ms, sid)
        return dict(subframe5=hit[0], subframe1=hit[0] + 6000)
    if name == "parity":
        slot = 7 + 3 * 6000 + 1199      # where the damaged third subframe would be emitted
        assert slot not in ms and any(m == slot - 6000 for m in ms), ("parity", ms)
        again = r20[r20 > slot]
        assert len(again) and any(m >= again[0] for m in ms), ("parity: no re-sync", r20, ms)
        return dict(dropped=slot, frame_sync_again=int(again[0]),
                    subframes=[m for m in ms if m >= again[0]])
    if name == "slip":
        assert len(r1) >= 2 and r1[1] > 5000 and any(m > r1[1] for m in ms), ("slip", r1, ms)
        return dict(bit_lock=[int(x) for x in r1[:2]], subframes=ms)
    if name == "carrier":
        assert len(r1) == 0 and len(kills) and kills[0] == 30001, ("carrier", r1, kills[:3])
        return dict(kill=int(kills[0]))
    if name == "qbias":
        assert len(kills) and kills[0] < 15000, ("qbias", kills[:3])
        dev = abs(float(carrier_nco[kills[0]]) - IF)
        assert dev > CARRIER_LIMIT, ("qbias: killed inside the carrier limit", dev)
        return dict(kill=int(kills[0]), carrier_nco=float(carrier_nco[kills[0]]))
    if name == "cn0":
        assert len(kills) == 0 and len(subs) >= 2, ("cn0", kills[:3], ms)
        squeezed = [int(lens[0])] + [int(b) for a, b in zip(lens, lens[1:]) if a != b]
        assert squeezed == [1, 20, 1], ("cn0: len in the snapshots", list(lens))
        return dict(subframes=ms)
    raise KeyError(name)


def decidable(name, tr):
    """Every float threshold of Channel::Error / DLL is cleared by MARGIN
    (relative) in the state after every call, hence on the deciding call and the
    one before it: the carrier limit, P_avg against 8e4, and C/N0 against 37
    (while len != 20) and 39 (while len != 1) under bit lock.  tr: STATE per call."""
    dev = np.abs(np.abs(tr["carrier_nco"] - IF) - CARRIER_LIMIT)
    assert dev.min() >= MARGIN * CARRIER_LIMIT, (name, "carrier limit", dev.min(), dev.argmin())
    # exactly 8e4 is Clear()'s constant after a Kill, not a computed value
    p = tr["P_avg"][tr["P_avg"] != np.float32(8e4)].astype(np.float64)
    assert np.abs(p - 8e4).min() >= MARGIN * 8e4, (name, "P_avg", np.abs(p - 8e4).min())
    for thr, idle_len in ((37.0, 20), (39.0, 1)):
        now = (tr["bit_lock"] != 0) & (tr["len"] != idle_len)
        use = now.copy()
        use[1:] |= now[:-1]
        use[:-1] |= now[1:]
        d = np.abs(tr["cn0"][use].astype(np.float64) - thr)
        assert len(d) == 0 or d.min() >= MARGIN * thr, (name, "cn0", thr, d.min())


def run_reference(k, sc):
    """(corr, fb, subs as (ms, id, words), final state, per-call STATE trace)."""
    corr = N.branch_corr(sc)
    ref = S.RefSdrChannel(k)
    ref.start(*N.branch_start(sc))
    tr = np.zeros(len(corr), ref.STATE)
    fb, subs, st = ref.run(corr, tr)
    assert all(int(s["sv"]) == sc["sv"] for _, s in subs)
    return corr, fb, [(m, int(s["subframe"]), s["word_buff"].copy()) for m, s in subs], st, tr


def snapshot_calls(tr):
    """The calls before and at each change of len."""
    c = np.flatnonzero(np.diff(tr["len"])) + 1
    return np.stack([c - 1, c], 1).reshape(-1)


def check_run(sc, fb, subs, tr, twin):
    name = sc["name"]
    flags = flags_of(fb)
    snaps = snapshot_calls(tr) if name == "cn0" else np.zeros(0, np.int64)
    took = reach(name, flags, fb["carrier_nco"], subs, twin=twin, lens=tr["len"][snaps])
    if name == "cn0":
        took["len"] = [(int(c), int(tr["len"][c])) for c in snaps[1::2]]
    if name == "carrier":   # Error()'s re-arm of the frequency lock at count == 15000
        assert tr["freq_lock"][14999] == 1 and tr["freq_lock"][15000] == 0, "carrier: no re-arm"
        took["freq_lock_rearmed"] = 15000
        took["freq_lock_again"] = 15000 + int(np.flatnonzero(tr["freq_lock"][15000:])[0])
    if name not in ("carrier", "qbias"):
        assert not (flags & KILL).any(), name
    decidable(name, tr)
    return flags, snaps, took


def main():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True)
    names = [sc["name"] for sc in N.BRANCH_SCENARIOS]
    flags, zc, nco, state, sha = [], [], [], [], []
    sub_rows, sub_words = [], []
    snap_calls, snap_state = None, None
    twin = None
    for k, sc in enumerate(N.BRANCH_SCENARIOS):
        corr, fb, subs, st, tr = run_reference(k, sc)
        assert len(corr) == N.BRANCH_MS
        f, snaps, took = check_run(sc, fb, subs, tr, twin)
        if sc["name"] == "upright":
            twin = (f, subs)
        if sc["name"] == "cn0":
            snap_calls = snaps
            snap_state = tr[snaps].copy().view(np.uint8).reshape(len(snaps), -1)
        sha.append(hashlib.sha256(corr.tobytes()).hexdigest())
        flags.append(f)
        zc.append(np.where(fb["set_z_count"] != 0, fb["z_count"], 0).astype(np.int32))
        nco.append(np.stack([fb["carrier_nco"][::NCO_EVERY], fb["code_nco"][::NCO_EVERY]], 1))
        state.append(st)
        for m, sid, w in subs:
            sub_rows.append((k, m, sc["sv"], sid))
            sub_words.append(w)
        print(sc["name"], took)
    np.savez_compressed(os.path.join(HERE, "sdr_channel_branches.npz"), names=np.array(names),
                        n_ms=np.array(N.BRANCH_MS), corr_sha256=np.array(sha),
                        flags=np.stack(flags), z_count=np.stack(zc), nco=np.stack(nco),
                        nco_every=np.array(NCO_EVERY), state=np.stack(state),
                        sub_rows=np.array(sub_rows, np.int32).reshape(-1, 4),
                        sub_words=np.array(sub_words, np.uint32).reshape(-1, 12),
                        snap_stream=np.array(names.index("cn0")), snap_calls=snap_calls,
                        snap_state=snap_state)


if __name__ == "__main__":
    main()
