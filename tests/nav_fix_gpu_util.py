"""GPU test plumbing that tests/test_navfix_gpu.py, test_navglo_gpu.py and test_navb1_gpu.py
share: outputs that start from 0xAA bytes, the set-up of a *_fix_dev call on a padded or
in-place absoluteSample series, and the comparison of its records with a restatement's.

TEST INFRASTRUCTURE ONLY.
"""
import numpy as np

PAD = 3              # epochs of padding after every channel's absoluteSample: NaN, never read


def poison(n, dtype):
    return np.full(n * np.dtype(dtype).itemsize, 0xAA, np.uint8)


def fix_dev(gc, nav, s, launch, in_place=False):
    """launch(d_eph, d_first, abs_sample, epoch_stride, chan_stride, n_epochs, d_n_meas, d_sol,
    d_chan) queues the scene's *_fix_dev call on nav (pointers; the scene's eph and first are
    uploaded here) -> n_meas, sol, chan and the poisoned arrays they started from"""
    n_ch, n_ep = s["abs_sample"].shape
    n_rx, mm = len(s["rx_first"]) - 1, s["cfg"]["max_meas"]
    if in_place:                                               # gnsscorr_sgt_epoch records
        ep = np.zeros((n_ch, n_ep), gc.SGT_EPOCH)
        for f in gc.SGT_EPOCH.names:
            if gc.SGT_EPOCH[f].kind == "f":
                ep[f] = np.nan
        ep["absoluteSample"] = s["abs_sample"]
        d_x = gc.DevBuf.from_array(ep)
        off, es = gc.epoch_field(gc.SGT_EPOCH, "absoluteSample")
        ptr, cs = d_x.ptr + off, n_ep * es
    else:
        padded = np.full((n_ch, n_ep + PAD), np.nan)
        padded[:, :n_ep] = s["abs_sample"]
        d_x = gc.DevBuf.from_array(padded)
        ptr, es, cs = d_x.ptr, 8, padded.strides[0]
    d_eph = gc.DevBuf.from_array(s["eph"])
    d_first = gc.DevBuf.from_array(s["first"])
    p_n, p_sol, p_chan = poison(n_rx, np.int32), poison(n_rx * mm, gc.GPS_FIX_SOL), \
        poison(n_ch * mm, gc.GPS_FIX_CHAN)
    d_n, d_sol, d_chan = (gc.DevBuf.from_array(a) for a in (p_n, p_sol, p_chan))
    launch(d_eph.ptr, d_first.ptr, ptr, es, cs, n_ep, d_n.ptr, d_sol.ptr, d_chan.ptr)
    nav.sync()
    return (d_n.download(np.int32), d_sol.download(gc.GPS_FIX_SOL).reshape(n_rx, mm),
            d_chan.download(gc.GPS_FIX_CHAN).reshape(n_ch, mm),
            p_sol.view(gc.GPS_FIX_SOL).reshape(n_rx, mm), p_chan.view(gc.GPS_FIX_CHAN).reshape(n_ch, mm))


def check_records(S, name, want, n_meas, sol, chan, p_sol, tol=None):
    """S: the scenario module whose GROUPS, TOL (or the table tol) and group_distance hold the
    records to want = (n_meas, sol, chan, written)"""
    tol = S.TOL if tol is None else tol
    w_n, want_sol, want_chan, written = want
    assert n_meas.tolist() == w_n.tolist(), name
    for k in ("status", "n_used"):
        assert np.array_equal(sol[k], want_sol[k]), (name, k)
    assert np.array_equal(chan["used"], want_chan["used"]), name
    assert chan["rawP"].tobytes() == want_chan["rawP"].tobytes(), name
    assert sol[~written].tobytes() == p_sol[~written].tobytes(), name     # rows past n_meas
    for g in S.GROUPS:
        dist = S.group_distance((sol, chan), (want_sol, want_chan), g)
        print(name, g, dist, tol[g])
        assert dist <= tol[g], (name, g, dist, tol[g])
