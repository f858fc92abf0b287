"""GPU test plumbing: the host-array twin of a NavCtx series call run beside its *_dev form
on the same inputs.  Every output starts as sentinel bytes on both sides and is GUARD elements
longer than the call may write, so a comparison sees exactly which bytes each form wrote.

TEST INFRASTRUCTURE ONLY.
"""
import numpy as np

GUARD = 16           # elements past the end of every output: neither form may write them
FILL = 0xAA


def sentinel(count, dtype):
    """count + GUARD elements of dtype, every byte FILL"""
    return np.full((count + GUARD) * np.dtype(dtype).itemsize, FILL, np.uint8).view(dtype)


def intact(a):
    return bool((a.view(np.uint8) == FILL).all())


def twin_and_dev(gc, nav, name, series, mid, outs):
    """nav.<name>_dev on uploaded copies of `series` (each [n_ch, n_epochs] fp64) and the
    exported gnsscorr_nav_<name> on the arrays themselves.  mid: the arguments between n_ch
    and the outputs; outs: (dtype, count) of each output, count 0 included.  Asserts that the
    twin's outputs equal the device form's byte for byte and that neither wrote past `count`;
    returns the twin's outputs."""
    series = [np.ascontiguousarray(x, np.float64) for x in series]
    n_ch, n_ep = series[0].shape
    geom = [8, 8 * n_ep, n_ep, n_ch, *mid]
    d_in = [gc.DevBuf.from_array(x) for x in series]
    d_out = [gc.DevBuf.from_array(sentinel(n, dt)) for dt, n in outs]
    getattr(nav, name + "_dev")(*[d.ptr for d in d_in], *geom, *[d.ptr for d in d_out])
    nav.sync()
    dev = [d.download(dt) for d, (dt, _) in zip(d_out, outs)]
    host = [sentinel(n, dt) for dt, n in outs]
    rc = getattr(nav, "_" + name)(nav.h, *[x.ctypes.data for x in series], *geom,
                                  *[h.ctypes.data for h in host])
    assert rc == 0, gc.lib().gnsscorr_last_error()
    for i, (h, d, (_, n)) in enumerate(zip(host, dev, outs)):
        assert h[:n].tobytes() == d[:n].tobytes(), (name, i)
        assert intact(h[n:]) and intact(d[n:]), (name, i)
    return [h[:n] for h, (_, n) in zip(host, outs)]
