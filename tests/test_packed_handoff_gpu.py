"""GPU: one packed record from the search to the float tracker, no int8 copy.

A GPS record with two planted PRNs lives on the device only as GNSSCORR_IF_PACKED2 bytes:
gnsscorr_acq_search_dev reads it with GNSSCORR_IF_IQ | GNSSCORR_IF_PACKED2, the results
initialise the sgt channels, and gnsscorr_sgt_track after gnsscorr_sgt_set_packed(1) runs
five closed-loop epochs on the same bytes.  The search result and the epochs must be
byte-equal to the all-int8 pipeline on the unpacked record, and both PRNs must be found on
their planted code phases.
"""
import numpy as np
import pytest

import acq_oracle as A

pytestmark = pytest.mark.gpu
FS, N = 16e6, 16000
PLANTED = [dict(system=0, prn=5, code_phase=321.5, doppler=1500.0, cn0=48.0, data_bits=1),
           dict(system=0, prn=21, code_phase=777.25, doppler=-2500.0, cn0=47.0, data_bits=1)]
PRNS = (5, 13, 21)                                   # 13 is not in the record


def _pipeline(gc, rec_bytes, packed):
    """Search 2 blocks on the device record, hand over, track 5 epochs; returns
    (search results, rows, epochs, channels)."""
    d_if = gc.DevBuf.from_array(rec_bytes)
    assert d_if.ptr % 16 == 0
    freqs = 2.42e6 + np.arange(-8, 9) * 500.0
    G, Bn = len(PRNS), len(freqs)
    acq = gc.AcqCtx(FS, N, max_freqs=32, max_blocks=2, max_codes=4)
    acq.set_codes(np.stack([A.make_ca_table_row(p, FS) for p in PRNS]))
    d_f = gc.DevBuf.from_array(freqs)
    d_gc = gc.DevBuf.from_array(np.arange(G, dtype=np.int32))
    d_gf = gc.DevBuf.from_array(np.tile(np.arange(Bn, dtype=np.int32), (G, 1)))
    d_rows = gc.DevBuf(G * Bn * gc.ACQ_ROW.itemsize)
    d_res = gc.DevBuf(G * gc.ACQ_RESULT.itemsize)
    acq.search_dev(d_if.ptr, 2, Bn, d_f.ptr, G, Bn, d_gc.ptr, d_gf.ptr, d_rows.ptr, d_res.ptr,
                   iq=gc.iq_flags(True, packed=packed))
    acq.sync()
    res, rows = d_res.download(gc.ACQ_RESULT), d_rows.download(gc.ACQ_ROW)
    found = [0, 2]
    trk = gc.SgtCtx(0, samplingFreq=FS)
    ch = trk.init_chans([PRNS[g] for g in found], res["code_phase"][found],
                        res["carr_freq"][found])
    if packed:
        trk.set_packed()
    n = 7 * N
    ep = trk.track(d_if.ptr, 0, n, ch, 5, closed_loop=True)
    return res, rows, ep, ch


def test_packed_record_from_search_to_tracking(gpu):
    gc = gpu
    IF = gc.ifgen(7 * N, PLANTED, fs=FS, seed=0x5EED0021)
    r8, w8, e8, c8 = _pipeline(gc, IF, False)
    rp, wp, ep, cp = _pipeline(gc, gc.pack2(IF), True)
    assert rp.tobytes() == r8.tobytes() and wp.tobytes() == w8.tobytes()
    assert ep.tobytes() == e8.tobytes() and cp.tobytes() == c8.tobytes()
    assert (ep["status"] == 0).all()
    # the planted signals: the code starts (1023 - code_phase) chips into the record
    # (1-based sample `start`).  The search resolves whole samples (one sample of
    # rounding), and the sampled replica's chip edges sit on ceil() of a 15.64-sample grid,
    # up to one more sample from the continuous edges: within 2 samples (1/8 chip, inside
    # the 0.2-chip early-late spacing), as tests/test_b1i_cpu.py bounds its search; and on
    # the 500 Hz bin next to the planted Doppler
    for g, sig in zip((0, 2), PLANTED):
        start = (1023 - sig["code_phase"]) / 1.023e6 * FS + 1
        assert abs(float(rp["code_phase"][g]) - start) <= 2.0, (g, rp["code_phase"][g], start)
        assert abs(float(rp["carr_freq"][g]) - (2.42e6 + sig["doppler"])) <= 250.0
        assert rp["metric"][g] > 2.0 * rp["metric"][1]          # PRN 13 is absent
