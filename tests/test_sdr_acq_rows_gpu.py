"""GPU parity, row by row: everything the GPS-SDR int16 acquisition kernels
(sdr_acq.hip) write, not only the winning cell.

The result of a search is six integers from one cell; the kernels compute 4 /
40 / 1240 spectra of 2048 cells per record and 2048 (strong) or 20480 (medium,
weak) cells per row.  Here the spectra are read back cell by cell
(gnsscorr_sdr_acq_read_spectra) and the per-row (magnitude, index) table whole
(gnsscorr_sdr_acq_read_rows) and compared with the C oracle (oracle/sdr_acq.c:
sdro_prep_if, sdro_prep_rows, sdro_acq_*_rows), which test_sdr_acq_rows_cpu.py
pins to the reference build.  Every comparison is exact equality of whole
integer arrays.  Inputs (sdr_rows_cases.py) are chosen so that the saturating
arm changes rows, the weak search's column shift crosses columns 2047/0 and
1023/1024 at lcv = +-100, and equal maxima occur across rows and within a row.

Reference: REALTIME_RECEIVERS/GPS/GPS_SDR_REAL_TIME_GPS_RECEIVER/objects/
acquisition.cpp:191-236, :244-301, :309-425, :433-570.
"""
import functools

import numpy as np
import pytest

import sdr_oracle as S
import sdr_rows_cases as K

pytestmark = pytest.mark.gpu
N = K.N
MS = {"strong": 1, "medium": 10, "weak": 310}


def _type(gpu, kind):
    return {"strong": gpu.SDR_ACQ_STRONG, "medium": gpu.SDR_ACQ_MEDIUM,
            "weak": gpu.SDR_ACQ_WEAK}[kind]


@pytest.fixture(scope="module")
def o(oracle):
    return S.OracleSDR()


@pytest.fixture(scope="module")
def codes(o):
    return o.prn_codes()


def _eq(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} values differ, first at "
                             f"{bad[0].tolist()}: got {got[tuple(bad[0])]}, "
                             f"oracle {want[tuple(bad[0])]}")


def _same_results(got, want):
    assert got.tobytes() == np.asarray(want, S.RESULT).tobytes(), (got, want)


def _prep(gpu, ctx, kind, bufs):
    """doPrepIF of kind's length for bufs [n_rec, ms*2048, 2] through the device API."""
    b = np.ascontiguousarray(bufs, np.int16).reshape(-1, MS[kind] * N, 2)
    d = gpu.DevBuf.from_array(b)
    ctx.prep_dev(_type(gpu, kind), d.ptr, b.shape[0])
    ctx.sync()


def _search(gpu, ctx, kind, n_rec, svs, dmin, dmax):
    """search_dev over the context's row store; returns (results, table)."""
    svs = np.ascontiguousarray(svs, np.int32)
    d_s = gpu.DevBuf.from_array(svs)
    d_r = gpu.DevBuf(n_rec * len(svs) * gpu.SDR_RESULT.itemsize)
    ctx.search_dev(_type(gpu, kind), n_rec, len(svs), d_s.ptr, d_r.ptr, dmin, dmax)
    table = ctx.read_rows(n_rec, len(svs), S.n_rows(kind, dmin, dmax))
    res = d_r.download(np.uint8).view(gpu.SDR_RESULT).reshape(n_rec, len(svs))
    return res, table


def _store(gpu, ctx, rec):
    return ctx.read_spectra(gpu.SDR_ACQ_WEAK, rec, 0, S.ROWS)


def _check_search(gpu, ctx, o, codes, kind, stores, svs, dmin, dmax, sat):
    """One medium / weak search over the context's store against the oracle's
    over `stores` (one per record): the whole table, and the results against a
    scan of the table."""
    res, table = _search(gpu, ctx, kind, len(stores), svs, dmin, dmax)
    want = np.stack([o.search_rows(kind, st, codes, svs, dmin, dmax, saturate=sat)
                     for st in stores])
    _eq(table, want, f"{kind} table {dmin}..{dmax} sat={sat}")
    _same_results(res, S.scan_rows(kind, want, svs, dmin))
    return want


# ---- inputs: two records with different contents -----------------------------------
@functools.lru_cache(maxsize=None)
def _records(name):
    """[2, 310*2048, 2] int16."""
    if name == "planted":
        return K.planted()
    if name == "int8":
        return np.stack([S.make_long_buffer(
            [dict(prn=9 + r, code_phase=123.0 + 300 * r, doppler=-6400.0 + 9000 * r, amp=4.0)],
            310, seed=70 + r, amp_noise=6.0) for r in range(2)])
    amp = {"u12000": 12000, "u20000": 20000, "full": 32768}[name]
    return np.stack([K.uniform(amp, 310, 80 + amp % 97 + r) for r in range(2)])


@functools.lru_cache(maxsize=None)
def _oracle_stores(name, sat):
    """The oracle's row stores after a 310-ms prep of _records(name)."""
    o = S.OracleSDR()
    out = []
    for b in _records(name):
        rows = o.new_rows()
        o.prep_rows(rows, b, 310, saturate=sat)
        out.append(rows)
    return out


@pytest.fixture(scope="module")
def weak_ctx(gpu):
    """weak_ctx(name, sat): a context whose store holds the 310-ms prep of
    _records(name), made once per (name, sat) and closed with the module."""
    made = {}

    def get(name, sat):
        if (name, sat) not in made:
            made[name, sat] = gpu.SdrAcqCtx(S.IF_SDR, saturate=sat)
            _prep(gpu, made[name, sat], "weak", _records(name))
        return made[name, sat]

    yield get
    for ctx in made.values():
        ctx.close()


# ---- a. the forward spectra, cell by cell ---------------------------------------------
@pytest.mark.parametrize("sat", [False, True])
@pytest.mark.parametrize("name", ["int8", "u20000", "full"])
def test_spectra_cell_by_cell(gpu, o, name, sat):
    """4 + 1240 + 1240 rows x 2048 cells x 2 records."""
    bufs = _records(name)
    ctx = gpu.SdrAcqCtx(S.IF_SDR, saturate=sat)
    ctx.strong(bufs[:, :N], [0], 0, 1000)
    for r in range(2):
        _eq(ctx.read_spectra(gpu.SDR_ACQ_STRONG, r, 0, 4), o.prep_if(bufs[r, :N], saturate=sat),
            f"strong spectra rec {r}")
        _eq(ctx.read_spectra(gpu.SDR_ACQ_STRONG, r, 2, 2),
            o.prep_if(bufs[r, :N], saturate=sat)[2:], f"strong spectra rec {r} rows 2..3")
    _prep(gpu, ctx, "weak", bufs)
    stores = [st.copy() for st in _oracle_stores(name, sat)]
    for r in range(2):
        _eq(_store(gpu, ctx, r), stores[r], f"310-ms store rec {r}")
    # a 10-ms prep (of other samples) over it: rows 0..39 new, 40..1239 kept
    tail = bufs[:, -10 * N:]
    _prep(gpu, ctx, "medium", tail)
    for r in range(2):
        o.prep_rows(stores[r], tail[r], 10, saturate=sat)
        assert not np.array_equal(stores[r][:40], _oracle_stores(name, sat)[r][:40])
        _eq(_store(gpu, ctx, r), stores[r], f"store after the 10-ms prep rec {r}")


@pytest.mark.parametrize("sat", [False, True])
def test_spectra_fresh_medium_prep_and_store_growth(gpu, o, sat):
    """The 40 rows of a 10-ms prep on a new context (the rest zero); then the
    store grows from 1 to 2 records and keeps what record 0 held."""
    bufs = _records("full")
    ctx = gpu.SdrAcqCtx(S.IF_SDR, saturate=sat)
    st0 = o.new_rows()
    _prep(gpu, ctx, "medium", bufs[:1, :10 * N])
    o.prep_rows(st0, bufs[0, :10 * N], 10, saturate=sat)
    _eq(_store(gpu, ctx, 0), st0, "fresh 10-ms store")
    assert not st0[40:].any() and st0[:40].any()
    with pytest.raises(gpu.GnssCorrError):
        _store(gpu, ctx, 1)
    _prep(gpu, ctx, "weak", bufs[1:])                 # record 0 <- the 310 ms of bufs[1]
    o.prep_rows(st0, bufs[1], 310, saturate=sat)
    _eq(_store(gpu, ctx, 0), st0, "310-ms store, one record")
    two = _records("u20000")[:, 5 * N:15 * N]
    _prep(gpu, ctx, "medium", two)                    # grows to 2 records
    st1 = o.new_rows()
    o.prep_rows(st0, two[0], 10, saturate=sat)
    o.prep_rows(st1, two[1], 10, saturate=sat)
    _eq(_store(gpu, ctx, 0), st0, "record 0 after the growth")
    _eq(_store(gpu, ctx, 1), st1, "record 1 after the growth")
    assert st0[40:].any() and not st1[40:].any()


# ---- b. the strong table -----------------------------------------------------------------
STRONG_RANGES = ((-15000, 15000), (-100000, -99000), (100000, 101000), (-999, 1999))


@pytest.mark.parametrize("name,sat", [("int8", False), ("full", False), ("full", True),
                                      ("u20000", True)])
def test_strong_table(gpu, o, codes, name, sat):
    """(120 + 4 + 4 + 8) rows x 3 svs x 2 records, each the maximum of 2048 cells."""
    bufs = _records(name)[:, :N]
    svs = np.array([13, 0, 31], np.int32)
    ctx = gpu.SdrAcqCtx(S.IF_SDR, saturate=sat)
    for dmin, dmax in STRONG_RANGES:
        res = ctx.strong(bufs, svs, dmin, dmax)
        n = S.n_rows("strong", dmin, dmax)
        table = ctx.read_rows(2, 3, n)
        want = np.stack([o.strong_rows(o.prep_if(b, saturate=sat), codes, svs, dmin, dmax,
                                       saturate=sat) for b in bufs])
        _eq(table, want, f"strong table {dmin}..{dmax}")
        _same_results(res, S.scan_rows("strong", want, svs, dmin))
        assert len(np.unique(want[..., 0])) > n           # rows do differ from each other


# ---- c. medium and weak tables, one lcv at a time ------------------------------------------
@pytest.mark.parametrize("lcv", K.LCVS)
@pytest.mark.parametrize("sat", [False, True])
@pytest.mark.parametrize("name", ["planted", "u12000", "full"])
def test_medium_weak_tables(gpu, o, codes, weak_ctx, name, sat, lcv):
    """(4 + 8) rows x 2 svs x 2 records, each the maximum of 20480 cells."""
    ctx, stores = weak_ctx(name, sat), _oracle_stores(name, sat)
    svs = np.array(K.PLANT_SVS, np.int32)
    for kind in ("weak", "medium"):
        want = _check_search(gpu, ctx, o, codes, kind, stores, svs, *K.one_lcv(kind, lcv), sat)
        assert (want[..., 0] > 0).all()
    if name == "planted" and abs(lcv) == 100:
        # the planted peaks cross column 2047/0 (sv 0) and 1023/1024 (sv 1)
        rec = 0 if lcv > 0 else 1
        t = o.search_rows("weak", stores[rec], codes, svs, *K.one_lcv("weak", lcv), saturate=sat)
        for s, boundary in enumerate((0, 1024)):
            row = int(np.argmax(t[s, :, 0]))
            cols = K.pass_columns(o, lcv, (row >> 1) & 3, int(t[s, row, 1]) % N)
            assert K.straddles(cols, boundary), (s, row, cols)


@pytest.mark.parametrize("sat", [False, True])
def test_weak_over_a_medium_prep_reads_zero_rows(gpu, o, codes, sat):
    """After a 10-ms prep only rows 0..39 are set: the weak search's passes
    read zero rows for lcv2 >= 1 and rows 20..39 as if they were its own."""
    bufs = _records("full")[:, :10 * N]
    ctx = gpu.SdrAcqCtx(S.IF_SDR, saturate=sat)
    _prep(gpu, ctx, "medium", bufs)
    stores = []
    for b in bufs:
        stores.append(o.new_rows())
        o.prep_rows(stores[-1], b, 10, saturate=sat)
    svs = np.array([0, 21], np.int32)
    want = _check_search(gpu, ctx, o, codes, "weak", stores, svs, 0, 1000, sat)
    assert (want[:, :, :2, 0] > 0).all() and not want[:, :, 2:].any()
    _check_search(gpu, ctx, o, codes, "medium", stores, svs, -1000, 1000, sat)


# ---- d. equal maxima across rows ------------------------------------------------------------
def test_equal_rows_strong(gpu, o, codes):
    imp = K.impulse(1)
    other = _records("int8")[0, :N]
    svs = np.array([13, 2], np.int32)
    ctx = gpu.SdrAcqCtx()
    res = ctx.strong(np.stack([imp, other]), svs)
    table = ctx.read_rows(2, 2, 120)
    want = np.stack([o.strong_rows(o.prep_if(b), codes, svs) for b in (imp, other)])
    _eq(table, want, "strong table, impulse record")
    assert (table[0, 0] == (2033480, 90)).all()           # 120 equal rows
    assert (table[0, 1] == table[0, 1, 0]).all() and table[0, 1, 0, 0] > 0
    _same_results(res, S.scan_rows("strong", want, svs, -15000))
    assert (res[0]["row"] == 0).all() and (res[0]["doppler"] == -15000).all()
    assert res[0, 0]["code_phase"] == N - 90 and res[0, 0]["magnitude"] == 2033480


def test_equal_rows_medium_weak(gpu, o, codes):
    """Medium: 68 equal rows (more than the 64 lanes of the row scan).  Weak:
    136 rows whose maximum is held by rows 60/61, 68/69 and 76/77."""
    imp = K.impulse(310)
    ctx = gpu.SdrAcqCtx()
    _prep(gpu, ctx, "weak", imp[None])
    store = o.new_rows()
    o.prep_rows(store, imp, 310)
    svs = np.array([13], np.int32)
    want = _check_search(gpu, ctx, o, codes, "medium", [store], svs, -8000, 8000, False)
    assert want.shape == (1, 1, 68, 2) and (want == want[0, 0, 0]).all() and want[0, 0, 0, 0] > 0
    res, _ = _search(gpu, ctx, "medium", 1, svs, -8000, 8000)
    assert res[0, 0]["row"] == 0 and res[0, 0]["doppler"] == -8000 + (want[0, 0, 0, 1] // N) * 25
    want = _check_search(gpu, ctx, o, codes, "weak", [store], svs, *K.IMPULSE_WEAK_RANGE, False)
    top = np.flatnonzero(want[0, 0, :, 0] == want[0, 0, :, 0].max())
    assert list(top) == [60, 61, 68, 69, 76, 77]
    res, _ = _search(gpu, ctx, "weak", 1, svs, *K.IMPULSE_WEAK_RANGE)
    assert res[0, 0]["row"] == 60


# ---- e. equal maxima within a row -----------------------------------------------------------
@pytest.mark.parametrize("kind", ["strong", "medium", "weak"])
def test_equal_cells_within_a_row(gpu, o, codes, kind):
    """Rows of sparse +-1 records whose maximum occurs at two or more cells
    (found on the oracle, sdr_rows_cases.ties): the index is the first of them."""
    ties = K.ties(kind)
    assert len(ties) >= (3 if kind == "strong" else 1)
    if kind == "strong":
        assert any(f["inverted"] for f in ties)
    ctx = gpu.SdrAcqCtx()
    for f in ties:
        buf = K.sparse(f["seed"], MS[kind])
        svs = np.array([f["sv"]], np.int32)
        dmin, dmax = K.one_lcv(kind, f["lcv"])
        row = (f["lcv2"] * 2 + f["k"]) if kind == "weak" else f["lcv2"]
        if kind == "strong":
            ctx.strong(buf, svs, dmin, dmax)
            table = ctx.read_rows(1, 1, 4)
            want = o.strong_rows(o.prep_if(buf), codes, svs, dmin, dmax)[None]
        else:
            _prep(gpu, ctx, kind, buf[None])
            store = o.new_rows()
            o.prep_rows(store, buf, MS[kind])
            _, table = _search(gpu, ctx, kind, 1, svs, dmin, dmax)
            want = o.search_rows(kind, store, codes, svs, dmin, dmax)[None]
        assert tuple(want[0, 0, row]) == (f["mag"], f["cells"][0])
        _eq(table, want, f"{kind} table with a tied row {f}")


# ---- f. the read-back calls' argument checks ------------------------------------------------
def test_read_back_argument_checks(gpu):
    ctx = gpu.SdrAcqCtx()
    S_, M_, W_ = gpu.SDR_ACQ_STRONG, gpu.SDR_ACQ_MEDIUM, gpu.SDR_ACQ_WEAK
    bad = pytest.raises(gpu.GnssCorrError)
    with bad:                                            # before any search
        ctx.read_rows(1, 1, 4)
    for t in (S_, M_, W_):                               # before any search / prep
        with bad:
            ctx.read_spectra(t, 0, 0, 1)
    z = np.zeros((2, N, 2), np.int16)
    z[:, 1] = (300, -200)
    ctx.strong(z, [0, 1], 0, 2000)                       # 2 x 2 x 8 pairs
    assert ctx.read_rows(2, 2, 8).shape == (2, 2, 8, 2)
    assert ctx.read_rows(1, 1, 1).shape == (1, 1, 1, 2)
    with bad:
        ctx.read_rows(2, 2, 9)                           # past what the search left
    with bad:
        ctx.read_rows(0, 2, 8)
    assert ctx.read_spectra(S_, 1, 3, 1).shape == (1, N, 2)
    for t, rec, row0, n in ((S_, 2, 0, 1), (S_, -1, 0, 1), (S_, 0, 4, 1), (S_, 0, 3, 2),
                            (S_, 0, -1, 2), (S_, 0, 0, 0), (S_, 0, 0, 5), (3, 0, 0, 1),
                            (-1, 0, 0, 1), (M_, 0, 0, 1), (S_, 0, 0, -1),
                            (S_, 0, 2**31 - 1, 2**31 - 1)):
        with bad:
            ctx.read_spectra(t, rec, row0, n)
    ctx.strong(z[:1], [0], 0, 1000)                      # a smaller search replaces it
    with bad:
        ctx.read_rows(2, 2, 8)
    with bad:
        ctx.read_spectra(S_, 1, 0, 1)
    ctx.acquire(M_, np.zeros((10 * N, 2), np.int16), [0], 0, 0)
    assert ctx.read_rows(1, 1, 4).shape == (1, 1, 4, 2)
    with bad:
        ctx.read_rows(1, 1, 5)
    assert not ctx.read_spectra(W_, 0, 1239, 1).any()
    assert ctx.read_spectra(M_, 0, 0, S.ROWS).shape == (S.ROWS, N, 2)
    for rec, row0, n in ((1, 0, 1), (0, 1240, 1), (0, 1239, 2), (0, -1, 1), (0, 0, 1241)):
        with bad:
            ctx.read_spectra(W_, rec, row0, n)
