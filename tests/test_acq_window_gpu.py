"""GPU: the edges of the second-peak window, on every acquisition engine.

Every engine reports, per row, `second` = the maximum outside the open circular
window (argmax - spc, argmax + spc) (acquisition.sci:147-166), and several compute it
in one pass from a per-thread top-2 that is exact only while the window is narrower
than the distance between one thread's samples.  The scenes of
tests/acq_window_scenes.py put the peak on sample p (both ends of the row, next to
them, one interior) and a copy exactly d samples to either side, d on the engine's
own threshold between the one pass and the exact pass, and 16:

  spc = d      d == spc counts, on both edges (`mirror`: the stronger copy at N - spc)
  spc = d + 1  d == spc - 1 does not, and the exact-pass branch runs

held to oracle/acq_oracle.py through test_acq_gpu.check_rows at the project's
tolerances (fp64: 1e-6 / 1e-9 class, decisions exact; fp32: 1e-4 of the row peak).  A
wrongly included or excluded copy moves `second` by at least 0.1 of the peak
(tests/test_acq_window_cpu.py shows that for every scene).

Tie rules: best-of-blocks keeps a later block unless the kept maximum is strictly
larger (acquisition.sci:126-132), so bit-identical blocks report the last one; a group
naming one frequency twice reports the first of the identical rows (Scilab's max).
"""
import numpy as np
import pytest

import acq_oracle as A
import acq_window_scenes as W
from test_acq_gpu import check_rows

pytestmark = pytest.mark.gpu
MODES = ["best", "noncoherent"]


def _make_ctx(gpu, engine, max_blocks=W.N_BLOCKS):
    e = W.ENGINES[engine]
    prec = gpu.ACQ_F32 if engine.startswith("f32") else gpu.ACQ_F64
    with pytest.MonkeyPatch.context() as mp:     # the engine choice is read at create
        for k, v in e.get("env", {}).items():
            mp.setenv(k, v)
        ctx = gpu.AcqCtx(e["fs"], e["n"], max_freqs=4, max_blocks=max_blocks, max_codes=1,
                         precision=prec)
    ctx.set_codes(W.code_row(e["n"]))
    return ctx


@pytest.fixture(scope="module")
def ctxs(gpu):
    """One context per engine for the whole module (3 blocks: the tie tests)."""
    made = {}

    def get(engine):
        if engine not in made:
            made[engine] = _make_ctx(gpu, engine, max_blocks=3)
        return made[engine]
    yield get
    for c in made.values():
        c.close()


def _window_case(gpu, ctx, engine, mode, case):
    e = W.ENGINES[engine]
    p, d, spc, mirror = case
    nc = mode == "noncoherent"
    f64 = not engine.startswith("f32")
    IF = W.scene_if(e["n"], p, d, mirror)
    res, rows = ctx.search(IF, W.N_BLOCKS, W.FREQS, [0], W.GF, spc=spc,
                           mode=gpu.ACQ_NONCOHERENT if nc else gpu.ACQ_BEST_OF_BLOCKS)
    ref, ref_rows = W.reference(e["fs"], e["n"], p, d, spc, mirror, nc)
    for b in range(3):
        print(f"[{engine} {mode} {W.case_id(case)}] row {b}: second/peak "
              f"{rows[0, b]['second'] / rows[0, b]['peak']:.6f} oracle "
              f"{ref_rows[0][b]['second'] / ref_rows[0][b]['peak']:.6f}")
    check_rows(res, rows, ref, ref_rows, f64, label=f"{engine}-{mode}-{W.case_id(case)}")
    # the peaks are clear (4 x any other sample), so the decisions hold in fp32 too
    assert (rows["argmax"] == p).all() and (rows["block"] == (-1 if nc else 1)).all()
    assert res[0]["bin"] == 1 and res[0]["code_phase"] == p + 1
    return res, rows


def _window_params(engine):
    return [pytest.param(c, id=W.case_id(c)) for c in W.cases(engine)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", _window_params("f64-16368"))
def test_window_f64_16368(gpu, ctxs, mode, case):
    _window_case(gpu, ctxs("f64-16368"), "f64-16368", mode, case)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", _window_params("f64-16000"))
def test_window_f64_16000(gpu, ctxs, mode, case):
    _window_case(gpu, ctxs("f64-16000"), "f64-16000", mode, case)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", _window_params("f32-16368"))
def test_window_f32(gpu, ctxs, mode, case):
    """best: acq_corr_pipe_kernel (spc <= 264) or acq_corr_kernel's exact pass (above);
    noncoherent: acq_corr_kernel, with and without the exact pass."""
    _window_case(gpu, ctxs("f32-16368"), "f32-16368", mode, case)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", _window_params("mixed-5000"))
def test_window_generic_mixed_radix_5000(gpu, ctxs, mode, case):
    _window_case(gpu, ctxs("mixed-5000"), "mixed-5000", mode, case)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", _window_params("bluestein-4111"))
def test_window_generic_bluestein_4111(gpu, ctxs, mode, case):
    _window_case(gpu, ctxs("bluestein-4111"), "bluestein-4111", mode, case)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", _window_params("m4-16368"))
def test_window_generic_four_step_16368(gpu, ctxs, mode, case):
    """The generic engine forced at 16368 (the {3, 16, 11, 31} four-step plan): the fused
    column top-2 (spc <= 24), the generic statistics' one pass (<= 504), their two."""
    _window_case(gpu, ctxs("m4-16368"), "m4-16368", mode, case)


def test_f32_power_row_beside_a_wide_window(gpu, ctxs):
    """The power-row dump (acq_corr_kernel<BEST_OF_BLOCKS, DUMP>) between two searches
    at spc = 265: the dumped row equals the oracle's, and the searches are unmoved."""
    e = W.ENGINES["f32-16368"]
    ctx = ctxs("f32-16368")
    case = (e["n"] - 1, 264, 265, False)
    first = _window_case(gpu, ctx, "f32-16368", "best", case)
    IF = W.scene_if(e["n"], case[0], case[1])
    got = ctx.power_row(IF, W.N_BLOCKS, 1, 0.0, 0)
    ref = A.power_rows(IF, e["fs"], W.code_row(e["n"])[0], 0.0)[1]
    assert np.abs(got - ref).max() < 2e-5 * ref.max()
    assert int(np.argmax(got)) == case[0]
    again = _window_case(gpu, ctx, "f32-16368", "best", case)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("spc", [264, 265])
def test_window_records(gpu, ctxs, spc, mode):
    """set_records(2) on the 16368 plan: record 0 peaks on the last sample, record 1 on
    the first; both equal their single-record searches byte for byte, and the oracle."""
    e = W.ENGINES["f64-16368"]
    n, d = e["n"], 264
    ps = (n - 1, 0)
    m = gpu.ACQ_NONCOHERENT if mode == "noncoherent" else gpu.ACQ_BEST_OF_BLOCKS
    batch = _make_ctx(gpu, "f64-16368", max_blocks=2 * W.N_BLOCKS)
    batch.set_records(2)
    IF = np.concatenate([W.scene_if(n, p, d) for p in ps])
    res, rows = batch.search(IF, W.N_BLOCKS, W.FREQS, [0], W.GF, spc=spc, mode=m)
    assert res.shape == (2, 1) and rows.shape == (2, 1, 3)
    for r, p in enumerate(ps):
        one_res, one_rows = _window_case(gpu, ctxs("f64-16368"), "f64-16368", mode,
                                         (p, d, spc, False))
        assert res[r].tobytes() == one_res.tobytes(), f"record {r} results"
        assert rows[r].tobytes() == one_rows.tobytes(), f"record {r} rows"
        ref, ref_rows = W.reference(e["fs"], n, p, d, spc, False, mode == "noncoherent")
        check_rows(res[r], rows[r], ref, ref_rows, True, label=f"records[{r}]-spc{spc}-{mode}")
    batch.close()


@pytest.mark.parametrize("case", [pytest.param(c, id=f"p{c[0]}-dist{c[1]}{'-mirror' if c[2] else ''}")
                                  for c in W.padded_cases()])
def test_window_zero_padded(gpu, case):
    """set_zero_padded with keep < L: the window is circular in keep, so a copy across
    the wrap at keep at distance spc counts and one at spc - 1 does not."""
    p, dist, mirror = case
    ctx = gpu.AcqCtx(W.PAD_FS, W.PAD_L, max_freqs=4, max_blocks=1, max_codes=1)
    ctx.set_zero_padded(W.PAD_KEEP)
    ctx.set_codes_padded(W.code_row(W.PAD_KEEP))
    res, rows = ctx.search(W.padded_if(p, dist, mirror), 1, W.FREQS, [0], W.GF, spc=W.PAD_SPC)
    ref, ref_rows = W.padded_reference(p, dist, mirror)
    check_rows(res, rows, ref, ref_rows, True, label=f"padded-window-p{p}-dist{dist}")
    assert (rows["argmax"] == p).all()
    ctx.close()


TIE_ENGINES = ["f64-16368", "f64-16000", "f32-16368"]


@pytest.mark.parametrize("n_blocks", [2, 3])
@pytest.mark.parametrize("engine", TIE_ENGINES)
def test_tied_blocks_report_the_last_block(gpu, ctxs, engine, n_blocks):
    e = W.ENGINES[engine]
    res, rows = ctxs(engine).search(W.tied_if(e["n"], n_blocks), n_blocks, W.FREQS, [0], W.GF)
    ref, ref_rows = W.tied_reference(e["fs"], e["n"], n_blocks)
    assert all(r["block"] == n_blocks - 1 for r in ref_rows[0])
    assert (rows["block"] == n_blocks - 1).all(), rows["block"]
    check_rows(res, rows, ref, ref_rows, not engine.startswith("f32"),
               label=f"tied-blocks-{engine}-{n_blocks}")
    assert (rows["argmax"] == 4321).all() and res[0]["bin"] == 1


@pytest.mark.parametrize("engine", TIE_ENGINES)
def test_repeated_frequency_reports_the_first_bin(gpu, ctxs, engine):
    e = W.ENGINES[engine]
    gf = ((1, 1, 0),)
    res, rows = ctxs(engine).search(W.tied_if(e["n"], 2), 2, W.FREQS, [0], np.array(gf))
    ref, ref_rows = W.tied_reference(e["fs"], e["n"], 2, group_freq=gf)
    assert ref[0]["bin"] == 0
    assert rows[0, 0].tobytes() == rows[0, 1].tobytes()
    assert res[0]["bin"] == 0 and res[0]["carr_freq"] == 0.0
    check_rows(res, rows, ref, ref_rows, not engine.startswith("f32"),
               label=f"repeated-frequency-{engine}")
