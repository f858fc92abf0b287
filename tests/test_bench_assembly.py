"""bench.py's result line on CPU: every section's measurement stubbed with
placeholder numbers, main() must assemble and print the one JSON line with the
contract's keys (a KeyError or a renamed field there would only show on the GPU
box, at the driver's round-end run)."""
import io
import json
import os
import sys
from contextlib import redirect_stdout

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _V(float):
    def __new__(cls, x=123456.789):   # printed like a real measurement (4 digits + exponent)
        return float.__new__(cls, x)


class _D(dict):
    def __missing__(self, k):
        return _V()


class _Dist:
    rank, world, local = 0, 1, 0

    def gather(self, x):
        return [x]

    def barrier(self):
        pass

    def max(self, x):
        return x

    def close(self):
        pass


def test_bench_main_assembles_the_json_line(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu-baseline",
                                      "--steps", "4000", "--warmup", "100"])
    monkeypatch.setattr(bench.gc, "lib", lambda: None)
    monkeypatch.setattr(bench.gc, "device_count", lambda: 1)
    monkeypatch.setattr(bench.gc, "pci_bus_id", lambda d: "0000:00:00.0")
    monkeypatch.setattr(bench.gc, "hip_runtime", lambda: "stub")
    monkeypatch.setattr(bench, "Dist", _Dist)
    lay = lambda: _D(channels=3072, ok=True)  # noqa: E731
    stubs = dict(
        run_acq=lambda *a, **k: _D(records=8, meta=_D(set_codes_ms=1.0), found=8, n_planted=8),
        run_track=lambda *a, **k: _D(steps=20, channels=3072, dumps_ok=True),
        run_track_io=lambda *a, **k: _D(steps=20, cs1_int8=lay(), cs1_packed2=lay(),
                                        rx12_packed2=lay(), host_int8=_D(channels=3072),
                                        host_packed2=_D(channels=3072),
                                        sim_gp2021_12ch=_D(nsamp=8184)),
        run_sgt=lambda *a, **k: _D(channels=3584, ok=True),
        run_fullsky=lambda *a, **k: _D(projection={"world_1_ms": 1.4}, found=12, n_planted=12),
        run_sdr=lambda *a, **k: _D(mw=_D(medium=_D(), weak=_D()), loop=_D(), long=_D(),
                                   bufs=None),
        run_glo_coherent=lambda *a, **k: _D(found=4, n_planted=4),
        run_gps_scilab=lambda *a, **k: _D(found=6, n_planted=6, nb=113, n=16000),
        run_acq_generic=lambda *a, **k: _D(found=8, n_planted=8, fs=38.192e6, n=38192))
    given = []   # (section, steps, warmup) as main() calls them

    def recorded(name, fn):
        def run(dist, dev, steps, warmup, *a, **k):
            given.append((name, steps, warmup))
            return fn(dist, dev, steps, warmup, *a, **k)
        return run
    for k, v in stubs.items():
        monkeypatch.setattr(bench, k, recorded(k, v))
    buf = io.StringIO()
    with redirect_stdout(buf):
        bench.main()
    lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    # the primary line takes --steps as given; every other section stays within the
    # default's counts, whose resident IF (0.4 GB per step in run_track_io) fits the device
    assert given[0] == ("run_acq", 4000, 100) and d["steps"] == 4000
    assert {name for name, _, _ in given} == set(stubs)
    assert all(s <= bench.FULL_MAX_STEPS and w <= bench.FULL_MAX_WARMUP for _, s, w in given[1:])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
                "roofline"):
        assert key in d, key
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(d["roofline"])
    t = d["tracking"]
    assert t["roofline"]["calls_per_launch"] == bench.TRACK_CPL
    assert t["roofline"]["kernel_ms_per_launch"] == t["roofline"]["kernel_ms_per_call"] * \
        bench.TRACK_CPL
    assert t["closed_loop"]["kernel"] == bench.TRACK_KERNEL + " + osg_isr_kernel"
    assert t["closed_loop"]["launches_per_call"] == 2
    for lay_key in ("cs1_int8", "cs1_packed2", "rx12_packed2"):
        r = t["layouts"][lay_key]["roofline"]
        assert {"hbm_GBs", "hbm_frac", "traffic"} <= set(r), lay_key
    # the driver keeps the last ~8000 characters of stdout: the whole line must fit,
    # with room for the cpu_baseline objects (off here) and N=8 ranks; tracking last
    assert len(lines[0]) < 6800, len(lines[0])
    assert list(d)[-1] == "tracking"
    assert "glonass_tracking" in d and "fullsky" in d and "shard_projection" in d["fullsky"]


def test_plain_run_is_the_primary_line_alone(monkeypatch, tmp_path):
    """Without --full only the config-2 fp64 search runs, once, with --steps timed
    steps; the line keeps the contract's keys and --dump-outputs writes every field
    of the results and rows as float64 .npy files."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2",
                                      "--dump-outputs", str(tmp_path / "out")])
    monkeypatch.setattr(bench.gc, "lib", lambda: None)
    monkeypatch.setattr(bench.gc, "device_count", lambda: 1)
    monkeypatch.setattr(bench.gc, "pci_bus_id", lambda d: "0000:00:00.0")
    monkeypatch.setattr(bench.gc, "hip_runtime", lambda: "stub")
    monkeypatch.setattr(bench, "Dist", _Dist)
    monkeypatch.setattr(bench, "write_detail", lambda out: pytest.fail("detail file in a plain run"))
    calls = []
    res = np.zeros((16, 32), bench.gc.ACQ_RESULT)
    res["code_phase"] = np.arange(16 * 32).reshape(16, 32)
    rows = np.zeros((16, 32, 41), bench.gc.ACQ_ROW)
    rows["peak"] = 0.5

    def run_acq(dist, dev, steps, warmup, precision, records=None, keep_outputs=False):
        calls.append((steps, warmup, precision, records, keep_outputs))
        return _D(records=16, dt=0.014, meta=_D(set_codes_ms=1.0), found=8, n_planted=8,
                  outputs=dict(result=res, row=rows))
    monkeypatch.setattr(bench, "run_acq", run_acq)
    for name in ("run_track", "run_track_io", "run_sgt", "run_fullsky", "run_sdr",
                 "run_glo_coherent", "run_gps_scilab", "run_acq_generic", "cpu_baseline_acq"):
        monkeypatch.setattr(bench, name, lambda *a, _n=name, **k: pytest.fail(_n + " in a plain run"))
    buf = io.StringIO()
    with redirect_stdout(buf):
        bench.main()
    assert calls == [(7, 2, bench.gc.ACQ_F64, None, True)]
    lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
                "roofline"):
        assert key in d, key
    assert d["steps"] == 7 and d["ms_per_step"] == pytest.approx(2.0)
    assert d["value"] == pytest.approx(bench.CELLS_PER_SEARCH * 7 * 16 / 0.014)
    assert not set(bench.SECTION_ORDER) & set(d) - {"executed_fp64", "ranks"}
    got = sorted(os.listdir(tmp_path / "out"))
    assert got == sorted([f"result_{f}.npy" for f in ("peak", "second", "metric", "bin",
                                                       "code_phase", "carr_freq")] +
                         [f"row_{f}.npy" for f in ("peak", "second", "argmax", "block")])
    cp = np.load(tmp_path / "out" / "result_code_phase.npy")
    assert cp.dtype == np.float64 and np.array_equal(cp, res["code_phase"])
    assert np.load(tmp_path / "out" / "row_peak.npy").shape == (16, 32, 41)


def test_bench_launches_n_ranks_itself():
    """`bench.py --gpus 2` without torch.distributed.run starts two rank processes
    that meet at the host-group barrier (BENCH_STUB: no library, no GPU)."""
    import subprocess
    env = dict(os.environ, BENCH_STUB="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2",
                        "--steps", "3", "--warmup", "1"], env=env, capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2
    assert sorted(r["rank"] for r in d["ranks"]) == [0, 1]
    assert [r["local_rank"] for r in d["ranks"]] == [0, 1]
    assert len({r["pid"] for r in d["ranks"]}) == 2
    assert d["max_rank"] == 1.0
    assert not any(r["torch_loaded"] for r in d["ranks"])   # no second HIP runtime
