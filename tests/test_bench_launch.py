"""bench.py --gpus N from a bare launch: the process (which has not touched the GPU) starts the N ranks under
torch.distributed.run as a child, relays rank 0's JSON line and leaves with the children's status.  A plain run times
the headline alone (exactly K steps) and --dump-outputs writes what its last step computed; --full adds the rest."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bare_launch_composes_the_torchrun_command(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    seen = {}

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env

        class R:
            returncode = 7
        return R()

    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "20", "--warmup", "5"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as ei:
        bench.main()
    assert ei.value.code == 7                                # the children's status is the exit status
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--master-addr" in cmd and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-6:] == ["--gpus", "4", "--steps", "20", "--warmup", "5"] and cmd[-7].endswith("bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


@pytest.mark.gpu
def test_bare_launch_two_ranks_on_one_gpu_prints_one_json_line():
    fake = os.path.join(ROOT, "tests", "fake_rccl", "_build", "libfake_rccl.so")
    assert os.path.exists(fake)
    # two ranks on the ONE test GPU: gloo for torch.distributed, the librccl stand-in for the library's own collective
    import tempfile
    import time
    counter = tempfile.NamedTemporaryFile(prefix="bench_gen_", suffix=".txt", delete=False).name
    env = dict(os.environ, BENCH_BACKEND="gloo", BENCH_ONE_DEVICE="1", VBNMF_RCCL_LIB=fake, BENCH_GEN_COUNTER=counter)
    env.pop("WORLD_SIZE", None)
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--small", "--steps", "5", "--warmup", "2",
                        "--no-cpu", "--no-ml", "--full"], env=env, capture_output=True, text=True, timeout=900)
    print(f"two-rank rehearsal: {time.perf_counter() - t0:.1f} s wall")
    assert p.returncode == 0, p.stderr[-2000:]
    # ONE generation of each synthetic matrix per node, whatever the number of ranks: the node's local
    # rank 0 generates, the others map its arrays
    gens = sorted(ln.split()[0] for ln in open(counter).read().splitlines())
    os.unlink(counter)
    assert gens == ["c3s", "c5s"], gens
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 5 and out["value"] > 0
    assert "value_host_stepped" in out and out["warmup_effective"] >= 2 and "setup" in out
    # config C4 and C5 ride in the same line (VERDICT r03 Next #3)
    sweep = out["rank_sweep"]
    assert "error" not in sweep, sweep
    assert sweep["wall_s"] > 0 and sweep["iterations_by_rank"] and set(sweep["iterations_by_rank"]) <= {str(r) for r in range(2, 7)}
    assert len(sweep["per_process"]) == 2 and sorted(r for q in sweep["per_process"] for r in q["ranks"]) == list(range(2, 7))
    split = sweep["one_unit_at_a_time"]                       # the stepping / set-up split comes from a second call, one unit at a time
    assert split["wall_s"] > 0 and all(q["stepping_s"] > 0 and q["setup_s"] > 0 for q in split["per_process"])
    cells = out["cells_partitioned"]
    assert "error" not in cells, cells
    assert cells["value"] > 0 and cells["allreduce_ms"] > 0 and "device-driven" in cells["loop"]
    assert 0 < cells["roofline"]["hbm"]["frac"] < 1 and 0 < cells["roofline"]["fp64"]["frac"] < 1


@pytest.mark.gpu
def test_plain_run_on_the_device_dumps_its_last_step(tmp_path):
    """A plain run on the small workload: one JSON line with the headline fields, the outputs of exactly K device-driven
    steps, and the same outputs from a second run with the same arguments."""
    runs = []
    for d in ("a", "b"):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--small", "--steps", "6", "--warmup", "2",
                            "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, p.stdout[-2000:]
        runs.append(json.loads(lines[0]))
    out = runs[0]
    assert out["steps"] == 6 and out["value"] > 0 and out["ms_per_step"] > 0 and out["dtype"] == "f64"
    assert "device-driven" in out["config"]["loop"] and "rank_sweep" not in out and "host_stepped" not in out
    a = {f.name: np.load(f) for f in (tmp_path / "a").iterdir()}
    b = {f.name: np.load(f) for f in (tmp_path / "b").iterdir()}
    assert set(a) == set(b) and {"ew.npy", "eh.npy", "lkh.npy", "history.npy"} <= set(a)
    assert a["history.npy"].shape == (6, 9) and a["lkh.npy"][0] == a["history.npy"][-1, 0] == out["config"]["lkh_last"]
    assert a["ew.npy"].shape == (out["config"]["n_genes"], 10) and np.all(np.isfinite(a["eh.npy"]))
    for k in a:
        assert np.array_equal(a[k], b[k]), k


class _CountingEngine:
    """The surface of VBEngine that bench.py's headline uses, counting what it is asked to do (no device)."""
    calls = []

    def __init__(self, M, r, device=0, **kw):
        self.n, self.m, self.rank = M.shape[0], M.shape[1], r
        self.state = None

    def set_state(self, lw, lh, eh):
        self.state = {"lw": np.array(lw), "lh": np.array(lh), "eh": np.array(eh)}

    def step(self, hyper):
        self.calls.append(("step", 1))
        return -1.0, (0.0, 0.0, 0.0, 0.0)

    def run(self, hyper, Itmax=10000, Tol=1e-5, n0=10, dn=1, flags=(True,) * 4, history=False):
        self.calls.append(("run", Itmax, history))
        it = min(Itmax, 2) if Tol == float("inf") else Itmax        # (an unbounded tolerance stops at the first test)
        hist = np.tile(np.arange(it, dtype=np.float64)[:, None], (1, 9)) if history else None
        return {"it": it, "lk0": -2.0, "lkh": -1.5, "reason": 4, "hyper": dict(hyper), "history": hist}

    def get_state(self):
        s = self.state
        return {"lw": s["lw"], "lh": s["lh"], "ew": 2 * s["lw"], "eh": 2 * s["eh"], "dw": 3 * s["lw"], "dh": 3 * s["lh"]}

    def timing_enable(self, on=True):
        self.calls.append(("timing", on))

    def close(self):
        pass


def _fresh_bench(monkeypatch):
    """bench.py loaded as a module of its own (not left in sys.modules); the sys.path entry it adds is undone after the test."""
    monkeypatch.setattr(sys, "path", list(sys.path))
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _plain_run(monkeypatch, tmp_path, argv):
    """bench.main() with the device replaced by _CountingEngine -> engine calls."""
    import scipy.sparse as sp
    import torch
    bench = _fresh_bench(monkeypatch)
    import ccfindr_amd as C
    from ccfindr_amd import engine as E
    X = sp.random(40, 60, density=0.2, format="csc", random_state=1, data_rvs=lambda k: np.ones(k))
    monkeypatch.setattr(bench, "make_workload", lambda small, world=1, local_rank=0: ("stub", X, 3))
    monkeypatch.setattr(C, "CountMatrix", lambda X: X)
    monkeypatch.setattr(C, "VBEngine", _CountingEngine)
    monkeypatch.setattr(E, "device_warmup", lambda device=0: None)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(_CountingEngine, "calls", [])
    bench.main()
    return _CountingEngine.calls


def test_plain_run_times_exactly_k_steps_and_dumps_the_last_step(monkeypatch, tmp_path, capsys):
    calls = _plain_run(monkeypatch, tmp_path, ["--gpus", "1", "--steps", "7", "--warmup", "3", "--dump-outputs", str(tmp_path)])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in out, key
    assert out["steps"] == 7 and out["ms_per_step"] > 0 and out["unit"] == "iterations/s" and out["dtype"] == "f64"
    # W host steps, the settle run, then ONE device-driven region of exactly K steps -- and nothing else on the engine
    assert [c for c in calls if c[0] != "timing"] == [("step", 1)] * 3 + [("run", 1200 - 3, True), ("run", 7, True)]
    for key in ("value_host_stepped", "roofline", "host_stepped", "cpu_baseline", "ml_nmf", "rank_sweep", "restarts_small_matrix"):
        assert key not in out, key
    got = {p.name: np.load(p) for p in tmp_path.iterdir()}
    assert set(got) == {f"{k}.npy" for k in ("lw", "lh", "ew", "eh", "dw", "dh", "lkh", "history")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["history.npy"].shape == (7, 9) and got["lkh.npy"].tolist() == [-1.5]
    assert got["ew.npy"].shape == (40, 3) and got["eh.npy"].shape == (3, 60)


def test_a_long_plain_run_sizes_the_history_before_the_timed_region(monkeypatch, tmp_path, capsys):
    """K above the settle run: one short run asked for K steps (history buffer sized for K rows) before the settle run."""
    calls = _plain_run(monkeypatch, tmp_path, ["--gpus", "1", "--steps", "1500", "--warmup", "3"])
    assert [c for c in calls if c[0] != "timing"] == [("step", 1)] * 3 + [("run", 1500, True), ("run", 1197, True), ("run", 1500, True)]
    out = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][0])
    assert out["steps"] == 1500 and out["config"]["history_presize_steps"] == 2 and out["warmup_effective"] == 3 + 2 + 1197


def test_dumped_outputs_stay_under_the_budget_with_a_fixed_sample(monkeypatch, tmp_path):
    bench = _fresh_bench(monkeypatch)
    rng = np.random.default_rng(4)
    arrays = {"a": rng.uniform(size=(300, 500)), "b": rng.uniform(size=10), "c": rng.uniform(size=(2000,))}
    budget = 200_000
    for d in ("one", "two"):
        bench.write_outputs(str(tmp_path / d), arrays, budget=budget)
    files = sorted(p.name for p in (tmp_path / "one").iterdir())
    assert files == ["a.npy", "a_sample_index.npy", "b.npy", "c.npy"]
    assert sum(np.load(tmp_path / "one" / f).nbytes for f in files) <= budget
    for f in files:                                            # the same sample on every run
        assert np.array_equal(np.load(tmp_path / "one" / f), np.load(tmp_path / "two" / f))
    idx = np.load(tmp_path / "one" / "a_sample_index.npy").astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "one" / "a.npy"), arrays["a"].reshape(-1)[idx])
    assert np.array_equal(np.load(tmp_path / "one" / "c.npy"), arrays["c"])
