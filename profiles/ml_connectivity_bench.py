"""One timing of the ML loop on the PBMC sample (1030 x 450, rank 5) with the package found first on sys.path.
usage: ml_connectivity_bench.py TREE MODE  (TREE: directory of the package; MODE: host_conn | dev_conn | host_conn8 | dev_conn8 | lk_run)"""
import json
import os
import sys
import time

tree, mode = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path.insert(0, tree)
import numpy as np
import scipy.sparse as sp
import ccfindr_amd as C
from ccfindr_amd.engine import batch_grid, run_batch_ml

assert os.path.abspath(C.__file__).startswith(tree), C.__file__
GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
d = np.load(os.path.join(GOLD, "pbmc_extdata_r5.npz"))
n, m, r = int(d["n"]), int(d["m"]), 5
X = sp.csc_matrix((d["data"].astype(np.float64), d["indices"], d["indptr"]), shape=(n, m))
M = C.CountMatrix(X)


def start(seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(size=(n, r)), rng.uniform(size=(r, m))


def host_loop(eng, steps):
    for _ in range(steps):
        eng.ml_step()
        eng.cluster_changes()


reps = []
if mode == "host_conn":
    N = 4000
    eng = C.VBEngine(M, r)
    eng.ml_set_state(*start(1)); host_loop(eng, 200)
    for rep in range(3):
        eng.ml_set_state(*start(1))
        t0 = time.perf_counter(); host_loop(eng, N); reps.append((time.perf_counter() - t0) / N)
elif mode == "dev_conn":
    N = 20000
    eng = C.VBEngine(M, r)
    eng.ml_set_state(*start(1)); eng.ml_run(criterion="connectivity", ncnn_step=N + 1, Itmax=500)
    for rep in range(3):
        eng.ml_set_state(*start(1))
        t0 = time.perf_counter(); run = eng.ml_run(criterion="connectivity", ncnn_step=N + 1, Itmax=N); dt = time.perf_counter() - t0
        assert run["it"] == N and run["reason"] == 4, run
        reps.append(dt / N)
elif mode == "host_conn8":
    N = 1000
    eng = C.VBEngine(M, r)
    eng.ml_set_state(*start(1)); host_loop(eng, 200)
    for rep in range(3):
        t0 = time.perf_counter()
        for b in range(8):
            eng.ml_set_state(*start(10 + b)); host_loop(eng, N)
        reps.append((time.perf_counter() - t0) / (8 * N))
elif mode == "dev_conn8":
    N = 10000
    engs = [C.VBEngine(M, r, grid=batch_grid(8)) for _ in range(8)]
    for b, e in enumerate(engs):
        e.ml_set_state(*start(10 + b))
    run_batch_ml(engs, Itmax=500, criterion="connectivity", ncnn_step=N + 1)
    for rep in range(3):
        t0 = time.perf_counter()
        for b, e in enumerate(engs):
            e.ml_set_state(*start(10 + b))
        got = run_batch_ml(engs, Itmax=N, criterion="connectivity", ncnn_step=N + 1)
        dt = time.perf_counter() - t0
        assert all(g["it"] == N for g in got)
        reps.append(dt / (8 * N))
elif mode == "lk_run":
    N = 20000
    eng = C.VBEngine(M, r)
    eng.ml_set_state(*start(1)); eng.ml_run(Itmax=500, Tol=0.0)
    for rep in range(5):
        eng.ml_set_state(*start(1))
        t0 = time.perf_counter(); run = eng.ml_run(Itmax=N, Tol=0.0); dt = time.perf_counter() - t0
        assert run["it"] == N, run
        reps.append(dt / N)
else:
    raise SystemExit("unknown mode")
print(json.dumps({"tree": os.path.basename(tree), "mode": mode, "us_per_iteration": [round(1e6 * v, 3) for v in reps]}), flush=True)
