"""One timing of the device-driven ML loop (criterion = 'likelihood', Tol = 0) -> one JSON line.
usage: ml_partition_bench.py MODE
  pbmc      the single engine's ml_run on the 1030 x 450 PBMC sample, rank 5
  big       ... on a 5 000 x 20 000, 5 %-dense Poisson matrix, rank 10
  group P   comm.ml_run of a local group of P partitions on that matrix (needs the partitioned ML step)
ML_BENCH_TREE names the directory holding the package to time, default this tree (parent commit against this one on one box:
run the modes alternately);
ML_BENCH_STEPS shortens the timed loops (a run under rocprofv3 --kernel-trace --stats)."""
import json
import os
import sys
import time

sys.path.insert(0, os.environ.get("ML_BENCH_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
import ccfindr_amd as C
from ccfindr_amd.parallel import cell_partition

mode = sys.argv[1]
GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def start(n, m, r, seed=1):
    rng = np.random.default_rng(seed)
    return rng.uniform(size=(n, r)), rng.uniform(size=(r, m))


def big():
    n, m = 5000, 20000
    X = sp.random(n, m, density=0.05, format="csc", random_state=np.random.default_rng(4),
                  data_rvs=lambda k: np.random.default_rng(5).poisson(2.0, k) + 1.0)
    X = X + sp.csc_matrix((np.ones(n), (np.arange(n), np.arange(n) % m)), shape=(n, m))      # no empty rows / columns
    X = X + sp.csc_matrix((np.ones(m), (np.arange(m) % n, np.arange(m))), shape=(n, m))
    return sp.csc_matrix(X), n, m, 10


if mode == "pbmc":
    d = np.load(os.path.join(GOLD, "pbmc_extdata_r5.npz"))
    n, m, r = int(d["n"]), int(d["m"]), 5
    X = sp.csc_matrix((d["data"].astype(np.float64), d["indices"], d["indptr"]), shape=(n, m))
    N = 20000
else:
    X, n, m, r = big()
    N = 2000
N = int(os.environ.get("ML_BENCH_STEPS", N))                 # (a short run under a profiler)
M = C.CountMatrix(X)
w, h = start(n, m, r)
reps = []
if mode in ("pbmc", "big"):
    eng = C.VBEngine(M, r)
    eng.ml_set_state(w, h); eng.ml_run(Itmax=200, Tol=0.0)
    for rep in range(5):
        eng.ml_set_state(w, h)
        t0 = time.perf_counter(); run = eng.ml_run(Itmax=N, Tol=0.0); dt = time.perf_counter() - t0
        assert run["it"] == N, run
        reps.append(dt / N)
elif mode == "group":
    P = int(sys.argv[2])
    cuts = cell_partition(m, P)
    comm = C.Communicator.local(P)
    parts = [C.VBEngine(M, r, cols=c, m_global=m) for c in cuts]
    for p in parts:
        p.attach_comm(comm)

    def load():
        for p, (b, e) in zip(parts, cuts):
            p.ml_set_state(w, h[:, b:e])
        comm.ml_state_finish()
    load(); comm.ml_run(Itmax=200, Tol=0.0)
    for rep in range(5):
        load()
        t0 = time.perf_counter(); run = comm.ml_run(Itmax=N, Tol=0.0); dt = time.perf_counter() - t0
        assert run["it"] == N, run
        reps.append(dt / N)
else:
    raise SystemExit("unknown mode")
print(json.dumps({"tree": os.path.dirname(os.path.dirname(os.path.abspath(C.__file__))), "mode": " ".join(sys.argv[1:]), "nnz": int(X.nnz),
                  "us_per_step": [round(1e6 * v, 2) for v in reps]}), flush=True)
