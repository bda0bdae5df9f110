"""One timing of the ML loop of a local group of 3 partitions on the PBMC sample (1030 x 450, rank 5), with the package found
first on sys.path -> one JSON line.
usage: ml_partitioned_connectivity_bench.py TREE MODE
  TREE  directory of the package to time (the parent commit's tree against this one on one box: one process per line, alternating)
  MODE  lk_run     comm.ml_run(Tol=0): the likelihood loop
        conn_run   comm.ml_run_connectivity(ncnn_step > Itmax): the connectivity loop, never stopping (needs this change)
        host_conn  the host-stepped path it replaces: ml_step_local / exchange / ml_step_local / exchange / ml_step_finish on every
                   partition and the labels of all cells gathered on the host, per iteration"""
import json
import os
import sys
import time

tree, mode = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path.insert(0, tree)
import numpy as np
import scipy.sparse as sp
import torch
import ccfindr_amd as C
from ccfindr_amd.parallel import cell_partition

assert os.path.abspath(C.__file__).startswith(tree), C.__file__
GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
d = np.load(os.path.join(GOLD, "pbmc_extdata_r5.npz"))
n, m, r, P = int(d["n"]), int(d["m"]), 5, 3
X = sp.csc_matrix((d["data"].astype(np.float64), d["indices"], d["indptr"]), shape=(n, m))
M = C.CountMatrix(X)
rng = np.random.default_rng(1)
w, h = rng.uniform(size=(n, r)), rng.uniform(size=(r, m))
cuts = cell_partition(m, P)
comm = C.Communicator.local(P)
parts = [C.VBEngine(M, r, cols=c, m_global=m) for c in cuts]
for p in parts:
    p.attach_comm(comm)


def load():
    for p, (b, e) in zip(parts, cuts):
        p.ml_set_state(w, h[:, b:e])
    comm.ml_state_finish()


def host_loop(steps, reds):
    off = parts[0].reduce_tail()[0]
    for _ in range(steps):
        for tail in (False, True):
            for p in parts:
                p.ml_step_local()
            torch.cuda.synchronize()
            o = off if tail else 0
            s = sum((q[o:] for q in reds[1:]), reds[0][o:].clone())
            for q in reds:
                q[o:].copy_(s)
            torch.cuda.synchronize()
        for p in parts:
            p.ml_step_finish()
        np.concatenate([p.cluster_ids() for p in parts])


reps = []
if mode in ("lk_run", "conn_run"):
    N = 20000
    run_it = ((lambda k: comm.ml_run(Itmax=k, Tol=0.0)) if mode == "lk_run"
              else (lambda k: comm.ml_run_connectivity(Itmax=k, ncnn_step=N + 1)))
    load(); run_it(500)
    for rep in range(5):
        load()
        t0 = time.perf_counter(); run = run_it(N); dt = time.perf_counter() - t0        # (the call returns behind a stream synchronise)
        assert run["it"] == N and run["reason"] == 4, run
        reps.append(dt / N)
elif mode == "host_conn":
    N = 2000
    reds = [p.reduce_tensor() for p in parts]
    load(); host_loop(100, reds)
    for rep in range(3):
        load()
        t0 = time.perf_counter(); host_loop(N, reds); reps.append((time.perf_counter() - t0) / N)
else:
    raise SystemExit("unknown mode")
print(json.dumps({"tree": os.path.basename(tree), "mode": mode, "us_per_iteration": [round(1e6 * v, 3) for v in reps]}), flush=True)
