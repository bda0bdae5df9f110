#!/usr/bin/env python3
"""tests/manual_qc_times.py -- gene_stats / filter_genes (csrc/qc.h, ccfindr_amd/qc.py) timed on one MI355X: the 20 000 x
50 000 matrix of bench.py's generator and the shipped 1030 x 450 sample.  Run by hand, like the other manual_* files:

    python tests/manual_qc_times.py [output file, default profiles/qc_times.txt] [small]

Per matrix: the four parts of gene_stats (grouping by gene, upload, kernel by device events, host finish), after one warm-up
call; the kernel's bytes read over its time as a share of the HBM peak; filter_genes(rescue_genes=True) as a whole, warmed, no
profiler; and the numpy statement of tests/util_qc.py on the same box (on a slice of the genes where the dense matrix would not
fit a sensible time, scaled up, and said so).  No number is asserted.
"""
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import util_qc as U  # noqa: E402

import ccfindr_amd as C  # noqa: E402
from ccfindr_amd import qc as Q  # noqa: E402

REPS = 5
HBM_PEAK = 8.0e12            # bytes / s, the MI355X's specified HBM3E peak
LINES = []


def say(*a):
    line = " ".join(str(v) for v in a)
    LINES.append(line)
    print(line)
    sys.stdout.flush()


def med(v):
    v = sorted(v)
    return "median %8.3f  min %8.3f  max %8.3f" % (v[len(v) // 2], v[0], v[-1])


def split_times(M, X, label):
    n, m = M.shape
    res = Q.gene_stats(M)                                # warm-up: code object, device pool
    rows, wall = [], []
    for _ in range(REPS):
        t = time.perf_counter()
        Q.gene_stats(M)
        wall.append((time.perf_counter() - t) * 1e3)
        rows.append(Q.qc_info()["times_ms"].copy())
    a = np.array(rows)
    say(f"{label}: gene_stats(CountMatrix), rows finished on the host: {res.host_finished}; ms:")
    for k, name in enumerate(("grouping by gene (host)", "upload", "kernel (device events)", "host finish")):
        say(f"    {name:28s} {med(list(a[:, k]))}")
    say(f"    {'gene_stats, wall':28s} {med(wall)}")
    kms = float(np.median(a[:, 2]))
    nbytes = X.nnz * 8 + 8 * (n + 1) + 28 * n
    say(f"    kernel bytes (values once, row pointers, results) {nbytes / 1e6:.1f} MB -> {nbytes / kms / 1e9:.3f} TB/s, "
        f"{100.0 * nbytes / (kms * 1e-3) / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak "
        "(the second pass over a long row is served by the caches and not counted)")


def numpy_statement(X, label, max_rows):
    n, m = X.shape
    rows = min(n, max_rows)
    A = X[:rows].toarray()
    t = time.perf_counter()
    U.calc_vmr(A)
    t_vmr = time.perf_counter() - t
    t = time.perf_counter()
    modes = sum(U.has_mode(r) for r in A)
    t_mode = time.perf_counter() - t
    scale = n / rows
    say(f"{label}: numpy statement (tests/util_qc.py) on this box's host, genes 0..{rows - 1} of {n}"
        + (f", scaled by {scale:.1f} to all genes" if rows < n else "") + f": calc_vmr {t_vmr * scale:.3f} s, has_mode of every gene "
        f"{t_mode * scale:.3f} s ({modes} of the {rows} have a mode)")


def whole_filter(x, label, **kw):
    Q.filter_genes(x, verbose=False, **kw)
    ts = []
    for _ in range(REPS):
        t = time.perf_counter()
        out = Q.filter_genes(x, verbose=False, **kw)
        ts.append((time.perf_counter() - t) * 1e3)
    say(f"{label}: filter_genes({', '.join(f'{k}={v}' for k, v in kw.items())}) on a CountData (ingestion of the scipy matrix, the "
        f"scan, the selection, the subset), wall ms: {med(ts)}; {out.counts.shape[0]} of {x.counts.shape[0]} genes kept")


def main():
    args = [a for a in sys.argv[1:] if a != "small"]
    small = "small" in sys.argv[1:]
    out = args[0] if args else os.path.join(ROOT, "profiles", "qc_times.txt")
    from bench import make_workload
    say("profiles/qc_times.txt -- gene_stats (csrc/qc.h, vbnmf_matrix_gene_stats) and filter_genes on one MI355X, one visit.")
    say(f"Written by tests/manual_qc_times.py.  One warm-up call, then {REPS} timed calls.")
    say(f"host threads of the library: {C.engine.host_threads()}; kernel constants: { {k: v for k, v in Q.qc_info().items() if k != 'times_ms'} }")
    say("")
    t = time.perf_counter()
    name, X, _ = make_workload(small)
    X = sp.csc_matrix(X)
    say(f"{name}: n={X.shape[0]} m={X.shape[1]} stored entries={X.nnz} ({100.0 * X.nnz / X.shape[0] / X.shape[1]:.2f} %), "
        f"largest count {X.data.max():.0f}, generated in {time.perf_counter() - t:.1f} s")
    t = time.perf_counter()
    M = C.CountMatrix(X)
    say(f"ingestion (CountMatrix from scipy CSC, first of the process): {time.perf_counter() - t:.3f} s")
    split_times(M, X, "C3")
    M.close()
    x = C.CountData(X, [[f"g{i}"] for i in range(X.shape[0])], [[f"c{j}"] for j in range(X.shape[1])])
    whole_filter(x, "C3", vmr_min=1.5, min_cells_expressed=50, rescue_genes=True)
    numpy_statement(X.tocsr(), "C3", 500)
    say("")
    z = np.load(os.path.join(HERE, "golden", "pbmc_extdata_r5.npz"))
    Xs = sp.csc_matrix((z["data"].astype(np.float64), z["indices"], z["indptr"]), shape=(int(z["n"]), int(z["m"])))
    say(f"shipped sample: n={Xs.shape[0]} m={Xs.shape[1]} stored entries={Xs.nnz}, largest count {Xs.data.max():.0f}")
    Ms = C.CountMatrix(Xs)
    split_times(Ms, Xs, "sample")
    Ms.close()
    xs = C.CountData(Xs, [[f"g{i}"] for i in range(Xs.shape[0])], [[f"c{j}"] for j in range(Xs.shape[1])])
    whole_filter(xs, "sample", vmr_min=1.5, min_cells_expressed=50, rescue_genes=True)
    numpy_statement(Xs.tocsr(), "sample", 1 << 30)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
