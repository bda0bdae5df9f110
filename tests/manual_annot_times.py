#!/usr/bin/env python3
"""tests/manual_annot_times.py -- assign_celltype (csrc/gsea.h, ccfindr_amd/annotate.py) timed on one MI355X: the meta table of
a rank-10 VB fit of bench.py's 20 000 x 50 000 matrix, 20 gene sets of 5-200 genes, p.value with nperm = 1000.  Run by hand,
like the other manual_* files:

    python tests/manual_annot_times.py [output file, default profiles/annot_times.txt] [small]

After one warm-up call: the parts of the library call (host checks with the permutations' inversion, upload, kernels by device
events, read-back), assign_celltype(p_value=True, nperm=1000) as a whole on the ready MetaTable (flags, permutations and all),
and the dense numpy restatement of tests/util_annot.py on the same host for 10 of the permutations, extrapolated to 1000 and
marked so.  The fit is cut at ITMAX iterations: the table's shape is what the timing needs, not a converged basis.  No number
is asserted.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import util_annot as U  # noqa: E402

import ccfindr_amd as C  # noqa: E402
from ccfindr_amd import annotate as A  # noqa: E402

REPS = 5
RANK = 10
NPERM = 1000
ITMAX = 200
LINES = []


def say(*a):
    line = " ".join(str(v) for v in a)
    LINES.append(line)
    print(line)
    sys.stdout.flush()


def med(v):
    v = sorted(v)
    return "median %9.3f  min %9.3f  max %9.3f" % (v[len(v) // 2], v[0], v[-1])


def main():
    args = [a for a in sys.argv[1:] if a != "small"]
    small = "small" in sys.argv[1:]
    out = args[0] if args else os.path.join(ROOT, "profiles", "annot_times.txt")
    from bench import make_workload
    say("profiles/annot_times.txt -- assign_celltype (csrc/gsea.h, vbnmf_gsea_perm) on one MI355X, one visit.")
    say(f"Written by tests/manual_annot_times.py.  One warm-up call, then {REPS} timed calls.")
    say(f"host threads of the library: {C.engine.host_threads()}")
    t = time.perf_counter()
    name, X, _ = make_workload(small)
    say(f"{name}: n={X.shape[0]} m={X.shape[1]}, generated in {time.perf_counter() - t:.1f} s")
    t = time.perf_counter()
    res = C.vb_factorize(X, ranks=RANK, nrun=1, verbose=0, progress_bar=False, seed=1, Itmax=ITMAX)
    say(f"vb_factorize(ranks={RANK}, nrun=1, Itmax={ITMAX}): {time.perf_counter() - t:.1f} s, {res.nsteps} iterations")
    n = X.shape[0]
    names = ["gene%d" % i for i in range(n)]
    t = time.perf_counter()
    meta = C.meta_gene_cv(res, rank=RANK, max_per_cluster=np.inf, gene_names=names, cv_max=np.inf)
    say(f"meta_gene_cv(max_per_cluster=inf, cv_max=inf): table of {meta.gene.shape[0]} rows x {meta.rank} clusters, "
        f"{int(np.isnan(meta.w).sum())} NA entries, {time.perf_counter() - t:.3f} s")
    rng = np.random.default_rng(7)
    sizes = rng.integers(5, 201, size=20)
    gset = {"set%d" % s: list(rng.choice(names, size=int(k), replace=False)) for s, k in enumerate(sizes)}
    say(f"20 gene sets of {sorted(int(k) for k in sizes)} genes, p = 1, grp_prefix = ('IG',)")
    N = meta.gene.shape[0]
    say(f"kernel constants: { {k: v for k, v in A.gsea_info(N).items() if k != 'times_ms'} }")
    perms = np.array([rng.permutation(N) for _ in range(NPERM)], dtype=np.int32)

    t = time.perf_counter()
    tb = A.gsea_tables(meta, gset, p=1)
    say(f"hit and miss flags on the host (gsea_tables, once per call): {(time.perf_counter() - t) * 1e3:.1f} ms, {len(tb['hit_row'])} hits in all")
    A.gsea_perm(tb["valid"], tb["wp"], tb["hit_ptr"], tb["hit_row"], tb["hit_is_miss"], tb["nsets"], perms=perms)      # warm-up
    rows, wall = [], []
    for _ in range(REPS):
        t = time.perf_counter()
        es, exceed, _ = A.gsea_perm(tb["valid"], tb["wp"], tb["hit_ptr"], tb["hit_row"], tb["hit_is_miss"], tb["nsets"], perms=perms)
        wall.append((time.perf_counter() - t) * 1e3)
        rows.append(A.gsea_info(N)["times_ms"].copy())
    a = np.array(rows)
    say(f"vbnmf_gsea_perm, nperm = {NPERM}, {NPERM * RANK * len(gset)} scores; ms:")
    for k, label in ((3, "host checks + inversion"), (0, "upload"), (1, "kernels (device events)"), (2, "read-back")):
        say(f"    {label:28s} {med(list(a[:, k]))}")
    say(f"    {'the library call, wall':28s} {med(wall)}")
    whole = []
    for _ in range(REPS):
        t = time.perf_counter()
        o = C.assign_celltype(meta, RANK, gset, p=1, p_value=True, nperm=NPERM, seed=3)
        whole.append((time.perf_counter() - t) * 1e3)
    say(f"assign_celltype(MetaTable, p_value=True, nperm={NPERM}) as a whole (flags, {NPERM} numpy permutations, the call), wall ms: {med(whole)}")
    say(f"    smallest p-value {np.nanmin(o['pvalue']):.3f}, NaN scores {int(np.isnan(o['ES']).sum())}")

    few = 10
    t = time.perf_counter()
    es_d, exceed_d, null_d = U.assign_dense(meta.gene, meta.w, tb["wp"].T, gset, perms[:few])
    td = time.perf_counter() - t
    es10, exceed10, null10 = A.gsea_perm(tb["valid"], tb["wp"], tb["hit_ptr"], tb["hit_row"], tb["hit_is_miss"], tb["nsets"],
                                         perms=perms[:few], return_null=True)
    say(f"dense numpy restatement (tests/util_annot.py) on this box's host: {few} permutations + the observed table {td:.2f} s; "
        f"EXTRAPOLATED to {NPERM} permutations: {td * (NPERM + 1) / (few + 1):.1f} s (not run)")
    say(f"    the device's scores for those {few} permutations equal the restatement's bit for bit: "
        f"{U.bits_equal(es10, es_d) and U.bits_equal(null10, null_d) and bool(np.array_equal(exceed10, exceed_d))}")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
