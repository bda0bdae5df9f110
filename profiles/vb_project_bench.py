#!/usr/bin/env python3
"""profiles/vb_project_bench.py -- vb_project() (csrc/vbproject.h) at the C3 shape, 20 000 x 50 000 at ~5 % stored entries,
ranks 10 and 20: wall and kernel time to Tol = 1e-5 and the per-cell iteration counts, next to project()'s ML kernel
(csrc/project.h) on the same matrix with the posterior's E[W] as its basis, in the same process.

    python profiles/vb_project_bench.py [small]
    python profiles/vb_project_bench.py coupled [small]      # the coupled form: profiles/vb_project_coupled_times.txt

Prints the text of profiles/vb_project_times.txt.  One MI355X.  The posterior is what 30 VB steps (hyper-parameters 1, 1, 1, 1)
from a random state leave on the same matrix: ew and sd = sqrt(dw) as a fit stores them; the cells placed are the matrix's own
50 000.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ccfindr_amd as C  # noqa: E402
import ccfindr_amd.project  # noqa: E402,F401
from ccfindr_amd import synth  # noqa: E402
from bench import make_workload  # noqa: E402

P = sys.modules["ccfindr_amd.project"]
REPS = 5


def say(*a):
    print(*a)
    sys.stdout.flush()


def med(v):
    v = sorted(v)
    return "median %.4f  min %.4f  max %.4f" % (v[len(v) // 2], v[0], v[-1])


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def spread(it, reason):
    q = np.percentile(it, [0, 5, 25, 50, 75, 95, 99, 100])
    return "mean %.1f | min %d  5%% %d  25%% %d  median %d  75%% %d  95%% %d  99%% %d  max %d | reasons %s" % (
        it.mean(), *q, {int(k): int(v) for k, v in zip(*np.unique(reason, return_counts=True))})


def sweep(ranks):
    """`python profiles/vb_project_bench.py sweep 14 16 ..`: the VB kernel alone over a list of ranks at the C3 shape, on a
    drawn posterior (alw ~ U(0.5, 6), bew ~ U(0.02, 0.3)) -- for comparing builds of the kernel (VBNMF_LIB) rank by rank."""
    name, X, _ = make_workload(False)
    X = X.tocsc()
    n, m = X.shape
    M = C.CountMatrix(X)
    hyper = {"ah": 1.0, "bh": 1.0}
    for r in ranks:
        rng = np.random.default_rng(r)
        alw, bew = rng.uniform(0.5, 6.0, size=(n, r)), rng.uniform(0.02, 0.3, size=(n, r))
        pair = (alw * bew, np.sqrt(alw) * bew)
        kerns = []
        for rep in range(4):
            p = C.vb_project(M, pair, hyper=hyper, Tol=1e-5)
            if rep:
                kerns.append(P.vb_last_kernel_ms())
        k = sorted(kerns)[1]
        say(f"rank {r:3d}: kernel ms median {k:9.3f}  min {min(kerns):9.3f}  max {max(kerns):9.3f} | mean iterations {p.nsteps.mean():6.1f}"
            f" max {p.nsteps.max():4d} | ms per mean iteration {k / p.nsteps.mean():7.3f} | lml_cells {p.lml_cells:.12g}")
    M.close()


def fitted_pair(M, n, m, r, hyper):
    """ew and sd = sqrt(dw) of what 30 VB steps from a random state leave on the matrix."""
    eng = C.VBEngine(M, r)
    wh = synth.random_state(n, m, r, hyper, seed=100 + r)
    eng.set_state(wh["lw"], wh["lh"], wh["eh"])
    for _ in range(30):
        eng.step(hyper)
    st = eng.get_state(("ew", "dw"))
    eng.close()
    return st["ew"], np.sqrt(st["dw"])


def coupled(small):
    """`python profiles/vb_project_bench.py coupled [small]`: time per iteration of the coupled form (k_vbp_step + k_vbp_control
    per step, the host reading the control block every eight) next to the per-cell kernel's (kernel time over mean nsteps) on
    the same posterior, in one process, interleaved, five repeats after a warm-up of each."""
    t, (name, X, _) = timed(lambda: make_workload(small))
    X = X.tocsc()
    n, m = X.shape
    say(f"{name}: n={n} m={m} stored entries={X.nnz} ({100.0 * X.nnz / n / m:.2f} %), generated in {t:.1f} s")
    M = C.CountMatrix(X)
    hyper = {"aw": 1.0, "bw": 1.0, "ah": 1.0, "bh": 1.0}
    modes = (("cell", "per-cell kernel, stop=\"cell\"          ", {}),
             ("off", "coupled, stop=\"global\", flags off    ", {"stop": "global"}),
             ("on", "coupled, hyper_update=(True, True)     ", {"hyper_update": (True, True)}))
    for r in (10, 20):
        say(f"\n== rank {r} ==")
        pair = fitted_pair(M, n, m, r, hyper)
        per_it = {k: [] for k, _, _ in modes}
        kern = {k: [] for k, _, _ in modes}
        last = {}
        for rep in range(REPS + 1):
            for key, _, kw in modes:
                p = C.vb_project(M, pair, hyper=hyper, Tol=1e-5, **kw)
                last[key] = p
                if rep:
                    ms = P.vb_last_kernel_ms()
                    kern[key].append(ms)
                    per_it[key].append(ms / p.nsteps.mean())
        for key, label, _ in modes:
            p = last[key]
            say(f"{label}: kernel ms {med(kern[key])} | mean iterations {p.nsteps.mean():.1f} (max {p.nsteps.max()}) | "
                f"ms per iteration {med(per_it[key])}")
            say(f"    reasons {dict(zip(*[a.tolist() for a in np.unique(p.reason, return_counts=True)]))}; evidence {p.evidence:.12g}; "
                f"(ah, bh) {p.hyper0['ah']:.6g}, {p.hyper0['bh']:.6g} -> {p.hyper['ah']:.6g}, {p.hyper['bh']:.6g}")
        base = sorted(per_it["cell"])[REPS // 2]
        for key in ("off", "on"):
            say(f"ms per iteration, {key} / per-cell: {sorted(per_it[key])[REPS // 2] / base:.3f}")
    M.close()


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "sweep":
        return sweep([int(a) for a in sys.argv[2:]])
    if len(sys.argv) > 1 and sys.argv[1] == "coupled":
        return coupled(len(sys.argv) > 2 and sys.argv[2] == "small")
    small = len(sys.argv) > 1 and sys.argv[1] == "small"
    t, (name, X, _) = timed(lambda: make_workload(small))
    X = X.tocsc()
    n, m = X.shape
    say(f"{name}: n={n} m={m} stored entries={X.nnz} ({100.0 * X.nnz / n / m:.2f} %), generated in {t:.1f} s")
    M = C.CountMatrix(X)
    hyper = {"aw": 1.0, "bw": 1.0, "ah": 1.0, "bh": 1.0}
    for r in (10, 20):
        say(f"\n== rank {r} ==")
        pair = fitted_pair(M, n, m, r, hyper)
        t_pb, _ = timed(lambda: C.posterior_basis(pair, hyper=hyper))
        say(f"posterior_basis (n r digammas on the host): {t_pb:.4f} s")
        walls, kerns = {"vb": [], "ml": []}, {"vb": [], "ml": []}
        for rep in range(REPS + 1):                           # the two kernels interleaved; the first call of each is the warm-up
            dt, pv = timed(lambda: C.vb_project(M, pair, hyper=hyper, Tol=1e-5))
            if rep:
                walls["vb"].append(dt)
                kerns["vb"].append(P.vb_last_kernel_ms() / 1e3)
            dt, pm = timed(lambda: C.project(M, pair[0], Tol=1e-5))
            if rep:
                walls["ml"].append(dt)
                kerns["ml"].append(P.last_kernel_ms() / 1e3)
        for key, label, p in (("vb", "vb_project(CountMatrix, (ew, sd))", pv), ("ml", "project(CountMatrix, ew)       ", pm)):
            k = sorted(kerns[key])[REPS // 2]
            say(f"{label}: wall s {med(walls[key])} | kernel s {med(kerns[key])}")
            say(f"    iterations per cell: {spread(p.nsteps, p.reason)}")
            say(f"    kernel ms per mean iteration: {1e3 * k / p.nsteps.mean():.3f}")
        say(f"lml_cells {pv.lml_cells:.12g}; ML likelihood {pm.likelihood:.12g}")
        same = np.mean(C.cluster_id(pv, rank=r) == C.cluster_id(pm, rank=r))
        say(f"share of cells whose largest coefficient is the same component under both: {same:.4f}")
    M.close()


if __name__ == "__main__":
    main()
