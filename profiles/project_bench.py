#!/usr/bin/env python3
"""profiles/project_bench.py -- project() (csrc/project.h) at the C3 shape, 20 000 x 50 000 at ~5 % stored entries, ranks 10
and 20: wall and kernel time to Tol = 1e-5, the per-cell iteration counts, and the same projection emulated with a full engine
(ingestion, both tiled layouts, then ml_step + read h + ml_set_state(W, h) per iteration).  FORMS: the kernel forms a build
offers, interleaved call by call (profiles/ubench/project_staged_form_experiment.patch adds the staged one).

    python profiles/project_bench.py [small]

Prints the text of profiles/project_times.txt.  One MI355X.  The basis is what 30 ML-NMF steps from a uniform start leave on the
same matrix; the cells placed are the matrix's own 50 000.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ccfindr_amd as C  # noqa: E402
import ccfindr_amd.project  # noqa: E402,F401
from bench import make_workload  # noqa: E402

P = sys.modules["ccfindr_amd.project"]
REPS = 5
FORMS = ("gather",)          # VBNMF_PROJECT_FORM of every timed call (read by the experiment build only)
EMU_STEPS = 6


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


def main():
    small = len(sys.argv) > 1 and sys.argv[1] == "small"
    t, (name, X, _) = timed(lambda: make_workload(small))
    X = X.tocsc()
    n, m = X.shape
    say(f"{name}: n={n} m={m} stored entries={X.nnz} ({100.0 * X.nnz / n / m:.2f} %), generated in {t:.1f} s")
    t_cold, M = timed(lambda: C.CountMatrix(X))
    say(f"first ingestion of the process (CountMatrix from scipy CSC; loads the library, starts the host threads): {t_cold:.3f} s")
    for r in (10, 20):
        say(f"\n== rank {r} ==")
        # the emulation's set-up, warm: a fresh handle every time, so that both layouts are cut (a handle caches its layouts)
        ings, engs = [], []
        for _ in range(3):
            dt, M2 = timed(lambda: C.CountMatrix(X))
            ings.append(dt)
            dt, e2 = timed(lambda: C.VBEngine(M2, r))
            engs.append(dt)
            e2.close()
            M2.close()
        say(f"ingestion (CountMatrix from scipy CSC): s {med(ings)}")
        say(f"engine creation on a fresh handle (both layouts cut and uploaded): s {med(engs)}")
        t_ing, t_eng = sorted(ings)[1], sorted(engs)[1]
        eng = C.VBEngine(M, r)
        rng = np.random.default_rng(r)
        eng.ml_set_state(rng.uniform(size=(n, r)), rng.uniform(size=(r, m)))
        for _ in range(30):
            eng.ml_step()
        W = eng.ml_get_state(("ew",))["ew"]
        h0 = P.default_start(M, W)
        # -- project(): the forms interleaved; the first call of each is the warm-up
        walls = {f: [] for f in FORMS}
        kerns = {f: [] for f in FORMS}
        outs = {}
        for rep in range(REPS + 1):
            for form in FORMS:
                os.environ["VBNMF_PROJECT_FORM"] = form
                dt, p = timed(lambda: C.project(M, W, Tol=1e-5))
                if rep:
                    walls[form].append(dt)
                    kerns[form].append(P.last_kernel_ms() / 1e3)
                outs[form] = p
        os.environ.pop("VBNMF_PROJECT_FORM")
        p = outs[FORMS[0]]
        for form in FORMS:
            say(f"project(CountMatrix, W), {form:6s}: wall s {med(walls[form])} | kernel s {med(kerns[form])}")
        if len(FORMS) > 1:
            g = outs[FORMS[1]]
            same = (np.array_equal(p.coeff[0], g.coeff[0]) and np.array_equal(p.cell_likelihood, g.cell_likelihood)
                    and np.array_equal(p.nsteps, g.nsteps))
            say(f"the two forms' H, cell likelihoods and iteration counts are the same bits: {same}")
        it = p.nsteps
        q = np.percentile(it, [0, 5, 25, 50, 75, 95, 99, 100])
        say("iterations per cell: mean %.1f | min %d  5%% %d  25%% %d  median %d  75%% %d  95%% %d  99%% %d  max %d | reasons %s" % (
            it.mean(), *q, dict(zip(*np.unique(p.reason, return_counts=True)))))
        say(f"likelihood {p.likelihood:.12g}")
        tw = []
        for _ in range(3):
            dt, _p = timed(lambda: C.project(X, W, Tol=1e-5))
            tw.append(dt)
        say(f"project(scipy CSC, W) (ingestion inside): wall s {med(tw)}")
        # -- the emulation: per iteration ml_step (which also updates W), read h, load (W, h) again
        eng.ml_set_state(W, h0)
        per = []
        for _ in range(EMU_STEPS):
            def one():
                eng.ml_step()
                h = eng.ml_get_state(("eh",))["eh"]
                eng.ml_set_state(W, h)
            per.append(timed(one)[0])
        eng.close()
        per_it = sorted(per[1:])[len(per[1:]) // 2]
        emu = t_ing + t_eng + it.mean() * per_it
        say(f"emulation: ml_step + get h + ml_set_state(W, h): s per iteration {med(per[1:])}")
        say(f"emulation total = ingestion {t_ing:.3f} + engine {t_eng:.3f} + mean iterations {it.mean():.1f} x {per_it:.4f} = {emu:.3f} s"
            f"   (set-up alone {t_ing + t_eng:.3f} s)")
        pw = sorted(tw)[len(tw) // 2]
        say(f"project from the same scipy matrix: {pw:.3f} s -> {'beats' if pw < emu else 'DOES NOT beat'} the emulation"
            f" ({emu / pw:.1f} x); set-up alone {'exceeds' if t_ing + t_eng > pw else 'does not exceed'} it")
    M.close()


if __name__ == "__main__":
    main()
