"""numpy restatement of the coupled VB projection loop (csrc/vbproject.h, k_vbp_step / k_vbp_control) -- TEST INFRASTRUCTURE ONLY.

The H half of ``vb_iterate`` (reference R/bayesian.R:336-352) with q(W) held: one step of ``util_vb_project.h_half`` for all cells
under the current (ah, bh), the cells' evidences (``util_vb_project.cell_evidence``) added to E, ``hyper_update`` (:2-53) with
``hyper.update = (F, F, fa, fb)`` from step n0 + 1 on, and the stop of :345-348 on E, after the hyper-update, without the
``lkh >= lk0`` clause (DESIGN.md sections 5g, 5h).  tests/test_vb_project_coupled_cpu.py ties ``hyper_update_h`` and the loop
to the committed oracle (``oracle.vbnmf_oracle.hyper_update``, ``vb_iterate``).
"""
import math

import numpy as np
from scipy.special import digamma, polygamma

import util_vb_project as U

EPS = U.EPS


def hyper_update_h(fa, fb, lhm, ehm, ah, bh, Niter=100, Tol=1e-3):
    """R/bayesian.R:2-53 with flags (F, F, fa, fb) on the statistics ``lhm = mean(log lh)``, ``ehm = mean(eh)``
    -> (ah1, bh1, failed, dfs).  The aw side's Newton step is 0, so its term of df (:37) is exactly 0.  ``failed``: Niter
    reached (:43), or a non-finite Newton step, on which the reference's halving loop (:28-35) would not end; (ah, bh) come
    back unchanged then.  ``dfs``: the df of every Newton decision."""
    if not (fa or fb):                                                               # :4
        return ah, bh, False, []
    ah0, bh0 = ah, bh
    ah1 = ah0
    dfs = []
    if fa:                                                                           # :15 (flags[0] + flags[2] > 0)
        i = 1
        while i < Niter:
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                dh = ((np.log(ah0) - digamma(ah0) - ehm / bh0 + 1 + lhm - np.log(bh0))
                      / (1 / ah0 - polygamma(1, ah0)))                               # :22-26
            if not np.isfinite(dh):
                return ah, bh, True, dfs
            ah1 = ah0 - dh
            halvings = 0
            while ah1 <= 0:                                                          # :32-35
                dh /= 2
                ah1 = ah0 - dh
                halvings += 1
                if halvings > 1100:
                    return ah, bh, True, dfs
            df = 0.0 + (1 - ah1 / ah0) ** 2                                          # :37
            dfs.append(float(df))
            if df < Tol:
                break
            ah0 = ah1
            i += 1
        if i == Niter:                                                               # :43
            return ah, bh, True, dfs
    return float(ah1), float(ehm), False, dfs                                        # :50-51: both branches assign ehm


def project_coupled(x, lw, ew, lh0, ah, bh, flags=(False, False), n0=10, dn=1, fudge=EPS, Itmax=10000, Tol=1e-5):
    """All cells stepped together to one stop -> dict(lh, eh, dh, ev, E, it, reason, hyper, history, stop_margin,
    newton_margin, lk0).

    reason: 5 the hyper-parameter update failed; 3 E is NaN; 1 ``it > 1, it > n0, abs(1 - E / lk0) < Tol``; 4 Itmax.
    history: a row [E, mean(log lh), mean(eh), ah, bh after the update] per step.  stop_margin: min over the stopping
    decisions of ``| |1 - E / lk0| - Tol | / Tol``; newton_margin: min over the Newton decisions of ``|df - 1e-3| / 1e-3``.
    lk0: the E the last decision compared against (it lags on a convergence stop, as :346-348 make it)."""
    x = np.asarray(x, dtype=np.float64)
    lw = np.asarray(lw, dtype=np.float64)
    cew = np.asarray(ew, dtype=np.float64).sum(axis=0)
    lh = np.array(lh0, dtype=np.float64, copy=True)
    lh[lh < fudge] = fudge
    fa, fb = bool(flags[0]), bool(flags[1])
    ah, bh = float(ah), float(bh)
    lk0, E = 0.0, float("nan")
    eh = dh = ev = None
    history = []
    stop_margin, newton_margin = math.inf, math.inf
    it, reason = 0, 0
    for it in range(1, int(Itmax) + 1):
        lh, eh, dh, alh = U.h_half(x, lw, cew, lh, ah, bh, fudge)
        ev = U.cell_evidence(x, lw, cew, lh, eh, alh, ah, bh)
        E = float(ev.sum())
        with np.errstate(divide="ignore", invalid="ignore"):
            lhm = float(np.mean(np.log(lh)))                                         # :9
        ehm = float(np.mean(eh))                                                     # :11
        reason = 0
        if it > n0 and it % dn == 0:                                                 # :342
            ah1, bh1, failed, dfs = hyper_update_h(fa, fb, lhm, ehm, ah, bh)
            for df in dfs:
                newton_margin = min(newton_margin, abs(df - 1e-3) / 1e-3)
            if failed:
                reason = 5
            else:
                ah, bh = ah1, bh1
        history.append([E, lhm, ehm, ah, bh])
        if not reason:
            if math.isnan(E):                                                        # :345
                reason = 3
            else:
                conv = False
                if it > 1 and it > n0:
                    with np.errstate(divide="ignore", invalid="ignore"):
                        rel = float(np.abs(1 - np.float64(E) / np.float64(lk0)))
                    if math.isfinite(rel) and Tol > 0:
                        stop_margin = min(stop_margin, abs(rel - Tol) / Tol)
                    conv = rel < Tol                                                 # :346-347 without `lkh >= lk0`
                if conv:
                    reason = 1
                else:
                    lk0 = E                                                          # :348
                    if it >= Itmax:
                        reason = 4
        if reason:
            break
    return {"lh": lh, "eh": eh, "dh": dh, "ev": ev, "E": E, "it": it, "reason": reason, "hyper": (ah, bh),
            "history": np.array(history).reshape(-1, 5), "stop_margin": stop_margin, "newton_margin": newton_margin, "lk0": lk0}


def case(seed, a, b):
    """90 x 140, rank 5: q(W) with alw ~ U(0.5, 6), bew ~ U(0.02, 0.3); H ~ Gamma(shape a, scale b / a); x ~ Poisson(ew H), an
    empty column given one count in row 0; the default start -> dict(x, ew, sd, lw, lh0)."""
    rng = np.random.default_rng(seed)
    n, m, r = 90, 140, 5
    alw = rng.uniform(0.5, 6.0, size=(n, r))
    bew = rng.uniform(0.02, 0.3, size=(n, r))
    ew = alw * bew
    lw = np.exp(digamma(alw)) * bew
    H = rng.gamma(shape=a, scale=b / a, size=(r, m))
    x = rng.poisson(ew @ H).astype(np.float64)
    x[0, x.sum(axis=0) == 0] = 1.0
    x = np.asfortranarray(x)
    return {"x": x, "ew": ew, "sd": np.sqrt(alw) * bew, "lw": lw, "lh0": U.default_start(x, ew)}


# the conditioned cases of the GPU tests: (seed, (a, b) the counts are drawn with, (ah, bh) the projection starts from)
CONDITIONS = [(seed, ab, start) for seed in (1, 2) for ab, start in (((0.6, 3.0), (1.0, 1.0)), ((2.0, 0.5), (0.3, 2.0)))]
FLAGS = [(True, True), (False, True)]
