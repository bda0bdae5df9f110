"""numpy restatement of the per-cell VB projection loop (csrc/vbproject.h) -- TEST INFRASTRUCTURE ONLY.

Dense, statement by statement after the reference: the H half of ``vbnmf_updateR`` (R/bayesian.R:71-95) with q(W) -- ``lw``
and ``ew`` -- held, the cell's evidence (its column of U1, :90-91, plus its column of U3, :94-95; U2 belongs to W), and
``vb_iterate``'s stopping test (:345-347) applied to every cell on its own, without the ``lkh >= lk0`` clause and without the
``hyper.update.n0`` gate.  tests/test_vb_project_cpu.py ties one H half and the evidence to the
committed oracle (``oracle.vbnmf_oracle.update_dense``).
"""
import numpy as np
from scipy.special import digamma, gammaln

EPS = float(np.finfo(np.float64).eps)          # .Machine$double.eps


def h_half(x, lw, cew, lh, ah, bh, fudge=EPS):
    """R/bayesian.R:71, :73, :79-81, :84, :87, :103 with lw untouched and ``cew = colSums(ew)`` given -> (lh, eh, dh, alh)."""
    x = np.asarray(x, dtype=np.float64)
    lw = np.asarray(lw, dtype=np.float64)
    lh = np.asarray(lh, dtype=np.float64)
    cew = np.asarray(cew, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        wth = lw @ lh                                            # :71
        quo = np.where(x != 0, x / wth, 0.0)                     # (stored entries only, as the compressed columns hold them)
        sh = lh * (lw.T @ quo)                                   # :73
        alh = ah + sh                                            # :79
        beh = (1.0 / (ah / bh + cew))[:, None]                   # :80
        eh = alh * beh                                           # :81
        new = np.exp(digamma(alh)) * beh                         # :84
        new[new < fudge] = fudge                                 # :87  (NaN stays NaN)
        dh = alh * beh ** 2                                      # :103
    return new, eh, dh, alh


def cell_evidence(x, lw, cew, lh, eh, alh, ah, bh):
    """The column sums of U1 (:90-91) and U3 (:94-95) at the NEW lh, not divided by n m.  ``-ew %*% eh`` summed over a column
    is ``-sum_k colSums(ew)_k eh_k``; the x-terms of U1 vanish where x is 0."""
    x = np.asarray(x, dtype=np.float64)
    cew = np.asarray(cew, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        wth = lw @ lh                                            # :89
        inner = ((lw * np.log(lw)) @ lh + lw @ (lh * np.log(lh))) / wth - np.log(wth)
        u1 = -(cew[:, None] * eh).sum(axis=0) - gammaln(x + 1).sum(axis=0) - np.where(x != 0, x * inner, 0.0).sum(axis=0)
        beh = (1.0 / (ah / bh + cew))[:, None]
        u3 = -(ah / bh) * eh - gammaln(ah) + ah * np.log(ah / bh) + alh * (1 + np.log(beh)) + gammaln(alh)
    return u1 + u3.sum(axis=0)


def default_start(x, ew):
    """lh_kj = sum_i x_ij / sum_k colSums(ew)_k for every k."""
    x = np.asarray(x, dtype=np.float64)
    ew = np.asarray(ew, dtype=np.float64)
    return np.repeat((x.sum(axis=0) / ew.sum(axis=0).sum())[None, :], ew.shape[1], axis=0)


def project(x, lw, ew, lh0, ah, bh, fudge=EPS, Itmax=10000, Tol=1e-5):
    """Every cell iterated to its own stop -> dict(lh, eh, dh, ev, it, reason, margin).

    reason: 3 ev is NaN; 1 ``abs(1 - ev / lk0) < Tol`` after a step ``it > 1`` (lk0 = 0 before the first step); 4 Itmax.
    margin[j]: the smallest ``| |1 - ev / lk0| - Tol |`` the cell's decisions met -- how clear they were."""
    x = np.asarray(x, dtype=np.float64)
    lw = np.asarray(lw, dtype=np.float64)
    cew = np.asarray(ew, dtype=np.float64).sum(axis=0)
    lh = np.array(lh0, dtype=np.float64, copy=True)
    lh[lh < fudge] = fudge
    r, m = lh.shape
    eh, dh = np.zeros((r, m)), np.zeros((r, m))
    ev = np.full(m, np.nan)
    lk0 = np.zeros(m)
    it = np.zeros(m, dtype=np.int32)
    reason = np.zeros(m, dtype=np.int32)
    margin = np.full(m, np.inf)
    live = np.arange(m)
    for step in range(1, int(Itmax) + 1):
        if live.size == 0:
            break
        xs = x[:, live]
        ln, en, dn, al = h_half(xs, lw, cew, lh[:, live], ah, bh, fudge)
        evn = cell_evidence(xs, lw, cew, ln, en, al, ah, bh)
        lh[:, live], eh[:, live], dh[:, live] = ln, en, dn
        ev[live] = evn
        it[live] = step
        old = lk0[live]
        nan = np.isnan(evn)
        if step > 1:
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.abs(1 - evn / old)
            conv = rel < Tol
            fin = np.isfinite(rel)
            margin[live[fin]] = np.minimum(margin[live[fin]], np.abs(rel - Tol)[fin])
        else:
            conv = np.zeros(live.size, dtype=bool)
        why = np.where(nan, 3, np.where(conv, 1, 4 if step >= Itmax else 0)).astype(np.int32)
        reason[live] = why
        keep = why == 0
        lk0[live[keep]] = evn[keep]
        live = live[keep]
    return {"lh": lh, "eh": eh, "dh": dh, "ev": ev, "it": it, "reason": reason, "margin": margin}
