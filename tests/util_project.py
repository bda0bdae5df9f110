"""numpy restatement of the per-cell projection loop (csrc/project.h) -- TEST INFRASTRUCTURE ONLY.

Dense, statement by statement after the reference: the H half of ``nmf_updateR`` (R/factorize.R:8-15) with ``w`` held, the
W half (:17-24) for the tie to the committed oracle, ``likelihood`` (:40-49) column by column, and ``factorize()``'s stopping
test (:208) applied to every cell on its own.  tests/test_project_cpu.py holds one H half followed by the W half to
``oracle.mlnmf_oracle.nmf_update_literal`` and the per-cell likelihoods to ``likelihood_literal``.
"""
import numpy as np

EPS = float(np.finfo(np.float64).eps)          # .Machine$double.eps


def h_half(x, w, h, prior=False, gamma_a=1.0, gamma_b=1.0):
    """R/factorize.R:8-15 with w untouched -> the new h."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    m = x.shape[1]
    with np.errstate(divide="ignore", invalid="ignore"):
        up = h * (w.T @ (x / (w @ h)))                       # :8
        down = np.repeat(w.sum(axis=0)[:, None], m, axis=1)  # :9
        if prior:
            up = up + gamma_a - 1                            # :11
            down = down + gamma_a / gamma_b                  # :12
        h = up / down                                        # :14
    h[h < EPS] = EPS                                         # :15  (NaN stays NaN)
    return h


def w_half(x, w, h, prior=False, gamma_a=1.0, gamma_b=1.0):
    """R/factorize.R:17-24 on the NEW h -> the new w."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    up = w * ((x / (w @ h)) @ h.T)                           # :17
    down = np.repeat(h.sum(axis=1)[None, :], n, axis=0)      # :18
    if prior:
        up = up + gamma_a - 1                                # :20
        down = down + gamma_a / gamma_b                      # :21
    w = up / down                                            # :23
    w[w < EPS] = EPS                                         # :24
    return w


def cell_likelihood(x, w, h):
    """R/factorize.R:40-49 of every column, not divided by n m: their sum / n / m is likelihood(x, w, h)."""
    x = np.asarray(x, dtype=np.float64)
    wh = np.asarray(w) @ np.asarray(h)                       # :42
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(x > 0, x * np.log(wh), 0.0 * wh) - wh   # :44  (0 * log(wh): 0 for wh > 0, NaN where R's is NaN)
        z = np.where(x > 0, -x * np.log(np.where(x > 0, x, 1.0)) + x, 0.0)       # :45-46
    return t.sum(axis=0) + z.sum(axis=0)


def default_start(x, w):
    """h_kj = sum_i x_ij / sum_k colSums(w)_k for every k."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    return np.repeat((x.sum(axis=0) / w.sum(axis=0).sum())[None, :], w.shape[1], axis=0)


def project(x, w, h0, prior=False, gamma_a=1.0, gamma_b=1.0, Itmax=10000, Tol=1e-5):
    """Every cell iterated to its own stop -> dict(h, lk, it, reason, margin).

    reason: 1 ``abs(lkold - lk) < Tol * abs(lkold)`` (:208, lkold = -Inf before the first step), 3 lk is NaN, 4 Itmax.
    margin[j]: the smallest ``| |lkold - lk| / |lkold| - Tol |`` the cell's decisions met -- how clear they were."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    h = np.array(h0, dtype=np.float64, copy=True)
    h[h < EPS] = EPS
    m = x.shape[1]
    lk = np.full(m, np.nan)
    lkold = np.full(m, -np.inf)
    it = np.zeros(m, dtype=np.int32)
    reason = np.zeros(m, dtype=np.int32)
    margin = np.full(m, np.inf)
    live = np.arange(m)
    for step in range(1, int(Itmax) + 1):
        if live.size == 0:
            break
        hn = h_half(x[:, live], w, h[:, live], prior, gamma_a, gamma_b)
        ln = cell_likelihood(x[:, live], w, hn)
        h[:, live] = hn
        lk[live] = ln
        it[live] = step
        old = lkold[live]
        with np.errstate(invalid="ignore"):
            conv = np.abs(old - ln) < Tol * np.abs(old)
            rel = np.abs(np.abs(old - ln) / np.abs(old) - Tol)
        nan = np.isnan(ln)
        fin = np.isfinite(old) & ~nan
        margin[live[fin]] = np.minimum(margin[live[fin]], rel[fin])
        why = np.where(nan, 3, np.where(conv, 1, 4 if step >= Itmax else 0)).astype(np.int32)
        reason[live] = why
        keep = why == 0
        lkold[live[keep]] = ln[keep]
        live = live[keep]
    return {"h": h, "lk": lk, "it": it, "reason": reason, "margin": margin}
