"""The two per-cell projection loops in 50-digit arithmetic (mpmath), and the cases the tests run them on -- TEST
INFRASTRUCTURE ONLY.

``ml_cell`` states csrc/project.h's cell (reference R/factorize.R:8-15 with w held, :40-49 of one column), ``vb_cell``
csrc/vbproject.h's (R/bayesian.R:71-95 with q(W) held: the H half and the cell's column of U1 and U3).  Both work on a cell's
stored entries only, so a step costs (entries x r) and not (n x r), and both take their start as doubles, so a second step can
start from a device result.  tests/test_project_mp_cpu.py ties them to the numpy restatements (tests/util_project.py,
tests/util_vb_project.py), which tests/test_project_cpu.py and tests/test_vb_project_cpu.py tie to the committed oracle;
tests/test_gpu_project_mp.py holds the kernels to them directly.

The bounds (``FACTOR_BOUND``, ``SUM_BOUND``) and the two guards are derived where they are defined below.
"""
import functools
from types import SimpleNamespace

import mpmath as mp
import numpy as np

mp.mp.dps = 50

EPS = 2.220446049250313e-16          # .Machine$double.eps
N_GENES = 560                        # (part of FACTOR_BOUND's derivation: do not raise it without redoing that sum)

# ---- bounds ------------------------------------------------------------------------------------------------------------------
# Factors (h; lh, eh, dh), largest relative error of one step against 50 digits: the figure tests/test_gpu_mpmath.py holds a
# full step to.  Here: every sum is of positive terms, so relative errors add and do not grow; the dot lambda_i adds at most
# 34 roundings (32 columns a lane, the shares of up to four lanes); the entry sum adds ceil(len / per) roundings in the slot,
# 6 butterfly levels and 3 wave adds; the host's sequential colSums adds at most (n - 1) u = 6.2e-14 at n = 560 in the worst
# case (sqrt(n) u = 2.6e-15 typically).  psi is held to 1.8e-15 max(1, |psi|) on the device (tests/util_special.py), and exp
# turns that absolute error into a relative one of the same size.
FACTOR_BOUND = 1e-13
# Likelihood and evidence: |got - ref| <= SUM_BOUND (sum_abs + nterms), sum_abs the sum of the absolute values of the terms
# that make the result and nterms their number.  Every term comes from a routine held to 1e-14 max(1, |term|) at worst (lgamma,
# tests/util_special.py), the summation tree adds <= 20 u sum_abs, and the factors' 1e-14-level error enters with O(1)
# sensitivity: about 2e-14 (sum_abs + nterms), which the bound gives a fivefold margin.  NOT relative to the result: the terms
# sum to about twenty times the evidence, and a bound relative to it could not tell the kernel's rounding from the reference's.
SUM_BOUND = 1e-13


def _f(v):
    return mp.mpf(float(v))


def col_sums(a):
    """colSums of a double matrix over all its rows, in 50 digits -> list of mpf (R/factorize.R:9, R/bayesian.R:80)."""
    a = np.asarray(a, dtype=np.float64)
    return [mp.fsum(_f(v) for v in a[:, k]) for k in range(a.shape[1])]


def _sums(v):
    return col_sums(v) if np.ndim(v) == 2 else list(v)


def _doubles(v):
    return np.array([float(t) for t in v], dtype=np.float64)


def ml_cell(rows, vals, W, h, prior=False, ga=1.0, gb=1.0, eps=EPS, iters=1, cw=None):
    """``iters`` steps of one cell of csrc/project.h in 50 digits, carried on in 50 digits from one step to the next.

    ``rows``, ``vals``: the cell's stored entries; ``W``: n x r doubles; ``h``: the start, r doubles; ``cw``: colSums(W) as
    ``col_sums`` gives it (None: taken here, over all n rows).  -> one dict per step: ``h`` (rounded to double), ``lk`` (mpf),
    ``sum_abs`` and ``nterms`` of the terms that make lk -- x_i log lambda_i, -cw_k h_k, -x_i log x_i, x_i --, and per
    component the numerator of :8 before (``up``) and after (``up_prior``) the ``+ gamma.a - 1`` of :11, as doubles."""
    W = np.asarray(W, dtype=np.float64)
    r = W.shape[1]
    w = [[_f(W[i, k]) for k in range(r)] for i in rows]
    x = [_f(v) for v in vals]
    cw = col_sums(W) if cw is None else list(cw)                              # :9
    a, b, e = _f(ga), _f(gb), _f(eps)
    dn = [c + a / b for c in cw] if prior else cw                             # :12
    hk = [_f(v) for v in h]
    zx = [-xi * mp.log(xi) for xi in x]                                       # :45-46 (stored entries are > 0)
    lam = [mp.fsum(wi[k] * hk[k] for k in range(r)) for wi in w]              # :8 w %*% h, the stored entries of the cell
    out = []
    for _ in range(int(iters)):
        q = [xi / li for xi, li in zip(x, lam)]
        up = [hk[k] * mp.fsum(wi[k] * qi for wi, qi in zip(w, q)) for k in range(r)]      # :8
        upp = [u + a - 1 for u in up] if prior else up                        # :11
        hk = [max(u / d, e) for u, d in zip(upp, dn)]                         # :14-15
        lam = [mp.fsum(wi[k] * hk[k] for k in range(r)) for wi in w]          # :42 at the new h
        t_data = [xi * mp.log(li) for xi, li in zip(x, lam)]                  # :44
        t_cross = [-cw[k] * hk[k] for k in range(r)]                          # :44  sum_i wh_i = sum_k colSums(w)_k h_k
        terms = t_data + t_cross + zx + x
        out.append({"h": _doubles(hk), "lk": mp.fsum(terms), "sum_abs": mp.fsum(abs(t) for t in terms), "nterms": len(terms),
                    "up": _doubles(up), "up_prior": _doubles(upp)})
    return out


def vb_cell(rows, vals, lw, cew_from_ew, lh, ah, bh, fudge=EPS, iters=1):
    """``iters`` steps of one cell of csrc/vbproject.h in 50 digits, carried on in 50 digits from one step to the next.

    ``lw``: n x r doubles (lw log lw is formed here, in 50 digits); ``cew_from_ew``: the n x r doubles ew, whose colSums are
    taken here over all n rows, or those sums as ``col_sums`` gives them; ``lh``: the start, r doubles.  -> one dict per step:
    ``lh``, ``eh``, ``dh``, ``alh`` (rounded to double), ``raw`` (exp(psi(alh)) beh before the floor of :87, as doubles),
    ``ev`` (mpf), ``sum_abs`` and ``nterms`` of the terms that make ev: per entry lgamma(x_i + 1), x_i (..)/lambda_i and
    x_i log lambda_i; per component cew_k eh_k, (ah/bh) eh_k, lgamma(ah), ah log(ah/bh), alh_k (1 + log beh_k), lgamma(alh_k)."""
    lw = np.asarray(lw, dtype=np.float64)
    r = lw.shape[1]
    w = [[_f(lw[i, k]) for k in range(r)] for i in rows]
    wl = [[v * mp.log(v) for v in wi] for wi in w]                            # :90 lw log(lw)
    x = [_f(v) for v in vals]
    cew = _sums(cew_from_ew)
    a, b, fud = _f(ah), _f(bh), _f(fudge)
    ab = a / b
    beh = [1 / (ab + c) for c in cew]                                         # :80
    lgx = [-mp.loggamma(xi + 1) for xi in x]                                  # :90
    lga = [-mp.loggamma(a), a * mp.log(ab)]                                   # :94
    hk = [_f(v) for v in lh]
    lam = [mp.fsum(wi[k] * hk[k] for k in range(r)) for wi in w]              # :71
    out = []
    for _ in range(int(iters)):
        q = [xi / li for xi, li in zip(x, lam)]
        alh = [a + hk[k] * mp.fsum(wi[k] * qi for wi, qi in zip(w, q)) for k in range(r)]         # :73, :79
        eh = [al * be for al, be in zip(alh, beh)]                            # :81
        dh = [al * be * be for al, be in zip(alh, beh)]                       # :103
        raw = [mp.exp(mp.digamma(al)) * be for al, be in zip(alh, beh)]       # :84
        hk = [max(v, fud) for v in raw]                                       # :87
        hl = [v * mp.log(v) for v in hk]                                      # :91 lh log(lh)
        lam = [mp.fsum(wi[k] * hk[k] for k in range(r)) for wi in w]          # :89
        g = [mp.fsum(wli[k] * hk[k] + wi[k] * hl[k] for k in range(r)) for wi, wli in zip(w, wl)]
        terms = list(lgx)
        terms += [-xi * gi / li for xi, gi, li in zip(x, g, lam)]             # :90-91
        terms += [xi * mp.log(li) for xi, li in zip(x, lam)]
        terms += [-c * v for c, v in zip(cew, eh)]                            # :90  the cell's column of ew %*% eh
        for k in range(r):                                                    # :94-95
            terms += [-ab * eh[k], lga[0], lga[1], alh[k] * (1 + mp.log(beh[k])), mp.loggamma(alh[k])]
        out.append({"lh": _doubles(hk), "eh": _doubles(eh), "dh": _doubles(dh), "alh": _doubles(alh), "raw": _doubles(raw),
                    "ev": mp.fsum(terms), "sum_abs": mp.fsum(abs(t) for t in terms), "nterms": len(terms)})
    return out


# ---- errors and guards ----------------------------------------------------------------------------------------------------
def relerr(got, want):
    """Largest relative error over ALL components (no exclusions)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.all(np.isfinite(got)) and np.all(want != 0)
    return float(np.max(np.abs(got - want) / np.abs(want)))


def sum_error(got, ref, key):
    """|got - ref[key]| / (sum_abs + nterms) of one cell's likelihood or evidence, the difference taken in 50 digits."""
    assert np.isfinite(got)
    return float(abs(_f(got) - ref[key]) / (ref["sum_abs"] + ref["nterms"]))


def clamp_guard(ref):
    """With the prior, no component's ``up + gamma.a - 1`` may cancel: |up + ga - 1| >= 1e-3 (|up| + 1).  Cancellation there
    makes any fp64 result arbitrarily far off in relative terms, and a value near eps flips the clamp of :15.  -> the smallest
    |up + ga - 1| / (|up| + 1) of the step."""
    return float(np.min(np.abs(ref["up_prior"]) / (np.abs(ref["up"]) + 1.0)))


def fudge_guard(ref, fudge):
    """No exp(psi(alh)) beh within a factor 2 of fudge, unless it is below fudge / 2 and so clearly clipped -> True if held."""
    raw = ref["raw"]
    return bool(np.all((raw > 2.0 * fudge) | (raw < 0.5 * fudge)))


# ---- cases: what the CPU and the GPU file run, drawn here once ---------------------------------------------------------------
WIDTHS = list(range(2, 33, 2)) + [40, 48, 56, 64] + [80, 96, 112, 128]       # the padded ranks with_rank instantiates
HYPERS = [(1.0, 1.0), (3.0, 0.3), (0.5, 9.0), (0.8, 1.5)]                      # (ah, bh) of util_mp_step.CASES
HYPER_FAR = (0.05, 2.0)               # psi(0.05) = -20.6: far negative, and exp() of it far from underflow; one step only
HYPER_WIDTHS = [6, 24, 40, 128]
EDGE_WIDTHS = [10, 24, 40, 128]
ML_EDGES = ["noninteger", "large", "fit", "floor", "prior", "prior_clamp"]
VB_EDGES = ["noninteger", "large", "fit", "floor"]
PRIOR = {"prior": (1.7, 0.6), "prior_clamp": (0.5, 1.0)}                      # in the second up + ga - 1 goes negative


def full_lengths(per):
    """Stored entries of the cells at r = R: one entry, two, and just below, at and above ONE pass of the workgroup and just
    above TWO."""
    return [1, 2, per - 1, per, per + 1, 2 * per + 1]


def short_lengths(per):
    return [1, 3, per + 1]


def edge_lengths(per):
    return [3, per + 1]


def draw_counts(n, lengths, rng, kind="integer"):
    """n x len(lengths) dense: column j holds lengths[j] stored entries, drawn as ``lengths_case`` of
    tests/test_gpu_vb_project.py draws them (30 % of the gene rows stay empty in every column short enough to leave them
    empty), counts 1..5.  ``noninteger``: counts x U(0.5, 1.5); ``large``: integers spread over 1e4..1e6, log-uniform."""
    rows = rng.permutation(n)
    used, spare = rows[: (7 * n) // 10], rows[(7 * n) // 10:]
    X = np.zeros((n, len(lengths)))
    for j, L in enumerate(lengths):
        take = rng.permutation(used)[:L]
        if L > used.size:
            take = np.concatenate((used, rng.permutation(spare)[:L - used.size]))
        v = rng.integers(1, 6, size=L).astype(np.float64)
        if kind == "noninteger":
            v = v * rng.uniform(0.5, 1.5, size=L)
        elif kind == "large":
            v = np.rint(10.0 ** rng.uniform(4.0, 6.0, size=L))
        X[take, j] = v
    assert [int(c) for c in (X > 0).sum(axis=0)] == list(lengths)
    return np.asfortranarray(X)


def fitted_magnitudes(n, r, rng):
    """A basis as a real ML fit leaves it: about a third of the entries exactly at the clamp of R/factorize.R:24, the rest
    spread over 1e-8..1e3, log-uniform; every gene row keeps at least one entry >= 1e-3."""
    W = 10.0 ** rng.uniform(-8.0, 3.0, size=(n, r))
    W[rng.uniform(size=(n, r)) < 1.0 / 3.0] = EPS
    for i in np.flatnonzero(W.max(axis=1) < 1e-3):
        W[i, rng.integers(0, r)] = 10.0 ** rng.uniform(-3.0, 3.0)
    return W


def floor_start(r, m, rng, floor):
    """U(0.05, 1) with about half of every cell's components AT the floor (component 0 always, component 1 never)."""
    h = rng.uniform(0.05, 1.0, size=(r, m))
    at = rng.uniform(size=(r, m)) < 0.5
    at[0] = True
    if r > 1:
        at[1] = False
    h[at] = floor
    return h


def cells_of(X):
    return [(np.flatnonzero(X[:, j]), X[np.flatnonzero(X[:, j]), j]) for j in range(X.shape[1])]


# Seeds are chosen so that the guards hold with zero components excluded (tests/test_project_mp_cpu.py asserts them); where
# a default seed did not, the one used is listed here.  Key: (kernel, r, edge).
SEEDS = {
    # 256 components a step lie densely around up = 1 - ga = 0.5; the default seed left one at 2.3e-3 (|up| + 1), inside the
    # guard but with up's rounding error amplified 140-fold in h; of thirty seeds tried this one keeps the widest distance
    # (8.9e-3 and 1.6e-2 in steps 1 and 2, a 37-fold amplification at most)
    ("ml", 128, "prior_clamp"): 12814,
}


def _seed(kernel, r, edge):
    default = (100000 if kernel == "vb" else 0) + 100 * r + (["plain"] + ML_EDGES).index(edge)
    return SEEDS.get((kernel, r, edge), default)


@functools.lru_cache(maxsize=None)
def ml_case(r, lengths, edge="plain"):
    """Inputs of k_project at rank r over cells of ``lengths`` (a tuple) stored entries: basis U(0.05, 1), start U(0.05, 1),
    counts 1..5, no prior -- or the value edge ``edge`` of ML_EDGES."""
    rng = np.random.default_rng(_seed("ml", r, edge))
    n, m = N_GENES, len(lengths)
    X = draw_counts(n, lengths, rng, edge if edge in ("noninteger", "large") else "integer")
    W = fitted_magnitudes(n, r, rng) if edge == "fit" else rng.uniform(0.05, 1.0, size=(n, r))
    h0 = floor_start(r, m, rng, EPS) if edge == "floor" else rng.uniform(0.05, 1.0, size=(r, m))
    ga, gb = PRIOR.get(edge, (1.0, 1.0))
    return SimpleNamespace(r=r, X=X, cells=cells_of(X), W=W, h0=h0, prior=edge in PRIOR, ga=ga, gb=gb, cw=col_sums(W),
                           name=f"ml r={r} {edge} lengths={list(lengths)}")


def ml_steps(case, h, iters):
    """The 50-digit steps of every cell of ``case`` from the start ``h`` (r x cells doubles) -> [cell][step] dicts."""
    return [ml_cell(rows, vals, case.W, h[:, j], case.prior, case.ga, case.gb, EPS, iters, cw=case.cw)
            for j, (rows, vals) in enumerate(case.cells)]


@functools.lru_cache(maxsize=None)
def ml_reference(r, lengths, edge="plain", iters=1):
    case = ml_case(r, lengths, edge)
    return ml_steps(case, case.h0, iters)


@functools.lru_cache(maxsize=None)
def vb_case(r, lengths, edge="plain", ah=0.8, bh=1.7, fudge=EPS):
    """Inputs of k_vb_project at rank r: q(W) from ``posterior()`` of tests/test_gpu_vb_project.py, start U(0.05, 1), counts
    1..5 -- or the value edge ``edge`` of VB_EDGES (``fit``: lw of a fitted basis' magnitudes, ew = lw x U(1, 3), as E[W] lies
    above the geometric mean)."""
    from test_gpu_vb_project import posterior
    rng = np.random.default_rng(_seed("vb", r, edge))
    n, m = N_GENES, len(lengths)
    X = draw_counts(n, lengths, rng, edge if edge in ("noninteger", "large") else "integer")
    if edge == "fit":
        lw = fitted_magnitudes(n, r, rng)
        ew = lw * rng.uniform(1.0, 3.0, size=(n, r))
    else:
        ew, _sd, lw = posterior(n, r, rng)
    lh0 = floor_start(r, m, rng, fudge) if edge == "floor" else rng.uniform(0.05, 1.0, size=(r, m))
    return SimpleNamespace(r=r, X=X, cells=cells_of(X), lw=lw, ew=ew, lh0=lh0, ah=ah, bh=bh, fudge=fudge, cew=col_sums(ew),
                           name=f"vb r={r} {edge} ah={ah} bh={bh} fudge={fudge} lengths={list(lengths)}")


def vb_steps(case, lh, iters):
    """The 50-digit steps of every cell of ``case`` from the start ``lh`` (r x cells doubles) -> [cell][step] dicts."""
    return [vb_cell(rows, vals, case.lw, case.cew, lh[:, j], case.ah, case.bh, case.fudge, iters)
            for j, (rows, vals) in enumerate(case.cells)]


@functools.lru_cache(maxsize=None)
def vb_reference(r, lengths, edge="plain", ah=0.8, bh=1.7, fudge=EPS, iters=1):
    case = vb_case(r, lengths, edge, ah, bh, fudge)
    return vb_steps(case, case.lh0, iters)


def ml_errors(h, lk, refs, step):
    """(r x cells h, per-cell lk) against step ``step`` of ``refs`` -> (largest relative error of h, largest
    |lk - ref| / (sum_abs + nterms))."""
    return relerr(h, stack(refs, step, "h")), max(sum_error(lk[j], c[step], "lk") for j, c in enumerate(refs))


def vb_errors(lh, eh, dh, ev, refs, step):
    """-> (largest relative errors of lh, eh, dh, largest |ev - ref| / (sum_abs + nterms))."""
    return (relerr(lh, stack(refs, step, "lh")), relerr(eh, stack(refs, step, "eh")), relerr(dh, stack(refs, step, "dh")),
            max(sum_error(ev[j], c[step], "ev") for j, c in enumerate(refs)))


def stack(refs, step, key):
    """[cell][step] dicts -> r x cells doubles of ``key`` at ``step``."""
    return np.stack([c[step][key] for c in refs], axis=1)
