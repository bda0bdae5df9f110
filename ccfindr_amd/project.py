"""Placing new cells on a fitted basis: ML-NMF with W held fixed (``vbnmf_matrix_project``, include/vbnmf.h).

The mathematics is the reference's own: the H half of ``nmf_updateR`` (reference R/factorize.R:8-15) iterated with ``w``
untouched, ``likelihood`` (:40-49) taken column by column, and ``factorize()``'s stopping test (:208) applied to every cell on
its own -- with W fixed nothing couples two cells.  The kernel (csrc/project.h) reads the matrix's compressed columns as they
are: no tiled layout is cut and no engine is created.  No CPU fallback: without the HIP library every call raises.

``vb_project`` is the same for a variational-Bayes fit (``vbnmf_matrix_vb_project``, csrc/vbproject.h): the H half of
``vbnmf_updateR`` (reference R/bayesian.R:71-95) under the fitted posterior q(W) and the fitted hyper-parameters, giving E[H],
sd[H] and an evidence term per cell.  With ``hyper_update=`` or ``stop="global"`` it is the H half of ``vb_iterate`` instead
(``vbnmf_matrix_vb_project_coupled``): the prior of H is re-estimated on the new cells as the loop goes (R/bayesian.R:342-344)
and all cells stop together.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np

from . import _native as N
from .engine import EPS, CountMatrix

REASONS = {1: "converged", 3: "NaN likelihood", 4: "Itmax reached", 5: "hyper-parameter update failed to converge"}


@dataclass
class Projection:
    """Coefficients of the projected cells; ``ranks`` / ``coeff`` as in ``MLResult``, so ``cluster_id(p, rank=r)`` reads it."""
    ranks: list = field(default_factory=list)
    basis: list = field(default_factory=list)       # the basis the cells were placed on, n x r
    coeff: list = field(default_factory=list)       # h, r x m
    cell_likelihood: np.ndarray = None              # :40-49 of every column, not divided by n m
    nsteps: np.ndarray = None                       # iterations of every cell
    reason: np.ndarray = None                       # why every cell stopped: 1 converged, 3 NaN likelihood, 4 Itmax
    likelihood: float = float("nan")                # likelihood(mat, W, H) of :40-49


def pass_entries(rank):
    """Stored entries of one cell that the kernel's workgroup takes in one pass of its threads at ``rank``; a longer column
    goes round again (``vbnmf_project_info``)."""
    v = ctypes.c_int32()
    N.check(N.load().vbnmf_project_info(int(rank), ctypes.byref(v), None))
    return v.value


def last_kernel_ms():
    """Kernel time of this thread's most recent ``project`` call, in ms."""
    v = ctypes.c_double()
    N.check(N.load().vbnmf_project_info(1, None, ctypes.byref(v)))
    return v.value


def _basis_of(basis, rank):
    if hasattr(basis, "ranks") and hasattr(basis, "basis"):
        if rank is None:
            if len(basis.ranks) != 1:
                raise ValueError("rank= is needed to pick one basis of a result that holds several ranks")
            rank = basis.ranks[0]
        hits = [i for i, r in enumerate(basis.ranks) if r == rank]
        if not hits:
            raise IndexError("subscript out of bounds")
        return np.asarray(basis.basis[hits[0]], dtype=np.float64)
    W = np.asarray(basis, dtype=np.float64)
    if W.ndim != 2:
        raise ValueError("basis must be an n x r matrix, or a factorisation result together with rank=")
    if rank is not None and int(rank) != W.shape[1]:
        raise ValueError(f"rank={rank} does not match the basis' {W.shape[1]} columns")
    return W


def default_start(M, W):
    """The deterministic start ``h_kj = sum_i x_ij / sum_k colSums(w)_k`` for every k (``M``: a ``CountMatrix`` without empty
    columns): ``sum(w h) = sum(x)`` in every cell."""
    cp, ri, xv = N.c_int64_p(), N.c_int32_p(), N.c_double_p()
    N.check(M._lib.vbnmf_matrix_csc(M._h, ctypes.byref(cp), ctypes.byref(ri), ctypes.byref(xv)))
    m = M.shape[1]
    indptr = np.ctypeslib.as_array(cp, shape=(m + 1,))
    data = np.ctypeslib.as_array(xv, shape=(max(M.nnz, 1),))[:M.nnz]
    csum = np.add.reduceat(data, indptr[:-1])                # (views of the handle's arrays: nothing is copied)
    W = np.asarray(W, dtype=np.float64)
    return np.repeat((csum / W.sum(axis=0).sum())[None, :], W.shape[1], axis=0)


def project_columns(M, W, H, col_begin, col_end, prior=False, gamma_a=1.0, gamma_b=1.0, Itmax=10000, Tol=1e-5, device=0):
    """``vbnmf_matrix_project`` on cells ``[col_begin, col_end)`` of the ``CountMatrix`` ``M``: ``H`` (r x cells, the start)
    -> ``(H, cell_likelihood, nsteps, reason)``.  No argument is vetted here beyond what the library checks itself."""
    W = N.fcol(W)
    r = W.shape[1]
    nc = int(col_end) - int(col_begin)
    Hout = np.array(H, dtype=np.float64, order="F", copy=True)
    lk = np.empty(max(nc, 0))
    it = np.zeros(max(nc, 0), dtype=np.int32)
    why = np.zeros(max(nc, 0), dtype=np.int32)
    N.check(N.load().vbnmf_matrix_project(M._h, int(col_begin), int(col_end), int(r), N.dptr(W), N.dptr(Hout), int(bool(prior)),
                                          float(gamma_a), float(gamma_b), int(Itmax), float(Tol), int(device), N.dptr(lk),
                                          it.ctypes.data_as(N.c_int32_p), why.ctypes.data_as(N.c_int32_p)))
    return Hout, lk, it, why


def project(mat, basis, rank=None, prior=False, gamma_a=1.0, gamma_b=1.0, Itmax=10000, Tol=1e-5, h0=None, device=0):
    """Coefficients of the cells of ``mat`` on a fixed ``basis``, every cell iterated to its own stop on the device.

    ``mat``: genes x new cells (dense array, scipy sparse, or ``CountMatrix``), the genes of the basis in the basis' order.
    ``basis``: an n x r array, or an ``MLResult`` / ``VBResult`` (its ``basis`` of ``rank``; a ``VBResult``'s E[W] serves as a
    point estimate).  ``prior``, ``gamma_a``, ``gamma_b``: the Gamma prior of R/factorize.R:10-13.  ``Itmax``, ``Tol``: the
    bounds of :208, per cell.  ``h0``: the start, r x m, clipped at eps; None: ``h_kj = sum_i x_ij / sum_k colSums(w)_k``
    for every k, which makes ``sum(w h) = sum(x)`` in every cell.  Returns ``Projection``.
    """
    W = _basis_of(basis, rank)
    n, r = W.shape
    own = not isinstance(mat, CountMatrix)
    M = CountMatrix(mat) if own else mat
    try:
        if M.is_shell:
            raise ValueError("a shell matrix holds no entries: project needs the matrix itself")
        nrow, m = M.shape
        if nrow != n:
            raise ValueError(f"mat has {nrow} rows (genes) but the basis has {n}")
        if r > n:
            raise ValueError(f"rank {r} exceeds the number of rows {n}")
        if r < 1 or r > N.MAX_RANK:
            raise ValueError(f"rank {r} is outside [1, {N.MAX_RANK}]")
        if int(Itmax) < 1:
            raise ValueError("Itmax must be at least 1")
        if M.empty_counts()[1] > 0:
            raise ValueError("Input matrix contains empty columns")                # R/factorize.R:152
        if h0 is None:
            H = default_start(M, W)
        else:
            H = np.array(h0, dtype=np.float64, copy=True)
            if H.shape != (r, m):
                raise ValueError(f"h0 must be {r} x {m}")
        H[H < EPS] = EPS                                                           # (NaN stays NaN)
        H, lk, it, why = project_columns(M, W, H, 0, m, prior, gamma_a, gamma_b, Itmax, Tol, device)
    finally:
        if own:
            M.close()
    return Projection(ranks=[r], basis=[W], coeff=[H], cell_likelihood=lk, nsteps=it, reason=why,
                      likelihood=float(lk.sum() / n / m))


# ---- the same for a VB fit: the H half of the VB update under the fitted posterior q(W) (vbnmf_matrix_vb_project) -----------
@dataclass
class VBProjection:
    """Posterior of the projected cells' coefficients; ``ranks`` / ``coeff`` / ``dcoeff`` as in ``VBResult``, so
    ``cluster_id(p, rank=r)`` reads it."""
    ranks: list = field(default_factory=list)
    basis: list = field(default_factory=list)       # E[W] of the posterior the cells were placed on, n x r
    dbasis: list = field(default_factory=list)      # sd[W]
    coeff: list = field(default_factory=list)       # E[H], r x m
    dcoeff: list = field(default_factory=list)      # sd[H] = sqrt(dh)
    lcoeff: list = field(default_factory=list)      # lh = exp(E[log H]): pass it as lh0= to resume
    cell_evidence: np.ndarray = None                # the cell's columns of U1 + U3 (R/bayesian.R:90-91, :94-95), not / (n m)
    nsteps: np.ndarray = None                       # iterations of every cell
    reason: np.ndarray = None                       # why every cell stopped: 1 converged, 3 NaN evidence, 4 Itmax, 5 (REASONS)
    hyper: dict = field(default_factory=dict)       # ah, bh the cells were placed under (the final pair of a coupled run)
    lml_cells: float = float("nan")                 # sum(cell_evidence) / (n m)
    evidence: float = float("nan")                  # E = sum(cell_evidence); of a coupled run: as its control step summed it
    hyper0: dict = field(default_factory=dict)      # ah, bh the projection started from
    history: np.ndarray = None                      # coupled run with history=True: a row [E, mean(log lh), mean(eh), ah, bh] per step


def vb_pass_entries(rank):
    """Stored entries of one cell that the VB kernel's workgroup takes in one pass of its threads at ``rank``
    (``vbnmf_vb_project_info``)."""
    v = ctypes.c_int32()
    N.check(N.load().vbnmf_vb_project_info(int(rank), ctypes.byref(v), None))
    return v.value


def vb_last_kernel_ms():
    """Kernel time of this thread's most recent ``vb_project`` call, in ms."""
    v = ctypes.c_double()
    N.check(N.load().vbnmf_vb_project_info(1, None, ctypes.byref(v)))
    return v.value


def _posterior_parts(res, rank, hyper):
    """-> (ew, sd, ah, bh) of a ``VBResult`` at ``rank`` or of an ``(ew, sd)`` pair, vetted."""
    if hasattr(res, "ranks") and hasattr(res, "basis"):
        if not hasattr(res, "dbasis"):
            raise ValueError("a VB projection needs a VBResult (basis and dbasis); an MLResult holds a point estimate: use project()")
        if rank is None:
            if len(res.ranks) != 1:
                raise ValueError("rank= is needed to pick one basis of a result that holds several ranks")
            rank = res.ranks[0]
        hits = [i for i, r in enumerate(res.ranks) if r == rank]
        if not hits:
            raise IndexError("subscript out of bounds")
        i = hits[0]
        if len(res.dbasis) <= i or res.dbasis[i] is None:
            raise ValueError(f"the result holds no dbasis for rank {rank}")
        ew, sd = res.basis[i], res.dbasis[i]
        measure = getattr(res, "measure", None) or {}
        own = {k: measure[k][i] for k in ("ah", "bh") if k in measure and len(measure[k]) > i}
        hyper = {**own, **(hyper or {})}
    else:
        try:
            ew, sd = res
        except (TypeError, ValueError):
            raise ValueError("a VBResult or an (ew, sd) pair of n x r arrays is needed") from None
    if hyper is None or "ah" not in hyper or "bh" not in hyper:
        raise ValueError('hyper={"ah": .., "bh": ..} is needed: the pair, or the result\'s measure, holds none')
    ew = np.asarray(ew, dtype=np.float64)
    sd = np.asarray(sd, dtype=np.float64)
    if ew.ndim != 2 or ew.shape != sd.shape:
        raise ValueError(f"ew {ew.shape} and sd {sd.shape} must be n x r matrices of one shape")
    if rank is not None and int(rank) != ew.shape[1]:
        raise ValueError(f"rank={rank} does not match the basis' {ew.shape[1]} columns")
    if not (np.all(ew > 0) and np.all(sd > 0)):
        raise ValueError("ew and sd must be positive everywhere (mean and sd of Gamma posteriors)")
    ah, bh = float(hyper["ah"]), float(hyper["bh"])
    if not (ah > 0 and bh > 0):
        raise ValueError("ah and bh must be > 0")
    return ew, sd, ah, bh


def posterior_basis(result_or_pair, rank=None, hyper=None, fudge=EPS):
    """What the H half of the VB update reads of a fitted q(W) -> ``(lw, ew, ah, bh)``.

    q(W_ik) is Gamma with shape ``alw`` and scale ``bew``; a fit stores ``ew = alw bew`` (its ``basis``) and
    ``sd = sqrt(alw) bew`` (its ``dbasis``; reference R/bayesian.R:75-77, :102, :380-382), so ``bew = sd^2 / ew``,
    ``alw = (ew / sd)^2`` and ``lw = exp(digamma(alw)) bew`` (:83).  ``result_or_pair``: a ``VBResult`` (its ``basis``,
    ``dbasis`` and the ``ah``, ``bh`` of ``measure`` at ``rank``), or an ``(ew, sd)`` pair of n x r arrays together with
    ``hyper={"ah": .., "bh": ..}``.  With a result, ``hyper`` overrides its own ``ah`` / ``bh``.  ``fudge``: the floor the fit
    held ``lw`` at (:85-86).  (n r values of digamma, once per fit, on the host: the per-cell iteration is the device's.)"""
    lw, ew, _sd, ah, bh = _posterior(result_or_pair, rank, hyper, fudge)
    return lw, ew, ah, bh


def _posterior(res, rank, hyper, fudge):
    """-> (lw, ew, sd, ah, bh): ``posterior_basis`` together with the sd it was rebuilt from."""
    from scipy.special import digamma
    ew, sd, ah, bh = _posterior_parts(res, rank, hyper)
    q = ew / sd
    lw = np.exp(digamma(q * q)) * (sd * sd / ew)             # :83 with alw = (ew / sd)^2, bew = sd^2 / ew
    lw[lw < fudge] = fudge                                   # :86
    return lw, ew, sd, ah, bh


def vb_project_columns(M, lw, ew, lh, ah, bh, col_begin, col_end, fudge=EPS, Itmax=10000, Tol=1e-5, device=0):
    """``vbnmf_matrix_vb_project`` on cells ``[col_begin, col_end)`` of the ``CountMatrix`` ``M``: ``lh`` (r x cells, the
    start) -> ``(lh, eh, dh, cell_evidence, nsteps, reason)``.  No argument is vetted here beyond what the library checks
    itself."""
    lw, ew = N.fcol(lw), N.fcol(ew)
    r = lw.shape[1]
    nc = int(col_end) - int(col_begin)
    lh = np.array(lh, dtype=np.float64, order="F", copy=True)
    eh, dh = np.zeros_like(lh, order="F"), np.zeros_like(lh, order="F")
    ev = np.empty(max(nc, 0))
    it = np.zeros(max(nc, 0), dtype=np.int32)
    why = np.zeros(max(nc, 0), dtype=np.int32)
    N.check(N.load().vbnmf_matrix_vb_project(M._h, int(col_begin), int(col_end), int(r), N.dptr(lw), N.dptr(ew), float(ah), float(bh),
                                             float(fudge), N.dptr(lh), N.dptr(eh), N.dptr(dh), int(Itmax), float(Tol), int(device),
                                             N.dptr(ev), it.ctypes.data_as(N.c_int32_p), why.ctypes.data_as(N.c_int32_p)))
    return lh, eh, dh, ev, it, why


def vb_project_coupled_columns(M, lw, ew, lh, ah, bh, col_begin, col_end, hyper_update=(False, False), n0=10, dn=1, fudge=EPS,
                               Itmax=10000, Tol=1e-5, device=0, history_rows=0):
    """``vbnmf_matrix_vb_project_coupled`` on cells ``[col_begin, col_end)`` of the ``CountMatrix`` ``M``: ``lh`` (r x cells,
    the start) -> ``(lh, eh, dh, cell_evidence, nsteps, reason, (ah, bh), it, why, evidence, history)``; ``history`` holds the
    rows of the steps made (at most ``history_rows``), or is None.  No argument is vetted here beyond what the library checks
    itself."""
    lw, ew = N.fcol(lw), N.fcol(ew)
    r = lw.shape[1]
    nc = int(col_end) - int(col_begin)
    lh = np.array(lh, dtype=np.float64, order="F", copy=True)
    eh, dh = np.zeros_like(lh, order="F"), np.zeros_like(lh, order="F")
    ev = np.empty(max(nc, 0))
    it = np.zeros(max(nc, 0), dtype=np.int32)
    why = np.zeros(max(nc, 0), dtype=np.int32)
    hy = np.array([ah, bh], dtype=np.float64)
    flags = np.array([bool(hyper_update[0]), bool(hyper_update[1])], dtype=np.int32)
    rows = max(int(history_rows), 0)
    hist = np.full((rows, 5), np.nan) if rows else None
    steps, stop, E = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double(float("nan"))
    N.check(N.load().vbnmf_matrix_vb_project_coupled(M._h, int(col_begin), int(col_end), int(r), N.dptr(lw), N.dptr(ew), N.dptr(hy),
                                                     flags.ctypes.data_as(N.c_int32_p), int(n0), int(dn), float(fudge), N.dptr(lh),
                                                     N.dptr(eh), N.dptr(dh), int(Itmax), float(Tol), int(device), N.dptr(ev),
                                                     it.ctypes.data_as(N.c_int32_p), why.ctypes.data_as(N.c_int32_p),
                                                     ctypes.byref(steps), ctypes.byref(stop), ctypes.byref(E), N.dptr(hist), rows))
    if hist is not None:
        hist = hist[:min(rows, steps.value)]
    return lh, eh, dh, ev, it, why, (float(hy[0]), float(hy[1])), steps.value, stop.value, E.value, hist


def _coupled_mode(hyper_update, stop, hyper_n0, hyper_dn):
    """-> (coupled?, (fa, fb)) of ``vb_project``'s arguments, vetted; touches no device."""
    if hyper_update is None:
        flags = (False, False)
    else:
        try:
            fa, fb = hyper_update
        except (TypeError, ValueError):
            raise ValueError("hyper_update must be a pair (update ah?, update bh?)") from None
        flags = (bool(fa), bool(fb))
    if stop is None:
        stop = "global" if any(flags) else "cell"
    if stop not in ("cell", "global"):
        raise ValueError(f'stop must be "cell" or "global", not {stop!r}')
    if stop == "cell" and any(flags):
        raise ValueError('stop="cell" cannot go with hyper_update: an updated hyper-parameter couples the cells (stop="global")')
    if int(hyper_dn) < 1:
        raise ValueError("hyper_dn must be at least 1")
    if int(hyper_n0) < 0:
        raise ValueError("hyper_n0 must be at least 0")
    return stop == "global", flags


def vb_project(mat, result, rank=None, hyper=None, Itmax=10000, Tol=1e-5, fudge=EPS, lh0=None, device=0, hyper_update=None, stop=None,
               hyper_n0=10, hyper_dn=1, history=False):
    """Posterior of the coefficients of the cells of ``mat`` under a fitted q(W), every cell iterated to its own stop on
    the device -- or, with ``hyper_update`` / ``stop="global"``, all cells together with the prior of H re-estimated on them.

    ``mat``: genes x new cells (dense array, scipy sparse, or ``CountMatrix``), the genes of the fit in the fit's order.
    ``result``: a ``VBResult`` (its ``basis``, ``dbasis`` and hyper-parameters of ``rank``) or an ``(ew, sd)`` pair with
    ``hyper={"ah": .., "bh": ..}`` (``posterior_basis``).  ``Itmax``, ``Tol``: the bounds of R/bayesian.R:345-347, per cell
    (without the ``lkh >= lk0`` clause).  ``lh0``: the start, r x m, clipped at ``fudge``; None:
    ``lh_kj = sum_i x_ij / sum_k colSums(ew)_k`` for every k.  Returns ``VBProjection``.

    ``hyper_update=(ah?, bh?)``: re-estimate the marked hyper-parameters of H on the cells of ``mat`` from step
    ``hyper_n0 + 1`` on, every ``hyper_dn`` steps, as ``vb_iterate`` does (R/bayesian.R:342-344, ``hyper_update`` :2-53; the
    reference sets ``bh`` to mean(E[H]) when either is marked).  The fit's own ``ah``, ``bh`` are the start (``hyper0`` of the
    result; ``hyper`` is the final pair).  The cells are then coupled and stop together: ``stop="global"`` applies :345-347 to
    the cells' total evidence (``evidence``), gate ``it > hyper_n0`` included, and is the default with a marked
    hyper-parameter; ``stop="cell"`` (the default without) is each cell's own stop.  ``stop="global"`` without
    ``hyper_update`` takes the per-cell steps under the global rule.  ``history=True`` keeps a row
    ``[E, mean(log lh), mean(E[H]), ah, bh]`` per step.  ``reason`` 5: the hyper-parameter update failed to converge.
    """
    coupled, flags = _coupled_mode(hyper_update, stop, hyper_n0, hyper_dn)
    lw, ew, sd, ah, bh = _posterior(result, rank, hyper, fudge)
    n, r = ew.shape
    own = not isinstance(mat, CountMatrix)
    M = CountMatrix(mat) if own else mat
    try:
        if M.is_shell:
            raise ValueError("a shell matrix holds no entries: vb_project needs the matrix itself")
        nrow, m = M.shape
        if nrow != n:
            raise ValueError(f"mat has {nrow} rows (genes) but the basis has {n}")
        if r > n:
            raise ValueError(f"rank {r} exceeds the number of rows {n}")
        if r < 1 or r > N.MAX_RANK:
            raise ValueError(f"rank {r} is outside [1, {N.MAX_RANK}]")
        if int(Itmax) < 1:
            raise ValueError("Itmax must be at least 1")
        if M.empty_counts()[1] > 0:
            raise ValueError("Input matrix contains empty columns")                # R/bayesian.R:247
        if lh0 is None:
            lh = default_start(M, ew)                                               # (on E[W])
        else:
            lh = np.array(lh0, dtype=np.float64, copy=True)
            if lh.shape != (r, m):
                raise ValueError(f"lh0 must be {r} x {m}")
        lh[lh < fudge] = fudge                                                     # (NaN stays NaN)
        if coupled:
            lh, eh, dh, ev, it, why, (ah1, bh1), _steps, _why, E, hist = vb_project_coupled_columns(
                M, lw, ew, lh, ah, bh, 0, m, flags, hyper_n0, hyper_dn, fudge, Itmax, Tol, device,
                history_rows=min(int(Itmax), 1 << 20) if history else 0)
        else:
            lh, eh, dh, ev, it, why = vb_project_columns(M, lw, ew, lh, ah, bh, 0, m, fudge, Itmax, Tol, device)
            ah1, bh1, E, hist = ah, bh, float(ev.sum()), None
    finally:
        if own:
            M.close()
    return VBProjection(ranks=[r], basis=[ew], dbasis=[sd], coeff=[eh], dcoeff=[np.sqrt(dh)], lcoeff=[lh], cell_evidence=ev,
                        nsteps=it, reason=why, hyper={"ah": ah1, "bh": bh1}, lml_cells=float(ev.sum() / n / m), evidence=E,
                        hyper0={"ah": ah, "bh": bh}, history=hist)
