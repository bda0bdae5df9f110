"""Placing new cells on a fitted basis: ML-NMF with W held fixed (``vbnmf_matrix_project``, include/vbnmf.h).

The mathematics is the reference's own: the H half of ``nmf_updateR`` (reference R/factorize.R:8-15) iterated with ``w``
untouched, ``likelihood`` (:40-49) taken column by column, and ``factorize()``'s stopping test (:208) applied to every cell on
its own -- with W fixed nothing couples two cells.  The kernel (csrc/project.h) reads the matrix's compressed columns as they
are: no tiled layout is cut and no engine is created.  No CPU fallback: without the HIP library every call raises.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np

from . import _native as N
from .engine import EPS, CountMatrix

REASONS = {1: "converged", 3: "NaN likelihood", 4: "Itmax reached"}


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
