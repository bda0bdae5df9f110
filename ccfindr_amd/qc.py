"""Quality control between the file and the fit: mirror of the reference's ``filter_cells`` (R/utils.R:78-95),
``filter_genes`` (:134-194, with ``calc_vmr`` :197-218, ``has_mode`` :329-339 and ``rowVars`` :341-344) and
``normalize_count`` (:318-327), without the plots.

The gene side -- the reference's slow part -- is one launch over the genes' rows (``vbnmf_matrix_gene_stats``,
csrc/qc.h): per gene the number of expressing cells, the sum, the centred sum of squares and ``has_mode``.  The cell
totals are a host pass of the library (``vbnmf_matrix_col_sums``): one sequential sum per stored column.  No CPU fallback
for the gene statistics: without a device ``gene_stats`` raises ``VBNMFError`` (status 2); ``filter_genes(stats=...)``
takes a result computed earlier.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import _native as N
from .engine import CountMatrix
from .io import CountData, remove_zeros as _remove_zeros


@dataclass
class GeneStats:
    """Per-gene statistics of a genes x cells count matrix (``vbnmf_matrix_gene_stats``)."""
    ncexpr: np.ndarray            # cells expressing the gene (stored entries of its row), R/utils.R:139
    sum: np.ndarray               # sum_j x_ij
    ss: np.ndarray                # sum_j (x_ij - mean_i)^2 over all cells, centred form (:211-212, :343)
    mode: np.ndarray              # has_mode(row i), :329-339 (bool)
    ncells: int = 0               # m
    host_finished: int = 0        # rows the kernel left to the host's sort-and-count

    def mean(self):
        """``Matrix::rowMeans`` (R/utils.R:199)."""
        return self.sum / self.ncells

    def vmr(self, save_memory=False):
        """``calc_vmr`` (R/utils.R:197-218): variance over mean.  The reference's two paths differ in the variance's
        denominator and so do these: ``rowVars`` divides by m - 1 (:343), the ``save.memory`` loop by m (:209-212)."""
        denom = self.ncells if save_memory else self.ncells - 1
        with np.errstate(divide="ignore", invalid="ignore"):
            return (self.ss / denom) / self.mean()


def qc_info():
    """Constants of the kernel and the calling thread's last ``gene_stats`` split (``vbnmf_qc_info``): a dict with
    ``short_row_max``, ``pass_entries``, ``default_hist_bins``, ``grid_workgroups`` and ``times_ms`` (grouping by gene,
    upload, kernel, host finish)."""
    a = [ctypes.c_int32() for _ in range(4)]
    t = np.zeros(4)
    N.check(N.load().vbnmf_qc_info(*[ctypes.byref(v) for v in a], N.dptr(t)))
    return {"short_row_max": a[0].value, "pass_entries": a[1].value, "default_hist_bins": a[2].value,
            "grid_workgroups": a[3].value, "times_ms": t}


def _counts_of(x):
    return x.counts if isinstance(x, CountData) else x


def _check_finite(M):
    if M.meta()[3] != 0.0:                # every stored value is an integer (found at ingestion): nothing to look for
        return
    cp, ri, xv = N.c_int64_p(), N.c_int32_p(), N.c_double_p()
    N.check(M._lib.vbnmf_matrix_csc(M._h, ctypes.byref(cp), ctypes.byref(ri), ctypes.byref(xv)))
    if M.nnz and not np.isfinite(np.ctypeslib.as_array(xv, shape=(M.nnz,))).all():
        raise ValueError("the count matrix holds non-finite values")


def _col_sums(M):
    out = np.empty(M.shape[1])
    N.check(M._lib.vbnmf_matrix_col_sums(M._h, 0, M.shape[1], N.dptr(out)))
    return out


def gene_stats(mat, device=0, hist_bins=0):
    """Per-gene ``ncexpr``, ``sum``, ``ss`` and ``has_mode`` of ``mat`` (a ``CountData``, a ``CountMatrix``, a scipy
    matrix or an ndarray; genes x cells) on HIP device ``device``.  ``hist_bins``: rows whose values are all integers in
    ``[1, hist_bins)`` are decided by the kernel, the others finished on the host (0: the library's default)."""
    mat = _counts_of(mat)
    own = not isinstance(mat, CountMatrix)
    M = CountMatrix(mat) if own else mat
    try:
        if not M.is_shell:
            _check_finite(M)
        n, m = M.shape
        nnz = np.zeros(n, dtype=np.int64)
        s, ss = np.zeros(n), np.zeros(n)
        mode = np.zeros(n, dtype=np.int32)
        hf = ctypes.c_int64()
        N.check(M._lib.vbnmf_matrix_gene_stats(M._h, int(device), int(hist_bins), nnz.ctypes.data_as(N.c_int64_p), N.dptr(s),
                                               N.dptr(ss), mode.ctypes.data_as(N.c_int32_p), ctypes.byref(hf)))
    finally:
        if own:
            M.close()
    return GeneStats(ncexpr=nnz, sum=s, ss=ss, mode=mode.astype(bool), ncells=int(m), host_finished=int(hf.value))


def _as_count_data(x):
    if isinstance(x, CountData):
        return x
    import scipy.sparse as sp
    if isinstance(x, CountMatrix):
        return CountData(x.to_scipy())
    return CountData(x.tocsc() if sp.issparse(x) else sp.csc_matrix(np.asarray(x, dtype=np.float64)))


def _subset(x, rows=None, cols=None):
    X = x.counts.tocsc()
    genes, barcodes = x.genes, x.barcodes
    if rows is not None:
        idx = np.flatnonzero(rows)
        X = X[idx]
        genes = [genes[i] for i in idx] if genes else []
    if cols is not None:
        idx = np.flatnonzero(cols)
        X = X[:, idx]
        barcodes = [barcodes[j] for j in idx] if barcodes else []
    return CountData(X.tocsc(), genes, barcodes)


def filter_cells(x, umi_min=0, umi_max=np.inf, remove_zeros=True, verbose=True):
    """``filter_cells(object, umi.min, umi.max, remove.zeros)``; reference R/utils.R:78-95.  Cells with
    ``umi_min <= colSums <= umi_max`` are kept (:81-82), the counts and the barcodes subset (:93).  ``remove_zeros`` is kept for
    the signature only: the reference removes empty rows and columns whatever it says (:94), and so does this."""
    x = _as_count_data(x)
    M = CountMatrix(x.counts)
    try:
        _check_finite(M)
        umi = _col_sums(M)                                                          # :81
    finally:
        M.close()
    selected = (umi_min <= umi) & (umi <= umi_max)                                  # :82
    if verbose and (umi_min or umi_max < np.inf):                                   # :90
        print(f"{int(selected.sum())} cells out of {x.counts.shape[1]} selected")   # :91
    return _remove_zeros(_subset(x, cols=selected))                                 # :93-94


def filter_genes(x, markers=None, vmr_min=0, min_cells_expressed=0, max_cells_expressed=np.inf, rescue_genes=False,
                 save_memory=False, verbose=True, device=0, stats=None, return_info=False):
    """``filter_genes(object, markers, vmr.min, min.cells.expressed, max.cells.expressed, rescue.genes, save.memory)``;
    reference R/utils.R:134-194.

    A gene is kept if it is a marker (any column of its ``genes`` row is in ``markers``, :150-153), or variable
    (``vmr_min < vmr`` and ``min_cells_expressed <= ncexpr <= max_cells_expressed``, :159-161), or -- with ``rescue_genes``,
    and only if not every gene is variable -- not variable but with a mode in its count distribution (:162-173).
    ``save_memory`` picks the variance's denominator as the reference's two paths do (``GeneStats.vmr``).  ``stats``: a
    ``gene_stats`` result of ``x`` computed earlier (no device is used then); ``device``: where to compute it otherwise.
    The reference's three message lines print under its conditions (:180-187) unless ``verbose`` is false.
    ``return_info``: also return what ``plot_genes`` would have been given: ``vmr``, ``ncexpr`` and the logical vectors
    ``selected_genes``, ``variable_genes``, ``mode_genes`` (None without a rescue), ``marker_genes`` (None without markers),
    all over the genes with ``ncexpr > 0``, plus ``kept`` = their row numbers in ``x``.

    Deviation: genes no cell expresses are dropped FIRST, and everything after works on the reduced object.  The reference
    reduces only the counts it hands to ``calc_vmr`` (:142-143) and then indexes the unreduced object with the reduced
    selection (:168, :193): an index shift whenever empty genes exist.  Objects from ``read_10x`` or ``filter_cells`` never
    have empty genes, so the two agree wherever the reference is well defined.
    """
    x = _as_count_data(x)
    nrow = x.counts.shape[0]
    if stats is None:
        stats = gene_stats(x.counts, device=device)
    if len(stats.ncexpr) != nrow:
        raise ValueError(f"stats describes {len(stats.ncexpr)} genes but x has {nrow}")
    expressed = stats.ncexpr > 0                                                    # :142
    kept = np.flatnonzero(expressed)
    ncexpr = stats.ncexpr[kept]                                                     # :143
    ngenes = len(kept)                                                              # :144
    selected = np.zeros(ngenes, dtype=bool)                                         # :146
    marker_genes = None
    if markers is not None:                                                         # :148-154
        mk = set(markers)
        if x.genes:
            selected = np.array([any(c in mk for c in x.genes[i]) for i in kept], dtype=bool)
        marker_genes = selected.copy()
    vmr = stats.vmr(save_memory=save_memory)[kept]                                  # :156
    with np.errstate(invalid="ignore"):
        variable = (vmr_min < vmr) & (min_cells_expressed <= ncexpr) & (ncexpr <= max_cells_expressed)   # :159-161
    if rescue_genes and variable.sum() < ngenes:                                    # :162
        mode_genes = stats.mode[kept] & ~variable                                   # :167-169
        selected = selected | variable | mode_genes                                 # :173
    else:
        selected = selected | variable                                              # :176
        mode_genes = None
    if verbose:
        if markers is not None and marker_genes.sum() > 0:                          # :180-181
            print(f"{int(marker_genes.sum())} marker genes found")
        if vmr_min > 0 or min_cells_expressed > 0 or max_cells_expressed < np.inf:  # :182
            print(f"{int(variable.sum())} variable genes out of {nrow} ")           # :183 (cat() leaves the blank)
            if rescue_genes:
                print(f"{int((selected & ~variable).sum())} additional genes rescued")   # :184-185
            print(f"{int(selected.sum())} genes selected")                          # :186
    rows = np.zeros(nrow, dtype=bool)
    rows[kept[selected]] = True
    out = _subset(x, rows=rows)                                                     # :193
    if not return_info:
        return out
    return out, {"vmr": vmr, "ncexpr": ncexpr, "selected_genes": selected, "variable_genes": variable, "mode_genes": mode_genes,
                 "marker_genes": marker_genes, "kept": kept}


def normalize_count(x):
    """``normalize_count(object)``; reference R/utils.R:318-327: every stored value becomes ``(x / umi_j) * med``, in that
    order of operations (:322, :324), ``med`` the median of the cells' totals (:323).  Returns a ``CountData`` with float
    values; the annotation tables are kept."""
    x = _as_count_data(x)
    X = x.counts.tocsc().astype(np.float64)
    X.eliminate_zeros()
    M = CountMatrix(X)
    try:
        _check_finite(M)
        umi = _col_sums(M)                                                          # :321
    finally:
        M.close()
    col = np.repeat(np.arange(X.shape[1]), np.diff(X.indptr))
    med = np.median(umi)                                                            # :323
    import scipy.sparse as sp
    data = (X.data / umi[col]) * med                                                # :322, :324
    return CountData(sp.csc_matrix((data, X.indices.copy(), X.indptr.copy()), shape=X.shape), x.genes, x.barcodes)
