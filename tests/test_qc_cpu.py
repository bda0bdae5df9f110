"""The quality-control step's host side (ccfindr_amd/qc.py; reference R/utils.R:78-95, :134-194, :318-339) against the
line-by-line numpy restatement of tests/util_qc.py: the host finisher of has_mode, the cell totals, normalize_count,
filter_cells, and filter_genes' selection logic driven with injected statistics.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_qc as U  # noqa: E402

import ccfindr_amd as C  # noqa: E402
from ccfindr_amd import _native as N  # noqa: E402
from ccfindr_amd import qc as Q  # noqa: E402


def host_mode(row):
    """vbnmf_test_gene_mode_host on a dense row: its stored (non-zero) values among len(row) cells."""
    v = np.ascontiguousarray(row[row != 0], dtype=np.float64)
    out = ctypes.c_int32(-1)
    N.check(N.load().vbnmf_test_gene_mode_host(len(row), len(v), N.dptr(v), ctypes.byref(out)))
    return bool(out.value)


def test_host_finisher_on_the_constructed_rows():
    for B in (8, 4096):
        X, want, tables = U.constructed_rows(B)
        for row, w, t in zip(X, want, tables):
            assert U.has_mode(row) == w, t              # (the table of the issue is what the restatement gives)
            assert host_mode(row) == w, t


def test_host_finisher_on_random_rows():
    rng = np.random.default_rng(2024)
    seen = set()
    for k in range(200):
        m = int(rng.integers(1, 60))
        kind = k % 4
        if kind == 0:
            row = rng.poisson(rng.uniform(0.1, 3.0), size=m).astype(np.float64)
        elif kind == 1:
            row = rng.integers(0, 3, size=m).astype(np.float64)
        elif kind == 2:
            row = np.round(rng.normal(0.0, 1.5, size=m))              # negative values: levels below the zeros'
        else:
            row = rng.choice([0.0, 0.5, 1.0, 2.5, -1.5], size=m)
        want = U.has_mode(row)
        assert host_mode(row) == want, (k, row)
        seen.add(want)
    assert seen == {True, False}


def test_host_finisher_rejects_an_impossible_row():
    out = ctypes.c_int32()
    v = np.ones(3)
    assert N.load().vbnmf_test_gene_mode_host(2, 3, N.dptr(v), ctypes.byref(out)) == N.ERR_BAD_ARG


def sequential_col_sums(X):
    X = sp.csc_matrix(X)
    X.sort_indices()
    out = np.zeros(X.shape[1])
    for j in range(X.shape[1]):
        s = 0.0
        for q in range(X.indptr[j], X.indptr[j + 1]):
            s += float(X.data[q])
        out[j] = s
    return out


@pytest.mark.parametrize("kind", ["int", "frac"])
def test_col_sums_are_the_sequential_sums(kind):
    rng = np.random.default_rng(3)
    A = rng.poisson(0.8, size=(70, 45)).astype(np.float64)
    if kind == "frac":
        A = A * rng.gamma(0.5, 2.0, size=A.shape) * 10.0 ** rng.integers(-8, 8, size=A.shape)
    A[:, 7] = 0.0                                                      # an empty column sums to 0
    M = C.CountMatrix(sp.csc_matrix(A))
    got = Q._col_sums(M)
    want = sequential_col_sums(A)
    assert got.tobytes() == want.tobytes()
    part = np.empty(10)
    N.check(N.load().vbnmf_matrix_col_sums(M._h, 5, 15, N.dptr(part)))
    assert part.tobytes() == want[5:15].tobytes()
    assert N.load().vbnmf_matrix_col_sums(M._h, 5, 46, N.dptr(part)) == N.ERR_BAD_ARG
    M.close()


def test_col_sums_of_a_shell_is_a_state_error():
    M = C.CountMatrix(np.ones((3, 4)))
    S = C.CountMatrix.shell(M.meta())
    out = np.empty(4)
    assert N.load().vbnmf_matrix_col_sums(S._h, 0, 4, N.dptr(out)) == N.ERR_STATE
    M.close(); S.close()


def test_normalize_count_bit_for_bit():
    rng = np.random.default_rng(1)
    A = rng.poisson(3.0, size=(40, 30)).astype(np.float64)             # the reference's example (:313)
    x = C.CountData(sp.csc_matrix(A), [[f"g{i}"] for i in range(40)], [[f"c{j}"] for j in range(30)])
    got = Q.normalize_count(x)
    want = U.normalize_count(A)
    assert got.counts.toarray().tobytes() == want.tobytes()
    assert got.genes == x.genes and got.barcodes == x.barcodes
    assert got.counts.dtype == np.float64
    # every cell now holds the median total, up to rounding (:300-306)
    assert np.allclose(np.asarray(got.counts.sum(axis=0)).ravel(), np.median(A.sum(axis=0)), rtol=1e-13)


def test_filter_cells_reference_example(capsys):
    rng = np.random.default_rng(1)
    A = rng.poisson(3.0, size=(40, 30)).astype(np.float64)             # rpois(n = 1200, lambda = 3), 40 x 30 (:75)
    A[5, :] = 0.0
    x = C.CountData(sp.csc_matrix(A), [[f"g{i}", f"sym{i}"] for i in range(40)], [[f"c{j}"] for j in range(30)])
    got = Q.filter_cells(x, umi_min=10 ** 2.0, umi_max=10 ** 2.1)      # (:76)
    rows, cols, msg = U.filter_cells(A, 10 ** 2.0, 10 ** 2.1)
    assert 0 < len(cols) < 30 and 5 not in rows
    assert capsys.readouterr().out == msg
    assert got.counts.toarray().tobytes() == A[np.ix_(rows, cols)].tobytes()
    assert got.rownames == [f"g{i}" for i in rows] and got.colnames == [f"c{j}" for j in cols]
    # no limit given: no line (:90); verbose=False: none either
    Q.filter_cells(x)
    Q.filter_cells(x, umi_min=100, verbose=False)
    assert capsys.readouterr().out == ""
    # remove_zeros is ignored, as in the reference (:94)
    got2 = Q.filter_cells(x, umi_min=10 ** 2.0, umi_max=10 ** 2.1, remove_zeros=False, verbose=False)
    assert got2.counts.shape == got.counts.shape


def stats_of(A):
    """The statistics a device would return, from numpy: what filter_genes(stats=...) takes."""
    nnz, s, ss, mode = U.dense_stats(A)
    return Q.GeneStats(ncexpr=nnz.astype(np.int64), sum=s, ss=ss, mode=mode, ncells=A.shape[1], host_finished=0)


@pytest.fixture(scope="module")
def genes_case():
    rng = np.random.default_rng(8)
    lam = rng.gamma(0.4, 1.5, size=(60, 1))
    A = rng.poisson(lam * rng.gamma(2.0, 0.5, size=(1, 50))).astype(np.float64)
    A[10] = 0.0
    A[10, :30] = 1.0                                                   # a gene with a mode that is not variable: vmr < 1
    A = A[A.sum(axis=1) > 0]
    genes = [[f"ENSG{i:03d}", f"SYM{i}"] for i in range(A.shape[0])]
    x = C.CountData(sp.csc_matrix(A), genes, [[f"c{j}"] for j in range(A.shape[1])])
    return A, genes, x, stats_of(A)


def check_against_statement(x, A, genes, st, capsys, **kw):
    got, info = Q.filter_genes(x, stats=st, return_info=True, **kw)
    out = capsys.readouterr().out
    want = U.filter_genes(A, genes=genes, **kw)
    assert out == want["messages"]
    assert np.array_equal(info["kept"][info["selected_genes"]], want["rows"])
    for k in ("selected_genes", "variable_genes", "mode_genes", "marker_genes"):
        if want[k] is None:
            assert info[k] is None, k
        else:
            assert np.array_equal(info[k], want[k]), k
    assert np.array_equal(info["ncexpr"], want["ncexpr"])
    assert np.allclose(info["vmr"], want["vmr"], rtol=1e-12, equal_nan=True)
    assert got.counts.toarray().tobytes() == A[want["rows"]].tobytes()
    assert got.rownames == [genes[i][0] for i in want["rows"]]
    assert got.barcodes == x.barcodes
    return want


def test_filter_genes_thresholds_one_at_a_time_and_together(genes_case, capsys):
    A, genes, x, st = genes_case
    vm = np.sort(U.calc_vmr(A))
    vmin = float((vm[len(vm) // 2] + vm[len(vm) // 2 + 1]) / 2)
    seen = []
    for kw in ({"vmr_min": vmin}, {"min_cells_expressed": 10}, {"max_cells_expressed": 25},
               {"vmr_min": vmin, "min_cells_expressed": 10, "max_cells_expressed": 25}, {}):
        w = check_against_statement(x, A, genes, st, capsys, **kw)
        seen.append(len(w["rows"]))
    assert 0 < seen[3] < min(seen[:3]) and seen[4] == A.shape[0]       # (vmr_min = 0 with no limit keeps every gene: vmr > 0)


def test_filter_genes_rescue_on_off_and_skipped(genes_case, capsys):
    A, genes, x, st = genes_case
    vm = np.sort(U.calc_vmr(A))
    vmin = float((vm[len(vm) // 2] + vm[len(vm) // 2 + 1]) / 2)
    on = check_against_statement(x, A, genes, st, capsys, vmr_min=vmin, min_cells_expressed=5, rescue_genes=True)
    off = check_against_statement(x, A, genes, st, capsys, vmr_min=vmin, min_cells_expressed=5, rescue_genes=False)
    assert on["mode_genes"].sum() > 0 and len(on["rows"]) > len(off["rows"]) and len(on["rows"]) < A.shape[0]
    # every gene variable: the scan is skipped (:162) and mode_genes is NULL (:177), but the rescue line still prints (:184)
    skipped = check_against_statement(x, A, genes, st, capsys, max_cells_expressed=1e9, rescue_genes=True)
    assert skipped["mode_genes"] is None and "0 additional genes rescued" in skipped["messages"]


def test_filter_genes_both_denominators(genes_case, capsys):
    A, genes, x, st = genes_case
    m = A.shape[1]
    v1, v0 = U.calc_vmr(A), U.calc_vmr(A, save_memory=True)
    assert np.allclose(v0 * m / (m - 1), v1, rtol=1e-12)
    # a threshold between the two values of one gene separates the two paths
    i = int(np.argmax(v1))
    vmin = float((v0[i] + v1[i]) / 2)
    a = check_against_statement(x, A, genes, st, capsys, vmr_min=vmin, save_memory=False)
    b = check_against_statement(x, A, genes, st, capsys, vmr_min=vmin, save_memory=True)
    assert i in a["rows"] and i not in b["rows"]


def test_filter_genes_markers_in_the_second_column(genes_case, capsys):
    A, genes, x, st = genes_case
    vm = U.calc_vmr(A)
    low = [int(i) for i in np.argsort(vm)[:3]]
    markers = [genes[low[0]][1], genes[low[1]][1], "NOT_A_GENE"]       # symbols: the second column of the table
    w = check_against_statement(x, A, genes, st, capsys, markers=markers, vmr_min=float(np.median(vm)))
    assert w["marker_genes"].sum() == 2 and low[0] in w["rows"] and low[1] in w["rows"] and low[2] not in w["rows"]
    assert w["messages"].startswith("2 marker genes found\n")
    # markers alone: only the marker line (:180-182)
    w = check_against_statement(x, A, genes, st, capsys, markers=markers)
    assert w["messages"] == "2 marker genes found\n"
    # no marker matches: no marker line
    w = check_against_statement(x, A, genes, st, capsys, markers=["NOT_A_GENE"], min_cells_expressed=3)
    assert "marker" not in w["messages"]
    Q.filter_genes(x, stats=st, markers=markers, vmr_min=1.0, verbose=False)
    assert capsys.readouterr().out == ""


def test_filter_genes_with_two_empty_genes(genes_case, capsys):
    A, genes, x, st = genes_case
    A2 = np.vstack([A[:4], np.zeros((1, A.shape[1])), A[4:20], np.zeros((1, A.shape[1])), A[20:]])
    genes2 = [[f"G{i}", f"S{i}"] for i in range(A2.shape[0])]
    x2 = C.CountData(sp.csc_matrix(A2), genes2, x.barcodes)
    vm = np.sort(U.calc_vmr(A))
    vmin = float((vm[len(vm) // 2] + vm[len(vm) // 2 + 1]) / 2)
    w = check_against_statement(x2, A2, genes2, stats_of(A2), capsys, vmr_min=vmin, min_cells_expressed=5, rescue_genes=True,
                                markers=["S4", "S6"])
    assert 4 not in w["rows"] and 21 not in w["rows"] and 6 in w["rows"]
    assert f"variable genes out of {A2.shape[0]} \n" in w["messages"]   # dim(object)[1]: the unreduced count (:183)
    with pytest.raises(ValueError):
        Q.filter_genes(x2, stats=stats_of(A))


def test_gene_stats_vmr_and_mean():
    A = np.array([[1.0, 0, 3, 0], [2, 2, 2, 2]])
    st = stats_of(A)
    assert np.array_equal(st.mean(), [1.0, 2.0])
    assert np.allclose(st.vmr(), U.calc_vmr(A)) and np.allclose(st.vmr(save_memory=True), U.calc_vmr(A, save_memory=True))


def test_gene_stats_arguments_and_no_device():
    M = C.CountMatrix(np.ones((4, 5)))
    L = N.load()
    n = 4
    nnz, s, ss, mode = np.zeros(n, dtype=np.int64), np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32)
    args = (nnz.ctypes.data_as(N.c_int64_p), N.dptr(s), N.dptr(ss), mode.ctypes.data_as(N.c_int32_p), None)
    assert L.vbnmf_matrix_gene_stats(M._h, 0, 1, *args) == N.ERR_BAD_ARG           # found before a device is looked for
    assert L.vbnmf_matrix_gene_stats(M._h, 0, 1 << 20, *args) == N.ERR_BAD_ARG     # more bins than LDS holds
    S = C.CountMatrix.shell(M.meta())
    assert L.vbnmf_matrix_gene_stats(S._h, 0, 0, *args) == N.ERR_STATE
    S.close()
    info = Q.qc_info()
    assert 0 < info["short_row_max"] < info["pass_entries"] and info["pass_entries"] % 64 == 0 and info["default_hist_bins"] >= 256
    with pytest.raises(ValueError):
        Q.gene_stats(np.array([[1.0, np.inf], [0.0, 2.0]]))
    if L.vbnmf_device_count() > 0:
        M.close()
        return                                                                     # (the device path: tests/test_gpu_qc.py)
    assert info["grid_workgroups"] == 0
    with pytest.raises(C.VBNMFError) as ei:
        Q.gene_stats(M)
    assert ei.value.code == 2 and "no CPU fallback" in str(ei.value)
    with pytest.raises(C.VBNMFError):
        Q.filter_genes(C.CountData(sp.csc_matrix(np.ones((4, 5)))), vmr_min=1.0)
    M.close()
