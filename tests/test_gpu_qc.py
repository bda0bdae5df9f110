"""k_gene_stats (csrc/qc.h) and the drivers on top of it (ccfindr_amd/qc.py) on the device, against tests/util_qc.py: the
line-by-line numpy restatement of the reference's quality-control step (R/utils.R:78-95, :134-194, :318-339) and the 50-digit
statement of a row's sum and centred sum of squares.  The row lengths and counts are aimed at the kernel's own boundaries
(vbnmf_qc_info): S = the longest row a wave takes alone, P = a long row's entries per pass, B = the default bin count of the
occurrence table, G = the persistent grid."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_qc as U  # noqa: E402

import ccfindr_amd as C  # noqa: E402
from ccfindr_amd import qc as Q  # noqa: E402
from ccfindr_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def info():
    i = Q.qc_info()
    assert i["grid_workgroups"] > 0
    return i


def check_rows(X, st, label):
    """nnz exactly; sum exactly for integer rows, else within SUM_BOUND sum|x|; ss within SS_BOUND (ss + 2 mu sum_j |x_ij - mu|),
    all against 50 digits.  Returns the largest two error figures seen."""
    m = X.shape[1]
    worst_s = worst_ss = 0.0
    for i, row in enumerate(X):
        v = row[row != 0]
        assert st.ncexpr[i] == len(v), (label, i)
        rs, rss = U.row_errors(v, m, st.sum[i], st.ss[i])
        print(f"{label} row {i} len {len(v)}: sum err {rs:.3e}  ss err {rss:.3e}")
        if np.all(v == np.floor(v)):
            assert rs == 0.0, (label, i, rs)
        assert rs <= U.SUM_BOUND, (label, i, rs)
        assert rss <= U.SS_BOUND, (label, i, rss)
        worst_s, worst_ss = max(worst_s, rs), max(worst_ss, rss)
    print(f"{label}: largest sum error {worst_s:.3e} (of sum|x|), largest ss error {worst_ss:.3e} (of ss + 2 mu sum|x - mu|)")
    return worst_s, worst_ss


# ---- (a) the constructed has_mode rows
@pytest.mark.parametrize("bins", [0, 8])
def test_constructed_rows(info, bins):
    B = bins or info["default_hist_bins"]
    X, want, tables = U.constructed_rows(B)
    st = Q.gene_stats(sp.csc_matrix(X), hist_bins=bins)
    assert [bool(v) for v in st.mode] == [bool(v) for v in want], list(zip(tables, st.mode, want))
    assert np.array_equal(want, [U.has_mode(r) for r in X])
    to_host = U.rows_for_host(X, B)
    assert to_host.sum() == (3 if B > 9 else 5)     # B, B + 1 and 2.5; with 8 bins also the two rows that hold a 9
    assert st.host_finished == int(to_host.sum())
    check_rows(X, st, f"constructed bins={B}")


def test_constructed_rows_small_table_sends_more_rows_to_the_host(info):
    # the rows written for the default table, run with 8 bins: 9, B - 1, B and B + 1 are all too large now
    X, want, _ = U.constructed_rows(info["default_hist_bins"])
    st = Q.gene_stats(sp.csc_matrix(X), hist_bins=8)
    to_host = U.rows_for_host(X, 8)
    assert to_host.sum() == 6 and st.host_finished == 6
    assert np.array_equal(st.mode, want)


def test_constructed_rows_as_long_rows(info):
    # the same occurrence tables in rows past the short class: every count times S + 1, among 300 (S + 1) cells, so that
    # the LDS table and the scan across the threads decide them
    S = info["short_row_max"]
    for B in (info["default_hist_bins"], 8):
        X0, want, tables = U.constructed_rows(B)
        rng = np.random.default_rng(4)
        X = np.stack([U.row_from_table({v: c * (S + 1) for v, c in t.items()}, 300 * (S + 1), rng) for t in tables])
        assert ((X != 0).sum(axis=1) > S).all()
        st = Q.gene_stats(sp.csc_matrix(X), hist_bins=B)
        assert np.array_equal(st.mode, want), list(zip(tables, st.mode, want))
        assert st.host_finished == (3 if B > 9 else 5)
        assert np.array_equal(st.ncexpr, (X != 0).sum(axis=1)) and np.array_equal(st.sum, X.sum(axis=1))


# ---- (b) row lengths around the class boundaries, against 50 digits
@pytest.mark.parametrize("kind", ["small", "large", "frac"])
def test_row_lengths(info, kind):
    S, P = info["short_row_max"], info["pass_entries"]
    X, lens = U.length_rows(S, P, kind)
    assert X.shape[1] == 2 * P + 1 and list((X != 0).sum(axis=1)) == lens
    st = Q.gene_stats(sp.csc_matrix(X))
    check_rows(X, st, f"lengths/{kind}")
    assert np.array_equal(st.mode, [U.has_mode(r) for r in X])
    assert st.host_finished == int(U.rows_for_host(X, info["default_hist_bins"]).sum())
    if kind == "frac":
        assert st.host_finished == len(lens)
    if kind == "small":
        assert st.host_finished == 0


def test_constant_gene_has_zero_ss(info):
    X = np.vstack([np.full((1, 300), 3.0), np.full((1, 300), 7.0)])
    X[1, :5] = 0.0
    st = Q.gene_stats(X)
    assert st.sum[0] == 900.0 and st.ss[0] == 0.0 and not st.mode[0]       # mu = 3 exactly: every centred term is 0
    check_rows(X, st, "constant")


# ---- (c) more genes than the grid
def test_more_genes_than_the_grid(info):
    G, P = info["grid_workgroups"], info["pass_entries"]
    rows_per_ticket = P // 64                      # a ticket is one row per wave (include/vbnmf.h: vbnmf_qc_info)
    for count in (3 * G + 1, 3 * G * rows_per_ticket + 1):              # ... more rows, and more tickets, than workgroups
        X = U.many_genes(count)
        st = Q.gene_stats(sp.csc_matrix(X))
        nnz, s, ss, mode = U.dense_stats(X)
        assert np.array_equal(st.ncexpr, nnz)
        assert np.array_equal(st.sum, s)                                # (integers)
        assert np.array_equal(st.mode, mode)
        mu = s / X.shape[1]
        bound = U.SS_BOUND * (ss + 2 * mu * np.abs(X - mu[:, None]).sum(axis=1))
        assert (np.abs(st.ss - ss) <= bound).all()
        assert st.host_finished == 0


# ---- (d) determinism
def test_two_runs_give_the_same_bits(info):
    X, _ = U.length_rows(info["short_row_max"], info["pass_entries"], "frac")
    Xs = sp.csc_matrix(X)
    a, b = Q.gene_stats(Xs), Q.gene_stats(Xs)
    for k in ("ncexpr", "sum", "ss", "mode"):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    assert a.host_finished == b.host_finished


# ---- (e) end to end on a random matrix
def test_end_to_end_random(info, capsys):
    A = synth.simulate_data(400, (60, 90, 150), seed=3, sparse=False)
    genes = [[f"ENSG{i:04d}", f"SYM{i}"] for i in range(A.shape[0])]
    x = C.CountData(sp.csc_matrix(A), genes, [[f"cell{j}"] for j in range(A.shape[1])])
    r0, c0, msg0 = U.filter_cells(A, umi_min=10 ** 2.6, umi_max=10 ** 3.7)
    xc = Q.filter_cells(x, umi_min=10 ** 2.6, umi_max=10 ** 3.7)
    assert capsys.readouterr().out == msg0
    Ac = A[np.ix_(r0, c0)]
    assert xc.counts.toarray().tobytes() == Ac.tobytes() and xc.rownames == [genes[i][0] for i in r0]
    gc = [genes[i] for i in r0]
    m = Ac.shape[1]
    # thresholds from the reference statement: vmr_min in the widest gap of the sorted vmr around the median
    vmr = U.calc_vmr(Ac)
    order = np.sort(vmr)
    lo, hi = len(order) // 3, 2 * len(order) // 3
    k = lo + int(np.argmax(np.diff(order[lo:hi])))
    vmr_min = float((order[k] + order[k + 1]) / 2)
    ncexpr = (Ac > 0).sum(axis=1)
    mce = int(np.sort(ncexpr)[len(ncexpr) // 4])
    # no gene's vmr lies within the device's error bound of vmr_min: vmr = ss / (m - 1) / mean, relative error <= that of ss
    # (SS_BOUND (ss + 2 mu sum_j |x - mu|) / ss) plus that of the sum (SUM_BOUND)
    mu = Ac.mean(axis=1)
    ss = ((Ac - mu[:, None]) ** 2).sum(axis=1)
    rel = U.SS_BOUND * (1 + 2 * mu * np.abs(Ac - mu[:, None]).sum(axis=1) / ss) + U.SUM_BOUND
    assert (np.abs(vmr - vmr_min) > 4 * rel * vmr).all()
    want = U.filter_genes(Ac, genes=gc, vmr_min=vmr_min, min_cells_expressed=mce, rescue_genes=True)
    assert want["variable_genes"].sum() >= 1                             # at least one variable gene,
    assert (want["selected_genes"] & ~want["variable_genes"]).sum() >= 1  # one rescued
    assert (~want["selected_genes"]).sum() >= 1                          # and one dropped: otherwise this shows nothing
    got, inf = Q.filter_genes(xc, vmr_min=vmr_min, min_cells_expressed=mce, rescue_genes=True, return_info=True)
    assert capsys.readouterr().out == want["messages"]
    for key in ("selected_genes", "variable_genes", "mode_genes"):
        assert np.array_equal(inf[key], want[key]), key
    assert np.array_equal(inf["ncexpr"], want["ncexpr"])
    assert (np.abs(inf["vmr"] - want["vmr"]) <= 4 * rel * vmr).all()
    assert got.counts.toarray().tobytes() == Ac[want["rows"]].tobytes()
    assert got.rownames == [gc[i][0] for i in want["rows"]] and got.barcodes == xc.barcodes
    # the other denominator, from the same scan
    st = Q.gene_stats(xc)
    got0 = Q.filter_genes(xc, vmr_min=vmr_min, min_cells_expressed=mce, rescue_genes=True, save_memory=True, stats=st, verbose=False)
    want0 = U.filter_genes(Ac, genes=gc, vmr_min=vmr_min, min_cells_expressed=mce, rescue_genes=True, save_memory=True)
    v0 = U.calc_vmr(Ac, save_memory=True)
    if (np.abs(v0 - vmr_min) > 4 * rel * v0).all():
        assert got0.rownames == [gc[i][0] for i in want0["rows"]]


# ---- (f) end to end on the shipped sample
def test_shipped_sample_modes(info):
    z = np.load(os.path.join(GOLD, "pbmc_extdata_r5.npz"))
    X = sp.csc_matrix((z["data"].astype(np.float64), z["indices"], z["indptr"]), shape=(int(z["n"]), int(z["m"])))
    A = X.toarray()
    want = np.array([U.has_mode(r) for r in A], dtype=bool)
    assert A.shape == (1030, 450) and want.sum() == 230
    ones, zeros = (A == 1).sum(axis=1), (A == 0).sum(axis=1)
    assert (zeros < ones).sum() == 100                                   # genes whose zeros are fewer than their ones
    assert A.max() == 113
    st = Q.gene_stats(X)
    assert np.array_equal(st.mode, want)
    assert st.host_finished == 0
    nnz, s, _, _ = U.dense_stats(A)
    assert np.array_equal(st.ncexpr, nnz) and np.array_equal(st.sum, s)
    vm = U.calc_vmr(A)
    assert np.allclose(st.vmr(), vm, rtol=1e-12)


def test_from_the_file_to_the_fit(info, tmp_path, capsys):
    # the README's path: read_10x -> filter_cells -> filter_genes -> vb_factorize, on a write_10x copy of the shipped sample
    z = np.load(os.path.join(GOLD, "pbmc_extdata_r5.npz"))
    X = sp.csc_matrix((z["data"].astype(np.float64), z["indices"], z["indptr"]), shape=(int(z["n"]), int(z["m"])))
    genes = [[f"ENSG{i:05d}", f"SYM{i}"] for i in range(X.shape[0])]
    C.write_10x(C.CountData(X, genes, [[f"BC{j}-1"] for j in range(X.shape[1])]), str(tmp_path))
    d = C.read_10x(str(tmp_path))
    A = d.counts.toarray()
    tot = A.sum(axis=0)
    lo, hi = float(np.quantile(tot, 0.1)), float(np.quantile(tot, 0.9))
    r0, c0, msg = U.filter_cells(A, lo, hi)
    d = C.filter_cells(d, umi_min=lo, umi_max=hi)
    assert capsys.readouterr().out == msg and 0 < len(c0) < A.shape[1]
    Ac = A[np.ix_(r0, c0)]
    gc = [d.genes[i] for i in range(len(d.genes))]
    assert d.counts.toarray().tobytes() == Ac.tobytes()
    want = U.filter_genes(Ac, genes=gc, markers=["SYM3"], vmr_min=1.5, min_cells_expressed=50, rescue_genes=True)
    assert np.abs(want["vmr"] - 1.5).min() > 1e-9                        # far outside the device's error bound
    d = C.filter_genes(d, markers=["SYM3"], vmr_min=1.5, min_cells_expressed=50, rescue_genes=True)
    assert capsys.readouterr().out == want["messages"]
    assert d.rownames == [gc[i][0] for i in want["rows"]] and 0 < len(want["rows"]) < Ac.shape[0]
    assert d.counts.toarray().tobytes() == Ac[want["rows"]].tobytes()
    vb = C.vb_factorize(d.count_matrix(), ranks=[2], nrun=1, Itmax=20, seed=1, verbose=0)
    assert vb.ranks == [2] and vb.basis[0].shape == (len(want["rows"]), 2) and np.isfinite(vb.measure["lml"][0])
