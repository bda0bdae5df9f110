"""ccfindr_amd/annotate.py on the host: meta_genes, meta_gene_cv, write_meta and the overlap flags against tests/util_annot.py
(the literal restatement of R/utils.R:605-641, R/utils2.R:16-29, :136-178, R/gsea.R:117-128) and against small tables worked
by hand; and the argument errors of assign_celltype / vbnmf_gsea_perm, all of which are raised before a device is looked for."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_annot as U  # noqa: E402

import ccfindr_amd as C  # noqa: E402
from ccfindr_amd import _native as NAT  # noqa: E402
from ccfindr_amd import annotate as A  # noqa: E402


def vb(w, dw):
    return SimpleNamespace(ranks=[w.shape[1]], basis=[w], dbasis=[dw])


def random_fit(n, r, seed):
    rng = np.random.default_rng(seed)
    w = rng.gamma(0.7, 1.0, size=(n, r)) + 1e-3
    dw = w * rng.uniform(0.05, 1.5, size=(n, r))
    return w, dw


# ---- meta_genes
def test_meta_genes_by_hand():
    # basis.matrix branch (no normalisation).  Cluster 1 is never any gene's largest entry; rows b and c tie in column 0.
    w = np.array([[5.0, 1.0, 0.0],      # a: largest in 0
                  [3.0, 0.5, 1.0],      # b: largest in 0 (ties with c in column 0: b first)
                  [3.0, 0.2, 4.0],      # c: largest in 2
                  [1.0, 0.9, 2.0],      # d: largest in 2
                  [2.0, 0.1, 2.0]])     # e: 0 and 2 tie: the first one, 0
    got = C.meta_genes(None, basis_matrix=w, gene_names=list("abcde"))
    assert got == [["a", "b", "e"], [], ["c", "d"]]
    assert C.meta_genes(None, basis_matrix=w, gene_names=list("abcde"), max_per_cluster=1) == [["a"], [], ["c"]]
    assert C.meta_genes(None, basis_matrix=w) == [["1", "2", "5"], [], ["3", "4"]]


@pytest.mark.parametrize("subtract_mean,log", [(True, True), (True, False), (False, True)])
def test_meta_genes_against_statement(subtract_mean, log):
    w, dw = random_fit(57, 4, 3)
    w[7] = w[9]                                    # whole rows tie
    w[11, 2] = w[12, 2]
    names = [f"G{i}" for i in range(57)]
    got = C.meta_genes(vb(w, dw), rank=4, gene_names=names, max_per_cluster=6, subtract_mean=subtract_mean, log=log)
    assert got == U.meta_genes(w, 6, names, subtract_mean, log)
    assert C.meta_genes(vb(w, dw), rank=4, basis_matrix=w, max_per_cluster=100) == U.meta_genes(w, 100, None, normalised=True)


# ---- meta_gene_cv
def test_meta_gene_cv_by_hand():
    w = np.array([[4.0, 1.0], [4.0, 3.0], [2.0, 8.0], [1.0, 2.0]])
    dw = w * np.array([[0.5, 1.0], [0.125, 0.125], [1.0, 0.125], [0.125, 2.0]])     # the cv, exact in binary
    t = C.meta_gene_cv(basis_matrix=w, dbasis=dw, gene_names=list("abcd"), max_per_cluster=3, cv_max=0.5)
    # column 0: order a, b (tie keeps rows), c -> cv .5, .125, 1 -> a, b;  column 1: c, b, d -> cv .125, .125, 2 -> c, b
    assert t.gene.tolist() == [["a", "c"], ["b", "b"]]
    assert t.w.tolist() == [[4.0, 8.0], [4.0, 3.0]]
    assert t.cv.tolist() == [[0.5, 0.125], [0.125, 0.125]]
    # packing: the rows passing cv_max move to the top, the shorter column is padded
    t = C.meta_gene_cv(basis_matrix=w, dbasis=dw, max_per_cluster=4, cv_max=0.2)
    assert t.gene.tolist() == [["2", "3"], ["4", "2"]]
    t = C.meta_gene_cv(basis_matrix=w, dbasis=dw, max_per_cluster=4, cv_max=0.75)
    assert t.gene.tolist() == [["1", "3"], ["2", "2"], ["4", ""]]
    assert np.isnan(t.w[2, 1]) and np.isnan(t.cv[2, 1]) and t.w[2, 0] == 1.0


@pytest.mark.parametrize("cv_max,mpc", [(np.inf, np.inf), (0.8, 20), (0.3, 100)])
def test_meta_gene_cv_against_statement(cv_max, mpc):
    w, dw = random_fit(83, 5, 11)
    w[20, 1] = w[30, 1] = w[40, 1]
    names = [f"G{i}" for i in range(83)]
    t = C.meta_gene_cv(vb(w, dw), rank=5, gene_names=names, max_per_cluster=mpc, cv_max=cv_max)
    g, wt, cv = U.meta_gene_cv(w, dw, mpc, names, cv_max=cv_max)
    assert t.gene.tolist() == g.tolist()
    assert U.bits_equal(t.w, wt) and U.bits_equal(t.cv, cv)
    # cv is taken before the normalisation; the basis.matrix branch does not normalise
    t2 = C.meta_gene_cv(basis_matrix=w, dbasis=dw, max_per_cluster=mpc, cv_max=cv_max)
    g2, wt2, cv2 = U.meta_gene_cv(w, dw, mpc, None, cv_max=cv_max, normalised=True)
    assert t2.gene.tolist() == g2.tolist() and U.bits_equal(t2.w, wt2) and U.bits_equal(t2.cv, cv2)
    if cv_max == np.inf:
        assert t.gene.shape == (83, 5) and not np.isnan(t.w).any()


def test_meta_gene_cv_errors():
    w, dw = random_fit(10, 2, 1)
    with pytest.raises(ValueError):
        C.meta_gene_cv(SimpleNamespace(ranks=[2], basis=[w]), rank=2)          # an ML fit: no dbasis
    with pytest.raises(ValueError):
        C.meta_gene_cv(vb(w, dw), rank=3)
    with pytest.raises(ValueError):
        C.meta_gene_cv(basis_matrix=w)
    with pytest.raises(ValueError):
        C.meta_gene_cv(vb(w, dw), rank=2, gene_names=["a"])


# ---- write_meta
def test_write_meta(tmp_path):
    meta = [["CD74", "IGHM"], [], ['A"B', "x,y", "z"]]
    f = tmp_path / "meta.csv"
    assert C.write_meta(meta, str(f)) is meta
    text = f.read_text()
    assert text == '"","1","2","3"\n"1","CD74","","A""B"\n"2","IGHM","","x,y"\n"3","","","z"\n'
    assert text == U.write_meta_text(meta)


# ---- overlap
def test_overlap_flags_by_hand():
    q = ["IGHM", "IG", "CD74", "HLA-A", "IGKC", "XIG", "LYZ"]
    # 'IG' in the set: a prefix, not a member.  IGHM / IGKC / IG match by prefix; only the gene literally named IG is no miss.
    x, y = A.overlap_flags(q, ["CD74", "IG", "HLA"], ("IG",))
    assert x.tolist() == [True, True, True, False, True, False, False]
    assert y.tolist() == [True, False, False, True, True, True, True]
    # both prefixes; 'KRT' is a prefix that the set does not hold
    x, y = A.overlap_flags(q, ["CD74", "IG", "HLA"], ("IG", "HLA", "KRT"))
    assert x.tolist() == [True, True, True, True, True, False, False]
    # the prefix is not in the set: IG genes are plain misses, and a set naming IGHM matches it exactly
    x, y = A.overlap_flags(q, ["IGHM", "LYZ"], ("IG",))
    assert x.tolist() == [True, False, False, False, False, False, True]
    assert y.tolist() == [False, True, True, True, True, True, False]
    x, y = A.overlap_flags(q, [], ("IG",))
    assert not x.any() and y.all()


def test_overlap_flags_against_statement():
    rng = np.random.default_rng(5)
    pool = ["IG", "IGH", "IGHM", "HLA", "HLA-B", "CD3", "CD3E", "KRT", "KRT8", "A", "B", "C", ""]
    for _ in range(200):
        q = list(rng.choice(pool, size=rng.integers(1, 12)))
        gs = list(rng.choice(pool, size=rng.integers(0, 6), replace=False))
        pf = tuple(rng.choice(["IG", "HLA", "KRT", "CD3"], size=rng.integers(0, 4), replace=False))
        x, y = A.overlap_flags(q, gs, pf)
        assert x.tolist() == U.overlap(q, gs, pf).tolist(), (q, gs, pf)
        assert y.tolist() == [g not in gs for g in q]


def test_gsea_tables_drop_na_rows():
    gene = np.array([["IGA", "b"], ["b", "IGA"], ["c", ""]])
    w = np.array([[3.0, 2.0], [2.0, 1.0], [1.0, np.nan]])
    meta = C.MetaTable(gene=gene, w=w, cv=w)
    tb = A.gsea_tables(meta, {"s0": ["b", "IG"], "s1": ["", "c"]}, p=1)
    assert tb["valid"].tolist() == [[1, 1, 1], [1, 1, 0]]
    assert tb["hit_ptr"].tolist() == [0, 2, 3, 5, 5]             # (k0,s0) IGA,b  (k0,s1) c  (k1,s0) b,IGA  (k1,s1): '' is an NA row
    assert tb["hit_row"].tolist() == [0, 1, 2, 0, 1]
    assert tb["hit_is_miss"].tolist() == [1, 0, 0, 0, 1]
    assert tb["wp"][0].tolist() == [3.0, 2.0, 1.0]


# ---- errors raised before any device is touched
def small_meta():
    gene = np.array([["a", "b"], ["b", "c"], ["c", "a"]])
    w = np.array([[3.0, 2.0], [2.0, 1.5], [1.0, 1.0]])
    return C.MetaTable(gene=gene, w=w, cv=w * 0.1)


def test_assign_celltype_argument_errors():
    m = small_meta()
    with pytest.raises(ValueError, match="Incorrect dimension"):
        C.assign_celltype(m, 3, {"s": ["a"]})
    with pytest.raises(ValueError, match="Incorrect input type"):
        C.assign_celltype([1, 2], 2, {"s": ["a"]})
    with pytest.raises(ValueError, match="perms"):
        C.assign_celltype(m, 2, {"s": ["a"]}, p_value=True, perms=np.zeros((2, 4), dtype=np.int32))
    with pytest.raises(ValueError):
        C.assign_celltype(m, 2, {"s": ["a"]}, p_value=True, nperm=-1)


def call(valid, wp, ptr, row, miss, ns, perms=None):
    return A.gsea_perm(valid, wp, ptr, row, miss, ns, perms=perms, device=0)


def test_library_checks_arguments_before_the_device():
    valid = np.ones((1, 4), dtype=np.uint8)
    wp = np.ones((1, 4))
    ok = dict(valid=valid, wp=wp, ptr=[0, 2], row=[1, 3], miss=[0, 0], ns=1)

    def bad(**kw):
        a = dict(ok, **kw)
        with pytest.raises(NAT.VBNMFError) as e:
            call(a["valid"], a["wp"], a["ptr"], a["row"], a["miss"], a["ns"], a.get("perms"))
        assert e.value.code == NAT.ERR_BAD_ARG, str(e.value)

    bad(row=[3, 1])                                   # not ascending
    bad(row=[1, 1])                                   # twice
    bad(row=[1, 4])                                   # outside
    bad(row=[-1, 2])
    bad(ptr=[1, 2], row=[1, 3])                       # does not start at 0
    v = valid.copy(); v[0, 3] = 0
    bad(valid=v)                                      # a hit on an NA row
    bad(perms=np.array([[0, 1, 2, 2]]))               # no permutation
    bad(perms=np.array([[0, 1, 2, 4]]))
    bad(perms=np.array([[0, 1, 2, 3], [3, 3, 3, 3]]))
    w2 = wp.copy(); w2[0, 0] = np.inf
    bad(wp=w2)                                        # a weight that is not finite
    # past the cap of one set (with M > 0)
    cap = A.gsea_info()["max_set_hits"]
    n = cap + 2
    bad(valid=np.ones((1, n), dtype=np.uint8), wp=np.ones((1, n)), ptr=[0, cap + 1], row=np.arange(cap + 1),
        miss=np.zeros(cap + 1, dtype=np.uint8))
    with pytest.raises(ValueError):
        call(valid, wp, [0, 2, 2], [1, 3], [0, 0], 1)
    with pytest.raises(ValueError):
        call(valid, wp, [0, 2], [1, 3], [0, 0], 1, perms=np.zeros((1, 5), dtype=np.int32))


def test_gsea_info_constants():
    i = A.gsea_info(4096)
    assert i["wave_width"] == 64 and i["workgroup_size"] % 64 == 0
    assert i["max_set_hits"] >= 4096
    assert i["chunk_perms"] >= 1
    assert A.gsea_info(1 << 30)["chunk_perms"] == 1


def test_gsea_tables_against_the_flags():
    """gsea_tables finds the hits through an index by name; the result is what overlap() and :104 give row by row."""
    rng = np.random.default_rng(17)
    pool = ["IG", "IGH", "IGHM", "HLA", "HLA-B", "CD3", "CD3E", "KRT", "KRT8", "A", "B", "C"]
    for trial in range(40):
        n, r = int(rng.integers(1, 30)), int(rng.integers(1, 4))
        gene = rng.choice(pool, size=(n, r)).astype(str)                      # names repeat within a column
        w = rng.uniform(0.1, 2.0, size=(n, r))
        for k in range(r):
            cut = n - int(rng.integers(0, n))
            w[cut:, k] = np.nan
            gene[cut:, k] = ""
        sets = [list(rng.choice(pool, size=rng.integers(0, 6), replace=False)) for _ in range(3)]
        pf = tuple(rng.choice(["IG", "HLA", "KRT"], size=rng.integers(0, 4), replace=False))
        tb = A.gsea_tables(C.MetaTable(gene=gene, w=w, cv=w), sets, p=0.5, grp_prefix=pf)
        q = 0
        for k in range(r):
            ok = ~np.isnan(w[:, k])
            for gs in sets:
                x = U.overlap(gene[:, k], gs, pf) & ok
                got = tb["hit_row"][tb["hit_ptr"][q]:tb["hit_ptr"][q + 1]]
                assert got.tolist() == np.flatnonzero(x).tolist(), (trial, k, gs, pf)
                assert tb["hit_is_miss"][tb["hit_ptr"][q]:tb["hit_ptr"][q + 1]].tolist() == [int(gene[i, k] not in gs) for i in got]
                q += 1
        assert U.bits_equal(tb["wp"], np.power(w.T, 0.5)) and tb["valid"].tolist() == (~np.isnan(w.T)).astype(int).tolist()


def test_no_cpu_fallback():
    """Without a device the scores are an error (status 2), after the arguments have been checked -- never a host computation."""
    if NAT.load().vbnmf_device_count() > 0:
        return                                                                     # (the device path: tests/test_gpu_annot.py)
    with pytest.raises(C.VBNMFError) as ei:
        C.assign_celltype(small_meta(), 2, {"s": ["a", "b"]})
    assert ei.value.code == NAT.ERR_NO_DEVICE and "no CPU fallback" in str(ei.value)
    with pytest.raises(C.VBNMFError) as ei:
        C.assign_celltype(small_meta(), 2, {"s": ["a", "b"]}, p_value=True, nperm=3, seed=1)
    assert ei.value.code == NAT.ERR_NO_DEVICE
