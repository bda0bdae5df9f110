"""Literal numpy restatement of the reference's cluster annotation: meta_genes (R/utils.R:605-641), meta_gene.cv
(R/utils2.R:136-178), write_meta (R/utils2.R:16-29) and gsea / overlap / assignCelltype's permutation loop (R/gsea.R:41-128).
Loops where R loops; nothing of the restatement shares code with ccfindr_amd/annotate.py or the library.

The GSEA part is the DENSE form: per (cluster, set) the rows are NA-filtered in (permuted) table order, both cumsums run over
all of them, and the score is the maximum of all their differences -- not the hit-position form the kernel uses.  R's NA is NaN
here and ``max`` propagates it as R's does.

Below the restatement: the input builders of the device tests (tests/test_gpu_annot.py, tests/test_gpu_annot_grid.py) and of
their companion without a device (tests/test_annot_grid_cpu.py), which checks on the same inputs that they are what the device
tests say they are.  ``compare`` is the one place that calls the library.
"""
import functools
import sys
import time

import numpy as np

import ccfindr_amd as C
from ccfindr_amd import annotate as A

U = sys.modules[__name__]                             # (compare() below reads as it did in tests/test_gpu_annot.py)


def order_decreasing(x):
    """order(x, decreasing=TRUE): stable, NaN last; 0-based."""
    x = list(x)
    idx = [i for i in range(len(x)) if not np.isnan(x[i])]
    idx.sort(key=lambda i: -x[i])                     # list.sort is stable
    return np.array(idx + [i for i in range(len(x)) if np.isnan(x[i])], dtype=np.int64)


def normalise(w, subtract_mean, log):
    w = np.array(w, dtype=np.float64)
    if subtract_mean:
        with np.errstate(divide="ignore", invalid="ignore"):
            if log:
                w = np.log10(w)
            w = w - np.mean(w, axis=1)[:, None]
            if log:
                w = 10.0 ** w
    return w


def meta_genes(w, max_per_cluster=10, gene_names=None, subtract_mean=True, log=True, normalised=False):
    """R/utils.R:605-641 on a basis matrix w (``normalised``: the basis.matrix branch, which does not normalise)."""
    w = np.array(w, dtype=np.float64) if normalised else normalise(w, subtract_mean, log)
    n, r = w.shape
    names = [str(i + 1) for i in range(n)] if gene_names is None else list(gene_names)
    nmax = int(min(max_per_cluster, n))
    select = []
    for k in range(r):
        idx = order_decreasing(w[:, k])
        itmp = []
        for i in range(n):
            x = w[idx[i]]
            ix = order_decreasing(x)
            if ix[0] != k:
                continue
            itmp.append(i)
        tmp = [names[idx[i]] for i in itmp]
        select.append(tmp[:nmax])
    return select


def meta_gene_cv(w, dw, max_per_cluster=100, gene_names=None, subtract_mean=True, log=True, cv_max=np.inf, normalised=False):
    """R/utils2.R:136-178; returns (gene, w, cv) of shape maxrow x r with '' / NaN padding."""
    w = np.array(w, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        cw = np.array(dw, dtype=np.float64) / w
    if not normalised:
        w = normalise(w, subtract_mean, log)
    n, r = w.shape
    names = [str(i + 1) for i in range(n)] if gene_names is None else list(gene_names)
    nmax = int(min(max_per_cluster, n))
    cols = []
    maxrow = 0
    for k in range(r):
        idx = order_decreasing(w[:, k])[:nmax]
        sig = [i for i in idx if cw[i, k] <= cv_max]
        cols.append(sig)
        maxrow = max(maxrow, len(sig))
    gene = [["" for _ in range(r)] for _ in range(maxrow)]
    wt = np.full((maxrow, r), np.nan)
    cv = np.full((maxrow, r), np.nan)
    for k, sig in enumerate(cols):
        for j, i in enumerate(sig):
            gene[j][k] = names[i]
            wt[j, k] = w[i, k]
            cv[j, k] = cw[i, k]
    return np.array(gene, dtype=str).reshape(maxrow, r), wt, cv


def write_meta_text(meta):
    """utils::write.csv of R/utils2.R:22-27 as text."""
    rank = len(meta)
    nmax = max([len(m) for m in meta] + [0])
    lines = ['"",' + ",".join('"%d"' % (k + 1) for k in range(rank))] if rank else ['""']
    for i in range(nmax):
        cells = ['"%d"' % (i + 1)]
        for m in meta:
            cells.append('"%s"' % (str(m[i]).replace('"', '""') if i < len(m) else ""))
        lines.append(",".join(cells))
    return "\n".join(lines) + "\n"


def overlap(query, glist, grp_prefix=("IG",)):
    """R/gsea.R:117-128 (%in% is numpy's isin)."""
    query = np.array([str(q) for q in query], dtype=str).reshape(-1)
    glist = [str(g) for g in glist]
    glist0 = [g for g in glist if g not in grp_prefix]                               # :119
    x = np.isin(query, np.array(glist0, dtype=str)) if glist0 else np.zeros(len(query), dtype=bool)   # :120
    grp = [g for g in grp_prefix if g in glist]                                      # :121
    for gr in grp:                                                                   # :122
        x1 = np.array([q[:len(gr)] == gr for q in query], dtype=bool)                # :124
        x = x | x1                                                                   # :125
    return x


def gsea_dense(glist, gwgt, wp, gset, grp_prefix=("IG",)):
    """R/gsea.R:79-115 on a table of N rows: glist N x r names, gwgt N x r weights (NaN = NA), wp N x r = gwgt^p as the caller
    formed it (so that the device and this statement raise to the power once, in the same place).  Returns ES nS x r."""
    N, r = gwgt.shape
    sets = list(gset.values()) if isinstance(gset, dict) else list(gset)
    ES = np.zeros((len(sets), r))
    for k in range(r):
        flag = ~np.isnan(gwgt[:, k])                          # :92
        gl = [str(g) for g in glist[flag, k]]                 # :93
        ph0 = wp[flag, k]                                     # :94, :100
        for s, gs in enumerate(sets):
            x = overlap(gl, gs, grp_prefix)                   # :95
            if x.sum() == 0:                                  # :96
                ES[s, k] = np.nan
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                ph = np.cumsum(x * ph0)                       # :101
                phit = ph / ph[-1]                            # :102
                y = ~np.isin(np.array(gl, dtype=str), np.array([str(g) for g in gs], dtype=str)) if len(gs) else np.ones(len(gl), dtype=bool)   # :104
                pm = np.cumsum(y.astype(np.int64))            # :105
                pmiss = pm.astype(np.float64) / float(pm[-1])  # :106
                d = phit - pmiss
            ES[s, k] = np.nan if np.isnan(d).any() else d.max()   # :108
    return ES


def assign_dense(glist, gwgt, wp, gset, perms, grp_prefix=("IG",)):
    """assignCelltype's loop (R/gsea.R:57-72) with given permutations (0-based rows).  Returns ES, exceed (the counts of :69
    before :74 divides; -1 where ES is NaN, where R's sum is NA) and the null scores nperm x nS x r."""
    ES = gsea_dense(glist, gwgt, wp, gset, grp_prefix)
    null = np.zeros((len(perms),) + ES.shape)
    for b, perm in enumerate(perms):
        null[b] = gsea_dense(glist[perm], gwgt[perm], wp[perm], gset, grp_prefix)
    with np.errstate(invalid="ignore"):
        exceed = (ES[None] < null).sum(axis=0).astype(np.int64) if len(perms) else np.zeros(ES.shape, dtype=np.int64)
    exceed[np.isnan(ES)] = -1
    return ES, exceed, null


def bits_equal(a, b):
    """Same shape, same bits where finite, NaN in the same places."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64)))


# ---- inputs of the device tests --------------------------------------------------------------------------------------------
def make_table(n, r, seed, na_clusters=(), all_prefixed=False):
    """A meta table of n rows: every cluster lists the same n genes in its own order, weights decreasing with ties.  The clusters
    in ``na_clusters`` end in NA rows (gene '', weight NaN), as a column shorter than the table does.  A tenth of the genes are
    named IG* (all of them with ``all_prefixed``)."""
    rng = np.random.default_rng(seed)
    names = np.array([("IG%d" % i) if (all_prefixed or i % 10 == 3) else ("g%d" % i) for i in range(n)])
    gene = np.empty((n, r), dtype=names.dtype)
    w = np.empty((n, r))
    for k in range(r):
        gene[:, k] = names[rng.permutation(n)]
        w[:, k] = np.sort(np.round(rng.gamma(0.8, 1.0, size=n), 1) + 0.1)[::-1]        # ties, and no zero
        if k in na_clusters and n > 1:
            cut = n - int(rng.integers(1, max(2, n // 3 + 1)))
            gene[cut:, k] = ""
            w[cut:, k] = np.nan
    return C.MetaTable(gene=gene.astype(str), w=w, cv=np.full((n, r), 0.1)), names


def make_sets(names, seed, sizes):
    rng = np.random.default_rng(seed)
    gset = {"none": ["absent1", "absent2"], "every": list(names)}
    for t in sizes:
        if 0 < t <= len(names):
            gset["size%d" % t] = list(rng.choice(names, size=t, replace=False))
    if len(names) >= 4:
        gset["prefix"] = ["IG", str(names[0]), str(names[1])]                            # IG* rows by prefix: hits AND misses
    return gset


def make_perms(n, nperm, seed):
    rng = np.random.default_rng(seed)
    perms = np.array([rng.permutation(n) for _ in range(nperm)], dtype=np.int32).reshape(nperm, n)
    perms[0] = np.arange(n)                                                              # the identity: exact ties meet the strict <
    if nperm > 2:
        perms[2] = perms[1]                                                              # and one permutation twice
    return perms


def compare(meta, gset, p, perms, label):
    out = C.assign_celltype(meta, meta.rank, gset, p=p, p_value=True, perms=perms, grp_prefix=("IG",), return_null=True)
    tb = A.gsea_tables(meta, gset, p=p, grp_prefix=("IG",))
    es, exceed, null = U.assign_dense(meta.gene, meta.w, tb["wp"].T, gset, perms, ("IG",))
    nan = int(np.isnan(es).sum())
    print(f"{label}: N={meta.gene.shape[0]} r={meta.rank} sets={len(gset)} p={p} nperm={len(perms)}: {nan} of {es.size} scores NaN, "
          f"largest set {int(np.diff(tb['hit_ptr']).max())} hits, exceed in [{exceed.min()}, {exceed.max()}]")
    assert U.bits_equal(out["ES"], es), (label, out["ES"], es)
    assert U.bits_equal(out["null_es"], null), label
    assert out["exceed"].dtype == np.int64 and np.array_equal(out["exceed"], exceed), (label, out["exceed"], exceed)
    with np.errstate(invalid="ignore"):
        want_p = np.where(np.isnan(es), np.nan, exceed / float(len(perms)))
    assert U.bits_equal(out["pvalue"], want_p)
    assert np.array_equal(null[0], es, equal_nan=True) and np.all(exceed[~np.isnan(es)] <= len(perms) - 1)
    # the observed scores alone: the same bits
    assert U.bits_equal(C.assign_celltype(meta, meta.rank, gset, p=p, grp_prefix=("IG",)), es)
    return out, es


# ---- inputs of tests/test_gpu_annot_grid.py: more items than workgroups, tables past 4096 and 16384 rows, nq past 256 ---------
GRID_PART = 2048                # workgroups of k_gsea_perm's grid on a 256-CU part (gsea.hip, gsea_grid: CUs x 2048 / 256)
LONG_SIZES = ((4200, 3), (16500, 2), (16440, 2))       # (N, r) of the tables with more than 64 validity words


def set_na(meta, k, start, stop):
    """Rows [start, stop) of cluster k become NA rows (gene '', weight NaN)."""
    meta.gene[start:stop, k] = ""
    meta.w[start:stop, k] = np.nan


def scan_shape(n):
    """-> (nW, per, first): the validity words of a table of n rows, the words a thread of k_gsea_perm's prefix scan owns, and the
    first position of the first word that thread 64 -- the first thread of wave 1 -- owns."""
    info = A.gsea_info()
    nw = -(-n // info["wave_width"])
    per = -(-nw // info["workgroup_size"])
    return nw, per, info["wave_width"] * per * info["wave_width"]


def launch_items(n, nperm, r):
    """Work items (b, k) of the largest launch of a call: the permutations of one chunk times the rank."""
    return min(A.gsea_info(n)["chunk_perms"], nperm) * r


def _long_table(n, r, seed):
    """A table of more than 4096 rows.  Cluster 0 has no NA rows.  The last cluster has a stretch of 400 NA rows from row 3000 on
    and 30 more at its end, so that in the observed table too every hit from row 3400 on has its rank from the scan, and the hits
    past `first` from a word that wave 1 owns.  At r = 3 cluster 1 is a column of 4000 genes: NA from there to the end.  The set
    `placed` names the genes that the last cluster holds at: row 63 and row first - 1 (the last position of a word), row `first`
    (the first position of the word that thread 64 owns), and the cluster's last valid row, n - 31, which is also the last valid
    position of the table's last word."""
    W = A.gsea_info()["wave_width"]
    meta, names = make_table(n, r, seed)
    first = scan_shape(n)[2]
    k = r - 1
    placed = [str(meta.gene[i, k]) for i in (W - 1, first - 1, first, n - 31)]
    set_na(meta, k, 3000, 3400)
    set_na(meta, k, n - 30, n)
    if r > 2:
        set_na(meta, 1, 4000, n)
    gset = make_sets(names, seed + 2, (1, W + 1, 300))
    del gset["every"]
    gset["placed"] = placed
    return dict(meta=meta, names=names, gset=gset, p=0.5, perms=make_perms(n, 6, seed + 6))


@functools.lru_cache(maxsize=None)
def _wide_perms(n):
    return make_perms(n, 1000, 257)                        # (80 MB: one array for both ranks)


def _wide_table(r):
    """N = 20 000 rows, the odd clusters ending in NA rows, 1000 seeded permutations."""
    W = A.gsea_info()["wave_width"]
    n = 20000
    meta, names = make_table(n, r, 251, na_clusters=tuple(range(1, r, 2)))
    gset = make_sets(names, 254, (1, W + 1, 300))          # (a seed whose single gene is no NA row of any of ten clusters)
    del gset["every"]
    return dict(meta=meta, names=names, gset=gset, p=0.5, perms=_wide_perms(n))


@functools.lru_cache(maxsize=None)
def grid_case(name):
    """-> dict meta, names, gset, p, perms, label: the inputs of one test of tests/test_gpu_annot_grid.py, built once a process.
    Nobody writes to them."""
    W = A.gsea_info()["wave_width"]
    if name == "default":
        # the default call's nperm = 1000 at rank 5: 5000 items.  Five sets: none, 1, W, W + 1 genes, the prefix set
        meta, names = make_table(130, 5, 211, na_clusters=(1, 3))
        gset = make_sets(names, 213, (1, W, W + 1))
        del gset["every"]
        c = dict(meta=meta, names=names, gset=gset, p=0.5, perms=make_perms(130, 1000, 217))
    elif name == "rank128":
        # 40 permutations x 128 clusters = 5120 items; 3 sets x 128 clusters = 384 scores: k_gsea_count's second workgroup
        # holds the prefix set's (make_sets lists `none` first)
        meta, names = make_table(33, 128, 221, na_clusters=tuple(range(3, 128, 4)))
        gset = make_sets(names, 223, (12,))
        del gset["every"]
        c = dict(meta=meta, names=names, gset=gset, p=1, perms=make_perms(33, 40, 227))
    elif name == "many_sets":
        # 300 sets of 1 .. 12 genes x 5 clusters = 1500 scores: six workgroups of k_gsea_count
        meta, names = make_table(40, 5, 231, na_clusters=(0, 3))
        rng = np.random.default_rng(233)
        gset = {"s%d" % s: list(rng.choice(names, size=1 + s % 12, replace=False)) for s in range(300)}
        c = dict(meta=meta, names=names, gset=gset, p=0.5, perms=make_perms(40, 8, 237))
    elif name.startswith("rows"):
        n = int(name[4:])
        c = _long_table(n, dict(LONG_SIZES)[n], 300 + n % 97)
    elif name == "chunk1":
        meta, names = make_table(257, 3, 241, na_clusters=(1,))
        c = dict(meta=meta, names=names, gset=make_sets(names, 243, (1, W, W + 1, 128)), p=1, perms=make_perms(257, 5, 247))
    elif name.startswith("wide"):
        c = _wide_table(int(name[4:]))
    else:
        raise KeyError(name)
    c["label"] = name
    for a in (c["meta"].gene, c["meta"].w, c["perms"]):
        a.setflags(write=False)
    return c


DENSE_CASES = ("default", "rank128", "many_sets") + tuple("rows%d" % n for n, _ in LONG_SIZES) + ("chunk1",)


@functools.lru_cache(maxsize=None)
def grid_dense(name):
    """The dense form on grid_case(name): dict tb (gsea_tables), es, exceed, null, seconds (of assign_dense alone)."""
    c = grid_case(name)
    tb = A.gsea_tables(c["meta"], c["gset"], p=c["p"], grp_prefix=("IG",))
    t0 = time.perf_counter()
    es, exceed, null = assign_dense(c["meta"].gene, c["meta"].w, tb["wp"].T, c["gset"], c["perms"], ("IG",))
    return dict(tb=tb, es=es, exceed=exceed, null=null, seconds=time.perf_counter() - t0)
