"""Cluster annotation after a fit: mirror of the reference's ``meta_genes`` (R/utils.R:605-641), ``meta_gene.cv``
(R/utils2.R:136-178), ``write_meta`` (R/utils2.R:16-29) and ``assignCelltype`` with ``gsea`` and ``overlap`` (R/gsea.R:41-128).

The tables are host work (a sort per cluster).  The enrichment scores -- the reference's slow part: ``gsea()`` once per
permutation, every cluster x every set x all rows (R/gsea.R:65-72) -- are the library's (``vbnmf_gsea_perm``, csrc/gsea.h): the
host forms the hit and miss flags once, the device sorts and walks the hits of every (permutation, cluster, set).  The scores
are those of the reference's dense ``cumsum`` bit for bit.  No CPU fallback: without a device ``assign_celltype`` raises
``VBNMFError`` (status 2).

Deviation: the permutations come from ``numpy.random.default_rng(seed)`` (or from ``perms=``), not from R's ``sample()`` stream.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import _native as N


@dataclass
class MetaTable:
    """``meta_gene.cv``'s data frame (R/utils2.R:160-175): per cluster k the columns Gene_k, W_k, CV_k, here three arrays of
    shape maxrow x r.  Rows past a cluster's last gene hold ``''`` and NaN (the reference's ``''`` and NA)."""
    gene: np.ndarray
    w: np.ndarray
    cv: np.ndarray

    @property
    def rank(self):
        return self.gene.shape[1]


def _order_decreasing(x):
    """R's ``order(x, decreasing=TRUE)``: ties keep their order, NaN last (0-based)."""
    return np.argsort(-np.asarray(x, dtype=np.float64), kind="stable")


def _basis_of(result, rank, what="basis"):
    ranks = [int(v) for v in result.ranks]
    if int(rank) not in ranks:
        raise ValueError(f"rank {rank} is not among the fitted ranks {ranks}")
    return np.array(getattr(result, what)[ranks.index(int(rank))], dtype=np.float64)


def _normalise(w, subtract_mean, log):
    if subtract_mean:
        with np.errstate(divide="ignore", invalid="ignore"):
            if log:
                w = np.log10(w)
            w = w - w.mean(axis=1, keepdims=True)
            if log:
                w = 10.0 ** w
    return w


def _row_names(n, gene_names):
    if gene_names is None:
        return np.array([str(i + 1) for i in range(n)], dtype=object)
    names = np.array([str(g) for g in gene_names], dtype=object)
    if len(names) != n:
        raise ValueError(f"gene_names has {len(names)} entries but the basis has {n} rows")
    return names


def meta_genes(result, rank=None, basis_matrix=None, max_per_cluster=10, gene_names=None, subtract_mean=True, log=True):
    """``meta_genes(object, rank, basis.matrix, max.per.cluster, gene_names, subtract.mean, log)``; reference
    R/utils.R:605-641.  Returns a list of r lists of gene names: per cluster the genes in decreasing order of their basis
    entry, kept only where that cluster is the gene's largest entry, ``max_per_cluster`` at the most."""
    if basis_matrix is None:                                                        # :609
        w = _basis_of(result, rank)                                                 # :610-611
        w = _normalise(w, subtract_mean, log)                                       # :612-616
    else:
        w = np.array(basis_matrix, dtype=np.float64)                                # :618
    r = w.shape[1]                                                                  # :619
    names = _row_names(w.shape[0], gene_names)                                      # :621
    nmax = int(min(max_per_cluster, w.shape[0]))                                    # :622
    select = []                                                                     # :623
    for k in range(r):                                                              # :624
        idx = _order_decreasing(w[:, k])                                            # :625
        v = w[idx]                                                                  # :626
        first = np.argsort(-v, axis=1, kind="stable")[:, 0] if len(v) else np.zeros(0, dtype=np.int64)   # :630, ix[1]
        itmp = np.flatnonzero(first == k)                                           # :631-634
        tmp = [names[i] for i in idx[itmp]]                                         # :636
        select.append(tmp[:nmax])                                                   # :637-638
    return select


def meta_gene_cv(result=None, rank=None, basis_matrix=None, dbasis=None, max_per_cluster=100, gene_names=None,
                 subtract_mean=True, log=True, cv_max=np.inf):
    """``meta_gene.cv(object, rank, basis.matrix, dbasis, max.per.cluster, gene_names, subtract.mean, log, cv.max)``;
    reference R/utils2.R:136-178.  Per cluster the ``max_per_cluster`` genes of largest basis entry (no "largest entry of its
    row" test here, unlike ``meta_genes``), of which those with ``cv <= cv_max`` are packed to the top.  ``cv`` is
    ``dbasis / w`` BEFORE the normalisation; with ``basis_matrix`` nothing is normalised."""
    if basis_matrix is None:                                                        # :141
        if result is None:
            raise ValueError("give a result, or basis_matrix with dbasis")
        if not hasattr(result, "dbasis"):
            raise ValueError("the result has no dbasis (an ML fit has no posterior width): give basis_matrix and dbasis")
        w = _basis_of(result, rank)                                                 # :142-143
        with np.errstate(divide="ignore", invalid="ignore"):
            cw = _basis_of(result, rank, "dbasis") / w                              # :144
        w = _normalise(w, subtract_mean, log)                                       # :145-149
    else:
        if dbasis is None:
            raise ValueError("basis_matrix needs dbasis")
        w = np.array(basis_matrix, dtype=np.float64)                                # :151
        with np.errstate(divide="ignore", invalid="ignore"):
            cw = np.asarray(dbasis, dtype=np.float64) / w                           # :153
        if cw.shape != w.shape:
            raise ValueError("basis_matrix and dbasis differ in shape")
    r = w.shape[1]                                                                  # :152
    names = _row_names(w.shape[0], gene_names)                                      # :155
    nmax = int(min(max_per_cluster, w.shape[0]))                                    # :156
    cols = []
    maxrow = 0                                                                      # :158
    for k in range(r):                                                              # :159
        idx = _order_decreasing(w[:, k])[:nmax]                                     # :163
        with np.errstate(invalid="ignore"):
            sig = idx[cw[idx, k] <= cv_max]                                         # :166 (NaN is dropped by which())
        cols.append(sig)
        maxrow = max(maxrow, len(sig))                                              # :171
    gene = np.full((maxrow, r), "", dtype=object)                                   # :160
    wt = np.full((maxrow, r), np.nan)
    cv = np.full((maxrow, r), np.nan)
    for k, sig in enumerate(cols):
        gene[:len(sig), k] = names[sig]                                             # :168
        wt[:len(sig), k] = w[sig, k]                                                # :169
        cv[:len(sig), k] = cw[sig, k]                                               # :170
    return MetaTable(gene=gene.astype(str) if gene.size else gene.astype("<U1"), w=wt, cv=cv)   # :175


def write_meta(meta, file):
    """``write_meta(meta, file)``; reference R/utils2.R:16-29: the lists of ``meta_genes`` side by side as ``write.csv`` lays
    them out -- every field quoted, a header of the cluster numbers behind an empty corner, the row numbers in front, ``''``
    below a shorter list.  Returns ``meta``."""
    rank = len(meta)                                                                # :18
    nmax = max([len(m) for m in meta], default=0)                                   # :19-21

    def q(s):
        return '"' + str(s).replace('"', '""') + '"'

    with open(file, "w", newline="") as fh:
        fh.write(",".join([q("")] + [q(k + 1) for k in range(rank)]) + "\n")        # :26
        for i in range(nmax):                                                       # :22-25
            fh.write(",".join([q(i + 1)] + [q(m[i]) if i < len(m) else q("") for m in meta]) + "\n")
    return meta                                                                     # :28


def overlap_flags(query, gs, grp_prefix=("IG",)):
    """``overlap(query, glist, grp.prefix)`` (R/gsea.R:117-128) and the miss flags of :104 for one gene set ``gs``: returns
    ``(x, y)``, boolean over ``query``.  A hit is an exact member of the set other than the prefixes (:119-120), or a name that
    starts with a prefix that is in the set (:121-126); a miss is a name not literally in the set (:104) -- so a gene matched
    through a prefix alone is both."""
    query = np.asarray(query, dtype=str)
    gs = [str(g) for g in gs]
    prefixes = [str(g) for g in grp_prefix]
    glist0 = [g for g in gs if g not in prefixes]                                   # :119
    x = np.isin(query, glist0) if len(glist0) else np.zeros(query.shape, dtype=bool)   # :120
    for gr in [g for g in prefixes if g in gs]:                                     # :121-122
        x = x | np.char.startswith(query, gr)                                       # :124-125
    y = ~np.isin(query, gs) if len(gs) else np.ones(query.shape, dtype=bool)        # :104
    return x, y


def gsea_tables(meta, gset, p=0, grp_prefix=("IG",)):
    """What ``vbnmf_gsea_perm`` takes, from a ``MetaTable`` and the gene sets: ``valid`` (r x N uint8, R/gsea.R:92), ``wp``
    (r x N, ``gw^p`` of :100), and the hits of every (cluster, set) in CSR form -- ``hit_ptr`` (r * nS + 1), ``hit_row``,
    ``hit_is_miss`` -- restricted to valid rows as :93 has it."""
    sets = [[str(g) for g in gs] for gs in (gset.values() if isinstance(gset, dict) else gset)]
    prefixes = [str(g) for g in grp_prefix]
    n, r = meta.gene.shape
    valid = np.ascontiguousarray(~np.isnan(meta.w.T))                               # :92
    with np.errstate(invalid="ignore", divide="ignore"):
        wp = np.ascontiguousarray(np.power(meta.w.T, float(p)))                     # :100
    hit_ptr = np.zeros(r * len(sets) + 1, dtype=np.int64)
    rows, miss = [], []
    for k in range(r):
        # overlap_flags per set would match all n names against every set; the same flags from an index of the cluster's valid
        # rows by name, and one startswith pass per prefix
        col = np.asarray(meta.gene[:, k])
        names = col.tolist() if col.dtype.kind == "U" else [str(g) for g in col]
        where = {}
        for i in np.flatnonzero(valid[k]).tolist():                                 # :93
            where.setdefault(names[i], []).append(i)
        by_prefix = {}
        for s, gs in enumerate(sets):
            members = set(gs)
            hit = set()
            for g in members.difference(prefixes):                                  # :119-120
                hit.update(where.get(g, ()))
            for gr in prefixes:
                if gr in members:                                                   # :121-126
                    if gr not in by_prefix:
                        by_prefix[gr] = np.flatnonzero(np.char.startswith(np.asarray(names, dtype=str), gr) & valid[k]) if n else []
                    hit.update(int(i) for i in by_prefix[gr])
            hit = np.array(sorted(hit), dtype=np.int32)
            rows.append(hit)
            miss.append(np.array([names[i] not in members for i in hit], dtype=np.uint8))      # :104
            hit_ptr[k * len(sets) + s + 1] = hit_ptr[k * len(sets) + s] + len(hit)
    hit_row = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int32)
    hit_is_miss = np.concatenate(miss) if miss else np.zeros(0, dtype=np.uint8)
    return {"valid": valid.astype(np.uint8), "wp": wp, "hit_ptr": hit_ptr, "hit_row": np.ascontiguousarray(hit_row, dtype=np.int32),
            "hit_is_miss": np.ascontiguousarray(hit_is_miss, dtype=np.uint8), "nsets": len(sets)}


def gsea_info(n=1):
    """Constants of the kernel and the calling thread's last ``gsea_perm`` split (``vbnmf_gsea_info``): a dict with
    ``wave_width``, ``workgroup_size``, ``max_set_hits`` (a cap: more hits in one (cluster, set) are refused),
    ``chunk_perms`` (permutations of one upload for a table of ``n`` rows; the environment variable
    ``VBNMF_GSEA_CHUNK_PERMS`` makes it smaller) and ``times_ms`` (upload, kernels, read-back, host checks and inversion)."""
    a = [ctypes.c_int32() for _ in range(3)]
    c = ctypes.c_int64()
    t = np.zeros(4)
    N.check(N.load().vbnmf_gsea_info(int(n), *[ctypes.byref(v) for v in a], ctypes.byref(c), N.dptr(t)))
    return {"wave_width": a[0].value, "workgroup_size": a[1].value, "max_set_hits": a[2].value, "chunk_perms": int(c.value),
            "times_ms": t}


def gsea_perm(valid, wp, hit_ptr, hit_row, hit_is_miss, nsets, perms=None, device=0, return_null=False):
    """``vbnmf_gsea_perm`` on arrays laid out as ``gsea_tables`` gives them.  Returns ``(es, exceed, null_es)``: ``es``
    nS x r (NaN for the reference's NA), ``exceed`` nS x r int64 (-1 where ``es`` is NaN), ``null_es`` nperm x nS x r or None."""
    valid = np.ascontiguousarray(valid, dtype=np.uint8)
    wp = np.ascontiguousarray(wp, dtype=np.float64)
    if valid.ndim != 2 or wp.shape != valid.shape:
        raise ValueError("valid and wp must both be r x N")
    r, n = valid.shape
    hit_ptr = np.ascontiguousarray(hit_ptr, dtype=np.int64)
    hit_row = np.ascontiguousarray(hit_row, dtype=np.int32)
    hit_is_miss = np.ascontiguousarray(hit_is_miss, dtype=np.uint8)
    nsets = int(nsets)
    if hit_ptr.shape != (r * nsets + 1,):
        raise ValueError(f"hit_ptr must have r * nS + 1 = {r * nsets + 1} entries")
    if len(hit_row) != len(hit_is_miss) or (len(hit_ptr) and hit_ptr[-1] != len(hit_row)):
        raise ValueError("hit_row, hit_is_miss and hit_ptr disagree on the number of hits")
    if perms is None:
        perms = np.zeros((0, n), dtype=np.int32)
    perms = np.ascontiguousarray(perms, dtype=np.int32)
    if perms.ndim != 2 or perms.shape[1] != n:
        raise ValueError(f"perms must be nperm x N = nperm x {n}")
    nperm = perms.shape[0]
    es = np.full((nsets, r), np.nan)
    exceed = np.full((nsets, r), -1, dtype=np.int64)
    null = np.full((nperm, nsets, r), np.nan) if return_null else None
    N.check(N.load().vbnmf_gsea_perm(int(device), n, r, nsets, valid.ctypes.data_as(N.c_uint8_p), N.dptr(wp),
                                     hit_ptr.ctypes.data_as(N.c_int64_p), hit_row.ctypes.data_as(N.c_int32_p),
                                     hit_is_miss.ctypes.data_as(N.c_uint8_p), nperm, perms.ctypes.data_as(N.c_int32_p),
                                     N.dptr(es), exceed.ctypes.data_as(N.c_int64_p), N.dptr(null)))
    return es, exceed, null


def assign_celltype(obj, rank, gset, gene_names=None, p=0, remove_na=False, p_value=False, nperm=1000, grp_prefix=("IG",),
                    seed=None, perms=None, device=0, return_null=False):
    """``assignCelltype(obj, rank, gset, gene_names, p, remove.na, p.value, nperm, grp.prefix)``; reference R/gsea.R:41-77.

    ``obj``: a ``VBResult`` (its table is ``meta_gene_cv(max_per_cluster=inf, cv_max=inf)``, :46-48) or a ``MetaTable``
    (:49-51).  ``gset``: a dict name -> genes, or a list of gene lists.  Returns ``ES`` (nS x r; NaN for the reference's NA:
    no gene of the set in the cluster's list, :96-99).  With ``p_value`` or ``return_null`` it returns a dict instead: ``ES``,
    ``pvalue`` (:74, the share of permutations whose score is strictly larger, :69; NaN where ES is), ``exceed`` (the counts),
    and with ``return_null`` ``null_es`` (nperm x nS x r).  ``remove_na`` drops the sets whose FIRST column is NaN (:112) from
    all of them.  ``perms``: nperm x N rows of 0-based permutations to use instead of ``default_rng(seed)``'s.
    """
    if isinstance(obj, MetaTable):                                                  # :49
        meta = obj
    elif hasattr(obj, "ranks") and hasattr(obj, "basis"):                           # :45
        meta = meta_gene_cv(obj, rank=rank, max_per_cluster=np.inf, gene_names=gene_names, subtract_mean=True, log=True,
                            cv_max=np.inf)                                          # :46-48
    else:
        raise ValueError("Incorrect input type of obj")                             # :52
    if meta.rank != int(rank):
        raise ValueError("Incorrect dimension of meta")                             # :51
    n = meta.gene.shape[0]                                                          # :61
    want_perms = bool(p_value or return_null)
    if want_perms:
        if perms is not None:
            perms = np.asarray(perms)
            if perms.ndim != 2 or perms.shape[1] != n:
                raise ValueError(f"perms must be nperm x N = nperm x {n}")
            perms = np.ascontiguousarray(perms, dtype=np.int32)
        else:
            if int(nperm) < 0:
                raise ValueError("nperm must not be negative")
            rng = np.random.default_rng(seed)
            perms = np.empty((int(nperm), n), dtype=np.int32)
            for b in range(int(nperm)):                                             # :66
                perms[b] = rng.permutation(n)
    else:
        perms = None
    if n == 0:
        raise ValueError("the meta table has no rows")
    tb = gsea_tables(meta, gset, p=p, grp_prefix=grp_prefix)
    es, exceed, null = gsea_perm(tb["valid"], tb["wp"], tb["hit_ptr"], tb["hit_row"], tb["hit_is_miss"], tb["nsets"],
                                 perms=perms, device=device, return_null=return_null)     # :57, :65-72
    keep = ~np.isnan(es[:, 0]) if remove_na else np.ones(es.shape[0], dtype=bool)   # :112
    es = es[keep]
    if not want_perms:                                                              # :60
        return es
    out = {"ES": es, "exceed": exceed[keep]}
    if p_value:
        nb = perms.shape[0]
        with np.errstate(invalid="ignore", divide="ignore"):
            out["pvalue"] = np.where(np.isnan(es), np.nan, exceed[keep] / float(nb))     # :74
    if return_null:
        out["null_es"] = null[:, keep]
    return out
