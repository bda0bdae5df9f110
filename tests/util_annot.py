"""Literal numpy restatement of the reference's cluster annotation: meta_genes (R/utils.R:605-641), meta_gene.cv
(R/utils2.R:136-178), write_meta (R/utils2.R:16-29) and gsea / overlap / assignCelltype's permutation loop (R/gsea.R:41-128).
Loops where R loops; nothing here shares code with ccfindr_amd/annotate.py or the library.

The GSEA part is the DENSE form: per (cluster, set) the rows are NA-filtered in (permuted) table order, both cumsums run over
all of them, and the score is the maximum of all their differences -- not the hit-position form the kernel uses.  R's NA is NaN
here and ``max`` propagates it as R's does.
"""
import numpy as np


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
