"""Helpers of the consensus tests: the reference's pair vector and the integer sums, from label matrices, in numpy."""
import numpy as np


def random_labels(R, m, r, seed, zero_at=None):
    """R runs of m labels in 1..r (int32)."""
    L = np.random.default_rng(seed).integers(1, r + 1, size=(R, m)).astype(np.int32)
    if zero_at is not None:
        L[zero_at] = 0
    return L


def pair_vector(L):
    """conav after len(L) runs (reference R/factorize.R:51-60, :218-219): per pair of cells (condensed order), the number
    of runs in which both carry the same label."""
    L = np.asarray(L)
    iu = np.triu_indices(L.shape[1], 1)
    return np.sum(L[:, iu[0]] == L[:, iu[1]], axis=0).astype(np.float64)


def pairs(c):
    c = np.asarray(c, dtype=np.int64)
    return int(np.sum(c * (c - 1) // 2))


def integer_sums(L, r):
    """(S1, S2) of the runs in L: S1 = sum_a pairs(counts of run a), S2 = sum_{a,b} pairs(contingency table of a, b)."""
    L = np.asarray(L, dtype=np.int64)
    q = r + 1
    s1 = sum(pairs(np.bincount(row, minlength=q)) for row in L)
    s2 = 0
    for a in range(L.shape[0]):
        for b in range(L.shape[0]):
            s2 += pairs(np.bincount(L[a] * q + L[b], minlength=q * q))
    return s1, s2


def groups_of(L):
    """Distinct label tuples of the cells, numbered by first cell: (tuples [G][R] uint8, sizes [G] int64)."""
    cols = np.ascontiguousarray(np.asarray(L).T)
    seen, tuples, sizes = {}, [], []
    for row in cols:
        k = row.tobytes()
        if k not in seen:
            seen[k] = len(sizes)
            tuples.append(row)
            sizes.append(0)
        sizes[seen[k]] += 1
    return np.array(tuples, dtype=np.uint8), np.array(sizes, dtype=np.int64)
