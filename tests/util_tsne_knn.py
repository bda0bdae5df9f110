"""The neighbour-limited t-SNE of csrc/tsne_knn.h restated in numpy fp64, line by line from DESIGN.md 5l, the same sums in
50-digit arithmetic (mpmath) for one row or one point, the bounds the GPU tests hold the kernels to, and the cases -- TEST
INFRASTRUCTURE ONLY.  Everything 5l leaves as in 5k (normalisation, D, the start, the schedule, the update, run's cost
bookkeeping) is taken from tests/util_tsne.py as it stands.

tests/test_tsne_knn_cpu.py ties the restatement to the 50-digit forms and checks the committed constants;
tests/test_gpu_tsne_knn.py holds the kernels to both.
"""
import functools
import math

import mpmath as mp
import numpy as np

import util_tsne as T

U, CAP, DBL_MIN, DBL_MAX, MAX_TRIPS, TOL, FLAG = T.U, T.CAP, T.DBL_MIN, T.DBL_MAX, T.MAX_TRIPS, T.TOL, T.FLAG


# ---- the restatement ------------------------------------------------------------------------------------------------------
def auto_k(u):
    return int(math.floor(3.0 * u))


def knn_lists(D, K):
    """N_i: the K indices j != i with the smallest (D_ij, j), in that order -> idx (n x K, int32), dist (n x K)."""
    n = len(D)
    j = np.arange(n)
    idx = np.zeros((n, K), dtype=np.int32)
    for i in range(n):
        order = np.lexsort((j, D[i]))
        idx[i] = order[order != i][:K]
    return idx, np.take_along_axis(D, idx.astype(np.int64), axis=1)


def affinities(dist, u):
    """util_tsne.bisection over the K listed distances of every row -> beta, S, trips, flagged."""
    def sums(rows, beta):
        p = np.exp(-beta[rows, None] * dist[rows])
        return p.sum(axis=1) + DBL_MIN, (dist[rows] * p).sum(axis=1)

    return T.bisection(len(dist), u, sums)


def cond_p(dist, beta, S):
    """p_{j|i} = exp(-beta_i D_ij) * (1 / S_i) over the lists."""
    return np.exp(-beta[:, None] * dist) * (1.0 / S)[:, None]


def sparse_p(idx, pc):
    """The pattern {(i, j): j in N_i or i in N_j} by rows with ascending j and (p_{j|i} + p_{i|j}) * 1/(2n)
    -> indptr (int64), indices (int32), values."""
    n, K = idx.shape
    r = np.repeat(np.arange(n, dtype=np.int64), K)
    c = idx.astype(np.int64).ravel()
    fwd, rev = r * n + c, c * n + r
    keys = np.unique(np.concatenate([fwd, rev]))
    pij, pji = np.zeros(len(keys)), np.zeros(len(keys))
    pij[np.searchsorted(keys, fwd)] = pc.ravel()
    pji[np.searchsorted(keys, rev)] = pc.ravel()
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(np.bincount(keys // n, minlength=n))
    return indptr, (keys % n).astype(np.int32), (pij + pji) * (1.0 / (2.0 * n))


def dense(indptr, indices, values):
    n = len(indptr) - 1
    P = np.zeros((n, n))
    P[np.repeat(np.arange(n), np.diff(indptr)), indices] = values
    return P


def forces(P, Y, e=1.0):
    """A over the stored row, R and z over all j, the cost over the entries with P_ij > 0: with P = dense(...) these are
    util_tsne.forces' sums (an entry that is not stored is 0 there and adds nothing)."""
    return T.forces(P, Y, e)


def run(P, Y, n_iter, **kw):
    return T.run(P, Y, n_iter, **kw)


# ---- 50 digits ---------------------------------------------------------------------------------------------------------------
_f = T._f


# Affinity sums over a list.  The terms are util_tsne's: p_j = exp(-beta D_ij) is off by 2u (exp) and by the exponent's
# (d + 3) beta D_ij u, relative.  The tree of k_tsne_knn: a thread adds the ceil(K / 256) terms q, q + 256, .. of the sorted
# list, then 6 butterfly levels, 3 additions of wave values and the DBL_MIN: depth = ceil(K / 256) + 6 + 3 + 1, each addition
# costing u of the (positive) partial sum.  K_S = 2 + depth + 1 (second-order terms): util_tsne.k_aff with K for n.
k_aff = T.k_aff


def mp_row(X, i, nbrs, beta, u):
    """Row i over its list at the given beta (a double) in 50 digits -> S, H, delta, bound_S (absolute)."""
    d = X.shape[1]
    xi = [_f(v) for v in X[i]]
    D = [mp.fsum((a - _f(b)) ** 2 for a, b in zip(xi, X[j])) for j in nbrs]
    b = _f(beta)
    p = [mp.exp(-b * Dj) for Dj in D]
    S = mp.fsum(p) + _f(DBL_MIN)
    H = b * mp.fsum(Dj * pj for Dj, pj in zip(D, p)) / S + mp.log(S)
    bound = mp.fsum((k_aff(len(D)) + (d + 3) * b * Dj) * U * pj for Dj, pj in zip(D, p))
    return S, H, H - mp.log(_f(u)), bound


# Force sums of point i, with X, beta, S, the lists and Y given as doubles.  The terms are util_tsne's:
#   P_ij = (p_{j|i} + p_{i|j}) / (2n) with a half that is not listed exactly 0:  dP_j = 7u P_ij + (d + 3) u D_ij (beta_i p_j|i +
#   beta_j p_i|j) / (2n);  w within 6u (the IEEE division);  an A term within dP / P + 9u, an R term 15u, a z term 6u.
#   Summation of A_i and the three cost sums (k_tsne_attract): lane l adds the entries l, l + 64, .. of the row, then 6
#   butterfly levels: depth_A = ceil(len_i / 64) + 6, where len_i is the row's length (K .. n - 1).
#   Summation of R_i and z_i (k_tsne_repulse): a wave adds its 256 terms of each of the ceil(n / 1024) tiles in a row, then two
#   additions join the four waves: depth_R = 256 ceil(n / 1024) + 2.
#   Each addition costs u of the sum of ABSOLUTE terms; the product with e adds u; one more u covers second-order terms.
#   Cost: as in util_tsne, with depth_A + 3 for the three sums and depth_R inside rZ (Z is the sum of the z_i).
# A stored value that ends among the subnormals (a far neighbour of a tight row: exp underflows gradually) is rounded there to
# a multiple of 2^-1074 whatever its size: the exponential (1 ulp), its product with 1 / S, the sum of the two halves' products
# and the product with 1 / (2n) add at most 2^-1074 each per half, 8 in all, on top of the relative terms.
SUBNORMAL = 8 * 2.0 ** -1074


def attract_depth(row_len):
    return -(-row_len // 64) + 6


def repulse_depth(n, tile=1024):
    return (tile // 4) * (-(-n // tile)) + 2


def masks(idx):
    n = len(idx)
    M = np.zeros((n, n), dtype=bool)
    M[np.repeat(np.arange(n), idx.shape[1]), idx.ravel()] = True
    return M


def mp_point(X, beta, S, idx, Y, i, e=1.0, Z=None):
    """Point i in 50 digits from the doubles X, beta, S, Y and the lists -> dict A (2), R (2), z, and cost if Z is given."""
    return T.mp_point(X, beta, S, Y, i, e, Z, idx)


def force_bounds(D, d, beta, S, idx, Y, e=1.0, tile=1024):
    """util_tsne.force_bounds with the depths above and SUBNORMAL -> absolute bounds A, R (n x 2), z, cost (n), the sums of
    absolute terms they are a share of, and the dense P the bounds were formed from."""
    M = masks(idx)
    depA = attract_depth((M | M.T).sum(1)).astype(np.float64)
    return T.force_bounds(D, d, beta, S, Y, e, M, depA, repulse_depth(len(D), tile), SUBNORMAL)


# A stored value against 50 digits (from the doubles beta and S): dP of the comment above, with SUBNORMAL.
# The sum of all of P.  In exact arithmetic sum_j p_{j|i} = (sum_j exp(-beta_i D_ij)) / S_i, which is 1 - DBL_MIN / S_i for the
# exact S_i; the device's S_i is off by K_S u + (d + 3) u beta_i sum_j D_ij p_{j|i} relative (k_aff and the exponent's term), and
# the mean over i of the second part is sum_ij (d + 3) u D_ij beta_i p_{j|i} / n: the second term of sum dP again.  So
# |sum P - 1| <= sum dP (the values) + (k_aff(K) u + sum dP) (the S_i) + DBL_MIN mean(1 / S) + u (fsum's one rounding).
def p_bounds(D, d, beta, S, idx):
    return T.p_bounds(D, d, beta, S, masks(idx), SUBNORMAL)


def sum_p_bound(dP, K, S):
    return 2.0 * dP.sum() + k_aff(K) * U + DBL_MIN * (1.0 / S).mean() + U


# ---- cases -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_lists(key, K, kw=()):
    """The restatement's lists and affinities of util_tsne.case(*key, **dict(kw)) with K neighbours (computed once)."""
    c = T.case(*key, **dict(kw))
    D = T.sq_dist(c["Xn"])
    idx, dist = knn_lists(D, K)
    out = {"D": D, "idx": idx, "dist": dist, "K": K}
    if c["u"] < K:
        beta, S, trips, flagged = affinities(dist, c["u"])
        out.update(beta=beta, S=S, trips=trips, flagged=flagged)
    return out


def handle_cases(i_block, j_tile, lds_row):
    """-> [(id, key, kw, K)], arguments of case_lists: every shape of util_tsne.shape_cases (the row past the LDS capacity
    included) and every util_tsne.SPECIAL input with K = floor(3u); K = n - 1 at n = 5, 65 and 257; K at the wave width, one
    above the workgroup size (a thread then adds two terms of the bisection's sums) and at the limit."""
    shapes, big = T.shape_cases(i_block, j_tile, lds_row)
    out = [("n%d-d%d" % c[:2], tuple(c), (), auto_k(T.perplexity_for(c[0]))) for c in shapes + [big]]
    for name, kw in T.SPECIAL.items():
        kw = dict(kw)
        key = (kw.pop("n"), kw.pop("d"))
        out.append((name, key, tuple(sorted(kw.items())), auto_k(T.perplexity_for(key[0]))))
    out += [("n5-K4", (5, 2, 4, 1), (), 4), ("n65-K64", (65, 10), (), 64), ("n257-K256", (257, 10), (), 256),
            ("n257-K64", (257, 33), (), 64), ("n1030-K257", (1030, 3), (), 257), ("n1030-K1024", (1030, 3), (), 1024)]
    return out


def k_edges(limit, workgroup, wave=64):
    """K one below, at and one above the wave width, the workgroup size (a thread's second term), every size of the sort
    (the powers of two up to the limit) from 128 on, and the limit with the one below it; for n = EDGE_N."""
    ks = {wave - 1, wave, wave + 1, workgroup - 1, workgroup, workgroup + 1, limit - 1, limit}
    p = 128
    while p < limit:
        ks |= {p - 1, p, p + 1}
        p *= 2
    return sorted(ks)


EDGE_CASE = (1030, 3)


def lattice(side=9):
    """side x side integer lattice in the plane: distances are small integers and tie in large groups."""
    g = np.arange(side, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)


LATTICE_K = (4, 5, 8, 9, 20)


def hub(n=257, d=64, seed=0):
    """Point 0 at the centre, the others on a sphere of radius 4 around it, in so many dimensions that two points of the sphere
    are farther from each other than from the centre: every point lists the hub first, and with K = 2 the hub's row of P has
    length n - 1 while the other rows have a handful of entries.  Points 1 and 2 sit a little inside the sphere (radius 3.6 and
    3.8): the hub's own two neighbours then differ by a tenth of their distance, and its bisection ends far from exp's
    underflow (with 256 equal distances of 16 it would need beta D of about 700).  Handed over with normalize=False."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n - 1, d))
    v /= np.linalg.norm(v, axis=1)[:, None]
    r = np.full(n - 1, 4.0)
    r[:2] = (3.6, 3.8)
    return np.vstack([np.zeros((1, d)), v * r[:, None]])


HUB = dict(n=257, d=64, K=2, u=1.5)


@functools.lru_cache(maxsize=None)
def hub_case():
    X = hub(HUB["n"], HUB["d"])
    D = T.sq_dist(X)
    idx, dist = knn_lists(D, HUB["K"])
    beta, S, trips, flagged = affinities(dist, HUB["u"])
    return {"X": X, "Xn": X, "u": HUB["u"], "n": HUB["n"], "d": HUB["d"], "normalize": False, "D": D, "idx": idx, "dist": dist, "K": HUB["K"],
            "beta": beta, "S": S, "trips": trips, "flagged": flagged}

# End to end: util_tsne.E2E (n = 300, d = 3, three clusters), perplexity 30, K = 90, the default schedule.  The restatement, on
# the CPU, from start(300, seed) for seed = 0 .. 4: every point's nearest neighbour in Y has its own cluster (300 of 300, all
# five seeds); the final costs are E2E_FINAL.
E2E_K = 90
E2E_FINAL = (0.29182967049827735, 0.2929884937872412, 0.27479244892655647, 0.27471104298210536, 0.28455907440822187)
E2E_NN_SAME = 300
