"""The exact t-SNE of csrc/tsne.h restated in numpy fp64, line by line from DESIGN.md 5k, the same sums in 50-digit arithmetic
(mpmath) for one row or one point, the bounds the GPU tests hold the kernels to, and the cases -- TEST INFRASTRUCTURE ONLY.

tests/test_tsne_cpu.py ties the restatement to the 50-digit forms and checks the committed seeds; tests/test_gpu_tsne.py holds
the kernels to both.  Rtsne is not involved: it cannot run here.
"""
import functools
import math

import mpmath as mp
import numpy as np

mp.mp.dps = 50

U = 2.0 ** -53                        # unit roundoff of a double
DBL_MAX = np.finfo(np.float64).max
DBL_MIN = np.finfo(np.float64).tiny
MAX_TRIPS = 200
TOL = 1e-5
FLAG = 1e-9                           # a trip with ||delta| - TOL| < FLAG or |delta| < FLAG flags its row
CAP = 1e-12                           # no derived bound may ask for more than this share of the sum of absolute terms
DEFAULTS = dict(eta=200.0, exaggeration=12.0, stop_lying_iter=250, mom_switch_iter=250, momentum=0.5, final_momentum=0.8,
                min_gain=0.01)


# ---- the restatement ------------------------------------------------------------------------------------------------------
def normalise(X):
    """Column means as a left-to-right sum over the points (cumsum is one), then the largest absolute value: the host's order."""
    X = np.array(X, dtype=np.float64)
    X = X - np.cumsum(X, axis=0)[-1] / len(X)
    mx = np.abs(X).max()
    return X / mx if mx > 0 else X


def sq_dist(X):
    """D_ij = sum_k (x_ik - x_jk)^2, added in the order k = 0 .. d-1."""
    n, d = X.shape
    D = np.zeros((n, n))
    for k in range(d):
        df = X[:, None, k] - X[None, :, k]
        D += df * df
    return D


def bisection(n, u, sums):
    """The bisection of every row -> beta, S, trips, flagged (rows where another summation order may branch otherwise);
    sums(rows, beta) -> S and sum D exp(-beta D) of those rows.  A row that uses up its trips keeps the beta of the last update
    and S is evaluated once more at it."""
    beta, lo, hi = np.ones(n), np.full(n, -DBL_MAX), np.full(n, DBL_MAX)
    S, trips, flagged = np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=bool)
    act = np.arange(n)
    lnu = math.log(u)
    for _ in range(MAX_TRIPS):
        if not len(act):
            break
        s, sdp = sums(act, beta)
        H = beta[act] * sdp / s + np.log(s)
        delta = H - lnu
        S[act] = s
        trips[act] += 1
        flagged[act] |= (np.abs(np.abs(delta) - TOL) < FLAG) | (np.abs(delta) < FLAG)
        conv = np.abs(delta) < TOL
        up = ~conv & (delta > 0)
        dn = ~conv & ~(delta > 0)
        r = act[up]
        lo[r] = beta[r]
        beta[r] = np.where(hi[r] == DBL_MAX, beta[r] * 2.0, (beta[r] + hi[r]) / 2.0)
        r = act[dn]
        hi[r] = beta[r]
        beta[r] = np.where(lo[r] == -DBL_MAX, beta[r] / 2.0, (beta[r] + lo[r]) / 2.0)
        act = act[~conv]
    if len(act):
        S[act] = sums(act, beta)[0]
    return beta, S, trips, flagged


def affinities(X, u, D=None):
    """The bisection over all j != i of every row (the entry i is zeroed, not left out: numpy's sum then rounds as it does)."""
    D = sq_dist(X) if D is None else D

    def sums(rows, beta):
        p = np.exp(-beta[rows, None] * D[rows])
        p[np.arange(len(rows)), rows] = 0.0
        return p.sum(axis=1) + DBL_MIN, (D[rows] * p).sum(axis=1)

    return bisection(len(D), u, sums)


def joint_p(D, beta, S):
    n = len(D)
    pc = np.exp(-beta[:, None] * D) / S[:, None]
    np.fill_diagonal(pc, 0.0)
    return (pc + pc.T) / (2.0 * n)


def forces(P, Y, e=1.0):
    """-> A (times e), R, z, cost_i of DESIGN.md 5k on Y."""
    dy = Y[:, None, :] - Y[None, :, :]
    w = 1.0 / (1.0 + dy[:, :, 0] * dy[:, :, 0] + dy[:, :, 1] * dy[:, :, 1])
    np.fill_diagonal(w, 0.0)
    z = w.sum(axis=1)
    A = e * ((P * w)[:, :, None] * dy).sum(axis=1)
    R = ((w * w)[:, :, None] * dy).sum(axis=1)
    Z = z.sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(P > 0, P * np.log(P * Z / np.where(w > 0, w, 1.0)), 0.0)
    return {"A": A, "R": R, "z": z, "cost_i": c.sum(axis=1)}


def update(Y, uY, gains, A, R, z, m, eta=200.0, min_gain=0.01):
    """One update from the forces (A already times e) -> Y, uY, gains, dY."""
    dY = A - R / z.sum()
    gains = np.where(np.sign(dY) != np.sign(uY), gains + 0.2, gains * 0.8)
    gains = np.maximum(gains, min_gain)
    uY = m * uY - eta * gains * dY
    Y = Y + uY
    return Y - Y.mean(axis=0), uY, gains, dY


def schedule(it, exaggeration=12.0, stop_lying_iter=250, mom_switch_iter=250, momentum=0.5, final_momentum=0.8, **_):
    return (exaggeration if it <= stop_lying_iter else 1.0), (momentum if it <= mom_switch_iter else final_momentum)


def run(P, Y, n_iter, uY=None, gains=None, first_iter=1, cost_every=50, **sch):
    """-> Y, uY, gains, [(iteration, cost)] after every iteration divisible by cost_every and after the last."""
    s = dict(DEFAULTS, **sch)
    uY = np.zeros_like(Y) if uY is None else uY
    gains = np.ones_like(Y) if gains is None else gains
    costs = []
    last = first_iter + n_iter - 1
    for it in range(first_iter, last + 1):
        e, m = schedule(it, **s)
        f = forces(P, Y, e)
        Y, uY, gains, _ = update(Y, uY, gains, f["A"], f["R"], f["z"], m, s["eta"], s["min_gain"])
        if it == last or (cost_every > 0 and it % cost_every == 0):
            costs.append((it, float(forces(P, Y, 1.0)["cost_i"].sum())))
    return Y, uY, gains, costs


def start(n, seed):
    return 1e-4 * np.random.default_rng(seed).standard_normal((n, 2))


# ---- 50 digits ---------------------------------------------------------------------------------------------------------------
def _f(v):
    return mp.mpf(float(v))


def mp_dist_row(X, i):
    xi = [_f(v) for v in X[i]]
    return [mp.fsum((a - _f(b)) ** 2 for a, b in zip(xi, X[j])) for j in range(len(X))]


# Affinity sums.  Term j of S is p_j = exp(-beta D_ij).  The kernel's p_j: D_ij carries d differences (u each, relative),
# d squares (the square of a value with relative error u: 2u, and its own rounding u) and d - 1 additions of positive values:
# (d + 2) u relative; the product beta D adds u: the exponent is off by at most (d + 3) beta D_ij u, which exp turns into that
# RELATIVE error of p_j.  exp itself is good to 1 ulp = 2u.  The sum: a thread adds ceil(n / 256) terms in a row, then 6
# butterfly levels, 3 additions of wave values and the DBL_MIN: each addition costs u of the (positive) partial sum, so
# depth u of the whole.  K_S = 2 + depth + 1 (second-order terms).  sum_j D_ij p_j: one more product, K + 1.
def k_aff(n):
    return 2 + (-(-n // 256) + 6 + 3 + 1) + 1


def mp_row(X, i, beta, u):
    """Row i at the given beta (a double) in 50 digits -> S, H, delta, bound_S (absolute)."""
    n, d = X.shape
    D = mp_dist_row(X, i)
    b = _f(beta)
    p = [mp.exp(-b * D[j]) if j != i else mp.mpf(0) for j in range(n)]
    S = mp.fsum(p) + _f(DBL_MIN)
    H = b * mp.fsum(Dj * pj for Dj, pj in zip(D, p)) / S + mp.log(S)
    bound = mp.fsum((k_aff(n) + (d + 3) * b * Dj) * U * pj for Dj, pj in zip(D, p))
    return S, H, H - mp.log(_f(u)), bound


# Force sums of point i, with X, beta, S and Y given as doubles (the kernel's own inputs).
#   P_ij: each exponential as above, 2u + (d + 3) beta D u; times 1/S (the reciprocal's rounding and the product's: 2u); the
#   sum of the two (u); times 1/(2n) (its rounding and the product's: 2u):  dP_j = 7u P_ij + (d + 3) u D_ij (beta_i p_j|i +
#   beta_j p_i|j) / (2n).
#   w_ij: the differences d0, d1 (u each), their squares (3u), 1 + d0^2 + d1^2 (2u more, all positive), the division (u): 6u.
#   A term P w d0: dP / P + 6u + the two products (2u) + d0's own u = dP / P + 9u;  R term w w d0: 12u + 3u = 15u;  z term: 6u.
#   Summation: a wave adds its 8 terms of each of the ceil(n / 32) tiles in a row, then two additions join the four waves:
#   depth = 8 ceil(n / 32) + 2, each costing u of the sum of ABSOLUTE terms (the terms of A and R cancel; the bound is
#   relative to that sum, never to the result).  The product with e adds u.  One more u covers second-order terms.
#   Cost: the terms are P ln P, P ln w and P ln Z.  log is good to 1 ulp (2u of its value); an argument off by a relative r
#   moves it by r.  d(P ln P) = dP (|ln P| + 1) + 3u |P ln P|;  d(P ln w) = dP |ln w| + 6u P + 3u |P ln w|;  Z is a sum of
#   positive z_i, each 6u + depth_z u off and added over depth_Z = ceil(n / 1024) + 6 + 15 levels: rZ = (6 + depth + depth_Z) u,
#   so d(P ln Z) = dP |ln Z| + (rZ + 3u |ln Z|) P.  The three sums add depth + 3 roundings of the sum of absolute terms.
def force_depth(n):
    return 8 * (-(-n // 32)) + 2


def mp_point(X, beta, S, Y, i, e=1.0, Z=None, idx=None):
    """Point i in 50 digits from the doubles X, beta, S, Y -> dict A (2), R (2), z, and cost if Z (50 digits) is given.
    idx: the neighbour lists (util_tsne_knn); a half p_{j|i} that is not listed is exactly 0.  None: every pair is listed."""
    n = len(X)
    D = mp_dist_row(X, i)
    mine = None if idx is None else set(int(j) for j in idx[i])
    bi, si = _f(beta[i]), _f(S[i])
    yi = [_f(Y[i, 0]), _f(Y[i, 1])]
    tA, tR, tz, tc = [[], []], [[], []], [], []
    for j in range(n):
        if j == i:
            continue
        P = mp.mpf(0)                                # (0 + a is exact)
        if idx is None or j in mine:
            P += mp.exp(-bi * D[j]) / si
        if idx is None or i in idx[j]:
            P += mp.exp(-_f(beta[j]) * D[j]) / _f(S[j])
        P /= 2 * n
        dy = [yi[0] - _f(Y[j, 0]), yi[1] - _f(Y[j, 1])]
        w = 1 / (1 + dy[0] ** 2 + dy[1] ** 2)
        tz.append(w)
        for c in range(2):
            tA[c].append(_f(e) * P * w * dy[c])
            tR[c].append(w * w * dy[c])
        if Z is not None and P > 0:
            tc.append(P * mp.log(P * Z / w))
    out = {"A": [mp.fsum(tA[0]), mp.fsum(tA[1])], "R": [mp.fsum(tR[0]), mp.fsum(tR[1])], "z": mp.fsum(tz)}
    if Z is not None:
        out["cost"] = mp.fsum(tc)
    return out


def p_bounds(D, d, beta, S, M=None, subnormal=0.0):
    """-> P and dP of the comment above, n x n.  M[i, j]: p_{j|i} is formed (None: for every j != i); `subnormal` is added to
    dP where either half is (util_tsne_knn.SUBNORMAL; the dense kernel's P has no such term)."""
    n = len(D)
    M = ~np.eye(n, dtype=bool) if M is None else M
    pc = np.where(M, np.exp(-beta[:, None] * D) / S[:, None], 0.0)
    P = (pc + pc.T) / (2.0 * n)
    bp = beta[:, None] * pc
    return P, 7 * U * P + (d + 3) * U * D * (bp + bp.T) / (2.0 * n) + np.where(M | M.T, subnormal, 0.0)


def force_bounds(D, d, beta, S, Y, e=1.0, M=None, depA=None, depR=None, subnormal=0.0):
    """The derivation above for every point at once (the bounds themselves need no more than fp64) -> absolute bounds A, R
    (n x 2), z, cost (n) for a device result against 50 digits, the sums of absolute terms they are a share of, and the P they
    were formed from.  depA, depR: the summation depths of A with the cost sums (a number or one per row) and of R with z;
    None: force_depth(n), the dense kernel's for both.  M, subnormal: as for p_bounds."""
    n = len(D)
    depA = force_depth(n) if depA is None else depA
    depR = force_depth(n) if depR is None else depR
    P, dP = p_bounds(D, d, beta, S, M, subnormal)
    dy = Y[:, None, :] - Y[None, :, :]
    w = 1.0 / (1.0 + dy[:, :, 0] ** 2 + dy[:, :, 1] ** 2)
    np.fill_diagonal(w, 0.0)
    out = {"A": np.zeros((n, 2)), "R": np.zeros((n, 2)), "abs_A": np.zeros((n, 2)), "abs_R": np.zeros((n, 2)), "P": P}
    for c in range(2):
        tA, tR = np.abs(e * P * w * dy[:, :, c]), np.abs(w * w * dy[:, :, c])
        out["abs_A"][:, c], out["abs_R"][:, c] = tA.sum(1), tR.sum(1)
        out["A"][:, c] = (np.abs(e * w * dy[:, :, c]) * dP + 10 * U * tA).sum(1) + (depA + 1) * U * tA.sum(1)
        out["R"][:, c] = (15 + depR + 1) * U * tR.sum(1)
    z = w.sum(1)
    out["z"], out["abs_z"] = (6 + depR + 1) * U * z, z
    lnZ = abs(math.log(z.sum()))
    rZ = (6 + depR + (-(-n // 1024)) + 6 + 15) * U
    with np.errstate(divide="ignore", invalid="ignore"):
        lp = np.where(P > 0, np.abs(np.log(np.where(P > 0, P, 1.0))), 0.0)
        lw = np.where(w > 0, np.abs(np.log(np.where(w > 0, w, 1.0))), 0.0)
    pos = P > 0
    ec = np.where(pos, dP * (lp + 1 + lw + lnZ) + U * (3 * P * lp + 6 * P + 3 * P * lw) + P * (rZ + 3 * U * lnZ), 0.0)
    sc = np.where(pos, P * lp + P * lw + P * lnZ, 0.0).sum(1)
    out["cost"], out["abs_cost"] = ec.sum(1) + (depA + 4) * U * sc, sc
    return out


def mp_Z(Y):
    """sum_{i != j} w_ij: the w in fp64 (each within 6u), added exactly; the cost bound's rZ covers the 6u."""
    dy = Y[:, None, :] - Y[None, :, :]
    w = 1.0 / (1.0 + dy[:, :, 0] * dy[:, :, 0] + dy[:, :, 1] * dy[:, :, 1])
    np.fill_diagonal(w, 0.0)
    return mp.mpf(math.fsum(w.ravel()))


# The update, element by element, given the device's own A (times e), R, z and state before the step.  Z is a sum of n positive
# doubles over ceil(n / 1024) + 6 + 15 additions: rZ = that many u.  dY = A - R / Z: |d dY| <= u |A|... A is an input, so:
# (rZ + u) |R / Z| + u |dY| =: bdY.  The gain is a choice (see below), exact up to one rounding (u gains).  uY = m uY - eta gains dY:
# |d uY| <= u |m uY| + eta gains (bdY + 3u |dY|) + u |uY'|.  Y + uY: + u |Y'|.  The column mean: n additions in a tree of depth
# ceil(n / 1024) + 21 and a division, of values that each carry the error above; subtracting it adds the mean's error and u.
# An element with |dY| <= bdY may have taken the other gain: the test tries both.
def update_bounds(Y, uY, gains, A, R, z, m, eta=200.0, min_gain=0.01):
    n = len(Y)
    depth = -(-n // 1024) + 21
    Zs = z.sum()
    dY = A - R / Zs
    bdY = (depth + 2) * U * np.abs(R / Zs) + U * np.abs(dY)
    Yn, uYn, gn, _ = update(Y, uY, gains, A, R, z, m, eta, min_gain)
    buY = U * np.abs(m * uY) + eta * gn * (bdY + 3 * U * np.abs(dY)) + 2 * U * np.abs(uYn)
    bYraw = buY + U * np.abs(Y + uYn)
    bmean = bYraw.mean(axis=0) + (depth + 2) * U * np.abs(Y + uYn).mean(axis=0)
    bY = bYraw + bmean + U * np.abs(Yn)
    return {"dY": dY, "bdY": bdY, "buY": buY, "bY": bY, "bgain": 2 * U * gn}


# ---- cases -----------------------------------------------------------------------------------------------------------------
def clusters(n, d, k=4, seed=0, spread=0.05):
    """Columns of a simulated h: n cells around k cluster profiles in d coordinates, non-negative like coefficients."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0.0, 1.0, size=(k, d)) + np.eye(k, d) * 1.5
    lab = rng.integers(0, k, size=n)
    return np.abs(centres[lab] + spread * rng.standard_normal((n, d))), lab


def perplexity_for(n):
    """30 where the rule 3u < n - 1 allows it, else the largest integer it allows (n = 5: 1)."""
    return float(min(30, -(-(n - 1) // 3) - 1))


def spread_Y(n, seed):
    """A late map: points spread over tens of units."""
    return 20.0 * np.random.default_rng(seed).standard_normal((n, 2))


@functools.lru_cache(maxsize=None)
def case(n, d, k=4, seed=0, kind="clusters", normalize=True, scale=1.0):
    """-> dict X (as handed to the library), Xn (what the affinities see), u, lab, and lazily the restatement's results."""
    X, lab = clusters(n, d, k, seed)
    if kind == "identical":
        X = np.tile(X[:1], (n, 1))
    elif kind == "outlier":
        X = X.copy()
        X[n // 2] += 1.0e3
    X = X * scale
    u = perplexity_for(n)
    Xn = normalise(X) if normalize else X.copy()
    return {"X": X, "Xn": Xn, "u": u, "lab": lab, "n": n, "d": d, "normalize": normalize}


@functools.lru_cache(maxsize=None)
def case_affinities(*key, **kw):
    c = case(*key, **kw)
    D = sq_dist(c["Xn"])
    beta, S, trips, flagged = affinities(c["Xn"], c["u"], D)
    return {"D": D, "beta": beta, "S": S, "trips": trips, "flagged": flagged}


# ---- shapes and inputs of the GPU tests; tests/test_tsne_cpu.py checks that the restatement flags no row of any of them --------
def shape_cases(i_block, j_tile, lds_row):
    """Arguments of case() -- (n, d) or (n, d, k, seed) -- : the perplexity rule's minimum, wave and workgroup edges, one below / at / one above the force kernel's
    i-block and j-tile, one above the affinity kernel's LDS row, every d at which a launch takes another path."""
    out = [(5, 2, 4, 1), (63, 10), (64, 33), (65, 128), (255, 10), (256, 2), (257, 33), (129, 20)]
    out += [(j_tile - 1, 1), (j_tile, 2), (j_tile + 1, 10)]
    out += [c for c in ((i_block - 1, 10), (i_block, 33), (i_block + 1, 128)) if c not in out]
    return out, (lds_row + 1, 10)


def full_lds_row(lds_row):
    """(n, d, k, seed) for the affinities alone: n = the LDS row's capacity, the largest n whose distance row stays in LDS, and
    more points than k_tsne_affinity has workgroups (min(n, 4 x CUs)) -- a workgroup fills its LDS row a second time.  (The
    seed is one at which the restatement flags no row at n = 2048: seeds 0, 1 and 2 flag two, one and one.)"""
    return (lds_row, 3, 4, 3)


def shape_kw(c):
    return dict(zip(("n", "d", "k", "seed"), c))


SPECIAL = {                                  # name -> arguments of case()
    "identical": dict(n=65, d=2, kind="identical"),
    # (the outlier's row converges where beta D is just short of exp's underflow, about 700: d = 5 keeps (d + 3) beta D u < CAP)
    "outlier": dict(n=65, d=5, kind="outlier", normalize=False),
    "scaled_up": dict(n=65, d=10, seed=1, normalize=False, scale=1.0e3),
    "scaled_down": dict(n=65, d=10, normalize=False, scale=1.0e-3),
}

# End to end: n = 300, d = 3, three clusters (case(300, 3, 3, 11)), perplexity 30, the default schedule.  The restatement, on
# the CPU, from start(300, seed) for seed = 0 .. 4: every point's nearest neighbour in Y has its own cluster (300 of 300, all
# five seeds); the cost after iteration 250 is 1.1698, 1.1695, 1.1689, 1.1696, 1.1695; the final costs are E2E_FINAL.
E2E = dict(n=300, d=3, k=3, seed=11)
E2E_FINAL = (0.28726339468839934, 0.2740588050049169, 0.28419602357038803, 0.2830980237485424, 0.30152232496421605)
E2E_NN_SAME = 300


def nn_same(Y, cid):
    """The points whose nearest neighbour in Y has their own cluster."""
    d2 = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d2, np.inf)
    return int((cid[d2.argmin(axis=1)] == cid).sum())
