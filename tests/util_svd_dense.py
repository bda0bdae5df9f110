"""Inputs, models and references for the dense kernels of the device-resident truncated SVD (csrc/init.h: k_gram, k_small,
k_apply), shared by tests/test_svd_dense_cpu.py (no GPU: the models against the bounds) and tests/test_gpu_svd_dense.py
(the kernels against the same bounds on the same inputs).

* jacobi_model / cholesky_model: plain Python restatements of k_small's two modes in the kernel's own order of
  operations (pair order, rotation formulas, stopping rule, selection sort; the library is compiled without fused
  multiply-adds outside explicit fma calls, and Python's float arithmetic is the same IEEE double arithmetic).
* References: products and sums of doubles are formed EXACTLY, as integers times a power of two (a double is one), and
  turned into 50-digit mpmath numbers only at the end; eigenvalues are mpmath.eigsy's and the Cholesky factor of G
  mpmath.cholesky's at 50 digits.
* The bounds are the issue's: derived from the arithmetic, none measured."""
import functools
import math

import mpmath as mp
import numpy as np

mp.mp.dps = 50
U = 2.0 ** -53                      # unit roundoff of a double
GRAM_BLOCKS = 256                   # kGramBlocks
WIDTHS = (2, 14, 32, 40, 64)


# ---------------------------------------------------------------- exact arithmetic on doubles
def to_fixed(A):
    """(I, e): object array of Python ints and an exponent with A == I * 2**e exactly."""
    A = np.asarray(A, dtype=np.float64)
    assert np.all(np.isfinite(A))
    m, ex = np.frexp(A)
    mant = np.ldexp(m, 53).astype(np.int64)                  # |m| < 1: 53-bit integers, exact
    ex = ex.astype(np.int64) - 53
    nz = mant != 0
    e = int(ex[nz].min()) if nz.any() else 0
    shift = np.where(nz, ex - e, 0)
    ints = np.left_shift(mant.astype(object), shift.astype(object))            # Python ints: no width to overflow
    return np.asarray(ints, dtype=object).reshape(A.shape), e


def exact_matmul(A, B):
    """(P, e) with A @ B == P * 2**e exactly (A, B arrays of doubles)."""
    Ia, ea = to_fixed(A)
    Ib, eb = to_fixed(B)
    return Ia.dot(Ib), ea + eb


def exact_chain(*mats):
    """(P, e) with the product of all the matrices == P * 2**e exactly."""
    P, e = to_fixed(mats[0])
    for M in mats[1:]:
        Im, em = to_fixed(M)
        P, e = P.dot(Im), e + em
    return P, e


def to_mp(P, e):
    """The exact numbers P * 2**e as a nested list of 50-digit mpmath numbers."""
    P = np.asarray(P, dtype=object)
    flat = [mp.ldexp(mp.mpf(int(v)), e) for v in P.ravel()]
    return np.asarray(flat, dtype=object).reshape(P.shape)


def abs_err(X, P, e):
    """|X - P * 2**e| as doubles, the difference formed in 50 digits."""
    X = np.asarray(X, dtype=np.float64)
    ref = to_mp(P, e)
    out = np.empty(X.shape)
    for idx in np.ndindex(X.shape):
        out[idx] = float(abs(mp.mpf(float(X[idx])) - ref[idx]))
    return out


def max_err_vs_identity(P, e):
    """max |P * 2**e - I| in 50 digits (P square)."""
    ref = to_mp(P, e)
    worst = mp.mpf(0)
    for (i, j), v in np.ndenumerate(ref):
        worst = max(worst, abs(v - (1 if i == j else 0)))
    return float(worst)


# ---------------------------------------------------------------- k_gram
GRAM_N = (1, 31, 32, 33, 255, 256, 257, 256 * 32 + 5, 20011)
# The real-valued cases: every N at every width.  The exact reference costs N integer products per entry of G, so it is
# formed for a sample of the entries (gram_sample_pairs: the corners of the 32 x 32 thread tiles, diagonal entries, random
# pairs); every entry is held to the blockwise numpy Gram matrix at twice the bound (each side obeys it), and the
# symmetry and two-launch comparisons, which need no reference, cover every entry as well.
GRAM_REAL_CASES = tuple((N, R) for R in WIDTHS for N in GRAM_N)


def gram_sample_pairs(R, seed=5):
    """(i, j) entries of G held to the exact reference: the corners of each 32 x 32 tile of G a thread block covers (four
    tiles from R = 40 on), diagonal entries, and random pairs -- every entry if G has at most 40 of them."""
    if R * R <= 40:
        return [(i, j) for i in range(R) for j in range(R)]
    edges = sorted({0, min(31, R - 1), min(32, R - 1), R - 1})
    pairs = {(i, j) for i in edges for j in edges}
    rng = np.random.default_rng([seed, R])
    pairs |= {(int(i), int(i)) for i in rng.integers(0, R, 4)}
    pairs |= {(int(i), int(j)) for i, j in rng.integers(0, R, size=(24, 2))}
    return sorted(pairs)


def gram_sample_errors(G, A, pairs):
    """|G_ij - sum_q a_qi a_qj| for the sampled entries, the sum formed exactly and the difference read off in 50 digits."""
    cols = sorted({c for p in pairs for c in p})
    where = {c: n for n, c in enumerate(cols)}
    ints, e = to_fixed(A[:, cols])
    lists = [ints[:, n].tolist() for n in range(len(cols))]
    out = []
    for i, j in pairs:
        exact = sum(map(int.__mul__, lists[where[i]], lists[where[j]]))
        out.append(float(abs(mp.mpf(float(G[i, j])) - mp.ldexp(mp.mpf(exact), 2 * e))))
    return np.array(out)


def blockwise_gram(A):
    """The block partials of t(A) A over k_gram's split of the rows, numpy's order inside a block."""
    N, R = A.shape
    gp = np.zeros((GRAM_BLOCKS, R, R))
    for b in range(GRAM_BLOCKS):
        n0, n1 = gram_rows_of_block(N, b)
        if n1 > n0:
            gp[b] = A[n0:n1].T @ A[n0:n1]
    return gp


def gram_integer_input(N, R, seed):
    """Integer-valued A, |a| <= 1024: every product and every partial sum of t(A) A is an integer below 2^53."""
    rng = np.random.default_rng([seed, N, R])
    return rng.integers(-1024, 1025, size=(N, R)).astype(np.float64)


def gram_real_input(N, R, seed):
    """Standard normal times a per-column scale spanning 1e-6 .. 1e6."""
    rng = np.random.default_rng([seed, N, R, 1])
    scale = np.logspace(-6, 6, R) if R > 1 else np.ones(1)
    return rng.standard_normal((N, R)) * rng.permutation(scale)[None, :]


def gram_bound(A):
    """|G_ij - ref_ij| <= (N + 256) 2^-53 sum_q |a_qi| |a_qj|: at most N - 1 + 255 additions and one rounding per product
    stand between any summation order over the rows and blocks and the exact sum."""
    N = A.shape[0]
    aa = np.abs(A)
    return (N + GRAM_BLOCKS) * U * (aa.T @ aa)


def gram_rows_of_block(N, b):
    """[n0, n1) of block b: k_gram's own split of the rows."""
    per = (N + GRAM_BLOCKS - 1) // GRAM_BLOCKS
    n0 = b * per
    return n0, max(n0, min(N, n0 + per))


def sum_partials(gp):
    """G as k_small forms it: the block partials added in block order."""
    G = np.zeros_like(gp[0])
    for b in range(gp.shape[0]):
        G = G + gp[b]
    return G


# ---------------------------------------------------------------- k_small, Jacobi mode
def jacobi_model(G, scale_free=True, max_sweeps=30):
    """k_small (mode 1) on the k x k symmetric G, in the kernel's order.  Returns (S [k][k] eigenvectors in columns,
    vals descending, S2 = S / sqrt(vals), sweeps done).  scale_free=False is the stopping rule before it was made
    invariant under scaling (off <= 1e-30 tr^2 on the squares of the entries themselves)."""
    G = [list(map(float, row)) for row in np.asarray(G, dtype=np.float64)]
    k = len(G)
    V = [[1.0 if i == j else 0.0 for j in range(k)] for i in range(k)]
    sweeps = 0
    for _ in range(max_sweeps):
        o = 0.0
        if scale_free:
            ex = math.frexp(max(abs(G[p][p]) for p in range(k)))[1]
            tr = 0.0
            for p in range(k):
                tr += math.ldexp(abs(G[p][p]), -ex)
            for p in range(k):
                for q in range(p + 1, k):
                    rel = math.ldexp(G[p][q], -ex)
                    o += rel * rel
            if o <= 1e-30 * tr * tr:
                break
        else:
            tr = 0.0
            for p in range(k):
                tr += abs(G[p][p])
            with np.errstate(over="ignore", invalid="ignore"):
                for p in range(k):
                    for q in range(p + 1, k):
                        o = float(np.float64(o) + np.float64(G[p][q]) * np.float64(G[p][q]))
                if bool(np.float64(o) <= np.float64(1e-30) * np.float64(tr) * np.float64(tr)):
                    break
        sweeps += 1
        for p in range(k - 1):
            for q in range(p + 1, k):
                apq = G[p][q]
                c, s = 1.0, 0.0
                if apq != 0.0:
                    tau = (G[q][q] - G[p][p]) / (2.0 * apq)
                    t = (1.0 if tau >= 0.0 else -1.0) / (abs(tau) + math.sqrt(1.0 + tau * tau))
                    c = 1.0 / math.sqrt(1.0 + t * t)
                    s = t * c
                for j in range(k):                           # columns p, q: G <- G J, V <- V J
                    gp_, gq_ = G[j][p], G[j][q]
                    G[j][p], G[j][q] = c * gp_ - s * gq_, s * gp_ + c * gq_
                    vp, vq = V[j][p], V[j][q]
                    V[j][p], V[j][q] = c * vp - s * vq, s * vp + c * vq
                Gp, Gq = G[p], G[q]
                for j in range(k):                           # rows p, q: G <- t(J) G
                    gp_, gq_ = Gp[j], Gq[j]
                    Gp[j], Gq[j] = c * gp_ - s * gq_, s * gp_ + c * gq_
    perm = list(range(k))
    for a in range(k):                                       # the kernel's selection sort, descending
        best = a
        for b in range(a + 1, k):
            if G[perm[b]][perm[b]] > G[perm[best]][perm[best]]:
                best = b
        perm[a], perm[best] = perm[best], perm[a]
    vals = np.array([G[perm[c]][perm[c]] for c in range(k)])
    S = np.array([[V[i][perm[j]] for j in range(k)] for i in range(k)])
    S2 = np.zeros((k, k))
    for j in range(k):
        if vals[j] > 0.0:
            S2[:, j] = S[:, j] / math.sqrt(vals[j])
    return S, vals, S2, sweeps


def spectrum_matrix(spec, seed):
    """G = Q diag(spec) t(Q), symmetrised, Q a random orthogonal matrix."""
    spec = np.asarray(spec, dtype=np.float64)
    k = spec.size
    rng = np.random.default_rng([seed, k])
    Q, _ = np.linalg.qr(rng.standard_normal((k, k)))
    G = (Q * spec[None, :]) @ Q.T
    return (G + G.T) / 2.0


def integer_spd(k, seed):
    """Integer-valued symmetric positive definite G (t(B) B, |b| <= 8) and 256 integer partials that sum to it exactly
    in any order (every partial sum is an integer far below 2^53)."""
    rng = np.random.default_rng([seed, k, 2])
    B = rng.integers(-8, 9, size=(3 * k, k)).astype(np.float64)
    G = B.T @ B
    parts = rng.integers(-1000, 1001, size=(GRAM_BLOCKS, k, k)).astype(np.float64)
    parts = parts + parts.transpose(0, 2, 1)
    parts[-1] += G - parts.sum(axis=0)
    assert np.array_equal(parts.sum(axis=0), G)
    return G, parts


def _jacobi_cases():
    cases = {
        # name: (R, k, G)
        "graded_1e-12_k64": (64, 64, spectrum_matrix(np.logspace(0, -12, 64), 1)),
        "graded_1e-6_k32": (32, 32, spectrum_matrix(np.logspace(0, -6, 32), 2)),
        "repeated_k40": (40, 40, spectrum_matrix(np.tile([5.0, 2.0, 2.0, 1.0], 10), 3)),
        "clustered_k64": (64, 64, spectrum_matrix(1.0 + 1e-9 * np.arange(64), 4)),
        "rank_deficient_k24": (32, 24, spectrum_matrix(np.concatenate([np.logspace(0, -6, 12), np.zeros(12)]), 5)),
        "k1": (2, 1, np.array([[3.25]])),
        "k13_in_R14": (14, 13, spectrum_matrix(np.logspace(0, -4, 13), 6)),
        "k6_in_R32": (32, 6, spectrum_matrix(np.array([9.0, 4.0, 4.0, 1.0, 0.5, 1e-3]), 7)),
        "k10_well_conditioned": (10, 10, spectrum_matrix(np.linspace(1.0, 2.0, 10), 8)),
        "integer_k20": (20, 20, integer_spd(20, 9)[0]),
    }
    return cases


JACOBI_CASES = _jacobi_cases()
SCALE_CASE = "k10_well_conditioned"             # the 10 x 10 matrix of the scaling tests (G 2^600, G 2^-600)
# ... and two powers nearer the ends of the range: at 2^1021 the entries are finite and their diagonal's sum is not; at
# 2^-900 the off-diagonal entries of the last sweep (1e-20 of the diagonal) are still normal numbers
SCALE_POWERS = (600, -600, 1021, -900)


@functools.lru_cache(maxsize=None)
def eigenvalues_50(name):
    """The eigenvalues of the fp64 matrix JACOBI_CASES[name] (descending), mpmath.eigsy at 50 digits."""
    G = JACOBI_CASES[name][2]
    E = mp.eigsy(mp.matrix(G.tolist()), eigvals_only=True)
    return sorted((E[i] for i in range(len(E))), reverse=True)


def jacobi_tolerances(G, ref):
    """(tol, orth_tol): tol = 30 k 2^-53 lambda_0 + 1e-15 sum |G_pp| bounds the errors of the eigenvalues and of G S -
    S diag(vals) (at most 30 k rounding errors of size lambda_0 per entry over 30 sweeps, plus the off-diagonal norm
    the stopping rule leaves: sqrt(1e-30) tr); orth_tol = 30 k 2^-53 bounds t(S) S - I."""
    k = G.shape[0]
    lam0 = float(max(abs(ref[0]), abs(ref[-1])))
    return 30 * k * U * lam0 + 1e-15 * float(np.sum(np.abs(np.diag(G)))), 30 * k * U


def jacobi_errors(G, S, vals, ref):
    """(eigenvalue error, residual max |G S - S diag(vals)|, orthogonality max |t(S) S - I|), each formed exactly and
    read off in 50 digits.  G, S: k x k; vals: k; ref: the 50-digit eigenvalues, descending."""
    k = G.shape[0]
    e_val = max(float(abs(mp.mpf(float(vals[i])) - ref[i])) for i in range(k))
    P1, e1 = exact_matmul(G, S)
    P2, e2 = exact_matmul(S, np.diag(vals))
    e = min(e1, e2)
    D = P1 * (1 << (e1 - e)) - P2 * (1 << (e2 - e))
    e_res = float(max(abs(v) for v in to_mp(D, e).ravel()))
    e_orth = max_err_vs_identity(*exact_matmul(S.T, S))
    return e_val, e_res, e_orth


# ---------------------------------------------------------------- k_small, Cholesky mode
def cholesky_model(G):
    """k_small (mode 0) on the k x k G, in the kernel's order: (status, S = inverse of the upper factor, diag of the factor)."""
    G = [list(map(float, row)) for row in np.asarray(G, dtype=np.float64)]
    k = len(G)
    V = [[1.0 if i == j else 0.0 for j in range(k)] for i in range(k)]
    for c in range(k):
        dsum = G[c][c]
        for q in range(c):
            dsum -= V[q][c] * V[q][c]
        if not dsum > 0.0:
            return 1, np.zeros((k, k)), np.array([V[i][i] for i in range(k)])
        dd = math.sqrt(dsum)
        V[c][c] = dd
        for t in range(c + 1, k):
            s2 = G[c][t]
            for q in range(c):
                s2 -= V[q][c] * V[q][t]
            V[c][t] = s2 / dd
        for t in range(c):
            V[c][t] = 0.0
    S = [[0.0] * k for _ in range(k)]
    for c in range(k):
        S[c][c] = 1.0 / V[c][c]
        for t in range(c - 1, -1, -1):
            s2 = 0.0
            for q in range(t + 1, c + 1):
                s2 += V[t][q] * S[q][c]
            S[t][c] = -s2 / V[t][t]
    return 0, np.array(S), np.array([V[i][i] for i in range(k)])


# name: (R, k, N, cond(A))
CHOLESKY_CASES = {
    "cond1e2_k64": (64, 64, 1000, 1e2),
    "cond1e5_k40": (40, 40, 700, 1e5),
    "cond1e5_k6_in_R32": (32, 6, 300, 1e5),
    "cond1e7_k13_in_R14": (14, 13, 600, 1e7),
}
TWO_PASS_CASE = "cond1e7_k13_in_R14"
# max |t(S) G S - I| of numpy's Cholesky factor and its triangular inverse, as tests/test_svd_dense_cpu.py printed it: the
# yardstick of the 16 x bound.  The tests take the yardstick afresh from the G at hand and hold it within 4 x of these.
CHOLESKY_NUMPY_BASELINE = {"cond1e2_k64": 3.12e-14, "cond1e5_k40": 3.04e-08, "cond1e5_k6_in_R32": 1.55e-07, "cond1e7_k13_in_R14": 5.98e-04}


def tall_block(name):
    """A [N][R] with singular values 1 .. 1/cond in its k leading columns, zeros in the padding columns."""
    R, k, N, cond = CHOLESKY_CASES[name]
    rng = np.random.default_rng([11, R, k, N])
    Q, _ = np.linalg.qr(rng.standard_normal((N, k)))
    W, _ = np.linalg.qr(rng.standard_normal((k, k)))
    A = np.zeros((N, R))
    A[:, :k] = (Q * np.logspace(0, -math.log10(cond), k)[None, :]) @ W.T
    return A


def cholesky_diag_50(G):
    """diag(U) of the Cholesky factor G = t(U) U of the fp64 matrix G, mpmath.cholesky at 50 digits."""
    L = mp.cholesky(mp.matrix(np.asarray(G).tolist()))
    return [L[i, i] for i in range(L.rows)]


def cholesky_diag_bound(G):
    """Bound on max |diag(U computed) - diag(U)| for a Cholesky factorisation of G in fp64 by inner products, or None
    where the theory promises nothing.  Backward error (Higham, Accuracy and Stability of Numerical Algorithms, Thm
    10.3): t(Uc) Uc = G + dG with |dG| <= g |t(Uc)| |Uc|, g = (k + 1) u / (1 - (k + 1) u), hence ||dG||_2 <= eps ||G||_2
    with eps = k g / (1 - k g).  Perturbation of the factor (Sun 1991; Higham Thm 10.8): ||Uc - U||_F / ||U||_2 <=
    x / (sqrt(2) (1 - x)), x = cond_2(G) eps, valid for x < 1 (taken here up to 1/2); ||U||_2 = sqrt(lambda_max).
    The eigenvalues of G behind cond_2 are mpmath.eigsy's at 50 digits."""
    k = G.shape[0]
    E = mp.eigsy(mp.matrix(np.asarray(G).tolist()), eigvals_only=True)
    lam = sorted(E[i] for i in range(len(E)))
    g = (k + 1) * U / (1 - (k + 1) * U)
    eps = k * g / (1 - k * g)
    x = float(lam[-1] / lam[0]) * eps if lam[0] > 0 else math.inf
    if not x < 0.5:
        return None
    return float(mp.sqrt(lam[-1])) * x / (math.sqrt(2.0) * (1 - x))


def cholesky_diag_error(diag, G):
    """max |diag - diag(U)| against the 50-digit factor."""
    ref = cholesky_diag_50(G)
    return max(float(abs(mp.mpf(float(d)) - r)) for d, r in zip(diag, ref))


def whitening_error(G, S):
    """max |t(S) G S - I| over the k x k blocks, formed exactly and read off in 50 digits."""
    return max_err_vs_identity(*exact_chain(S.T, G, S))


def numpy_whitening_error(G):
    """The same quantity for numpy's Cholesky factor of the same fp64 G and its triangular inverse."""
    import scipy.linalg
    Uf = np.linalg.cholesky(G).T
    S = scipy.linalg.solve_triangular(Uf, np.eye(G.shape[0]), lower=False)
    return whitening_error(G, np.triu(S))


def equal_columns_gram(k, R):
    """(A, t(A) A) for an integer block whose columns 0 and 1 are equal, 25 entries of +-1 each: exactly singular, and the
    recurrence meets the zero pivot without a rounding on the way (sqrt(25), 25 / 5 and 25 - 5 * 5 are exact), so
    `not positive definite` is the only right answer, not one of two that rounding could choose between."""
    rng = np.random.default_rng([13, k, R])
    A = np.zeros((50, R))
    A[:, :k] = rng.integers(-4, 5, size=(50, k))
    A[:, 0] = np.where(np.arange(50) % 2 == 0, rng.choice([-1.0, 1.0], size=50), 0.0)
    A[:, 1] = A[:, 0]
    return A, A.T @ A


# ---------------------------------------------------------------- k_apply
APPLY_N = (1, 255, 256, 257, 5000)
APPLY_S_CASES = ("k6_in_R32", "k13_in_R14", "repeated_k40", "clustered_k64")     # S = the Jacobi eigenvectors of these


def apply_input(N, R, seed=21):
    rng = np.random.default_rng([seed, N, R])
    return rng.standard_normal((N, R)) * np.exp(rng.uniform(-3, 3, size=(N, 1)))


def apply_check_rows(N):
    """The rows held to the 50-digit product: all of them up to N = 257; beyond, the ends, the rows either side of the
    256-row blocks' edges, and a spread."""
    if N <= 257:
        return np.arange(N)
    rows = {0, 1, 254, 255, 256, 257, 511, 512, N - 2, N - 1} | set(range(7, N, max(1, N // 12)))
    return np.array(sorted(r for r in rows if 0 <= r < N))


def apply_bound(A, S):
    """|B_rc - ref_rc| <= R 2^-53 sum_q |a_rq| |s_qc|: R - 1 additions and one rounding per product, in any order."""
    return A.shape[1] * U * (np.abs(A) @ np.abs(S))


def pad_square(M, R):
    out = np.zeros((R, R))
    out[:M.shape[0], :M.shape[1]] = M
    return out


# ---------------------------------------------------------------- k_normal_init
NORMAL_SHAPES = ((1, 1, 2), (257, 13, 14), (5000, 40, 40), (700, 6, 32))
NORMAL_SEEDS = (12345, (1 << 40) + 977)
