"""GPU: the dense kernels of the device-resident truncated SVD (csrc/init.h: k_gram, k_small in its Cholesky and Jacobi
modes, k_apply, k_normal_init), each launched ALONE through its test hook (vbnmf_test_svd_*: the product's kernel, the
product's launch geometry) and held to exact or 50-digit references (tests/util_svd_dense.py) with bounds derived from
the arithmetic.  No iteration stands between a kernel and its check, and nothing can fall back to the host.

Every input here is run through a numpy / plain-Python model of the same operation by tests/test_svd_dense_cpu.py, which
holds the model to the same bounds.  That test's figures for the Cholesky mode (numpy.linalg.cholesky and a triangular
inverse of the same kind of matrix; max |t(S) G S - I| in 50 digits), which the 16 x bound below is taken from at run
time on the kernel's own G:
    cond(A) 1e2, k 64: 3.1e-14    cond(A) 1e5, k 40: 3.0e-08    cond(A) 1e5, k 6 in R 32: 1.6e-07    cond(A) 1e7, k 13: 6.0e-04
and the model of the kernel's own order: 4.8e-14, 9.8e-09, 4.2e-08, 4.8e-04; two passes at cond 1e7 leave 3.5e-16.
On an MI355X the kernel itself (its G comes from k_gram, so it is not the model's to the bit): 7.4e-14, 1.6e-08, 3.5e-08,
7.6e-04 against 16 x numpy's 3.3e-14, 3.2e-08, 2.6e-07, 2.6e-04 on that G; two passes leave 6.0e-16.  The Jacobi mode
reproduced the model's figures digit for digit (worst: eigenvalues 8.4e-14 against a bound of 7.7e-13, repeated
spectrum at k = 40); k_gram and k_apply used 0.02 and 0.16 of their any-order bounds; k_normal_init was within 8.9e-16."""
import ctypes
import math

import numpy as np
import pytest

import util_svd_dense as D

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- the hooks
def _lib():
    from ccfindr_amd import _native as N
    return N, N.load()


def gram(A):
    N_, L = _lib()
    A = np.ascontiguousarray(A, dtype=np.float64)
    n, R = A.shape
    gp = np.full((D.GRAM_BLOCKS, R, R), np.nan)
    N_.check(L.vbnmf_test_svd_gram(R, n, N_.dptr(A), N_.dptr(gp)))
    return gp


def small(gp, k, mode, seq=0.0):
    """(S [R][R], S2 [R][R], vals [R], vals_host [R + 1], status) of one k_small launch on the partials gp [nb][R][R]."""
    N_, L = _lib()
    gp = np.ascontiguousarray(gp, dtype=np.float64)
    nb, R, _ = gp.shape
    S, S2 = np.full((R, R), np.nan), np.full((R, R), np.nan)
    vals, vals_host = np.full(R, np.nan), np.full(R + 1, np.nan)
    status = np.full(1, -1, dtype=np.int32)
    N_.check(L.vbnmf_test_svd_small(R, k, mode, nb, N_.dptr(gp), float(seq), N_.dptr(S), N_.dptr(S2) if mode == 1 else None,
                                    N_.dptr(vals), N_.dptr(vals_host), status.ctypes.data_as(N_.c_int32_p)))
    return S, S2, vals, vals_host, int(status[0])


def apply(A, S, in_place):
    N_, L = _lib()
    A = np.ascontiguousarray(A, dtype=np.float64)
    S = np.ascontiguousarray(S, dtype=np.float64)
    B = np.full(A.shape, np.nan)
    N_.check(L.vbnmf_test_svd_apply(A.shape[1], A.shape[0], N_.dptr(A), N_.dptr(S), 1 if in_place else 0, N_.dptr(B)))
    return B


def normal(nmaj, r, R, seed):
    N_, L = _lib()
    g = np.full((nmaj, R), np.nan)
    N_.check(L.vbnmf_test_svd_normal(nmaj, r, R, ctypes.c_uint64(seed), N_.dptr(g)))
    return g


def one_partial(G, R, fill=np.nan):
    """G (k x k) as a single R x R partial; what lies outside the k x k block is the kernel's to ignore."""
    k = G.shape[0]
    gp = np.full((1, R, R), fill)
    gp[0, :k, :k] = G
    return gp


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# ---------------------------------------------------------------- k_gram
@pytest.mark.parametrize("R", D.WIDTHS)
def test_gram_of_integer_blocks_is_exact_block_by_block(R):
    """|a| <= 1024, integers: every product and sum is exact in fp64, so each block's partial must EQUAL the Gram matrix of
    the rows the block owns, blocks without rows must hold exact zeros, and the sum must equal t(A) A in integers."""
    for N in D.GRAM_N:
        A = D.gram_integer_input(N, R, seed=3)
        gp = gram(A)
        assert same_bits(gp, gram(A)), N                                      # two launches, equal bits
        Ai = A.astype(np.int64)
        assert np.array_equal(gp.sum(axis=0), (Ai.T @ Ai).astype(np.float64)), N
        owners = 0
        for b in range(D.GRAM_BLOCKS):
            n0, n1 = D.gram_rows_of_block(N, b)
            owners += n1 > n0
            assert np.array_equal(gp[b], A[n0:n1].T @ A[n0:n1]), (N, b)         # (exact in numpy too; +0 for an empty block)
            assert n1 > n0 or not np.signbit(gp[b]).any()
        per = -(-N // D.GRAM_BLOCKS)
        assert owners == -(-N // per)                                          # (most blocks own nothing below N = 256)


@pytest.mark.parametrize("R", D.WIDTHS)
def test_gram_of_real_blocks_within_the_any_order_bound(R):
    """Every N at every width.  A sample of G's entries (the corners of the 32 x 32 thread tiles, diagonal entries, random
    pairs) against the exact sum read off in 50 digits, to the bound; every entry against numpy's Gram matrix over the
    same split of the rows, to twice the bound (each side obeys it); symmetry and two launches on every entry."""
    pairs = D.gram_sample_pairs(R)
    worst = 0.0
    for N in D.GRAM_N:
        assert (N, R) in D.GRAM_REAL_CASES
        A = D.gram_real_input(N, R, seed=4)
        gp = gram(A)
        assert same_bits(gp, gram(A)), N
        G = D.sum_partials(gp)
        assert same_bits(G, G.T.copy()), N                                    # the same fma chain with the factors swapped
        for b in range(D.GRAM_BLOCKS):
            n0, n1 = D.gram_rows_of_block(N, b)
            assert n1 > n0 or not gp[b].any(), (N, b)
        bound = D.gram_bound(A)
        assert np.all(np.abs(G - D.sum_partials(D.blockwise_gram(A))) <= 2 * bound), N
        ratio = float(np.max(D.gram_sample_errors(G, A, pairs) / np.array([bound[i, j] for i, j in pairs])))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (N, ratio)
    print(f"k_gram R = {R}: largest |G - exact| / ((N + 256) 2^-53 sum |a||a|) = {worst:.3g} (bound 1)")


# ---------------------------------------------------------------- k_small, Jacobi
def check_jacobi(name, G, R, out, seq):
    S, S2, vals, vals_host, status = out
    k = G.shape[0]
    ref = D.eigenvalues_50(name)
    tol, orth_tol = D.jacobi_tolerances(G, ref)
    e_val, e_res, e_orth = D.jacobi_errors(G, S[:k, :k], vals[:k], ref)
    print(f"k_small jacobi {name}: values {e_val:.3g}, residual {e_res:.3g} (bound {tol:.3g}), orthogonality {e_orth:.3g} (bound {orth_tol:.3g})")
    assert status == 0
    assert e_val <= tol and e_res <= tol and e_orth <= orth_tol
    assert np.all(np.diff(vals[:k]) <= 0)
    for M in (S, S2):
        assert not M[k:, :].any() and not M[:, k:].any() and np.all(np.isfinite(M))
    for j in range(k):
        if vals[j] > 0:
            want = S[:k, j] / math.sqrt(vals[j])
            assert np.all(np.abs(S2[:k, j] - want) <= 2 * np.spacing(np.abs(want))), j
        else:
            assert not S2[:, j].any(), j
    assert same_bits(vals_host[:k], vals[:k]) and vals_host[R] == seq
    return e_val, e_res, e_orth


@pytest.mark.parametrize("name", sorted(D.JACOBI_CASES))
def test_jacobi_against_50_digit_eigenvalues(name):
    R, k, G = D.JACOBI_CASES[name]
    out = small(one_partial(G, R), k, 1, seq=41.0)
    check_jacobi(name, G, R, out, 41.0)
    again = small(one_partial(G, R, fill=123.0), k, 1, seq=41.0)               # other padding, equal bits
    assert all(same_bits(a, b) for a, b in zip(out[:4], again[:4]))


def test_jacobi_sums_its_partials():
    """The same integer-valued G as one partial and as 256 partials that sum to it exactly: equal bits."""
    R, k, G = D.JACOBI_CASES["integer_k20"]
    _, parts = D.integer_spd(20, 9)
    one = small(one_partial(G, R), k, 1, seq=7.0)
    many = small(parts, k, 1, seq=7.0)
    assert all(same_bits(a, b) for a, b in zip(one[:4], many[:4]))
    check_jacobi("integer_k20", G, R, many, 7.0)


@pytest.mark.parametrize("power", D.SCALE_POWERS)
def test_jacobi_is_invariant_under_scaling_by_a_power_of_two(power):
    """G 2^+-600 on the well-conditioned 10 x 10 matrix (and 2^1021, where even the sum of the diagonal overflows, and
    2^-900): the eigenvalues are the unscaled run's times that power and the vectors the unscaled run's, bit for bit -- a
    power of two commutes with every operation of the rotations and with the stopping rule, which is taken on G scaled
    by the exponent of its largest diagonal entry.  (The rule on the squares of the entries themselves
    compared inf with inf, or 0 with 0, stopped before the first sweep and returned G's diagonal and the identity:
    eigenvalues off by 0.42 relative, with no status.)"""
    R, k, G = D.JACOBI_CASES[D.SCALE_CASE]
    S, _, vals, _, _ = small(one_partial(G, R), k, 1)
    Ss, _, vals_s, _, status = small(one_partial(np.ldexp(G, power), R), k, 1)
    assert status == 0
    assert same_bits(vals_s, np.ldexp(vals, power))
    assert same_bits(Ss, S)
    ref = D.eigenvalues_50(D.SCALE_CASE)
    tol, _ = D.jacobi_tolerances(G, ref)
    err = max(abs(float(np.ldexp(vals_s[i], -power)) - float(ref[i])) for i in range(k))
    print(f"k_small jacobi at 2^{power}: values {err:.3g} (bound {tol:.3g})")
    assert err <= tol


# ---------------------------------------------------------------- k_small, Cholesky
@pytest.mark.parametrize("name", sorted(D.CHOLESKY_CASES))
def test_cholesky_whitens_the_gram_matrix_as_well_as_numpy_does(name):
    R, k, N, cond = D.CHOLESKY_CASES[name]
    gp = gram(D.tall_block(name))
    S, _, vals, vals_host, status = small(gp, k, 0)
    G = D.sum_partials(gp)[:k, :k]                                            # the kernel's G, bit for bit
    assert status == 0
    assert np.all(np.isfinite(S)) and same_bits(S, np.triu(S)) and not S[k:, :].any() and not S[:, k:].any()
    want = 1.0 / np.diag(S)[:k]
    assert np.all(np.abs(vals[:k] - want) <= 2 * np.spacing(want))
    assert same_bits(vals_host[:k], vals[:k])
    bound = D.cholesky_diag_bound(G)                                          # (None at cond(G) 1e14: the theory promises nothing)
    assert (bound is None) == (name == D.TWO_PASS_CASE)
    err = D.cholesky_diag_error(vals[:k], G)
    print(f"k_small cholesky {name}: max|diag(U) - 50-digit diag| {err:.3g} (bound {bound})")
    assert bound is None or err <= bound
    got, base = D.whitening_error(G, S[:k, :k]), D.numpy_whitening_error(G)
    recorded = D.CHOLESKY_NUMPY_BASELINE[name]                                # what tests/test_svd_dense_cpu.py printed
    assert recorded / 4 <= base <= 4 * recorded, (base, recorded)             # the yardstick itself has not moved
    print(f"k_small cholesky {name}: max|t(S) G S - I| {got:.3g} (numpy {base:.3g}, bound {16 * base:.3g})")
    assert got <= 16 * base


def test_cholesky_qr_twice_on_the_cond_1e7_block():
    R, k, N, cond = D.CHOLESKY_CASES[D.TWO_PASS_CASE]
    A = D.tall_block(D.TWO_PASS_CASE)
    for _ in range(2):                                                        # orthonormalise(): gram, small, apply in place
        S, _, _, _, status = small(gram(A), k, 0)
        assert status == 0
        A = apply(A, S, in_place=True)
    assert not A[:, k:].any()
    err = D.max_err_vs_identity(*D.exact_matmul(A[:, :k].T, A[:, :k]))
    print(f"CholeskyQR2 at cond 1e7: max|t(A) A - I| {err:.3g} (bound 1e-13)")
    assert err <= 1e-13


def test_cholesky_reports_a_matrix_that_is_not_positive_definite():
    A, G = D.equal_columns_gram(8, 14)
    gp = gram(A)
    assert np.array_equal(gp.sum(axis=0), G)
    S, _, _, _, status = small(gp, 8, 0)
    assert status == 1 and same_bits(S, np.zeros((14, 14)))
    Gn = D.JACOBI_CASES["k13_in_R14"][2].copy()
    Gn[2, 5] = Gn[5, 2] = np.nan
    S, _, _, _, status = small(one_partial(Gn, 14), 13, 0)
    assert status == 1 and same_bits(S, np.zeros((14, 14)))


# ---------------------------------------------------------------- k_apply
@pytest.mark.parametrize("name", D.APPLY_S_CASES)
def test_apply_against_the_50_digit_product_in_and_out_of_place(name):
    """Every row is held to the exact product, read off in 50 digits, at N <= 257; at N = 5000 the rows of
    apply_check_rows are (the ends, both sides of the 256-row blocks' edges, a spread), and every row is within twice the
    bound of numpy's product, which obeys the bound itself.  In place and out of place agree on every bit of every row."""
    R, k, G = D.JACOBI_CASES[name]
    S = small(one_partial(G, R), k, 1)[0]
    assert not S[:, k:].any() and not S[k:, :].any()
    worst = 0.0
    for N in D.APPLY_N:
        A = D.apply_input(N, R)
        B = apply(A, S, in_place=False)
        assert same_bits(B, apply(A, S, in_place=True)), N
        assert np.all(np.isfinite(B)) and not B[:, k:].any()
        bound = D.apply_bound(A, S)
        assert np.all(np.abs(B - A @ S) <= 2 * bound), N                      # every row: numpy's product obeys the bound too
        rows = D.apply_check_rows(N)                                          # (every row up to N = 257)
        err = D.abs_err(B[rows], *D.exact_matmul(A[rows], S))
        assert np.all(err <= bound[rows]), N
        nz = bound[rows] > 0
        worst = max(worst, float(np.max(err[nz] / bound[rows][nz])))
    print(f"k_apply {name}: largest |B - exact| / (R 2^-53 sum |a||s|) = {worst:.3g} (bound 1)")


# ---------------------------------------------------------------- k_normal_init
@pytest.mark.parametrize("seed", D.NORMAL_SEEDS)
@pytest.mark.parametrize("nmaj,r,R", D.NORMAL_SHAPES)
def test_normal_block_element_by_element(nmaj, r, R, seed):
    from util_philox import normal_draws
    g = normal(nmaj, r, R, seed)
    want = normal_draws(nmaj, r, seed)
    err = float(np.max(np.abs(g[:, :r] - want)))
    print(f"k_normal_init {nmaj} x {r} in {R}, seed {seed}: largest difference {err:.3g} (bound 1e-12)")
    assert err <= 1e-12
    assert same_bits(g[:, r:], np.zeros((nmaj, R - r)))
    if (nmaj, r) == (5000, 40):
        import scipy.stats
        n = g.size
        assert abs(g.mean()) <= 5 / math.sqrt(n)
        assert abs(g.var() - 1.0) <= 5 * math.sqrt(2.0 / n)
        assert scipy.stats.kstest(g.ravel(), "norm").pvalue > 1e-3
        c = np.corrcoef(g.T)
        assert np.max(np.abs(c - np.diag(np.diag(c)))) <= 5 / math.sqrt(5000)


def test_normal_block_depends_on_both_halves_of_the_seed():
    a, b = normal(9, 3, 4, 5), normal(9, 3, 4, 5 + (1 << 32))
    assert not np.array_equal(a, b) and same_bits(a, normal(9, 3, 4, 5))
