"""No GPU: the models and references of tests/util_svd_dense.py, on every input tests/test_gpu_svd_dense.py hands the dense
kernels of the truncated SVD (csrc/init.h).  A numpy / plain-Python evaluation of each operation must sit inside every
bound the GPU test holds the kernel to -- the inputs are then known to be passable before a GPU sees them -- and the
Jacobi model never needs more than 20 of the kernel's 30 sweeps, so the cap is never what ends a case.  The figures are
printed (run with -s): the Cholesky ones are the baseline the GPU test's docstring records."""
import math

import numpy as np
import pytest

import util_svd_dense as D
from util_svd_dense import U


def test_exact_arithmetic_is_exact():
    rng = np.random.default_rng(1)
    A = rng.standard_normal((7, 5)) * np.logspace(-9, 9, 5)[None, :]
    A[2, 3] = 0.0
    ints, e = D.to_fixed(A)
    for (i, j), v in np.ndenumerate(A):
        assert float(D.mp.ldexp(D.mp.mpf(int(ints[i, j])), e)) == v
    B = rng.integers(-1000, 1000, size=(5, 4)).astype(np.float64)
    Ai = rng.integers(-1000, 1000, size=(6, 5)).astype(np.float64)
    P, e = D.exact_matmul(Ai, B)
    assert np.array_equal(np.array([[float(D.mp.ldexp(D.mp.mpf(int(v)), e)) for v in row] for row in P]), Ai @ B)
    assert np.max(D.abs_err(Ai @ B, P, e)) == 0.0
    # a sum that fp64 gets wrong: 1 + 2^-60 - 1
    P, e = D.exact_matmul(np.array([[1.0, 2.0 ** -60, -1.0]]), np.ones((3, 1)))
    assert D.abs_err(np.array([[0.0]]), P, e)[0, 0] == 2.0 ** -60


def test_gram_row_split_covers_every_row_once():
    for N in D.GRAM_N:
        edges = [D.gram_rows_of_block(N, b) for b in range(D.GRAM_BLOCKS)]
        covered = np.zeros(N, dtype=int)
        for n0, n1 in edges:
            covered[n0:n1] += 1
        assert np.all(covered == 1), N


@pytest.mark.parametrize("R", D.WIDTHS)
def test_gram_integer_inputs_are_exact_in_fp64(R):
    for N in D.GRAM_N:
        A = D.gram_integer_input(N, R, seed=3)
        Ai = A.astype(np.int64)
        want = Ai.T @ Ai
        assert np.max(np.abs(Ai)) <= 1024 and np.max(np.abs(Ai).T @ np.abs(Ai)) < 2 ** 53
        assert np.array_equal(D.sum_partials(D.blockwise_gram(A)).astype(np.int64), want)


def test_gram_real_inputs_numpy_within_the_any_order_bound():
    assert set(D.GRAM_REAL_CASES) == {(N, R) for N in D.GRAM_N for R in D.WIDTHS}
    for R in D.WIDTHS:
        pairs = D.gram_sample_pairs(R)
        assert all(0 <= i < R and 0 <= j < R for i, j in pairs) and len(set(pairs)) == len(pairs)
        if R > 32:                                              # an entry of each of the four thread tiles, and their inner corners
            assert {(0, 0), (0, R - 1), (R - 1, 0), (R - 1, R - 1), (31, 32), (32, 31), (32, 32), (31, 31)} <= set(pairs)
    worst = 0.0
    for N, R in D.GRAM_REAL_CASES:
        A = D.gram_real_input(N, R, seed=4)
        if R > 2:
            assert np.ptp(np.log10(np.max(np.abs(A), axis=0))) > 9            # the column scales do span 1e-6 .. 1e6
        G = D.sum_partials(D.blockwise_gram(A))
        pairs = D.gram_sample_pairs(R)
        bound = D.gram_bound(A)
        err = D.gram_sample_errors(G, A, pairs)
        ratio = float(np.max(err / np.array([bound[i, j] for i, j in pairs])))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (N, R, ratio)
    # the sampled reference is the full one: every entry of a small case, both ways
    A = D.gram_real_input(33, 14, seed=4)
    G = D.sum_partials(D.blockwise_gram(A))
    every = [(i, j) for i in range(14) for j in range(14)]
    assert np.array_equal(D.gram_sample_errors(G, A, every).reshape(14, 14), D.abs_err(G, *D.exact_matmul(A.T, A)))
    print(f"gram, numpy blockwise: largest sampled error / bound = {worst:.3g}")


@pytest.mark.parametrize("name", sorted(D.JACOBI_CASES))
def test_jacobi_model_within_the_bounds(name):
    R, k, G = D.JACOBI_CASES[name]
    assert G.shape == (k, k) and k <= R and np.array_equal(G, G.T)
    S, vals, S2, sweeps = D.jacobi_model(G)
    ref = D.eigenvalues_50(name)
    tol, orth_tol = D.jacobi_tolerances(G, ref)
    e_val, e_res, e_orth = D.jacobi_errors(G, S, vals, ref)
    print(f"jacobi model {name}: sweeps {sweeps}, values {e_val:.3g}, residual {e_res:.3g} (tol {tol:.3g}), orthogonality {e_orth:.3g} (tol {orth_tol:.3g})")
    assert sweeps <= 20
    assert e_val <= tol and e_res <= tol and e_orth <= orth_tol
    assert np.all(np.diff(vals) <= 0)
    for j in range(k):
        if vals[j] > 0:
            assert np.array_equal(S2[:, j], S[:, j] / math.sqrt(vals[j]))
        else:
            assert not S2[:, j].any()


def test_jacobi_cases_are_what_they_say():
    ev = lambda name: np.array([float(v) for v in D.eigenvalues_50(name)])
    e = ev("repeated_k40")
    assert np.allclose(e, np.sort(np.tile([5.0, 2.0, 2.0, 1.0], 10))[::-1], atol=1e-13)
    e = ev("clustered_k64")
    assert e[0] - e[-1] < 1e-7 and e[0] - e[-1] > 5e-8
    e = ev("rank_deficient_k24")
    assert np.all(np.abs(e[12:]) < 1e-15) and e[11] > 5e-7
    e = ev("graded_1e-12_k64")
    assert e[0] / e[-1] > 5e11
    G, parts = D.integer_spd(20, 9)
    assert np.array_equal(G, D.JACOBI_CASES["integer_k20"][2]) and np.array_equal(D.sum_partials(parts), G)
    e = ev(D.SCALE_CASE)
    assert e[0] / e[-1] < 2.5


@pytest.mark.parametrize("power", D.SCALE_POWERS)
def test_jacobi_stopping_rule_is_scale_free(power):
    """G 2^+-600 (and 2^1021, where even the sum of the diagonal overflows, and 2^-900): every operation of the rotation, and
    the stopping rule on G scaled by the exponent of its largest diagonal entry, commute with a power of two.  The rule on
    the squares of the entries themselves (off <= 1e-30 tr^2) saw inf <= inf or 0 <= 0 before the first sweep and returned
    the diagonal of G with the identity."""
    R, k, G = D.JACOBI_CASES[D.SCALE_CASE]
    S, vals, _, sweeps = D.jacobi_model(G)
    Gs = np.ldexp(G, power)
    Ss, vals_s, _, sweeps_s = D.jacobi_model(Gs)
    assert sweeps_s == sweeps and np.array_equal(Ss, S) and np.array_equal(vals_s, np.ldexp(vals, power))
    ref = D.eigenvalues_50(D.SCALE_CASE)
    tol, _ = D.jacobi_tolerances(G, ref)
    assert max(abs(float(np.ldexp(vals_s[i], -power)) - float(ref[i])) for i in range(k)) <= tol
    # the rule before the fix, on the same input: no sweep, and "eigenvalues" that are G's diagonal
    So, vals_o, _, sweeps_o = D.jacobi_model(Gs, scale_free=False)
    assert sweeps_o == 0 and np.array_equal(np.sort(vals_o), np.sort(np.diag(Gs)))
    assert set(np.unique(So)) == {0.0, 1.0} and np.array_equal(So.sum(axis=0), np.ones(k)) and np.array_equal(So.sum(axis=1), np.ones(k))
    rel = np.max(np.abs(np.ldexp(vals_o, -power) - np.array([float(v) for v in ref])) / np.array([float(v) for v in ref]))
    print(f"old stopping rule at 2^{power}: sweeps {sweeps_o}, relative eigenvalue error {rel:.3g}")
    assert rel > 0.1


def test_jacobi_model_all_zero_matrix_stops_at_once():
    S, vals, S2, sweeps = D.jacobi_model(np.zeros((5, 5)))
    assert sweeps == 0 and not vals.any() and np.array_equal(S, np.eye(5)) and not S2.any()


@pytest.mark.parametrize("name", sorted(D.CHOLESKY_CASES))
def test_cholesky_model_against_numpy(name):
    R, k, N, cond = D.CHOLESKY_CASES[name]
    A = D.tall_block(name)
    sv = np.linalg.svd(A[:, :k], compute_uv=False)
    assert abs(sv[0] / sv[-1] / cond - 1) < 1e-6 and not A[:, k:].any()
    G = (A.T @ A)[:k, :k]
    status, S, diag = D.cholesky_model(G)
    assert status == 0
    assert np.array_equal(S, np.triu(S))
    got, base = D.whitening_error(G, S), D.numpy_whitening_error(G)
    print(f"cholesky {name}: max|t(S) G S - I| model {got:.3g}, numpy {base:.3g}")
    assert got <= 16 * base
    recorded = D.CHOLESKY_NUMPY_BASELINE[name]
    assert recorded / 4 <= base <= 4 * recorded, (base, recorded)
    assert np.max(np.abs(1.0 / np.diag(S) / diag - 1)) <= 4 * U
    # the factor's diagonal against the 50-digit Cholesky factor of the same fp64 G, where the theory gives a bound
    bound = D.cholesky_diag_bound(G)
    assert (bound is None) == (name == D.TWO_PASS_CASE)                # cond(G) 1e14: cond * eps > 1/2, no promise
    err = D.cholesky_diag_error(diag, G)
    print(f"cholesky {name}: max|diag(U) - 50-digit diag| model {err:.3g}, bound {bound}")
    assert bound is None or err <= bound


def test_cholesky_qr_twice_restores_orthogonality():
    R, k, N, cond = D.CHOLESKY_CASES[D.TWO_PASS_CASE]
    A = D.tall_block(D.TWO_PASS_CASE)[:, :k]
    for _ in range(2):
        status, S, _ = D.cholesky_model(A.T @ A)
        assert status == 0
        A = A @ S
    err = D.max_err_vs_identity(*D.exact_matmul(A.T, A))
    print(f"two passes at cond 1e7: max|t(A) A - I| = {err:.3g}")
    assert err <= 1e-13


def test_cholesky_model_failure_side():
    A, G = D.equal_columns_gram(8, 14)
    assert np.array_equal(A[:, 0], A[:, 1]) and np.array_equal(A, np.round(A))
    status, S, _ = D.cholesky_model(G[:8, :8])
    assert status == 1 and not S.any()
    Gn = D.JACOBI_CASES["k13_in_R14"][2].copy()
    Gn[2, 5] = Gn[5, 2] = np.nan
    status, S, _ = D.cholesky_model(Gn)
    assert status == 1 and not S.any()


def test_apply_numpy_within_the_any_order_bound():
    worst = 0.0
    for name in D.APPLY_S_CASES:
        R, k, G = D.JACOBI_CASES[name]
        S = D.pad_square(D.jacobi_model(G)[0], R)
        for N in D.APPLY_N:
            A = D.apply_input(N, R)
            rows = D.apply_check_rows(N)
            assert rows[0] == 0 and rows[-1] == N - 1
            B = A @ S
            err = D.abs_err(B[rows], *D.exact_matmul(A[rows], S))
            bound = D.apply_bound(A[rows], S)
            ok = err <= bound
            assert ok.all(), (name, N)
            assert not B[:, k:].any()
            worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))
    print(f"apply, numpy: largest error / bound = {worst:.3g}")


def normal_block_statistics(g):
    """(|mean| sqrt(n), |var - 1| / sqrt(2 / n), KS p-value, largest |column correlation| sqrt(rows))."""
    import scipy.stats
    n = g.size
    c = np.corrcoef(g.T)
    off = np.max(np.abs(c - np.diag(np.diag(c))))
    return (abs(g.mean()) * math.sqrt(n), abs(g.var() - 1.0) / math.sqrt(2.0 / n), scipy.stats.kstest(g.ravel(), "norm").pvalue,
            off * math.sqrt(g.shape[0]))


def test_normal_draws_model():
    from util_philox import normal_draws, philox4x32, u53
    # element by element against a scalar restatement of the keying
    seed = D.NORMAL_SEEDS[1]
    g = normal_draws(5, 3, seed)
    for M in range(5):
        for k in range(3):
            el = M * 3 + k
            q = philox4x32([el & 0xFFFFFFFF], [el >> 32], [7], [0], seed & 0xFFFFFFFF, seed >> 32)
            want = math.sqrt(-2.0 * math.log(float(u53(q[0], q[1])[0]))) * math.cos(6.283185307179586476925 * float(u53(q[2], q[3])[0]))
            assert abs(g[M, k] - want) <= 1e-15 * max(1.0, abs(want))
    assert not np.array_equal(normal_draws(4, 2, D.NORMAL_SEEDS[0]), normal_draws(4, 2, D.NORMAL_SEEDS[0] + (1 << 32)))
    for seed in D.NORMAL_SEEDS:
        mean, var, p, corr = normal_block_statistics(normal_draws(5000, 40, seed))
        print(f"normal block, seed {seed}: mean {mean:.2f} sigma, variance {var:.2f} sigma, KS p {p:.3g}, correlation {corr:.2f} sigma")
        assert mean <= 5 and var <= 5 and p > 1e-3 and corr <= 5


def test_hooks_refuse_bad_arguments_before_they_look_for_a_device():
    import ctypes
    from ccfindr_amd import _native as N
    L = N.load()
    a = np.zeros(64 * 64 + 8)
    st = np.zeros(1, dtype=np.int32)
    p, sp = N.dptr(a), st.ctypes.data_as(N.c_int32_p)
    bad = N.ERR_BAD_ARG
    assert L.vbnmf_test_svd_gram(5, 1, p, p) == bad                     # no such width
    assert L.vbnmf_test_svd_gram(72, 1, p, p) == bad
    assert L.vbnmf_test_svd_gram(4, 0, p, p) == bad
    assert L.vbnmf_test_svd_gram(4, 1, None, p) == bad
    assert L.vbnmf_test_svd_small(4, 5, 1, 1, p, 0.0, p, p, p, p, sp) == bad        # k > R
    assert L.vbnmf_test_svd_small(4, 0, 1, 1, p, 0.0, p, p, p, p, sp) == bad
    assert L.vbnmf_test_svd_small(4, 2, 2, 1, p, 0.0, p, p, p, p, sp) == bad        # no such mode
    assert L.vbnmf_test_svd_small(4, 2, 1, 0, p, 0.0, p, p, p, p, sp) == bad        # no partial
    assert L.vbnmf_test_svd_small(3, 2, 1, 1, p, 0.0, p, p, p, p, sp) == bad
    assert L.vbnmf_test_svd_small(4, 2, 1, 1, p, 0.0, p, p, p, p, None) == bad
    assert L.vbnmf_test_svd_apply(4, 0, p, p, 0, p) == bad
    assert L.vbnmf_test_svd_apply(7, 1, p, p, 0, p) == bad
    assert L.vbnmf_test_svd_apply(4, 1, p, None, 1, p) == bad
    assert L.vbnmf_test_svd_normal(1, 3, 2, ctypes.c_uint64(1), p) == bad          # r > R
    assert L.vbnmf_test_svd_normal(0, 1, 2, ctypes.c_uint64(1), p) == bad
    assert L.vbnmf_test_svd_normal(1, 1, 3, ctypes.c_uint64(1), p) == bad
    assert L.vbnmf_test_svd_normal(1, 1, 2, ctypes.c_uint64(1), None) == bad
    if L.vbnmf_device_count() == 0:                                    # a good call, no GPU: a status, not a crash
        assert L.vbnmf_test_svd_normal(1, 1, 2, ctypes.c_uint64(1), p) == N.ERR_NO_DEVICE
