"""The stored-entry 50-digit steps (tests/util_mp_train.py) against the dense 50-digit steps (tests/util_mp_step.py), and the
committed fp64 oracles against them on every case tests/test_gpu_train_mp.py runs -- so the reference and the bounds the
kernels are held to are themselves proven without a GPU, and the oracle's own error on each case is on record as the
yardstick for the device's.

The layout conditions and the guards need no device -- the layout export is host code -- so they are asserted here as well
as in the GPU file: every width, both layouts, and the cut variants.

Bounds: those of the GPU file (derived in util_mp_train.py): factors 1e-13 relative over all components; lkh, lk and the four
statistics 1e-13 (sum_abs + nterms) of the un-normalised sum.
"""
import numpy as np
import pytest

import util_mp_step as S
import util_mp_train as T

ORACLE_MAX = {}


@pytest.fixture(scope="module", autouse=True)
def _print_maxima():
    yield
    for k in sorted(ORACLE_MAX):
        print("fp64 oracle, largest over the file, %-4s R = %3d: factors %.3g, sum %.3g of (sum_abs + nterms)" % (*k, *ORACLE_MAX[k]))


def note(kind, R, e_f, e_s):
    old = ORACLE_MAX.get((kind, R), (0.0, 0.0))
    ORACLE_MAX[kind, R] = (max(old[0], e_f), max(old[1], e_s))


# ---- the stored-entry steps are the dense steps ----------------------------------------------------------------------------------
@pytest.mark.parametrize("noninteger", [False, True])
@pytest.mark.parametrize("case", S.CASES, ids=[f"n{c[0]}m{c[1]}r{c[2]}" for c in S.CASES])
def test_sparse_vb_step_is_the_dense_step(case, noninteger):
    """Every output to 1e-40: lkh as 50-digit numbers; the six factors as doubles rounded from 50 digits, which two values
    that agree to 1e-40 round alike (unless one lies within 1e-40 of a rounding boundary), so they must be EQUAL."""
    n, m, r, lam, hyper, fudge, seed = case
    X, wh = S.make_case(n, m, r, lam, hyper, fudge, seed, noninteger)
    want = S.step(X, wh, hyper, fudge)
    got = T.vb_step(n, m, T.entries_of(X), wh["lw"], wh["lh"], wh["eh"], hyper, fudge)
    for k in T.FACT:
        assert np.array_equal(got[k], want[k]), k
    assert abs(got["lkh"] / want["lkh"] - 1) <= 1e-40
    # the four statistics: exact values of the rounded factors' sums, to the doubles' own rounding
    for q, a in enumerate((np.log(want["lw"]), np.log(want["lh"]), want["ew"], want["eh"])):
        assert abs(float(got["stats"][q]) - a.mean()) <= 1e-13 * (np.abs(a).mean() + 1.0), q
    assert got["lkh_abs"] >= abs(got["lkh"]) * n * m and got["lkh_n"] == 4 * np.count_nonzero(X) + r + 5 * r * (n + m)


@pytest.mark.parametrize("prior", [False, True])
@pytest.mark.parametrize("n,m,r,seed", [(7, 9, 3, 1), (12, 6, 2, 2), (5, 14, 4, 3)])
def test_sparse_ml_step_is_the_dense_step(n, m, r, seed, prior):
    """The shapes of tests/test_gpu_mpmath.py::test_ml_engine_against_50_digit_step."""
    rng = np.random.default_rng(seed)
    X, _ = S.make_case(n, m, r, 1.1, {"aw": 1.0, "bw": 1.0, "ah": 1.0, "bh": 1.0}, 0.0, seed, noninteger=bool(seed % 2))
    w, h = rng.uniform(0.05, 1.0, size=(n, r)), rng.uniform(0.05, 1.0, size=(r, m))
    ew, eh, lk = S.ml_step(X, w, h, prior, 1.7, 0.6)
    got = T.ml_step(n, m, T.entries_of(X), w, h, prior, 1.7, 0.6)
    assert np.array_equal(got["ew"], ew) and np.array_equal(got["eh"], eh)
    assert abs(got["lk"] / lk - 1) <= 1e-40
    assert got["lk_n"] == 3 * np.count_nonzero(X) + r


# ---- the fp64 oracles on every case of the GPU file -------------------------------------------------------------------------------
def check_vb_oracle(case):
    from oracle import vbnmf_oracle as O
    ref = T.vb_reference(case)
    got = O.update_dense(case.X, case.wh, case.hyper, case.fudge)
    e_f, e_l = T.vb_errors(got, got["lkh"], ref, case.nm)
    stats = (np.mean(np.log(got["lw"])), np.mean(np.log(got["lh"])), np.mean(got["ew"]), np.mean(got["eh"]))
    e_s = max(T.stats_errors(stats, ref))
    print(f"{case.name}: oracle factors %.3g, lkh %.3g, statistics %.3g of (sum_abs + nterms)" % (e_f, e_l, e_s))
    note("vb", case.R, e_f, max(e_l, e_s))
    assert T.fudge_guard(ref, case.fudge) and np.all(ref["lw"] > 0.0) and np.all(ref["lh"] > 0.0)
    assert e_f <= T.FACTOR_BOUND and e_l <= T.SUM_BOUND and e_s <= T.SUM_BOUND
    return ref


def check_ml_oracle(case):
    from oracle import mlnmf_oracle as OM
    ref = T.ml_reference(case)
    got = OM.nmf_update_literal(case.X, case.w, case.h, case.prior, case.ga, case.gb)
    lk = OM.likelihood_literal(case.X, got["ew"], got["eh"])
    e_f, e_l = T.ml_errors(got, lk, ref, case.nm)
    held, ratio = T.clamp_guard(ref, case.prior)
    print(f"{case.name}: oracle factors %.3g, lk %.3g of (sum_abs + nterms); clamp guard %.3g" % (e_f, e_l, ratio))
    note("ml", case.R, e_f, e_l)
    assert held
    assert e_f <= T.FACTOR_BOUND and e_l <= T.SUM_BOUND
    return ref


@pytest.mark.parametrize("layout", T.LAYOUTS)
@pytest.mark.parametrize("R,r", T.RANKS, ids=[f"R{R}-r{r}" for R, r in T.RANKS])
def test_vb_oracle_within_the_bounds_at_every_width(R, r, layout):
    from ccfindr_amd.engine import padded_rank
    assert padded_rank(r) == R
    check_vb_oracle(T.vb_case(R, r, layout))


@pytest.mark.parametrize("layout", T.LAYOUTS)
@pytest.mark.parametrize("R,r", T.RANKS, ids=[f"R{R}-r{r}" for R, r in T.RANKS])
def test_ml_oracle_within_the_bounds_at_every_width(R, r, layout):
    check_ml_oracle(T.ml_case(R, r, layout))


@pytest.mark.parametrize("edge", list(T.EDGES_VB))
@pytest.mark.parametrize("R", T.EDGE_WIDTHS)
def test_vb_oracle_within_the_bounds_on_the_edge_sets(R, edge):
    case = T.vb_case(R, R, "packed", edge)
    ref = check_vb_oracle(case)
    if edge in T.CLIPPING:                                   # the fudge that clips: it does, and not everywhere
        for k in ("lw", "lh"):
            print(case.name, k, "floored:", int((ref[k] == case.fudge).sum()), "of", ref[k].size)
        assert (ref["lw"] == case.fudge).any() and (ref["lw"] > case.fudge).any()
    if edge in ("case1", "far"):                             # psi far negative
        assert case.hyper["aw"] == 0.05


@pytest.mark.parametrize("edge", list(T.EDGES_ML))
@pytest.mark.parametrize("R", T.EDGE_WIDTHS)
def test_ml_oracle_within_the_bounds_on_the_edge_sets(R, edge):
    case = T.ml_case(R, R, "packed", edge)
    ref = check_ml_oracle(case)
    if edge == "prior_clamp":                                # the eps clamp is met, and not everywhere, in both factors
        for k in ("ew", "eh"):
            assert (ref[k] == T.EPS).any() and (ref[k] > T.EPS).any(), k


# ---- the layouts hold what the sweep's trip modes need ----------------------------------------------------------------------------
def test_the_widths_are_the_padded_ranks():
    from ccfindr_amd.engine import padded_rank
    assert sorted({padded_rank(r) for r in range(1, 129)}) == T.WIDTHS and len(T.WIDTHS) == 24
    for R, r in T.RANKS:
        assert padded_rank(r) == R


@pytest.mark.parametrize("layout", T.LAYOUTS)
@pytest.mark.parametrize("R,r", T.RANKS, ids=[f"R{R}-r{r}" for R, r in T.RANKS])
def test_layout_conditions_at_every_width(R, r, layout):
    import ccfindr_amd as C
    M = C.CountMatrix(T.matrix(layout))
    try:
        c = T.assert_layout_conditions(M, r, layout)
    finally:
        M.close()
    print(R, r, layout, c)


def test_layout_conditions_of_the_quarter_scaled_matrix():
    import ccfindr_amd as C
    M = C.CountMatrix(T.matrix("wide", True))
    try:
        for R in (2, 32, 40, 128):
            T.assert_layout_conditions(M, R, "wide")
    finally:
        M.close()


@pytest.mark.parametrize("merge", [True, False], ids=["merge", "no_merge"])
@pytest.mark.parametrize("R", T.CUT_WIDTHS)
def test_cut_variants_cut(monkeypatch, R, merge):
    import ccfindr_amd as C
    for layout in T.LAYOUTS:
        M = C.CountMatrix(T.matrix(layout))
        try:
            T.assert_cut(monkeypatch, M, R, merge)
        finally:
            M.close()
