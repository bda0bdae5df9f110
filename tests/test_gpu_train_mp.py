"""The training steps -- k_sweep / k_sweep1, k_update / k_update2 / k_prime, k_final / k_control and the ML twins k_ml_update /
k_ml_final -- and the sparse products (k_spmm) against 50-digit arithmetic (tests/util_mp_train.py), with no fp64 restatement
in between, at every padded rank the kernels are compiled for.

``with_rank`` instantiates 24 widths: 2, 4, .., 32 (one lane per task), 40..64 (two lanes share a task) and 80..128 (four);
each sweep exists packed and wide, pairs its entries on one reciprocal or not (``sweep_pairs``), keeps two row buffers or one.
Every width runs at r = R and at r = R - 1 (r = 1 at R = 2), where the padding column must stay inert, packed (integer counts)
and wide (the same counts times a per-cell factor), on ONE 28 x 200 matrix whose layouts -- read back from the library and
asserted, test by test -- hold a leading stretch of ones, a longer stretch of ones or twos, general entries behind it, slices
and tasks of an odd number of groups and of a single one (``assert_layout_conditions``).  Cut variants (task cap 8, pieces
merged and not) and value edges run at a few widths.

A STEP IS CHECKED AS A STEP: the reference of step 2 starts from the device's own state after step 1 (``get_state``), so
nothing compounds.  Bounds (derived in util_mp_train.py, never read off the device): the factors 1e-13 relative over ALL
components; lkh, lk and the four statistics |got - ref| <= 1e-13 (sum_abs + nterms) of the un-normalised sum.  The guards
(fudge, clamp, lw lh > 0) are asserted on the reference of every case; tests/test_train_mp_cpu.py holds the same cases'
fp64 oracles to the same bounds without a GPU, and prints the oracle's own error as the yardstick.  The sparse products with
integer operands have no tolerance: every product and partial sum is an exact double, so the result is the exact product
bit for bit in any order of summation.

Largest errors seen on the MI355X, per family and width, next to the oracle's: DESIGN.md section 6.
"""
import numpy as np
import pytest

import util_mp_train as T
from test_gpu_limits import make_engine

pytestmark = pytest.mark.gpu

MAXIMA = {}
FLAGS_OFF = (False,) * 4


@pytest.fixture(scope="module", autouse=True)
def _print_maxima():
    yield
    for fam, R in sorted(MAXIMA):
        print("largest over the file, %-22s R = %3d: factors %.3g, sums %.3g of (sum_abs + nterms)" % (fam, R, *MAXIMA[fam, R]))


def note(family, R, e_f, e_s):
    old = MAXIMA.get((family, R), (0.0, 0.0))
    MAXIMA[family, R] = (max(old[0], e_f), max(old[1], e_s))


def rank_cases():
    return [pytest.param(R, r, id=f"R{R}-r{r}") for R, r in T.RANKS]


def count_matrix(case, monkeypatch=None, cut=None):
    """The case's CountMatrix, its layouts' conditions asserted from the library's own export: the layout conditions of
    util_mp_train, or (``cut`` = merge on / off) the cut variant's geometry, which is then in force for the engines made."""
    import ccfindr_amd as C
    from ccfindr_amd.engine import padded_rank
    assert padded_rank(case.r) == case.R
    M = C.CountMatrix(case.X)
    if cut is None:
        T.assert_layout_conditions(M, case.r, case.layout)
    else:
        T.assert_cut(monkeypatch, M, case.R, cut)
    return M


def assert_vb_guards(case, ref):
    assert T.fudge_guard(ref, case.fudge) and np.all(ref["lw"] > 0.0) and np.all(ref["lh"] > 0.0), case.name


def check_vb(family, case, ref, state, lkh, stats=None, tag=""):
    """One step's results against its reference: the six factors, lkh, and (resident engine) the four statistics."""
    assert_vb_guards(case, ref)
    e_f, e_l = T.vb_errors(state, lkh, ref, case.nm)
    e_s = max(T.stats_errors(stats, ref)) if stats is not None else 0.0
    print(f"{case.name} {family} {tag}: factors %.3g, lkh %.3g, statistics %.3g of (sum_abs + nterms)" % (e_f, e_l, e_s))
    note(family, case.R, e_f, max(e_l, e_s))
    assert e_f <= T.FACTOR_BOUND, (case.name, family, tag, e_f)
    assert e_l <= T.SUM_BOUND and e_s <= T.SUM_BOUND, (case.name, family, tag, e_l, e_s)


def check_ml(family, case, ref, state, lks, tag=""):
    held, ratio = T.clamp_guard(ref, case.prior)
    assert held, (case.name, ratio)
    e_f = max(T.relerr(state["ew"], ref["ew"]), T.relerr(state["eh"], ref["eh"]))
    e_l = max(T.sum_error(lk, ref, "lk", case.nm) for lk in lks)
    print(f"{case.name} {family} {tag}: factors %.3g, lk %.3g of (sum_abs + nterms); clamp guard %.3g" % (e_f, e_l, ratio))
    note(family, case.R, e_f, e_l)
    assert e_f <= T.FACTOR_BOUND and e_l <= T.SUM_BOUND, (case.name, family, tag, e_f, e_l)


def resident_vb(family, case, eng, steps=2):
    """``steps`` host-stepped steps from the case's start; step 2's reference starts from the device's state after step 1
    -> that state."""
    eng.set_state(case.wh["lw"], case.wh["lh"], case.wh["eh"])
    start, first = None, None
    for t in range(steps):
        lkh, stats = eng.step(case.hyper, case.fudge)
        state = eng.get_state()
        check_vb(family, case, T.vb_reference(case, start), state, lkh, stats, tag=f"step {t + 1}")
        start = state
        first = first or state
    return first


def resident_ml(family, case, eng, steps=2):
    eng.ml_set_state(case.w, case.h)
    start, last = None, None
    for t in range(steps):
        lk = eng.ml_step(case.prior, case.ga, case.gb)
        again = eng.ml_likelihood()
        last = eng.ml_get_state()
        check_ml(family, case, T.ml_reference(case, start), last, (lk, again), tag=f"step {t + 1}")
        start = last
    return last


# ---- (a) VB, stateless -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", T.LAYOUTS)
@pytest.mark.parametrize("R,r", rank_cases())
def test_vb_stateless_every_width(R, r, layout):
    """``vbnmf_update``: one step, the six factors and lkh."""
    import ccfindr_amd as C
    case = T.vb_case(R, r, layout)
    got = C.vbnmf_update(case.X, case.wh, case.hyper, case.fudge)
    check_vb("vb stateless", case, T.vb_reference(case), got, got["lkh"])


# ---- (b) VB, resident --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", T.LAYOUTS)
@pytest.mark.parametrize("R,r", rank_cases())
def test_vb_resident_two_steps_every_width(R, r, layout):
    """``set_state`` and two ``step`` calls: both lkh, both sets of four statistics, the six factors after each."""
    import ccfindr_amd as C
    case = T.vb_case(R, r, layout)
    M = count_matrix(case)
    eng = C.VBEngine(M, r)
    try:
        resident_vb("vb resident", case, eng)
    finally:
        eng.close()
        M.close()


@pytest.mark.parametrize("pair", [True, False], ids=["one_launch", "two_launches"])
@pytest.mark.parametrize("layout", T.LAYOUTS)
@pytest.mark.parametrize("R", T.FORM_WIDTHS)
def test_vb_resident_under_each_update_form(monkeypatch, R, layout, pair):
    """k_update2 (VBNMF_UPDATE_PAIR=1: colSums(ew) from the sweep's column sums) and k_update twice (VBNMF_NO_UPDATE_PAIR=1)."""
    case = T.vb_case(R, R, layout)
    M = count_matrix(case)
    eng = make_engine(monkeypatch, M, R, pair=pair)
    try:
        resident_vb("vb one launch" if pair else "vb two launches", case, eng)
    finally:
        eng.close()
        M.close()


# ---- (c) VB, device loop -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", [True, False], ids=["fold", "separate_control"])
@pytest.mark.parametrize("layout", T.LAYOUTS)
@pytest.mark.parametrize("R", T.LOOP_WIDTHS)
def test_vb_device_loop_two_steps(monkeypatch, R, layout, fold):
    """``run(Itmax=2, Tol=0)`` with the hyper-parameter updates off and n0 past the end: the history's lkh and statistics
    against the two step references, the second from a host-stepped engine's state after one step; the state left behind
    against the second."""
    case = T.vb_case(R, R, layout)
    M = count_matrix(case)
    host = make_engine(monkeypatch, M, R, fold=fold)
    loop = make_engine(monkeypatch, M, R, fold=fold)
    try:
        host.set_state(case.wh["lw"], case.wh["lh"], case.wh["eh"])
        host.step(case.hyper, case.fudge)
        after_one = host.get_state()
        loop.set_state(case.wh["lw"], case.wh["lh"], case.wh["eh"])
        out = loop.run(case.hyper, Itmax=2, Tol=0.0, n0=10, dn=1, flags=FLAGS_OFF, fudge=case.fudge, history=True)
        left = loop.get_state()
    finally:
        host.close()
        loop.close()
        M.close()
    assert out["it"] == 2 and out["reason"] == 4 and out["history"].shape == (2, 9) and out["hyper"] == case.hyper
    refs = (T.vb_reference(case), T.vb_reference(case, after_one))
    family = "vb loop fold" if fold else "vb loop control"
    for t, ref in enumerate(refs):
        assert_vb_guards(case, ref)
        e_l = T.sum_error(out["history"][t, 0], ref, "lkh", case.nm)
        e_s = max(T.stats_errors(out["history"][t, 1:5], ref))
        print(f"{case.name} {family} step {t + 1}: lkh %.3g, statistics %.3g of (sum_abs + nterms)" % (e_l, e_s))
        note(family, R, 0.0, max(e_l, e_s))
        assert e_l <= T.SUM_BOUND and e_s <= T.SUM_BOUND, (case.name, t, e_l, e_s)
    assert out["lkh"] == out["history"][1, 0]
    e_f = max(T.relerr(left[k], refs[1][k]) for k in T.FACT)
    note(family, R, e_f, 0.0)
    assert e_f <= T.FACTOR_BOUND, (case.name, e_f)


# ---- (d) ML ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", T.LAYOUTS)
@pytest.mark.parametrize("R,r", rank_cases())
def test_ml_stateless_every_width(R, r, layout):
    """``nmf_update``: one step, both factors and the likelihood of the updated pair."""
    import ccfindr_amd as C
    case = T.ml_case(R, r, layout)
    got = C.nmf_update(case.X, case.w, case.h, prior=case.prior, gamma_a=case.ga, gamma_b=case.gb)
    check_ml("ml stateless", case, T.ml_reference(case), got, (got["lk"],))


@pytest.mark.parametrize("layout", T.LAYOUTS)
@pytest.mark.parametrize("R,r", rank_cases())
def test_ml_resident_two_steps_every_width(R, r, layout):
    """``ml_set_state`` / ``ml_step`` / ``ml_likelihood``, two steps, the second from the device's own pair."""
    import ccfindr_amd as C
    case = T.ml_case(R, r, layout)
    M = count_matrix(case)
    eng = C.VBEngine(M, r)
    try:
        resident_ml("ml resident", case, eng)
    finally:
        eng.close()
        M.close()


# ---- (e) edge sets and cut variants --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge", list(T.EDGES_VB))
@pytest.mark.parametrize("R", T.EDGE_WIDTHS)
def test_vb_edge_sets(R, edge):
    """The hyper-parameter sets of tests/util_mp_step.py's CASES with their fudge; (0.05, 2) on both sides -- psi = -20.6 --
    for one step; fudge 0 (no lw, lh is 0: the reference shows it) and the fudge that clips (the floor is met, not everywhere)."""
    import ccfindr_amd as C
    case = T.vb_case(R, R, "packed", edge)
    M = count_matrix(case)
    eng = C.VBEngine(M, R)
    try:
        first = resident_vb("vb edges", case, eng, steps=case.steps)
    finally:
        eng.close()
        M.close()
    if edge in T.CLIPPING:
        assert (first["lw"] == case.fudge).any() and (first["lw"] > case.fudge).any()


@pytest.mark.parametrize("edge", list(T.EDGES_ML))
@pytest.mark.parametrize("R", T.EDGE_WIDTHS)
def test_ml_edge_sets(R, edge):
    """No prior; the prior (1.7, 0.6); the prior (0.5, 1.0), where up + gamma.a - 1 goes negative and the eps clamp is met."""
    import ccfindr_amd as C
    case = T.ml_case(R, R, "packed", edge)
    M = count_matrix(case)
    eng = C.VBEngine(M, R)
    try:
        last = resident_ml("ml edges", case, eng)
    finally:
        eng.close()
        M.close()
    if edge == "prior_clamp":
        for k in ("ew", "eh"):
            assert (last[k] == T.EPS).any() and (last[k] > T.EPS).any(), k


@pytest.mark.parametrize("merge", [True, False], ids=["merge", "no_merge"])
@pytest.mark.parametrize("layout", T.LAYOUTS)
@pytest.mark.parametrize("R", T.CUT_WIDTHS)
def test_cut_variants(monkeypatch, R, layout, merge):
    """Task cap 8: every (major, block) pair of more than 8 entries is cut, the pieces merged in the wave (ranks <= 32) or
    summed by the updates.  Two VB steps, two ML steps and both exact sparse products under that geometry."""
    import ccfindr_amd as C
    case, mcase = T.vb_case(R, R, layout), T.ml_case(R, R, layout)
    M = count_matrix(case, monkeypatch, cut=merge)
    eng = C.VBEngine(M, R)
    try:
        resident_vb("vb cut", case, eng)
        resident_ml("ml cut", mcase, eng)
    finally:
        eng.close()
        M.close()
    Xq = T.matrix(layout, True)
    Mq = C.CountMatrix(Xq)
    T.assert_cut(monkeypatch, Mq, R, merge)
    eng = C.VBEngine(Mq, R)
    try:
        check_spmm_exact(eng, Xq, R, seed=7000 + R)
    finally:
        eng.close()
        Mq.close()


# ---- (f) sparse products, exactly ------------------------------------------------------------------------------------------------
def check_spmm_exact(eng, X, r, seed):
    B, W = T.spmm_operands(r, seed)
    want_xb, want_wx = T.spmm_exact(X, B, W)
    for which, got, want in (("X B'", eng.spmm(B), want_xb), ("W' X", eng.spmm(W, transpose=True), want_wx)):
        assert got.shape == want.shape
        assert np.array_equal(got, want), (which, r, int(np.count_nonzero(got != want)), float(np.max(np.abs(got - want))))
        # an accumulator starts at +0, x + (-x) = +0 in round-to-nearest and +0 + -0 = +0: no zero of the result is negative
        assert not np.signbit(got[want == 0]).any(), which
    assert (want_xb == 0).any()


@pytest.mark.parametrize("layout", T.LAYOUTS)
@pytest.mark.parametrize("R,r", rank_cases())
def test_sparse_products_bit_for_bit_every_width(R, r, layout):
    """Integer operands -8 .. 8 with zeros and an all-zero row; the wide matrix scaled by multiples of 1 / 4."""
    import ccfindr_amd as C
    X = T.matrix(layout, True)
    M = C.CountMatrix(X)
    T.assert_layout_conditions(M, r, layout)
    eng = C.VBEngine(M, r)
    try:
        check_spmm_exact(eng, X, r, seed=5000 + 10 * R + (R - r))
    finally:
        eng.close()
        M.close()


@pytest.mark.parametrize("layout", T.LAYOUTS)
@pytest.mark.parametrize("R", T.REAL_SPMM_WIDTHS)
def test_sparse_products_componentwise_with_real_operands(R, layout):
    """Normal operands: |got - exact| <= (len + 8) u (|X| |B|), len the stored entries of the result's row (column), u = 2^-53,
    exact from math.fsum over the error-free products."""
    import ccfindr_amd as C
    X = T.matrix(layout)
    rng = np.random.default_rng(9000 + R)
    B, W = rng.standard_normal((R, T.N_CELLS)), rng.standard_normal((T.N_GENES, R))
    (xb, xb_abs, row_len), (wx, wx_abs, col_len) = T.spmm_real(X, B, W)
    M = C.CountMatrix(X)
    eng = C.VBEngine(M, R)
    try:
        got_xb, got_wx = eng.spmm(B), eng.spmm(W, transpose=True)
    finally:
        eng.close()
        M.close()
    worst = 0.0
    for got, want, scale, length in ((got_xb, xb, xb_abs, row_len[:, None]), (got_wx, wx, wx_abs, col_len[None, :])):
        bound = (length + 8) * T.U * scale
        assert np.all(bound > 0)
        worst = max(worst, float(np.max(np.abs(got - want) / bound)))
    print(f"k_spmm R={R} {layout}: largest |got - exact| / ((len + 8) u |X||B|) = %.3g" % worst)
    note("spmm real (of bound)", R, worst, 0.0)
    assert worst <= 1.0
