"""The 50-digit statements of the two projection loops (tests/util_mp_project.py) against the numpy restatements
(tests/util_project.py, tests/util_vb_project.py), which tests/test_project_cpu.py and tests/test_vb_project_cpu.py tie to the
committed oracle -- so the reference tests/test_gpu_project_mp.py holds the kernels to is itself checked without a GPU.

Same generators as the GPU file.  Bounds, those of the GPU file (derived in util_mp_project.py): factors 1e-13 relative, likelihood
and evidence 1e-13 (sum_abs + nterms).  The input conditions that go with the bounds are asserted here on the reference alone,
over every value-edge and hyper-parameter case the GPU file runs, with zero components excluded:
  clamp guard   with the prior, no component has |up + ga - 1| < 1e-3 (|up| + 1);
  fudge guard   no exp(psi(alh)) beh within a factor 2 of fudge unless it is below fudge / 2;
  fudge = 0     only where the reference shows every lh > 0.
"""
import importlib

import numpy as np
import pytest

import util_mp_project as MP
import util_project as UP
import util_vb_project as UV

EPS = MP.EPS


def P():
    return importlib.import_module("ccfindr_amd.project")      # (the package attribute `project` is the function)


def per_of(r):
    per = P().pass_entries(r)
    assert per == P().vb_pass_entries(r)
    return per


def check_ml(r, lengths, edge):
    """Two steps of every cell: restatement against 50 digits, step by step; the clamp guard on every step -> the references."""
    case = MP.ml_case(r, lengths, edge)
    refs = MP.ml_reference(r, lengths, edge, 2)
    h = case.h0
    for step in (0, 1):
        h = UP.h_half(case.X, case.W, h, case.prior, case.ga, case.gb)
        e_h, e_lk = MP.ml_errors(h, UP.cell_likelihood(case.X, case.W, h), refs, step)
        guard = min(MP.clamp_guard(c[step]) for c in refs) if case.prior else np.inf
        print(f"{case.name}, step {step + 1}: h %.3g, lk %.3g of (sum_abs + nterms), clamp guard %.3g" % (e_h, e_lk, guard))
        assert e_h <= MP.FACTOR_BOUND and e_lk <= MP.SUM_BOUND
        assert guard >= 1e-3
    return case, refs


def check_vb(r, lengths, edge="plain", ah=0.8, bh=1.7, fudge=EPS, iters=2):
    case = MP.vb_case(r, lengths, edge, ah, bh, fudge)
    refs = MP.vb_reference(r, lengths, edge, ah, bh, fudge, iters)
    cew = case.ew.sum(axis=0)
    lh = case.lh0
    for step in range(iters):
        lh, eh, dh, alh = UV.h_half(case.X, case.lw, cew, lh, ah, bh, fudge)
        ev = UV.cell_evidence(case.X, case.lw, cew, lh, eh, alh, ah, bh)
        errs = MP.vb_errors(lh, eh, dh, ev, refs, step)
        print(f"{case.name}, step {step + 1}: lh %.3g eh %.3g dh %.3g, evidence %.3g of (sum_abs + nterms)" % errs)
        assert max(errs[:3]) <= MP.FACTOR_BOUND and errs[3] <= MP.SUM_BOUND
        assert all(MP.fudge_guard(c[step], fudge) for c in refs)
        assert np.all(MP.stack(refs, step, "lh") > 0.0)
    return case, refs


# ---- the generators' plain cases, at a subset of ranks ------------------------------------------------------------------------
@pytest.mark.parametrize("r,full", [(1, False), (10, True), (24, True), (33, False), (128, True)])
def test_ml_restatement_against_50_digits(r, full):
    per = per_of(r)
    check_ml(r, tuple(MP.full_lengths(per) if full else MP.short_lengths(per)), "plain")


@pytest.mark.parametrize("r,full", [(1, False), (10, True), (24, True), (33, False), (128, True)])
def test_vb_restatement_against_50_digits(r, full):
    per = per_of(r)
    check_vb(r, tuple(MP.full_lengths(per) if full else MP.short_lengths(per)))


# ---- every value edge the GPU file runs, at its ranks -----------------------------------------------------------------------
@pytest.mark.parametrize("edge", MP.ML_EDGES)
@pytest.mark.parametrize("r", MP.EDGE_WIDTHS)
def test_ml_value_edges(r, edge):
    case, refs = check_ml(r, tuple(MP.edge_lengths(per_of(r))), edge)
    if edge == "noninteger":
        assert np.any(case.X != np.rint(case.X))
    if edge == "large":
        assert case.X[case.X > 0].min() >= 1e4 and case.X.max() <= 1e6
    if edge == "fit":
        assert 0.25 < np.mean(case.W == EPS) < 0.4 and case.W.max() > 100.0 and np.all(case.W.max(axis=1) >= 1e-3)
    if edge == "floor":
        assert np.all((case.h0 == EPS).any(axis=0)) and np.all((case.h0 > EPS).any(axis=0))
    if edge == "prior_clamp":
        for step in (0, 1):
            h = MP.stack(refs, step, "h")
            assert (h == EPS).any() and (h > EPS).any()          # the eps clamp of :15 is taken, and not everywhere


@pytest.mark.parametrize("edge", MP.VB_EDGES)
@pytest.mark.parametrize("r", MP.EDGE_WIDTHS)
def test_vb_value_edges(r, edge):
    case, refs = check_vb(r, tuple(MP.edge_lengths(per_of(r))), edge)
    if edge == "fit":
        t = case.lw * np.log(case.lw)
        assert 0.25 < np.mean(case.lw == EPS) < 0.4 and t.min() < -0.3 and t.max() > 100.0       # lw log lw spans its range
    if edge == "floor":
        assert np.all((case.lh0 == EPS).any(axis=0)) and np.all((case.lh0 > EPS).any(axis=0))


# ---- every hyper-parameter case the GPU file runs ---------------------------------------------------------------------------
@pytest.mark.parametrize("fudge", [EPS, 0.0], ids=["eps", "0"])
@pytest.mark.parametrize("ah,bh", MP.HYPERS + [MP.HYPER_FAR])
@pytest.mark.parametrize("r", MP.HYPER_WIDTHS)
def test_vb_hyper_parameters(r, ah, bh, fudge):
    check_vb(r, tuple(MP.edge_lengths(per_of(r))), "plain", ah, bh, fudge, iters=1 if (ah, bh) == MP.HYPER_FAR else 2)


# ---- the kernels' pass, rank by rank ----------------------------------------------------------------------------------------
def test_pass_entries_of_every_rank():
    """256, 128, 64 entries of a cell per pass by padded rank <= 32, <= 64, <= 128, for both kernels; the padded ranks are the
    24 widths the GPU file walks, each reached by r = R and by r = R - 1."""
    from ccfindr_amd.engine import padded_rank
    seen = set()
    for r in range(1, 129):
        R = padded_rank(r)
        seen.add(R)
        want = 256 if R <= 32 else (128 if R <= 64 else 64)
        assert P().pass_entries(r) == want and P().vb_pass_entries(r) == want, r
    assert sorted(seen) == MP.WIDTHS and len(MP.WIDTHS) == 24
    for R in MP.WIDTHS:
        assert padded_rank(R) == R and padded_rank(max(R - 1, 1)) == R
