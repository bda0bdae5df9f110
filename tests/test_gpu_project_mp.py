"""k_project (csrc/project.h) and k_vb_project (csrc/vbproject.h) against their cells evaluated in 50-digit arithmetic
(tests/util_mp_project.py), with no fp64 restatement in between, at every padded rank the kernels are compiled for.

Both kernels are templates on the padded rank R and ``with_rank`` instantiates 24 widths: 2, 4, .., 32 (one lane per entry),
40..64 (two lanes) and 80..128 (four).  Each has its own register allocation, spill code and unrolled dots -- R = 16..24, 48 and
96 of k_vb_project are capped to two waves per SIMD (``vbp_waves_per_simd``) and spill by design; R = 32 and 64 are its most
register-heavy forms -- so every width runs here, at r = R and at r = R - 1 (where the padding column must stay inert).

Through ``project_columns`` / ``vb_project_columns`` with Tol = 0, so that no cell stops early, Itmax 1 and 2 from one start.
STEP 2 IS CHECKED AS A STEP: its 50-digit reference starts from the device's own Itmax = 1 output (the first iteration of an
Itmax = 2 run does the same arithmetic in the same order, so its bits are those), which holds ``pass(false)`` -- the pass whose
lambda_i(new) serves this step's likelihood term AND the next step's quotients -- to the one-step bound, with no compounded error.

Bounds (derived in util_mp_project.py): factors (h; lh, eh, dh) 1e-13 relative over ALL components; likelihood and evidence
|got - ref| <= 1e-13 (sum_abs + nterms) -- not relative to the result, whose terms sum to about twenty times itself.  The input
conditions that go with the bounds (clamp guard, fudge guard, lh > 0 wherever fudge = 0) are asserted on the reference;
tests/test_project_mp_cpu.py holds them for these same cases without a GPU.  No NaN cases here: tests/test_gpu_project.py and
tests/test_gpu_vb_project.py have them.

Largest errors seen on the MI355X: DESIGN.md sections 5f and 5g.
"""
import importlib

import numpy as np
import pytest

import util_mp_project as MP

pytestmark = pytest.mark.gpu

EPS = MP.EPS
MAXIMA = {}


def P():
    return importlib.import_module("ccfindr_amd.project")      # (the package attribute `project` is the function)


@pytest.fixture(scope="module", autouse=True)
def _print_maxima():
    yield
    for k in sorted(MAXIMA):
        print("largest over the file, %-28s %.3g" % (k, MAXIMA[k]))


def note(kernel, step, names, errs):
    for nm, e in zip(names, errs):
        k = f"{kernel} step {step} {nm}"
        MAXIMA[k] = max(MAXIMA.get(k, 0.0), e)


def check_ml(r, lengths, edge="plain"):
    """Itmax = 1 and Itmax = 2 of every cell against 50 digits -> (the case, h after one step, h after two)."""
    import ccfindr_amd as C
    case = MP.ml_case(r, lengths, edge)
    m = len(lengths)
    M = C.CountMatrix(case.X)
    run = [P().project_columns(M, case.W, case.h0, 0, m, case.prior, case.ga, case.gb, Itmax=it, Tol=0.0) for it in (1, 2)]
    M.close()
    refs = (MP.ml_reference(r, lengths, edge, 1), MP.ml_steps(case, run[0][0], 1))       # step 2 from the device's step 1
    for it, (h, lk, nsteps, why), ref in zip((1, 2), run, refs):
        errs = MP.ml_errors(h, lk, ref, 0)
        guard = min(MP.clamp_guard(c[0]) for c in ref) if case.prior else np.inf
        print(f"{case.name}, step {it}: h %.3g, lk %.3g of (sum_abs + nterms); clamp guard %.3g" % (*errs, guard))
        note("k_project", it, ("h", "lk"), errs)
        assert guard >= 1e-3
        assert errs[0] <= MP.FACTOR_BOUND and errs[1] <= MP.SUM_BOUND
        assert np.all(nsteps == it) and np.all(why == 4)
    return case, run[0][0], run[1][0]


def check_vb(r, lengths, edge="plain", ah=0.8, bh=1.7, fudge=EPS, its=(1, 2)):
    import ccfindr_amd as C
    case = MP.vb_case(r, lengths, edge, ah, bh, fudge)
    m = len(lengths)
    M = C.CountMatrix(case.X)
    run = [P().vb_project_columns(M, case.lw, case.ew, case.lh0, ah, bh, 0, m, fudge=fudge, Itmax=it, Tol=0.0) for it in its]
    M.close()
    refs = [MP.vb_reference(r, lengths, edge, ah, bh, fudge, 1)]
    if len(its) > 1:
        refs.append(MP.vb_steps(case, run[0][0], 1))                                      # step 2 from the device's step 1
    for it, (lh, eh, dh, ev, nsteps, why), ref in zip(its, run, refs):
        errs = MP.vb_errors(lh, eh, dh, ev, ref, 0)
        print(f"{case.name}, step {it}: lh %.3g eh %.3g dh %.3g, evidence %.3g of (sum_abs + nterms)" % errs)
        note("k_vb_project", it, ("lh", "eh", "dh", "evidence"), errs)
        assert all(MP.fudge_guard(c[0], fudge) for c in ref) and np.all(MP.stack(ref, 0, "lh") > 0.0)
        assert max(errs[:3]) <= MP.FACTOR_BOUND and errs[3] <= MP.SUM_BOUND
        assert np.all(nsteps == it) and np.all(why == 4)
    return case


def width_cases():
    return [pytest.param(R, R if full else max(R - 1, 1), full, id=f"R{R}-r{R if full else max(R - 1, 1)}")
            for R in MP.WIDTHS for full in (True, False)]


def width_lengths(R, r, full, per):
    from ccfindr_amd.engine import padded_rank
    assert padded_rank(r) == R and per == (256 if R <= 32 else (128 if R <= 64 else 64))
    return tuple(MP.full_lengths(per) if full else MP.short_lengths(per))


# ---- (a) every compiled width ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,r,full", width_cases())
def test_ml_every_width(R, r, full):
    """n = 560, basis and start U(0.05, 1), counts 1..5.  r = R: cells of [1, 2, per - 1, per, per + 1, 2 per + 1] stored
    entries; r = R - 1 (r = 1 at R = 2): [1, 3, per + 1], one padding column."""
    check_ml(r, width_lengths(R, r, full, P().pass_entries(r)))


@pytest.mark.parametrize("R,r,full", width_cases())
def test_vb_every_width(R, r, full):
    """The same cells on a posterior drawn by ``posterior()`` of tests/test_gpu_vb_project.py, (ah, bh) = (0.8, 1.7)."""
    check_vb(r, width_lengths(R, r, full, P().vb_pass_entries(r)))


# ---- (b) hyper-parameters -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fudge", [EPS, 0.0], ids=["eps", "0"])
@pytest.mark.parametrize("ah,bh", MP.HYPERS + [MP.HYPER_FAR])
@pytest.mark.parametrize("r", MP.HYPER_WIDTHS)
def test_vb_hyper_parameters(r, ah, bh, fudge):
    """The (ah, bh) of util_mp_step.CASES, and (0.05, 2) -- psi far negative -- for one iteration; fudge eps and 0 (no lh is 0
    there: the reference shows it)."""
    check_vb(r, tuple(MP.edge_lengths(P().vb_pass_entries(r))), "plain", ah, bh, fudge,
             its=(1,) if (ah, bh) == MP.HYPER_FAR else (1, 2))


# ---- (c) value edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge", MP.ML_EDGES)
@pytest.mark.parametrize("r", MP.EDGE_WIDTHS)
def test_ml_value_edges(r, edge):
    """Non-integer counts; counts of 1e4..1e6; a basis as a fit leaves it (a third at the clamp, the rest over 1e-8..1e3); a start
    with components at eps; the prior with (1.7, 0.6) and with (0.5, 1.0), where up + ga - 1 goes negative and the eps clamp of
    R/factorize.R:15 is taken."""
    case, h1, h2 = check_ml(r, tuple(MP.edge_lengths(P().pass_entries(r))), edge)
    if edge == "prior_clamp":
        for h in (h1, h2):
            assert (h == EPS).any() and (h > EPS).any()


@pytest.mark.parametrize("edge", MP.VB_EDGES)
@pytest.mark.parametrize("r", MP.EDGE_WIDTHS)
def test_vb_value_edges(r, edge):
    """Non-integer counts; counts of 1e4..1e6 (lgamma(x + 1) dominates the evidence, the asymptotic branch of dev_psi_lgamma
    carries alh); lw of a fitted basis' magnitudes (lw log lw spans its range); a start with components at fudge."""
    check_vb(r, tuple(MP.edge_lengths(P().vb_pass_entries(r))), edge)
