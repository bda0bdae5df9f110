"""The hyper-parameter Newton update (reference R/bayesian.R:2-53) of the library's HOST build against 50-digit math
(tests/util_mp_hyper.py), one iteration at a time, on the seeded grid the device test (tests/test_gpu_hyper_update.py) runs
as well; the 50-digit statement itself against the committed fp64 oracle.  No GPU.

Measured here (CPU build):
  trigamma           plain-float restatement of the series: worst 8.1e-16 relative on trigamma_grid() (its worst at
                     x = 10.00015, just past the seam) -> the library's bound is twice that, 1.62e-15; the library itself,
                     host and device build alike: 8.1e-16.
  per iteration      25 622 transitions of 1 950 cases, worst error 0.17 of the derived tolerance (c_f = 18.7, c_g = 9.3).
  oracle per decade  worst relative error of oracle.vbnmf_oracle.hyper_update's final shape against the 50-digit update, by
                     decade of the start shape, 1 292 comparable cases:
                       1e-4: 4.6e-13   1e-3: 1.2e-13   1e-2: 1.7e-14   1e-1: 4.4e-14   1e0: 6.5e-13   1e1: 1.5e-12
                       1e2: 5.9e-11    1e3: 9.1e-10    1e4: 2.1e-07    1e5: 1.3e-05    (1e-300: 0)
                     (log(a) - psi(a) and 1/a - psi'(a) cancel for large a: the reference's own formula in fp64.)
                     The whole-update tolerance is 10 x these, floor 1e-12; the host build's worst: 1.9e-05 (decade 1e5).
  skipped share      threshold-adjacent + halving-adjacent: 0 of 1 950 by the 50-digit reference alone (cap 5 %); 539 cases
                     have no root, run away and fail in every arithmetic: checked per iteration until fp64 no longer
                     determines the step (a ~ 1e14), then only for `failed` and the untouched outputs.
"""
import numpy as np
import pytest

import util_mp_hyper as U
import util_special as S


def test_trigamma_host_build():
    """dev_trigamma (csrc/special.h) against mpmath.psi(1, x); bound: twice the plain-float series' own worst error on this
    grid (measured 8.1e-16 -> 1.62e-15), not anything the library returns."""
    xs = U.trigamma_grid()
    bound = U.trigamma_bound()
    assert 1e-15 < bound < 2.5e-15, bound                           # the series itself is good to a few ulp
    err = U.trigamma_rel_err(xs, S.evaluate(7, xs, device=False))
    print("trigamma host: worst %.3g at x = %r, bound %.3g" % (err.max(), xs[err.argmax()], bound))
    assert err.max() <= bound, (err.max(), xs[err.argmax()])


def test_trigamma_guard_is_nan_before_the_shift_loop():
    """x <= 0, NaN, +-inf: NaN at once (the shift loop `while (x < 10) x += 1` would never end from -2^53 down)."""
    bad = np.array([0.0, -0.0, -1.0, -1e17, -np.inf, np.nan, np.inf])
    assert np.all(np.isnan(S.evaluate(7, bad, device=False)))


def test_grid_has_every_stratum():
    G, ref = U.case_grid(), U.reference()
    n = len(ref)
    assert 1900 <= n <= 2100
    assert {tuple(f) for f in G["flags"]} == set(U.FLAG_SETS)
    a0 = np.concatenate([G["hyper"][:, 0], G["hyper"][:, 2]])
    assert np.all(a0 > 0) and np.all(np.isfinite(G["hyper"])) and np.all(G["hyper"] > 0)     # nothing a kernel must not see
    assert np.sum((a0 > 9.999) & (a0 < 10.001)) >= 100 and np.sum(a0 == 1e-300) >= 20
    first_halves = one_iteration = one_lane = no_newton = no_root = 0
    for c in range(n):
        fl, st, hy = G["flags"][c], G["stats"][c], G["hyper"][c]
        steps = [U.newton_step(hy[2 * s], hy[2 * s + 1], st[s], st[2 + s], fl[2 * s]) for s in range(2)]
        first_halves += any(s["halvings"] > 0 for s in steps)
        one_iteration += ref[c]["iters"] == 1 and not ref[c]["failed"]
        one_lane += fl[0] + fl[2] == 1
        no_newton += tuple(fl) in ((0, 1, 0, 0), (0, 0, 0, 1))
        root = [1 + st[s] - np.log(hy[2 * s + 1]) - st[2 + s] / hy[2 * s + 1] < 0 for s in range(2)]
        # (not from 1e-300: there psigamma overflows, the step is -0 and the shape stays where it is)
        if any(fl[2 * s] and not root[s] and np.isfinite(st[s]) and hy[2 * s] > 1e-150 for s in range(2)):
            no_root += 1
            assert ref[c]["failed"], c                              # no root: the iterates run away, the update fails
    assert first_halves >= 150 and one_iteration >= 100 and one_lane >= 100 and no_newton >= 150 and no_root >= 100
    assert all(ref[c]["failed"] for c in np.flatnonzero(G["stratum"] == "minus_inf"))
    tiny = [c for c in np.flatnonzero(G["stratum"] == "tiny") if G["flags"][c][0]]
    for c in tiny:                                                  # 1 / (x x) overflows: the step is -0, aw stays
        assert ref[c]["trace"][0][0] == U._f(1e-300), c


def test_skip_cap_by_the_reference_alone():
    """Threshold-adjacent (df within 1e-9 relative of Tol, or within the steps' own fp64 tolerance of it) and
    halving-adjacent (some a0 - d / 2^h within tolerance of 0) cases: at most 5 % of the grid.  Measured: 0 of 1 950."""
    ref = U.reference()
    near = sum(1 for R in ref if R["near_tol"] or R["near_zero"])
    print("skipped share by the reference alone: %d of %d" % (near, len(ref)))
    assert near <= 0.05 * len(ref)


def test_mp_step_against_the_committed_oracle_one_iteration_at_a_time():
    """oracle.vbnmf_oracle.hyper_update with Niter = 2, Tol = inf makes exactly one Newton iteration, halvings included
    (:17-38 once, then the break).  From every start of the grid whose step is finite (the oracle states the reference's
    unbounded halving loop literally) its aw, ah lie within the derived per-iteration tolerance of the 50-digit step:
    no path, so nothing to allow for.  SciPy's digamma / polygamma are taken to meet the bounds the library's are held to."""
    from oracle import vbnmf_oracle as O
    G = U.case_grid()
    checked, worst = 0, 0.0
    for c in range(len(G["flags"])):
        fl, st, hy = G["flags"][c], G["stats"][c], G["hyper"][c]
        if fl[0] + fl[2] == 0 or not (np.all(np.isfinite(st)) and np.all(st[:2] > -700.0)):      # (exp(lm) must not underflow)
            continue
        wh = {"lw": np.exp(st[0:1]), "lh": np.exp(st[1:2]), "ew": st[2:3], "eh": st[3:4]}
        st2 = [float(np.log(wh["lw"])[0]), float(np.log(wh["lh"])[0]), st[2], st[3]]         # what the oracle will form
        steps = [U.newton_step(hy[2 * s], hy[2 * s + 1], st2[s], st2[2 + s], fl[2 * s]) for s in range(2)]
        if any(s_["bad"] or s_["near_zero"] for s_ in steps):
            continue
        got = O.hyper_update(fl, wh, dict(zip(("aw", "bw", "ah", "bh"), (float(v) for v in hy))), Niter=2, Tol=np.inf)
        for s, key in ((0, "aw"), (1, "ah")):
            a0 = hy[2 * s]
            err = abs((U._f(a0) - U._f(got[key])) - steps[s]["d"])
            tol = U.step_tolerance(steps[s], a0)
            assert err <= tol, (c, key, a0, got[key], float(steps[s]["a1"]), float(err), float(tol))
            worst = max(worst, float(err / tol))
            checked += 1
    print("oracle, one iteration: %d steps, worst error %.3g of the tolerance" % (checked, worst))
    assert checked >= 2500


def test_mp_update_against_the_committed_oracle():
    """The whole update on every comparable case of the grid (the 50-digit update converges, no decision of it sits at its
    threshold): bw, bh equal exactly; aw, ah within Tol = 1e-3 relative -- two Newton runs that take the same number of
    steps and stop on a relative step below sqrt(Tol) both end within the square of that of the root.  The errors by decade
    of the start shape (this module's docstring) are what the whole-update tolerance of the hooks' tests is taken from:
    they grow to 1.3e-05 above 1e4, where the start's step is ill-conditioned and the stop at Tol leaves the difference
    of the paths standing.  That is the reference's own formula in fp64, and the reason for the per-iteration checks."""
    worst, count = U.oracle_errors()
    print("oracle vs 50 digits, worst relative error by decade of the start shape (%d cases):" % count,
          {d: "%.2g" % e for d, e in sorted(worst.items())})
    assert count >= 1200 and set(range(-4, 6)) <= set(worst)
    assert max(worst.values()) <= 1e-3
    assert max(e for d, e in worst.items() if d <= 0) <= 1e-11      # well-conditioned starts: the paths coincide


def test_host_hook_on_the_grid():
    """vbnmf_test_hyper_update_host: every traced iteration, every stop decision, iters / failed, the outputs, and the whole
    update against 50-digit math (U.check_hook states each); then the skip cap on what was actually skipped."""
    G = U.case_grid()
    got = U.run_hook(G["flags"], G["stats"], G["hyper"], device=False)
    fig = U.check_hook(got)
    print("host hook:", fig)
    assert fig["skipped_tol"] + fig["skipped_zero"] <= 0.05 * len(G["flags"])
    assert fig["transitions"] > 20000


@pytest.mark.parametrize("bad", [0.0, -1.0, -1e17, -np.inf, np.nan, np.inf])
def test_host_hook_fails_a_shape_that_is_no_positive_number(bad):
    """Host hook only (no kernel ever sees one): the update comes back failed, at once, all four values bit for bit."""
    flags = np.array([[1, 1, 1, 1], [1, 0, 0, 0], [0, 0, 1, 0], [1, 1, 1, 1]], dtype=np.int32)
    hyper = np.array([[bad, 1.0, 2.0, 1.0], [bad, 1.0, 2.0, 1.0], [2.0, 1.0, bad, 1.0], [2.0, 1.0, bad, 3.0]])
    stats = np.tile([-0.3, -0.2, 1.1, 0.9], (4, 1))
    got = U.run_hook(flags, stats, hyper, device=False)
    assert np.all(got["failed"] == 1) and np.all(got["iters"] == 1)
    assert np.array_equal(got["hyper"].view(np.uint64), hyper.view(np.uint64))
    for c in range(4):
        assert U.update(flags[c], stats[c], hyper[c])["failed"]
