"""The stopping rules of the three device-driven loops, restated once in numpy -- TEST INFRASTRUCTURE ONLY.

A loop run with Tol = 0 and history=True returns the evidence (or likelihood) of every step.  Each rule is a few IEEE
operations on those doubles -- a division, a subtraction, fabs and comparisons (VB, coupled projection); a subtraction, a
multiplication, fabs and a comparison (ML) -- and the library is built with -ffp-contract=off, so the same expressions on
the returned column give the device's decision EXACTLY, for any Tol, n0 and Itmax.  Every predictor returns
``(it, reason, lk0, lk_last)``: the step the loop ends on, why, the lagging value and the last step's own value.

    vb_predict   csrc/kernels.h, vb_control_step     (reference R/bayesian.R:342-348)
    ml_predict   csrc/mlnmf.h, ml_control_step       (reference R/factorize.R:211-213)
    vbp_predict  csrc/vbproject.h, k_vbp_control     (the VB rule on the total evidence, without its direction clause)

tests/test_stop_rules_cpu.py holds them to the product's own host loops; tests/test_gpu_stop_rules.py holds the device to them.
"""
import numpy as np

F = np.float64


def vb_rel(lkh, lk0):
    """|1 - lkh / lk0| as the rule forms it (lk0 = 0 at step 1 gives inf or NaN, never an exception)."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return np.abs(F(1.0) - F(lkh) / F(lk0))


def vb_predict(lkh, Tol, n0, Itmax):
    """``lkh``: the evidence column of a Tol = 0 history of at least min(Itmax, the NaN step) rows.  Reason 1: NaN evidence;
    2: converged, lk0 NOT refreshed; 4: Itmax."""
    Tol, lk0, l = F(Tol), F(0.0), F(np.nan)
    for it in range(1, int(Itmax) + 1):
        l = F(lkh[it - 1])
        if l != l:
            return it, 1, float(lk0), float(l)
        if it > 1 and it > n0 and l >= lk0 and vb_rel(l, lk0) < Tol:
            return it, 2, float(lk0), float(l)
        lk0 = l
    return int(Itmax), 4, float(lk0), float(l)


def ml_converged(lkold, lk, Tol):
    """abs(lkold - lk) < Tol * abs(lkold); false whenever a NaN takes part (inf - inf, inf * 0, a NaN likelihood)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return bool(np.abs(F(lkold) - F(lk)) < F(Tol) * np.abs(F(lkold)))


def ml_predict(lk, Tol, Itmax):
    """``lk``: the likelihood history of a Tol = 0 run.  lkold starts at -inf, so the first step never stops; reason 2:
    converged, lkold NOT refreshed; 4: Itmax."""
    lkold, l = F(-np.inf), F(np.nan)
    for it in range(1, int(Itmax) + 1):
        l = F(lk[it - 1])
        if ml_converged(lkold, l, Tol):
            return it, 2, float(lkold), float(l)
        lkold = l
    return int(Itmax), 4, float(lkold), float(l)


def vbp_predict(E, Tol, n0, Itmax):
    """``E``: the total-evidence column of a Tol = 0 history of the coupled projection.  Reason 3: NaN; 1: converged -- the VB
    rule WITHOUT ``lkh >= lk0``, a falling step stops too --, lk0 not refreshed; 4: Itmax."""
    Tol, lk0, e = F(Tol), F(0.0), F(np.nan)
    for it in range(1, int(Itmax) + 1):
        e = F(E[it - 1])
        if e != e:
            return it, 3, float(lk0), float(e)
        if it > 1 and it > n0 and vb_rel(e, lk0) < Tol:
            return it, 1, float(lk0), float(e)
        lk0 = e
    return int(Itmax), 4, float(lk0), float(e)


def straddle(pred, lo_guess, max_walk=64):
    """Two adjacent doubles ``(tol_no, tol_yes)``: ``pred(tol_no)`` is false, ``pred(tol_yes)`` true.  ``pred``: one step's
    predicate as a function of the tolerance, monotone in it; ``lo_guess``: a tolerance at or next to the flip -- for the VB
    rules the step's own d_t = |1 - l_t / l_(t-1)| (false there, true one ulp above), for ML |lkold - lk| / |lkold|, from where
    the walk is a few ulps because the rule multiplies where the guess divides."""
    x = F(lo_guess)
    assert np.isfinite(x) and x >= 0
    for _ in range(max_walk):
        if not pred(x):
            break
        x = np.nextafter(x, F(-np.inf))
    else:
        raise AssertionError("the predicate stays true below the guess")
    for _ in range(max_walk):
        y = np.nextafter(x, F(np.inf))
        if pred(y):
            break
        x = y
    else:
        raise AssertionError("the predicate stays false above the guess")
    assert not pred(x) and pred(y) and np.nextafter(x, F(np.inf)) == y and y > x
    return float(x), float(y)


def vb_straddle(col, t):
    """The straddle of step ``t`` (1-based, t >= 2) of the VB / coupled rule on the history column ``col`` -> (tol_no, tol_yes, d_t)."""
    d = vb_rel(col[t - 1], col[t - 2])
    no, yes = straddle(lambda tol: bool(d < F(tol)), d)
    assert no == float(d)
    return no, yes, float(d)


def ml_straddle(col, t):
    """The same for the ML rule -> (tol_no, tol_yes)."""
    lkold, lk = F(col[t - 2]), F(col[t - 1])
    return straddle(lambda tol: ml_converged(lkold, lk, tol), np.abs(lkold - lk) / np.abs(lkold))


# ---- the case lists both test files run (each case states its precondition on the base history) ----------------------------
A_STEPS = (6, 7, 8, 9, 15, 16, 17, 24, 25)       # either side of the queued batches of eight
BASE_ITMAX = 60


def rising(col, t):
    return bool(col[t - 1] >= col[t - 2])


def first_rising(col, after):
    """The first step t > after, t >= 2, whose evidence is at least the step's before."""
    for t in range(max(after + 1, 2), len(col) + 1):
        if rising(col, t):
            return t
    raise AssertionError("no rising step")


def vb_cases(col):
    """Cases (a) to (f) of the VB loop on the evidence column ``col`` of a flags-off base run: dicts of id, Tol, n0, Itmax
    and the outcome the case requires (it, reason, lk0_row: the 1-based history row lk0 must equal; not_it: a step the run
    must not end on).  The predictor is held to these outcomes, the loops to the predictor."""
    assert len(col) == BASE_ITMAX and np.all(np.isfinite(col))
    cases = []

    def add(id, Tol, n0, Itmax=BASE_ITMAX, **want):
        cases.append(dict(id=id, Tol=float(Tol), n0=int(n0), Itmax=int(Itmax), want=want))

    for t in A_STEPS:                                                        # (a)
        assert rising(col, t), f"(a) step {t} does not rise"
        no, yes, d = vb_straddle(col, t)
        assert d > 0
        add(f"a{t}-no", no, t - 1, not_it=t)
        add(f"a{t}-yes", yes, t - 1, it=t, reason=2, lk0_row=t - 1)
    ds = [float(vb_rel(col[t - 1], col[t - 2])) for t in (3, 4, 5)]         # (b)
    tol_b = 2.0 * max(ds)
    assert not any(rising(col, t) for t in (3, 4, 5)) and all(d < tol_b for d in ds), "(b) steps 3..5 must fall, inside Tol"
    s = first_rising(col, 2)
    assert s > 5 and vb_rel(col[s - 1], col[s - 2]) < tol_b
    add("b", tol_b, 2, it=s, reason=2, lk0_row=s - 1)
    for t in (7, 8):                                                         # (c)
        assert all(rising(col, u) and vb_rel(col[u - 1], col[u - 2]) < 1.0 for u in (t, t + 1))
        add(f"c{t}-n0={t}", 1.0, t, it=t + 1, reason=2, lk0_row=t)
        add(f"c{t}-n0={t - 1}", 1.0, t - 1, it=t, reason=2, lk0_row=t - 1)
    for n0 in (0, 1):                                                        # (d)
        add(f"d-n0={n0}", 1e300, n0, it=first_rising(col, 1), reason=2, not_it=1)
    no, yes, _ = vb_straddle(col, 9)                                         # (e)
    add("e-rule-on-itmax", yes, 8, Itmax=9, it=9, reason=2, lk0_row=8)
    add("e-itmax", no, 8, Itmax=9, it=9, reason=4, lk0_row=9)
    add("f-tol=0", 0.0, 2, Itmax=30, it=30, reason=4, lk0_row=30)            # (f)
    add("f-tol<0", -1.0, 2, Itmax=30, it=30, reason=4, lk0_row=30)
    add("f-tol=inf", np.inf, 2, it=first_rising(col, 2), reason=2)
    return cases


def decisive_steps(col, n0, count, after=0, predict=vb_predict, Itmax=BASE_ITMAX):
    """The first ``count`` steps t > max(n0, after, 1) that a run with this FIXED n0 ends on under the tolerance one ulp above
    step t's own change: no earlier step past n0 is inside that tolerance (with n0 = t - 1, as in case (a), every rising step
    is such a step; with the n0 of a flags-on base run only the steps whose change is the smallest so far are)."""
    found = []
    for t in range(max(n0, after, 1) + 1, Itmax):
        if vb_rel(col[t - 1], col[t - 2]) > 0 and predict(col, vb_straddle(col, t)[1], n0, Itmax)[0] == t:
            found.append(t)
            if len(found) == count:
                return tuple(found)
    raise AssertionError(f"fewer than {count} decisive steps past n0 = {n0}")


def straddle_cases(col, steps, n0, label):
    """Case (g): the straddle of (a) at ``steps`` (decisive_steps) of a base run whose (n0, dn) the case shares."""
    cases = []
    for t in steps:
        assert t > n0 and rising(col, t), f"({label}) step {t} does not rise"
        no, yes, d = vb_straddle(col, t)
        assert d > 0 and vb_predict(col, yes, n0, BASE_ITMAX)[0] == t, f"({label}) step {t} does not decide"
        cases.append(dict(id=f"{label}{t}-no", Tol=no, n0=n0, Itmax=BASE_ITMAX, want=dict(not_it=t)))
        cases.append(dict(id=f"{label}{t}-yes", Tol=yes, n0=n0, Itmax=BASE_ITMAX, want=dict(it=t, reason=2, lk0_row=t - 1)))
    return cases


def first_step_cases(col):
    """Case (d) on a trajectory that RISES at step 2 (a start some steps on): n0 = 0 and n0 = 1 with a huge Tol end at step 2,
    not at step 1, where lk0 is still 0."""
    assert rising(col, 2) and vb_rel(col[1], col[0]) < 1.0
    return [dict(id=f"d-rising-n0={n0}-tol={tol}", Tol=tol, n0=n0, Itmax=BASE_ITMAX, want=dict(it=2, reason=2, lk0_row=1, not_it=1))
            for n0 in (0, 1) for tol in (1e300, float("inf"))]


def hold(case, col, pred):
    """The predicted ``(it, reason, lk0, lk_last)`` is the outcome the case requires."""
    it, reason, lk0, last = pred
    w = case["want"]
    assert 1 <= it <= case["Itmax"] and last == col[it - 1], case["id"]
    assert "it" not in w or it == w["it"], (case["id"], it)
    assert "reason" not in w or reason == w["reason"], (case["id"], reason)
    assert "not_it" not in w or it != w["not_it"], (case["id"], it)
    assert "lk0_row" not in w or lk0 == col[w["lk0_row"] - 1], case["id"]
    if reason == 2:
        assert lk0 == col[it - 2], case["id"]                  # lagging: the break does not refresh it
    elif reason == 4:
        assert it == case["Itmax"] and lk0 == col[it - 1], case["id"]


ML_STEPS = (2, 8, 9, 17)


def ml_cases(col):
    """The ML likelihood loop's cases on the history ``col`` of a Tol = 0 run: straddles at ML_STEPS, Tol = 0, Tol = inf."""
    assert len(col) >= 30 and np.all(np.isfinite(col))
    cases = []
    for t in ML_STEPS:
        no, yes = ml_straddle(col, t)
        assert ml_predict(col, yes, 30)[:2] == (t, 2), f"ML step {t}: an earlier step is inside its tolerance"
        cases.append(dict(id=f"ml{t}-no", Tol=no, Itmax=30, want=dict(not_it=t)))
        cases.append(dict(id=f"ml{t}-yes", Tol=yes, Itmax=30, want=dict(it=t, reason=2)))
    cases.append(dict(id="ml-tol=0", Tol=0.0, Itmax=30, want=dict(it=30, reason=4)))
    cases.append(dict(id="ml-tol=inf", Tol=float("inf"), Itmax=30, want=dict(it=2, reason=2, not_it=1)))   # inf < inf is false
    cases.append(dict(id="ml-itmax=1", Tol=float("inf"), Itmax=1, want=dict(it=1, reason=4)))
    return cases


# ---- the coupled projection's cases ----
def vbp_cases(col, n0):
    """Straddles at n0 + 1 and at the next step that decides a run with this n0 (decisive_steps); each also with Itmax on that
    step: the tolerance that stops gives the rule's reason and a lagging lk0, the other one reason 4 and lk0 refreshed."""
    cases = []
    steps = (n0 + 1,) + decisive_steps(col, n0, 1, after=n0 + 1, predict=vbp_predict, Itmax=40)
    for t in steps:
        no, yes, d = vb_straddle(col, t)
        assert d > 0 and vbp_predict(col, yes, n0, 40)[0] == t
        cases.append(dict(id=f"vbp{t}-no", Tol=no, n0=n0, Itmax=40, want=dict(not_it=t)))
        cases.append(dict(id=f"vbp{t}-yes", Tol=yes, n0=n0, Itmax=40, want=dict(it=t, reason=1, lk0_row=t - 1)))
        cases.append(dict(id=f"vbp{t}-yes-itmax", Tol=yes, n0=n0, Itmax=t, want=dict(it=t, reason=1, lk0_row=t - 1)))
        cases.append(dict(id=f"vbp{t}-no-itmax", Tol=no, n0=n0, Itmax=t, want=dict(it=t, reason=4, lk0_row=t)))
    return cases


def vbp_n0_cases(col, n0):
    """Tol chosen so that steps n0 and n0 + 1 are both inside it: n0 against n0 - 1 moves the stop from n0 + 1 to n0."""
    tol = 2.0 * max(float(vb_rel(col[t - 1], col[t - 2])) for t in (n0, n0 + 1))
    return [dict(id=f"vbp-n0={n0}", Tol=tol, n0=n0, Itmax=40, want=dict(it=n0 + 1, reason=1, lk0_row=n0)),
            dict(id=f"vbp-n0={n0 - 1}", Tol=tol, n0=n0 - 1, Itmax=40, want=dict(it=n0, reason=1, lk0_row=n0 - 1))]


def hold_vbp(case, col, pred):
    it, reason, lk0, last = pred
    w = case["want"]
    assert last == col[it - 1]
    for key, got in (("it", it), ("reason", reason)):
        assert key not in w or got == w[key], (case["id"], key, got)
    assert "not_it" not in w or it != w["not_it"], case["id"]
    assert "lk0_row" not in w or lk0 == col[w["lk0_row"] - 1], case["id"]
