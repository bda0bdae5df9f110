"""CPU: the restated stopping rules (tests/util_stop_rules.py) against the product's own host loops -- the device_loop=False
path of ccfindr_amd/bayesian.py (vb_run_rank) and the host loop of ccfindr_amd/factorize.py -- driven by the numpy engines
(tests/fake_engine.py, tests/fake_ml_engine.py), and against the numpy restatement of the coupled projection
(tests/util_vb_project_coupled.py).  The case list is the one tests/test_gpu_stop_rules.py runs on the device, straddled
tolerances included: every comparison is exact, the engines are deterministic and each rule is a few IEEE operations.

The VB rule's three clauses are then mutated one at a time; each mutant must predict another (it, reason) on at least one
case of the list, or the list does not discriminate."""
import warnings

import numpy as np
import pytest

import util_stop_rules as S
from fake_engine import EPS, NumpyPhaseEngine
from fake_ml_engine import OracleMLEngine

HY1 = {"aw": 1.0, "bw": 1.0, "ah": 1.0, "bh": 1.0}
OFF, ON = (False,) * 4, (True,) * 4
RANK = 3


def problem():
    from ccfindr_amd import synth
    X = synth.drop_empty(synth.simulate_data(60, (40, 50, 30), seed=4, sparse=False))
    n, m = X.shape
    return X, synth.random_state(n, m, RANK, HY1, seed=3)


class Recorder(NumpyPhaseEngine):
    """The numpy engine from a fixed start (whatever vb_init drew), keeping every step's evidence."""

    def __init__(self, X, rank, start):
        super().__init__(X, rank)
        self.start, self.trace = start, []

    def set_state(self, lw, lh, eh):
        super().set_state(self.start["lw"], self.start["lh"], self.start["eh"])

    def step(self, hyper, fudge=EPS):
        lkh, stats = super().step(hyper, fudge)
        self.trace.append(self.poison(len(self.trace) + 1, lkh))
        return self.trace[-1], stats

    def poison(self, it, lkh):
        return lkh


def host_vb(X, start, Tol, n0, Itmax, flags=OFF, dn=1, engine=Recorder):
    """ccfindr_amd.bayesian.vb_run_rank stepping from the host -> (it, lk0, the evidence of every step made)."""
    from ccfindr_amd import bayesian as B
    made = []

    def factory(M, r):
        made.append(engine(X, r, start))
        return made[-1]

    bundle = B.make_bundle(X, [RANK], 1, 0, "random", Itmax, flags, 1, 1, Tol, n0, dn, None, False, 0, 0, engine_factory=factory)
    bundle["device_loop"] = False
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rec = B.vb_run_rank(1, RANK, bundle)
    bundle["mat"].close()
    return rec["nsteps"], rec["lk0"], np.array(made[0].trace)


def hold_host(case, col, flags=OFF, dn=1, predict=S.vb_predict, engine=Recorder):
    X, start = problem()
    pred = predict(col, case["Tol"], case["n0"], case["Itmax"])
    it, lk0, trace = host_vb(X, start, case["Tol"], case["n0"], case["Itmax"], flags, dn, engine)
    assert it == pred[0] and len(trace) == it, (case["id"], it, pred)
    assert lk0 == pred[2] or (np.isnan(lk0) and np.isnan(pred[2])), (case["id"], lk0, pred)
    assert np.array_equal(trace, col[:it], equal_nan=True), case["id"]          # the base history's first `it` rows
    # stop or no stop: a rule stop leaves lk0 one step behind, Itmax refreshes it
    assert (pred[1] == 2) == (it > 1 and lk0 == col[it - 2] and lk0 != col[it - 1]), (case["id"], pred)
    return pred


@pytest.fixture(scope="module")
def base():
    X, start = problem()
    it, lk0, col = host_vb(X, start, 0.0, 10, S.BASE_ITMAX)
    again = host_vb(X, start, 0.0, 3, S.BASE_ITMAX)[2]
    assert it == S.BASE_ITMAX and np.array_equal(col, again)                     # flags off: n0 does not move the trajectory
    falls = [t for t in range(2, S.BASE_ITMAX + 1) if not S.rising(col, t)]
    print("numpy engine, flags off: evidence falls at steps", falls, "d_t of steps 2..9:",
          ["%.3g" % S.vb_rel(col[t - 1], col[t - 2]) for t in range(2, 10)])
    return col


def test_vb_host_loop_stops_where_the_restated_rule_says(base):
    cases = S.vb_cases(base)
    assert len(cases) == 2 * len(S.A_STEPS) + 12
    for case in cases:
        S.hold(case, base, hold_host(case, base))


@pytest.mark.parametrize("n0,dn", [(3, 2), (5, 1)])
def test_vb_host_loop_with_the_hyper_update_on(n0, dn):
    """Case (g): with the flags on the trajectory depends on (n0, dn), so the base run shares them; the straddles sit at the
    first two steps that decide a run with that n0."""
    X, start = problem()
    col = host_vb(X, start, 0.0, n0, S.BASE_ITMAX, ON, dn)[2]
    assert len(col) == S.BASE_ITMAX and np.array_equal(col, host_vb(X, start, 0.0, n0, S.BASE_ITMAX, ON, dn)[2])
    steps = S.decisive_steps(col, n0, 2)
    print(f"flags on, (n0, dn) = ({n0}, {dn}): straddled steps", steps)
    for case in S.straddle_cases(col, steps, n0, "g"):
        S.hold(case, col, hold_host(case, col, ON, dn))


def test_vb_host_loop_does_not_stop_at_step_one():
    """Case (d) where it can decide: from a start thirty steps on the evidence rises at step 2."""
    X, start = problem()
    eng = NumpyPhaseEngine(X, RANK)
    eng.set_state(start["lw"], start["lh"], start["eh"])
    for _ in range(30):
        eng.step(HY1)
    later = eng.get_state(("lw", "lh", "eh"))
    col = host_vb(X, later, 0.0, 10, S.BASE_ITMAX)[2]
    for case in S.first_step_cases(col):
        pred = S.vb_predict(col, case["Tol"], case["n0"], case["Itmax"])
        S.hold(case, col, pred)
        it, lk0, trace = host_vb(X, later, case["Tol"], case["n0"], case["Itmax"])
        assert (it, lk0) == (pred[0], pred[2]) and np.array_equal(trace, col[:it]), case["id"]


@pytest.mark.parametrize("s", [1, 4])
def test_vb_host_loop_nan_is_reason_1_also_on_itmax(s, base):
    """Case (h): a NaN evidence at step s.  Itmax = s ends on the NaN, not on Itmax: lk0 keeps step s - 1's value."""
    class NaNAt(Recorder):
        def poison(self, it, lkh):
            return float("nan") if it >= s else lkh

    col = base.copy()
    col[s - 1:] = np.nan
    for Itmax, reason in ((S.BASE_ITMAX, 1), (s, 1)) + (((s - 1, 4),) if s > 1 else ()):
        case = dict(id=f"h-s={s}-Itmax={Itmax}", Tol=1e-5, n0=10, Itmax=Itmax, want={})
        X, start = problem()
        pred = S.vb_predict(col, 1e-5, 10, Itmax)
        it, lk0, trace = host_vb(X, start, 1e-5, 10, Itmax, engine=NaNAt)
        assert pred[:2] == (min(s, Itmax), reason), case["id"]
        assert (it, lk0) == (pred[0], pred[2]) and np.array_equal(trace, col[:it], equal_nan=True), case["id"]
        assert lk0 == (0.0 if s == 1 else col[s - 2])


# ---- the mutants ------------------------------------------------------------------------------------------------------------
def mutant(kind):
    """vb_predict with one clause changed: 'no-direction' drops lkh >= lk0, 'le' has <= for <, 'ge-n0' has it >= n0 for it > n0."""
    def predict(lkh, Tol, n0, Itmax):
        Tol, lk0, l = S.F(Tol), S.F(0.0), S.F(np.nan)
        for it in range(1, int(Itmax) + 1):
            l = S.F(lkh[it - 1])
            if l != l:
                return it, 1, float(lk0), float(l)
            past = it >= n0 if kind == "ge-n0" else it > n0
            up = True if kind == "no-direction" else l >= lk0
            d = S.vb_rel(l, lk0)
            if it > 1 and past and up and (d <= Tol if kind == "le" else d < Tol):
                return it, 2, float(lk0), float(l)
            lk0 = l
        return int(Itmax), 4, float(lk0), float(l)
    return predict


@pytest.mark.parametrize("kind", ["no-direction", "le", "ge-n0"])
def test_every_mutant_of_the_vb_rule_is_killed_by_the_case_list(kind, base):
    cases = S.vb_cases(base)
    killers = [c["id"] for c in cases
               if mutant(kind)(base, c["Tol"], c["n0"], c["Itmax"])[:2] != S.vb_predict(base, c["Tol"], c["n0"], c["Itmax"])[:2]]
    print(f"mutant {kind}: killed by", killers)
    assert killers
    # ... and the product's host loop sides with the rule, not with the mutant, on the first of them
    case = next(c for c in cases if c["id"] == killers[0])
    with pytest.raises(AssertionError):
        hold_host(case, base, predict=mutant(kind))
    hold_host(case, base)


# ---- ML likelihood loop -------------------------------------------------------------------------------------------------------
class MLRecorder(OracleMLEngine):
    def __init__(self, X, rank, start):
        super().__init__(X, rank)
        self.start, self.trace = start, []

    def ml_set_state(self, w, h):
        super().ml_set_state(*self.start)

    def ml_step(self, **kw):
        self.trace.append(super().ml_step(**kw))
        return self.trace[-1]


def host_ml(X, start, Tol, Itmax):
    """ccfindr_amd.factorize.factorize's host loop -> (it, the last likelihood, the likelihood of every step made)."""
    import importlib
    F = importlib.import_module("ccfindr_amd.factorize")
    made = []

    def factory(M, r):
        made.append(MLRecorder(X, r, start))
        return made[-1]

    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        res = F.factorize(X, ranks=[RANK], nrun=1, verbose=0, Itmax=Itmax, Tol=Tol, seed=1, engine_factory=factory)
    return res.nsteps[0][0], res.measure["likelihood"][0], np.array(made[0].trace)


def ml_problem(nan=False):
    X, _ = problem()
    rng = np.random.default_rng(12)
    w, h = rng.uniform(0.1, 1.0, size=(X.shape[0], RANK)), rng.uniform(0.1, 1.0, size=(RANK, X.shape[1]))
    if nan:
        w[5, 1] = np.nan
    else:
        # the rule has no n0, and from a random pair the relative change GROWS over the first nine steps: twelve steps on it
        # falls from step to step, so that a tolerance straddling step t is first met at step t
        from oracle import mlnmf_oracle as O
        for _ in range(12):
            o = O.nmf_update_literal(X, w, h)
            w, h = o["ew"], o["eh"]
    return np.asfortranarray(X), (w, h)


def test_ml_host_loop_stops_where_the_restated_rule_says():
    X, start = ml_problem()
    it, lk, col = host_ml(X, start, 0.0, 30)
    assert it == 30 and np.array_equal(col, host_ml(X, start, 0.0, 30)[2])
    for case in S.ml_cases(col):
        pred = S.ml_predict(col, case["Tol"], case["Itmax"])
        S.hold(case, col, pred)
        it, lk, trace = host_ml(X, start, case["Tol"], case["Itmax"])
        assert (it, lk) == (pred[0], pred[3]), (case["id"], it, pred)
        assert np.array_equal(trace, col[:it]), case["id"]


@pytest.mark.parametrize("Tol", [0.0, 1e-5, 1.0, float("inf")])
def test_ml_host_loop_nan_runs_to_itmax(Tol):
    X, start = ml_problem(nan=True)
    col = np.full(5, np.nan)
    assert S.ml_predict(col, Tol, 5)[:2] == (5, 4)
    from ccfindr_amd.factorize import factorize
    made = []

    def factory(M, r):
        made.append(MLRecorder(X, r, start))
        return made[-1]

    with warnings.catch_warnings(), np.errstate(all="ignore"), pytest.raises(FloatingPointError, match="NaN likelihood"):
        warnings.simplefilter("ignore")
        factorize(X, ranks=[RANK], nrun=1, verbose=0, Itmax=5, Tol=Tol, seed=1, engine_factory=factory)
    assert len(made[0].trace) == 5 and np.all(np.isnan(made[0].trace))          # every step made: the NaN never stopped the loop


# ---- the coupled projection -----------------------------------------------------------------------------------------------------
def vbp_problem():
    import util_vb_project_coupled as UC
    c = UC.case(1, 0.6, 3.0)
    c["lh_random"] = np.random.default_rng(101).uniform(0.05, 1.0, size=c["lh0"].shape)
    return c


@pytest.mark.parametrize("flags,n0,start", [((False, False), 5, "lh0"), ((True, True), 5, "lh0"), ((False, False), 2, "lh_random")])
def test_the_coupled_projection_restatement_stops_where_the_restated_rule_says(flags, n0, start):
    import util_vb_project_coupled as UC
    c = vbp_problem()
    run = lambda **kw: UC.project_coupled(c["x"], c["lw"], c["ew"], c[start], 1.0, 1.0, flags=flags, n0=kw.pop("n0", n0), **kw)
    col = run(Itmax=40, Tol=0.0)["history"][:, 0]
    falls = [t for t in range(2, 41) if not S.rising(col, t)]
    print(f"coupled projection, flags {flags}, n0 {n0}, start {start}: E falls at steps", falls)
    cases = S.vbp_cases(col, n0)
    if flags == (False, False):                                  # (with the flags on n0 moves the trajectory)
        cases += S.vbp_n0_cases(col, n0)
    if start == "lh_random":
        # the direction case: step 3 FALLS, past n0 = 2, and this rule stops there -- the VB loop's rule would pass it over
        assert falls[:2] == [2, 3]
        no, yes, d = S.vb_straddle(col, 3)
        cases.append(dict(id="vbp-falling-step-stops", Tol=yes, n0=2, Itmax=40, want=dict(it=3, reason=1, lk0_row=2)))
        assert S.vb_predict(col, yes, 2, 40)[0] != 3
    for case in cases:
        pred = S.vbp_predict(col, case["Tol"], case["n0"], case["Itmax"])
        S.hold_vbp(case, col, pred)
        w = run(Itmax=case["Itmax"], Tol=case["Tol"], n0=case["n0"])
        assert (w["it"], w["reason"], w["lk0"], w["E"]) == pred, (case["id"], pred)
        assert np.array_equal(w["history"][:, 0], col[:pred[0]]), case["id"]
