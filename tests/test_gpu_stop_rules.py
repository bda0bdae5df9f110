"""The stopping rules of the device-driven loops at their exact boundaries (csrc/kernels.h vb_control_step, csrc/mlnmf.h
ml_control_step, csrc/vbproject.h k_vbp_control; the hand-over to the host: csrc/loop.h drive_loop).

A run with Tol = 0 and history=True returns every step's evidence.  The rule is a few IEEE operations on those doubles, so
tests/util_stop_rules.py restates it exactly (tests/test_stop_rules_cpu.py holds that restatement to the product's host
loops) and every later run from the same start must
  - end on the predicted step, for the predicted reason, with the predicted lk0 and lkh -- equal, not close: the tolerances
    sit one ulp either side of a step's own relative change;
  - return the base history's first `it` rows bit for bit;
  - after a rule stop at step t, hold the state of a fresh run with Itmax = t, Tol = 0: the steps drive_loop had queued past
    the stop changed nothing.
There is no tolerance in this file.  Configurations: the control step folded into the next update and the separate control
kernel, a local group of three partitions, a batch of three engines; the ML likelihood loop the same four ways; the coupled
projection.  One 60 x 120 problem of rank 3 (rank 40 once, for the two-lanes-per-task update), at most 60 steps a run."""
import os

import numpy as np
import pytest

import util_stop_rules as S

pytestmark = pytest.mark.gpu

HY = {"aw": 1.0, "bw": 1.0, "ah": 1.0, "bh": 1.0}
OFF, ON = (False,) * 4, (True,) * 4
RANK, P = 3, 3


def same(a, b):
    """Equal bit for bit; NaNs in the same places (a NaN's own payload is not compared)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


def same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert same(a[k], b[k]), k


def with_fold(fold, make):
    """VBNMF_NO_CONTROL_FOLD is read when an engine is created."""
    old = os.environ.get("VBNMF_NO_CONTROL_FOLD")
    os.environ["VBNMF_NO_CONTROL_FOLD"] = "0" if fold else "1"
    try:
        return make()
    finally:
        if old is None:
            del os.environ["VBNMF_NO_CONTROL_FOLD"]
        else:
            os.environ["VBNMF_NO_CONTROL_FOLD"] = old


@pytest.fixture(scope="module")
def problem():
    import ccfindr_amd as C
    from ccfindr_amd import synth
    X = synth.drop_empty(synth.simulate_data(60, (40, 50, 30), seed=4, sparse=False))
    n, m = X.shape
    assert (n, m) == (60, 120)
    M = C.CountMatrix(X)
    yield {"M": M, "n": n, "m": m, "X": X}
    M.close()


def vb_start(pb, r=RANK, seed=3):
    from ccfindr_amd import synth
    return synth.random_state(pb["n"], pb["m"], r, HY, seed=seed)


# ---- the VB loop: one engine (fold / separate control kernel) or a local group -------------------------------------------------
class VBConfig:
    def __init__(self, pb, kind):
        self.pb, self.kind = pb, kind
        self.bases, self.states = {}, {}

    def run(self, wh, r, **kw):
        """One fresh engine (or group) from ``wh`` -> (the loop's result, the full state afterwards)."""
        import ccfindr_amd as C
        from ccfindr_amd.parallel import cell_partition
        M, m = self.pb["M"], self.pb["m"]
        if self.kind != "group3":
            eng = with_fold(self.kind == "fold", lambda: C.VBEngine(M, r))
            try:
                eng.set_state(wh["lw"], wh["lh"], wh["eh"])
                return eng.run(HY, history=True, **kw), eng.get_state()
            finally:
                eng.close()
        cuts = cell_partition(m, P)
        comm = C.Communicator.local(P)
        parts = [C.VBEngine(M, r, cols=c, m_global=m) for c in cuts]
        try:
            for p, (b, e) in zip(parts, cuts):
                p.attach_comm(comm)
                p.set_state(wh["lw"], wh["lh"][:, b:e], wh["eh"][:, b:e])
            comm.state_finish()
            out = comm.run(HY, history=True, **kw)
            sts = [p.get_state() for p in parts]
        finally:
            for p in parts:
                p.close()
            comm.close()
        for k in ("lw", "ew", "dw"):
            assert all(same(sts[0][k], q[k]) for q in sts[1:]), k            # the gene side is replicated bit for bit
        st = {k: sts[0][k] for k in ("lw", "ew", "dw")}
        st.update({k: np.concatenate([q[k] for q in sts], axis=1) for k in ("lh", "eh", "dh")})
        return out, st

    def base(self, name, wh, r, flags=OFF, n0=10, dn=1, Itmax=S.BASE_ITMAX, **kw):
        """The premise: the Tol = 0 run, made twice, returns the same history bit for bit."""
        if name not in self.bases:
            a = self.run(wh, r, Itmax=Itmax, Tol=0.0, n0=n0, dn=dn, flags=flags, **kw)[0]
            b = self.run(wh, r, Itmax=Itmax, Tol=0.0, n0=n0, dn=dn, flags=flags, **kw)[0]
            assert a["it"] == b["it"] and a["reason"] == b["reason"] and same(a["history"], b["history"]), name
            self.bases[name] = a
            col = a["history"][:, 0]
            falls = [t for t in range(2, len(col) + 1) if not S.rising(col, t)]
            print(f"[{self.kind}] base {name}: {a['it']} steps, reason {a['reason']}, evidence falls at steps {falls}")
        return self.bases[name]

    def state_at(self, name, wh, r, t, **kw):
        if (name, t) not in self.states:
            out, st = self.run(wh, r, Itmax=t, Tol=0.0, **kw)
            assert out["it"] == t and out["reason"] == 4
            self.states[(name, t)] = st
        return self.states[(name, t)]

    def hold(self, name, case, wh, r, flags=OFF, dn=1, **kw):
        """One case: the prediction is what the case requires, and the device does what is predicted."""
        hist = self.base(name, wh, r, flags=flags, **kw)["history"]
        col = hist[:, 0]
        pred = S.vb_predict(col, case["Tol"], case["n0"], case["Itmax"])
        S.hold(case, col, pred)
        loop = dict(n0=case["n0"], dn=dn, flags=flags, **kw)
        out, st = self.run(wh, r, Itmax=case["Itmax"], Tol=case["Tol"], **loop)
        got = (out["it"], out["reason"], out["lk0"], out["lkh"])
        print(f"[{self.kind}] {name} {case['id']}: Tol {case['Tol']!r} n0 {case['n0']} Itmax {case['Itmax']} -> {got}")
        assert got == pred, (self.kind, case["id"], got, pred)
        assert same(out["history"], hist[:pred[0]]), case["id"]
        if pred[1] == 2:
            same_state(st, self.state_at(name, wh, r, pred[0], **loop))
        return pred


@pytest.fixture(scope="module", params=["fold", "separate", "group3"])
def cfg(request, problem):
    return VBConfig(problem, request.param)


def test_vb_rule_cases_a_to_f(cfg, problem):
    wh = vb_start(problem)
    base = cfg.base("off", wh, RANK)
    assert base["it"] == S.BASE_ITMAX and base["reason"] == 4
    col = base["history"][:, 0]
    assert same(cfg.run(wh, RANK, Itmax=S.BASE_ITMAX, Tol=0.0, n0=3, dn=2, flags=OFF)[0]["history"], base["history"])   # flags off: no n0, dn
    print(f"[{cfg.kind}] d_t of the straddled steps:", {t: float(S.vb_rel(col[t - 1], col[t - 2])) for t in S.A_STEPS})
    print(f"[{cfg.kind}] d_t of steps 2..6:", [float(S.vb_rel(col[t - 1], col[t - 2])) for t in range(2, 7)])
    cases = S.vb_cases(col)
    for case in cases:
        cfg.hold("off", case, wh, RANK)
    # (d) where it can decide: thirty steps on the evidence rises at step 2, and a huge Tol ends the run there, not at step 1
    later = {k: v for k, v in cfg.run(wh, RANK, Itmax=30, Tol=0.0, flags=OFF)[1].items() if k in ("lw", "lh", "eh")}
    for case in S.first_step_cases(cfg.base("later", later, RANK)["history"][:, 0]):
        cfg.hold("later", case, later, RANK)


@pytest.mark.parametrize("n0,dn", [(3, 2), (5, 1)])
def test_vb_rule_with_the_hyper_update_on(cfg, problem, n0, dn):
    """Case (g): with the flags on the trajectory depends on (n0, dn); the base run shares the case's."""
    wh = vb_start(problem)
    name = f"on-{n0}-{dn}"
    base = cfg.base(name, wh, RANK, flags=ON, n0=n0, dn=dn)
    assert base["it"] == S.BASE_ITMAX and base["reason"] == 4
    col = base["history"][:, 0]
    assert not np.array_equal(base["history"][:, 5:], np.ones((S.BASE_ITMAX, 4)))       # the hyper-parameters did move
    steps = S.decisive_steps(col, n0, 2)                  # (the first two steps that decide a run with this n0)
    print(f"[{cfg.kind}] {name}: straddled steps and d_t", {t: float(S.vb_rel(col[t - 1], col[t - 2])) for t in steps})
    for case in S.straddle_cases(col, steps, n0, "g"):
        cfg.hold(name, case, wh, RANK, flags=ON, dn=dn)


def test_vb_nan_evidence_is_reason_1_also_on_itmax(cfg, problem):
    """Case (h): a whole factor row 0 with fudge = 0 (the state of test_gpu_control_fold's NaN test).  The first NaN step s ends
    the run with reason 1 -- also when s is Itmax; one step less is an ordinary Itmax."""
    wh = vb_start(problem, seed=6)
    wh["lw"][0, :] = 0.0
    base = cfg.base("nan", wh, RANK, Itmax=20, fudge=0.0)
    s, col = base["it"], base["history"][:, 0]
    print(f"[{cfg.kind}] first NaN step: {s}")
    assert base["reason"] == 1 and np.isnan(col[s - 1]) and np.all(np.isfinite(col[:s - 1]))
    for Itmax, reason in ((20, 1), (s, 1)) + (((s - 1, 4),) if s > 1 else ()):
        case = dict(id=f"h-Itmax={Itmax}", Tol=1e-5, n0=10, Itmax=Itmax, want={})
        pred = S.vb_predict(col, 1e-5, 10, Itmax)
        assert pred[:2] == (min(s, Itmax), reason)
        out = cfg.run(wh, RANK, Itmax=Itmax, Tol=1e-5, n0=10, dn=1, flags=OFF, fudge=0.0)[0]
        assert (out["it"], out["reason"], out["lk0"]) == pred[:3], (case["id"], out, pred)
        assert same([out["lkh"]], [pred[3]]) and same(out["history"], base["history"][:pred[0]])


def test_vb_rule_at_rank_40_where_two_lanes_share_a_task(problem):
    """One straddle with the fold carried by the two-lanes-per-task update: the first rising step from 9 on at which a run with
    n0 = t - 1 is decided by step t alone."""
    cfg = VBConfig(problem, "fold")
    wh = vb_start(problem, r=40, seed=5)
    col = cfg.base("r40", wh, 40)["history"][:, 0]
    t = next(t for t in range(9, 40) if S.rising(col, t) and S.vb_rel(col[t - 1], col[t - 2]) > 0)
    print("rank 40: straddled step", t, "d_t", float(S.vb_rel(col[t - 1], col[t - 2])))
    for case in S.straddle_cases(col, (t,), t - 1, "r40-"):
        pred = cfg.hold("r40", case, wh, 40)
        assert (pred[0] == t) == case["id"].endswith("yes")


# ---- a batch of three engines -------------------------------------------------------------------------------------------------
def test_vb_batch_engines_stop_each_where_its_own_history_says(problem):
    """Three engines stepped by one launch, shared Tol and n0: each stops where ITS base history predicts, one inside the first
    queued batch and one past the second; the batch goes on stepping around an engine that has stopped, and that engine's state
    stays the state of its stopping step."""
    import ccfindr_amd as C
    M, grid = problem["M"], C.batch_grid(3)
    a = vb_start(problem)
    eng = C.VBEngine(M, RANK)
    eng.set_state(a["lw"], a["lh"], a["eh"])
    assert eng.run(HY, Itmax=30, Tol=0.0, flags=OFF)["it"] == 30
    adv = eng.get_state(("lw", "lh", "eh"))
    eng.close()
    starts = [a, adv, vb_start(problem, seed=11)]

    def run(**kw):
        engs = [C.VBEngine(M, RANK, grid=grid) for _ in starts]
        try:
            for e, wh in zip(engs, starts):
                e.set_state(wh["lw"], wh["lh"], wh["eh"])
            outs = C.run_batch(engs, [HY] * 3, flags=OFF, history=True, **kw)
            return outs, [e.get_state() for e in engs]
        finally:
            for e in engs:
                e.close()

    base = run(Itmax=S.BASE_ITMAX, Tol=0.0)[0]
    again = run(Itmax=S.BASE_ITMAX, Tol=0.0)[0]
    for x, y in zip(base, again):
        assert x["it"] == y["it"] == S.BASE_ITMAX and same(x["history"], y["history"])
    cols = [b["history"][:, 0] for b in base]
    n0 = 2
    # the first step past 16 of engine 0 that a tolerance one ulp above its own change stops at
    t = next(t for t in range(17, 50) if S.rising(cols[0], t) and S.vb_predict(cols[0], S.vb_straddle(cols[0], t)[1], n0, 60)[0] == t)
    no, yes, d = S.vb_straddle(cols[0], t)
    print("batch: engine 0 straddled at step", t, "d_t", d)
    at = {}
    for tol in (yes, no):
        preds = [S.vb_predict(c, tol, n0, S.BASE_ITMAX) for c in cols]
        print("batch: Tol", repr(tol), "predicted", preds)
        assert min(p[0] for p in preds) <= 8 and max(p[0] for p in preds) > 16
        assert (preds[0][0] == t) == (tol == yes)
        outs, sts = run(Itmax=S.BASE_ITMAX, Tol=tol, n0=n0)
        for b, (out, st, pred) in enumerate(zip(outs, sts, preds)):
            assert (out["it"], out["reason"], out["lk0"], out["lkh"]) == pred, (b, out, pred)
            assert same(out["history"], base[b]["history"][:pred[0]]), b
            if pred[1] == 2:
                if pred[0] not in at:
                    at[pred[0]] = run(Itmax=pred[0], Tol=0.0)[1]
                same_state(st, at[pred[0]][b])


# ---- the ML likelihood loop ---------------------------------------------------------------------------------------------------
class MLConfig:
    """ml_run of one engine (fold / separate), run_batch_ml of three engines (the first is the one the cases are cut for), the
    partitioned loop of a local group.  run -> a list of (result, state) per engine."""

    def __init__(self, pb, kind):
        self.pb, self.kind = pb, kind

    def run(self, starts, **kw):
        import ccfindr_amd as C
        from ccfindr_amd.parallel import cell_partition
        M, m = self.pb["M"], self.pb["m"]
        if self.kind == "group3":
            w, h = starts[0]
            cuts = cell_partition(m, P)
            comm = C.Communicator.local(P)
            parts = [C.VBEngine(M, RANK, cols=c, m_global=m) for c in cuts]
            try:
                for p, (b, e) in zip(parts, cuts):
                    p.attach_comm(comm)
                    p.ml_set_state(w, h[:, b:e])
                comm.ml_state_finish()
                out = comm.ml_run(history=True, **kw)
                sts = [p.ml_get_state() for p in parts]
            finally:
                for p in parts:
                    p.close()
                comm.close()
            assert all(same(sts[0]["ew"], q["ew"]) for q in sts[1:])
            return [(out, {"ew": sts[0]["ew"], "eh": np.concatenate([q["eh"] for q in sts], axis=1)})]
        if self.kind == "batch3":
            engs = [C.VBEngine(M, RANK, grid=C.batch_grid(3)) for _ in starts]
            try:
                for e, (w, h) in zip(engs, starts):
                    e.ml_set_state(w, h)
                outs = C.run_batch_ml(engs, history=True, **kw)
                return [(o, e.ml_get_state()) for o, e in zip(outs, engs)]
            finally:
                for e in engs:
                    e.close()
        eng = with_fold(self.kind == "fold", lambda: C.VBEngine(M, RANK))
        try:
            eng.ml_set_state(*starts[0])
            return [(eng.ml_run(history=True, **kw), eng.ml_get_state())]
        finally:
            eng.close()


@pytest.fixture(scope="module")
def ml_starts(problem):
    """A random pair twelve steps on (the rule has no n0, and from a random pair the relative change grows over the first steps:
    later it falls from step to step, so a tolerance straddling step t is first met at step t); two more for the batch."""
    import ccfindr_amd as C
    rng = np.random.default_rng(12)
    n, m = problem["n"], problem["m"]
    pairs = [(rng.uniform(0.1, 1.0, size=(n, RANK)), rng.uniform(0.1, 1.0, size=(RANK, m))) for _ in range(3)]
    eng = C.VBEngine(problem["M"], RANK)
    out = []
    for k, (w, h) in enumerate(pairs):
        eng.ml_set_state(w, h)
        assert eng.ml_run(Itmax=(12, 40, 20)[k], Tol=0.0)["reason"] == 4
        st = eng.ml_get_state()
        out.append((st["ew"], st["eh"]))
    eng.close()
    return out


@pytest.mark.parametrize("prior", [False, True])
@pytest.mark.parametrize("kind", ["fold", "separate", "batch3", "group3"])
def test_ml_rule_straddles_and_limits(problem, ml_starts, kind, prior):
    cfg = MLConfig(problem, kind)
    kw = dict(prior=prior, gamma_a=1.3, gamma_b=0.8)
    base = cfg.run(ml_starts, Itmax=30, Tol=0.0, **kw)
    again = cfg.run(ml_starts, Itmax=30, Tol=0.0, **kw)
    for (x, _), (y, _) in zip(base, again):
        assert x["it"] == y["it"] == 30 and x["reason"] == 4 and same(x["history"], y["history"])
    cols = [b[0]["history"] for b in base]
    print(f"[ml {kind} prior={prior}] relative change at the straddled steps:",
          {t: float(abs(cols[0][t - 2] - cols[0][t - 1]) / abs(cols[0][t - 2])) for t in S.ML_STEPS})
    at = {}
    for case in S.ml_cases(cols[0]):
        preds = [S.ml_predict(c, case["Tol"], case["Itmax"]) for c in cols]
        S.hold(case, cols[0], preds[0])
        runs = cfg.run(ml_starts, Itmax=case["Itmax"], Tol=case["Tol"], **kw)
        print(f"[ml {kind} prior={prior}] {case['id']}: Tol {case['Tol']!r} ->", [(o["it"], o["reason"]) for o, _ in runs])
        for b, ((out, st), pred) in enumerate(zip(runs, preds)):
            assert (out["it"], out["reason"], out["lk"]) == (pred[0], pred[1], pred[3]), (case["id"], b, out, pred)
            assert same(out["history"], cols[b][:pred[0]]), (case["id"], b)
            if pred[1] == 2:
                if pred[0] not in at:
                    at[pred[0]] = cfg.run(ml_starts, Itmax=pred[0], Tol=0.0, **kw)
                same_state(st, at[pred[0]][b][1])


@pytest.mark.parametrize("kind", ["fold", "separate", "batch3", "group3"])
def test_ml_nan_never_satisfies_the_rule(problem, kind):
    """A NaN in w: the likelihood is NaN from step 1 on, no comparison with it is true, Itmax = 5 ends the run -- for every Tol."""
    rng = np.random.default_rng(4)
    n, m = problem["n"], problem["m"]
    starts = [(rng.uniform(size=(n, RANK)), rng.uniform(size=(RANK, m))) for _ in range(3)]
    starts[0][0][5, 1] = np.nan
    cfg = MLConfig(problem, kind)
    for Tol in (0.0, 1e-5, 1.0, float("inf")):
        out = cfg.run(starts, Itmax=5, Tol=Tol)[0][0]
        assert S.ml_predict(np.full(5, np.nan), Tol, 5)[:2] == (5, 4)
        assert (out["it"], out["reason"]) == (5, 4) and np.isnan(out["lk"]) and np.all(np.isnan(out["history"])), (Tol, out)


# ---- the coupled projection ---------------------------------------------------------------------------------------------------
VBP_KEYS = ("lh", "eh", "dh", "ev", "it", "reason", "hyper", "steps", "why", "E", "history")


@pytest.mark.parametrize("flags,n0,start", [((False, False), 5, "lh0"), ((True, True), 5, "lh0"), ((False, False), 2, "lh_random")])
def test_coupled_projection_rule(flags, n0, start):
    """vb_project(stop="global")'s loop at the ABI: straddles at n0 + 1 and at the next step that decides, Itmax on the stop step, n0 against n0 - 1,
    and -- from a random start, whose total evidence falls at steps 2 to 4 (tests/test_stop_rules_cpu.py finds the same on the
    CPU) -- a FALLING step past n0 that stops the run: this rule has no direction clause."""
    import importlib
    import ccfindr_amd as C
    import util_vb_project_coupled as UC
    proj = importlib.import_module("ccfindr_amd.project")
    c = UC.case(1, 0.6, 3.0)
    c["lh_random"] = np.random.default_rng(101).uniform(0.05, 1.0, size=c["lh0"].shape)
    M = C.CountMatrix(c["x"])

    def run(Itmax, Tol, n0=n0):
        return dict(zip(VBP_KEYS, proj.vb_project_coupled_columns(M, c["lw"], c["ew"], c[start], 1.0, 1.0, 0, c["x"].shape[1], flags,
                                                                  n0=n0, Itmax=Itmax, Tol=Tol, history_rows=Itmax)))
    try:
        base, again = run(40, 0.0), run(40, 0.0)
        assert base["steps"] == 40 and base["why"] == 4 and same(base["history"], again["history"])
        col = base["history"][:, 0]
        falls = [t for t in range(2, 41) if not S.rising(col, t)]
        print(f"coupled projection, flags {flags}, n0 {n0}, start {start}: E falls at steps {falls}; d_t",
              {t: float(S.vb_rel(col[t - 1], col[t - 2])) for t in (2, 3, n0, n0 + 1)})
        cases = S.vbp_cases(col, n0)
        if flags == (False, False):
            cases += S.vbp_n0_cases(col, n0)
        if start == "lh_random":
            assert falls[:2] == [2, 3]
            no, yes, d = S.vb_straddle(col, 3)
            cases.append(dict(id="vbp-falling-step-stops", Tol=yes, n0=2, Itmax=40, want=dict(it=3, reason=1, lk0_row=2)))
            cases.append(dict(id="vbp-falling-step-no", Tol=no, n0=2, Itmax=40, want=dict(not_it=3)))
            assert S.vb_predict(col, yes, 2, 40)[0] != 3                    # (the VB loop's rule passes that step over)
        at = {}
        for case in cases:
            pred = S.vbp_predict(col, case["Tol"], case["n0"], case["Itmax"])
            S.hold_vbp(case, col, pred)
            got = run(case["Itmax"], case["Tol"], case["n0"])
            print(f"coupled {case['id']}: Tol {case['Tol']!r} n0 {case['n0']} Itmax {case['Itmax']} ->", (got["steps"], got["why"], got["E"]))
            assert (got["steps"], got["why"], got["E"]) == (pred[0], pred[1], pred[3]), (case["id"], pred)
            assert np.all(got["it"] == pred[0]) and np.all(got["reason"] == pred[1])
            assert same(got["history"], base["history"][:pred[0]]), case["id"]
            if pred[1] == 1:
                key = (pred[0], case["n0"] if any(flags) else None)
                if key not in at:
                    at[key] = run(pred[0], 0.0, case["n0"])
                for k in ("lh", "eh", "dh", "ev"):
                    assert same(got[k], at[key][k]), (case["id"], k)
                assert got["hyper"] == at[key]["hyper"]
    finally:
        M.close()
