"""Engine options in combination against the CPU oracles: the seeded covering set of tests/util_configs.py (one test per case, the
drawn configuration in every message), ML on the stretch-shaped matrices, partitioned groups, and the device's Gamma draws.

Every number is held to an independent statement of the step, never to another engine:
  * oracle.vbnmf_oracle (reference src/vbnmf_update.cpp) for VB steps -- lkh and the four statistics 1e-10 per step, the state
    1e-11 after the steps; loops (run, run_batch, a group's run) against test_gpu_device_loop.host_loop driving the oracle,
    history, hyper-parameters and final state 1e-9 (the device's Newton step has its own digamma / trigamma);
  * oracle.mlnmf_oracle (reference R/factorize.R:2-27, :40-49) for ML -- factors 1e-12 per step, 1e-10 over a run, the
    likelihood within 1e-10 of the size of its sums (test_gpu_random_cases.test_ml_step_random_case);
  * tests/util_philox.py (a numpy restatement of csrc/init.h) for random_state's draws, 1e-12.
With fudge = 0, lw / lh are held to max(bound, 2e-15 |psi(alpha)|) (util_configs.psi_bound)."""
import numpy as np
import pytest

import util_configs as U
from test_gpu_device_loop import host_loop
from test_gpu_random_cases import _counts as stretch_counts

pytestmark = pytest.mark.gpu


def _stats(ref):
    with np.errstate(divide="ignore"):
        return (np.mean(np.log(ref["lw"])), np.mean(np.log(ref["lh"])), np.mean(ref["ew"]), np.mean(ref["eh"]))


class _Oracle:
    """The dense literal oracle behind VBEngine.step's interface (host_loop drives it)."""

    def __init__(self, X, wh, fudge):
        self.X, self.ref, self.fudge = X, wh, fudge

    def step(self, hyper):
        from oracle import vbnmf_oracle as O
        self.ref = O.update_dense(self.X, self.ref, hyper, self.fudge)
        return self.ref["lkh"], _stats(self.ref)


def _close(a, b, tol):
    if np.isnan(b) or np.isinf(b):
        return a == b or (np.isnan(a) and np.isnan(b))
    return abs(a - b) <= tol * abs(b)


def _ml_scale(X, w, h):
    wh = w @ h
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.nansum(np.abs(X * np.log(wh))) + wh.sum()) / X.shape[0] / X.shape[1]


def _start(c, X, r, salt=0):
    from ccfindr_amd import synth
    return synth.random_state(X.shape[0], X.shape[1], r, c["hyper"], seed=c["state_seed"] + salt)


def _ml_start(c, X, r, salt=0):
    rng = np.random.default_rng(c["state_seed"] + salt)
    return rng.uniform(0.05, 1.0, size=(X.shape[0], r)), rng.uniform(0.05, 1.0, size=(r, X.shape[1]))


# ---- paths ----------------------------------------------------------------------------------------------------------------
def _vb_steps(tag, eng, X, wh, hy, fudge, steps):
    from oracle import vbnmf_oracle as O
    ref = wh
    for t in range(steps):
        lkh, st = eng.step(hy, fudge)
        ref = O.update_dense(X, ref, hy, fudge)
        assert _close(lkh, ref["lkh"], 1e-10), (tag, t, lkh, ref["lkh"])
        want = _stats(ref)
        for q in range(4):
            assert _close(st[q], want[q], 1e-10), (tag, t, q, st[q], want[q])
    U.check_factors(eng.get_state(), ref, 1e-11, fudge, tag)


def _loop_against_oracle(tag, out, X, wh, hy, fudge, lp, state):
    """One device loop's result ``out`` (and final ``state``) against host_loop over the oracle from ``wh``."""
    ora = _Oracle(X, wh, fudge)
    try:
        it, lk0, hyper, trace = host_loop(ora, dict(hy), lp["Itmax"], 0.0, lp["n0"], lp["dn"], lp["flags"])
    except (RuntimeError, ValueError):
        assert out is None or out["reason"] == 3, (tag, "the oracle's hyper-parameter update failed, the device's did not")
        return
    assert out is not None, (tag, "the device's hyper-parameter update failed, the oracle's did not")
    stopped = np.isnan(trace[-1, 0])
    assert out["it"] == it and out["reason"] == (1 if stopped else 4), (tag, out["it"], it, out["reason"])
    assert U.nan_relerr(out["history"], trace) <= 1e-9, (tag, U.nan_relerr(out["history"], trace))
    for k in ("aw", "bw", "ah", "bh"):
        assert _close(out["hyper"][k], hyper[k], 1e-9), (tag, k, out["hyper"][k], hyper[k])
    if not stopped:
        U.check_factors(state, ora.ref, 1e-9, fudge, tag)


def _run_vb_case(c, X, M):
    import ccfindr_amd as C
    tag, hy, fudge, r = U.case_id(c), c["hyper"], c["fudge"], c["rank"]
    path = c["path"]
    if path == "steps":
        eng = C.VBEngine(M, r, **U.engine_kw(c))
        wh = _start(c, X, r)
        eng.set_state(wh["lw"], wh["lh"], wh["eh"])
        _vb_steps(tag, eng, X, wh, hy, fudge, 3)
        eng.close()
    elif path == "init":
        from util_philox import random_state
        eng = C.VBEngine(M, r, **U.engine_kw(c))
        eng.random_state(hy, seed=c["init_seed"])
        st = eng.get_state()
        W, H = random_state(X.shape[0], X.shape[1], r, hy, c["init_seed"])
        assert U.relerr(st["lw"], W) <= 1e-12 and U.relerr(st["lh"], H) <= 1e-12, (tag, U.relerr(st["lw"], W), U.relerr(st["lh"], H))
        _vb_steps(tag, eng, X, {"lw": st["lw"], "lh": st["lh"], "eh": st["eh"]}, hy, fudge, 2)
        eng.close()
    elif path == "run":
        eng = C.VBEngine(M, r, **U.engine_kw(c))
        wh = _start(c, X, r)
        eng.set_state(wh["lw"], wh["lh"], wh["eh"])
        lp = c["loop"]
        try:
            out = eng.run(hy, Itmax=lp["Itmax"], Tol=0.0, n0=lp["n0"], dn=lp["dn"], flags=lp["flags"], fudge=fudge, history=True)
        except RuntimeError:
            out = None
        _loop_against_oracle(tag, out, X, wh, hy, fudge, lp, eng.get_state() if out else None)
        eng.close()
    elif path == "batch":
        lp, B = c["loop"], c["B"]
        hys = [dict(hy, aw=hy["aw"] * (1 + 0.03 * b), bh=hy["bh"] * (1 - 0.01 * b)) for b in range(B)]
        engs = [C.VBEngine(M, rb, **U.engine_kw(c)) for rb in c["ranks"]]
        whs = [_start(c, X, rb, salt=b) for b, rb in enumerate(c["ranks"])]
        for eng, wh in zip(engs, whs):
            eng.set_state(wh["lw"], wh["lh"], wh["eh"])
        outs = C.run_batch(engs, hys, Itmax=lp["Itmax"], Tol=0.0, n0=lp["n0"], dn=lp["dn"], flags=lp["flags"], fudge=fudge,
                           history=True)
        for b in range(B):
            out = outs[b] if outs[b]["reason"] != 3 else None
            _loop_against_oracle(f"{tag} engine {b} rank {c['ranks'][b]}", out, X, whs[b], hys[b], fudge, lp,
                                 engs[b].get_state() if out else None)
        for eng in engs:
            eng.close()
    elif path == "group":
        _group_against_oracle(tag, X, M, r, c["cuts"], hy, fudge, c["loop"], _start(c, X, r))


def _group_against_oracle(tag, X, M, r, cuts, hy, fudge, lp, wh):
    import ccfindr_amd as C
    m = X.shape[1]
    comm = C.Communicator.local(len(cuts))
    parts = [C.VBEngine(M, r, cols=cut, m_global=m) for cut in cuts]
    for p, (b, e) in zip(parts, cuts):
        p.attach_comm(comm)
        p.set_state(wh["lw"], wh["lh"][:, b:e], wh["eh"][:, b:e])
    comm.state_finish()
    try:
        out = comm.run(hy, Itmax=lp["Itmax"], Tol=0.0, n0=lp["n0"], dn=lp["dn"], flags=lp["flags"], fudge=fudge, history=True)
    except RuntimeError:
        out = None
    state = None
    if out is not None:
        st = [p.get_state() for p in parts]
        for q in st[1:]:
            for k in ("lw", "ew", "dw"):
                assert np.array_equal(st[0][k], q[k]), (tag, k)             # the gene side is replicated bit for bit
        state = {k: st[0][k] for k in ("lw", "ew", "dw")}
        state.update({k: np.concatenate([q[k] for q in st], axis=1) for k in ("lh", "eh", "dh")})
    _loop_against_oracle(tag, out, X, wh, hy, fudge, lp, state)
    for p in parts:
        p.close()
    comm.close()


def _ml_oracle_run(X, w, h, ml, steps):
    from oracle import mlnmf_oracle as O
    lks, scales = [], []
    for _ in range(steps):
        nx = O.nmf_update_literal(X, w, h, ml["prior"], ml["gamma_a"], ml["gamma_b"])
        w, h = nx["ew"], nx["eh"]
        lks.append(O.likelihood_literal(X, w, h))
        scales.append(_ml_scale(X, w, h))
    return w, h, np.array(lks), np.array(scales)


def _ml_steps(tag, eng, X, w, h, ml, steps=3):
    eng.ml_set_state(w, h)
    for t in range(steps):
        lk = eng.ml_step(ml["prior"], ml["gamma_a"], ml["gamma_b"])
        st = eng.ml_get_state()
        w1, h1, lks, scales = _ml_oracle_run(X, w, h, ml, 1)           # one oracle step from the device's previous pair
        assert U.relerr(st["ew"], w1) <= 1e-12 and U.relerr(st["eh"], h1) <= 1e-12, (
            tag, t, U.relerr(st["ew"], w1), U.relerr(st["eh"], h1))
        assert abs(lk - lks[0]) <= 1e-10 * scales[0], (tag, t, lk, lks[0], scales[0])
        w, h = st["ew"], st["eh"]


def _ml_run(tag, eng, X, w, h, ml, Itmax):
    eng.ml_set_state(w, h)
    out = eng.ml_run(Itmax=Itmax, Tol=0.0, prior=ml["prior"], gamma_a=ml["gamma_a"], gamma_b=ml["gamma_b"], history=True)
    _check_ml_run(tag, out, eng.ml_get_state(), X, w, h, ml, Itmax)


def _check_ml_run(tag, out, st, X, w, h, ml, Itmax):
    w1, h1, lks, scales = _ml_oracle_run(X, w, h, ml, Itmax)
    assert out["it"] == Itmax and out["reason"] == 4, (tag, out["it"], out["reason"])
    assert U.relerr(st["ew"], w1) <= 1e-10 and U.relerr(st["eh"], h1) <= 1e-10, (tag, U.relerr(st["ew"], w1), U.relerr(st["eh"], h1))
    assert np.all(np.abs(out["history"] - lks) <= 1e-10 * scales), (tag, np.max(np.abs(out["history"] - lks) / scales))


def _run_ml_case(c, X, M):
    import ccfindr_amd as C
    tag, r, ml = U.case_id(c), c["rank"], c["ml"]
    if c["path"] == "batch_ml":
        engs = [C.VBEngine(M, rb, **U.engine_kw(c)) for rb in c["ranks"]]
        starts = [_ml_start(c, X, rb, salt=b) for b, rb in enumerate(c["ranks"])]
        for eng, (w, h) in zip(engs, starts):
            eng.ml_set_state(w, h)
        Itmax = c["loop"]["Itmax"]
        outs = C.run_batch_ml(engs, Itmax=Itmax, Tol=0.0, prior=ml["prior"], gamma_a=ml["gamma_a"], gamma_b=ml["gamma_b"], history=True)
        for b, (eng, (w, h)) in enumerate(zip(engs, starts)):
            _check_ml_run(f"{tag} engine {b} rank {c['ranks'][b]}", outs[b], eng.ml_get_state(), X, w, h, ml, Itmax)
        for eng in engs:
            eng.close()
        return
    eng = C.VBEngine(M, r, **U.engine_kw(c))
    w, h = _ml_start(c, X, r)
    if c["path"] == "ml_steps":
        _ml_steps(tag, eng, X, w, h, ml)
    else:
        _ml_run(tag, eng, X, w, h, ml, c["loop"]["Itmax"])
    eng.close()


@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_config_sweep_case_against_the_oracle(case):
    """Each case creates its CountMatrix under its own switches (cell order, forced geometry): the switches are read when the
    matrix's first layout is cut."""
    import ccfindr_amd as C
    X = U.case_matrix(case)
    with U.switches(U.case_env(case)):
        M = C.CountMatrix(X)
        try:
            if case["path"] in U.ML_PATHS:
                _run_ml_case(case, X, M)
            else:
                _run_vb_case(case, X, M)
        finally:
            M.close()


# ---- ML on the stretch-shaped matrices ---------------------------------------------------------------------------------------
STRETCH_KINDS = ["all_ones", "all_twos", "ones_and_twos", "no_ones", "ones_then_big", "mixed"]


@pytest.mark.parametrize("kind", STRETCH_KINDS)
@pytest.mark.parametrize("r", [3, 10, 16, 28, 30, 40, 56, 80, 128])
def test_ml_on_the_leading_stretch_matrices(kind, r):
    """The ML sweep is the only one that runs its CELL side with the logarithm, so the only reader of the cell side's stretch
    of ones or twos (kernels.h TWO mode; layout slice_fast's high half).  Three ml_steps and an ml_run against the ML oracle;
    ranks <= 16 also through run_batch_ml at width 16.  The ranks cover both sweep loops and all three lane-sharing modes."""
    import ccfindr_amd as C
    n, m = 300, 460
    X = stretch_counts(kind, n, m, seed=len(kind) * 10 + r)
    ml = {"prior": r % 2 == 1, "gamma_a": 1.7, "gamma_b": 0.6}
    rng = np.random.default_rng(r)
    w, h = rng.uniform(0.05, 1.0, size=(n, r)), rng.uniform(0.05, 1.0, size=(r, m))
    M = C.CountMatrix(X)
    tag = f"ml {kind} r{r}"
    eng = C.VBEngine(M, r)
    _ml_steps(tag, eng, X, w, h, ml)
    _ml_run(tag, eng, X, w, h, ml, 4)
    eng.close()
    if r <= 16:
        rks = (r, max(1, r - 1), min(16, r + 1))
        engs = [C.VBEngine(M, rb, grid=C.batch_grid(3), pad_rank=16) for rb in rks]
        starts = [(w, h)] + [(rng.uniform(0.05, 1.0, size=(n, rb)), rng.uniform(0.05, 1.0, size=(rb, m))) for rb in rks[1:]]
        for eng, (w0, h0) in zip(engs, starts):
            eng.ml_set_state(w0, h0)
        outs = C.run_batch_ml(engs, Itmax=4, Tol=0.0, prior=ml["prior"], gamma_a=ml["gamma_a"], gamma_b=ml["gamma_b"], history=True)
        for b, (eng, (w0, h0)) in enumerate(zip(engs, starts)):
            _check_ml_run(f"{tag} batch engine {b}", outs[b], eng.ml_get_state(), X, w0, h0, ml, 4)
            eng.close()
    M.close()


# ---- partitioned groups against the oracle -----------------------------------------------------------------------------------
def _partition_matrix(kind, n, m, seed):
    """Counts of ``kind`` with no empty gene or cell; the columns from 2 m / 3 on hold entries in five genes only."""
    rng = np.random.default_rng(seed)
    X = rng.poisson(0.6, size=(n, m)).astype(np.float64)
    X[5:, 2 * m // 3:] = 0.0
    X[rng.integers(0, 5, m), np.arange(m)] += 1.0
    X[np.arange(n), rng.integers(0, 2 * m // 3, n)] += 1.0
    if kind == "binary":
        X = (X > 0).astype(np.float64)
    elif kind == "twos":
        X = 2.0 * (X > 0)
    elif kind == "noninteger":
        X = X * rng.uniform(0.5, 1.5, size=(1, m))
    elif kind == "split":
        X[n // 3, m // 2] = 16384.0
        X[n // 2, m // 4] = 20017.0
    return np.asfortranarray(X)


@pytest.mark.parametrize("kind", ["counts", "noninteger", "split", "binary", "twos"])
@pytest.mark.parametrize("r", [1, 3, 17, 40, 80])
def test_partitioned_group_against_the_oracle(kind, r):
    """Twelve steps of a local group's device loop (hyper-parameter updates from step 4) against host_loop over the oracle:
    P = 2, 3 or 8 partitions, one of them a single cell, one of them cells whose entries sit in five of the genes."""
    import ccfindr_amd as C
    from ccfindr_amd import synth
    n, m = 120, 211
    X = _partition_matrix(kind, n, m, seed=r + len(kind))
    P = (2, 3, 8)[(r + len(kind)) % 3]
    third = 2 * m // 3
    if P > 2:
        cuts = [(0, 1)] + [(1 + (third - 1) * q // (P - 2), 1 + (third - 1) * (q + 1) // (P - 2)) for q in range(P - 2)] + [(third, m)]
    else:
        cuts = [(0, 1), (1, m)]
    hy = {"aw": 1.2, "bw": 0.9, "ah": 0.8, "bh": 1.5}
    wh = synth.random_state(n, m, r, hy, seed=r)
    M = C.CountMatrix(X)
    lp = {"Itmax": 12, "n0": 3, "dn": 1, "flags": (True,) * 4}
    _group_against_oracle(f"group {kind} r{r} P{P}", X, M, r, cuts, hy, C.EPS, lp, wh)
    M.close()


# ---- device initialisation against the restatement -------------------------------------------------------------------------
@pytest.mark.parametrize("a", [0.05, 0.3, 1.0, 12.0])
def test_device_gamma_draws_match_the_restatement(a):
    """random_state's draws within 1e-12 of tests/util_philox.py: plain, padded (pad_rank), cell order on, a partition
    (col_begin), and two seeds that differ only in their high 32 bits; then two steps from the drawn state (get_state)
    against the oracle."""
    import ccfindr_amd as C
    from util_philox import random_state
    n, m = 90, 170
    rng = np.random.default_rng(int(a * 100))
    X = rng.poisson(0.5, size=(n, m)).astype(np.float64)
    X[np.arange(n), rng.integers(0, m, n)] += 1.0
    X[rng.integers(0, n, m), np.arange(m)] += 1.0
    X = np.asfortranarray(X)
    hy = {"aw": a, "bw": 1.3, "ah": a, "bh": 0.7}
    seeds = (0x0123456789ABCDEF, 0x0123456789ABCDEF ^ (0x5A5A << 40))
    for order in (0, 1):
        with U.switches({"VBNMF_CELL_ORDER": str(order)}):
            M = C.CountMatrix(X)
            for r, kw in ((5, {}), (5, {"pad_rank": 16}), (7, {"pad_rank": 8}), (33, {})):
                for seed in seeds:
                    tag = (a, order, r, kw, hex(seed))
                    eng = C.VBEngine(M, r, **kw)
                    eng.random_state(hy, seed=seed)
                    st = eng.get_state()
                    W, H = random_state(n, m, r, hy, seed)
                    assert U.relerr(st["lw"], W) <= 1e-12 and U.relerr(st["lh"], H) <= 1e-12, (tag, U.relerr(st["lw"], W), U.relerr(st["lh"], H))
                    assert np.array_equal(st["ew"], st["lw"]) and np.array_equal(st["eh"], st["lh"]) and not st["dh"].any()
                    if seed == seeds[0]:
                        _vb_steps(tag, eng, X, {"lw": st["lw"], "lh": st["lh"], "eh": st["eh"]}, hy, C.EPS, 2)
                    eng.close()
            b, e = 61, 150
            part = C.VBEngine(M, 6, cols=(b, e), m_global=m)
            part.random_state(hy, seed=seeds[1])
            W, H = random_state(n, e - b, 6, hy, seeds[1], col_begin=b)
            st = part.get_state(("lw", "lh"))
            assert U.relerr(st["lw"], W) <= 1e-12 and U.relerr(st["lh"], H) <= 1e-12, (a, order, "partition")
            part.close()
            M.close()
