"""factorize()'s connectivity stopping rule (reference R/factorize.R:198-208) run inside the device loop
(vbnmf_engine_ml_run_connectivity, vbnmf_batch_ml_run_connectivity; csrc/mlnmf.h: MlConn) against the same rule stepped from
the host with ml_step() + cluster_changes().  Both run the same update kernels in the same order and count the changed pairs
in integers, so everything is compared with np.array_equal: iteration count, stop reason, likelihood history, the change
count of every step, the factors and the labels -- for stops inside, at and beyond the loop's batches of eight queued steps,
at ranks whose thread rows straddle wavefront boundaries, with the control step folded or not, one engine or a batch."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def counts(n, m, lam, seed):
    rng = np.random.default_rng(seed)
    X = rng.poisson(lam, size=(n, m)).astype(np.float64)
    X[np.arange(n), rng.integers(0, m, n)] += 1      # no empty rows
    X[rng.integers(0, n, m), np.arange(m)] += 1      # no empty columns
    return np.asfortranarray(X)


def uniform_state(n, m, r, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(size=(n, r)), rng.uniform(size=(r, m))


class _Env:
    """An environment switch the library reads when an engine (or its first layout) is made."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        os.environ[self.name] = self.value

    def __exit__(self, *a):
        if self.old is None:
            del os.environ[self.name]
        else:
            os.environ[self.name] = self.old


def host_loop(eng, w0, h0, ncnn_step, Itmax):
    """R/factorize.R:194-208 stepped from the host, as factorize(device_loop=False) does."""
    eng.ml_set_state(w0, h0)
    npair = eng.m * (eng.m - 1) // 2
    zstep, hist, chg, reason, it = 0, [], [], 4, 0
    for it in range(1, Itmax + 1):
        hist.append(eng.ml_step())
        n = eng.cluster_changes()[0]
        if n is None or it == 1:
            n = npair                                                    # :200
        chg.append(n)
        zstep = zstep + 1 if n == 0 else 0                               # :206-207
        if zstep == ncnn_step:                                           # :208
            reason = 2
            break
    st = eng.ml_get_state()
    return {"it": it, "reason": reason, "history": np.array(hist), "changes": np.array(chg, dtype=np.int64),
            "lk": hist[-1], "ew": st["ew"], "eh": st["eh"], "ids": eng.cluster_ids()}


def device_loop(eng, w0, h0, ncnn_step, Itmax):
    eng.ml_set_state(w0, h0)
    run = eng.ml_run(criterion="connectivity", ncnn_step=ncnn_step, Itmax=Itmax, history=True, changes=True)
    st = eng.ml_get_state()
    run.update(ew=st["ew"], eh=st["eh"], ids=eng.cluster_ids())
    return run


def same(a, b):
    assert a["it"] == b["it"] and a["reason"] == b["reason"], (a["it"], b["it"], a["reason"], b["reason"])
    assert np.array_equal(a["history"], b["history"])
    assert a["lk"] == b["lk"]
    if "changes" in a and "changes" in b:
        assert a["changes"].dtype == np.int64 and np.array_equal(a["changes"], b["changes"])
    assert np.array_equal(a["ew"], b["ew"]) and np.array_equal(a["eh"], b["eh"])
    if "ids" in a and "ids" in b:
        assert np.array_equal(a["ids"], b["ids"])


def _inputs(name):
    if name == "poisson":
        X = counts(50, 90, 0.8, seed=71)
        w0, h0 = uniform_state(50, 90, 3, seed=72)
        return X, w0, h0
    z = np.load(os.path.join(GOLD, "ml_traj_120x200_r3.npz"))
    return z["X"], z["w0"], z["h0"]


@pytest.fixture(scope="module", params=["poisson", "golden"])
def problem(request):
    """One matrix, one rank-3 engine on it and the start state; the host-stepped loops are kept per ncnn_step."""
    import ccfindr_amd as C
    X, w0, h0 = _inputs(request.param)
    M = C.CountMatrix(X)
    eng = C.VBEngine(M, 3)
    yield {"X": X, "M": M, "eng": eng, "w0": w0, "h0": h0}
    eng.close()
    M.close()


@pytest.mark.parametrize("s", range(1, 13))
def test_device_loop_equals_host_stepped_loop(problem, s):
    """Stops inside, at and beyond the batches of eight queued steps."""
    eng, w0, h0 = problem["eng"], problem["w0"], problem["h0"]
    dev = device_loop(eng, w0, h0, s, 400)
    assert eng.cluster_changes()[0] == 0                 # the run's last labels are the engine's previous labels
    host = host_loop(eng, w0, h0, s, 400)
    same(dev, host)
    m = eng.m
    assert dev["changes"][0] == m * (m - 1) // 2 and dev["changes"].shape == (dev["it"],)
    assert dev["it"] >= s + 1                            # the first step never counts towards zstep
    if dev["reason"] == 2:
        assert np.all(dev["changes"][-s:] == 0) and (dev["it"] == s + 1 or dev["changes"][-s - 1] != 0)


def test_itmax_before_the_stop(problem):
    eng, w0, h0 = problem["eng"], problem["w0"], problem["h0"]
    dev = device_loop(eng, w0, h0, 12, 10)               # twelve quiet steps cannot fit into ten
    assert dev["reason"] == 4 and dev["it"] == 10
    same(dev, host_loop(eng, w0, h0, 12, 10))


def test_iteration_counts_of_the_oracle():
    import ccfindr_amd as C
    from oracle import mlnmf_oracle as O
    X = counts(50, 90, 0.8, seed=71)
    rng = np.random.default_rng(9)
    M = C.CountMatrix(X)
    eng = C.VBEngine(M, 3)
    try:
        for irun in range(2):
            wh = O.init(50, 90, 3, rng)
            want = O.factorize_run(lambda a, b: O.nmf_update_literal(X, a, b), X, wh, Itmax=400, criterion="connectivity", ncnn_step=12)
            eng.ml_set_state(wh["ew"], wh["eh"])
            got = eng.ml_run(criterion="connectivity", ncnn_step=12, Itmax=400)
            assert got["it"] == want["it"], (irun, got["it"], want["it"])
    finally:
        eng.close()
        M.close()


@pytest.fixture(scope="module")
def wide():
    import ccfindr_amd as C
    X = counts(60, 150, 0.8, seed=5)
    M = C.CountMatrix(X)
    yield X, M
    M.close()


@pytest.mark.parametrize("r", [2, 5, 10, 13, 16, 33])
def test_thread_rows_across_wave_boundaries_and_lane_sharing(wide, r):
    """Padded ranks 2, 6, 10, 14, 16 and 40: rows of 6, 10 and 14 threads straddle wavefronts, 40 is the two-lanes-per-task sweep."""
    import ccfindr_amd as C
    X, M = wide
    w0, h0 = uniform_state(60, 150, r, seed=100 + r)
    eng = C.VBEngine(M, r)
    try:
        dev = device_loop(eng, w0, h0, 5, 60)
        host = host_loop(eng, w0, h0, 5, 60)
        same(dev, host)
        assert np.array_equal(dev["ids"], np.argmax(dev["eh"], axis=0) + 1)
    finally:
        eng.close()


def test_labels_after_a_run_and_an_exact_tie(problem):
    import ccfindr_amd as C
    eng, w0, h0 = problem["eng"], problem["w0"], problem["h0"]
    dev = device_loop(eng, w0, h0, 6, 400)
    assert dev["ids"].dtype == np.int32 and np.array_equal(dev["ids"], np.argmax(dev["eh"], axis=0) + 1)
    eng.ml_set_state(w0, h0)
    eng.ml_run(criterion="connectivity", ncnn_step=6, Itmax=400)
    assert eng.cluster_changes()[0] == 0
    # components 1 and 2 start identical (same column of w, same row of h): every update keeps them identical, so wherever
    # they lead a column the maximum is an exact tie, and which.max takes the first
    wt, ht = w0.copy(), h0.copy()
    wt[:, 1] = wt[:, 0]
    ht[1, :] = ht[0, :]
    dev = device_loop(eng, wt, ht, 6, 200)
    host = host_loop(eng, wt, ht, 6, 200)
    same(dev, host)
    tied = (dev["eh"][0] == dev["eh"][1]) & (dev["eh"][0] > dev["eh"][2])
    assert tied.any() and np.all(dev["ids"][tied] == 1) and not np.any(dev["ids"] == 2)


def test_internal_cell_order_does_not_move_the_counts():
    import ccfindr_amd as C
    X, w0, h0 = _inputs("poisson")
    runs = []
    for on in ("1", "0"):
        with _Env("VBNMF_CELL_ORDER", on):
            M = C.CountMatrix(X)
            eng = C.VBEngine(M, 3)                       # the order is fixed when the first layout is cut
        try:
            runs.append(device_loop(eng, w0, h0, 12, 400))
        finally:
            eng.close()
            M.close()
    a, b = runs
    assert a["it"] == b["it"] and a["reason"] == b["reason"]
    assert np.array_equal(a["changes"], b["changes"]) and np.array_equal(a["ids"], b["ids"])


def test_unfolded_control_step_is_identical(problem):
    import ccfindr_amd as C
    eng, w0, h0 = problem["eng"], problem["w0"], problem["h0"]
    with _Env("VBNMF_NO_CONTROL_FOLD", "1"):
        plain = C.VBEngine(problem["M"], 3)
    try:
        for s, Itmax in ((3, 400), (12, 400), (12, 10)):
            a = device_loop(plain, w0, h0, s, Itmax)
            assert plain.cluster_changes()[0] == 0
            same(a, device_loop(eng, w0, h0, s, Itmax))
    finally:
        plain.close()


@pytest.mark.parametrize("B", [1, 3, 8])
def test_batch_equals_single_engines_of_the_same_grid(B):
    import ccfindr_amd as C
    from ccfindr_amd.engine import batch_grid, run_batch_ml
    X = counts(50, 90, 0.8, seed=71)
    M = C.CountMatrix(X)
    engs = [C.VBEngine(M, 3, grid=batch_grid(B)) for _ in range(B)]
    try:
        starts = [uniform_state(50, 90, 3, seed=300 + b) for b in range(B)]
        alone = [device_loop(e, w, h, 8, 400) for e, (w, h) in zip(engs, starts)]
        for e, (w, h) in zip(engs, starts):
            e.ml_set_state(w, h)
        got = run_batch_ml(engs, Itmax=400, criterion="connectivity", ncnn_step=8, history=True)
        for e, g, a in zip(engs, got, alone):
            st = e.ml_get_state()
            g.update(ew=st["ew"], eh=st["eh"], ids=e.cluster_ids())
            assert e.cluster_changes()[0] == 0
            same(g, a)
        if B > 1:                                        # engines of one batch stop at different steps, each on its own
            assert len({g["it"] for g in got}) >= 2
    finally:
        for e in engs:
            e.close()
        M.close()


def test_driver_runs_the_rule_on_the_device():
    import ccfindr_amd as C
    from ccfindr_amd.engine import batch_grid
    from ccfindr_amd.factorize import init
    X = counts(50, 90, 0.8, seed=71)
    kw = dict(ranks=3, nrun=3, verbose=0, criterion="connectivity", ncnn_step=8, Itmax=400, seed=21)
    dev = C.factorize(X, device_loop=True, batch=1, **kw)
    host = C.factorize(X, device_loop=False, **kw)
    assert dev.nsteps == host.nsteps and sorted(dev.measure) == sorted(host.measure)
    for key in dev.measure:
        assert np.array_equal(np.asarray(dev.measure[key], dtype=float), np.asarray(host.measure[key], dtype=float), equal_nan=True), key
    assert np.array_equal(dev.basis[0], host.basis[0]) and np.array_equal(dev.coeff[0], host.coeff[0])
    # no batch unless asked for: the default is the single engine's result
    auto = C.factorize(X, device_loop=True, **kw)
    assert auto.nsteps == dev.nsteps and np.array_equal(auto.basis[0], dev.basis[0])
    # batch = 3: the three restarts one at a time on engines of the batch's grid
    bat = C.factorize(X, device_loop=True, batch=3, **kw)
    rng = np.random.default_rng(21)
    M = C.CountMatrix(X)
    eng = C.VBEngine(M, 3, grid=batch_grid(3))
    try:
        steps, best = [], None
        for irun in range(3):
            wh = init(50, 90, 3, rng)
            run = device_loop(eng, wh["ew"], wh["eh"], 8, 400)
            steps.append(run["it"])
            if best is None or run["lk"] > best["lk"]:
                best = run
    finally:
        eng.close()
        M.close()
    assert bat.nsteps[0] == steps
    assert bat.measure["likelihood"] == [best["lk"]]
    assert np.array_equal(bat.basis[0], best["ew"]) and np.array_equal(bat.coeff[0], best["eh"])
