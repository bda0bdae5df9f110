"""VB projection of new cells onto a fitted posterior basis (ccfindr_amd.vb_project, vbnmf_matrix_vb_project), the parts that
need no GPU: the numpy restatement the GPU tests compare against (tests/util_vb_project.py) is tied to the committed oracle,
``posterior_basis`` rebuilds the oracle's lw from what a fit stores, and the argument checks of the Python entry and of the
C ABI."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.special import gammaln

import util_vb_project as U

HYPER = {"aw": 0.7, "bw": 1.3, "ah": 0.9, "bh": 1.1}


def relerr(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def oracle_step(hyper, seed=11, n=40, m=30, r=3):
    """One oracle.vbnmf_oracle.update_dense step from a random state -> (X, old state, new state)."""
    from oracle import vbnmf_oracle as O
    rng = np.random.default_rng(seed)
    X = rng.poisson(1.2, size=(n, m)).astype(np.float64)
    X[np.arange(n), rng.integers(0, m, n)] += 1
    X[rng.integers(0, n, m), np.arange(m)] += 1
    wh = O.vb_init_random(n, m, r, hyper, rng)
    return X, wh, O.update_dense(X, wh, hyper)


def test_h_half_is_the_oracles_h_half():
    """The restatement's h_half on (old lw, colSums of the oracle's NEW ew, old lh) against the oracle's lh, eh, dh: 1e-13."""
    X, old, new = oracle_step(HYPER)
    lh, eh, dh, _ = U.h_half(X, old["lw"], new["ew"].sum(axis=0), old["lh"], HYPER["ah"], HYPER["bh"])
    errs = relerr(lh, new["lh"]), relerr(eh, new["eh"]), relerr(dh, new["dh"])
    print("lh %.3g, eh %.3g, dh %.3g" % errs)
    assert max(errs) <= 1e-13


def test_cell_evidence_plus_u2_is_the_oracles_evidence():
    """sum_j cell_evidence at the oracle's new state plus U2 (R/bayesian.R:92-93) against lkh n m: 1e-12."""
    X, old, new = oracle_step(HYPER)
    n, m = X.shape
    aw, bw, ah, bh = (HYPER[k] for k in ("aw", "bw", "ah", "bh"))
    cew = new["ew"].sum(axis=0)
    lh, eh, dh, alh = U.h_half(X, old["lw"], cew, old["lh"], ah, bh)
    cells = U.cell_evidence(X, new["lw"], cew, lh, eh, alh, ah, bh)
    bew = 1.0 / (aw / bw + np.tile(old["eh"].sum(axis=1), (n, 1)))                       # :76
    alw = new["ew"] / bew                                                                # :77
    u2 = -(aw / bw) * new["ew"] - gammaln(aw) + aw * np.log(aw / bw) + alw * (1 + np.log(bew)) + gammaln(alw)
    total = cells.sum() + u2.sum()
    print("sum of cells + U2 %.15g, lkh n m %.15g" % (total, new["lkh"] * n * m))
    assert abs(total / (new["lkh"] * n * m) - 1) <= 1e-12


@pytest.mark.parametrize("aw", [0.7, 0.02])
def test_posterior_basis_rebuilds_lw(aw):
    """lw from (ew, sqrt(dw)) as a fit stores them against the oracle's own lw: 1e-12 (3 ulp in alw = (ew / sd)^2 times the
    sensitivity a psi'(a) <~ 1 / a of exp(psi(a)), for aw >= 0.02); ah, bh from measure."""
    import ccfindr_amd as C
    hyper = dict(HYPER, aw=aw)
    X, old, new = oracle_step(hyper, seed=12)
    res = C.VBResult(ranks=[2, 3], basis=[None, new["ew"]], dbasis=[None, np.sqrt(new["dw"])], coeff=[None, new["eh"]],
                     dcoeff=[None, np.sqrt(new["dh"])],
                     measure={"rank": [2, 3], "lml": [0.0, 0.0], "aw": [1.0, aw], "bw": [1.0, 1.3], "ah": [1.0, 0.9], "bh": [1.0, 1.1],
                              "nunif": [0, 0]})
    lw, ew, ah, bh = C.posterior_basis(res, rank=3)
    err = relerr(lw, new["lw"])
    print("aw = %g: lw %.3g, smallest alw %.3g" % (aw, err, float((new["ew"] ** 2 / new["dw"]).min())))
    assert err <= 1e-12
    assert np.array_equal(ew, new["ew"]) and (ah, bh) == (0.9, 1.1)
    lw2, _, ah2, bh2 = C.posterior_basis((new["ew"], np.sqrt(new["dw"])), hyper={"ah": 2.0, "bh": 3.0})
    assert np.array_equal(lw2, lw) and (ah2, bh2) == (2.0, 3.0)


def test_restatement_loop_stops_per_cell():
    """Every cell of the restatement's loop carries its own count and reason: no cell stops at step 1, Itmax ends the
    unconverged ones with 4, a NaN start ends its cell with 3 at the first step and leaves the other cells as they are."""
    X, old, new = oracle_step(HYPER, seed=13)
    lw, ew = new["lw"], new["ew"]
    lh0 = U.default_start(X, ew)
    full = U.project(X, lw, ew, lh0, 0.9, 1.1, Itmax=2000)
    assert set(np.unique(full["reason"])) <= {1, 4} and np.all(full["it"] >= 2)
    cut = U.project(X, lw, ew, lh0, 0.9, 1.1, Itmax=4)
    late = full["it"] > 4
    assert late.any() and np.all(cut["it"][late] == 4) and np.all(cut["reason"][late] == 4)
    assert np.array_equal(cut["it"][~late], full["it"][~late])
    bad = lh0.copy()
    bad[1, 3] = np.nan
    nan = U.project(X, lw, ew, bad, 0.9, 1.1, Itmax=4)
    assert nan["reason"][3] == 3 and nan["it"][3] == 1
    keep = np.arange(X.shape[1]) != 3
    assert np.array_equal(nan["lh"][:, keep], cut["lh"][:, keep]) and np.array_equal(nan["it"][keep], cut["it"][keep])


def test_argument_errors():
    """Everything is refused before any device call (this test runs without a GPU)."""
    import ccfindr_amd as C
    import importlib
    P = importlib.import_module("ccfindr_amd.project")
    rng = np.random.default_rng(5)
    X = rng.poisson(1.0, size=(12, 9)).astype(np.float64) + np.eye(12, 9)
    ew = rng.uniform(0.1, 1.0, size=(12, 3))
    sd = rng.uniform(0.1, 1.0, size=(12, 3))
    hy = {"ah": 1.0, "bh": 1.0}
    measure = {"rank": [3], "ah": [1.0], "bh": [1.0]}
    res = C.VBResult(ranks=[3], basis=[ew], dbasis=[sd], measure=measure)
    # posterior_basis
    with pytest.raises(ValueError, match="MLResult"):
        C.posterior_basis(C.MLResult(ranks=[3], basis=[ew], coeff=[None]))
    with pytest.raises(ValueError, match="dbasis"):
        C.posterior_basis(C.VBResult(ranks=[3], basis=[ew], dbasis=[], measure=measure))
    with pytest.raises(ValueError, match="positive"):
        C.posterior_basis((ew, np.where(sd > 0.5, sd, 0.0)), hyper=hy)
    with pytest.raises(ValueError, match="positive"):
        C.posterior_basis((-ew, sd), hyper=hy)
    with pytest.raises(ValueError, match="shape"):
        C.posterior_basis((ew, sd[:, :2]), hyper=hy)
    with pytest.raises(ValueError, match="hyper"):
        C.posterior_basis((ew, sd))
    with pytest.raises(ValueError, match="> 0"):
        C.posterior_basis((ew, sd), hyper={"ah": 0.0, "bh": 1.0})
    with pytest.raises(IndexError, match="subscript out of bounds"):
        C.posterior_basis(res, rank=5)
    two = C.VBResult(ranks=[2, 3], basis=[ew[:, :2], ew], dbasis=[sd[:, :2], sd], measure={"rank": [2, 3], "ah": [1.0, 1.0], "bh": [1.0, 1.0]})
    with pytest.raises(ValueError, match="rank="):
        C.posterior_basis(two)
    # vb_project: the checks of project()
    with pytest.raises(ValueError, match="rows"):
        C.vb_project(X[:11], res)
    with pytest.raises(ValueError, match="exceeds"):
        C.vb_project(X[:2], (ew[:2], sd[:2]), hyper=hy)
    Z = X.copy()
    Z[:, 4] = 0.0
    for mat in (Z, sp.csc_matrix(Z), C.CountMatrix(Z)):
        with pytest.raises(ValueError, match="Input matrix contains empty columns"):
            C.vb_project(mat, res)
    with pytest.raises(ValueError, match="lh0"):
        C.vb_project(X, res, lh0=np.ones((3, 8)))
    with pytest.raises(ValueError, match="Itmax"):
        C.vb_project(X, res, Itmax=0)
    with pytest.raises(IndexError):
        C.vb_project(X, res, rank=4)
    M = C.CountMatrix(X)
    shell = C.CountMatrix.shell(M.meta())
    with pytest.raises(ValueError, match="shell"):
        C.vb_project(shell, res)
    # the C entry itself: a status and a message
    lh = np.ones((3, 9))
    with pytest.raises(C.VBNMFError) as ei:
        P.vb_project_columns(shell, ew, ew, lh, 1.0, 1.0, 0, 9)
    assert ei.value.code == 1 and "shell" in str(ei.value)
    for cb, ce in ((0, 0), (4, 3), (0, 10), (-1, 3)):
        with pytest.raises(C.VBNMFError) as ei:
            P.vb_project_columns(M, ew, ew, lh, 1.0, 1.0, cb, ce)
        assert ei.value.code == 1
    with pytest.raises(C.VBNMFError) as ei:
        P.vb_project_columns(M, ew, ew, lh, 1.0, 1.0, 0, 9, Itmax=0)
    assert ei.value.code == 1
    for ah, bh in ((0.0, 1.0), (1.0, -1.0), (float("nan"), 1.0)):
        with pytest.raises(C.VBNMFError) as ei:
            P.vb_project_columns(M, ew, ew, lh, ah, bh, 0, 9)
        assert ei.value.code == 1
    L = C.load()
    N = C._native
    h = np.ones((3, 9), order="F")
    wf = np.asfortranarray(ew)
    tail = (10, 1e-5, 0, None, None, None)
    f = L.vbnmf_matrix_vb_project
    assert f(M._h, 0, 9, 0, N.dptr(wf), N.dptr(wf), 1.0, 1.0, 0.0, N.dptr(h), None, None, *tail) == 1             # r < 1
    assert f(M._h, 0, 9, N.MAX_RANK + 1, N.dptr(wf), N.dptr(wf), 1.0, 1.0, 0.0, N.dptr(h), None, None, *tail) == 1
    assert f(M._h, 0, 9, 3, None, N.dptr(wf), 1.0, 1.0, 0.0, N.dptr(h), None, None, *tail) == 1                   # NULL lw
    assert f(M._h, 0, 9, 3, N.dptr(wf), None, 1.0, 1.0, 0.0, N.dptr(h), None, None, *tail) == 1                   # NULL ew
    assert f(M._h, 0, 9, 3, N.dptr(wf), N.dptr(wf), 1.0, 1.0, 0.0, None, None, None, *tail) == 1                  # NULL lh
    assert f(None, 0, 9, 3, N.dptr(wf), N.dptr(wf), 1.0, 1.0, 0.0, N.dptr(h), None, None, *tail) == 1
    M.close()


def test_no_device_is_a_status():
    import ccfindr_amd as C
    if C.load().vbnmf_device_count() > 0:
        pytest.skip("a GPU is present")
    rng = np.random.default_rng(6)
    X = rng.poisson(1.0, size=(12, 9)).astype(np.float64) + np.eye(12, 9)
    pair = rng.uniform(0.1, 1.0, size=(12, 3)), rng.uniform(0.1, 1.0, size=(12, 3))
    with pytest.raises(C.VBNMFError) as ei:
        C.vb_project(X, pair, hyper={"ah": 1.0, "bh": 1.0})
    assert ei.value.code == 2 and "no CPU fallback" in str(ei.value)


def test_kernel_constants_are_exported():
    """Entries of a cell per pass of the kernel's 256 threads: those of the ML projection kernel."""
    import ctypes
    import importlib
    import ccfindr_amd as C
    P = importlib.import_module("ccfindr_amd.project")
    L = C.load()
    for r, per in ((1, 256), (10, 256), (32, 256), (33, 128), (64, 128), (65, 64), (128, 64)):
        e = ctypes.c_int32()
        assert L.vbnmf_vb_project_info(r, ctypes.byref(e), None) == 0
        assert e.value == per == P.vb_pass_entries(r)
    assert L.vbnmf_vb_project_info(0, None, None) == 1
    assert P.vb_last_kernel_ms() >= 0.0
