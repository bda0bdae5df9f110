"""GPU parity of the VB projection of new cells onto a fitted posterior basis (ccfindr_amd.vb_project,
vbnmf_matrix_vb_project, csrc/vbproject.h) against tests/util_vb_project.py, the numpy restatement of reference
R/bayesian.R:71-95 and :345-347 that tests/test_vb_project_cpu.py ties to the committed oracle.

Tolerances (fp64), those of tests/test_gpu_project.py: one step on identical inputs -- factors max relative error <= 1e-12,
evidence relative error <= 1e-10; trajectories of tens of steps -- 1e-9.
"""
import functools
import glob
import importlib
import os

import numpy as np
import pytest

import util_vb_project as U

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STEP_GOLDENS = sorted(glob.glob(os.path.join(GOLD, "step_*.npz")))
EPS = U.EPS


def relerr(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def P():
    return importlib.import_module("ccfindr_amd.project")      # (the package attribute `project` is the function)


def posterior(n, r, rng):
    """q(W) drawn as alw ~ U(0.5, 6), bew ~ U(0.02, 0.3) -> (ew, sd, lw) as a fit stores and reads them."""
    from scipy.special import digamma
    alw = rng.uniform(0.5, 6.0, size=(n, r))
    bew = rng.uniform(0.02, 0.3, size=(n, r))
    return alw * bew, np.sqrt(alw) * bew, np.exp(digamma(alw)) * bew


def run_columns(X, lw, ew, lh0, ah, bh, **kw):
    """vb_project_columns over all cells of the dense X -> dict like the restatement's."""
    import ccfindr_amd as C
    M = C.CountMatrix(X)
    out = P().vb_project_columns(M, lw, ew, lh0, ah, bh, 0, X.shape[1], **kw)
    M.close()
    return dict(zip(("lh", "eh", "dh", "ev", "it", "reason"), out))


# ---- one iteration ----------------------------------------------------------------------------------------------------------
def test_the_step_goldens_are_there():
    names = [os.path.basename(p) for p in STEP_GOLDENS]
    assert len(names) == 7 and any("noninteger" in s for s in names) and any("fudge0" in s for s in names)


@pytest.mark.parametrize("path", STEP_GOLDENS, ids=[os.path.basename(p)[5:-4] for p in STEP_GOLDENS])
def test_one_iteration(path):
    """Itmax = 1 from the step_* goldens' (X, lw0, lh0, eh0, hyper, fudge).  (a) On a posterior made of the golden's lw0 and
    an ew of its own: lh, eh, dh against the restatement 1e-12, every cell's evidence 1e-10.  (b) VBEngine.step from the same
    state, then the kernel on (old lw, the engine's NEW ew, old lh): the engine's lh, eh, dh, 1e-12."""
    import ccfindr_amd as C
    z = np.load(path)
    X, lw0, lh0, eh0, fudge = z["X"], z["lw0"], z["lh0"], z["eh0"], float(z["fudge"])
    hy = dict(zip(("aw", "bw", "ah", "bh"), (float(v) for v in z["hyper"])))
    n, m = X.shape
    r = lw0.shape[1]
    eng = C.VBEngine(C.CountMatrix(X), r)
    eng.set_state(lw0, lh0, eh0)
    eng.step(hy, fudge)
    st = eng.get_state(("ew", "lh", "eh", "dh"))
    eng.close()
    got = run_columns(X, lw0, st["ew"], lh0, hy["ah"], hy["bh"], fudge=fudge, Itmax=1)
    cew = st["ew"].sum(axis=0)
    wl, we, wd, alh = U.h_half(X, lw0, cew, lh0, hy["ah"], hy["bh"], fudge)      # (the start as it is: no clip at this level)
    want = {"lh": wl, "eh": we, "dh": wd, "ev": U.cell_evidence(X, lw0, cew, wl, we, alh, hy["ah"], hy["bh"])}
    e_rest = [relerr(got[k], want[k]) for k in ("lh", "eh", "dh")]
    e_eng = [relerr(got[k], st[k]) for k in ("lh", "eh", "dh")]
    e_ev = relerr(got["ev"], want["ev"])
    print(os.path.basename(path), "lh/eh/dh vs restatement %.3g %.3g %.3g, vs VBEngine.step %.3g %.3g %.3g, evidence %.3g"
          % (*e_rest, *e_eng, e_ev))
    assert max(e_rest) <= 1e-12 and max(e_eng) <= 1e-12
    assert e_ev <= 1e-10
    assert np.all(got["it"] == 1) and np.all(got["reason"] == 4)
    # the public entry on a posterior given as (ew, sd): alw = 2.5 everywhere makes sd = ew / sqrt(2.5)
    assert r <= n and np.all(X.sum(axis=0) > 0)
    ew, hyp = st["ew"], {"ah": hy["ah"], "bh": hy["bh"]}
    p = C.vb_project(X, (ew, ew / np.sqrt(2.5)), hyper=hyp, Itmax=1, fudge=fudge, lh0=lh0)
    lw = C.posterior_basis((ew, ew / np.sqrt(2.5)), hyper=hyp, fudge=fudge)[0]
    w2 = U.project(X, lw, ew, lh0, hy["ah"], hy["bh"], fudge=fudge, Itmax=1)
    assert relerr(p.coeff[0], w2["eh"]) <= 1e-12 and relerr(p.lcoeff[0], w2["lh"]) <= 1e-12
    assert relerr(p.cell_evidence, w2["ev"]) <= 1e-10
    assert np.all(p.nsteps == 1) and np.all(p.reason == 4)
    d = run_columns(X, lw, ew, np.maximum(lh0, fudge), hy["ah"], hy["bh"], fudge=fudge, Itmax=1)
    assert np.array_equal(p.dcoeff[0], np.sqrt(d["dh"])) and relerr(d["dh"], w2["dh"]) <= 1e-12
    assert abs(p.lml_cells - p.cell_evidence.sum() / n / m) <= 1e-15 * abs(p.lml_cells)
    assert np.array_equal(C.cluster_id(p, rank=r), np.argmax(p.coeff[0], axis=0) + 1)
    assert p.ranks == [r] and p.hyper == hyp


# ---- column lengths around the workgroup's pass ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lengths_case(r):
    """n = 700.  Columns of 1, 2, 63, 64, 65 and 700 (= n) stored entries, of the counts just below, at and just above ONE pass
    of the kernel's workgroup and just above TWO -- from the kernel's own constant --, and of 3 and 200, in one matrix.  30 % of
    the gene rows are empty in every column short enough to leave them empty.  -> (X, lw, ew, lh0, lengths, restatement runs)."""
    per = P().vb_pass_entries(r)
    n = 700
    lengths = [1, 2, 63, 64, 65, n, per - 1, per, per + 1, 2 * per + 1, 3, 200]
    rng = np.random.default_rng(2000 + r)
    rows = rng.permutation(n)
    used, spare = rows[: (7 * n) // 10], rows[(7 * n) // 10:]
    X = np.zeros((n, len(lengths)))
    for j, L in enumerate(lengths):
        take = rng.permutation(used)[:L]
        if L > used.size:
            take = np.concatenate((used, rng.permutation(spare)[:L - used.size]))
        X[take, j] = rng.integers(1, 6, size=L)
    assert [int(v) for v in (X > 0).sum(axis=0)] == lengths
    ew, sd, lw = posterior(n, r, rng)
    lh0 = rng.uniform(0.05, 1.0, size=(r, len(lengths)))
    return X, lw, ew, lh0, lengths, {it: U.project(X, lw, ew, lh0, 1.0, 1.0, Itmax=it, Tol=0.0) for it in (1, 20)}


@pytest.mark.parametrize("r", [128, 33, 65, 10])
def test_column_lengths_around_the_pass(r):
    """One call over columns shorter than, equal to and longer than one and two passes of the workgroup (and of one entry, and
    of all n): one iteration 1e-12 / 1e-10, twenty iterations with Tol = 0 1e-9.  Ranks 33 and 65: two and four lanes share an
    entry."""
    X, lw, ew, lh0, lengths, want = lengths_case(r)
    for it, tol_h, tol_l in ((1, 1e-12, 1e-10), (20, 1e-9, 1e-9)):
        got = run_columns(X, lw, ew, lh0, 1.0, 1.0, Itmax=it, Tol=0.0)
        errs = [relerr(got[k], want[it][k]) for k in ("lh", "eh", "dh", "ev")]
        print(f"rank {r}, {it} iterations, lengths {lengths}: lh %.3g eh %.3g dh %.3g evidence %.3g" % tuple(errs))
        assert max(errs[:3]) <= tol_h and errs[3] <= tol_l
        assert np.all(got["it"] == it) and np.all(got["reason"] == 4)


# ---- stopping rule ----------------------------------------------------------------------------------------------------------
def counts(n, m, lam, seed):
    """Poisson(lam) counts; an empty column is given one count."""
    rng = np.random.default_rng(seed)
    X = rng.poisson(lam, size=(n, m)).astype(np.float64)
    for j in np.flatnonzero(X.sum(axis=0) == 0):
        X[rng.integers(0, n), j] = 1.0
    return np.asfortranarray(X)


@functools.lru_cache(maxsize=None)
def stop_case(seed, ah, bh):
    """90 x 140 Poisson(0.6), rank 5, q(W) from default_rng(seed), the default start -> (X, ew, sd, lw, the restatement's run to
    Tol = 1e-5 and its run cut at Itmax = 7)."""
    rng = np.random.default_rng(seed)
    X = counts(90, 140, 0.6, seed)
    ew, sd, lw = posterior(90, 5, rng)
    lh0 = U.default_start(X, ew)
    return X, ew, sd, lw, U.project(X, lw, ew, lh0, ah, bh, Tol=1e-5), U.project(X, lw, ew, lh0, ah, bh, Tol=1e-5, Itmax=7)


def check_stopping(seed, ah, bh):
    import ccfindr_amd as C
    X, ew, sd, lw, want, _ = stop_case(seed, ah, bh)
    clear = want["margin"] > 1e-3 * 1e-5
    held = int((want["lh"] == EPS).sum())
    print("seed %d, ah %g, bh %g: clear share %.4f, closest margin / Tol %.3g, iterations %d..%d (%d distinct), lh entries at fudge %d"
          % (seed, ah, bh, clear.mean(), want["margin"].min() / 1e-5, want["it"].min(), want["it"].max(),
             len(set(want["it"].tolist())), held))
    assert clear.mean() >= 0.95
    p = C.vb_project(X, (ew, sd), hyper={"ah": ah, "bh": bh}, Tol=1e-5)
    assert relerr(C.posterior_basis((ew, sd), hyper={"ah": ah, "bh": bh})[0], lw) <= 1e-12
    assert np.array_equal(p.nsteps[clear], want["it"][clear]) and np.array_equal(p.reason[clear], want["reason"][clear])
    assert np.all(p.reason[clear] == 1) and len(set(p.nsteps.tolist())) > 5
    errs = (relerr(p.lcoeff[0][:, clear], want["lh"][:, clear]), relerr(p.coeff[0][:, clear], want["eh"][:, clear]),
            relerr(p.cell_evidence[clear], want["ev"][clear]))
    print("lh %.3g, eh %.3g, evidence %.3g" % errs)
    assert max(errs) <= 1e-9
    return p, want


def test_stopping_rule_per_cell():
    """90 x 140, rank 5, ah = bh = 1, Tol = 1e-5, the default start, seed 65: nsteps and reason equal the restatement's in
    every cell whose decisions there were clear (| |1 - ev / lk0| - Tol | > 1e-3 Tol at every step), and at least 95 % of the
    cells are; lh, eh and the evidence there 1e-9."""
    check_stopping(65, 1.0, 1.0)


def test_itmax_ends_the_unconverged_cells():
    import ccfindr_amd as C
    X, ew, sd, lw, full, want = stop_case(65, 1.0, 1.0)
    p = C.vb_project(X, (ew, sd), hyper={"ah": 1.0, "bh": 1.0}, Tol=1e-5, Itmax=7)
    late = full["it"] > 7
    assert late.any()
    assert np.all(p.nsteps[late] == 7) and np.all(p.reason[late] == 4)
    clear = full["margin"] > 1e-3 * 1e-5
    early = ~late & clear
    assert early.any()
    assert np.array_equal(p.nsteps[early], full["it"][early]) and np.all(p.reason[early] == 1)
    assert relerr(p.coeff[0][:, early], full["eh"][:, early]) <= 1e-9
    assert np.array_equal(p.nsteps[clear], want["it"][clear])
    assert relerr(p.coeff[0][:, clear], want["eh"][:, clear]) <= 1e-9


def test_fudge_clip():
    """The same shape with ah = 0.02, bh = 0.5, seed 63: exp(psi(alh)) underflows the floor in components a cell does not use,
    so lh entries are held at fudge across the run.  The assertions of the stopping test, and some lcoeff entry equals fudge
    exactly."""
    p, want = check_stopping(63, 0.02, 0.5)
    assert (want["lh"] == EPS).any()
    assert (p.lcoeff[0] == EPS).any()


# ---- independence, bit for bit ----------------------------------------------------------------------------------------------
def bitwise_under_cut_and_permutation(X, lw, ew, lh0, cut, seed, **kw):
    import ccfindr_amd as C
    m = X.shape[1]
    whole = run_columns(X, lw, ew, lh0, 1.0, 1.0, **kw)
    M = C.CountMatrix(X)
    a = P().vb_project_columns(M, lw, ew, lh0[:, :cut], 1.0, 1.0, 0, cut, **kw)
    b = P().vb_project_columns(M, lw, ew, lh0[:, cut:], 1.0, 1.0, cut, m, **kw)
    M.close()
    for q, k in enumerate(("lh", "eh", "dh", "ev", "it", "reason")):
        assert np.array_equal(np.concatenate((a[q], b[q]), axis=-1), whole[k]), k
    perm = np.random.default_rng(seed).permutation(m)
    pp = run_columns(np.asfortranarray(X[:, perm]), lw, ew, lh0[:, perm], 1.0, 1.0, **kw)
    for k in ("lh", "eh", "dh", "ev", "it", "reason"):
        assert np.array_equal(pp[k], whole[k][..., perm]), k
    return whole


def test_halves_and_permutation_bitwise():
    """One call over all cells equals two calls cut at column 7 through col_begin / col_end, and a column permutation of X
    permutes lh, eh, dh, the evidence and nsteps exactly: a cell's sums do not depend on the grid or on its neighbours."""
    X, lw, ew, lh0, lengths, _ = lengths_case(33)
    rng = np.random.default_rng(9)
    X = np.concatenate((X, counts(X.shape[0], 300, 0.05, seed=10)), axis=1)
    lh0 = rng.uniform(0.05, 1.0, size=(33, X.shape[1]))
    whole = bitwise_under_cut_and_permutation(X, lw, ew, lh0, 7, 9, Itmax=40, Tol=1e-3)
    assert len(set(whole["it"].tolist())) > 3


# ---- more cells than workgroups: the persistent grid goes round ----------------------------------------------------------
def grid_workgroups():
    """Workgroups of the kernel's persistent grid: as many as the CUs hold threads for (project.hip, project_grid: CUs x 2048 / 256)."""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 8


@functools.lru_cache(maxsize=None)
def many_cells_case(r):
    """80 genes x 6000 short columns (1 to 40 stored entries, about 3 cells per workgroup of the grid); a third of the cells
    start far from their fixed point, so that iteration counts differ widely between the cells one workgroup takes in turn.
    -> (X, lw, ew, lh0, the restatement's run to Tol = 1e-4 within 60 steps and its 3-step run)."""
    n, m = 80, 6000
    rng = np.random.default_rng(700 + r)
    X = np.zeros((n, m))
    for j, L in enumerate(rng.integers(1, 41, size=m)):
        X[rng.permutation(n)[:L], j] = rng.integers(1, 6, size=L)
    ew, sd, lw = posterior(n, r, rng)
    lh0 = U.default_start(X, ew) * rng.uniform(0.5, 2.0, size=(r, m))
    lh0[:, ::3] = rng.uniform(1e-6, 10.0, size=lh0[:, ::3].shape)
    return (X, lw, ew, lh0, U.project(X, lw, ew, lh0, 1.0, 1.0, Itmax=60, Tol=1e-4),
            U.project(X, lw, ew, lh0, 1.0, 1.0, Itmax=3, Tol=0.0))


@pytest.mark.parametrize("r", [5, 65])
def test_workgroups_take_many_cells_in_turn(r):
    """More cells than twice the grid's workgroups, so that every workgroup draws several tickets and takes cells with
    different iteration counts one after the other: three iterations against the restatement (1e-9: a short trajectory), the
    stopping run's counts and reasons in the clear cells, and -- bit for bit -- the whole call against its halves and against a
    column permutation, which hands every cell to another workgroup behind another predecessor."""
    X, lw, ew, lh0, want, want3 = many_cells_case(r)
    m = X.shape[1]
    assert m > 2 * grid_workgroups(), (m, grid_workgroups())
    g3 = run_columns(X, lw, ew, lh0, 1.0, 1.0, Itmax=3, Tol=0.0)
    e3 = [relerr(g3[k], want3[k]) for k in ("lh", "eh", "dh", "ev")]
    print(f"rank {r}, {m} cells on {grid_workgroups()} workgroups, 3 iterations: lh %.3g eh %.3g dh %.3g evidence %.3g" % tuple(e3))
    assert max(e3) <= 1e-9
    clear = want["margin"] > 1e-3 * 1e-4
    whole = bitwise_under_cut_and_permutation(X, lw, ew, lh0, m // 2 + 17, r, Itmax=60, Tol=1e-4)
    print("iterations %d..%d, %d distinct; clear share %.4f" % (whole["it"].min(), whole["it"].max(), len(set(whole["it"].tolist())),
                                                                clear.mean()))
    assert len(set(whole["it"].tolist())) > 10 and clear.mean() >= 0.95
    assert np.array_equal(whole["it"][clear], want["it"][clear]) and np.array_equal(whole["reason"][clear], want["reason"][clear])
    assert relerr(whole["lh"][:, clear], want["lh"][:, clear]) <= 1e-9 and relerr(whole["eh"][:, clear], want["eh"][:, clear]) <= 1e-9
    assert relerr(whole["ev"][clear], want["ev"][clear]) <= 1e-9


# ---- non-finite input -------------------------------------------------------------------------------------------------------
def test_non_finite_input_ends_cells():
    """One NaN in a row of lw, Itmax = 5: the call returns status 0; every cell that stores that gene stops with reason 3
    within 5 steps; every other cell is bit for bit its result without the NaN (colSums(ew) holds no NaN: nothing of the
    gene's row reaches a cell that does not gather it)."""
    rng = np.random.default_rng(92)
    X = counts(60, 80, 0.3, seed=91)
    ew, sd, lw = posterior(60, 4, rng)
    lh0 = rng.uniform(0.05, 1.0, size=(4, 80))
    clean = run_columns(X, lw, ew, lh0, 1.0, 1.0, Itmax=5, Tol=1e-5)
    bad = lw.copy()
    bad[17, 2] = np.nan
    got = run_columns(X, bad, ew, lh0, 1.0, 1.0, Itmax=5, Tol=1e-5)             # (returns: status 0)
    touch = X[17] != 0
    assert touch.any() and not touch.all()
    assert np.all(got["reason"][touch] == 3) and np.all(got["it"][touch] >= 1) and np.all(got["it"][touch] <= 5)
    for k in ("lh", "eh", "dh", "ev", "it", "reason"):
        assert np.array_equal(got[k][..., ~touch], clean[k][..., ~touch]), k


# ---- an all-zero column, legal at the ABI level -----------------------------------------------------------------------------
def test_all_zero_column_at_the_abi_level():
    """Through CountMatrix and vb_project_columns a column without entries gives alh = ah: eh = ah beh and
    lh = max(exp(psi(ah)) beh, fudge), as the restatement; vb_project itself raises the reference's empty-columns error."""
    import ccfindr_amd as C
    from scipy.special import digamma
    rng = np.random.default_rng(31)
    X = counts(50, 20, 0.4, seed=30)
    X[:, 6] = 0.0
    ew, sd, lw = posterior(50, 3, rng)
    lh0 = rng.uniform(0.05, 1.0, size=(3, 20))
    ah, bh = 0.8, 1.7
    got = run_columns(X, lw, ew, lh0, ah, bh, Itmax=3, Tol=0.0)
    want = U.project(X, lw, ew, lh0, ah, bh, Itmax=3, Tol=0.0)
    beh = 1.0 / (ah / bh + ew.sum(axis=0))
    assert relerr(got["eh"][:, 6], ah * beh) <= 1e-12
    assert relerr(got["lh"][:, 6], np.maximum(np.exp(digamma(ah)) * beh, EPS)) <= 1e-12
    for k, tol in (("lh", 1e-9), ("eh", 1e-9), ("dh", 1e-9), ("ev", 1e-9)):
        assert relerr(got[k], want[k]) <= tol, k
    assert got["it"][6] == 3 and got["reason"][6] == 4
    with pytest.raises(ValueError, match="Input matrix contains empty columns"):
        C.vb_project(X, (ew, sd), hyper={"ah": ah, "bh": bh})


# ---- end to end -------------------------------------------------------------------------------------------------------------
def test_fit_on_a_subsample_then_place_the_rest():
    """The 450-cell, three-cluster simulate_data case of tests/test_gpu_project.py: vb_factorize() at rank 3 on the first 300
    cells, then vb_project() of the other 150 under the fitted posterior.  The projected cells' cluster_id equals the
    restatement's, run on the same posterior, cell for cell; against the planted clusters (through the label map the fit's own
    cells define) it agrees in the share the restatement reaches, which the test prints; every cell converges."""
    import ccfindr_amd as C
    from ccfindr_amd import synth
    seed, sizes = 5, (150, 150, 150)
    m = sum(sizes)
    deal = np.random.default_rng(1000 + seed).permutation(m)
    A = synth.simulate_data(200, sizes, seed=seed, sparse=False, shuffle=False)[:, deal]
    planted = np.repeat(np.arange(3), sizes)[deal]
    fit, new = np.asfortranarray(A[:, :300]), np.asfortranarray(A[:, 300:])
    assert fit.shape == (200, 300) and np.all(fit.sum(axis=1) > 0)
    assert np.all(fit.sum(axis=0) > 0) and np.all(new.sum(axis=0) > 0)
    res = C.vb_factorize(fit, ranks=3, nrun=2, verbose=0, progress_bar=False, seed=3)
    fit_ids = C.cluster_id(res, rank=3)
    relabel = np.array([np.bincount(planted[:300][fit_ids == k], minlength=3).argmax() if np.any(fit_ids == k) else -1
                        for k in (1, 2, 3)])
    p = C.vb_project(new, res, rank=3)
    ids = C.cluster_id(p, rank=3)
    lw, ew, ah, bh = C.posterior_basis(res, rank=3)
    assert (ah, bh) == (res.measure["ah"][0], res.measure["bh"][0])
    want = U.project(new, lw, ew, U.default_start(new, ew), ah, bh)
    want_ids = np.argmax(want["eh"], axis=0) + 1
    share = float(np.mean(relabel[want_ids - 1] == planted[300:]))
    print("restatement against the planted clusters: %.4f; fitted cells: %.4f; iterations %d..%d"
          % (share, float(np.mean(relabel[fit_ids - 1] == planted[:300])), p.nsteps.min(), p.nsteps.max()))
    assert np.array_equal(ids, want_ids)
    assert float(np.mean(relabel[ids - 1] == planted[300:])) == share
    assert np.all(p.reason == 1)
    assert np.array_equal(p.basis[0], res.basis[0]) and np.array_equal(p.dbasis[0], res.dbasis[0])
    own = C.vb_project(fit, res, rank=3)
    print("the fit's own 300 cells projected on its posterior: largest relative difference to the fit's coeff %.3g, in Frobenius"
          " norm %.3g; same cluster_id in %.4f of the cells"
          % (relerr(own.coeff[0], res.coeff[0]), np.linalg.norm(own.coeff[0] - res.coeff[0]) / np.linalg.norm(res.coeff[0]),
             float(np.mean(C.cluster_id(own, rank=3) == fit_ids))))
