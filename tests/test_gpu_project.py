"""GPU parity of the projection of new cells onto a fitted basis (ccfindr_amd.project, vbnmf_matrix_project, csrc/project.h)
against tests/util_project.py, the numpy restatement of reference R/factorize.R:8-15, :40-49 and :208 that
tests/test_project_cpu.py ties to the committed oracle.

Tolerances (fp64), those of tests/test_gpu_mlnmf.py: one step on identical inputs -- factors max relative error <= 1e-12,
likelihood relative error <= 1e-10; trajectories of tens of steps -- 1e-9.
"""
import functools
import os

import numpy as np
import pytest

import util_project as U

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def relerr(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def counts(n, m, lam, seed):
    rng = np.random.default_rng(seed)
    X = rng.poisson(lam, size=(n, m)).astype(np.float64)
    X[np.arange(n), rng.integers(0, m, n)] += 1      # no empty rows
    X[rng.integers(0, n, m), np.arange(m)] += 1      # no empty columns
    return np.asfortranarray(X)


# ---- one iteration ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,prior,ga,gb", [("sparse5pct_300x400_r10", False, 1.0, 1.0), ("dense_64x96_r4", False, 1.0, 1.0),
                                             ("rank1_50x70_r1", False, 1.0, 1.0), ("noninteger_80x150_r5", False, 1.0, 1.0),
                                             ("prior_90x140_r5", True, 2.0, 0.5)])
def test_one_iteration(name, prior, ga, gb):
    """Itmax = 1 from the ml_step_* goldens' (X, w0, h0): H against the restatement's H half AND against the H that
    VBEngine.ml_step leaves from the same pair, 1e-12; every cell's likelihood against the restatement's, 1e-10."""
    import ccfindr_amd as C
    z = np.load(os.path.join(GOLD, f"ml_step_{name}.npz"))
    X, w0, h0 = z["X"], z["w0"], z["h0"]
    p = C.project(X, w0, prior=prior, gamma_a=ga, gamma_b=gb, Itmax=1, h0=h0)
    want = U.h_half(X, w0, h0, prior, ga, gb)
    eng = C.VBEngine(C.CountMatrix(X), w0.shape[1])
    eng.ml_set_state(w0, h0)
    eng.ml_step(prior=prior, gamma_a=ga, gamma_b=gb)
    stepped = eng.ml_get_state(("eh",))["eh"]
    eng.close()
    lk = U.cell_likelihood(X, w0, want)
    errs = relerr(p.coeff[0], want), relerr(p.coeff[0], stepped), relerr(p.cell_likelihood, lk)
    print(name, "H vs restatement %.3g, H vs ml_step %.3g, cell likelihood %.3g" % errs)
    assert p.ranks == [w0.shape[1]] and p.coeff[0].shape == h0.shape
    assert errs[0] <= 1e-12 and errs[1] <= 1e-12
    assert errs[2] <= 1e-10
    assert np.all(p.nsteps == 1) and np.all(p.reason == 4)
    assert abs(p.likelihood - lk.sum() / X.shape[0] / X.shape[1]) <= 1e-10 * abs(p.likelihood)
    assert np.array_equal(C.cluster_id(p, rank=w0.shape[1]), np.argmax(p.coeff[0], axis=0) + 1)


# ---- column lengths around the workgroup's pass ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lengths_case(r):
    """n = 700.  Columns of 1, 2, 63, 64, 65 and 700 (= n) stored entries, and of the counts just below, at and just above ONE
    pass of the kernel's workgroup and just above TWO -- from the kernel's own constant -- in one matrix.  30 % of the gene rows
    are empty in every column short enough to leave them empty.  -> (X, W, h0, lengths, restatement runs).

    (The kernel that was measured and kept reads a cell's rows from global memory in every pass and holds no LDS image of them,
    DESIGN.md section 5f: the pass, 256 / 128 / 64 entries by rank, is the size at which its code takes another path.)"""
    import importlib
    P = importlib.import_module("ccfindr_amd.project")      # (the package attribute of that name is the function)
    import ccfindr_amd as C
    per = P.pass_entries(r)
    n = 700
    lengths = [1, 2, 63, 64, 65, n, per - 1, per, per + 1, 2 * per + 1, 3, 200]
    # ... and, as further lengths only (the product has no such boundary), where the dropped staged form changed paths: around
    # one and two 160 KB images of R * 8 + 8 bytes per entry
    img = 160 * 1024 // (int(C.load().vbnmf_padded_rank(r)) * 8 + 8)
    lengths += [L for L in (img - 1, img, img + 1, 2 * img + 1) if L <= n]
    rng = np.random.default_rng(1000 + r)
    rows = rng.permutation(n)
    used, spare = rows[: (7 * n) // 10], rows[(7 * n) // 10:]
    X = np.zeros((n, len(lengths)))
    for j, L in enumerate(lengths):
        take = rng.permutation(used)[:L]
        if L > used.size:
            take = np.concatenate((used, rng.permutation(spare)[:L - used.size]))
        X[take, j] = rng.integers(1, 6, size=L)
    assert [int(v) for v in (X > 0).sum(axis=0)] == lengths
    W = rng.uniform(0.05, 1.0, size=(n, r))
    h0 = rng.uniform(0.05, 1.0, size=(r, len(lengths)))
    return X, W, h0, lengths, {it: U.project(X, W, h0, Itmax=it, Tol=0.0) for it in (1, 20)}


@pytest.mark.parametrize("r", [128, 33, 65, 10])
def test_column_lengths_around_the_pass(r):
    """One call over columns shorter than, equal to and longer than one and two passes of the workgroup (and of one entry, and
    of all n): one iteration 1e-12 / 1e-10, twenty iterations with Tol = 0 1e-9.  Ranks 33 and 65: two and four lanes share an
    entry."""
    import ccfindr_amd as C
    X, W, h0, lengths, want = lengths_case(r)
    for it, tol_h, tol_l in ((1, 1e-12, 1e-10), (20, 1e-9, 1e-9)):
        p = C.project(X, W, Itmax=it, Tol=0.0, h0=h0)
        eh, el = relerr(p.coeff[0], want[it]["h"]), relerr(p.cell_likelihood, want[it]["lk"])
        print(f"rank {r}, {it} iterations, lengths {lengths}: H {eh:.3g}, cell likelihood {el:.3g}")
        assert eh <= tol_h and el <= tol_l
        assert np.all(p.nsteps == it) and np.all(p.reason == 4)


# ---- stopping rule ----------------------------------------------------------------------------------------------------------
STOP_SEED = 68


@functools.lru_cache(maxsize=None)
def stop_case():
    X = counts(90, 140, 0.6, seed=STOP_SEED)
    W = np.random.default_rng(STOP_SEED + 1).uniform(0.05, 1.0, size=(90, 5))
    h0 = U.default_start(X, W)
    return X, W, h0, U.project(X, W, h0, Itmax=10000, Tol=1e-5), U.project(X, W, h0, Itmax=7, Tol=1e-5)


def test_stopping_rule_per_cell():
    """90 x 140, rank 5, Tol = 1e-5, the default start: nsteps and reason equal the restatement's in every cell whose decisions
    there were clear (| |dlk| / |lkold| - Tol | > 1e-3 Tol at every step), and at least 95 % of the cells are.  Seed 68 (of the
    seeds 60..79, whose shares on the CPU lie between 0.929 and 0.986): 138 of the restatement's 140 cells are clear, share
    0.9857; its cells stop after 28 to 101 iterations."""
    import ccfindr_amd as C
    X, W, h0, want, _ = stop_case()
    clear = want["margin"] > 1e-3 * 1e-5
    print("clear share %.4f, closest margin / Tol %.3g, iterations %d..%d" % (clear.mean(), want["margin"].min() / 1e-5,
                                                                             want["it"].min(), want["it"].max()))
    assert clear.mean() >= 0.95
    p = C.project(X, W, Tol=1e-5)
    assert np.array_equal(p.nsteps[clear], want["it"][clear]) and np.array_equal(p.reason[clear], want["reason"][clear])
    assert np.all(p.reason[clear] == 1) and len(set(p.nsteps.tolist())) > 5
    assert relerr(p.coeff[0][:, clear], want["h"][:, clear]) <= 1e-9
    assert relerr(p.cell_likelihood[clear], want["lk"][clear]) <= 1e-9


def test_itmax_ends_the_unconverged_cells():
    import ccfindr_amd as C
    X, W, h0, full, want = stop_case()
    p = C.project(X, W, Tol=1e-5, Itmax=7)
    late = full["it"] > 7
    assert late.any()
    assert np.all(p.nsteps[late] == 7) and np.all(p.reason[late] == 4)
    clear = full["margin"] > 1e-3 * 1e-5
    early = ~late & clear
    assert np.array_equal(p.nsteps[early], want["it"][early]) and np.all(p.reason[early] == 1)
    assert relerr(p.coeff[0], want["h"]) <= 1e-9


# ---- likelihood -------------------------------------------------------------------------------------------------------------
def test_likelihood_is_the_literal_one_and_never_decreases():
    """p.likelihood against oracle.likelihood_literal(X, W, H), 1e-10; every cell's likelihood over Itmax = 1..12 never
    decreases (slack 1e-13 |lk|, as the ML tests)."""
    import ccfindr_amd as C
    from oracle import mlnmf_oracle as O
    X = counts(120, 90, 0.5, seed=77)
    W = np.random.default_rng(78).uniform(0.05, 1.0, size=(120, 6))
    M = C.CountMatrix(X)
    prev = None
    for it in range(1, 13):
        p = C.project(M, W, Itmax=it, Tol=0.0)
        lit = O.likelihood_literal(X, W, p.coeff[0])
        assert abs(p.likelihood / lit - 1) <= 1e-10, (it, p.likelihood, lit)
        if prev is not None:
            assert np.all(p.cell_likelihood >= prev - 1e-13 * np.abs(prev)), it
        prev = p.cell_likelihood
    M.close()


# ---- independence, bit for bit ----------------------------------------------------------------------------------------------
def test_halves_and_permutation_bitwise():
    """The whole matrix in one call equals two calls on its halves through col_begin / col_end, and a column permutation of X
    permutes H, cell_likelihood and nsteps exactly: a cell's sums do not depend on the grid or on its neighbours."""
    import ccfindr_amd as C
    import importlib
    P = importlib.import_module("ccfindr_amd.project")
    X, W, h0, lengths, _ = lengths_case(33)
    rng = np.random.default_rng(9)
    X = np.concatenate((X, counts(X.shape[0], 300, 0.05, seed=10)), axis=1)
    m = X.shape[1]
    h0 = rng.uniform(0.05, 1.0, size=(33, m))
    kw = dict(Itmax=40, Tol=1e-3)
    p = C.project(X, W, h0=h0, **kw)
    assert len(set(p.nsteps.tolist())) > 3
    M = C.CountMatrix(X)
    cut = 7
    a = P.project_columns(M, W, h0[:, :cut], 0, cut, **kw)
    b = P.project_columns(M, W, h0[:, cut:], cut, m, **kw)
    M.close()
    for q, whole in enumerate((p.coeff[0], p.cell_likelihood, p.nsteps, p.reason)):
        assert np.array_equal(np.concatenate((a[q], b[q]), axis=-1), whole), q
    perm = rng.permutation(m)
    pp = C.project(X[:, perm], W, h0=h0[:, perm], **kw)
    assert np.array_equal(pp.coeff[0], p.coeff[0][:, perm]) and np.array_equal(pp.cell_likelihood, p.cell_likelihood[perm])
    assert np.array_equal(pp.nsteps, p.nsteps[perm]) and np.array_equal(pp.reason, p.reason[perm])


# ---- more cells than workgroups: the persistent grid goes round ----------------------------------------------------------
def grid_workgroups():
    """Workgroups of the kernel's persistent grid: as many as the CUs hold threads for (project.hip, project_grid: CUs x 2048 / 256)."""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 8


@functools.lru_cache(maxsize=None)
def many_cells_case(r):
    """80 genes x 6000 short columns (1 to 40 stored entries, about 3 cells per workgroup of the grid); a third of the cells
    start far from their fixed point, so that iteration counts differ widely between the cells one workgroup takes in turn.
    -> (X, W, h0, the restatement's run to Tol = 1e-4 within 60 steps and its 3-step run)."""
    n, m = 80, 6000
    rng = np.random.default_rng(500 + r)
    X = np.zeros((n, m))
    for j, L in enumerate(rng.integers(1, 41, size=m)):
        X[rng.permutation(n)[:L], j] = rng.integers(1, 6, size=L)
    W = rng.uniform(0.05, 1.0, size=(n, r))
    h0 = U.default_start(X, W) * rng.uniform(0.5, 2.0, size=(r, m))
    h0[:, ::3] = rng.uniform(1e-6, 10.0, size=h0[:, ::3].shape)
    return X, W, h0, U.project(X, W, h0, Itmax=60, Tol=1e-4), U.project(X, W, h0, Itmax=3, Tol=0.0)


@pytest.mark.parametrize("r", [5, 65])
def test_workgroups_take_many_cells_in_turn(r):
    """More cells than twice the grid's workgroups, so that every workgroup draws several tickets and takes cells with
    different iteration counts one after the other: three iterations against the restatement (1e-9: a short trajectory), the
    stopping run's counts and reasons in the clear cells, and -- bit for bit -- the whole call against its halves and against a
    column permutation, which hands every cell to another workgroup behind another predecessor."""
    import ccfindr_amd as C
    import importlib
    P = importlib.import_module("ccfindr_amd.project")
    X, W, h0, want, want3 = many_cells_case(r)
    m = X.shape[1]
    assert m > 2 * grid_workgroups(), (m, grid_workgroups())
    p3 = C.project(X, W, Itmax=3, Tol=0.0, h0=h0)
    e3 = relerr(p3.coeff[0], want3["h"]), relerr(p3.cell_likelihood, want3["lk"])
    print(f"rank {r}, {m} cells on {grid_workgroups()} workgroups, 3 iterations: H {e3[0]:.3g}, cell likelihood {e3[1]:.3g}")
    assert e3[0] <= 1e-9 and e3[1] <= 1e-9
    kw = dict(Itmax=60, Tol=1e-4)
    p = C.project(X, W, h0=h0, **kw)
    clear = want["margin"] > 1e-3 * 1e-4
    print("iterations %d..%d, %d distinct; clear share %.4f" % (p.nsteps.min(), p.nsteps.max(), len(set(p.nsteps.tolist())), clear.mean()))
    assert len(set(p.nsteps.tolist())) > 10 and clear.mean() >= 0.95
    assert np.array_equal(p.nsteps[clear], want["it"][clear]) and np.array_equal(p.reason[clear], want["reason"][clear])
    assert relerr(p.coeff[0][:, clear], want["h"][:, clear]) <= 1e-9
    M = C.CountMatrix(X)
    cut = m // 2 + 17
    a = P.project_columns(M, W, h0[:, :cut], 0, cut, **kw)
    b = P.project_columns(M, W, h0[:, cut:], cut, m, **kw)
    M.close()
    for q, whole in enumerate((p.coeff[0], p.cell_likelihood, p.nsteps, p.reason)):
        assert np.array_equal(np.concatenate((a[q], b[q]), axis=-1), whole), q
    perm = np.random.default_rng(r).permutation(m)
    pp = C.project(X[:, perm], W, h0=h0[:, perm], **kw)
    assert np.array_equal(pp.coeff[0], p.coeff[0][:, perm]) and np.array_equal(pp.cell_likelihood, p.cell_likelihood[perm])
    assert np.array_equal(pp.nsteps, p.nsteps[perm]) and np.array_equal(pp.reason, p.reason[perm])


# ---- non-finite input -------------------------------------------------------------------------------------------------------
def test_non_finite_input_ends_every_cell():
    """One NaN in W, Itmax = 5: status 0 and every cell ends within 5 steps with reason 3 or 4.  colSums(w)_k of the NaN's
    column k is NaN, and it divides h_k of EVERY cell (R/factorize.R:9, :14) -- so no cell is left untouched by it, whether it
    expresses that gene or not: what stays unchanged, bit for bit, in the cells that do not touch the gene is every OTHER row of
    their first-step H (its sums never met the NaN).  A NaN that belongs to one cell -- in its start -- ends that cell with
    reason 3 and leaves all the others unchanged bit for bit."""
    import ccfindr_amd as C
    X = counts(60, 80, 0.3, seed=91)
    rng = np.random.default_rng(92)
    W = rng.uniform(0.05, 1.0, size=(60, 4))
    h0 = rng.uniform(0.05, 1.0, size=(4, 80))
    clean1 = C.project(X, W, Itmax=1, Tol=1e-5, h0=h0)
    clean5 = C.project(X, W, Itmax=5, Tol=1e-5, h0=h0)
    bad = W.copy()
    bad[17, 2] = np.nan
    p = C.project(X, bad, Itmax=5, Tol=1e-5, h0=h0)                     # (returns: status 0)
    touch = X[17] > 0
    assert touch.any() and not touch.all()
    assert np.all(np.isin(p.reason, (3, 4))) and np.all(p.nsteps <= 5) and np.all(p.nsteps >= 1)
    assert np.all(np.isin(p.reason[touch], (3, 4))) and np.all(p.nsteps[touch] <= 5)
    others = [0, 1, 3]
    assert np.all(p.nsteps[~touch] == 1)
    assert np.array_equal(p.coeff[0][np.ix_(others, ~touch)], clean1.coeff[0][np.ix_(others, ~touch)])
    assert np.all(np.isnan(p.coeff[0][2]))
    start = h0.copy()
    start[1, 11] = np.nan
    q = C.project(X, W, Itmax=5, Tol=1e-5, h0=start)
    keep = np.arange(80) != 11
    assert q.reason[11] == 3 and q.nsteps[11] <= 5
    assert np.array_equal(q.coeff[0][:, keep], clean5.coeff[0][:, keep])
    assert np.array_equal(q.cell_likelihood[keep], clean5.cell_likelihood[keep])
    assert np.array_equal(q.nsteps[keep], clean5.nsteps[keep]) and np.array_equal(q.reason[keep], clean5.reason[keep])


# ---- end to end -------------------------------------------------------------------------------------------------------------
def test_fit_on_a_subsample_then_place_the_rest():
    """450 cells of three clusters, 200 genes, from ONE simulate_data call (seed 5, clusters in order: cell j belongs to cluster
    j // 150), dealt out by one permutation: factorize() at rank 3 on the first 300 (200 x 300), then project() of the other
    150.  The projected cells' cluster_id equals the restatement's, run on the same basis, cell for cell; against the planted
    clusters (through the label map the fit's own cells define) the restatement agrees in the share the test prints: 1.0000
    (150 of 150; the fit's own 300 cells: 1.0000)."""
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
    res = C.factorize(fit, ranks=3, nrun=4, verbose=0, seed=3)
    fit_ids = C.cluster_id(res, rank=3)
    relabel = np.array([np.bincount(planted[:300][fit_ids == k], minlength=3).argmax() if np.any(fit_ids == k) else -1
                        for k in (1, 2, 3)])
    p = C.project(new, res, rank=3)
    ids = C.cluster_id(p, rank=3)
    W = res.basis[0]
    want = U.project(new, W, U.default_start(new, W))
    want_ids = np.argmax(want["h"], axis=0) + 1
    share = float(np.mean(relabel[want_ids - 1] == planted[300:]))
    print("restatement against the planted clusters: %.4f; fitted cells: %.4f" % (share, float(np.mean(relabel[fit_ids - 1] == planted[:300]))))
    assert np.array_equal(ids, want_ids)
    assert float(np.mean(relabel[ids - 1] == planted[300:])) == share
    assert np.all(p.reason == 1)
