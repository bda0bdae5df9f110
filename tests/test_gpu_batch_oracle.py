"""Engines built the ways only the batched drivers use -- padded row widths (pad_rank), narrow grids (batch_grid) and the batch
kernels (vbnmf_batch_run, vbnmf_batch_ml_run) -- against the CPU oracles and the 50-digit step, not against themselves.

tests/test_gpu_batch_run.py holds a batch to the stand-alone engine of the same grid and width, bit for bit; that cannot see a
mistake both forms share (a pad column in the statistics or the prior terms of the evidence, a wrong k < r bound, an update table
that is wrong when one block holds thousands of majors).  Here every number is held to an independent statement of the step:
  * oracle.vbnmf_oracle (reference src/vbnmf_update.cpp:19-101), stepped on the host, for states, statistics and evidence;
  * bayesian.hyper_update on the ORACLE's statistics for the hyper-parameter trajectory (the device's Newton step differs only
    by its digamma / trigamma: 1e-9, as in tests/test_gpu_device_loop.py);
  * tests/util_mp_step.py (50 digits) for one step, at the bounds of tests/test_gpu_mpmath.py;
  * oracle.mlnmf_oracle (reference R/factorize.R:2-27, :40-49) for the ML batch.
"""
import heapq
import os

import numpy as np
import pytest

from test_gpu_device_loop import host_loop
from util_layout import build_layout
from util_mp_step import CASES, make_case, ml_step, step

pytestmark = pytest.mark.gpu

HY = {"aw": 1.1, "bw": 0.9, "ah": 0.8, "bh": 1.3}
FACT = ("lw", "lh", "ew", "eh", "dw", "dh")
UPD_TAB_WORDS = 16384                  # kernels.h kUpdTabWords: the LDS copy of one block's row of k_update2's table (64 KB)
UPDATE_THREADS = 1024                  # kernels.h kUpdateThreads


def relerr(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def _counts(n, m, seed, kind="counts"):
    rng = np.random.default_rng(seed)
    X = rng.poisson(0.7, size=(n, m)).astype(np.float64)
    X[np.arange(n), rng.integers(0, m, n)] += 1.0               # no empty gene
    X[rng.integers(0, n, m), np.arange(m)] += 1.0               # no empty cell
    if kind == "noninteger":                                    # the wide layout (value + index streams)
        X = X * rng.uniform(0.5, 1.5, size=(1, m))
    elif kind == "split":                                       # integer counts, one beyond the packed range: split entries
        X[n // 3, m // 2] = 20000.0 + 17.0
    return np.asfortranarray(X)


def _sparse_counts(n, m, per_cell, seed):
    """n x m integer counts, about per_cell stored entries per cell, no empty gene or cell (scipy CSC)."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    rows = [rng.choice(n, size=per_cell, replace=False) for _ in range(m)]
    i = np.concatenate(rows + [np.arange(n)])
    j = np.concatenate([np.full(per_cell, c) for c in range(m)] + [rng.integers(0, m, n)])
    x = rng.poisson(1.0, size=i.size).astype(np.float64) + 1.0
    X = sp.coo_matrix((x, (i, j)), shape=(n, m)).tocsc()
    X.sum_duplicates()
    return X


def _stats(ref):
    with np.errstate(divide="ignore"):                          # (a factor row of zeros: the NaN-evidence case)
        return (np.mean(np.log(ref["lw"])), np.mean(np.log(ref["lh"])), np.mean(ref["ew"]), np.mean(ref["eh"]))


def _oracle(X):
    """The dense literal oracle, or -- for the large table cases -- its stored-entries form (held to it by
    tests/test_oracle_golden.py), on every core."""
    from oracle import vbnmf_oracle as O
    if not hasattr(X, "tocsc"):
        return lambda wh, hy, fud: O.update_dense(X, wh, hy, fud)
    X = X.tocsc()
    n, m = X.shape
    nt = max(1, min(16, O.lib().oracle_max_threads()))
    return lambda wh, hy, fud: O.update_csc(n, m, X.indptr, X.indices, X.data, wh, hy, fud, nthreads=nt)


def _three_steps_against_the_oracle(M, X, r, wh, hy=HY, fudge=None, steps=3, **engine_kw):
    """``steps`` resident steps of VBEngine(M, r, **engine_kw) from ``wh``: lkh and the four statistics of every step within
    1e-10 of the oracle's (means over the r columns of the rank, not the stored width), the final state within 1e-11.
    Returns the oracle's last state."""
    import ccfindr_amd as C
    fudge = C.EPS if fudge is None else fudge
    upd = _oracle(X)
    eng = C.VBEngine(M, r, **engine_kw)
    try:
        eng.set_state(wh["lw"], wh["lh"], wh["eh"])
        ref = wh
        for t in range(steps):
            lkh, st = eng.step(hy, fudge)
            ref = upd(ref, hy, fudge)
            assert abs(lkh / ref["lkh"] - 1) <= 1e-10, (r, engine_kw, t, lkh, ref["lkh"])
            want = _stats(ref)
            for q in range(4):
                assert abs(st[q] / want[q] - 1) <= 1e-10, (r, engine_kw, t, q, st[q], want[q])
        got = eng.get_state()
    finally:
        eng.close()
    for k in FACT:
        assert got[k].shape == ref[k].shape
        assert relerr(got[k], ref[k]) <= 1e-11, (r, engine_kw, k, relerr(got[k], ref[k]))
    return ref


# ---- the update table's row: which side of the 64 KB limit an engine is on --------------------------------------------------
def update_table_stride(M, R, n_wg, ub):
    """Words per block of k_update2's table for an engine of padded rank R, n_wg sweep workgroups and ub update blocks on M:
    engine.hip build_update_table, restated from the layouts' inverse index (inv_ptr) -- items of cost (tasks + 4) dealt to
    1024 / R thread rows longest first, each to the least loaded row (ties to the lowest); stride = 3 words per visit of the
    fullest row times the rows, plus the block's task ids, each rounded up to 4.  The layouts are cut at the engine's grid
    (VBNMF_NWG for the host view, as the engine creation passes its n_wg)."""
    old = os.environ.get("VBNMF_NWG")
    os.environ["VBNMF_NWG"] = str(int(n_wg))
    try:
        views = [build_layout(M, side, R) for side in (0, 1)]
    finally:
        if old is None:
            del os.environ["VBNMF_NWG"]
        else:
            os.environ["VBNMF_NWG"] = old
    assert all(v["n_wg"] == n_wg for v in views)
    assert views[0]["n_major"] == M.shape[0] and views[1]["n_major"] == M.shape[1]
    RB = UPDATE_THREADS // R
    cnts = [np.diff(v["inv_ptr"]).astype(np.int64) for v in views]
    per = [(c.size + ub - 1) // ub for c in cnts]
    V, max_ids = 1, 0
    for b in range(ub):
        items, ids = [], 0
        for sd in (0, 1):
            m0 = min(cnts[sd].size, b * per[sd]); m1 = min(cnts[sd].size, m0 + per[sd])
            c = cnts[sd][m0:m1]
            items += [(-(int(k) + 4), (sd << 31) | q) for q, k in enumerate(c)]     # cost descending, then code ascending
            ids += int(c.sum())
        max_ids = max(max_ids, ids)
        items.sort()
        heap = [(0, q) for q in range(RB)]
        size = [0] * RB
        for negcost, _ in items:
            load, q = heapq.heappop(heap)
            size[q] += 1
            heapq.heappush(heap, (load - negcost, q))
        V = max(V, max(size))
    vis_words = (RB * V * 3 + 3) & ~3
    return (vis_words + max_ids + 3) & ~3


# ---- 1. padded engines, step by step ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [2, 4, 6, 8, 10, 12, 14, 16])
def test_padded_engine_of_every_rank_up_to_its_width_against_the_oracle(W):
    """VBEngine(M, r, pad_rank=W) for every 1 <= r <= W: integer counts (packed layout) for every rank; non-integer values (wide
    layout) and a count above the packed range (split entries) for the lowest, a middle and the full rank."""
    import ccfindr_amd as C
    from ccfindr_amd import synth
    for kind in ("counts", "noninteger", "split"):
        X = _counts(150, 230, seed=W, kind=kind)
        M = C.CountMatrix(X)
        ranks = range(1, W + 1) if kind == "counts" else sorted({1, (W + 1) // 2, W})
        for r in ranks:
            wh = synth.random_state(150, 230, r, HY, seed=100 * W + r)
            _three_steps_against_the_oracle(M, X, r, wh, pad_rank=W)
        M.close()


@pytest.mark.parametrize("r,W", [(3, 32), (17, 32), (33, 40), (33, 64), (41, 64), (65, 128), (100, 128)])
def test_padded_engine_beyond_the_batch_widths_against_the_oracle(r, W):
    import ccfindr_amd as C
    from ccfindr_amd import synth
    X = _counts(150, 230, seed=r + W)
    M = C.CountMatrix(X)
    wh = synth.random_state(150, 230, r, HY, seed=r * W)
    _three_steps_against_the_oracle(M, X, r, wh, pad_rank=W)
    M.close()


@pytest.mark.parametrize("r,W", [(3, 16), (5, 8), (9, 32)])
def test_padded_engine_with_an_active_fudge_clip(r, W):
    """fudge = 1e-3 with small Gamma shapes: exp(psi(alpha)) / beta falls below the fudge for many entries (reference
    src/vbnmf_update.cpp:60, :64), so the clipped values and their evidence terms enter all three steps."""
    import ccfindr_amd as C
    from ccfindr_amd import synth
    hy = {"aw": 0.3, "bw": 0.5, "ah": 0.2, "bh": 0.4}
    X = _counts(150, 230, seed=7 + r)
    M = C.CountMatrix(X)
    wh = synth.random_state(150, 230, r, hy, seed=r)
    ref = _three_steps_against_the_oracle(M, X, r, wh, hy=hy, fudge=1e-3, pad_rank=W)
    assert (ref["lw"] == 1e-3).sum() + (ref["lh"] == 1e-3).sum() > 0          # the clip was hit
    M.close()


# ---- 2. narrow grids -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(8, 8), (16, 16), (32, 32), (64, 64), (8, 64), (64, 8)])
def test_narrow_grid_engines_against_the_oracle(grid):
    import ccfindr_amd as C
    from ccfindr_amd import synth
    X = _counts(300, 460, seed=grid[0] + 3 * grid[1])
    M = C.CountMatrix(X)
    for r in (3, 10, 16):
        wh = synth.random_state(*X.shape, r, HY, seed=r + grid[1])
        _three_steps_against_the_oracle(M, X, r, wh, grid=grid)
    M.close()


# (n genes, m cells, about per_cell entries per cell): the rank-3 table at grid (8, 8) just inside and just beyond one block's row
TABLE_NEAR = (400, 29300, 2)
TABLE_OVER = (400, 29500, 2)


@pytest.mark.parametrize("shape,fits", [(TABLE_NEAR, True), (TABLE_OVER, False)], ids=["near_fill", "just_over"])
def test_update_table_at_the_limit_of_one_block_row(shape, fits):
    """A wide, very sparse matrix at grid (8, 8): ~3 700 majors per update block.  Inside the limit the engine takes the
    one-launch update (k_update2), beyond it the two-launch form; both against the oracle.  Which side a case is on is asserted
    from the layouts, and observed from the engine: only the one-launch form is accepted by vbnmf_batch_run."""
    import ccfindr_amd as C
    from ccfindr_amd import synth
    n, m, pc = shape
    X = _sparse_counts(n, m, pc, seed=m)
    M = C.CountMatrix(X)
    r, grid = 3, (8, 8)
    stride = update_table_stride(M, C.engine.padded_rank(r), grid[0], grid[1])
    if fits:
        assert UPD_TAB_WORDS - 512 <= stride <= UPD_TAB_WORDS, stride
    else:
        assert UPD_TAB_WORDS < stride <= UPD_TAB_WORDS + 1024, stride
    wh = synth.random_state(n, m, r, HY, seed=5)
    _three_steps_against_the_oracle(M, X, r, wh, grid=grid)
    eng = C.VBEngine(M, r, grid=grid)
    eng.set_state(wh["lw"], wh["lh"], wh["eh"])
    if fits:
        assert C.run_batch([eng], [HY], Itmax=2, Tol=0.0)[0]["it"] == 2
    else:
        with pytest.raises(C.VBNMFError) as exc:
            C.run_batch([eng], [HY], Itmax=2, Tol=0.0)
        assert exc.value.code == 5                                          # VBNMF_ERR_STATE: the engine's form, no step taken
    eng.close()
    M.close()


# ---- 3. batched trajectories against the oracle driven by the host loop -----------------------------------------------------
class _OracleEngine:
    """The oracle behind VBEngine.step's interface, so that host_loop (tests/test_gpu_device_loop.py) drives it: its own
    statistics feed bayesian.hyper_update."""

    def __init__(self, X, wh, fudge):
        self.upd, self.ref, self.fudge = _oracle(X), wh, fudge

    def step(self, hyper):
        self.ref = self.upd(self.ref, hyper, self.fudge)
        return self.ref["lkh"], _stats(self.ref)


def _close_with_nan(a, b, rtol):
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb)
    return float(np.max(np.abs(a[~na] - b[~na]) / np.maximum(np.abs(b[~na]), 1e-300), initial=0.0)) <= rtol


@pytest.mark.parametrize("flags", [(True,) * 4, (False,) * 4], ids=["hyper_on", "hyper_off"])
@pytest.mark.parametrize("B,ranks", [(1, [5]), (3, [4]), (16, [7]), (64, [3]), (16, list(range(1, 17)))],
                         ids=["B1", "B3", "B16", "B64", "B16_ranks1to16"])
def test_batched_trajectories_against_the_oracle(B, ranks, flags):
    import ccfindr_amd as C
    from ccfindr_amd import synth
    X = _counts(150, 230, seed=B + len(ranks))
    n, m = X.shape
    M = C.CountMatrix(X)
    rk = [ranks[b % len(ranks)] for b in range(B)]
    pad = C.engine.padded_rank(max(rk))
    grid = C.batch_grid(B)
    hys = [dict(HY, aw=HY["aw"] * (1 + 0.03 * b), bw=HY["bw"] * (1 + 0.01 * (b % 5)), bh=HY["bh"] * (1 - 0.005 * b)) for b in range(B)]
    whs = [synth.random_state(n, m, rk[b], hys[b], seed=50 + b) for b in range(B)]
    kw = dict(Itmax=20, Tol=0.0, n0=3, dn=1, flags=flags)
    engs = [C.VBEngine(M, rk[b], grid=grid, pad_rank=pad) for b in range(B)]
    for eng, wh in zip(engs, whs):
        eng.set_state(wh["lw"], wh["lh"], wh["eh"])
    got = C.run_batch(engs, hys, history=True, **kw)
    for b in range(B):
        ora = _OracleEngine(X, whs[b], C.EPS)
        it, lk0, hyper, trace = host_loop(ora, dict(hys[b]), kw["Itmax"], kw["Tol"], kw["n0"], kw["dn"], flags)
        assert got[b]["it"] == it == 20 and got[b]["reason"] == 4
        assert got[b]["history"].shape == trace.shape
        assert relerr(got[b]["history"], trace) <= 1e-9, (b, rk[b], relerr(got[b]["history"], trace))
        for k in ("aw", "bw", "ah", "bh"):
            assert abs(got[b]["hyper"][k] / hyper[k] - 1) <= 1e-9
        st = engs[b].get_state()
        for k in FACT:
            assert relerr(st[k], ora.ref[k]) <= 1e-9, (b, rk[b], k, relerr(st[k], ora.ref[k]))
    for eng in engs:
        eng.close()
    M.close()


def test_batched_nan_engine_agrees_with_the_oracle():
    """One engine of a mixed-rank batch starts from a state whose evidence is NaN (a whole factor row 0, fudge = 0): the oracle
    gives NaN at step 1 as well, and the engine stops there with reason 1; the others run their 20 steps as the oracle does."""
    import ccfindr_amd as C
    from ccfindr_amd import synth
    X = _counts(150, 230, seed=11)
    n, m = X.shape
    M = C.CountMatrix(X)
    rk = [2, 5, 8, 3]
    grid, pad = C.batch_grid(len(rk)), 8
    whs = [synth.random_state(n, m, r, HY, seed=r) for r in rk]
    whs[2]["lw"][0, :] = 0.0
    kw = dict(Itmax=20, Tol=0.0, n0=3, dn=1, flags=(True,) * 4)
    engs = [C.VBEngine(M, r, grid=grid, pad_rank=pad) for r in rk]
    for eng, wh in zip(engs, whs):
        eng.set_state(wh["lw"], wh["lh"], wh["eh"])
    got = C.run_batch(engs, [HY] * len(rk), fudge=0.0, history=True, **kw)
    for b in range(len(rk)):
        it, lk0, hyper, trace = host_loop(_OracleEngine(X, whs[b], 0.0), dict(HY), kw["Itmax"], kw["Tol"], kw["n0"], kw["dn"], kw["flags"])
        assert got[b]["it"] == it
        if b == 2:
            assert it == 1 and np.isnan(trace[0, 0])
            assert got[b]["reason"] == 1 and np.isnan(got[b]["lkh"]) and np.isnan(got[b]["history"][0, 0])
        else:
            assert it == 20 and got[b]["reason"] == 4
            assert _close_with_nan(got[b]["history"], trace, 1e-9), b
    for eng in engs:
        eng.close()
    M.close()


# ---- 4. the 50-digit step ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[f"n{c[0]}m{c[1]}r{c[2]}" for c in CASES])
@pytest.mark.parametrize("noninteger", [False, True])
def test_width_16_narrow_grid_engine_against_50_digit_step(case, noninteger):
    """One step of an engine 16 columns wide on grid (8, 8), through VBEngine.step and through a mixed-rank batch of 3
    (vbnmf_batch_run, the case's engine in the middle): state within 1e-13, lkh within 1e-12 (tests/test_gpu_mpmath.py)."""
    import ccfindr_amd as C
    n, m, r, lam, hyper, fudge, seed = case
    X, wh = make_case(n, m, r, lam, hyper, fudge, seed, noninteger)
    want = step(X, wh, hyper, fudge)
    M = C.CountMatrix(X)
    grid, pad = (8, 8), 16
    eng = C.VBEngine(M, r, grid=grid, pad_rank=pad)
    eng.set_state(wh["lw"], wh["lh"], wh["eh"])
    lkh, _ = eng.step(hyper, fudge)
    got = eng.get_state()
    eng.close()
    assert abs(lkh / float(want["lkh"]) - 1) <= 1e-12, (lkh, float(want["lkh"]))
    for k in FACT:
        assert relerr(got[k], want[k]) <= 1e-13, (k, relerr(got[k], want[k]))
    # in a batch of three engines of ranks r - 1, r, r + 1 (within the matrix's) at the same width
    rng = np.random.default_rng(seed)
    rks = (max(1, r - 1), r, min(r + 1, n, m))
    engs = [C.VBEngine(M, rr, grid=grid, pad_rank=pad) for rr in rks]
    for b, (eng, rr) in enumerate(zip(engs, rks)):
        if b == 1:
            eng.set_state(wh["lw"], wh["lh"], wh["eh"])
        else:
            eng.set_state(rng.uniform(0.1, 1.0, (n, rr)), rng.uniform(0.1, 1.0, (rr, m)), rng.uniform(0.1, 1.0, (rr, m)))
    out = C.run_batch(engs, [hyper] * 3, Itmax=1, Tol=0.0, flags=(False,) * 4, fudge=fudge, history=True)
    assert out[1]["it"] == 1 and out[1]["reason"] == 4
    assert abs(out[1]["history"][0, 0] / float(want["lkh"]) - 1) <= 1e-12
    got = engs[1].get_state()
    for e in engs:
        e.close()
    for k in FACT:
        assert relerr(got[k], want[k]) <= 1e-13, ("batch", k, relerr(got[k], want[k]))
    M.close()


@pytest.mark.parametrize("prior", [False, True])
@pytest.mark.parametrize("n,m,r,seed", [(7, 9, 3, 1), (12, 6, 2, 2), (5, 14, 4, 3)])
def test_ml_batch_step_against_50_digit_step(n, m, r, seed, prior):
    """One ML step through run_batch_ml (a mixed-rank batch of 3 at width 16 on grid (8, 8)) against the 50-digit nmf_updateR +
    likelihood, at the bounds of tests/test_gpu_mpmath.py::test_ml_engine_against_50_digit_step."""
    import ccfindr_amd as C
    rng = np.random.default_rng(seed)
    X, _ = make_case(n, m, r, 1.1, {"aw": 1.0, "bw": 1.0, "ah": 1.0, "bh": 1.0}, 0.0, seed, noninteger=bool(seed % 2))
    w, h = rng.uniform(0.05, 1.0, size=(n, r)), rng.uniform(0.05, 1.0, size=(r, m))
    ew, eh, lk = ml_step(X, w, h, prior, 1.7, 0.6)
    M = C.CountMatrix(X)
    rks = (max(1, r - 1), r, min(r + 1, n, m))
    engs = [C.VBEngine(M, rr, grid=(8, 8), pad_rank=16) for rr in rks]
    for b, (eng, rr) in enumerate(zip(engs, rks)):
        if b == 1:
            eng.ml_set_state(w, h)
        else:
            eng.ml_set_state(rng.uniform(0.05, 1.0, size=(n, rr)), rng.uniform(0.05, 1.0, size=(rr, m)))
    out = C.run_batch_ml(engs, Itmax=1, Tol=0.0, prior=prior, gamma_a=1.7, gamma_b=0.6, history=True)
    st = engs[1].ml_get_state()
    for e in engs:
        e.close()
    M.close()
    assert out[1]["it"] == 1
    assert relerr(st["ew"], ew) <= 1e-13 and relerr(st["eh"], eh) <= 1e-13
    wh = ew @ eh
    scale = (np.abs(X * np.log(wh)).sum() + wh.sum()) / n / m
    assert abs(out[1]["lk"] - float(lk)) <= 1e-12 * scale
    assert abs(out[1]["history"][0] - float(lk)) <= 1e-12 * scale


# ---- 5. the ML batch against the ML oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("prior,ga,gb", [(True, 0.5, 0.7), (True, 2.5, 0.7), (False, 1.0, 1.0)],
                         ids=["prior_ga0.5", "prior_ga2.5", "no_prior"])
@pytest.mark.parametrize("B,ranks,kind", [(2, [4], "counts"), (7, [6], "noninteger"), (16, [3], "counts"),
                                          (7, [1, 2, 3, 5, 8, 11, 12], "counts")],
                         ids=["B2", "B7_wide", "B16", "B7_ranks_width12"])
def test_ml_batch_against_the_ml_oracle(B, ranks, kind, prior, ga, gb):
    """run_batch_ml for 1, 8 and 19 steps (Tol = 0) at batch_grid(B): every engine's ew / eh within 1e-10 of nmf_update_literal
    iterated on the host, every step's likelihood within 1e-10 of the size of its sums (test_ml_step_random_case).  With
    gamma_a = 0.5 the prior's numerator up + gamma_a - 1 goes negative and the eps clamp (R/factorize.R:15, :24) is hit."""
    import ccfindr_amd as C
    from oracle import mlnmf_oracle as O
    X = _counts(150, 230, seed=B * 10 + len(ranks), kind=kind)
    n, m = X.shape
    M = C.CountMatrix(X)
    rk = [ranks[b % len(ranks)] for b in range(B)]
    pad = C.engine.padded_rank(max(rk))
    grid = C.batch_grid(B)
    rng = np.random.default_rng(B + len(ranks))
    starts = [(rng.uniform(0.05, 1.0, size=(n, r)), rng.uniform(0.05, 1.0, size=(r, m))) for r in rk]
    clamped = False
    for Itmax in (1, 8, 19):
        engs = [C.VBEngine(M, r, grid=grid, pad_rank=pad) for r in rk]
        for eng, (w0, h0) in zip(engs, starts):
            eng.ml_set_state(w0, h0)
        got = C.run_batch_ml(engs, Itmax=Itmax, Tol=0.0, prior=prior, gamma_a=ga, gamma_b=gb, history=True)
        for b in range(B):
            w, h = starts[b]
            lks, scales = [], []
            for _ in range(Itmax):
                nx = O.nmf_update_literal(X, w, h, prior, ga, gb)
                w, h = nx["ew"], nx["eh"]
                lks.append(O.likelihood_literal(X, w, h))
                wh = w @ h
                scales.append((np.abs(X * np.log(wh)).sum() + wh.sum()) / n / m)
            st = engs[b].ml_get_state()
            assert got[b]["it"] == Itmax and got[b]["reason"] == 4
            assert relerr(st["ew"], w) <= 1e-10 and relerr(st["eh"], h) <= 1e-10, (Itmax, b, relerr(st["ew"], w), relerr(st["eh"], h))
            assert np.all(np.abs(got[b]["history"] - np.array(lks)) <= 1e-10 * np.array(scales)), (Itmax, b)
            if (st["ew"] == C.EPS).any() or (st["eh"] == C.EPS).any():
                clamped = True
                assert np.array_equal(st["ew"] == C.EPS, w == C.EPS) and np.array_equal(st["eh"] == C.EPS, h == C.EPS)
        for eng in engs:
            eng.close()
    assert clamped == (prior and ga < 1.0)
    M.close()


# ---- 6. a table that does not fit at the grid of the default batch -------------------------------------------------------
def test_default_vb_factorize_when_the_update_table_overflows_at_the_batch_grid():
    """2 000 x 70 000 with ~1e6 stored entries, ranks 2-5, nrun = 4: 16 units, so the default call batches 16 at a time on grid
    (16, 16) -- ~4 500 majors per update block, beyond one block's 64 KB row at the sweep's width.  The engines keep the two-launch
    update, which the batch kernels do not take: the default call must still return what batch = 1 returns on the same grid and
    width, bit for bit."""
    import warnings
    import ccfindr_amd as C
    X = _sparse_counts(2000, 70000, 13, seed=2)
    M = C.CountMatrix(X)
    assert M.nnz <= 1_000_000 and M.empty_counts() == (0, 0)
    ranks, nrun = range(2, 6), 4
    nb = C.engine.auto_batch(M.nnz, nrun * len(ranks))
    grid, pad = C.batch_grid(nb), C.engine.padded_rank(max(ranks))
    assert nb == 16 and grid == (16, 16)
    assert update_table_stride(M, pad, grid[0], grid[1]) > UPD_TAB_WORDS
    kw = dict(ranks=ranks, nrun=nrun, verbose=0, Tol=1e-5, seed=3, Itmax=30)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = C.vb_factorize(M, **kw)
        b = C.vb_factorize(M, batch=1, grid=grid, pad_rank=pad, **kw)
    assert a.ranks == b.ranks and a.measure == b.measure and a.nsteps == b.nsteps
    for x, y in zip(a.basis + a.coeff + a.dbasis + a.dcoeff, b.basis + b.coeff + b.dbasis + b.dcoeff):
        assert np.array_equal(x, y)
    M.close()
