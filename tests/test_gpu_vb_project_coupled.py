"""GPU parity of the coupled VB projection (ccfindr_amd.vb_project with hyper_update= / stop="global",
vbnmf_matrix_vb_project_coupled; csrc/vbproject.h, k_vbp_step and k_vbp_control) against tests/util_vb_project_coupled.py, the
numpy restatement that tests/test_vb_project_coupled_cpu.py ties to the committed oracle's hyper_update and vb_iterate -- and,
with both flags off, bit for bit against the per-cell kernel k_vb_project, which tests/test_gpu_project_mp.py holds to 50-digit
arithmetic at every rank width.

Tolerances (fp64), those of tests/test_gpu_vb_project.py: one step on identical inputs -- lh, eh, dh and the new (ah, bh) max
relative error <= 1e-12, evidences <= 1e-10; trajectories (here up to 234 steps: a permuted summation order moves eh, lh by
<= 3e-12 and ah by <= 6e-15 over such runs) -- 1e-9.
"""
import functools
import importlib

import numpy as np
import pytest

import util_vb_project as U
import util_vb_project_coupled as UC
from test_gpu_vb_project import P, posterior, relerr

pytestmark = pytest.mark.gpu

EPS = U.EPS
KEYS = ("lh", "eh", "dh", "ev", "it", "reason", "hyper", "steps", "why", "E", "history")


def run_columns(X, lw, ew, lh0, ah, bh, flags, **kw):
    """vb_project_coupled_columns over all cells of the dense X -> dict."""
    import ccfindr_amd as C
    M = C.CountMatrix(X)
    try:
        return dict(zip(KEYS, P().vb_project_coupled_columns(M, lw, ew, lh0, ah, bh, 0, X.shape[1], flags, **kw)))
    finally:
        M.close()


def one_step_bounds(got, want, what):
    """(a)'s bounds: lh, eh, dh 1e-12; cell evidences and E 1e-10; the new (ah, bh) 1e-12.  ``got``: a VBProjection."""
    errs = (relerr(got.lcoeff[0], want["lh"]), relerr(got.coeff[0], want["eh"]), relerr(got.dcoeff[0] ** 2, want["dh"]),
            relerr(got.cell_evidence, want["ev"]), abs(got.evidence / want["E"] - 1),
            abs(got.hyper["ah"] / want["hyper"][0] - 1), abs(got.hyper["bh"] / want["hyper"][1] - 1))
    print(what + ": lh %.3g eh %.3g dh %.3g, cell evidence %.3g E %.3g, ah %.3g bh %.3g" % errs)
    assert max(errs[:3]) <= 1e-12
    assert max(errs[3:5]) <= 1e-10
    assert max(errs[5:]) <= 1e-12


# ---- (a) one step, with the update ------------------------------------------------------------------------------------------
def test_one_step_with_the_update():
    """Itmax = 1, n0 = 0, flags (T, T), seed 1 drawn with (0.6, 3), from (1, 1): the step, the evidences and the updated pair."""
    import ccfindr_amd as C
    c = UC.case(1, 0.6, 3.0)
    hy = {"ah": 1.0, "bh": 1.0}
    p = C.vb_project(c["x"], (c["ew"], c["sd"]), hyper=hy, hyper_update=(True, True), hyper_n0=0, Itmax=1, history=True)
    lw = C.posterior_basis((c["ew"], c["sd"]), hyper=hy)[0]
    want = UC.project_coupled(c["x"], lw, c["ew"], c["lh0"], 1.0, 1.0, flags=(True, True), n0=0, Itmax=1)
    assert want["reason"] == 4 and want["newton_margin"] > 1e-6 and want["hyper"] != (1.0, 1.0)
    one_step_bounds(p, want, "seed 1, one step")
    assert np.all(p.nsteps == 1) and np.all(p.reason == 4) and p.hyper0 == hy
    assert p.history.shape == (1, 5) and p.history[0, 0] == p.evidence and tuple(p.history[0, 3:]) == (p.hyper["ah"], p.hyper["bh"])
    assert relerr(p.history[0, 1:3], want["history"][0, 1:3]) <= 1e-12
    assert abs(p.lml_cells - p.cell_evidence.sum() / 90 / 140) <= 1e-15 * abs(p.lml_cells)


# ---- (b) the gate -----------------------------------------------------------------------------------------------------------
def test_the_gate_n0_and_dn():
    """n0 = 3, dn = 2, Itmax = 12, Tol = 0: the pair moves at steps 4, 6, .., 12 only -- rows 1 to 3 and every odd row carry the
    (ah, bh) of the row before, bit for bit -- and all rows follow the restatement, 1e-9."""
    import ccfindr_amd as C
    c = UC.case(1, 0.6, 3.0)
    hy = {"ah": 1.0, "bh": 1.0}
    p = C.vb_project(c["x"], (c["ew"], c["sd"]), hyper=hy, hyper_update=(True, True), hyper_n0=3, hyper_dn=2, Itmax=12, Tol=0.0,
                     history=True)
    want = UC.project_coupled(c["x"], c["lw"], c["ew"], c["lh0"], 1.0, 1.0, flags=(True, True), n0=3, dn=2, Itmax=12, Tol=0.0)
    assert want["reason"] == 4 and want["newton_margin"] > 1e-6
    h = p.history
    assert h.shape == (12, 5) and np.all(p.nsteps == 12) and np.all(p.reason == 4)
    before = np.vstack(([1.0, 1.0], h[:-1, 3:]))
    for row in range(1, 13):
        same = np.array_equal(h[row - 1, 3:], before[row - 1])
        assert same == (row <= 3 or row % 2 == 1), row
    err = relerr(h, want["history"])
    print("history against the restatement: %.3g" % err)
    assert err <= 1e-9
    assert tuple(h[-1, 3:]) == (p.hyper["ah"], p.hyper["bh"]) and h[-1, 0] == p.evidence


# ---- (c), (d) column lengths around the pass; every compiled width --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lengths_case(r):
    """n = 560: columns of 1, 2, per - 1, per, per + 1 and 2 per + 1 stored entries, per = the stored entries one pass of the
    kernel's workgroup takes at rank r (the kernel's own constant) -> (X, ew, sd, lw, lh0)."""
    per = P().vb_pass_entries(r)
    n = 560
    lengths = [1, 2, per - 1, per, per + 1, 2 * per + 1]
    assert max(lengths) <= n
    rng = np.random.default_rng(4000 + r)
    X = np.zeros((n, len(lengths)))
    for j, L in enumerate(lengths):
        X[rng.permutation(n)[:L], j] = rng.integers(1, 6, size=L)
    assert [int(v) for v in (X > 0).sum(axis=0)] == lengths
    ew, sd, lw = posterior(n, r, rng)
    return np.asfortranarray(X), ew, sd, lw, rng.uniform(0.05, 1.0, size=(r, len(lengths)))


@pytest.mark.parametrize("r", [5, 33, 65])
def test_flags_off_equals_the_per_cell_kernel_bit_for_bit(r):
    """Flags off, stop="global", Tol = 0, Itmax 1, 2 and 5, over columns shorter than, equal to and longer than one and two
    passes, with one, two and four lanes per entry: lh, eh, dh and the cell evidences are those of stop="cell", bit for bit."""
    import ccfindr_amd as C
    X, ew, sd, lw, lh0 = lengths_case(r)
    hy = {"ah": 0.8, "bh": 1.7}
    for k in (1, 2, 5):
        g = C.vb_project(X, (ew, sd), hyper=hy, stop="global", Tol=0.0, Itmax=k, lh0=lh0)
        cell = C.vb_project(X, (ew, sd), hyper=hy, stop="cell", Tol=0.0, Itmax=k, lh0=lh0)
        for name in ("lcoeff", "coeff", "dcoeff"):
            assert np.array_equal(getattr(g, name)[0], getattr(cell, name)[0]), (k, name)
        assert np.array_equal(g.cell_evidence, cell.cell_evidence), k
        assert np.all(np.isfinite(g.cell_evidence))
        assert np.all(g.nsteps == k) and np.all(g.reason == 4) and np.all(cell.nsteps == k)
        assert g.hyper == hy and g.hyper0 == hy and cell.hyper == hy
        assert abs(g.evidence - cell.evidence) <= 1e-14 * np.abs(g.cell_evidence).sum()      # (E: the control step's order against numpy's)


def padded_ranks():
    from ccfindr_amd import _native as N
    L = N.load()
    return sorted({int(L.vbnmf_padded_rank(r)) for r in range(1, N.MAX_RANK + 1)})


def test_there_are_24_compiled_widths():
    assert len(padded_ranks()) == 24


@pytest.mark.parametrize("R", [2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 26, 28, 30, 32, 40, 48, 56, 64, 80, 96, 112, 128])
def test_every_compiled_width(R):
    """r = R at each of the 24 padded ranks the kernels are compiled for, the six column lengths of (c), one step with
    n0 = 0 and flags (T, T): the bounds of (a)."""
    import ccfindr_amd as C
    assert R in padded_ranks()
    X, ew, sd, lw, lh0 = lengths_case(R)
    hy = {"ah": 0.8, "bh": 1.7}
    want = UC.project_coupled(X, C.posterior_basis((ew, sd), hyper=hy)[0], ew, lh0, 0.8, 1.7, flags=(True, True), n0=0, Itmax=1)
    assert want["reason"] == 4 and want["newton_margin"] > 1e-6
    p = C.vb_project(X, (ew, sd), hyper=hy, hyper_update=(True, True), hyper_n0=0, Itmax=1, lh0=lh0)
    one_step_bounds(p, want, f"R = {R}")
    assert np.all(p.nsteps == 1) and np.all(p.reason == 4)


# ---- (e) full runs ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def full_case(seed, ab, start, flags):
    c = UC.case(seed, *ab)
    return c, UC.project_coupled(c["x"], c["lw"], c["ew"], c["lh0"], *start, flags=flags, Tol=1e-5)


@pytest.mark.parametrize("seed,ab,start", UC.CONDITIONS, ids=[f"seed{s}-a{ab[0]}" for s, ab, st in UC.CONDITIONS])
def test_full_runs(seed, ab, start):
    """To Tol = 1e-5 with flags (T, T) and (F, T): ``it`` and ``reason`` are the restatement's (its decisions are clear:
    tests/test_vb_project_coupled_cpu.py), the pair, eh, lh and the evidences 1e-9.  A second run gives the same bits; (T, F)
    gives the bits of (T, T) (R/bayesian.R:50-51 set bh in both branches); under (F, T) ah comes back with its input bits."""
    import ccfindr_amd as C
    hy = {"ah": start[0], "bh": start[1]}
    runs = {}
    for flags in ((True, True), (False, True)):
        c, want = full_case(seed, ab, start, flags)
        assert want["reason"] == 1 and want["stop_margin"] > 1e-3 and want["newton_margin"] > 1e-6
        p = C.vb_project(c["x"], (c["ew"], c["sd"]), hyper=hy, hyper_update=flags, Tol=1e-5, history=True)
        runs[flags] = p
        errs = (relerr(p.lcoeff[0], want["lh"]), relerr(p.coeff[0], want["eh"]), relerr(p.cell_evidence, want["ev"]),
                abs(p.evidence / want["E"] - 1), abs(p.hyper["ah"] / want["hyper"][0] - 1), abs(p.hyper["bh"] / want["hyper"][1] - 1))
        print(f"seed {seed}, drawn with {ab}, from {start}, flags {flags}: it {p.nsteps[0]} (restatement {want['it']}), "
              "lh %.3g eh %.3g cell evidence %.3g E %.3g ah %.3g bh %.3g" % errs)
        assert np.all(p.nsteps == want["it"]) and np.all(p.reason == 1)
        assert max(errs) <= 1e-9
        assert p.history.shape == (want["it"], 5) and relerr(p.history, want["history"]) <= 1e-9
        assert p.hyper0 == hy
        again = C.vb_project(c["x"], (c["ew"], c["sd"]), hyper=hy, hyper_update=flags, Tol=1e-5, history=True)
        for name in ("lcoeff", "coeff", "dcoeff"):
            assert np.array_equal(getattr(again, name)[0], getattr(p, name)[0]), name
        assert np.array_equal(again.cell_evidence, p.cell_evidence) and np.array_equal(again.history, p.history)
        assert again.hyper == p.hyper and again.evidence == p.evidence and np.array_equal(again.nsteps, p.nsteps)
    assert runs[(False, True)].hyper["ah"] == start[0]
    c = UC.case(seed, *ab)
    tf = C.vb_project(c["x"], (c["ew"], c["sd"]), hyper=hy, hyper_update=(True, False), Tol=1e-5, history=True)
    tt = runs[(True, True)]
    for name in ("lcoeff", "coeff", "dcoeff"):
        assert np.array_equal(getattr(tf, name)[0], getattr(tt, name)[0]), name
    assert np.array_equal(tf.cell_evidence, tt.cell_evidence) and np.array_equal(tf.history, tt.history)
    assert tf.hyper == tt.hyper and tf.evidence == tt.evidence and np.array_equal(tf.nsteps, tt.nsteps)


# ---- (f) more cells than the control kernel has threads and the step grid has workgroups -------------------------------------------
def test_more_cells_than_threads_and_workgroups():
    """n = 60, m = 2500 (> 1024 threads of the control kernel, > 2048 workgroups of the step grid on a 256-CU part), r = 4,
    about 10 % stored, three steps with n0 = 0, flags (T, T): 1e-9 against the restatement."""
    rng = np.random.default_rng(77)
    n, m, r = 60, 2500, 4
    X = np.where(rng.uniform(size=(n, m)) < 0.10, rng.integers(1, 6, size=(n, m)), 0).astype(np.float64)
    X[0, X.sum(axis=0) == 0] = 1.0
    X = np.asfortranarray(X)
    ew, sd, lw = posterior(n, r, rng)
    lh0 = U.default_start(X, ew)
    want = UC.project_coupled(X, lw, ew, lh0, 1.0, 1.0, flags=(True, True), n0=0, Itmax=3, Tol=0.0)
    assert want["reason"] == 4 and want["newton_margin"] > 1e-6
    got = run_columns(X, lw, ew, lh0, 1.0, 1.0, (True, True), n0=0, Itmax=3, Tol=0.0, history_rows=3)
    errs = [relerr(got[k], want[k]) for k in ("lh", "eh", "dh", "ev")] + [abs(got["E"] / want["E"] - 1),
                                                                          relerr(np.array(got["hyper"]), np.array(want["hyper"])),
                                                                          relerr(got["history"], want["history"])]
    print("2500 cells, 3 steps: lh %.3g eh %.3g dh %.3g cell evidence %.3g E %.3g hyper %.3g history %.3g" % tuple(errs))
    assert max(errs) <= 1e-9
    assert got["steps"] == 3 and got["why"] == 4 and np.all(got["it"] == 3) and np.all(got["reason"] == 4)


# ---- (g) stops --------------------------------------------------------------------------------------------------------------
def test_itmax_stops_all_cells():
    import ccfindr_amd as C
    c, want = full_case(1, (0.6, 3.0), (1.0, 1.0), (True, True))
    assert want["it"] > 7
    p = C.vb_project(c["x"], (c["ew"], c["sd"]), hyper={"ah": 1.0, "bh": 1.0}, hyper_update=(True, True), Tol=1e-5, Itmax=7)
    assert p.nsteps.shape == (140,) and np.all(p.nsteps == 7) and np.all(p.reason == 4)
    assert p.hyper == {"ah": 1.0, "bh": 1.0}                       # (the default n0 = 10: no update yet)
    assert relerr(p.coeff[0], want_at(c, 7)["eh"]) <= 1e-9


def want_at(c, k):
    return UC.project_coupled(c["x"], c["lw"], c["ew"], c["lh0"], 1.0, 1.0, flags=(True, True), Itmax=k, Tol=1e-5)


def test_nan_ends_the_run_at_step_one():
    """One NaN in lw, the default n0: E is NaN after the first step -- reason 3 for every cell, at step 1, status 0."""
    c = UC.case(1, 0.6, 3.0)
    bad = c["lw"].copy()
    bad[17, 2] = np.nan
    assert (c["x"][17] != 0).any()
    got = run_columns(c["x"], bad, c["ew"], c["lh0"], 1.0, 1.0, (True, True), Itmax=50)      # (returns: status 0)
    assert got["steps"] == 1 and got["why"] == 3 and np.isnan(got["E"])
    assert np.all(got["it"] == 1) and np.all(got["reason"] == 3) and got["hyper"] == (1.0, 1.0)


def test_a_failed_hyper_update_is_reason_5():
    """At the ABI level: one all-zero column, fudge = 0, ah = 1e-4, n0 = 0.  exp(psi(1e-4)) underflows to 0, so that column's lh
    is 0, mean(log lh) is -inf and the Newton step is not finite: the bounded path -- reason 5 at step 1, status 0, and the
    hyper-parameters come back unchanged."""
    c = UC.case(1, 0.6, 3.0)
    X = c["x"].copy(order="F")
    X[:, 6] = 0.0
    want = UC.project_coupled(X, c["lw"], c["ew"], c["lh0"], 1e-4, 1.0, flags=(True, True), n0=0, fudge=0.0, Itmax=20)
    assert want["reason"] == 5 and want["it"] == 1 and want["hyper"] == (1e-4, 1.0)
    got = run_columns(X, c["lw"], c["ew"], c["lh0"], 1e-4, 1.0, (True, True), n0=0, fudge=0.0, Itmax=20, history_rows=20)
    assert got["steps"] == 1 and got["why"] == 5 and got["hyper"] == (1e-4, 1.0)
    assert np.all(got["it"] == 1) and np.all(got["reason"] == 5)
    assert np.all(got["lh"][:, 6] == 0.0) and got["history"].shape == (1, 5) and got["history"][0, 1] == -np.inf
    assert tuple(got["history"][0, 3:]) == (1e-4, 1.0)
    assert importlib.import_module("ccfindr_amd.project").REASONS[5].startswith("hyper-parameter update failed")


# ---- (h) what it is for -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_the_update_raises_the_total_evidence(seed):
    """Counts drawn with (0.6, 3), projected from (1, 1): the total evidence with hyper_update=(True, True) exceeds that of
    stop="global" without flags at the same Tol, and the pair ends near what the counts were drawn with."""
    import ccfindr_amd as C
    c = UC.case(seed, 0.6, 3.0)
    hy = {"ah": 1.0, "bh": 1.0}
    fixed = C.vb_project(c["x"], (c["ew"], c["sd"]), hyper=hy, stop="global", Tol=1e-5)
    both = C.vb_project(c["x"], (c["ew"], c["sd"]), hyper=hy, hyper_update=(True, True), Tol=1e-5)
    print(f"seed {seed}: E fixed prior {fixed.evidence!r} in {fixed.nsteps[0]} steps, updated prior {both.evidence!r} in {both.nsteps[0]} steps, "
          f"(ah, bh) -> ({both.hyper['ah']:.4f}, {both.hyper['bh']:.4f})")
    assert np.all(fixed.reason == 1) and np.all(both.reason == 1) and fixed.hyper == hy
    assert both.evidence > fixed.evidence
    assert 0.7 < both.hyper["ah"] < 1.0 and 2.5 < both.hyper["bh"] < 3.5


def test_defaults_take_the_per_cell_path():
    """Without the new arguments vb_project is the per-cell projection: cells stop on their own, evidence = sum(cell_evidence)."""
    import ccfindr_amd as C
    c = UC.case(1, 0.6, 3.0)
    hy = {"ah": 1.0, "bh": 1.0}
    p = C.vb_project(c["x"], (c["ew"], c["sd"]), hyper=hy, Tol=1e-5)
    assert len(set(p.nsteps.tolist())) > 5 and p.history is None and p.hyper == hy and p.hyper0 == hy
    assert p.evidence == float(p.cell_evidence.sum())
    M = C.CountMatrix(c["x"])
    got = P().vb_project_columns(M, C.posterior_basis((c["ew"], c["sd"]), hyper=hy)[0], c["ew"], c["lh0"], 1.0, 1.0, 0, 140, Tol=1e-5)
    M.close()
    assert np.array_equal(got[1], p.coeff[0]) and np.array_equal(got[3], p.cell_evidence) and np.array_equal(got[4], p.nsteps)
