"""The code the sweep and update kernels run only when one workgroup's share outgrows a fixed on-chip table, on 700 x 700
matrices (tests/util_limits.py holds the cases, tests/test_limits_cpu.py proves on the host that each crosses its limit):

  1. segments longer than kLdsEvSlots = 128 slices (kernels.h sweep_side: the list is pulled in chunks, the evidence slots and
     the ticket word are reused, take_ticket_ends counts per chunk, colsum_finish runs at the first chunk end) -- VB steps in
     both update forms, the ML step, the sparse products (EV = 3), the split sweep of a partitioned group, reproducibility;
  2. the non-temporal entry stream (ld_stream(..., nt = 1), VBNMF_STREAM_NT): a cache policy, so bit for bit against nt = 0;
  3. the update kernels' unstaged gather (k_update, k_ml_update: a block beyond kStagePtr majors or kStageIds task ids reads
     the inverse index from global memory), alone and mixed with staged blocks in one launch.

Every number is held to the CPU oracles at the bounds of the tests named beside it; nothing here sets a bound of its own."""
import numpy as np
import pytest

import util_limits as U
from test_gpu_batch_oracle import UPD_TAB_WORDS, _oracle, _stats
from test_gpu_control_fold import _same
from util_layout import build_layout

pytestmark = pytest.mark.gpu

HY = U.HY
FACT = ("lw", "lh", "ew", "eh", "dw", "dh")
STEPS = 3


def relerr(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


# ---- references: computed once per process, shared, read-only -----------------------------------------------------------
_refs = {}


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def vb_reference(key, X, r, seed):
    """Start state and STEPS oracle steps from it: lkh and the four statistics of every step, the last state."""
    from ccfindr_amd import synth
    import ccfindr_amd as C
    if ("vb", key) not in _refs:
        n, m = X.shape
        wh = _freeze(synth.random_state(n, m, r, HY, seed=seed))
        upd, cur, lkh, stats = _oracle(X), wh, [], []
        for _ in range(STEPS):
            cur = upd(cur, HY, C.EPS)
            lkh.append(cur["lkh"])
            stats.append(_stats(cur))
        _refs["vb", key] = {"wh": wh, "lkh": lkh, "stats": stats, "state": _freeze({k: cur[k] for k in FACT})}
    return _refs["vb", key]


def ml_reference(key, X, r, seed):
    """Start pair and one nmf_updateR step from it (the stored-entries form for a sparse X), with its likelihood."""
    from oracle import mlnmf_oracle as OM
    if ("ml", key) not in _refs:
        n, m = X.shape
        rng = np.random.default_rng(seed)
        w, h = rng.uniform(0.05, 1.0, size=(n, r)), rng.uniform(0.05, 1.0, size=(r, m))
        if hasattr(X, "tocsc"):
            S = X.tocsc()
            o = OM.update_csc(n, m, S.indptr, S.indices, S.data, w, h, nthreads=8)
            ew, eh, lk = o["ew"], o["eh"], o["lk"]
        else:
            o = OM.nmf_update_literal(X, w, h)
            ew, eh = o["ew"], o["eh"]
            lk = OM.likelihood_literal(X, ew, eh)
        _refs["ml", key] = _freeze({"w": w, "h": h, "ew": ew, "eh": eh, "lk": float(lk)})
    return _refs["ml", key]


# ---- engines and checks -----------------------------------------------------------------------------------------------------
def make_engine(monkeypatch, M, r, pair=None, nt=None, fold=None, **kw):
    """VBEngine under the switches read at its creation: the update form (as tests/test_gpu_update_pair.py), the entry stream's
    cache policy, the control fold (as tests/test_gpu_control_fold.py)."""
    import ccfindr_amd as C
    if pair is not None:
        monkeypatch.setenv("VBNMF_NO_UPDATE_PAIR", "0" if pair else "1")
        monkeypatch.setenv("VBNMF_UPDATE_PAIR", "1" if pair else "0")
    if nt is not None:
        monkeypatch.setenv("VBNMF_STREAM_NT", "1" if nt else "0")
    if fold is not None:
        monkeypatch.setenv("VBNMF_NO_CONTROL_FOLD", "0" if fold else "1")
    return C.VBEngine(M, r, **kw)


def vb_steps(eng, wh):
    eng.set_state(wh["lw"], wh["lh"], wh["eh"])
    steps = [eng.step(HY) for _ in range(STEPS)]
    return steps, eng.get_state()


def check_vb(tag, steps, state, ref):
    """The bounds of tests/test_gpu_forced_geometry.py::test_many_segments_per_workgroup (lkh 1e-10 every step, the six factors
    1e-11 after the last) and of _three_steps_against_the_oracle (the four statistics of every step 1e-10)."""
    for t, (lkh, st) in enumerate(steps):
        e_l = abs(lkh / ref["lkh"][t] - 1)
        e_s = [abs(st[q] / ref["stats"][t][q] - 1) for q in range(4)]
        print(tag, "step", t, "lkh", e_l, "stats", e_s)
        assert e_l <= 1e-10, (tag, t, lkh, ref["lkh"][t])
        assert max(e_s) <= 1e-10, (tag, t, st, ref["stats"][t])
    errs = {k: relerr(state[k], ref["state"][k]) for k in FACT}
    print(tag, "state", errs)
    for k in FACT:
        assert state[k].shape == ref["state"][k].shape and errs[k] <= 1e-11, (tag, k, errs[k])


def ml_step(eng, ref):
    eng.ml_set_state(ref["w"], ref["h"])
    lk = eng.ml_step()
    return lk, eng.ml_likelihood(), eng.ml_get_state()


def check_ml(tag, lk, lk_again, state, ref):
    """Factors 1e-12 (test_many_segments_per_workgroup), likelihood 1e-10 (tests/test_gpu_mlnmf.py, one step)."""
    e_w, e_h, e_l = relerr(state["ew"], ref["ew"]), relerr(state["eh"], ref["eh"]), abs(lk / ref["lk"] - 1)
    print(tag, "ml ew", e_w, "eh", e_h, "lk", e_l)
    assert e_w <= 1e-12 and e_h <= 1e-12, (tag, e_w, e_h)
    assert e_l <= 1e-10 and abs(lk_again / ref["lk"] - 1) <= 1e-10, (tag, lk, lk_again, ref["lk"])


def spmm_both(eng, X, r, seed):
    rng = np.random.default_rng(seed)
    B, W = rng.standard_normal((r, X.shape[1])), rng.standard_normal((X.shape[0], r))
    return (eng.spmm(B), X @ B.T), (eng.spmm(W, transpose=True), W.T @ X)


def check_spmm(tag, pairs):
    """The bound of tests/test_gpu_spmm_svd.py::test_spmm_both_orientations."""
    for which, (got, want) in zip(("X B", "t(X) B"), pairs):
        err = np.max(np.abs(got - want)) / np.max(np.abs(want))
        print(tag, which, err)
        assert got.shape == want.shape and err <= 1e-12, (tag, which, err)


def case_key(case):
    return U.case_id(case)


# ---- 1. segments of more than 128 slices -----------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [True, False], ids=["pair", "two_launches"])
@pytest.mark.parametrize("case", U.LIMIT_CASES, ids=U.LIMIT_IDS)
def test_long_segments_three_steps_against_the_oracle(monkeypatch, case, pair):
    """Three resident steps.  In the one-launch form colsum_finish adds the per-slice column sums of a multi-chunk share: that
    this form is really taken is asserted from the layouts (the table's row fits the kernel's 64 KB)."""
    import ccfindr_amd as C
    U.set_switches(monkeypatch, case)
    X = U.case_matrix(case)
    M = C.CountMatrix(X)
    if pair:
        stride = U.update_table_stride(M, C.engine.padded_rank(case.r), case.nwg, 256)
        print(case_key(case), "update table stride", stride)
        assert stride <= UPD_TAB_WORDS, stride
    ref = vb_reference(case_key(case), X, case.r, seed=case.r)
    eng = make_engine(monkeypatch, M, case.r, pair=pair)
    steps, state = vb_steps(eng, ref["wh"])
    eng.close()
    M.close()
    check_vb(case_key(case), steps, state, ref)


@pytest.mark.parametrize("case", U.LIMIT_CASES, ids=U.LIMIT_IDS)
def test_long_segments_ml_step_against_the_oracle(monkeypatch, case):
    import ccfindr_amd as C
    U.set_switches(monkeypatch, case)
    X = U.case_matrix(case)
    M = C.CountMatrix(X)
    ref = ml_reference(case_key(case), X, case.r, seed=case.r + 1)
    eng = C.VBEngine(M, case.r)
    got = ml_step(eng, ref)
    eng.close()
    M.close()
    check_ml(case_key(case), *got, ref)


SPMM_CASES = [U.find_case(10, "counts"), U.find_case(10, "noninteger"), U.find_case(40, "counts")]


@pytest.mark.parametrize("case", SPMM_CASES, ids=[U.case_id(c) for c in SPMM_CASES])
def test_long_segments_sparse_products(monkeypatch, case):
    """k_spmm: the same list loop with EV = 3."""
    import ccfindr_amd as C
    U.set_switches(monkeypatch, case)
    X = U.case_matrix(case)
    M = C.CountMatrix(X)
    eng = C.VBEngine(M, case.r)
    pairs = spmm_both(eng, X, case.r, seed=2)
    eng.close()
    M.close()
    check_spmm(case_key(case), pairs)


# (rank 10: the denser case -- at Poisson mean 0.9 half of the cells leave the cell side's lists at 103-120 slices)
GROUP_CASES = [U.find_case(10, "counts", 1.5), U.find_case(40, "counts")]


@pytest.mark.parametrize("case", GROUP_CASES, ids=[U.case_id(c) for c in GROUP_CASES])
def test_long_segments_partitioned_group(monkeypatch, case):
    """Two partitions (k_sweep1<VB = true>, the split sweep) under the case's switches against the single engine on the default
    geometry, after the pattern of test_partition_group_loop_with_many_segments."""
    import ccfindr_amd as C
    from ccfindr_amd import synth
    from ccfindr_amd.parallel import cell_partition
    X = U.case_matrix(case)
    n, m, r = case.n, case.m, case.r
    M = C.CountMatrix(X)
    wh = synth.random_state(n, m, r, HY, seed=9)
    kw = dict(Itmax=6, Tol=0.0, n0=2, dn=1, history=True)
    whole = C.VBEngine(M, r)                                   # default geometry
    whole.set_state(wh["lw"], wh["lh"], wh["eh"])
    want = whole.run(HY, **kw)
    ref = whole.get_state()
    whole.close()
    U.set_switches(monkeypatch, case)
    cuts = cell_partition(m, 2)
    for cut in cuts:
        for side in (0, 1):
            v = build_layout(M, side, r, cols=cut)
            longest = int(U.segment_lengths(v).max())
            print(case_key(case), "partition", cut, "side", side, "longest segment", longest)
            assert v["n_wg"] == case.nwg and longest > U.LDS_EV_SLOTS, (cut, side, longest)
    comm = C.Communicator.local(len(cuts))
    parts = [C.VBEngine(M, r, cols=c, m_global=m) for c in cuts]
    for p, (b, e) in zip(parts, cuts):
        p.attach_comm(comm)
        p.set_state(wh["lw"], wh["lh"][:, b:e], wh["eh"][:, b:e])
    comm.state_finish()
    got = comm.run(HY, **kw)
    st = [p.get_state() for p in parts]
    comm.close()
    for p in parts:
        p.close()
    M.close()
    assert got["it"] == want["it"] == 6
    print(case_key(case), "history", relerr(got["history"], want["history"]), "lw", relerr(st[0]["lw"], ref["lw"]))
    assert relerr(got["history"], want["history"]) <= 1e-10
    assert np.array_equal(st[0]["lw"], st[1]["lw"])
    assert relerr(st[0]["lw"], ref["lw"]) <= 1e-9
    assert relerr(np.concatenate([q["lh"] for q in st], axis=1), ref["lh"]) <= 1e-9


REPRO_CASES = [U.find_case(10, "counts"), U.find_case(40, "counts")]


@pytest.mark.parametrize("case", REPRO_CASES, ids=[U.case_id(c) for c in REPRO_CASES])
def test_long_segments_are_bit_reproducible(monkeypatch, case):
    """Which wave pulls which slice, and in which chunk, varies from run to run; the results must not: the same three steps
    twice on one engine and once on a second one."""
    import ccfindr_amd as C
    U.set_switches(monkeypatch, case)
    X = U.case_matrix(case)
    M = C.CountMatrix(X)
    wh = vb_reference(case_key(case), X, case.r, seed=case.r)["wh"]
    a, b = C.VBEngine(M, case.r), C.VBEngine(M, case.r)
    runs = [vb_steps(a, wh), vb_steps(a, wh), vb_steps(b, wh)]
    a.close()
    b.close()
    M.close()
    for steps, state in runs[1:]:
        assert [s[0] for s in steps] == [s[0] for s in runs[0][0]]
        for k in FACT:
            assert np.array_equal(state[k], runs[0][1][k]), k


# ---- 2. the non-temporal entry stream ---------------------------------------------------------------------------------------
def _drive_both_policies(monkeypatch, M, X, r, vref, mref, with_run):
    """Everything an engine computes from the entry stream, under VBNMF_STREAM_NT=0 and =1: three VB steps in both update forms
    (and, with_run, a 10-iteration device loop with the hyper-parameter updates on), one ML step, both sparse products."""
    out = []
    for nt in (False, True):
        res = {}
        for pair in (True, False):
            eng = make_engine(monkeypatch, M, r, pair=pair, nt=nt)
            res["vb", pair] = vb_steps(eng, vref["wh"])
            if with_run:
                eng.set_state(vref["wh"]["lw"], vref["wh"]["lh"], vref["wh"]["eh"])
                res["run", pair] = (eng.run(HY, Itmax=10, Tol=0.0, n0=3, dn=1, flags=(True,) * 4, history=True), eng.get_state())
            if pair:
                res["ml"] = ml_step(eng, mref)
                res["spmm"] = spmm_both(eng, X, r, seed=3)
            eng.close()
        out.append(res)
    return out


def _check_policies(tag, out, vref, mref, with_run):
    plain, nt = out
    for pair in (True, False):
        (s0, st0), (s1, st1) = plain["vb", pair], nt["vb", pair]
        assert s0 == s1, (tag, pair, s0, s1)                   # lkh and the four statistics of every step
        for k in FACT:
            assert np.array_equal(st0[k], st1[k]), (tag, pair, k)
        if with_run:
            (r0, q0), (r1, q1) = plain["run", pair], nt["run", pair]
            _same(r0, r1)
            assert r0["it"] == 10 and r0["history"].shape == (10, 9)
            for k in FACT:
                assert np.array_equal(q0[k], q1[k]), (tag, pair, "run", k)
    (lk0, la0, m0), (lk1, la1, m1) = plain["ml"], nt["ml"]
    assert lk0 == lk1 and la0 == la1 and np.array_equal(m0["ew"], m1["ew"]) and np.array_equal(m0["eh"], m1["eh"]), tag
    for (g0, _), (g1, _) in zip(plain["spmm"], nt["spmm"]):
        assert np.array_equal(g0, g1), tag
    # ... and the non-temporal results are right, not merely equal
    for pair in (True, False):
        check_vb(f"{tag} nt pair={pair}", *nt["vb", pair], vref)
    check_ml(tag + " nt", *nt["ml"], mref)
    check_spmm(tag + " nt", nt["spmm"])


NT_SMALL = [(r, kind) for r in (3, 10, 30, 40, 80) for kind in ("counts", "noninteger")] + [(10, "split")]


@pytest.mark.parametrize("r,kind", NT_SMALL, ids=[f"r{r}_{kind}" for r, kind in NT_SMALL])
def test_stream_policy_changes_no_bit(monkeypatch, r, kind):
    """260 x 700 on the default geometry: the packed, the wide and the split stream; the two-buffer, the one-row-buffer and the
    shared-lane loops."""
    import ccfindr_amd as C
    n, m = 260, 700
    X = U.limit_matrix(n, m, 0.5, kind, seed=300 + r)
    M = C.CountMatrix(X)
    key = f"nt_{r}_{kind}"
    vref, mref = vb_reference(key, X, r, seed=r), ml_reference(key, X, r, seed=r + 1)
    with_run = r in (10, 40)
    out = _drive_both_policies(monkeypatch, M, X, r, vref, mref, with_run)
    M.close()
    _check_policies(key, out, vref, mref, with_run)


NT_LONG = [U.find_case(10, "noninteger"), U.find_case(40, "counts")]


@pytest.mark.parametrize("case", NT_LONG, ids=[U.case_id(c) for c in NT_LONG])
def test_stream_policy_changes_no_bit_on_long_segments(monkeypatch, case):
    import ccfindr_amd as C
    U.set_switches(monkeypatch, case)
    X = U.case_matrix(case)
    M = C.CountMatrix(X)
    key = case_key(case)
    vref, mref = vb_reference(key, X, case.r, seed=case.r), ml_reference(key, X, case.r, seed=case.r + 1)
    out = _drive_both_policies(monkeypatch, M, X, case.r, vref, mref, True)
    M.close()
    _check_policies(key, out, vref, mref, True)


# ---- 3. the update kernels' unstaged gather ---------------------------------------------------------------------------------
@pytest.mark.parametrize("g", U.GATHER_CASES, ids=U.GATHER_IDS)
def test_unstaged_gather_against_the_oracles(monkeypatch, g):
    """Two-launch form, so that k_update itself gathers: three VB steps and one ML step (k_ml_update) against the oracles."""
    import ccfindr_amd as C
    U.set_gather_switches(monkeypatch, g)
    monkeypatch.setenv("VBNMF_NO_UPDATE_PAIR", "1")
    monkeypatch.setenv("VBNMF_UPDATE_PAIR", "0")
    X = U.gather_matrix(g.name)
    n, m = X.shape
    M = C.CountMatrix(X)
    key = f"gather_{g.name}_{g.r}"
    vref, mref = vb_reference(key, X, g.r, seed=5), ml_reference(key, X, g.r, seed=6)
    eng = C.VBEngine(M, g.r, grid=g.grid)
    steps, state = vb_steps(eng, vref["wh"])
    ml = ml_step(eng, mref)
    eng.close()
    M.close()
    check_vb(key, steps, state, vref)
    check_ml(key, *ml, mref)


@pytest.mark.parametrize("g", U.GATHER_CASES, ids=U.GATHER_IDS)
def test_unstaged_gather_with_the_folded_control_step(monkeypatch, g):
    """The fold's prologue sits next to the staging code in k_update: a 6-iteration device loop with it against the same loop
    with the separate control kernel, bit for bit (as tests/test_gpu_control_fold.py)."""
    import ccfindr_amd as C
    U.set_gather_switches(monkeypatch, g)
    X = U.gather_matrix(g.name)
    M = C.CountMatrix(X)
    wh = vb_reference(f"gather_{g.name}_{g.r}", X, g.r, seed=5)["wh"]
    runs = []
    for fold in (True, False):
        eng = make_engine(monkeypatch, M, g.r, pair=False, fold=fold, grid=g.grid)
        eng.set_state(wh["lw"], wh["lh"], wh["eh"])
        out = eng.run(HY, Itmax=6, Tol=0.0, n0=2, dn=1, flags=(True,) * 4, history=True)
        runs.append((out, eng.get_state()))
        eng.close()
    M.close()
    _same(runs[0][0], runs[1][0])
    assert runs[0][0]["it"] == 6 and runs[0][0]["reason"] == 4
    for k in FACT:
        assert np.array_equal(runs[0][1][k], runs[1][1][k]), k
