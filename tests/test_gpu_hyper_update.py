"""The device's hyper-parameter Newton update (csrc/kernels.h dev_hyper_update_pair, reference R/bayesian.R:2-53) against
50-digit math (tests/util_mp_hyper.py): the traced two-lane routine itself on the seeded grid of
tests/test_hyper_update_cpu.py, in one launch, and its four call sites -- the fold of k_update / update2_body
(VBEngine.run), k_update2_batch (run_batch), k_control behind a local group's exchange, k_vbp_control (the coupled
vb_project) -- through the history rows of the public API: every row carries the step's statistics and the
hyper-parameters after the update, the row before (or the start) those before it, so each row is held to the 50-digit
whole update of exactly those doubles, not to another engine.

Bounds: those of tests/test_hyper_update_cpu.py (its docstring has the measured figures) -- trigamma 2 x the plain-float
series' own worst error (1.62e-15); per iteration the derived tolerance of util_mp_hyper.step_tolerance; whole updates
10 x the committed oracle's own error against 50-digit math in the start shape's decade, floor 1e-12.

Measured on the MI355X: trigamma worst 8.1e-16 (x = 10.00015; bound 1.62e-15); the traced routine on the 1 950 cases:
25 622 transitions, worst error 0.17 of the per-iteration tolerance, whole updates off by at most 1.9e-05 (start shapes
above 1e5; tolerance there 1.3e-04), nothing skipped as threshold- or halving-adjacent (cap 5 %), 539 rootless cases
followed until fp64 no longer determines the step and then held to `failed` -- the same figures as the host build's,
whose iterates the device's equal on this grid.

No test here hands a kernel a shape or scale that is not a positive finite number: those are refused at the ABI, before any
launch, which the last tests check.
"""
import ctypes

import numpy as np
import pytest

import util_mp_hyper as U
import util_special as S

pytestmark = pytest.mark.gpu

KEYS = ("aw", "bw", "ah", "bh")
STARTS = [(0.05, 2.0, 3.0, 0.3), (40.0, 0.7, 0.5, 9.0), (1.0, 1.0, 1.0, 1.0)]
FLAGS = [(1, 1, 1, 1), (1, 0, 0, 0), (0, 0, 1, 0), (0, 1, 0, 1), (0, 0, 0, 0)]


# ---- the routine itself -----------------------------------------------------------------------------------------------
def test_trigamma_device_build():
    xs = U.trigamma_grid()
    assert np.all(xs > 0) and np.all(np.isfinite(xs))
    err = U.trigamma_rel_err(xs, S.evaluate(7, xs, device=True))
    print("trigamma device: worst %.3g at x = %r, bound %.3g" % (err.max(), xs[err.argmax()], U.trigamma_bound()))
    assert err.max() <= U.trigamma_bound(), (err.max(), xs[err.argmax()])


_GOT = {}


def _device_results():
    """The grid through vbnmf_test_hyper_update_device: ONE launch, one wave per case; shared by the tests below."""
    if "d" not in _GOT:
        G = U.case_grid()
        assert np.all(np.isfinite(G["hyper"])) and np.all(G["hyper"] > 0)
        _GOT["d"] = U.run_hook(G["flags"], G["stats"], G["hyper"], device=True)
    return _GOT["d"]


def test_device_hook_on_the_grid():
    """Every traced iteration of both lanes from the device's own iterate, every stop decision, iters / failed, the store
    rules and the whole update (U.check_hook states each), then the skip cap on what was actually skipped."""
    fig = U.check_hook(_device_results())
    print("device hook:", fig)
    n = len(U.case_grid()["flags"])
    assert fig["skipped_tol"] + fig["skipped_zero"] <= 0.05 * n
    assert fig["transitions"] > 20000


def test_host_and_device_hooks_agree():
    """Same iters and failed on every case whose 50-digit update has no decision at its threshold and no ill-conditioned
    step; the final shapes within the sum of the two builds' per-iteration tolerances of their last steps, plus a tenth of
    the distance of the iterates those steps started from (the Newton map's slope where the stop |d| / a < 0.032 holds)."""
    G, ref = U.case_grid(), U.reference()
    dev = _device_results()
    host = U.run_hook(G["flags"], G["stats"], G["hyper"], device=False)
    compared = 0
    for c in range(len(ref)):
        R = ref[c]
        if R["near_tol"] or R["near_zero"]:
            continue
        tag = (c, G["stratum"][c], tuple(G["flags"][c]), tuple(G["hyper"][c]), tuple(G["stats"][c]))
        assert dev["failed"][c] == host["failed"][c], tag
        if R["ill"]:
            continue
        assert dev["iters"][c] == host["iters"][c], tag
        compared += 1
        if dev["failed"][c]:
            continue
        it, fl, st, hy = int(dev["iters"][c]), G["flags"][c], G["stats"][c], G["hyper"][c]
        assert dev["hyper"][c][1] == host["hyper"][c][1] and dev["hyper"][c][3] == host["hyper"][c][3], tag
        for s in range(2):
            if it == 0:
                assert dev["hyper"][c][2 * s] == host["hyper"][c][2 * s], tag
                continue
            prev = [float(hy[2 * s]) if it == 1 else float(h["trace"][c][s, it - 2]) for h in (dev, host)]
            tol = sum(U.step_tolerance(U.newton_step(p, hy[2 * s + 1], st[s], st[2 + s], fl[2 * s]), p) for p in prev)
            diff = abs(dev["hyper"][c][2 * s] - host["hyper"][c][2 * s])
            assert diff <= float(tol) + 0.1 * abs(prev[0] - prev[1]), tag + (s, diff, float(tol), prev)
    assert compared >= 1300


def test_device_hook_refuses_what_a_kernel_must_not_see():
    """A shape or scale that is not a positive finite number: VBNMF_ERR_BAD_ARG from the hook, before a launch."""
    import ccfindr_amd as C
    for bad in (0.0, -1.0, np.nan, np.inf):
        for pos in range(4):
            hy = np.array([[1.0, 1.0, 1.0, 1.0], [2.0, 1.0, 2.0, 1.0]])
            hy[1, pos] = bad
            with pytest.raises(C.VBNMFError) as ei:
                U.run_hook(np.ones((2, 4), dtype=np.int32), np.tile([-0.3, -0.2, 1.1, 0.9], (2, 1)), hy, device=True)
            assert ei.value.code == 1


# ---- the call sites, through the history rows -------------------------------------------------------------------------
def _matrix():
    from ccfindr_amd import synth
    return synth.drop_empty(synth.simulate_data(60, (40, 50), seed=3, sparse=False))


def _raw_run(fn, handle, hyper, Itmax, flags, fudge=2.220446049250313e-16, Tol=0.0, n0=0):
    """vbnmf_engine_run / vbnmf_group_run at the ABI (dn = 1, with history): reason 3 is returned, not raised."""
    from ccfindr_amd import _native as N
    hy = (ctypes.c_double * 4)(*(float(v) for v in hyper))
    fl = (ctypes.c_int32 * 4)(*(int(f) for f in flags))
    it, reason, lk0, lkh = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double(), ctypes.c_double()
    hist = np.zeros((Itmax, 9))
    N.check(fn(handle, hy, float(fudge), int(Itmax), float(Tol), int(n0), 1, fl, ctypes.byref(it), ctypes.byref(lk0), ctypes.byref(lkh),
               ctypes.byref(reason), N.dptr(hist), Itmax))
    return {"it": it.value, "reason": reason.value, "hyper": tuple(float(v) for v in hy), "history": hist[:it.value].copy()}


def check_rows(rows_stats, rows_hyper, start, flags, reason, failed_reason, where):
    """rows_stats [it, 4], rows_hyper [it, 4] (after each step's update), the start hyper-parameters and the flags: every
    row against the 50-digit whole update of that row's statistics from the row before's hyper-parameters."""
    before = np.array(start, dtype=np.float64)
    checked = 0
    for i in range(len(rows_stats)):
        st, after = rows_stats[i], rows_hyper[i]
        R = U.update(flags, st, before)
        tag = (where, tuple(flags), tuple(start), i, tuple(st), tuple(before), tuple(after))
        if R["near_tol"] or R["near_zero"] or R["ill"]:
            before = after
            continue
        if R["failed"]:
            assert i == len(rows_stats) - 1 and reason == failed_reason, tag
            assert np.array_equal(np.ascontiguousarray(after).view(np.uint64), np.ascontiguousarray(before).view(np.uint64)), tag
            return checked
        for s in (0, 2):
            rel = float(abs(U._f(after[s]) - R["hyper"][s]) / R["hyper"][s])
            assert rel <= U.whole_update_tolerance(before[s]), tag + (s, rel, U.whole_update_tolerance(before[s]))
        assert after[1] == float(R["hyper"][1]) and after[3] == float(R["hyper"][3]), tag
        if sum(flags) == 0 or (flags[0] + flags[2] == 0):
            assert after[0] == before[0] and after[2] == before[2], tag
        checked += 1
        before = after
    assert reason != failed_reason, (where, tuple(flags), tuple(start), reason)
    return checked


def _state(X, r, seed=2):
    from ccfindr_amd import synth
    return synth.random_state(X.shape[0], X.shape[1], r, dict(zip(KEYS, (1.0,) * 4)), seed=seed)


def test_engine_run_rows_against_50_digit_updates():
    """VBEngine.run: the control fold of k_update / update2_body."""
    import ccfindr_amd as C
    X = _matrix()
    wh = _state(X, 3)
    eng = C.VBEngine(C.CountMatrix(X), 3)
    checked = 0
    for start in STARTS:
        for flags in FLAGS:
            eng.set_state(wh["lw"], wh["lh"], wh["eh"])
            got = _raw_run(eng._lib.vbnmf_engine_run, eng._h, start, 10, flags)
            assert got["it"] == 10 and got["reason"] == 4, (start, flags, got["reason"])
            h = got["history"]
            checked += check_rows(h[:, 1:5], h[:, 5:9], start, flags, got["reason"], 3, "engine_run")
            assert got["hyper"] == tuple(h[-1, 5:9])
    eng.close()
    assert checked >= 140


def test_batch_run_rows_against_50_digit_updates():
    """run_batch with B = 4: k_update2_batch, every engine following its own control block."""
    import ccfindr_amd as C
    X = _matrix()
    M = C.CountMatrix(X)
    B = 4
    engs = [C.VBEngine(M, 2, grid=C.batch_grid(B)) for _ in range(B)]
    states = [_state(X, 2, seed=10 + b) for b in range(B)]
    starts = STARTS + [(0.3, 0.5, 0.2, 0.4)]
    checked = 0
    for flags in FLAGS:
        for e, wh in zip(engs, states):
            e.set_state(wh["lw"], wh["lh"], wh["eh"])
        res = C.run_batch(engs, [dict(zip(KEYS, s)) for s in starts], Itmax=8, Tol=0.0, n0=0, dn=1, flags=flags, history=True)
        for b in range(B):
            assert res[b]["it"] == 8 and res[b]["reason"] == 4, (flags, b, res[b]["reason"])
            h = res[b]["history"]
            checked += check_rows(h[:, 1:5], h[:, 5:9], starts[b], flags, res[b]["reason"], 3, "run_batch[%d]" % b)
    for e in engs:
        e.close()
    assert checked >= 150


def _group(M, r, m, wh, P=2):
    import ccfindr_amd as C
    from ccfindr_amd.parallel import cell_partition
    cuts = cell_partition(m, P)
    comm = C.Communicator.local(len(cuts))
    parts = [C.VBEngine(M, r, cols=c, m_global=m) for c in cuts]
    for p, (b, e) in zip(parts, cuts):
        p.attach_comm(comm)
        p.set_state(wh["lw"], wh["lh"][:, b:e], wh["eh"][:, b:e])
    comm.state_finish()
    return comm, parts, cuts


def test_local_group_rows_against_50_digit_updates():
    """A local group of two partitions: k_control with the all-reduced tail handed in."""
    import ccfindr_amd as C
    X = _matrix()
    wh = _state(X, 2)
    M = C.CountMatrix(X)
    comm, parts, cuts = _group(M, 2, X.shape[1], wh)
    checked = 0
    for start in STARTS:
        for flags in FLAGS:
            for p, (b, e) in zip(parts, cuts):
                p.set_state(wh["lw"], wh["lh"][:, b:e], wh["eh"][:, b:e])
            comm.state_finish()
            got = _raw_run(comm._lib.vbnmf_group_run, comm._h, start, 8, flags)
            assert got["it"] == 8 and got["reason"] == 4, (start, flags, got["reason"])
            h = got["history"]
            checked += check_rows(h[:, 1:5], h[:, 5:9], start, flags, got["reason"], 3, "group_run")
    for p in parts:
        p.close()
    comm.close()
    assert checked >= 110


def _project(X, c, ah, bh, flags, **kw):
    import importlib
    import ccfindr_amd as C
    P = importlib.import_module("ccfindr_amd.project")
    M = C.CountMatrix(X)
    try:
        out = P.vb_project_coupled_columns(M, c["lw"], c["ew"], c["lh0"], ah, bh, 0, X.shape[1], flags, **kw)
    finally:
        M.close()
    return {"hyper": out[6], "steps": out[7], "why": out[8], "history": out[10]}


def test_coupled_projection_rows_against_50_digit_updates():
    """The coupled vb_project: k_vbp_control, lane 0's side switched off (flags 0, 0, fa, fb; aw = bw = 1 unused)."""
    import util_vb_project_coupled as UC
    c = UC.case(1, 0.6, 3.0)
    checked = 0
    for start in STARTS:
        for fa, fb in sorted({(f[2], f[3]) for f in FLAGS}):   # what the five flag sets leave of the H side
            flags = (0, 0, fa, fb)
            got = _project(c["x"], c, start[2], start[3], (fa, fb), n0=0, dn=1, Itmax=8, Tol=0.0, history_rows=8)
            h = got["history"]
            assert got["steps"] == 8 and got["why"] == 4 and h.shape == (8, 5), (start, flags, got["why"])
            it = len(h)
            stats = np.column_stack([np.zeros(it), h[:, 1], np.ones(it), h[:, 2]])
            hyper = np.column_stack([np.ones(it), np.ones(it), h[:, 3], h[:, 4]])
            if fa + fb == 0:                                   # no update at all: (ah, bh) stay what they were
                assert np.all(h[:, 3] == start[2]) and np.all(h[:, 4] == start[3])
            checked += check_rows(stats, hyper, (1.0, 1.0, start[2], start[3]), (0, 0, fa, fb), got["why"], 5, "vb_project")
            assert got["hyper"] == tuple(h[-1, 3:5])
    assert checked >= 90


# ---- a failed update inside a loop leaves the hyper-parameters as they were --------------------------------------------
def _last_rows_equal(h, start):
    prev = np.array(start, dtype=np.float64) if len(h) == 1 else h[-2, 5:9]
    return np.array_equal(h[-1, 5:9].view(np.uint64), np.ascontiguousarray(prev).view(np.uint64))


def test_failed_update_inside_a_loop_leaves_the_row_unchanged():
    """fudge = 0 from shapes of 1e-4, as tests/test_gpu_device_loop.py's degenerate run, made certain: five genes start with
    1e-12 of their second component, so alw = 1e-4 + O(1e-12) there, exp(psi(alw)) underflows to 0, mean(log lw) is -inf at
    the first step and the first Newton step is not finite.  With n0 = 0 the loop ends at step 1 with reason 3 -- 5 for the
    projection, whose all-zero cell does the same -- and that row's hyper-parameters are those before it (the start),
    bit for bit; so are the ones handed back.  (A failure behind earlier rows is held to the row before by check_rows.)"""
    import ccfindr_amd as C
    import util_vb_project_coupled as UC
    X = _matrix()
    M = C.CountMatrix(X)
    start = (1e-4, 1.0, 1e-4, 1.0)

    def state(seed):
        wh = _state(X, 2, seed=seed)
        wh["lw"] = wh["lw"].copy()
        wh["lw"][:5, 1] *= 1e-12
        return wh

    def check(got, n0, where):
        h = got["history"]
        assert got["reason"] == 3 and got["it"] == n0 + 1 and len(h) == n0 + 1, (where, n0, got["reason"], got["it"])
        assert h[-1, 1] == -np.inf, (where, n0, h[-1])
        assert _last_rows_equal(h, start), (where, n0, h[:, 5:9])
        assert tuple(h[-1, 5:9]) == start == tuple(got["hyper"]), (where, n0)

    wh = state(2)
    for n0 in (0,):                                            # (later the step's NaN evidence would end the loop first)
        eng = C.VBEngine(M, 2)
        eng.set_state(wh["lw"], wh["lh"], wh["eh"])
        check(_raw_run(eng._lib.vbnmf_engine_run, eng._h, start, 12, (1, 1, 1, 1), fudge=0.0, Tol=1e-5, n0=n0), n0, "engine_run")
        eng.close()
        engs = [C.VBEngine(M, 2, grid=C.batch_grid(4)) for _ in range(4)]
        for b, e in enumerate(engs):
            s = state(10 + b)
            e.set_state(s["lw"], s["lh"], s["eh"])
        res = C.run_batch(engs, [dict(zip(KEYS, start))] * 4, Itmax=12, Tol=1e-5, n0=n0, dn=1, fudge=0.0, history=True)
        for b, r_ in enumerate(res):
            r_["hyper"] = tuple(r_["hyper"][k] for k in KEYS)
            check(r_, n0, "run_batch[%d]" % b)
        for e in engs:
            e.close()
        comm, parts, _ = _group(M, 2, X.shape[1], wh)
        check(_raw_run(comm._lib.vbnmf_group_run, comm._h, start, 12, (1, 1, 1, 1), fudge=0.0, Tol=1e-5, n0=n0), n0, "group_run")
        for p in parts:
            p.close()
        comm.close()
    c = UC.case(1, 0.6, 3.0)
    Xp = c["x"].copy(order="F")
    Xp[:, 6] = 0.0                                             # an all-zero cell: its lh underflows to 0 under fudge = 0
    for n0 in (0,):
        got = _project(Xp, c, 1e-4, 1.0, (True, True), n0=n0, fudge=0.0, Itmax=12, history_rows=12)
        h = got["history"]
        assert got["why"] == 5 and got["steps"] == n0 + 1 and h[-1, 1] == -np.inf, (n0, got["why"], got["steps"])
        prev = (1e-4, 1.0) if len(h) == 1 else tuple(h[-2, 3:5])
        assert tuple(h[-1, 3:5]) == prev == got["hyper"] == (1e-4, 1.0)


# ---- rejection at the ABI: before any launch, and the engine stays usable -----------------------------------------------
def test_bad_hyper_parameters_are_refused_and_the_engine_stays_usable():
    import ccfindr_amd as C
    X = _matrix()
    M = C.CountMatrix(X)
    wh = _state(X, 2)
    hy = dict(zip(KEYS, (1.2, 0.9, 0.8, 1.5)))
    kw = dict(Itmax=6, Tol=0.0, n0=0, dn=1, history=True)
    fresh = C.VBEngine(M, 2)
    fresh.set_state(wh["lw"], wh["lh"], wh["eh"])
    want = fresh.run(hy, **kw)
    fresh.close()
    eng = C.VBEngine(M, 2)
    eng.set_state(wh["lw"], wh["lh"], wh["eh"])
    comm, parts, _ = _group(M, 2, X.shape[1], wh)
    for key in KEYS:
        for bad in (0.0, -1.0, np.nan, np.inf):
            h = dict(hy)
            h[key] = bad
            with pytest.raises(C.VBNMFError) as ei:
                eng.run(h, **kw)
            assert ei.value.code == 1, (key, bad)
            with pytest.raises(C.VBNMFError) as ei:
                C.run_batch([eng], [h], **kw)
            assert ei.value.code == 1, (key, bad)
            with pytest.raises(C.VBNMFError) as ei:
                comm.run(h, **kw)
            assert ei.value.code == 1, (key, bad)
    got = eng.run(hy, **kw)                                    # nothing was launched, nothing moved
    assert got["it"] == want["it"] and got["reason"] == want["reason"] and got["hyper"] == want["hyper"]
    assert np.array_equal(got["history"], want["history"])
    for p in parts + [eng]:
        p.close()
    comm.close()
