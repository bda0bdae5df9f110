"""The coupled VB projection (ccfindr_amd.vb_project with hyper_update= / stop="global", vbnmf_matrix_vb_project_coupled), the
parts that need no GPU: the numpy restatement the GPU tests compare against (tests/util_vb_project_coupled.py) is tied to the
committed oracle's ``hyper_update`` and ``vb_iterate``; the conditions under which the GPU tests may ask for equal step counts
are asserted; the argument checks of the public entry.
"""
import functools

import numpy as np
import pytest

import util_vb_project as U
import util_vb_project_coupled as UC


@functools.lru_cache(maxsize=None)
def run(seed, ab, start, flags):
    c = UC.case(seed, *ab)
    return c, UC.project_coupled(c["x"], c["lw"], c["ew"], c["lh0"], *start, flags=flags, Tol=1e-5)


ALL = [(seed, ab, start, flags) for seed, ab, start in UC.CONDITIONS for flags in UC.FLAGS]


def test_hyper_update_equals_the_oracles_to_the_last_bit():
    """``hyper_update_h`` against ``oracle.vbnmf_oracle.hyper_update`` with flags (F, F, fa, fb) on the statistics of real
    states (three steps into each case) and from several (ah, bh): the same bits, and (T, F) sets bh as (T, T) does."""
    from oracle import vbnmf_oracle as O
    checked = 0
    for seed, ab, start in UC.CONDITIONS:
        c = UC.case(seed, *ab)
        w = UC.project_coupled(c["x"], c["lw"], c["ew"], c["lh0"], *start, Itmax=3, Tol=0.0)
        wh = {"lw": c["lw"], "ew": c["ew"], "lh": w["lh"], "eh": w["eh"]}
        lhm, ehm = float(np.mean(np.log(w["lh"]))), float(np.mean(w["eh"]))
        for ah, bh in (start, (1.0, 1.0), (0.05, 7.0), (12.0, 0.2)):
            for fa, fb in ((True, True), (False, True), (True, False), (False, False)):
                want = O.hyper_update((False, False, fa, fb), wh, {"aw": 1.3, "bw": 0.7, "ah": ah, "bh": bh}, Niter=100, Tol=1e-3)
                ah1, bh1, failed, dfs = UC.hyper_update_h(fa, fb, lhm, ehm, ah, bh)
                assert not failed
                assert (ah1, bh1) == (want["ah"], want["bh"]), (seed, ab, ah, bh, fa, fb)
                assert (want["aw"], want["bw"]) == (1.3, 0.7)
                assert bool(dfs) == fa
                if fa or fb:
                    assert bh1 == ehm
                if not fa:
                    assert ah1 == ah
                checked += 1
    assert checked == 64


def test_a_non_finite_statistic_fails_the_update():
    """mean(log lh) = -inf (an lh of 0 under fudge = 0): the Newton step is not finite -- the bounded failure, reason 5."""
    ah1, bh1, failed, dfs = UC.hyper_update_h(True, True, -np.inf, 0.4, 1e-4, 1.0)
    assert failed and (ah1, bh1) == (1e-4, 1.0) and dfs == []
    ah1, bh1, failed, dfs = UC.hyper_update_h(False, True, -np.inf, 0.4, 1e-4, 1.0)
    assert not failed and (ah1, bh1) == (1e-4, 0.4)


@pytest.mark.parametrize("seed,ab,start,flags", ALL, ids=[f"seed{s}-a{ab[0]}-{'TT' if f[0] else 'FT'}" for s, ab, st, f in ALL])
def test_the_loop_equals_vb_iterate_where_the_dropped_clause_does_not_bite(seed, ab, start, flags):
    """``project_coupled`` against ``oracle.vbnmf_oracle.vb_iterate`` driven with an update that does the H half only: the
    same ``it`` and the same hyper-parameters, bit for bit, wherever E >= lk0 at the restatement's stop (the oracle keeps the
    reference's ``lkh >= lk0`` clause and goes on otherwise: then it must still be running one step later)."""
    from oracle import vbnmf_oracle as O
    c, w = run(seed, ab, start, flags)
    x, lw, ew = c["x"], c["lw"], c["ew"]
    cew = ew.sum(axis=0)

    def update(wh, hyper, fudge):
        lh, eh, dh, alh = U.h_half(x, lw, cew, wh["lh"], hyper["ah"], hyper["bh"], fudge)
        ev = U.cell_evidence(x, lw, cew, lh, eh, alh, hyper["ah"], hyper["bh"])
        return {"lw": lw, "ew": ew, "lh": lh, "eh": eh, "dh": dh, "lkh": float(ev.sum())}

    bites = not (w["E"] >= w["lk0"])
    wh, hyper, lk0, it, trace = O.vb_iterate(update, {"lw": lw, "ew": ew, "lh": c["lh0"], "eh": None},
                                             {"aw": 1.0, "bw": 1.0, "ah": start[0], "bh": start[1]},
                                             Itmax=w["it"] + (1 if bites else 50), Tol=1e-5,
                                             hyper_flags=(False, False) + tuple(flags), n0=10, dn=1)
    print(f"seed {seed}, drawn with {ab}, from {start}, flags {flags}: it {w['it']}, E {w['E']!r}, lk0 {w['lk0']!r}, clause bites: {bites}")
    if bites:
        assert it == w["it"] + 1                             # the oracle went past the restatement's stop
        assert trace[w["it"] - 1][0] == w["E"]
        return
    assert it == w["it"]
    assert (hyper["ah"], hyper["bh"]) == w["hyper"]
    assert wh["lkh"] == w["E"] and lk0 == w["lk0"]
    assert np.array_equal(wh["lh"], w["lh"]) and np.array_equal(wh["eh"], w["eh"])
    assert [t[0] for t in trace] == w["history"][:, 0].tolist()


def test_the_clause_bites_in_two_of_the_eight_cases_only():
    assert sum(not (run(*k)[1]["E"] >= run(*k)[1]["lk0"]) for k in ALL) <= 2


@pytest.mark.parametrize("seed,ab,start,flags", ALL, ids=[f"seed{s}-a{ab[0]}-{'TT' if f[0] else 'FT'}" for s, ab, st, f in ALL])
def test_conditions_of_the_gpu_tests(seed, ab, start, flags):
    """What lets tests/test_gpu_vb_project_coupled.py ask for the restatement's ``it`` and ``reason``: every case stops with
    reason 1, no stopping decision closer to Tol than 1e-3 Tol, no Newton decision closer to 1e-3 than 1e-6 of it.  Seen:
    stop margins >= 3.0e-3, Newton margins >= 1.5e-2, 40 to 234 steps."""
    c, w = run(seed, ab, start, flags)
    print(f"seed {seed}, drawn with {ab}, from {start}, flags {flags}: it {w['it']}, hyper {w['hyper']}, stop margin "
          f"{w['stop_margin']:.3g}, Newton margin {w['newton_margin']:.3g}")
    assert w["reason"] == 1
    assert w["stop_margin"] > 1e-3
    assert w["newton_margin"] > 1e-6
    assert 20 <= w["it"] <= 400
    if not flags[0]:
        assert w["hyper"][0] == start[0]
    assert w["history"].shape == (w["it"], 5)
    assert np.array_equal(w["history"][:10, 3:], np.tile(start, (10, 1)))      # the n0 gate: nothing moves in steps 1..10
    assert tuple(w["history"][-1, 3:]) == w["hyper"]


def test_the_update_raises_the_total_evidence():
    """What it is for: on counts drawn with (0.6, 3) and projected from (1, 1), the re-estimated prior ends at a higher total
    evidence than the fixed one under the same rule, and near what the counts were drawn with."""
    for seed in (1, 2):
        c = UC.case(seed, 0.6, 3.0)
        fixed = UC.project_coupled(c["x"], c["lw"], c["ew"], c["lh0"], 1.0, 1.0, flags=(False, False), Tol=1e-5)
        _, both = run(seed, (0.6, 3.0), (1.0, 1.0), (True, True))
        assert fixed["reason"] == 1 and both["E"] > fixed["E"]
        assert 0.7 < both["hyper"][0] < 1.0 and 2.5 < both["hyper"][1] < 3.5


def test_api_errors_need_no_device():
    import ccfindr_amd as C
    c = UC.case(1, 0.6, 3.0)
    pair, hy = (c["ew"], c["sd"]), {"ah": 1.0, "bh": 1.0}
    for flags in ((True, False), (False, True), (True, True)):
        with pytest.raises(ValueError, match="couples the cells"):
            C.vb_project(c["x"], pair, hyper=hy, stop="cell", hyper_update=flags)
    with pytest.raises(ValueError, match='stop must be "cell" or "global"'):
        C.vb_project(c["x"], pair, hyper=hy, stop="all")
    for dn in (0, -3):
        with pytest.raises(ValueError, match="hyper_dn must be at least 1"):
            C.vb_project(c["x"], pair, hyper=hy, hyper_update=(True, True), hyper_dn=dn)
    with pytest.raises(ValueError, match="hyper_n0 must be at least 0"):
        C.vb_project(c["x"], pair, hyper=hy, hyper_update=(True, True), hyper_n0=-1)
    with pytest.raises(ValueError, match="hyper_update must be a pair"):
        C.vb_project(c["x"], pair, hyper=hy, hyper_update=True)
    import importlib
    P = importlib.import_module("ccfindr_amd.project")         # (the package attribute `project` is the function)
    assert P.REASONS[5] == "hyper-parameter update failed to converge" and set(P.REASONS) == {1, 3, 4, 5}
    v = C.VBProjection()
    assert np.isnan(v.evidence) and v.hyper0 == {} and v.history is None


def test_abi_argument_checks():
    """dn < 1, n0 < 0 and NULL hyper / flags are statuses of vbnmf_matrix_vb_project_coupled, found before a device is."""
    import ctypes
    import importlib
    import ccfindr_amd as C
    from ccfindr_amd import _native as N
    P = importlib.import_module("ccfindr_amd.project")
    c = UC.case(1, 0.6, 3.0)
    M = C.CountMatrix(c["x"])
    try:
        for kw in ({"dn": 0}, {"n0": -1}, {"Itmax": 0}):
            with pytest.raises(C.VBNMFError) as ei:
                P.vb_project_coupled_columns(M, c["lw"], c["ew"], c["lh0"], 1.0, 1.0, 0, 140, **kw)
            assert ei.value.code == N.ERR_BAD_ARG
        for ah, bh in ((0.0, 1.0), (1.0, -1.0), (float("nan"), 1.0)):
            with pytest.raises(C.VBNMFError) as ei:
                P.vb_project_coupled_columns(M, c["lw"], c["ew"], c["lh0"], ah, bh, 0, 140)
            assert ei.value.code == N.ERR_BAD_ARG
        lw, ew, lh = N.fcol(c["lw"]), N.fcol(c["ew"]), N.fcol(c["lh0"])
        rc = N.load().vbnmf_matrix_vb_project_coupled(M._h, 0, 140, 5, N.dptr(lw), N.dptr(ew), None, None, 10, 1, 0.0, N.dptr(lh), None,
                                                      None, 5, 1e-5, 0, None, None, None, None, None, None, None, 0)
        assert rc == N.ERR_BAD_ARG
    finally:
        M.close()
