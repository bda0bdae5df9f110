"""The t-SNE restatement of tests/util_tsne.py against its 50-digit forms, the committed seeds, the argument checks of
vbnmf_tsne_create (before a device is looked for) and visualize_clusters' bookkeeping with an injected embedding.  No GPU."""
import ctypes
import math
from types import SimpleNamespace

import mpmath as mp
import numpy as np
import pytest

import util_tsne as T

import ccfindr_amd as C
from ccfindr_amd import _native as N
from ccfindr_amd import embed as E
from ccfindr_amd.post import cluster_id


def _info():
    return E.tsne_info()


def _all_cases():
    info = _info()
    shapes, big = T.shape_cases(info["i_block"], info["j_tile"], info["lds_row_capacity"])
    cases = [("shape", T.shape_kw(c)) for c in shapes] + [(k, v) for k, v in T.SPECIAL.items()]
    return cases, big


def _aff(kw):
    kw = dict(kw)
    key = (kw.pop("n"), kw.pop("d"))
    return T.case(*key, **kw), T.case_affinities(*key, **kw)


def test_info_without_a_device():
    info = _info()
    assert info["wave_width"] == 64 and info["workgroup_size"] % 64 == 0
    assert info["i_block"] >= 1 and info["j_tile"] >= 1 and info["lds_row_capacity"] >= 64


def test_restatement_rows_sum_to_one_and_meet_the_entropy():
    cases, _ = _all_cases()
    for name, kw in cases:
        c, a = _aff(kw)
        D, beta, S = a["D"], a["beta"], a["S"]
        p = np.exp(-beta[:, None] * D) / S[:, None]
        np.fill_diagonal(p, 0.0)
        # S_i carries the DBL_MIN of its definition: the row sums to 1 - DBL_MIN / S_i, which is 1 unless the row sits at
        # the edge of exp's underflow (the outlier's)
        assert np.allclose(p.sum(axis=1), 1.0 - T.DBL_MIN / S, rtol=0, atol=1e-13), name
        H = beta * (D * p).sum(axis=1) + np.log(S)                     # H_i as the bisection forms it
        done = a["trips"] < T.MAX_TRIPS
        assert np.all(np.abs(H[done] - math.log(c["u"])) < T.TOL + 1e-12), name


def test_special_inputs_do_what_they_are_for():
    _, a = _aff(T.SPECIAL["identical"])
    assert np.all(a["trips"] == T.MAX_TRIPS) and np.all(a["beta"] == 2.0 ** 200)
    c, a = _aff(T.SPECIAL["outlier"])
    assert a["beta"][c["n"] // 2] < 1e-3                     # its exponentials underflow at beta = 1, beta halves
    _, up = _aff(T.SPECIAL["scaled_up"])
    _, dn = _aff(T.SPECIAL["scaled_down"])
    assert up["beta"].max() < 1e-2 and dn["beta"].min() > 1e2


def test_committed_seeds_flag_no_row():
    cases, big = _all_cases()
    full = T.full_lds_row(_info()["lds_row_capacity"])
    for name, kw in cases + [("lds_row + 1", dict(n=big[0], d=big[1])), ("lds_row", T.shape_kw(full))]:
        _, a = _aff(kw)
        assert not a["flagged"].any(), (name, kw)


def test_restatement_affinity_row_against_50_digits():
    for kw in (dict(n=65, d=10), dict(n=33, d=10), T.SPECIAL["outlier"], T.SPECIAL["scaled_down"]):
        c, a = _aff(kw)
        for i in (0, c["n"] // 2, c["n"] - 1):
            S, H, delta, bound = T.mp_row(c["Xn"], i, a["beta"][i], c["u"])
            assert bound <= T.CAP * S
            assert abs(mp.mpf(float(a["S"][i])) - S) <= bound, (kw, i)
            if a["trips"][i] < T.MAX_TRIPS:
                assert abs(delta) < T.TOL + T.FLAG


def test_restatement_forces_against_50_digits():
    c, a = _aff(dict(n=65, d=10))
    P = T.joint_p(a["D"], a["beta"], a["S"])
    for Y, e in ((T.start(65, 3), 12.0), (T.spread_Y(65, 4), 1.0)):
        f = T.forces(P, Y, e)
        b = T.force_bounds(a["D"], 10, a["beta"], a["S"], Y, e)
        Z = T.mp_Z(Y)
        for key in ("A", "R", "z", "cost"):
            assert np.all(b[key] <= T.CAP * b["abs_" + key] + 1e-300), key
        for i in (0, 32, 64):
            ref = T.mp_point(c["Xn"], a["beta"], a["S"], Y, i, e, Z)
            for col in range(2):
                assert abs(mp.mpf(float(f["A"][i, col])) - ref["A"][col]) <= b["A"][i, col]
                assert abs(mp.mpf(float(f["R"][i, col])) - ref["R"][col]) <= b["R"][i, col]
            assert abs(mp.mpf(float(f["z"][i])) - ref["z"]) <= b["z"][i]
            assert abs(mp.mpf(float(f["cost_i"][i])) - ref["cost"]) <= b["cost"][i]


@pytest.mark.parametrize("n,d,iters", [(65, 10, 10), (1030, 2, 3)])         # the cases of tests/test_gpu_tsne.py::test_step_by_step
def test_step_seeds_have_no_element_inside_its_own_bound(n, d, iters):
    c, a = _aff(dict(n=n, d=d))
    P = T.joint_p(a["D"], a["beta"], a["S"])
    sch = dict(stop_lying_iter=3, mom_switch_iter=3)
    Y, uY, g = T.start(n, 5), np.zeros((n, 2)), np.ones((n, 2))
    for it in range(1, iters + 1):
        e, m = T.schedule(it, **sch)
        f = T.forces(P, Y, e)
        ub = T.update_bounds(Y, uY, g, f["A"], f["R"], f["z"], m)
        assert not np.any(np.abs(ub["dY"]) <= ub["bdY"]), it
        Y, uY, g, _ = T.update(Y, uY, g, f["A"], f["R"], f["z"], m)
        assert np.all(np.abs(Y.mean(axis=0)) <= n * T.U * np.abs(Y).max())


def test_schedule_switches_after_the_named_iterations():
    assert T.schedule(3, stop_lying_iter=3, mom_switch_iter=3) == (12.0, 0.5)
    assert T.schedule(4, stop_lying_iter=3, mom_switch_iter=3) == (1.0, 0.8)


def test_end_to_end_margin_is_derived_from_the_recorded_spread():
    assert len(T.E2E_FINAL) == 5 and T.E2E_NN_SAME == T.E2E["n"]
    assert 0.02 < max(T.E2E_FINAL) - min(T.E2E_FINAL) < 0.03


# ---- the library's argument checks: all of them before a device is looked for ------------------------------------------------
def _create(n, d, x, u, normalize=1, handle=True):
    h = ctypes.c_void_p()
    rc = N.load().vbnmf_tsne_create(0, n, d, N.dptr(x) if x is not None else None, u, normalize, ctypes.byref(h) if handle else None)
    if rc == 0:
        N.load().vbnmf_tsne_destroy(h)
    return rc


def test_bad_arguments_arrive_before_no_device():
    x = np.ascontiguousarray(T.case(65, 10)["X"])
    bad = x.copy()
    bad[7, 3] = np.nan
    inf = x.copy()
    inf[0, 0] = np.inf
    assert _create(65, 10, None, 20.0) == N.ERR_BAD_ARG
    assert _create(65, 10, x, 20.0, handle=False) == N.ERR_BAD_ARG
    assert _create(0, 10, x, 20.0) == N.ERR_BAD_ARG
    assert _create(2 ** 31, 10, x, 20.0) == N.ERR_BAD_ARG
    assert _create(65, 0, x, 20.0) == N.ERR_BAD_ARG
    assert _create(65, N.MAX_RANK + 1, x, 20.0) == N.ERR_BAD_ARG
    assert _create(65, 10, x, 0.5) == N.ERR_BAD_ARG
    assert _create(65, 10, x, float("nan")) == N.ERR_BAD_ARG
    assert _create(64, 10, x, 21.0) == N.ERR_BAD_ARG                  # 3 u = n - 1: not below
    assert _create(4, 10, x, 1.0) == N.ERR_BAD_ARG                    # n = 5 is the smallest the rule allows
    assert _create(65, 10, bad, 20.0) == N.ERR_BAD_ARG
    assert _create(65, 10, inf, 20.0) == N.ERR_BAD_ARG
    L = N.load()
    one, cnt = np.zeros(4), ctypes.c_int32(0)
    assert L.vbnmf_tsne_set_state(None, N.dptr(one), None, None) == N.ERR_BAD_ARG
    assert L.vbnmf_tsne_get_state(None, N.dptr(one), None, None) == N.ERR_BAD_ARG
    assert L.vbnmf_tsne_forces(None, 1.0, None, None, None, None) == N.ERR_BAD_ARG
    assert L.vbnmf_tsne_affinity(None, None, None, None) == N.ERR_BAD_ARG
    assert L.vbnmf_tsne_run(None, 1, 1, 12.0, 250, 250, 0.5, 0.8, 200.0, 0.01, 50, N.dptr(one), np.zeros(4, dtype=np.int32).ctypes.data_as(N.c_int32_p),
                            ctypes.byref(cnt)) == N.ERR_BAD_ARG
    if L.vbnmf_device_count() > 0:
        return
    assert _create(65, 10, x, 20.0) == N.ERR_NO_DEVICE
    with pytest.raises(C.VBNMFError) as ei:
        C.TSNE(x, perplexity=20.0)
    assert ei.value.code == N.ERR_NO_DEVICE and "no CPU fallback" in str(ei.value)


# ---- visualize_clusters' bookkeeping (R/utils.R:692-712) with an injected embedding -----------------------------------------
def _fake(h_list, ranks):
    return SimpleNamespace(ranks=list(ranks), coeff=list(h_list))


def test_visualize_clusters_rank_cid_counts():
    rng = np.random.default_rng(0)
    h3, h5 = rng.uniform(size=(3, 40)), rng.uniform(size=(5, 40))
    h5[3] = 0.0                                                      # cluster 4 never occurs
    seen = {}

    def embed(x, **kw):
        seen["x"], seen["kw"] = x, kw
        return SimpleNamespace(Y=x[:, :2].copy())

    res = _fake([h3, h5], [3, 5])
    m = C.visualize_clusters(res, embed=embed, perplexity=7)
    assert m.rank == 3 and seen["kw"] == {"perplexity": 7}           # :695-698 the first rank
    assert np.array_equal(seen["x"], h3.T) and m.Y.shape == (40, 2)  # :700 t(h)
    assert np.array_equal(m.cid, np.argmax(h3, axis=0) + 1) and m.names == ["1", "2", "3"]
    m = C.visualize_clusters(res, rank=5, embed=embed)
    cid = np.argmax(h5, axis=0) + 1
    assert np.array_equal(m.cid, cid) and np.array_equal(m.cid, cluster_id(res, 5))
    assert list(m.counts) == sorted(set(cid.tolist())) and 4 not in m.counts
    assert all(m.counts[k] == int((cid == k).sum()) for k in m.counts) and sum(m.counts.values()) == 40
    with pytest.raises(IndexError, match="subscript out of bounds"):
        C.visualize_clusters(res, rank=4, embed=embed)


def test_visualize_clusters_accepts_the_four_result_types():
    h = np.random.default_rng(1).uniform(size=(2, 12))
    for cls in (C.VBResult, C.MLResult, C.Projection, C.VBProjection):
        r = cls()
        r.ranks, r.coeff = [2], [h]
        m = C.visualize_clusters(r, embed=lambda x, **kw: SimpleNamespace(Y=np.zeros((len(x), 2))))
        assert m.rank == 2 and sum(m.counts.values()) == 12


def test_tsne_rejects_unknown_schedule_names():
    with pytest.raises(TypeError):
        C.tsne(np.zeros((10, 2)), thetaa=0.5)
