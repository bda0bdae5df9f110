"""The neighbour-limited t-SNE restatement of tests/util_tsne_knn.py against its 50-digit forms, the committed cases and
constants, and the argument checks of vbnmf_tsne_create_knn and vbnmf_knn (before a device is looked for).  No GPU."""
import ctypes
import inspect

import mpmath as mp
import numpy as np
import pytest

import util_tsne as T
import util_tsne_knn as TK

import ccfindr_amd as C
from ccfindr_amd import _native as N
from ccfindr_amd import embed as E


def _cases():
    info = E.tsne_info()
    return TK.handle_cases(info["i_block"], info["j_tile"], info["lds_row_capacity"])


def test_info_without_a_device():
    info = E.tsne_knn_info()
    assert info["neighbor_limit"] >= 1024 and info["workgroup_size"] % 64 == 0 and info["lds_row_capacity"] >= 64
    assert info["repulse_tile"] % 4 == 0 and info["repulse_i_block"] == 64 and info["attract_rows"] >= 1
    assert info["neighbors"] == 0 and info["nnz"] == 0 and info["longest_row"] == 0
    assert info["lds_row_capacity"] == E.tsne_info()["lds_row_capacity"]


def test_lists_are_the_k_smallest_in_distance_then_index_order():
    X = TK.lattice()
    D = T.sq_dist(X)
    for K in TK.LATTICE_K:
        idx, dist = TK.knn_lists(D, K)
        for i in (0, 4, 40, 80):
            pairs = sorted((D[i, j], j) for j in range(len(X)) if j != i)[:K]
            assert [j for _, j in pairs] == idx[i].tolist() and [v for v, _ in pairs] == dist[i].tolist()
        assert all(i not in idx[i] for i in range(len(X)))
    # the ties are there: at K = 5 and K = 9 the centre point's K-th and (K + 1)-th distance are equal
    row = np.sort(np.delete(D[40], 40))
    assert row[4] == row[5] and row[8] == row[9]


def test_committed_cases_flag_no_row():
    for name, key, kw, K in _cases():
        L = TK.case_lists(key, K, kw)
        assert not L["flagged"].any(), (name, K)
        assert 1 <= L["trips"].min() and (name == "identical" or L["trips"].max() < T.MAX_TRIPS), name
    h = TK.hub_case()
    assert not h["flagged"].any() and h["trips"].max() < T.MAX_TRIPS
    for n in (65, 257):                                    # the dense handles the K = n - 1 lists are compared with
        assert not T.case_affinities(n, 10)["flagged"].any()
    X = TK.lattice()
    D = T.sq_dist(X)
    for K in TK.LATTICE_K:
        _, dist = TK.knn_lists(D, K)
        assert not TK.affinities(dist, float(K - 1))[3].any(), K


def test_identical_points():
    L = TK.case_lists((65, 2), 63, (("kind", "identical"),))
    want = np.array([[j for j in range(65) if j != i][:63] for i in range(65)])
    assert np.array_equal(L["idx"], want) and np.all(L["dist"] == 0.0)
    assert np.all(L["trips"] == T.MAX_TRIPS) and np.all(L["beta"] == 2.0 ** 200) and np.all(L["S"] == 63.0)


def test_restatement_affinity_row_against_50_digits():
    for name, key, kw, K in _cases():
        if name not in ("n65-d128", "n257-d33", "outlier", "scaled_down", "n1030-K257", "n1030-K1024"):
            continue
        c = T.case(*key, **dict(kw))
        L = TK.case_lists(key, K, kw)
        for i in (0, c["n"] // 2, c["n"] - 1):
            S, H, delta, bound = TK.mp_row(c["Xn"], i, L["idx"][i], L["beta"][i], c["u"])
            assert bound <= T.CAP * S, (name, i)
            assert abs(mp.mpf(float(L["S"][i])) - S) <= bound, (name, i)
            assert abs(delta) < T.TOL + T.FLAG


def _sparse(L):
    return TK.sparse_p(L["idx"], TK.cond_p(L["dist"], L["beta"], L["S"]))


def test_restatement_sparse_p():
    for name, key, kw, K in _cases():
        L = TK.case_lists(key, K, kw)
        n = len(L["idx"])
        indptr, indices, values = _sparse(L)
        rows = np.diff(indptr)
        assert rows.min() >= K and rows.max() <= n - 1, name
        P = TK.dense(indptr, indices, values)
        assert np.array_equal(P, P.T), name
        M = TK.masks(L["idx"])
        assert np.array_equal(np.repeat(np.arange(n), rows) * n + indices, np.flatnonzero((M | M.T).ravel())), name
    h = TK.hub_case()
    rows = np.diff(_sparse(h)[0])
    assert rows[0] == h["n"] - 1 and rows[1:].max() <= 8 and rows.min() >= 2
    # the largest row is far from K: nothing may size a buffer by K
    L = TK.case_lists((2049, 10), 90)
    assert np.diff(_sparse(L)[0]).max() > 3 * 90


def test_restatement_forces_against_50_digits():
    for key, K in (((65, 10), 63), ((129, 20), 90)):
        c = T.case(*key)
        L = TK.case_lists(key, K)
        n, d = key
        P = TK.dense(*_sparse(L))
        for Y, e in ((T.start(n, 3), 12.0), (T.spread_Y(n, 4), 1.0)):
            f = TK.forces(P, Y, e)
            b = TK.force_bounds(L["D"], d, L["beta"], L["S"], L["idx"], Y, e)
            Z = T.mp_Z(Y)
            for k in ("A", "R", "z", "cost"):
                assert np.all(b[k] <= T.CAP * b["abs_" + k] + 1e-300), k
            assert np.all(np.abs(b["P"] - P) <= TK.p_bounds(L["D"], d, L["beta"], L["S"], L["idx"])[1])
            for i in (0, n // 2, n - 1):
                ref = TK.mp_point(c["Xn"], L["beta"], L["S"], L["idx"], Y, i, e, Z)
                for col in range(2):
                    assert abs(mp.mpf(float(f["A"][i, col])) - ref["A"][col]) <= b["A"][i, col]
                    assert abs(mp.mpf(float(f["R"][i, col])) - ref["R"][col]) <= b["R"][i, col]
                assert abs(mp.mpf(float(f["z"][i])) - ref["z"]) <= b["z"][i]
                assert abs(mp.mpf(float(f["cost_i"][i])) - ref["cost"]) <= b["cost"][i]


def test_depths_stay_under_the_cap():
    info = E.tsne_knn_info()
    n = info["lds_row_capacity"] + 1
    assert (15 + TK.repulse_depth(n, info["repulse_tile"]) + 1) * T.U <= T.CAP
    assert (TK.attract_depth(n - 1) + 11) * T.U <= T.CAP and TK.k_aff(info["neighbor_limit"]) * T.U <= T.CAP


def test_end_to_end_constants():
    assert len(TK.E2E_FINAL) == 5 and TK.E2E_NN_SAME == T.E2E["n"] and TK.E2E_K == TK.auto_k(30.0)
    assert 0.015 < max(TK.E2E_FINAL) - min(TK.E2E_FINAL) < 0.025
    # the first 20 iterations of the committed run, recomputed: the constants belong to this restatement
    L = TK.case_lists((T.E2E["n"], T.E2E["d"], T.E2E["k"], T.E2E["seed"]), TK.E2E_K)
    P = TK.dense(*_sparse(L))
    assert abs(P.sum() - 1.0) < 1e-12
    _, _, _, costs = TK.run(P, T.start(T.E2E["n"], 0), 20, cost_every=0)
    assert costs[-1][0] == 20 and np.isfinite(costs[-1][1]) and costs[-1][1] > max(TK.E2E_FINAL)


# ---- the library's argument checks: all of them before a device is looked for ------------------------------------------------
def _create(n, d, x, u, K, normalize=1):
    h = ctypes.c_void_p()
    rc = N.load().vbnmf_tsne_create_knn(0, n, d, N.dptr(x), u, normalize, K, ctypes.byref(h))
    if rc == 0:
        N.load().vbnmf_tsne_destroy(h)
    return rc


def _knn(x, k):
    n, d = x.shape
    idx, dist = np.zeros((n, max(k, 1)), dtype=np.int32), np.zeros((n, max(k, 1)))
    return N.load().vbnmf_knn(0, n, d, N.dptr(x), k, idx.ctypes.data_as(N.c_int32_p), N.dptr(dist))


def test_bad_arguments_arrive_before_no_device():
    limit = E.tsne_knn_info()["neighbor_limit"]
    x = np.ascontiguousarray(T.case(65, 10)["X"])
    big = np.ascontiguousarray(T.case(limit + 6, 3)["X"])
    bad = x.copy()
    bad[7, 3] = np.nan
    assert _create(65, 10, x, 20.0, -1) == N.ERR_BAD_ARG
    assert _create(65, 10, x, 20.0, 65) == N.ERR_BAD_ARG                  # K = n
    assert _create(65, 10, x, 20.0, 20) == N.ERR_BAD_ARG                  # K = perplexity
    assert _create(65, 10, x, 20.0, 19) == N.ERR_BAD_ARG                  # K < perplexity
    assert _create(64, 10, x, 21.0, 0) == N.ERR_BAD_ARG                   # today's rule: 3 u = n - 1 is not below
    assert _create(65, 10, bad, 20.0, 0) == N.ERR_BAD_ARG
    assert _create(limit + 6, 3, big, 30.0, limit + 1) == N.ERR_BAD_ARG   # above the limit, below n
    assert _create(3 * limit, 3, np.zeros((3 * limit, 3)), (limit + 3) / 3.0, 0) == N.ERR_BAD_ARG      # "auto" above the limit
    assert _knn(x, 0) == N.ERR_BAD_ARG and _knn(x, 65) == N.ERR_BAD_ARG and _knn(x, -3) == N.ERR_BAD_ARG
    assert _knn(big, limit + 1) == N.ERR_BAD_ARG and _knn(bad, 5) == N.ERR_BAD_ARG
    assert _knn(x[:1], 1) == N.ERR_BAD_ARG
    L = N.load()
    assert L.vbnmf_tsne_neighbors(None, None, None) == N.ERR_BAD_ARG
    assert L.vbnmf_tsne_sparse_p(None, None, None, None, None) == N.ERR_BAD_ARG
    for call in (lambda: C.knn(x, 0), lambda: C.knn(x, 65), lambda: C.TSNE(x, perplexity=20.0, neighbors=65),
                 lambda: C.TSNE(x, perplexity=20.0, neighbors=20), lambda: C.TSNE(x, perplexity=20.0, neighbors=0),
                 lambda: C.TSNE(big, perplexity=30.0, neighbors=limit + 1), lambda: C.tsne(x, perplexity=20.0, neighbors=12)):
        with pytest.raises(C.VBNMFError) as ei:
            call()
        assert ei.value.code == N.ERR_BAD_ARG
    for wrong in (2.5, "nearest", True, [5]):
        with pytest.raises(TypeError):
            C.TSNE(x, perplexity=20.0, neighbors=wrong)
    with pytest.raises(TypeError):
        C.knn(x, 2.0)
    if L.vbnmf_device_count() > 0:
        return
    assert _create(65, 10, x, 20.0, 0) == N.ERR_NO_DEVICE and _create(65, 10, x, 20.0, 64) == N.ERR_NO_DEVICE
    assert _knn(x, 1) == N.ERR_NO_DEVICE and _knn(x, 64) == N.ERR_NO_DEVICE
    with pytest.raises(C.VBNMFError) as ei:
        C.TSNE(x, perplexity=20.0, neighbors="auto")
    assert ei.value.code == N.ERR_NO_DEVICE and "no CPU fallback" in str(ei.value)


def test_tsne_takes_neighbors():
    """tsne(x, neighbors=...) is an argument of the map, not an unknown schedule name (a TypeError before this path existed):
    it reaches the library, which runs it or says that there is no device."""
    assert "neighbors" in inspect.signature(C.tsne).parameters and "neighbors" in inspect.signature(C.TSNE).parameters
    assert inspect.signature(C.tsne).parameters["neighbors"].default is None
    x = T.case(65, 10)["X"]
    try:
        emb = C.tsne(x, perplexity=20.0, neighbors="auto", max_iter=2)
    except C.VBNMFError as err:
        assert err.code == N.ERR_NO_DEVICE and C.load().vbnmf_device_count() == 0
    else:
        assert emb.neighbors == 60 and emb.Y.shape == (65, 2)
    assert C.Embedding(Y=None, itercosts=None, cost_iters=None, costs=None, beta=None, trips=None).neighbors is None
