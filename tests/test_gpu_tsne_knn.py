"""k_tsne_knn / k_tsne_attract / k_tsne_repulse (csrc/tsne_knn.h) behind ccfindr_amd.embed on the device, against the numpy
restatement and the 50-digit forms of tests/util_tsne_knn.py, where every bound is derived.  Sizes are aimed at the kernels'
edges, taken from vbnmf_tsne_info and vbnmf_tsne_knn_info.  The figures of the end-to-end test are in its docstring."""
import math
import os
import sys

import mpmath as mp
import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_tsne as T  # noqa: E402
import util_tsne_knn as TK  # noqa: E402

import ccfindr_amd as C  # noqa: E402
from ccfindr_amd import embed as E  # noqa: E402

pytestmark = pytest.mark.gpu

INFO, KINFO = E.tsne_info(), E.tsne_knn_info()
IB, JT, ROW = INFO["i_block"], INFO["j_tile"], INFO["lds_row_capacity"]
LIMIT, WG, TILE = KINFO["neighbor_limit"], KINFO["workgroup_size"], KINFO["repulse_tile"]
HANDLES = TK.handle_cases(IB, JT, ROW)
CASES = [pytest.param(c, id=c[0]) for c in HANDLES]
FORCE_CASES = CASES + [pytest.param("hub", id="hub")]


_f = T._f


def _case(c):
    """-> the inputs (util_tsne.case or the hub) and the restatement's lists and affinities, computed once per case."""
    if c == "hub":
        h = TK.hub_case()
        return h, h
    _, key, kw, K = c
    return T.case(*key, **dict(kw)), TK.case_lists(key, K, kw)


def _handle(c, L):
    return C.TSNE(c["X"], perplexity=c["u"], normalize=c["normalize"], neighbors=L["K"])


def _sample(n):
    """The first and last row and the rows at the edges of a wave, the attraction workgroup's rows and the repulsion's i-block."""
    rows = (0, 1, 3, 4, 63, 64, IB - 1, IB, n // 2, n - 2, n - 1) if n <= 1024 else (0, IB, n // 2, n - 1)     # (a row costs n 50-digit terms)
    return sorted({i for i in rows if 0 <= i < n})


def _same_lists(idx, dist, L):
    assert idx.dtype == np.int32 and idx.shape == L["idx"].shape
    assert np.array_equal(idx, L["idx"]), np.argwhere(idx != L["idx"])[:5]
    assert dist.tobytes() == np.ascontiguousarray(L["dist"]).tobytes()


# ---- 1. lists, exactly ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES)
def test_lists(c):
    case, L = _case(c)
    with _handle(case, L) as h:
        assert h.neighbors == L["K"]
        _same_lists(*h.knn(), L)
        info = h.knn_info()
    assert info["neighbors"] == L["K"] and info["attract_grid"] == -(-case["n"] // KINFO["attract_rows"])
    _same_lists(*C.knn(case["Xn"], L["K"]), L)
    if c[0] == "n%d-d10" % (ROW + 1):
        assert case["n"] == ROW + 1                                     # the row past the LDS capacity is among the cases


def test_lists_at_the_edges_of_k():
    c = T.case(*TK.EDGE_CASE)
    D = T.sq_dist(c["Xn"])
    ks = TK.k_edges(LIMIT, WG)
    assert {63, 64, 65, WG - 1, WG, WG + 1, LIMIT - 1, LIMIT} <= set(ks) and max(ks) == LIMIT
    for K in ks:
        idx, dist = TK.knn_lists(D, K)
        _same_lists(*C.knn(c["Xn"], K), {"idx": idx, "dist": dist})
    for n, d in ((5, 2), (65, 10)):
        X = T.case(n, d)["Xn"]
        D = T.sq_dist(X)
        for K in (1, n - 1):
            idx, dist = TK.knn_lists(D, K)
            _same_lists(*C.knn(X, K), {"idx": idx, "dist": dist})


def test_identical_points():
    c, L = _case([h for h in HANDLES if h[0] == "identical"][0])
    n, K = c["n"], L["K"]
    with _handle(c, L) as h:
        idx, dist = h.knn()
        assert np.array_equal(idx, [[j for j in range(n) if j != i][:K] for i in range(n)]) and np.all(dist == 0.0)
        assert np.all(h.trips == T.MAX_TRIPS) and np.all(h.beta == 2.0 ** 200) and np.all(h.sum_p == K)


@pytest.mark.parametrize("K", TK.LATTICE_K)
def test_lattice_ties_go_to_the_lower_index(K):
    X = TK.lattice()
    D = T.sq_dist(X)
    idx, dist = TK.knn_lists(D, K)
    assert np.all(dist == np.round(dist)) and (np.ptp(np.sort(np.delete(D[40], 40))[K - 1:K + 1]) == 0) == (K in (5, 9))
    _same_lists(*C.knn(X, K), {"idx": idx, "dist": dist})
    with C.TSNE(X, perplexity=float(K - 1), normalize=False, neighbors=K) as h:
        _same_lists(*h.knn(), {"idx": idx, "dist": dist})
        beta, S, trips, flagged = TK.affinities(dist, float(K - 1))
        assert not flagged.any() and np.array_equal(h.beta, beta) and np.array_equal(h.trips, trips)


# ---- 2. affinities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES + [pytest.param("hub", id="hub")])
def test_affinities(c):
    case, L = _case(c)
    n = case["n"]
    with _handle(case, L) as h:
        beta, trips, sum_p = h.beta, h.trips, h.sum_p
    flagged = L["flagged"]
    assert flagged.sum() <= 0.01 * n
    same = (beta == L["beta"]) & (trips == L["trips"])
    assert np.all(same | flagged), np.flatnonzero(~(same | flagged))[:10]
    for i in sorted(set(_sample(n)) | set(np.flatnonzero(flagged).tolist())):
        S, H, delta, bound = TK.mp_row(case["Xn"], i, L["idx"][i], beta[i], case["u"])
        assert bound <= T.CAP * S
        assert abs(_f(sum_p[i]) - S) <= bound, (i, float(_f(sum_p[i]) - S), float(bound))
        if trips[i] < T.MAX_TRIPS:
            assert abs(delta) < T.TOL + T.FLAG, (i, float(delta))
    assert 1 <= trips.min() and trips.max() <= T.MAX_TRIPS


# ---- 3. sparse P -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES + [pytest.param("hub", id="hub")])
def test_sparse_p(c):
    case, L = _case(c)
    n, d, K = case["n"], case["d"], L["K"]
    with _handle(case, L) as h:
        P = h.sparse_p()
        beta, S = h.beta, h.sum_p
        info = h.knn_info()
    indptr, indices, _ = TK.sparse_p(L["idx"], TK.cond_p(L["dist"], L["beta"], L["S"]))
    assert np.array_equal(P.indptr, indptr) and np.array_equal(P.indices, indices)
    rows = np.diff(indptr)
    assert info["nnz"] == P.nnz == indptr[-1] and info["longest_row"] == rows.max() and K <= rows.min() and rows.max() <= n - 1
    Pd = TK.dense(P.indptr, P.indices, P.data)
    assert Pd.tobytes() == np.ascontiguousarray(Pd.T).tobytes()         # symmetric bit for bit
    want, dP = TK.p_bounds(L["D"], d, beta, S, L["idx"])                # from the device's own beta and S
    # the cap is on a share of a SUM of absolute terms: of a row of P here, as of S_i in test_affinities.  A single far entry
    # (beta D in the hundreds, a value of e^-300) is off by more than CAP of ITSELF through its exponent, and by nothing of its row.
    assert np.all(dP.sum(axis=1) <= T.CAP * want.sum(axis=1))
    assert np.all(np.abs(Pd - want) <= 2 * dP)                          # both sides within dP of the exact value
    for i in _sample(n):                                                # and against 50 digits
        for q in range(indptr[i], indptr[i + 1]):
            j = int(indices[q])
            Dij = mp.fsum((_f(a) - _f(b)) ** 2 for a, b in zip(case["Xn"][i], case["Xn"][j]))
            ex = mp.mpf(0)
            if j in L["idx"][i]:
                ex += mp.exp(-_f(beta[i]) * Dij) / _f(S[i])
            if i in L["idx"][j]:
                ex += mp.exp(-_f(beta[j]) * Dij) / _f(S[j])
            assert abs(_f(P.data[q]) - ex / (2 * n)) <= dP[i, j], (i, j)
    assert abs(math.fsum(P.data) - 1.0) <= TK.sum_p_bound(dP, K, S)
    if c == "hub":
        assert rows[0] == n - 1 and rows[1:].max() <= 8


# ---- 4. forces ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FORCE_CASES)
def test_forces(c):
    case, L = _case(c)
    n, d = case["n"], case["d"]
    with _handle(case, L) as h:
        beta, S = h.beta, h.sum_p                       # the force kernels' own inputs
        sp_ = h.sparse_p()
        P = TK.dense(sp_.indptr, sp_.indices, sp_.data)
        for Y in (T.start(n, 3), T.spread_Y(n, 4)):
            h.set_state(Y)
            Z = T.mp_Z(Y)
            ref = {i: TK.mp_point(case["Xn"], beta, S, L["idx"], Y, i, 1.0, Z) for i in _sample(n)}
            for e in (12.0, 1.0):
                got = h.forces(e)
                again = h.forces(e)
                for key in got:
                    assert got[key].tobytes() == again[key].tobytes()
                want = TK.forces(P, Y, e)
                b = TK.force_bounds(L["D"], d, beta, S, L["idx"], Y, e, TILE)
                for key in ("A", "R", "z", "cost"):
                    assert np.all(b[key] <= T.CAP * b["abs_" + key] + 1e-300), key
                assert np.all(np.abs(got["A"] - want["A"]) <= 2 * b["A"])
                assert np.all(np.abs(got["R"] - want["R"]) <= 2 * b["R"])
                assert np.all(np.abs(got["z"] - want["z"]) <= 2 * b["z"])
                assert np.all(np.abs(got["cost_i"] - want["cost_i"]) <= 2 * b["cost"])
                for i, r in ref.items():
                    for col in range(2):
                        assert abs(_f(got["A"][i, col]) - _f(e) * r["A"][col]) <= b["A"][i, col], (i, col)
                        assert abs(_f(got["R"][i, col]) - r["R"][col]) <= b["R"][i, col], (i, col)
                    assert abs(_f(got["z"][i]) - r["z"]) <= b["z"][i], i
                    assert abs(_f(got["cost_i"][i]) - r["cost"]) <= b["cost"][i], i
            assert np.array_equal(h.state()[0], Y)      # forces() changes nothing


# ---- 5. against the dense path ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 257])
def test_all_neighbours_agree_with_the_dense_path(n):
    c = T.case(n, 10)
    D = T.sq_dist(c["Xn"])
    with C.TSNE(c["X"], perplexity=c["u"], neighbors=n - 1) as hk, C.TSNE(c["X"], perplexity=c["u"]) as hd:
        assert hk.neighbors == n - 1 and hd.neighbors is None
        idx = hk.knn()[0]
        for Y in (T.start(n, 3), T.spread_Y(n, 4)):
            hk.set_state(Y)
            hd.set_state(Y)
            for e in (12.0, 1.0):
                fk, fd = hk.forces(e), hd.forces(e)
                bk = TK.force_bounds(D, 10, hk.beta, hk.sum_p, idx, Y, e, TILE)
                bd = T.force_bounds(D, 10, hd.beta, hd.sum_p, Y, e)
                # not bitwise: the trees differ (the lists are in distance order, the dense rows in index order)
                assert np.array_equal(hk.beta, hd.beta) and np.array_equal(hk.trips, hd.trips)      # (no row of these is flagged)
                for key, bkey in (("A", "A"), ("R", "R"), ("z", "z"), ("cost_i", "cost")):
                    assert np.all(np.abs(fk[key] - fd[key]) <= bk[bkey] + bd[bkey]), key
        with pytest.raises(C.VBNMFError) as ei:
            hd.knn()
        assert ei.value.code == C._native.ERR_STATE
        with pytest.raises(C.VBNMFError):
            hd.sparse_p()


# ---- 6. stepping and reproducibility ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,K,iters", [(65, 10, 63, 10), (1030, 2, 90, 3)])
def test_step_by_step(n, d, K, iters):
    c = T.case(n, d)
    sch = dict(stop_lying_iter=3, mom_switch_iter=3)
    with C.TSNE(c["X"], perplexity=c["u"], neighbors=K) as h:
        h.set_state(T.start(n, 5))
        inside = total = 0
        for it in range(1, iters + 1):
            e, m = T.schedule(it, **sch)
            Y, uY, g = h.state()
            f = h.forces(e)
            h.run(1, first_iter=it, **sch)
            Y1, uY1, g1 = h.state()
            wY, wuY, wg, _ = T.update(Y, uY, g, f["A"], f["R"], f["z"], m)
            ub = T.update_bounds(Y, uY, g, f["A"], f["R"], f["z"], m)
            either = np.abs(ub["dY"]) <= ub["bdY"]      # may have taken the other gain: left out, and counted
            inside += int(either.sum())
            total += either.size
            ok = ~either
            assert np.all(np.abs(g1 - wg)[ok] <= ub["bgain"][ok]), it
            assert np.all(np.abs(uY1 - wuY)[ok] <= 2 * ub["buY"][ok]), it
            rows = ok.all(axis=1)
            assert np.all(np.abs(Y1 - wY)[rows] <= 2 * ub["bY"][rows]), it
            assert np.all(np.abs(Y1.mean(axis=0)) <= n * T.U * np.abs(Y1).max()), it
        assert inside <= 0.01 * total


def test_loop_is_reproducible_and_costs_are_those_of_forces():
    c = T.case(257, 10)
    sch = dict(stop_lying_iter=3, mom_switch_iter=3)
    Y0 = T.start(257, 6)
    with C.TSNE(c["X"], perplexity=c["u"], neighbors="auto") as h, C.TSNE(c["X"], perplexity=c["u"], neighbors=90) as h2:
        assert h.neighbors == 90
        assert h.sparse_p().data.tobytes() == h2.sparse_p().data.tobytes() and h.beta.tobytes() == h2.beta.tobytes()
        h.set_state(Y0)
        iters, costs = h.run(10, cost_every=3, **sch)
        whole = h.state()
        assert list(iters) == [3, 6, 9, 10]
        h2.set_state(Y0)
        iters2, costs2 = h2.run(10, cost_every=3, **sch)
        for x, y in zip(whole, h2.state()):
            assert x.tobytes() == y.tobytes()
        assert costs.tobytes() == costs2.tobytes()
        tm = h.knn_info()["times_ms"]
        assert all(tm[k] > 0.0 for k in ("search", "pattern", "last_attract", "last_repulse", "last_update"))
        assert h.info()["times_ms"]["last_force"] >= tm["last_attract"]
        h.set_state(Y0)
        single = {}
        for it in range(1, 11):
            its, cs = h.run(1, first_iter=it, cost_every=3, **sch)
            assert list(its) == [it]
            single[it] = cs[0]
            ci = h.forces(1.0)["cost_i"]
            # the same C_i, added in the device's tree (depth ceil(n / 1024) + 21) here and exactly there
            assert abs(cs[0] - math.fsum(ci)) <= 23 * T.U * math.fsum(np.abs(ci)), it
        for x, y in zip(whole, h.state()):
            assert x.tobytes() == y.tobytes()
        assert [single[int(i)] for i in iters] == list(costs)


# ---- 7. end to end -----------------------------------------------------------------------------------------------------------
_nn_same = T.nn_same


def test_three_clusters_end_to_end():
    """The restatement's final costs from the five starts are util_tsne_knn.E2E_FINAL (0.27471 .. 0.29299, a spread of
    0.01828); the device's run from start(300, 0) must end at or below E2E_FINAL[0] + 3 spreads = 0.34666."""
    c = T.case(T.E2E["n"], T.E2E["d"], T.E2E["k"], T.E2E["seed"])
    emb = C.tsne(c["X"], perplexity=c["u"], neighbors="auto", Y_init=T.start(c["n"], 0), cost_every=250)
    print("final cost", emb.itercosts[-1], "nn_same", _nn_same(emb.Y, c["lab"]))
    assert emb.neighbors == TK.E2E_K and list(emb.cost_iters) == [250, 500, 750, 1000]
    assert emb.itercosts[-1] < emb.itercosts[0]
    assert _nn_same(emb.Y, c["lab"]) == TK.E2E_NN_SAME
    spread = max(TK.E2E_FINAL) - min(TK.E2E_FINAL)
    assert emb.itercosts[-1] <= TK.E2E_FINAL[0] + 3 * spread
    assert abs(math.fsum(emb.costs) - emb.itercosts[-1]) <= 23 * T.U * math.fsum(np.abs(emb.costs))


# ---- 8. visualize_clusters -------------------------------------------------------------------------------------------------
def test_visualize_clusters_with_neighbors():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pbmc_extdata_r5.npz"))
    X = sp.csc_matrix((z["data"].astype(np.float64), z["indices"], z["indptr"]), shape=(int(z["n"]), int(z["m"])))
    vb = C.vb_factorize(C.CountMatrix(X), ranks=[5], nrun=1, Itmax=30, seed=1, verbose=0)
    m = C.visualize_clusters(vb, rank=5, neighbors="auto", max_iter=100, seed=2)
    cells = X.shape[1]
    assert m.rank == 5 and m.Y.shape == (cells, 2) and np.all(np.isfinite(m.Y))
    assert np.array_equal(m.cid, C.post.cluster_id(vb, 5)) and m.names == ["1", "2", "3", "4", "5"]
    assert sum(m.counts.values()) == cells and list(m.counts) == sorted(m.counts)
    assert all(m.counts[k] == int((m.cid == k).sum()) for k in m.counts)
    assert m.embedding.neighbors == 90 and np.all(np.isfinite(m.embedding.itercosts)) and len(m.embedding.beta) == cells
