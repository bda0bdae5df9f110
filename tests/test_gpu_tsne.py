"""k_tsne_affinity / k_tsne_force / k_tsne_update (csrc/tsne.h) behind ccfindr_amd.embed on the device, against the numpy
restatement and the 50-digit forms of tests/util_tsne.py, where every bound is derived.  Sizes are aimed at the kernels' edges,
taken from vbnmf_tsne_info: IB = the force kernel's i-block, JT = its j-tile, ROW = the affinity kernel's LDS row capacity."""
import math
import os
import sys

import mpmath as mp
import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_tsne as T  # noqa: E402

import ccfindr_amd as C  # noqa: E402
from ccfindr_amd import embed as E  # noqa: E402

pytestmark = pytest.mark.gpu

INFO = E.tsne_info()
IB, JT, ROW = INFO["i_block"], INFO["j_tile"], INFO["lds_row_capacity"]
SHAPES, BIG = T.shape_cases(IB, JT, ROW)
CASES = [pytest.param(T.shape_kw(c), id="n%d-d%d" % c[:2]) for c in SHAPES] + [pytest.param(v, id=k) for k, v in T.SPECIAL.items()]


def _case(kw):
    kw = dict(kw)
    key = (kw.pop("n"), kw.pop("d"))
    return T.case(*key, **kw), T.case_affinities(*key, **kw)


def _sample(n):
    """The first and last row and the rows at the edges of a wave, the j-tile and the i-block."""
    return sorted({i for i in (0, 1, JT - 1, JT, 63, 64, IB - 1, IB, n // 2, n - 2, n - 1) if 0 <= i < n})


def _handle(c):
    return C.TSNE(c["X"], perplexity=c["u"], normalize=c["normalize"])


_f = T._f


# ---- 1. affinities -----------------------------------------------------------------------------------------------------------
def _check_affinities(c, a, h):
    n = c["n"]
    flagged = a["flagged"]
    assert flagged.sum() <= 0.01 * n
    same = (h.beta == a["beta"]) & (h.trips == a["trips"])
    assert np.all(same | flagged), np.flatnonzero(~(same | flagged))[:10]
    rows = sorted(set(_sample(n)) | set(np.flatnonzero(flagged).tolist()))
    for i in rows:
        S, H, delta, bound = T.mp_row(c["Xn"], i, h.beta[i], c["u"])
        assert bound <= T.CAP * S
        assert abs(_f(h.sum_p[i]) - S) <= bound, (i, float(_f(h.sum_p[i]) - S), float(bound))
        if h.trips[i] < T.MAX_TRIPS:
            assert abs(delta) < T.TOL + T.FLAG, (i, float(delta))
    assert 1 <= h.trips.min() and h.trips.max() <= T.MAX_TRIPS


FULL_ROW = T.full_lds_row(ROW)


@pytest.mark.parametrize("kw", CASES + [pytest.param(T.shape_kw(FULL_ROW), id="n%d-d%d" % FULL_ROW[:2])])
def test_affinities(kw):
    c, a = _case(kw)
    with _handle(c) as h:
        _check_affinities(c, a, h)
        info = h.info()
    assert info["force_grid"] == -(-c["n"] // IB) and 1 <= info["affinity_grid"] <= c["n"]
    if c["n"] == ROW:
        # fewer workgroups than points: a workgroup takes its second point's distances into the LDS row of its first
        assert info["affinity_grid"] < c["n"], info["affinity_grid"]


def test_affinities_row_past_the_lds_capacity():
    c, a = _case(dict(n=BIG[0], d=BIG[1]))
    assert c["n"] == ROW + 1
    with _handle(c) as h:
        _check_affinities(c, a, h)


def test_special_inputs_on_the_device():
    c, _ = _case(T.SPECIAL["identical"])
    with _handle(c) as h:
        assert np.all(h.trips == T.MAX_TRIPS) and np.all(h.beta == 2.0 ** 200) and np.all(h.sum_p == c["n"] - 1)
    c, _ = _case(T.SPECIAL["outlier"])
    with _handle(c) as h:
        assert h.beta[c["n"] // 2] < 1e-3


# ---- 2. forces ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", CASES)
def test_forces(kw):
    c, a = _case(kw)
    n, d = c["n"], c["d"]
    with _handle(c) as h:
        beta, S = h.beta, h.sum_p                       # the force kernel's own inputs
        P = T.joint_p(a["D"], beta, S)
        for Y in (T.start(n, 3), T.spread_Y(n, 4)):
            h.set_state(Y)
            Z = T.mp_Z(Y)
            ref = {i: T.mp_point(c["Xn"], beta, S, Y, i, 1.0, Z) for i in _sample(n)}
            for e in (12.0, 1.0):
                got = h.forces(e)
                again = h.forces(e)
                for key in got:
                    assert got[key].tobytes() == again[key].tobytes()
                want = T.forces(P, Y, e)
                b = T.force_bounds(a["D"], d, beta, S, Y, e)
                for key in ("A", "R", "z", "cost"):
                    assert np.all(b[key] <= T.CAP * b["abs_" + key] + 1e-300), key
                # every point against the restatement: both sides are within the bound of the exact value
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


# ---- 3. step -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,iters", [(65, 10, 10), (1030, 2, 3)])
def test_step_by_step(n, d, iters):
    c = T.case(n, d)
    sch = dict(stop_lying_iter=3, mom_switch_iter=3)
    with _handle(c) as h:
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


# ---- 4. loop -----------------------------------------------------------------------------------------------------------------
def test_loop_is_reproducible_and_costs_are_those_of_forces():
    c = T.case(257, 10)
    sch = dict(stop_lying_iter=3, mom_switch_iter=3)
    Y0 = T.start(257, 6)
    with _handle(c) as h:
        h.set_state(Y0)
        iters, costs = h.run(10, cost_every=3, **sch)
        whole = h.state()
        assert list(iters) == [3, 6, 9, 10]
        h.set_state(Y0)
        iters2, costs2 = h.run(10, cost_every=3, **sch)
        again = h.state()
        for x, y in zip(whole, again):
            assert x.tobytes() == y.tobytes()
        assert costs.tobytes() == costs2.tobytes()
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


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------
_nn_same = T.nn_same


def test_three_clusters_end_to_end():
    c = T.case(T.E2E["n"], T.E2E["d"], T.E2E["k"], T.E2E["seed"])
    emb = C.tsne(c["X"], perplexity=c["u"], Y_init=T.start(c["n"], 0), cost_every=250)
    assert list(emb.cost_iters) == [250, 500, 750, 1000]
    assert emb.itercosts[-1] < emb.itercosts[0]                        # below the cost when the exaggeration ends
    assert _nn_same(emb.Y, c["lab"]) == T.E2E_NN_SAME                  # as the restatement on the CPU (tests/util_tsne.py)
    # The trajectories are chaotic and need not agree pointwise.  The restatement's final cost from the same start is
    # E2E_FINAL[0] = 0.28726; over the five starts its final costs span 0.27406 .. 0.30152, a spread of 0.02746 (measured on
    # the CPU, recorded in tests/util_tsne.py): the margin is three times that spread.
    spread = max(T.E2E_FINAL) - min(T.E2E_FINAL)
    assert emb.itercosts[-1] <= T.E2E_FINAL[0] + 3 * spread
    assert abs(math.fsum(emb.costs) - emb.itercosts[-1]) <= 23 * T.U * math.fsum(np.abs(emb.costs))


def test_visualize_clusters_on_a_fit_of_the_shipped_sample():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pbmc_extdata_r5.npz"))
    X = sp.csc_matrix((z["data"].astype(np.float64), z["indices"], z["indptr"]), shape=(int(z["n"]), int(z["m"])))
    vb = C.vb_factorize(C.CountMatrix(X), ranks=[3, 4], nrun=1, Itmax=30, seed=1, verbose=0)
    m = C.visualize_clusters(vb, max_iter=100, seed=2)
    cells = X.shape[1]
    assert m.rank == 3 and m.Y.shape == (cells, 2) and np.all(np.isfinite(m.Y))
    assert np.array_equal(m.cid, C.post.cluster_id(vb, 3)) and m.names == ["1", "2", "3"]
    assert sum(m.counts.values()) == cells and list(m.counts) == sorted(m.counts)
    assert all(m.counts[k] == int((m.cid == k).sum()) for k in m.counts)
    assert np.all(np.isfinite(m.embedding.itercosts)) and len(m.embedding.beta) == cells
    m4 = C.visualize_clusters(vb, rank=4, max_iter=20, seed=2)
    assert m4.rank == 4 and m4.names == ["1", "2", "3", "4"]
    with pytest.raises(IndexError):
        C.visualize_clusters(vb, rank=7)
