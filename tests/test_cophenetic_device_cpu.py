"""What the device cophenetic (csrc/cophenet.h) rests on, checked without a GPU: the host core's dendrogram trace
(vbnmf_test_cophenetic_trace, where = 0), the per-merge sums that replace the walk over member pairs, and the status of
a device request on a machine that has none."""
import ctypes

import numpy as np
import pytest

METHODS = ("average", "single", "complete")


def tie_case(G, R, seed, top=50):
    """G random label tuples in 1..3 (few values: many equal distances), their Hamming distances / R, sizes in 1..top."""
    rng = np.random.default_rng(seed)
    tuples = rng.integers(1, 4, size=(G, R)).astype(np.uint8)
    dist = np.sum(tuples[:, None, :] != tuples[None, :, :], axis=2).astype(np.float64) / R
    sizes = rng.integers(1, top + 1, size=G).astype(np.int64)
    return tuples, dist, sizes


def real_case(G, seed):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.1, 1.0, size=(G, G))
    d = np.triu(d, 1)
    return np.ascontiguousarray(d + d.T), rng.integers(1, 9, size=G).astype(np.int64)


def trace(where, dist, sizes, method, device=0):
    """(status, coefficient, merges [G-1][2], heights [G-1]) of vbnmf_test_cophenetic_trace."""
    from ccfindr_amd import _native as N
    L = N.load()
    G = len(sizes)
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    merges = np.full((max(G - 1, 0), 2), -1, dtype=np.int64)
    heights = np.full(max(G - 1, 0), np.nan)
    coph = ctypes.c_double()
    rc = L.vbnmf_test_cophenetic_trace(where, device, G, dist.ctypes.data_as(N.c_double_p), sizes.ctypes.data_as(N.c_int64_p),
                                       method.encode(), ctypes.byref(coph), merges.ctypes.data_as(N.c_int64_p),
                                       heights.ctypes.data_as(N.c_double_p))
    return rc, coph.value, merges, heights


def dist_hook(dist, sizes, method):
    from ccfindr_amd import _native as N
    L = N.load()
    coph = ctypes.c_double()
    N.check(L.vbnmf_test_cophenetic_dist(len(sizes), dist.ctypes.data_as(N.c_double_p), sizes.ctypes.data_as(N.c_int64_p),
                                         method.encode(), ctypes.byref(coph)))
    return coph.value


@pytest.mark.parametrize("G,R", [(2, 2), (3, 5), (65, 2), (257, 5)])
def test_host_trace_is_a_dendrogram_and_leaves_the_coefficient_alone(G, R):
    _, dist, sizes = tie_case(G, R, seed=10 * G + R)
    for method in METHODS:
        rc, coph, merges, heights = trace(0, dist, sizes, method)
        assert rc == 0
        keep, drop = merges[:, 0], merges[:, 1]
        assert np.all(keep < drop) and np.all(keep >= 0) and np.all(drop < G)
        assert sorted(drop.tolist()) == sorted(set(drop.tolist())) and len(drop) == G - 1      # each group leaves once ...
        assert 0 not in drop                                                                    # ... but the lowest, which is kept
        gone = {}
        for step, (k, d) in enumerate(merges.tolist()):
            assert k not in gone and d not in gone, (method, step)      # both clusters are still there when they merge
            gone[d] = step
        assert np.all(np.isfinite(heights)) and np.all(heights >= 0)
        if method != "average":                   # min and max are exact; a weighted mean of equal heights may round below them
            assert_heights_rise(merges, heights)
        want = dist_hook(dist, sizes, method)
        assert np.array([coph]).view(np.uint64)[0] == np.array([want]).view(np.uint64)[0], (method, coph, want)


def assert_heights_rise(merges, heights):
    """No inversion: the merge that absorbs a cluster is never lower than the merge that built it ('single', and
    'complete' as well).  The nearest-neighbour chain emits a merge when it finds a reciprocal pair, so in the
    order of the trace the heights may fall; it is along every path to the root that they do not."""
    last = {}                                     # cluster number -> height of the merge that last formed it
    for (k, d), h in zip(merges.tolist(), heights.tolist()):
        assert h >= last.get(k, 0.0) and h >= last.get(d, 0.0), (k, d, h)
        last[k] = h


def test_single_linkage_heights_are_those_of_the_minimum_spanning_tree():
    """'single' does not depend on tie choices: sorted, its heights are non-decreasing and equal the edge lengths of a
    minimum spanning tree of the distances (Prim, in numpy)."""
    G, R = 129, 5
    _, dist, sizes = tie_case(G, R, seed=77)
    rc, _, merges, heights = trace(0, dist, sizes, "single")
    assert rc == 0
    assert_heights_rise(merges, heights)
    best = dist[0].copy()
    inside = np.zeros(G, dtype=bool)
    inside[0] = True
    edges = []
    for _ in range(G - 1):
        j = int(np.argmin(np.where(inside, np.inf, best)))
        edges.append(best[j])
        inside[j] = True
        best = np.minimum(best, dist[j])
    assert np.array_equal(np.sort(heights), np.sort(np.array(edges)))


def agglomerate(dist, sizes, method):
    """The host rule in numpy, with the correlation's sums formed both ways: by the walk over member pairs and by the
    per-merge terms  h Wx Wy,  h^2 Wx Wy,  h S[x][y]  with S additive under merging."""
    G = len(sizes)
    W = dist.copy()
    S = dist * np.outer(sizes, sizes).astype(np.float64)
    weight = sizes.astype(np.float64)
    members = [[i] for i in range(G)]
    active = np.ones(G, dtype=bool)
    chain = []
    walk = np.zeros(3)
    terms = np.zeros(3)
    for _ in range(G - 1):
        if not chain:
            chain.append(int(np.flatnonzero(active)[0]))
        while True:
            x = chain[-1]
            prev = chain[-2] if len(chain) >= 2 else -1
            cand = np.where(active, W[x], np.inf)
            cand[x] = np.inf
            j = int(np.argmin(cand))              # the lowest-numbered minimum
            y = j if prev < 0 or cand[j] < W[x, prev] else prev
            if y == prev:
                break
            chain.append(y)
        chain.pop(), chain.pop()
        h = W[x, y]
        for i in members[x]:
            for j in members[y]:
                w = float(sizes[i]) * float(sizes[j])
                walk += (w * h, w * h * h, w * dist[i, j] * h)
        terms += (h * weight[x] * weight[y], h * h * weight[x] * weight[y], h * S[x, y])
        keep, drop = min(x, y), max(x, y)
        if method == "single":
            v = np.minimum(W[keep], W[drop])
        elif method == "complete":
            v = np.maximum(W[keep], W[drop])
        else:
            v = (weight[keep] * W[keep] + weight[drop] * W[drop]) / (weight[keep] + weight[drop])
        W[keep, :] = v
        W[:, keep] = v
        S[keep, :] += S[drop, :]
        S[:, keep] = S[keep, :]
        active[drop] = False
        weight[keep] += weight[drop]
        members[keep] += members[drop]
    return walk, terms


@pytest.mark.parametrize("method", METHODS)
def test_per_merge_terms_equal_the_member_pair_walk(method):
    for G, R, seed in ((40, 2, 1), (61, 5, 2)):
        _, dist, sizes = tie_case(G, R, seed)
        walk, terms = agglomerate(dist, sizes, method)
        # both are sums of at most G^2 / 2 non-negative terms in double: they agree to that many roundings
        assert np.all(np.abs(walk - terms) <= G * G * np.finfo(float).eps * np.abs(walk)), (method, walk, terms)
    dist, sizes = real_case(50, seed=3)
    walk, terms = agglomerate(dist, sizes, method)
    assert np.all(np.abs(walk - terms) <= 50 * 50 * np.finfo(float).eps * np.abs(walk)), (method, walk, terms)


def test_device_request_without_a_device_is_a_status():
    import ccfindr_amd as C
    if C.load().vbnmf_device_count() > 0:
        pytest.skip("a GPU is present")
    tuples, dist, sizes = tie_case(5, 2, seed=4)
    rc, coph, _, _ = trace(1, dist, sizes, "average")
    assert rc == 2 and np.isnan(coph)
    with pytest.raises(C.VBNMFError) as ei:
        C.cophenetic_grouped(tuples, sizes, "average", device=0)
    assert ei.value.code == 2
    # what is refused before a device is looked for
    assert trace(1, dist[:1, :1], sizes[:1], "average")[:1] == (0,)
    assert np.isnan(trace(1, dist[:1, :1], sizes[:1], "average")[1])
    assert trace(1, dist, sizes, "ward")[0] == 1
    assert trace(2, dist, sizes, "average")[0] == 1
    bad = dist.copy()
    bad[1, 3] = bad[3, 1] = np.inf
    assert trace(1, bad, sizes, "average")[0] == 1
    with pytest.raises(C.VBNMFError) as ei:
        C.cophenetic_grouped(tuples[:2], np.array([10 ** 8, 10 ** 8]), "average", device=0)      # cells^2 R / 2 >= 2^53
    assert ei.value.code == 1
