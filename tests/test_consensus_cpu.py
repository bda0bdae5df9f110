"""Host side of the consensus measures (csrc/consensus.cpp, ccfindr_amd/consensus.py): the grouped cophenetic
correlation against scipy on the expanded cell matrix and against the oracle's cophenet on the pair vector, its edge
cases, and the arguments of factorize(consensus=...).  No GPU.

Tolerances: tie-free distances against scipy 1e-12 (both sides are a few roundings of the same sums); single linkage on
label matrices against the oracle 1e-9, the project's bound for the cophenetic (tests/test_gpu_mlnmf.py).
"""
import ctypes

import numpy as np
import pytest

from util_consensus import groups_of, pair_vector, random_labels

METHODS = ("average", "single", "complete")


def grouped_from_distances(D, sizes, method):
    from ccfindr_amd import _native as N
    L = N.load()
    D = np.ascontiguousarray(D, dtype=np.float64)
    s = np.ascontiguousarray(sizes, dtype=np.int64)
    out = ctypes.c_double()
    rc = L.vbnmf_test_cophenetic_dist(D.shape[0], N.dptr(D), s.ctypes.data_as(N.c_int64_p), method.encode(), ctypes.byref(out))
    return rc, out.value


def scipy_on_cells(D, sizes, method):
    """scipy's coefficient on the expanded matrix: every group as `size` cells at distance 0 from each other."""
    from scipy.cluster.hierarchy import cophenet, linkage
    from scipy.spatial.distance import squareform
    owner = np.repeat(np.arange(len(sizes)), sizes)
    full = D[np.ix_(owner, owner)]
    d = squareform(full, checks=False)
    c, _ = cophenet(linkage(d, method=method), d)
    return float(c)


@pytest.mark.parametrize("method", METHODS)
def test_tie_free_distances_match_scipy_on_the_expanded_matrix(method):
    rng = np.random.default_rng(20)
    worst = 0.0
    for G in range(3, 15):
        for trial in range(3):
            A = rng.uniform(0.05, 1.0, size=(G, G))
            D = np.triu(A, 1) + np.triu(A, 1).T            # symmetric, zero diagonal, all distances distinct
            sizes = rng.integers(1, 9, size=G)
            rc, got = grouped_from_distances(D, sizes, method)
            assert rc == 0
            want = scipy_on_cells(D, sizes, method)
            worst = max(worst, abs(got - want))
            assert abs(got - want) <= 1e-12, (G, trial, sizes.tolist(), got, want)
    print(f"{method}: largest difference {worst:.3g}")


@pytest.mark.parametrize("seed", range(8))
def test_single_linkage_on_label_matrices_matches_the_oracle(seed):
    import ccfindr_amd as C
    from oracle import mlnmf_oracle as O
    rng = np.random.default_rng(100 + seed)
    m, r, R = int(rng.integers(20, 121)), int(rng.integers(2, 6)), int(rng.integers(2, 8))
    L = random_labels(R, m, r, seed=200 + seed)
    tuples, sizes = groups_of(L)
    assert int(sizes.sum()) == m
    got = C.cophenetic_grouped(tuples, sizes, "single")
    want = O.cophenet(pair_vector(L) / R, m, "single")
    assert abs(got - want) <= 1e-9, (m, r, R, got, want)


def test_no_variance_gives_nan():
    import ccfindr_amd as C
    for method in METHODS:
        assert np.isnan(C.cophenetic_grouped(np.array([[1, 2, 1]]), [7], method))                 # G = 1: every distance is 0
        # three groups of one cell, each pair differing in every run: all distances are 1
        assert np.isnan(C.cophenetic_grouped(np.array([[1, 1], [2, 2], [3, 3]]), [1, 1, 1], method))
        rc, v = grouped_from_distances(0.3 * (1 - np.eye(4)), [1, 1, 1, 1], method)
        assert rc == 0 and np.isnan(v)
    # the same constant distance between groups of several cells has variance: pairs inside a group are at 0
    assert C.cophenetic_grouped(np.array([[1, 1], [2, 2], [3, 3]]), [2, 1, 1], "average") == pytest.approx(1.0, abs=1e-12)


def test_unknown_method_is_a_bad_argument():
    import ccfindr_amd as C
    with pytest.raises(C.VBNMFError) as ei:
        C.cophenetic_grouped(np.array([[1, 2], [2, 1]]), [1, 1], "ward")
    assert ei.value.code == 1
    rc, _ = grouped_from_distances(1 - np.eye(2), [1, 1], "centroid")
    assert rc == 1


def test_bad_sizes_and_shapes():
    import ccfindr_amd as C
    with pytest.raises(C.VBNMFError) as ei:
        C.cophenetic_grouped(np.array([[1, 2], [2, 1]]), [1, 0], "single")
    assert ei.value.code == 1
    with pytest.raises(ValueError):
        C.cophenetic_grouped(np.array([[1, 2], [2, 1]]), [1, 1, 1], "single")


def test_consensus_without_a_device_is_a_status():
    import ccfindr_amd as C
    if C.load().vbnmf_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(C.VBNMFError) as ei:
        C.Consensus(10, 3, 4)
    assert ei.value.code == 2 and "no CPU fallback" in str(ei.value)


def test_factorize_rejects_an_unknown_consensus_mode():
    import ccfindr_amd as C
    X = np.ones((4, 5))
    with pytest.raises(ValueError, match="consensus"):
        C.factorize(X, ranks=2, nrun=1, consensus="bogus")
    # what 'tables' cannot serve is refused before any engine is made
    with pytest.raises(ValueError, match="linkage"):
        C.factorize(X, ranks=2, nrun=1, consensus="tables", linkage="ward")
    with pytest.raises(ValueError, match="store_connectivity"):
        C.factorize(X, ranks=2, nrun=1, consensus="tables", store_connectivity=True)
