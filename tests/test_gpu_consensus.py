"""The consensus accumulator on the device (vbnmf_consensus_*, csrc/consensus.h) and factorize(consensus='tables').

The checker is the reference's own arithmetic on the O(m^2) pair vector (oracle/mlnmf_oracle.py: dispersion, cophenet) and an
int64 numpy restatement of the sums S1, S2.  Tolerances are the project's (tests/test_gpu_mlnmf.py): dispersion 1e-12,
cophenetic 1e-9; the integer sums are compared exactly.
"""
import importlib

import numpy as np
import pytest

from util_consensus import groups_of, integer_sums, pair_vector, random_labels

pytestmark = pytest.mark.gpu

RANKS = (1, 2, 5, 16, 17, 64, 128)


def counts(n, m, lam, seed):
    rng = np.random.default_rng(seed)
    X = rng.poisson(lam, size=(n, m)).astype(np.float64)
    X[np.arange(n), rng.integers(0, m, n)] += 1      # no empty rows
    X[rng.integers(0, n, m), np.arange(m)] += 1      # no empty columns
    return np.asfortranarray(X)


@pytest.mark.parametrize("m", [1, 2, 255, 256, 257, 1031])
def test_host_labels_against_the_pair_vector(m):
    import ccfindr_amd as C
    from oracle import mlnmf_oracle as O
    R = 7
    for r in RANKS:
        L = random_labels(R, m, r, seed=1000 * r + m)
        cons = C.Consensus(m, r, R)
        conav = np.zeros(m * (m - 1) // 2)
        for irun in range(1, R + 1):
            cons.add(L[irun - 1])
            conav = conav + pair_vector(L[irun - 1:irun])
            got, want = cons.dispersion(), O.dispersion(conav / irun, m)
            assert abs(got - want) <= 1e-12, (m, r, irun, got, want)
            s = cons.sums()
            s1, s2 = integer_sums(L[:irun], r)
            assert (s["runs"], s["s1"], s["s2"], s["unlabelled"]) == (irun, s1, s2, False), (m, r, irun)
        assert np.array_equal(cons.labels(R - 1), L[R - 1]) and cons.labels(0).dtype == np.int32
        cons.close()


@pytest.mark.parametrize("r", [128, 3])
def test_sums_past_one_workgroup_one_chunk_and_64k_of_lds(r):
    """70 001 cells: nine chunks of cells per stored run; rank 128: a 129 x 129 table of uint32 = 66.6 KB of LDS.  2.45e9 pairs:
    no pair vector is formed here, the integers are checked against numpy's and against a second pass."""
    import ccfindr_amd as C
    m, R = 70001, 3
    L = random_labels(R, m, r, seed=5 + r)
    L[1, : m // 2] = L[0, : m // 2]                   # runs that agree on half the cells: large bins beside the small ones
    want = integer_sums(L, r)
    seen = []
    for _ in range(2):
        cons = C.Consensus(m, r, R)
        for row in L:
            cons.add(row)
        s = cons.sums()
        seen.append((s["s1"], s["s2"]))
        d = cons.dispersion()
        cons.close()
        assert seen[-1] == want and s["runs"] == R and not s["unlabelled"]
        assert 0.0 < d <= 1.0
    assert seen[0] == seen[1]


def test_label_zero_gives_nan_and_raises_the_flag():
    import ccfindr_amd as C
    m, r = 300, 4
    L = random_labels(3, m, r, seed=8, zero_at=(1, 17))
    cons = C.Consensus(m, r, 3)
    cons.add(L[0])
    assert not cons.sums()["unlabelled"] and np.isfinite(cons.dispersion())
    cons.add(L[1])
    cons.add(L[2])
    s = cons.sums()
    assert s["unlabelled"] and np.isnan(cons.dispersion())
    assert (s["s1"], s["s2"]) == integer_sums(L, r)      # label 0 is a bin like any other in the integers
    assert np.isnan(cons.cophenetic("single"))
    cons.reset()
    cons.add(L[0])
    assert not cons.sums()["unlabelled"] and cons.sums()["runs"] == 1 and np.isfinite(cons.dispersion())
    cons.close()


def test_cophenetic_of_the_accumulator_and_the_group_cap():
    import ccfindr_amd as C
    from oracle import mlnmf_oracle as O
    m, r, R = 90, 3, 5
    L = random_labels(R, m, r, seed=31)
    cons = C.Consensus(m, r, R)
    for row in L:
        cons.add(row)
    tuples, sizes = groups_of(L)
    got, groups = cons.cophenetic("single", with_groups=True)
    assert groups == len(sizes)
    assert got == C.cophenetic_grouped(tuples, sizes, "single")
    assert abs(got - O.cophenet(pair_vector(L) / R, m, "single")) <= 1e-9
    for method in ("average", "complete"):
        assert cons.cophenetic(method) == C.cophenetic_grouped(tuples, sizes, method)
    capped, groups = cons.cophenetic("single", max_groups=len(sizes) - 1, with_groups=True)
    assert np.isnan(capped) and groups == len(sizes)
    with pytest.raises(C.VBNMFError) as ei:
        cons.cophenetic("ward")
    assert ei.value.code == 1
    cons.close()


def test_add_engine_takes_the_engines_labels_and_leaves_its_label_state():
    import ccfindr_amd as C
    n, m, r = 50, 300, 4
    X = counts(n, m, 0.8, seed=71)
    rng = np.random.default_rng(72)
    w, h = rng.uniform(size=(n, r)), rng.uniform(size=(r, m))
    h[:, 3] = [0.5, 0.9, 0.9, 0.1]                    # a tie: the first maximum wins
    h[:, 4] = [np.nan, 0.2, 0.1, 0.05]                # NaN never wins
    h[:, 7] = np.nan                                  # no label
    M = C.CountMatrix(X)
    eng = C.VBEngine(M, r)
    eng.ml_set_state(w, h)
    cons = C.Consensus(m, r, 2)
    cons.add(eng)
    ids = eng.cluster_ids()
    got = cons.labels(0)
    assert np.array_equal(got, ids) and (got[3], got[4], got[7]) == (2, 2, 0)
    assert cons.sums()["unlabelled"] and np.isnan(cons.dispersion())
    assert (cons.sums()["s1"], cons.sums()["s2"]) == integer_sums(ids[None, :], r)
    cons.close()
    # the engine's previous-label state: a twin that never meets an accumulator reports the same counts and labels
    h = rng.uniform(size=(r, m))
    twin = C.VBEngine(M, r)
    cons = C.Consensus(m, r, 3)
    trace = []
    for e, adds in ((eng, True), (twin, False)):
        e.ml_set_state(w, h)
        seq = []
        for _ in range(3):
            e.ml_step()
            if adds:
                cons.add(e)
            ch, ids = e.cluster_changes(want_ids=True)
            seq.append((ch, ids.tolist()))
        trace.append(seq)
    assert trace[0] == trace[1]
    for k in range(3):
        assert np.array_equal(cons.labels(k), np.array(trace[0][k][1]))
    cons.close()
    eng.close()
    twin.close()
    M.close()


def _same_fit(a, b):
    assert a.measure["likelihood"] == b.measure["likelihood"] and a.nsteps == b.nsteps
    for k in range(len(a.ranks)):
        assert np.array_equal(a.basis[k], b.basis[k]) and np.array_equal(a.coeff[k], b.coeff[k])


@pytest.mark.parametrize("kw", [dict(nrun=3), dict(nrun=4, batch=2)])
def test_factorize_tables_against_pairs(kw):
    import ccfindr_amd as C
    X = counts(60, 110, 0.8, seed=41)
    args = dict(ranks=[2, 3], verbose=0, seed=5, Itmax=300, linkage="single", **kw)
    a = C.factorize(X, consensus="pairs", **args)
    b = C.factorize(X, consensus="tables", **args)
    c = C.factorize(X, **args)                                 # auto below the cap: the pair vector, bit for bit
    _same_fit(a, b)
    _same_fit(a, c)
    assert a.measure["dispersion"] == c.measure["dispersion"] and a.measure["cophenetic"] == c.measure["cophenetic"]
    for k in range(2):
        assert abs(a.measure["dispersion"][k] - b.measure["dispersion"][k]) <= 1e-12, (a.measure, b.measure)
        assert abs(a.measure["cophenetic"][k] - b.measure["cophenetic"][k]) <= 1e-9, (a.measure, b.measure)


def test_factorize_above_the_pair_cap_reports_the_measures(monkeypatch):
    import ccfindr_amd as C
    F = importlib.import_module("ccfindr_amd.factorize")
    monkeypatch.setattr(F, "MAX_PAIRS", 1000)                    # 110 cells: 5 995 pairs
    X = counts(60, 110, 0.8, seed=41)
    args = dict(ranks=[2, 3], nrun=3, verbose=0, seed=5, Itmax=300)
    auto = C.factorize(X, **args)
    tab = C.factorize(X, consensus="tables", **args)
    _same_fit(auto, tab)
    for k in range(2):
        d, c = auto.measure["dispersion"][k], auto.measure["cophenetic"][k]
        assert 0.0 < d <= 1.0 and -1.0 <= c <= 1.0, auto.measure
        assert d == tab.measure["dispersion"][k] and c == tab.measure["cophenetic"][k]
    # what the tables cannot serve stays NaN under auto, as before
    other = C.factorize(X, linkage="ward", store_connectivity=True, **args)
    assert np.all(np.isnan(other.measure["cophenetic"])) and other.metadata == {}
    assert other.measure["dispersion"] == auto.measure["dispersion"]
    # an explicit 'pairs' above the cap is today's answer
    pairs = C.factorize(X, consensus="pairs", **args)
    assert np.all(np.isnan(pairs.measure["dispersion"])) and np.all(np.isnan(pairs.measure["cophenetic"]))


def test_handle_errors():
    import ccfindr_amd as C
    n, m, r = 30, 64, 3
    X = counts(n, m, 1.0, seed=3)
    M = C.CountMatrix(X)
    rng = np.random.default_rng(4)
    eng = C.VBEngine(M, r)
    cons = C.Consensus(m, r, 2)
    with pytest.raises(C.VBNMFError) as ei:
        cons.add(eng)                                          # no state yet
    assert ei.value.code == 5
    with pytest.raises(C.VBNMFError) as ei:
        cons.dispersion()                                      # no run yet
    assert ei.value.code == 5
    eng.ml_set_state(rng.uniform(size=(n, r)), rng.uniform(size=(r, m)))
    cons.add(eng)
    cons.add(eng.cluster_ids())
    for extra in (eng, eng.cluster_ids()):
        with pytest.raises(C.VBNMFError) as ei:
            cons.add(extra)                                    # past max_runs
        assert ei.value.code == 1
    assert cons.sums()["runs"] == 2 and cons.dispersion() == 1.0      # the same partition twice
    for bad in (np.full(m, r + 1), np.array([1, 2, -1] + [1] * (m - 3))):
        with pytest.raises(C.VBNMFError) as ei:
            cons.add(bad)
        assert ei.value.code == 1
    cons.close()
    mismatched = [C.Consensus(m + 1, r, 2), C.Consensus(m, r + 1, 2)]
    if C.load().vbnmf_device_count() > 1:
        mismatched.append(C.Consensus(m, r, 2, device=1))
    for other in mismatched:
        with pytest.raises(C.VBNMFError) as ei:
            other.add(eng)
        assert ei.value.code == 1
        other.close()
    for bad in (dict(m=0, rank=r, max_runs=2), dict(m=m, rank=129, max_runs=2), dict(m=m, rank=r, max_runs=0)):
        with pytest.raises(C.VBNMFError) as ei:
            C.Consensus(**bad)
        assert ei.value.code == 1
    # a partitioned engine holds part of the cells: its labels go through the host
    comm = C.Communicator.local(2)
    cuts = [(0, m // 2), (m // 2, m)]
    parts = [C.VBEngine(M, r, cols=c, m_global=m) for c in cuts]
    for p in parts:
        p.attach_comm(comm)
    cons = C.Consensus(m // 2, r, 2)
    with pytest.raises(C.VBNMFError) as ei:
        cons.add(parts[0])
    assert ei.value.code == 5
    cons.close()
    for t in parts + [comm, eng, M]:
        t.close()
