"""The grouped cophenetic with the agglomeration on the device (csrc/cophenet.h) against the host form (csrc/consensus.cpp):
the same dendrogram merge for merge and bit for bit, ties included; the same coefficient to the rounding of the sums; the
oracle's pair form under 'single'; more groups than the host form's cap; statuses instead of faults.

Tolerance of the coefficient.  The two sides sum differently (a long double walk over member pairs on the host,
compensated per-merge terms on the device), so they agree to rounding, not to the bit.  The largest |device - host| over
the inputs of test_same_coefficient_as_the_host, measured on an MI355X, is MEASURED_DIFF
(profiles/cophenetic_device.txt); the tests allow 16 times that, and never more than the 1e-9 that
tests/test_gpu_consensus.py allows between the grouped form and the oracle's pair form.
"""
import functools

import numpy as np
import pytest

from test_cophenetic_device_cpu import METHODS, real_case, tie_case, trace
from util_consensus import groups_of, pair_vector, random_labels

pytestmark = pytest.mark.gpu

MEASURED_DIFF = 6.856e-15
TOL = min(16 * MEASURED_DIFF, 1e-9)
SIZES = (2, 3, 63, 64, 65, 257, 1025, 2049)      # a wave, one and two passes of the 1024-thread workgroup, and their edges
CASES = [(G, R) for R in (2, 5) for G in SIZES]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def case(G, R):
    tuples, dist, sizes = tie_case(G, R, seed=100 * G + R)
    for a in (tuples, dist, sizes):
        a.setflags(write=False)
    return tuples, dist, sizes


def extra_cases():
    """Every size 1 (no pair of cells inside a group); sizes around 2e5 (weights near 4e10)."""
    t, _, s = tie_case(257, 5, seed=901)
    yield "ones", t, np.ones_like(s)
    t, _, s = tie_case(65, 5, seed=902)
    yield "large", t, 200000 + s


@pytest.mark.parametrize("G,R", CASES)
def test_same_dendrogram_as_the_host_under_ties(G, R):
    _, dist, sizes = case(G, R)
    for method in METHODS:
        rh, ch, mh, hh = trace(0, dist, sizes, method)
        rd, cd, md, hd = trace(1, dist, sizes, method)
        assert rh == 0 and rd == 0, (method, rh, rd)
        assert np.array_equal(mh, md), (method, np.flatnonzero(np.any(mh != md, axis=1))[:5])
        assert np.array_equal(bits(hh), bits(hd)), method
        print(f"trace G={G} R={R} {method}: |device - host| = {abs(cd - ch):.3e}")
        assert abs(cd - ch) <= TOL or (np.isnan(cd) and np.isnan(ch)), (method, cd, ch)


def test_same_dendrogram_on_tie_free_distances():
    dist, sizes = real_case(300, seed=5)
    for method in METHODS:
        rh, ch, mh, hh = trace(0, dist, sizes, method)
        rd, cd, md, hd = trace(1, dist, sizes, method)
        assert rh == 0 and rd == 0
        assert np.array_equal(mh, md) and np.array_equal(bits(hh), bits(hd)), method
        print(f"trace real G=300 {method}: |device - host| = {abs(cd - ch):.3e}")
        assert abs(cd - ch) <= TOL, (method, cd, ch)


def test_same_coefficient_as_the_host():
    import ccfindr_amd as C
    inputs = [(f"G={G} R={R}", *case(G, R)[::2]) for G, R in CASES] + list(extra_cases())
    worst = 0.0
    failed = []
    for name, tuples, sizes in inputs:
        for method in METHODS:
            host = C.cophenetic_grouped(tuples, sizes, method)
            dev = C.cophenetic_grouped(tuples, sizes, method, device=0)
            if np.isnan(host) or np.isnan(dev):
                assert np.isnan(host) and np.isnan(dev), (name, method, host, dev)
                continue
            diff = abs(dev - host)
            worst = max(worst, diff)
            print(f"coefficient {name} {method}: host {host!r} device {dev!r} diff {diff:.3e}")
            if diff > TOL:
                failed.append((name, method, host, dev))
    print(f"largest |device - host| = {worst:.3e}")
    assert not failed, failed


@pytest.mark.parametrize("m,r,R", [(90, 3, 5), (400, 4, 8)])
def test_against_the_oracles_pair_form(m, r, R):
    import ccfindr_amd as C
    from oracle import mlnmf_oracle as O
    L = random_labels(R, m, r, seed=31 + m)
    cons = C.Consensus(m, r, R)
    for row in L:
        cons.add(row)
    got = cons.cophenetic("single", where="device")
    cons.close()
    assert abs(got - O.cophenet(pair_vector(L) / R, m, "single")) <= 1e-9


@pytest.fixture(scope="module")
def past_the_cap():
    """6000 cells with random labels in 1..4 over 12 runs: 5999 distinct tuples.  (accumulator, tuples, sizes)"""
    import ccfindr_amd as C
    m, r, R = 6000, 4, 12
    L = random_labels(R, m, r, seed=61)
    cons = C.Consensus(m, r, R)
    for row in L:
        cons.add(row)
    yield (cons, *groups_of(L))
    cons.close()


def test_past_the_host_cap(past_the_cap):
    import ccfindr_amd as C
    cons, tuples, sizes = past_the_cap
    got, groups = cons.cophenetic("average", with_groups=True)
    assert groups == len(sizes) and groups > C.consensus.DEFAULT_MAX_GROUPS
    assert np.isfinite(got) and -1.0 <= got <= 1.0
    assert got == C.cophenetic_grouped(tuples, sizes, "average", device=0) == cons.cophenetic("average", where="device")
    assert np.isnan(cons.cophenetic("average", where="host"))
    for where in ("host", "device", None):
        capped, g = cons.cophenetic("average", max_groups=groups - 1, with_groups=True, where=where)
        assert np.isnan(capped) and g == groups


def test_past_the_host_cap_agrees_with_the_uncapped_host(past_the_cap):
    """5999 groups, 'average': the cophenetic distances have little variance here (sum c^2 / var c = 1510), which magnifies
    any loss in the sums a thousandfold.  The same sums in exact rational arithmetic (Python fractions over the host's merges
    and heights) give 0.15447341519300772; the device gives 0.154473415193002.  The host walk adds 1.8e7 terms: with plain
    long double sums it gave 0.1544734151912227, 1.8e-12 off, which is why above 4096 groups it keeps each addition's
    rounding error (csrc/consensus.cpp: WalkSum) and now returns the exact value's double."""
    import ccfindr_amd as C
    cons, tuples, sizes = past_the_cap
    got = cons.cophenetic("average")
    want = C.cophenetic_grouped(tuples, sizes, "average")                 # the host form has no cap of its own
    print(f"past the cap: groups {len(sizes)} host {want!r} device {got!r} diff {abs(got - want):.3e} allowed {TOL:.3e}")
    assert abs(got - want) <= TOL


def test_two_calls_give_the_same_bits():
    import ccfindr_amd as C
    tuples, dist, sizes = case(1025, 5)
    for method in METHODS:
        a = trace(1, dist, sizes, method)
        b = trace(1, dist, sizes, method)
        assert a[0] == 0 and b[0] == 0
        assert np.array_equal(bits([a[1]]), bits([b[1]])) and np.array_equal(a[2], b[2]) and np.array_equal(bits(a[3]), bits(b[3]))
        c = [C.cophenetic_grouped(tuples, sizes, method, device=0) for _ in range(2)]
        assert np.array_equal(bits([c[0]]), bits([c[1]]))
    dist, sizes = real_case(300, seed=5)
    a, b = trace(1, dist, sizes, "average"), trace(1, dist, sizes, "average")
    assert np.array_equal(bits([a[1]]), bits([b[1]])) and np.array_equal(a[2], b[2]) and np.array_equal(bits(a[3]), bits(b[3]))


def test_statuses_not_faults():
    import ccfindr_amd as C
    tuples, dist, sizes = tie_case(9, 3, seed=7)
    # one group: NaN, status OK
    rc, coph, _, _ = trace(1, dist[:1, :1], sizes[:1], "average")
    assert rc == 0 and np.isnan(coph)
    assert np.isnan(C.cophenetic_grouped(tuples[:1], sizes[:1], "average", device=0))
    # a distance that is not finite
    for bad_value in (np.inf, np.nan):
        bad = dist.copy()
        bad[2, 5] = bad[5, 2] = bad_value
        assert trace(1, bad, sizes, "average")[0] == 1
    # a linkage that is not served
    assert trace(1, dist, sizes, "ward")[0] == 1
    with pytest.raises(C.VBNMFError) as ei:
        C.cophenetic_grouped(tuples, sizes, "ward", device=0)
    assert ei.value.code == 1
    # cells^2 R / 2 >= 2^53: the weighted sums would no longer be exact
    with pytest.raises(C.VBNMFError) as ei:
        C.cophenetic_grouped(tuples[:2], np.array([10 ** 8, 10 ** 8]), "average", device=0)
    assert ei.value.code == 1
    # a size below 1, a device that is not there, a `where` that means nothing
    with pytest.raises(C.VBNMFError) as ei:
        C.cophenetic_grouped(tuples, np.zeros_like(sizes), "average", device=0)
    assert ei.value.code == 1
    with pytest.raises(C.VBNMFError) as ei:
        C.cophenetic_grouped(tuples, sizes, "average", device=C.load().vbnmf_device_count())
    assert ei.value.code == 1
    assert trace(2, dist, sizes, "average")[0] == 1
    # a label 0 in the accumulator: NaN
    m, r = 300, 4
    L = random_labels(3, m, r, seed=8, zero_at=(1, 17))
    cons = C.Consensus(m, r, 3)
    for row in L:
        cons.add(row)
    assert np.isnan(cons.cophenetic("single", where="device"))
    with pytest.raises(ValueError):
        cons.cophenetic("single", where="gpu")
    cons.close()
