#!/usr/bin/env python3
"""profiles/cophenetic_device_bench.py -- the grouped cophenetic on the host (csrc/consensus.cpp) and on the device
(csrc/cophenet.h): wall time per linkage on random label tuples, the group counts of two factorize() runs, and the
host-device differences the tolerance of tests/test_gpu_cophenetic_device.py rests on.

    python profiles/cophenetic_device_bench.py [times] [groups] [diffs]      (default: all three)

Prints the text of profiles/cophenetic_device.txt.  One MI355X.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ccfindr_amd as C  # noqa: E402
from ccfindr_amd import consensus as K  # noqa: E402

METHODS = ("average", "single", "complete")
HOST_UP_TO = 8192           # the host form is run (with no cap of its own) up to this many groups for every linkage,
HOST_ONE_AT = 16384         # and for 'average' alone at this many (2 GB of doubles and 0.5 GB of Hamming distances a call)


def say(*a):
    print(*a)
    sys.stdout.flush()


def random_groups(G, R, seed, rank=10):
    """G distinct random label tuples of R runs with labels in 1..rank, sizes in 1..50."""
    rng = np.random.default_rng(seed)
    tuples = np.unique(rng.integers(1, rank + 1, size=(G + G // 8, R)).astype(np.uint8), axis=0)
    tuples = np.ascontiguousarray(rng.permutation(tuples)[:G])
    assert len(tuples) == G
    return tuples, rng.integers(1, 51, size=G).astype(np.int64)


def times():
    say("Wall time of one coefficient, random distinct tuples, R = 20, labels 1..10, sizes 1..50 (upload, both kernels and")
    say("downloads included on the device; the host form run with no cap: the parent commit's code, above 4096 groups with compensated sums):")
    C.cophenetic_grouped(*random_groups(64, 20, 0), "average", device=0)          # first use of the device
    for G in (1024, 4096, 8192, 16384, 32768):
        tuples, sizes = random_groups(G, 20, seed=G)
        for method in METHODS:
            t0 = time.perf_counter()
            dev = C.cophenetic_grouped(tuples, sizes, method, device=0)
            td = time.perf_counter() - t0
            if G <= HOST_UP_TO or (G == HOST_ONE_AT and method == "average"):
                t0 = time.perf_counter()
                host = C.cophenetic_grouped(tuples, sizes, method)
                th = time.perf_counter() - t0
                say(f"  G {G:6d} {method:9s} device {td:8.3f} s   host {th:8.3f} s   device {dev:.15f} host {host:.15f} diff {abs(dev - host):.2e}")
            else:
                say(f"  G {G:6d} {method:9s} device {td:8.3f} s   host not run   device {dev:.15f}")


def groups():
    import scipy.sparse as sp
    from ccfindr_amd import synth
    seen = []
    plain = K.Consensus.cophenetic

    def counting(self, method="average", max_groups=None, with_groups=False, where=None):
        t0 = time.perf_counter()
        coph, g = plain(self, method, max_groups, True, where)
        seen.append((g, coph, time.perf_counter() - t0))
        return (coph, g) if with_groups else coph

    K.Consensus.cophenetic = counting
    try:
        n, m, k = 20000, 50000, 10
        depth = np.round(np.random.default_rng(3).lognormal(np.log(1500.0), 0.3, size=m)).astype(np.int64)
        X = synth.fill_empty(synth.simulate_data(n, [m // k] * k, alpha0=0.065, seed=3, depth=depth), seed=3)
        t0 = time.perf_counter()
        res = C.factorize(X, ranks=10, nrun=20, Itmax=30, seed=3, verbose=0)
        say(f"factorize(ranks=10, nrun=20, Itmax=30, seed=3) on the 20000 x 50000 generator of consensus_tables.txt, nnz {X.nnz}: "
            f"{time.perf_counter() - t0:.2f} s")
        say(f"  groups {seen[-1][0]}, cophenetic {seen[-1][1]!r} in {seen[-1][2]:.3f} s, dispersion {res.measure['dispersion'][0]!r}")
        d = np.load(os.path.join(ROOT, "tests", "golden", "pbmc_extdata_r5.npz"))
        n, m = int(d["n"]), int(d["m"])
        X = sp.csc_matrix((d["data"].astype(np.float64), d["indices"], d["indptr"]), shape=(n, m))
        t0 = time.perf_counter()
        res = C.factorize(X, ranks=5, nrun=20, seed=3, verbose=0, consensus="tables")
        say(f"factorize(ranks=5, nrun=20, seed=3, consensus='tables') on the PBMC sample ({n} x {m}): {time.perf_counter() - t0:.2f} s")
        say(f"  groups {seen[-1][0]}, cophenetic {seen[-1][1]!r} in {seen[-1][2]:.3f} s, dispersion {res.measure['dispersion'][0]!r}")
    finally:
        K.Consensus.cophenetic = plain


def diffs():
    import test_gpu_cophenetic_device as T
    say("Largest |device - host| of the coefficient over the inputs of tests/test_gpu_cophenetic_device.py")
    say("(test_same_coefficient_as_the_host: tuples built to tie, G in 2..2049, R in {2, 5}, sizes 1..50; every size 1; sizes near 2e5):")
    worst = 0.0
    inputs = [(f"G={G} R={R}", *T.case(G, R)[::2]) for G, R in T.CASES] + list(T.extra_cases())
    for name, tuples, sizes in inputs:
        row = []
        for method in METHODS:
            host = C.cophenetic_grouped(tuples, sizes, method)
            dev = C.cophenetic_grouped(tuples, sizes, method, device=0)
            d = 0.0 if np.isnan(host) and np.isnan(dev) else abs(dev - host)
            worst = max(worst, d)
            row.append(f"{method} {d:.2e}")
        say(f"  {name:14s} " + "  ".join(row))
    say(f"  largest: {worst:.3e}")


if __name__ == "__main__":
    want = sys.argv[1:] or ["diffs", "groups", "times"]
    for part in want:
        {"times": times, "groups": groups, "diffs": diffs}[part]()
