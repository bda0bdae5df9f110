"""The CPU yardstick of the connectivity stopping rule (reference R/factorize.R:194-213 under criterion = 'connectivity'):
oracle.mlnmf_oracle.nmf_update_literal iterated from a given start, labels argmax + 1, nchange from the contingency
arithmetic of ccfindr_amd.factorize.connectivity_changes, the stop at zstep == ncnn_step.  Shared by the tests of the
cell-partitioned device loop; every trajectory is computed once per process."""
import functools

import numpy as np


def counts(n, m, lam, seed):
    rng = np.random.default_rng(seed)
    X = rng.poisson(lam, size=(n, m)).astype(np.float64)
    X[np.arange(n), rng.integers(0, m, n)] += 1      # no empty rows
    X[rng.integers(0, n, m), np.arange(m)] += 1      # no empty columns
    return np.asfortranarray(X)


def uniform_state(n, m, r, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(size=(n, r)), rng.uniform(size=(r, m))


# n, m, r, lam, X seed, state seed, ncnn_step -- every one stops before Itmax = 400; the step of the stop and the smallest
# relative gap between a cell's two largest h entries over the trajectory are asserted where the case is used
TABLE = [
    (120, 260, 4, 0.3, 7, 2, 5),         # stops at 97, gap 2.9e-5
    (64, 96, 10, 0.7, 5, 3, 5),          # 59, 2.7e-5
    (40, 90, 20, 0.7, 9, 4, 4),          # 55, 7.9e-5: the 512-thread sweep
    (50, 120, 40, 0.7, 1, 8, 3),         # 89, 1.1e-5: two lanes per task, the table past the LDS form's rank 32
    (37, 53, 3, 0.7, 93, 11, 6),         # 33, 1.3e-5: 53 does not divide
]
STOPS = [97, 59, 55, 89, 33]
# a 2-cell partition next to a wide one (test_gpu_ml_partitioned.py: CASES): stops at 104, gap 1.2e-4 (measured on the CPU;
# the widest gap among X seeds 1-8 x state seeds 1-8)
UNEVEN = (64, 300, 4, 0.7, 7, 4, 5)
MIN_GAP = 1e-6          # three orders above the 1e-9 the partitioned state is held to: no label sits on a near-tie


def oracle_loop(X, w, h, ncnn_step, itmax=400):
    """The host loop, literally, from the pair (w, h) -> dict(it, reason, changes, history, gap, ew, eh, labels)."""
    from oracle import mlnmf_oracle as O
    from ccfindr_amd.factorize import connectivity_changes
    m, r = X.shape[1], w.shape[1]
    cur, cid0, zstep, reason = {"ew": w, "eh": h}, None, 0, 4
    changes, history, gap = [], [], np.inf
    for it in range(1, itmax + 1):
        cur = O.nmf_update_literal(X, cur["ew"], cur["eh"])
        history.append(O.likelihood_literal(X, cur["ew"], cur["eh"]))
        top = np.sort(cur["eh"], axis=0)[-2:]
        gap = min(gap, float(np.min((top[1] - top[0]) / top[1])))
        cid = np.argmax(cur["eh"], axis=0)
        nchange = m * (m - 1) // 2 if it == 1 else connectivity_changes(cid0, cid, r)      # :200-202
        changes.append(nchange)
        zstep = zstep + 1 if nchange == 0 else 0                                           # :206-207
        cid0 = cid
        if zstep == ncnn_step:                                                             # :208
            reason = 2
            break
    return {"it": it, "reason": reason, "changes": np.asarray(changes, dtype=np.int64), "history": np.asarray(history),
            "gap": gap, "ew": cur["ew"], "eh": cur["eh"], "labels": (cid + 1).astype(np.int32)}


@functools.lru_cache(maxsize=None)
def oracle_run(n, m, r, lam, xseed, sseed, ncnn_step, itmax=400):
    """A case of TABLE (or UNEVEN) -> oracle_loop's dictionary plus the inputs X, w, h; computed once per process."""
    X = counts(n, m, lam, xseed)
    w, h = uniform_state(n, m, r, sseed)
    return dict(oracle_loop(X, w, h, ncnn_step, itmax), X=X, w=w, h=h)
