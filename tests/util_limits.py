"""Cases that push the sweep and update kernels past their per-workgroup limits on matrices small enough for a unit test.

With the default geometry (one workgroup per CU, 256 update blocks) a workgroup's share outgrows the fixed on-chip tables
only on matrices of several hundred thousand cells.  The layout switches (VBNMF_LDS_KB, VBNMF_NWG, VBNMF_MAX_LEN) and the
``grid`` argument of VBEngine reach the same code on 700 x 700:

  * LIMIT_CASES: more minor blocks than workgroups, so pack_blocks (csrc/layout.cpp) makes every block one segment, and
    tasks of four entries, so every segment's slice list is longer than the kLdsEvSlots = 128 evidence slots of the sweep
    (csrc/kernels.h, sweep_side: the ``c0 += kLdsEvSlots`` loop) and is pulled in two or three chunks;
  * GATHER_CASES: update blocks whose stretch of the inverse index is beyond what k_update / k_ml_update stage in LDS
    (kStagePtr = 2 048 majors, kStageIds = 14 336 task ids), so the gather reads its ids from global memory (task_sum).

tests/test_limits_cpu.py proves on the host that every case is what it claims; tests/test_gpu_limits.py runs them."""
import os
import re
from collections import namedtuple

import numpy as np

from test_gpu_batch_oracle import _sparse_counts, update_table_stride          # noqa: F401  (shared with the GPU tests)



def _kernel_constant(name):
    """``constexpr int name = value;`` of csrc/kernels.h: the limits are the kernels' own, so a case that no longer crosses a
    limit after the limit has moved fails tests/test_limits_cpu.py."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ccfindr_amd", "csrc", "kernels.h")
    with open(path) as f:
        found = re.findall(r"^constexpr int %s = (\d+);" % name, f.read(), flags=re.M)
    assert len(found) == 1, (name, found)
    return int(found[0])


LDS_EV_SLOTS = _kernel_constant("kLdsEvSlots")         # 128: evidence slots of the sweep, slices per chunk of a segment's list
STAGE_IDS = _kernel_constant("kStageIds")              # 14 336: task ids an update block stages in LDS
STAGE_PTR = _kernel_constant("kStagePtr")              # 2 048: ... and the pointers of its majors (fewer than this many majors)
HY = {"aw": 1.2, "bw": 0.9, "ah": 0.8, "bh": 1.5}

# kind: "counts" (packed layout), "noninteger" (wide layout), "split" (counts beyond the packed range), "ones_twos" (the
# deferred-logarithm stretches).  chunks: how many chunks the longest list of at least one side is pulled in.
LimitCase = namedtuple("LimitCase", "n m lam r kind lds_kb nwg max_len chunks")

LIMIT_CASES = [
    LimitCase(700, 700, 0.9, 3, "counts", 8, 2, 4, 2),             # padded rank below 8: neither side pulls from both ends
    LimitCase(700, 700, 0.9, 10, "counts", 16, 3, 4, 2),           # 8 to 15: the gene side only
    LimitCase(700, 700, 0.9, 10, "noninteger", 16, 3, 4, 2),       # wide layout (value + index streams)
    LimitCase(700, 700, 0.9, 30, "counts", 48, 2, 4, 3),           # 16 and above: both sides; the one-row-buffer loop
    LimitCase(700, 700, 0.9, 40, "counts", 64, 2, 4, 3),           # two lanes per task
    LimitCase(700, 700, 0.9, 80, "counts", 128, 1, 4, 3),          # four lanes per task
    LimitCase(700, 700, 0.9, 10, "split", 16, 3, 4, 2),            # counts of 16 383, 16 384 and 100 000
    LimitCase(700, 700, 0.9, 10, "ones_twos", 16, 3, 4, 2),        # mostly ones and twos
    # denser: three chunks at rank 10, and each half of the cells (two partitions) still beyond the slots on both sides
    LimitCase(700, 700, 1.5, 10, "counts", 16, 3, 4, 3),
]


def case_id(c):
    return f"r{c.r}_{c.kind}{'' if c.lam == 0.9 else '_mean%g' % c.lam}_lds{c.lds_kb}_nwg{c.nwg}"


LIMIT_IDS = [case_id(c) for c in LIMIT_CASES]


def find_case(r, kind, lam=0.9):
    return next(c for c in LIMIT_CASES if c.r == r and c.kind == kind and c.lam == lam)


def _repair(X, rng):
    n, m = X.shape
    X[np.arange(n), rng.integers(0, m, n)] += 1.0               # no empty gene
    X[rng.integers(0, n, m), np.arange(m)] += 1.0               # no empty cell
    return X


def limit_matrix(n, m, lam, kind, seed):
    """Poisson(lam) counts without an empty row or column, as counts() of tests/test_gpu_forced_geometry.py."""
    rng = np.random.default_rng(seed)
    if kind == "ones_twos":
        X = ((rng.random((n, m)) < 0.6) * (1 + (rng.random((n, m)) < 0.3))).astype(np.float64)
    else:
        X = rng.poisson(lam, size=(n, m)).astype(np.float64)
    X = _repair(X, rng)
    if kind == "noninteger":
        X = X * rng.uniform(0.5, 1.5, size=(1, m))
    elif kind == "split":                                       # the last packed count, the first split one, a count of seven pieces
        X[n // 3, m // 2] = 16383.0
        X[n // 2, m // 3] = 16384.0
        X[n // 5, m // 7] = 100000.0
    return np.asfortranarray(X)


_matrices = {}


def case_matrix(c):
    """The case's matrix (read-only, cut once per process)."""
    key = (c.n, c.m, c.lam, c.kind, c.r)
    if key not in _matrices:
        X = limit_matrix(c.n, c.m, c.lam, c.kind, seed=1000 + c.r + int(100 * c.lam))
        X.setflags(write=False)
        _matrices[key] = X
    return _matrices[key]


def set_switches(monkeypatch, c):
    monkeypatch.setenv("VBNMF_LDS_KB", str(c.lds_kb))
    monkeypatch.setenv("VBNMF_NWG", str(c.nwg))
    monkeypatch.setenv("VBNMF_MAX_LEN", str(c.max_len))


def segment_lengths(view):
    return np.diff(view["seg_ptr"])


# ---- the update kernels' unstaged gather -------------------------------------------------------------------------------
# name -> (rank, grid, VBNMF_MAX_LEN or None)
GatherCase = namedtuple("GatherCase", "name r grid max_len")
GATHER_CASES = [
    GatherCase("A", 3, (8, 1), 4), GatherCase("A", 10, (8, 1), 4),      # one block: < 2 048 majors, ~74 000 ids
    GatherCase("B", 3, (8, 4), 4),                                       # staged and unstaged blocks in one launch
    GatherCase("C", 3, (8, 4), None),                                    # 2 250 cell-side majors per block
]
GATHER_IDS = [f"{g.name}_r{g.r}" for g in GATHER_CASES]


def gather_matrix(name):
    """A, B: dense arrays; C: scipy CSC."""
    if name not in _matrices:
        if name == "A":
            X = limit_matrix(700, 700, 0.9, "counts", seed=51)
        elif name == "B":
            rng = np.random.default_rng(52)
            X = np.concatenate([rng.poisson(3.0, size=(175, 700)), rng.poisson(0.2, size=(525, 700))]).astype(np.float64)
            X = np.asfortranarray(_repair(X, rng))
        else:
            X = _sparse_counts(400, 9000, 2, 53)
        if not hasattr(X, "tocsc"):
            X.setflags(write=False)
        _matrices[name] = X
    return _matrices[name]


def set_gather_switches(monkeypatch, g):
    """The host-side view of the layouts an engine of grid g.grid cuts (the engine passes its own n_wg)."""
    monkeypatch.setenv("VBNMF_NWG", str(g.grid[0]))
    if g.max_len:
        monkeypatch.setenv("VBNMF_MAX_LEN", str(g.max_len))


def block_split(view, ub):
    """k_update's split of a side's majors over ub blocks: (majors, task ids) of every block."""
    nmaj, ptr = int(view["n_major"]), view["inv_ptr"]
    per0 = (nmaj + ub - 1) // ub
    out = []
    for b in range(ub):
        m0, m1 = min(nmaj, b * per0), min(nmaj, (b + 1) * per0)
        out.append((m1 - m0, int(ptr[m1] - ptr[m0])))
    return out


def block_is_staged(majors, ids):
    """The kernel's per-block decision (k_update, ml_update_body)."""
    return 0 < majors < STAGE_PTR and ids <= STAGE_IDS
