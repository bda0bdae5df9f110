"""Helpers for the tests of merged pieces: small matrices whose (major, block) pairs are cut into 2 ... more than 64 pieces,
the layout view with its row index, and the runs of a layout (host only)."""
import ctypes

import numpy as np

from ccfindr_amd import _native as N

IDLE = 0xFFFFFFFF
# LDS given to the staged block, by rank: both ranks then cut the 3 000 cells of the second matrix into the SAME two blocks
# (an explicit VBNMF_LDS_KB also switches the density rule of the block width off)
LDS_KB = {3: 96, 10: 160}


def set_geometry(monkeypatch, r, merge=None, max_len=16):
    monkeypatch.setenv("VBNMF_MAX_LEN", str(int(max_len)))
    monkeypatch.setenv("VBNMF_EQUAL_BLOCKS", "1")
    monkeypatch.setenv("VBNMF_LDS_KB", str(LDS_KB.get(r, 160)))
    if merge is None:
        monkeypatch.delenv("VBNMF_MERGE_PIECES", raising=False)
    else:
        monkeypatch.setenv("VBNMF_MERGE_PIECES", str(int(merge)))


def _plant(X, rng, gene, cells, count, value):
    cols = rng.choice(cells, size=count, replace=False)
    X[gene, :] = 0.0
    X[gene, cols] = value


def matrix_300x700(wide=False):
    """Sparse counts with a few dense genes and dense cells, and genes whose entry counts give runs of 2, 3, 5 and 8."""
    rng = np.random.default_rng(41)
    X = rng.poisson(0.02, size=(300, 700)).astype(np.float64)
    X[3, :] = 1.0                                       # dense genes: 44 pieces each
    X[7, :] = rng.integers(1, 4, 700)
    X[:, 11] = 2.0                                      # dense cells: 19 pieces each on the cell side
    X[:, 500] = rng.integers(1, 6, 300)
    for gene, count, value in ((20, 24, 1.0), (21, 40, 1.0), (22, 72, 2.0), (23, 120, 1.0), (24, 30, 5.0), (25, 45, 1.0),
                               (26, 75, 3.0), (27, 125, 1.0), (28, 200, 1.0), (29, 333, 2.0)):
        _plant(X, rng, gene, np.arange(20, 480), count, value)
    X[np.arange(300), rng.integers(0, 700, 300)] += 1.0              # no empty gene, no empty cell
    X[rng.integers(0, 300, 700), np.arange(700)] += 1.0
    if wide:
        X = X * 0.37
    return np.asfortranarray(X)


def matrix_64x3000():
    """64 genes x 3 000 cells.  Gene 0 is stored in every cell (188 pieces in one block, 94 in each of two); the cells from
    1 504 on are stored by genes 0, 1 and 2 alone, so the second block's list ends in runs with idle lanes behind them."""
    rng = np.random.default_rng(43)
    X = rng.poisson(0.03, size=(64, 3000)).astype(np.float64)
    X[:, 1504:] = 0.0
    X[0, :] = 1.0
    X[5, :1504] = rng.integers(1, 4, 1504)                          # another dense gene in the first block
    X[:, 77] = 3.0                                                  # dense cells: 4 pieces each on the cell side
    X[:, 901] = rng.integers(1, 3, 64)
    for gene, count, value in ((10, 24, 1.0), (11, 40, 1.0), (12, 72, 1.0), (13, 120, 1.0), (14, 29, 2.0), (15, 45, 1.0),
                               (16, 76, 1.0), (17, 127, 3.0), (18, 250, 1.0), (19, 500, 1.0), (20, 333, 1.0), (21, 39, 1.0)):
        _plant(X, rng, gene, np.arange(100, 1400), count, value)
    X[1, 1504:] = 0.0
    X[2, 1504:] = 0.0
    X[1, 1600 + 7 * np.arange(24)] = 3.0                            # 24 entries each in the second block: two pieces of 12
    X[2, 1700 + 11 * np.arange(24)] = 3.0
    X[np.arange(3, 64), rng.integers(0, 1504, 61)] += 1.0
    X[rng.integers(3, 64, 1504), np.arange(1504)] += 1.0
    return np.asfortranarray(X)


def layout_view(M, side, r):
    """The layout of the whole matrix as numpy copies, row index included."""
    L = N.load()
    h, v = ctypes.c_void_p(), N.LayoutView()
    N.check(L.vbnmf_layout_build(M._h, 0, M.shape[1], side, r, ctypes.byref(h), ctypes.byref(v)))
    try:
        arr = lambda p, cnt: np.ctypeslib.as_array(p, shape=(cnt,)).copy() if cnt else np.zeros(0, dtype=np.int64)
        out = {k: getattr(v, k) for k in ("side", "wide", "n_major", "n_minor", "n_blocks", "max_len", "n_tasks", "n_slices", "n_rows", "merge")}
        out["task_major"] = arr(v.task_major, v.n_slices * 64)
        out["slice_block"] = arr(v.slice_block, v.n_slices)
        out["block_start"] = arr(v.block_start, v.n_blocks + 1)
        out["inv_ptr"] = arr(v.inv_ptr, v.n_major + 1)
        out["inv_task"] = arr(v.inv_task, v.n_tasks)
        out["row_ptr"] = arr(v.row_ptr, v.n_major + 1)
        out["row_task"] = arr(v.row_task, v.n_rows)
    finally:
        L.vbnmf_layout_destroy(h)
    return out


def runs_of(view):
    """The runs of a layout: (slice, first lane, length, idle lanes behind the slice's last run or 0) per run."""
    tm = view["task_major"].reshape(-1, 64)
    out = []
    for s in range(tm.shape[0]):
        lane = 0
        while lane < 64:
            if tm[s, lane] == IDLE:
                lane += 1
                continue
            end = lane + 1
            while end < 64 and tm[s, end] == tm[s, lane]:
                end += 1
            idle_behind = 64 - end if (end == 64 or (tm[s, end:] == IDLE).all()) else 0
            out.append((s, lane, end - lane, idle_behind))
            lane = end
    return out


def run_shapes(view):
    """Names of the run shapes the GPU tests must meet, as found in this layout."""
    found = set()
    runs = runs_of(view)
    tm = view["task_major"].reshape(-1, 64)
    for s, lane, length, idle_behind in runs:
        if length in (1, 2, 3, 5, 8):
            found.add(f"len{length}")
        if length == 64:
            found.add("len64")
        if lane <= 15 and lane + length > 16:
            found.add("cross15_16")
        if lane <= 31 and lane + length > 32:
            found.add("cross31_32")
        if length >= 2 and idle_behind > 0:
            found.add("idle_tail_behind_run")
    # a run that ends at lane 63 while another slice of the same block begins with the same major: one pair, two rows
    first = {}
    for s in range(tm.shape[0]):
        if tm[s, 0] != IDLE:
            first.setdefault((int(view["slice_block"][s]), int(tm[s, 0])), []).append(s)
    for s in range(tm.shape[0]):
        if tm[s, 63] != IDLE and any(t != s for t in first.get((int(view["slice_block"][s]), int(tm[s, 63])), [])):
            found.add("straddle")
    return found


ALL_SHAPES = {"len1", "len2", "len3", "len5", "len8", "len64", "cross15_16", "cross31_32", "straddle", "idle_tail_behind_run"}
