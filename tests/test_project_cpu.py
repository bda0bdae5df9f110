"""Projection of new cells onto a fitted basis (ccfindr_amd.project, vbnmf_matrix_project), the parts that need no GPU:
the numpy restatement the GPU tests compare against (tests/util_project.py) is tied to the committed oracle, and the
argument checks of the Python entry and of the C ABI."""
import glob
import os

import numpy as np
import pytest
import scipy.sparse as sp

import util_project as U

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ML_STEP_GOLDENS = sorted(glob.glob(os.path.join(GOLD, "ml_step_*.npz")))


def relerr(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def test_the_ml_step_goldens_are_there():
    assert len(ML_STEP_GOLDENS) == 5


@pytest.mark.parametrize("path", ML_STEP_GOLDENS, ids=[os.path.basename(p)[8:-4] for p in ML_STEP_GOLDENS])
def test_h_half_then_w_half_is_the_oracles_full_step(path):
    """One H half-step of the restatement (R/factorize.R:8-15), then the W half (:17-24) on the new h, against
    oracle.mlnmf_oracle.nmf_update_literal on the ml_step_* goldens' inputs: 1e-14.  Its per-cell likelihoods (:40-49 column by
    column) sum to the oracle's likelihood: 1e-14 of the size of the sums."""
    from oracle import mlnmf_oracle as O
    z = np.load(path)
    X, w0, h0, prior = z["X"], z["w0"], z["h0"], bool(z["prior"])
    ga, gb = (float(v) for v in z["gamma"])
    h1 = U.h_half(X, w0, h0, prior, ga, gb)
    w1 = U.w_half(X, w0, h1, prior, ga, gb)
    want = O.nmf_update_literal(X, w0, h0, prior, ga, gb)
    assert relerr(h1, want["eh"]) <= 1e-14 and relerr(w1, want["ew"]) <= 1e-14
    n, m = X.shape
    for w, h in ((w0, h1), (want["ew"], want["eh"])):
        cells = U.cell_likelihood(X, w, h)
        lk = O.likelihood_literal(X, w, h)
        wh = w @ h
        scale = (np.abs(X * np.log(wh)).sum() + wh.sum()) / n / m
        assert abs(cells.sum() / n / m - lk) <= 1e-14 * scale, (cells.sum() / n / m, lk)


def test_restatement_loop_stops_per_cell():
    """Every cell of the restatement's loop carries its own count and reason: Itmax ends the unconverged ones with 4, a NaN
    start ends its cell with 3 at the first step and leaves the other cells as they are."""
    z = np.load(os.path.join(GOLD, "ml_step_prior_90x140_r5.npz"))
    X, w = z["X"], z["w0"]
    h0 = U.default_start(X, w)
    assert np.allclose((w @ h0).sum(axis=0), X.sum(axis=0), rtol=1e-13)
    full = U.project(X, w, h0, Itmax=400, Tol=1e-5)
    assert set(np.unique(full["reason"])) <= {1, 4} and np.all(full["it"] >= 2)
    cut = U.project(X, w, h0, Itmax=7, Tol=1e-5)
    late = full["it"] > 7
    assert late.any() and np.all(cut["it"][late] == 7) and np.all(cut["reason"][late] == 4)
    assert np.array_equal(cut["it"][~late], full["it"][~late]) and np.all(cut["reason"][~late] == full["reason"][~late])
    bad = h0.copy()
    bad[1, 3] = np.nan
    nan = U.project(X, w, bad, Itmax=7, Tol=1e-5)
    assert nan["reason"][3] == 3 and nan["it"][3] == 1
    keep = np.arange(X.shape[1]) != 3
    assert np.array_equal(nan["h"][:, keep], cut["h"][:, keep]) and np.array_equal(nan["it"][keep], cut["it"][keep])


def test_argument_errors():
    import ccfindr_amd as C
    import importlib
    P = importlib.import_module("ccfindr_amd.project")      # (the package attribute of that name is the function)
    rng = np.random.default_rng(5)
    X = rng.poisson(1.0, size=(12, 9)).astype(np.float64) + np.eye(12, 9)
    W = rng.uniform(size=(12, 3))
    with pytest.raises(ValueError, match="rows"):
        C.project(X[:11], W)                                                   # other genes than the basis
    with pytest.raises(ValueError, match="exceeds"):
        C.project(X[:2], rng.uniform(size=(2, 3)))                             # r > n
    Z = X.copy()
    Z[:, 4] = 0.0
    for mat in (Z, sp.csc_matrix(Z), C.CountMatrix(Z)):
        with pytest.raises(ValueError, match="Input matrix contains empty columns"):
            C.project(mat, W)
    with pytest.raises(ValueError, match="h0"):
        C.project(X, W, h0=np.ones((3, 8)))
    with pytest.raises(ValueError, match="rank"):
        C.project(X, W, rank=4)
    res = C.MLResult(ranks=[2, 3], basis=[W[:, :2], W], coeff=[None, None])
    with pytest.raises(ValueError, match="rank="):
        C.project(X, res)
    with pytest.raises(IndexError):
        C.project(X, res, rank=5)
    M = C.CountMatrix(X)
    shell = C.CountMatrix.shell(M.meta())
    with pytest.raises(ValueError, match="shell"):
        C.project(shell, W)
    H = np.ones((3, 9))
    with pytest.raises(C.VBNMFError) as ei:                                    # the C entry itself: a status and a message
        P.project_columns(shell, W, H, 0, 9)
    assert ei.value.code == 1 and "shell" in str(ei.value)
    for kw in (dict(col_begin=0, col_end=0), dict(col_begin=4, col_end=3), dict(col_begin=0, col_end=10), dict(col_begin=-1, col_end=3)):
        with pytest.raises(C.VBNMFError) as ei:
            P.project_columns(M, W, H, kw["col_begin"], kw["col_end"])
        assert ei.value.code == 1
    with pytest.raises(C.VBNMFError) as ei:
        P.project_columns(M, W, H, 0, 9, Itmax=0)
    assert ei.value.code == 1
    L = C.load()
    h = np.ones((3, 9), order="F")
    args = (1.0, 1.0, 10, 1e-5, 0, None, None, None)
    Wf = np.asfortranarray(W)
    N = C._native
    assert L.vbnmf_matrix_project(M._h, 0, 9, 0, N.dptr(Wf), N.dptr(h), 0, *args) == 1          # r < 1
    assert L.vbnmf_matrix_project(M._h, 0, 9, N.MAX_RANK + 1, N.dptr(Wf), N.dptr(h), 0, *args) == 1
    assert L.vbnmf_matrix_project(M._h, 0, 9, 3, None, N.dptr(h), 0, *args) == 1                # NULL w
    assert L.vbnmf_matrix_project(M._h, 0, 9, 3, N.dptr(Wf), None, 0, *args) == 1               # NULL h
    assert L.vbnmf_matrix_project(None, 0, 9, 3, N.dptr(Wf), N.dptr(h), 0, *args) == 1


def test_no_device_is_a_status():
    import ccfindr_amd as C
    if C.load().vbnmf_device_count() > 0:
        pytest.skip("a GPU is present")
    rng = np.random.default_rng(6)
    X = rng.poisson(1.0, size=(12, 9)).astype(np.float64) + np.eye(12, 9)
    with pytest.raises(C.VBNMFError) as ei:
        C.project(X, rng.uniform(size=(12, 3)))
    assert ei.value.code == 2 and "no CPU fallback" in str(ei.value)


def test_kernel_constants_are_exported():
    """Entries of a cell per pass of the kernel's 256 threads: one lane per entry up to padded rank 32, two up to 64, four above."""
    import ctypes
    import importlib
    import ccfindr_amd as C
    P = importlib.import_module("ccfindr_amd.project")      # (the package attribute of that name is the function)
    L = C.load()
    for r, per in ((1, 256), (10, 256), (32, 256), (33, 128), (64, 128), (65, 64), (128, 64)):
        e = ctypes.c_int32()
        assert L.vbnmf_project_info(r, ctypes.byref(e), None) == 0
        assert e.value == per == P.pass_entries(r)
    assert L.vbnmf_project_info(0, None, None) == 1
    assert P.last_kernel_ms() >= 0.0
