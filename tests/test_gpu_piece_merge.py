"""GPU: the sweep adds the pieces of a cut (major, block) pair inside the wave and stores one partial row per run
(csrc/kernels.h: sweep_side, SweepSide::merge; csrc/layout.cpp: cut_tasks, build_rows).

Small matrices under VBNMF_MAX_LEN=16, so that pairs are cut into 2 ... 188 pieces and the layouts hold runs of every shape
the segmented sum has to get right: lengths 1, 2, 3, 5, 8 and 64, runs across lanes 15/16 and 31/32, a pair that straddles two
slices, idle lanes behind a slice's last run.  The shapes are asserted on the host through the layout view: a layout that
lacks one fails the test.  Checkers: oracle/vbnmf_oracle (reference src/vbnmf_update.cpp:33-90), oracle/mlnmf_oracle
(reference R/factorize.R:2-27, :40-49), scipy's sparse product; tolerances 1e-12 (factors) and 1e-10 (evidence) as
everywhere; merging on against off 1e-13 (the same sums in another order)."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

from util_piece_merge import ALL_SHAPES, LDS_KB, layout_view, matrix_300x700, matrix_64x3000, run_shapes

pytestmark = pytest.mark.gpu
HY = {"aw": 1.1, "bw": 0.9, "ah": 0.8, "bh": 1.3}
STATE = ("lw", "lh", "ew", "eh", "dw", "dh")
# (matrix, rank): the last one is the wide (non-integer) layout
CASES = [("300x700", 3), ("300x700", 10), ("64x3000", 3), ("64x3000", 10), ("300x700w", 10)]
# 700 cells hold 44 pieces of a gene at most: no run of 64 lanes on the smaller matrix
REQUIRED = {"300x700": ALL_SHAPES - {"len64"}, "300x700w": ALL_SHAPES - {"len64"}, "64x3000": ALL_SHAPES}


def relerr(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


@functools.lru_cache(maxsize=None)
def matrix(name):
    X = {"300x700": matrix_300x700, "64x3000": matrix_64x3000, "300x700w": lambda: matrix_300x700(wide=True)}[name]()
    X.setflags(write=False)
    return X


class geometry:
    """The environment the layouts of a case are cut under (read when an engine or a view cuts them)."""

    def __init__(self, r, merge=None):
        self.env = {"VBNMF_MAX_LEN": "16", "VBNMF_EQUAL_BLOCKS": "1", "VBNMF_LDS_KB": str(LDS_KB.get(r, 160)),
                    "VBNMF_MERGE_PIECES": None if merge is None else str(int(merge))}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        for k, v in self.env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def state(name, r):
    from ccfindr_amd import synth
    n, m = matrix(name).shape
    return synth.random_state(n, m, r, HY, seed=17 + r)


@functools.lru_cache(maxsize=None)
def vb_reference(name, r):
    from oracle import vbnmf_oracle as O
    import ccfindr_amd as C
    return O.update_dense(np.asfortranarray(matrix(name)), state(name, r), HY, C.EPS)


@pytest.mark.parametrize("name,r", CASES)
def test_the_layouts_hold_every_run_shape(name, r):
    import ccfindr_amd as C
    with geometry(r):
        M = C.CountMatrix(np.asfortranarray(matrix(name)))
        found = set()
        for side in (0, 1):
            v = layout_view(M, side, r)
            assert v["merge"] == 1 and v["wide"] == (1 if name.endswith("w") else 0)
            found |= run_shapes(v)
        M.close()
    assert REQUIRED[name] <= found, sorted(REQUIRED[name] - found)


@pytest.mark.parametrize("name,r", CASES)
def test_vb_step_against_the_oracle_merged_and_unmerged(name, r):
    import ccfindr_amd as C
    X = np.asfortranarray(matrix(name))
    wh, want = state(name, r), vb_reference(name, r)
    got = {}
    for merge in (1, 0, 1):
        with geometry(r, merge):
            out = C.vbnmf_update(X, wh, HY, C.EPS)
        for k in STATE:
            assert relerr(out[k], want[k]) <= 1e-12, (merge, k, relerr(out[k], want[k]))
        assert abs(out["lkh"] / want["lkh"] - 1) <= 1e-10, (merge, out["lkh"], want["lkh"])
        if merge in got:                                              # a second run of the same form: bit for bit
            for k in STATE:
                assert np.array_equal(out[k], got[merge][k]), k
            assert out["lkh"] == got[merge]["lkh"]
        got[merge] = out
    for k in STATE:
        assert relerr(got[1][k], got[0][k]) <= 1e-13, (k, relerr(got[1][k], got[0][k]))
    assert abs(got[1]["lkh"] / got[0]["lkh"] - 1) <= 1e-13


@pytest.mark.parametrize("name,r", CASES)
def test_ml_step_and_sparse_product(name, r):
    import ccfindr_amd as C
    from oracle import mlnmf_oracle as OM
    X = np.asfortranarray(matrix(name))
    n, m = X.shape
    rng = np.random.default_rng(5 + r)
    w0, h0 = rng.uniform(size=(n, r)), rng.uniform(size=(r, m))
    want = OM.nmf_update_literal(X, w0, h0)
    want_lk = OM.likelihood_literal(X, want["ew"], want["eh"])
    B, W = rng.standard_normal((r, m)), rng.standard_normal((n, r))
    S = sp.csr_matrix(X)
    want_xb, want_wx = S @ B.T, (S.T @ W).T
    outs = {}
    for merge in (1, 0):
        with geometry(r, merge):
            got = C.nmf_update(X, w0, h0)
            Mx = C.CountMatrix(X)
            eng = C.VBEngine(Mx, r)
            xb, wx = eng.spmm(B), eng.spmm(W, transpose=True)
            eng.close(); Mx.close()
        for k in ("ew", "eh"):
            assert relerr(got[k], want[k]) <= 1e-12, (merge, k, relerr(got[k], want[k]))
        assert abs(got["lk"] / want_lk - 1) <= 1e-10, (merge, got["lk"], want_lk)
        assert np.max(np.abs(xb - want_xb)) <= 1e-12 * np.max(np.abs(want_xb))
        assert np.max(np.abs(wx - want_wx)) <= 1e-12 * np.max(np.abs(want_wx))
        outs[merge] = (got, xb, wx)
    for k in ("ew", "eh"):
        assert relerr(outs[1][0][k], outs[0][0][k]) <= 1e-13, k
    assert abs(outs[1][0]["lk"] / outs[0][0]["lk"] - 1) <= 1e-13


@pytest.mark.parametrize("name,r", CASES)
def test_group_of_two_partitions_and_batch_of_four(name, r):
    """As tests/test_gpu_partition_loop.py and tests/test_gpu_batch_run.py hold them to the single engine: the local group to
    1e-10 (history) / 1e-9 (state), every engine of the batch bit for bit."""
    import ccfindr_amd as C
    from ccfindr_amd import synth
    from ccfindr_amd.parallel import cell_partition
    X = np.asfortranarray(matrix(name))
    n, m = X.shape
    kw = dict(Itmax=12, Tol=0.0, n0=4, dn=1, flags=(True,) * 4, history=True)
    with geometry(r):
        M = C.CountMatrix(X)
        wh = state(name, r)
        whole = C.VBEngine(M, r)
        whole.set_state(wh["lw"], wh["lh"], wh["eh"])
        want = whole.run(HY, **kw)
        ref = whole.get_state()
        cuts = cell_partition(m, 2)
        comm = C.Communicator.local(2)
        parts = [C.VBEngine(M, r, cols=c, m_global=m) for c in cuts]
        for p, (b, e) in zip(parts, cuts):
            p.attach_comm(comm)
            p.set_state(wh["lw"], wh["lh"][:, b:e], wh["eh"][:, b:e])
        comm.state_finish()
        got = comm.run(HY, **kw)
        assert got["it"] == want["it"] == 12
        assert relerr(got["history"], want["history"]) <= 1e-10
        st = [p.get_state() for p in parts]
        assert np.array_equal(st[0]["ew"], st[1]["ew"]) and relerr(st[0]["ew"], ref["ew"]) <= 1e-9
        assert relerr(np.concatenate([q["eh"] for q in st], axis=1), ref["eh"]) <= 1e-9
        for e in parts + [whole]:
            e.close()
        comm.close()
        # a batch of four engines: each its stand-alone run, bit for bit
        whs = [synth.random_state(n, m, r, HY, seed=30 + b) for b in range(4)]
        alone = []
        for b in range(4):
            eng = C.VBEngine(M, r)
            eng.set_state(whs[b]["lw"], whs[b]["lh"], whs[b]["eh"])
            alone.append((eng.run(HY, **kw), eng.get_state()))
            eng.close()
        engs = [C.VBEngine(M, r) for _ in range(4)]
        for eng, w in zip(engs, whs):
            eng.set_state(w["lw"], w["lh"], w["eh"])
        outs = C.run_batch(engs, [HY] * 4, **kw)
        for b in range(4):
            assert outs[b]["it"] == alone[b][0]["it"] and outs[b]["lkh"] == alone[b][0]["lkh"]
            assert np.array_equal(outs[b]["history"], alone[b][0]["history"], equal_nan=True)
            stb = engs[b].get_state()
            for k in stb:
                assert np.array_equal(stb[k], alone[b][1][k]), (b, k)
        for eng in engs:
            eng.close()
        M.close()


def test_rank_40_keeps_one_row_per_task():
    """Ranks above 32 share a task between lanes: their layouts are not merged and their sweep is the one it was."""
    import ccfindr_amd as C
    from ccfindr_amd import synth
    from oracle import vbnmf_oracle as O
    X = np.asfortranarray(matrix("300x700"))
    n, m = X.shape
    r = 40
    wh = synth.random_state(n, m, r, HY, seed=3)
    want = O.update_dense(X, wh, HY, C.EPS)
    outs = []
    for merge in (None, 0):
        with geometry(r, merge):
            M = C.CountMatrix(X)
            v = layout_view(M, 0, r)
            assert v["merge"] == 0 and np.array_equal(v["row_task"], v["inv_task"])
            M.close()
            outs.append(C.vbnmf_update(X, wh, HY, C.EPS))
    for k in STATE:
        assert relerr(outs[0][k], want[k]) <= 1e-12, k
        assert np.array_equal(outs[0][k], outs[1][k]), k            # the switch changes nothing at this rank
    assert abs(outs[0]["lkh"] / want["lkh"] - 1) <= 1e-10 and outs[0]["lkh"] == outs[1]["lkh"]
