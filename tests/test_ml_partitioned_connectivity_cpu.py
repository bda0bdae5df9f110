"""The connectivity stopping rule (reference R/factorize.R:198-208) on cell-partitioned engines, on a machine without a GPU:
vbnmf_group_ml_run_connectivity's C ABI (exported, bound, declared, refusing bad arguments before any device is touched),
factorize()'s dispatch to an engine's ``ml_run_connectivity``, and ``CellPartitionedEngine.cluster_ids`` /
``ml_run_connectivity`` / ``ml_run`` over a numpy partition engine in a gloo world of two."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAME = "vbnmf_group_ml_run_connectivity"


def _header():
    return open(os.path.join(ROOT, "include", "vbnmf.h")).read()


def test_group_entry_is_exported_bound_and_declared_with_13_arguments():
    from ccfindr_amd import _native as N
    L = N.load()
    assert hasattr(L, NAME)
    restype, argtypes = N.SIGNATURES[NAME]
    assert restype is ctypes.c_int and len(argtypes) == 13
    assert getattr(L, NAME).argtypes == argtypes
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, text)
    assert m, f"{NAME} is not declared in include/vbnmf.h"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == 13


def test_header_cites_the_reference_rule():
    text = _header()
    comment = text[:text.index("int " + NAME)].rsplit("/*", 1)[1]
    assert "R/factorize.R" in comment and "198-208" in comment


def test_bad_arguments_are_a_status_without_a_device():
    from ccfindr_amd import _native as N
    L = N.load()
    it, reason, lk = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double()
    out = (ctypes.byref(it), ctypes.byref(lk), ctypes.byref(reason), None, 0, None, 0)
    rc = L.vbnmf_group_ml_run_connectivity(None, 0, 1.0, 1.0, 10, 5, *out)
    assert rc == N.ERR_BAD_ARG and b"NULL" in L.vbnmf_last_error()
    # max_it and ncnn_step are checked before the handle is read: any non-NULL pointer will do
    bogus = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))
    for comm in (None, bogus):
        for max_it, ncnn in ((0, 5), (10, 0), (-1, -1)):
            rc = L.vbnmf_group_ml_run_connectivity(comm, 0, 1.0, 1.0, max_it, ncnn, *out)
            assert rc == N.ERR_BAD_ARG and b"ncnn_step" in L.vbnmf_last_error()


class _Recorder:
    """A stand-in engine over the oracle's step that records which loop factorize() drives."""

    def __init__(self, X, rank, log):
        from tests.fake_ml_engine import OracleMLEngine
        self._e, self.log = OracleMLEngine(X, rank), log

    def __getattr__(self, name):
        return getattr(self._e, name)

    def _loop(self, Itmax, ncnn_step):
        from ccfindr_amd.factorize import cluster_ids, connectivity_changes
        cid0, zstep, lk, it = None, 0, np.nan, 0
        for it in range(1, Itmax + 1):
            lk = self._e.ml_step()
            cid = cluster_ids(self._e.ml_get_state(("eh",))["eh"])
            zstep = zstep + 1 if it > 1 and connectivity_changes(cid0, cid, self._e.rank) == 0 else 0
            cid0 = cid
            if zstep == ncnn_step:
                break
        return {"it": it, "lk": lk, "reason": 2 if zstep == ncnn_step else 4}


class _WithOwnLoop(_Recorder):
    def ml_run(self, **kw):
        raise AssertionError("an engine with ml_run_connectivity is driven through it")

    def ml_run_connectivity(self, **kw):
        self.log.append(("ml_run_connectivity", dict(kw)))
        return self._loop(kw["Itmax"], kw["ncnn_step"])


class _MlRunOnly(_Recorder):
    def ml_run(self, **kw):
        self.log.append(("ml_run", dict(kw)))
        return self._loop(kw["Itmax"], kw.get("ncnn_step", kw["Itmax"] + 1))      # (the likelihood rule with Tol = 0: to Itmax)


def test_factorize_dispatches_the_connectivity_loop():
    from ccfindr_amd.factorize import factorize
    rng = np.random.default_rng(3)
    X = rng.poisson(0.9, size=(30, 40)).astype(np.float64)
    X[np.arange(30), rng.integers(0, 40, 30)] += 1
    X[rng.integers(0, 30, 40), np.arange(40)] += 1
    kw = dict(ranks=[2], nrun=2, verbose=0, seed=4, Itmax=60, ncnn_step=3, criterion="connectivity")
    own, plain, stepped = [], [], []
    a = factorize(X, engine_factory=lambda M, r: _WithOwnLoop(M.host, r, own), **kw)
    b = factorize(X, engine_factory=lambda M, r: _MlRunOnly(M.host, r, plain), **kw)
    c = factorize(X, engine_factory=lambda M, r: _WithOwnLoop(M.host, r, stepped), device_loop=False, **kw)
    assert [name for name, _ in own] == ["ml_run_connectivity"] * 2
    assert all(k == {"Itmax": 60, "ncnn_step": 3} for _, k in own)
    assert [name for name, _ in plain] == ["ml_run"] * 2
    assert all(k["criterion"] == "connectivity" and k["ncnn_step"] == 3 and k["Itmax"] == 60 for _, k in plain)
    assert stepped == []                                           # device_loop=False: the host rule, neither loop
    assert a.nsteps == b.nsteps == c.nsteps and np.array_equal(a.basis[0], b.basis[0])
    # the likelihood rule goes through ml_run whatever else the engine has
    lik = []
    factorize(X, engine_factory=lambda M, r: _MlRunOnly(M.host, r, lik), ranks=[2], nrun=1, verbose=0, seed=4, Itmax=5, Tol=0.0)
    assert [name for name, _ in lik] == ["ml_run"] and "criterion" not in lik[0][1]


def _problem():
    sys.path.insert(0, HERE)
    from test_ml_partition_cpu import counts
    n, m, r = 30, 47, 3
    rng = np.random.default_rng(3)
    return counts(n, m, 0.8, seed=17), n, m, r, rng.uniform(size=(n, r)), rng.uniform(size=(r, m))


def _worker(rank, world, port, q):
    import torch.distributed as dist
    sys.path.insert(0, ROOT); sys.path.insert(0, HERE)
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from test_ml_partition_cpu import NumpyMLPartition
        from test_ml_partitioned_connectivity_cpu import _problem
        from ccfindr_amd import parallel
        X, n, m, r, w, h = _problem()
        cols = parallel.cell_partition(m, world)[rank]
        part = NumpyMLPartition(X, r, cols=cols, m_global=m)
        assert not hasattr(part, "cluster_ids")
        eng = parallel.CellPartitionedEngine(X, r, engine=part)
        eng.ml_set_state(w, h)
        for _ in range(3):
            eng.ml_step()
        ids = eng.cluster_ids()
        # a column of NaNs in each block (label 0) and an exact tie (the first maximum wins), planted in the local state
        part.h[:, 1] = np.nan
        part.h[:, 2] = [0.25, 0.5, 0.5]
        part.h[:, 3] = [np.nan, 0.125, 0.125]
        planted = eng.cluster_ids()
        errors = []
        for call in (lambda: eng.ml_run_connectivity(Itmax=3, ncnn_step=2), lambda: eng.ml_run(criterion="connectivity")):
            try:
                call()
                errors.append(None)
            except (ValueError, RuntimeError) as exc:
                errors.append(type(exc).__name__)
        q.put((rank, ids, planted, errors, cols))
    finally:
        dist.destroy_process_group()


def test_cell_partitioned_engine_cluster_ids_and_refusals_world2():
    import torch.multiprocessing as mp
    from oracle import mlnmf_oracle as O
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 36300 + (os.getpid() % 1500)
    procs = [ctx.Process(target=_worker, args=(k, 2, port, q)) for k in range(2)]
    for p in procs:
        p.start()
    try:
        outs = sorted([q.get(timeout=240) for _ in procs], key=lambda o: o[0])
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.terminate()
    assert all(p.exitcode == 0 for p in procs)
    X, n, m, r, w, h = _problem()
    want = {"ew": w, "eh": h}
    for _ in range(3):
        want = O.nmf_update_literal(X, want["ew"], want["eh"])
    top = np.sort(want["eh"], axis=0)[-2:]
    assert np.min((top[1] - top[0]) / top[1]) >= 1e-6                # no label of the oracle's state sits on a near-tie
    labels = (np.argmax(want["eh"], axis=0) + 1).astype(np.int32)
    planted = labels.copy()
    for rank, ids, got, errors, (cb, ce) in outs:
        planted[cb + 1], planted[cb + 2], planted[cb + 3] = 0, 2, 2
    for rank, ids, got, errors, cols in outs:
        assert ids.dtype == np.int32 and ids.shape == (m,)            # all m_global cells on every process
        assert np.array_equal(ids, labels)
        assert np.array_equal(got, planted)
        assert errors == ["RuntimeError", "ValueError"]
