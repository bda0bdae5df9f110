"""ML-NMF with the cells partitioned, on the CPU: the algebra of the partitioned step restated in numpy
and held to oracle/mlnmf_oracle.py, and the ``CellPartitionedEngine.ml_*`` surface over that numpy engine in a gloo world of 2.

The step (reference R/factorize.R:2-27, :40-49), partition p owning the cells J_p, its columns of h and a full copy of w:
  1  h_p <- h_p .* (t(w) %*% (x_p / (w h_p))) / colSums(w)                  local
  2  S_p = (x_p / (w h_p_new)) %*% t(h_p_new) ; rowSums(h_p_new)            local
  3  exchange 1: [S | rowSums(h_new)] summed over the partitions
  4  w <- w .* S / rowSums(h_new)                                            replicated
  5  data_p = sum x_p log(w_new h_p_new) ; xlx_p = sum_{x>0}(-x log x + x)   local
  6  exchange 2: [data | xlx] summed over the partitions
  7  lk = ((data - sum_k colSum(w)_k rowSum(h)_k) + xlx) / n / m_global
Tolerances: the project's single-step ones -- factors 1e-12 max-rel, likelihood 1e-10."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EPS = float(np.finfo(np.float64).eps)


def relerr(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def counts(n, m, lam, seed):
    rng = np.random.default_rng(seed)
    X = rng.poisson(lam, size=(n, m)).astype(np.float64)
    X[np.arange(n), rng.integers(0, m, n)] += 1
    X[rng.integers(0, n, m), np.arange(m)] += 1
    return X


class NumpyMLPartition:
    """One partition's engine in numpy, speaking the host-stepped protocol of include/vbnmf.h: the reduce buffer is
    [S (n x r, gene-major) | rowSums(h) (r) | 0 0 | data | xlx], and a step is ml_step_local / sum / ml_step_local / sum of the
    tail / ml_step_finish."""

    def __init__(self, X, rank, cols=None, m_global=None):
        X = np.asarray(X.host if hasattr(X, "host") else X, dtype=np.float64)
        cb, ce = cols if cols is not None else (0, X.shape[1])
        self.X = X[:, cb:ce]
        self.n, self.m = self.X.shape
        self.m_global = int(m_global if m_global is not None else X.shape[1])
        self.rank = int(rank)
        self.red = np.zeros(self.n * self.rank + self.rank + 4)
        z = self.X[self.X > 0]
        self.xlx = float(np.sum(-z * np.log(z) + z))
        self.phase, self.pending, self.lk = 0, False, np.nan

    def reduce_tensor(self):
        import torch
        return torch.from_numpy(self.red)                    # aliases self.red

    def _tail(self):
        nr, r = self.n * self.rank, self.rank
        with np.errstate(divide="ignore", invalid="ignore"):
            logs = np.where(self.X > 0, self.X * np.log(self.w @ self.h), 0.0)
        self.red[nr:nr + r] = self.h.sum(axis=1)
        self.red[nr + r:nr + r + 2] = 0.0
        self.red[nr + r + 2] = np.sum(logs)
        self.red[nr + r + 3] = self.xlx

    def _likelihood(self):
        nr, r = self.n * self.rank, self.rank
        cross = float(np.sum(self.w.sum(axis=0) * self.red[nr:nr + r]))
        self.lk = ((self.red[nr + r + 2] - cross) + self.red[nr + r + 3]) / self.n / self.m_global

    def reduce_tail(self):
        return self.n * self.rank, self.rank + 4

    def ml_set_state(self, w, h, finish=True):
        self.w, self.h = np.array(w, dtype=np.float64), np.array(h, dtype=np.float64)
        assert self.h.shape == (self.rank, self.m)
        self._tail()
        self.phase, self.pending = 0, True

    def ml_state_finish(self):
        assert self.pending
        self._likelihood()
        self.pending = False

    def ml_step_local(self, prior=False, gamma_a=1.0, gamma_b=1.0):
        assert not self.pending and self.phase < 2
        nr, r = self.n * self.rank, self.rank
        if self.phase == 0:
            up = self.h * (self.w.T @ (self.X / (self.w @ self.h)))
            down = self.w.sum(axis=0)[:, None]
            if prior:
                up, down = up + gamma_a - 1, down + gamma_a / gamma_b
            self.h = np.maximum(up / down, EPS)
            self.red[:nr] = ((self.X / (self.w @ self.h)) @ self.h.T).ravel()
            self.red[nr:nr + r] = self.h.sum(axis=1)
            self.red[nr + r:nr + r + 2] = 0.0
        else:
            up = self.w * self.red[:nr].reshape(self.n, r)
            down = self.red[nr:nr + r][None, :]
            if prior:
                up, down = up + gamma_a - 1, down + gamma_a / gamma_b
            self.w = np.maximum(up / down, EPS)
            self._tail()
        self.phase += 1

    def ml_step_finish(self):
        if self.phase != 2:
            raise RuntimeError("ml_step_finish without ml_step_local")
        self._likelihood()
        self.phase = 0
        return self.lk

    def ml_likelihood(self):
        return self.lk

    def ml_get_state(self, names=("ew", "eh")):
        return {k: v.copy() for k, v in (("ew", self.w), ("eh", self.h)) if k in names}

    def close(self):
        pass


def _exchange(parts, tail=False):
    off = parts[0].n * parts[0].rank if tail else 0
    s = sum(p.red[off:] for p in parts)
    for p in parts:
        p.red[off:] = s


def _group_step(parts, **kw):
    for p in parts:
        p.ml_step_local(**kw)
    _exchange(parts)
    for p in parts:
        p.ml_step_local(**kw)
    _exchange(parts, tail=True)
    return [p.ml_step_finish() for p in parts]


@pytest.mark.parametrize("cuts", [((0, 20), (20, 53)), ((0, 7), (7, 30), (30, 53))])
@pytest.mark.parametrize("steps", [1, 5])
@pytest.mark.parametrize("prior", [False, True])
def test_partition_algebra_matches_the_oracle(cuts, steps, prior):
    from oracle import mlnmf_oracle as O
    n, m, r = 37, 53, 3
    X = counts(n, m, 0.9, seed=41)
    rng = np.random.default_rng(5)
    w, h = rng.uniform(size=(n, r)), rng.uniform(size=(r, m))
    kw = dict(prior=prior, gamma_a=2.5, gamma_b=0.7)
    parts = [NumpyMLPartition(X, r, cols=c, m_global=m) for c in cuts]
    for p, (b, e) in zip(parts, cuts):
        p.ml_set_state(w, h[:, b:e])
    _exchange(parts, tail=True)
    for p in parts:
        p.ml_state_finish()
        assert abs(p.ml_likelihood() / O.likelihood_literal(X, w, h) - 1) <= 1e-10
    want = {"ew": w, "eh": h}
    for _ in range(steps):
        lks = _group_step(parts, **kw)
        want = O.nmf_update_literal(X, want["ew"], want["eh"], prior, 2.5, 0.7)
        assert all(v == lks[0] for v in lks)                      # the same bits on every partition
        assert abs(lks[0] / O.likelihood_literal(X, want["ew"], want["eh"]) - 1) <= 1e-10
    st = [p.ml_get_state() for p in parts]
    for q in st[1:]:
        assert np.array_equal(st[0]["ew"], q["ew"])               # w replicated bit for bit
    assert relerr(st[0]["ew"], want["ew"]) <= 1e-12
    assert relerr(np.concatenate([q["eh"] for q in st], axis=1), want["eh"]) <= 1e-12


def test_numpy_partition_refuses_finish_without_local():
    p = NumpyMLPartition(counts(8, 9, 1.0, 1), 2)
    p.ml_set_state(np.ones((8, 2)), np.ones((2, 9)))
    p.ml_state_finish()
    with pytest.raises(RuntimeError):
        p.ml_step_finish()


def _worker(rank, world, port, q):
    import torch.distributed as dist
    sys.path.insert(0, ROOT); sys.path.insert(0, HERE)
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from test_ml_partition_cpu import NumpyMLPartition, counts
        from ccfindr_amd import parallel
        n, m, r = 30, 47, 3
        X = counts(n, m, 0.8, seed=17)
        rng = np.random.default_rng(3)
        w, h = rng.uniform(size=(n, r)), rng.uniform(size=(r, m))
        cols = parallel.cell_partition(m, world)[rank]
        eng = parallel.CellPartitionedEngine(X, r, engine=NumpyMLPartition(X, r, cols=cols, m_global=m))
        eng.ml_set_state(w, h)                                    # the FULL h: each process takes its block
        lk0 = eng.ml_likelihood()
        trace = [eng.ml_step() for _ in range(4)]
        trace.append(eng.ml_step(prior=True, gamma_a=2.0, gamma_b=1.5))
        state = eng.ml_get_state()
        errors = []
        for call in (lambda: eng.ml_run(criterion="connectivity"), lambda: eng.ml_run(Itmax=3)):
            try:
                call()
                errors.append(None)
            except (ValueError, RuntimeError) as exc:
                errors.append(type(exc).__name__)
        q.put((rank, lk0, trace, eng.ml_likelihood(), state, errors))
    finally:
        dist.destroy_process_group()


def test_cell_partitioned_engine_ml_surface_world2():
    import torch.multiprocessing as mp
    from oracle import mlnmf_oracle as O
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33700 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(k, 2, port, q)) for k in range(2)]
    for p in procs:
        p.start()
    outs = sorted([q.get(timeout=240) for _ in procs], key=lambda o: o[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    n, m, r = 30, 47, 3
    X = counts(n, m, 0.8, seed=17)
    rng = np.random.default_rng(3)
    w, h = rng.uniform(size=(n, r)), rng.uniform(size=(r, m))
    want, lks = {"ew": w, "eh": h}, []
    for t in range(5):
        want = O.nmf_update_literal(X, want["ew"], want["eh"], t == 4, 2.0, 1.5)
        lks.append(O.likelihood_literal(X, want["ew"], want["eh"]))
    for rank, lk0, trace, lk_last, state, errors in outs:
        assert abs(lk0 / O.likelihood_literal(X, w, h) - 1) <= 1e-10
        assert np.allclose(trace, lks, rtol=1e-10, atol=0)
        assert lk_last == trace[-1]
        assert state["ew"].shape == (n, r) and state["eh"].shape == (r, m)          # eh all-gathered to full width
        assert relerr(state["ew"], want["ew"]) <= 1e-11 and relerr(state["eh"], want["eh"]) <= 1e-11
        # the connectivity rule is refused; so is a device loop without the native communicator
        assert errors == ["ValueError", "RuntimeError"]
    assert outs[0][2] == outs[1][2]                               # identical on every partition
    assert np.array_equal(outs[0][4]["ew"], outs[1][4]["ew"])
