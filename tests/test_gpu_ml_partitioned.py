"""ML-NMF (factorize()'s step, reference R/factorize.R:2-27, :40-49, loop :194-213) with the cells partitioned: the
host-stepped protocol (ml_step_local / exchange / ml_step_local / exchange of the tail / ml_step_finish), the device-driven
loop of a local group and of an engine with an RCCL communicator, and factorize() over a CellPartitionedEngine.

ONE test GPU: the multi-partition runs use a local group (partition engines side by side in this process, the sum a kernel
in partition order), real RCCL runs with one rank, and two ranks go through tests/fake_rccl's stand-in.  Tolerances: one to
three steps -- factors 1e-12 max-rel, likelihood 1e-10; state after a loop 1e-9; histories 1e-10."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FAKE = os.path.join(HERE, "fake_rccl", "_build", "libfake_rccl.so")


def relerr(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def counts(n, m, lam, seed):
    rng = np.random.default_rng(seed)
    X = rng.poisson(lam, size=(n, m)).astype(np.float64)
    X[np.arange(n), rng.integers(0, m, n)] += 1      # no empty rows
    X[rng.integers(0, n, m), np.arange(m)] += 1      # no empty columns
    return np.asfortranarray(X)


def uniform_state(n, m, r, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(size=(n, r)), rng.uniform(size=(r, m))


def _group(M, r, cuts, m, w, h):
    import ccfindr_amd as C
    comm = C.Communicator.local(len(cuts))
    parts = [C.VBEngine(M, r, cols=c, m_global=m) for c in cuts]
    for p, (b, e) in zip(parts, cuts):
        p.attach_comm(comm)
        p.ml_set_state(w, h[:, b:e])
    if len(cuts) > 1:                                # (one partition of everything is an unpartitioned engine: nothing pending)
        comm.ml_state_finish()
    return comm, parts


def _exchange(parts, reds, tail):
    import torch
    torch.cuda.synchronize()
    off = parts[0].reduce_tail()[0] if tail else 0
    s = sum((q[off:] for q in reds[1:]), reds[0][off:].clone())
    for q in reds:
        q[off:].copy_(s)
    torch.cuda.synchronize()


def _host_step(parts, reds, **kw):
    for p in parts:
        p.ml_step_local(**kw)
    _exchange(parts, reds, False)
    for p in parts:
        p.ml_step_local(**kw)
    _exchange(parts, reds, True)
    return [p.ml_step_finish() for p in parts]


def _close(*things):
    for t in things:
        t.close()


CASES = [
    # n, m, r, cuts (None: cell_partition(m, P)), P, integer X, prior
    (37, 53, 3, None, 1, True, False),
    (37, 53, 3, None, 2, True, False),
    (37, 53, 3, None, 3, True, False),               # 53 does not divide
    (64, 96, 10, None, 2, True, False),
    (40, 90, 20, None, 2, True, False),              # the 512-thread sweep
    (50, 120, 40, None, 2, True, False),             # two lanes per task
    (48, 77, 5, None, 2, False, False),              # non-integer X: the wide layout
    (37, 53, 3, None, 2, True, True),                # Gamma prior
    (64, 300, 4, ((0, 2), (2, 300)), 2, True, False),   # a 2-cell partition next to a wide one: fewer majors than update blocks
]


@pytest.mark.parametrize("n,m,r,cuts,P,integer,prior", CASES)
def test_host_stepped_steps_equal_single_engine_and_oracle(n, m, r, cuts, P, integer, prior):
    import ccfindr_amd as C
    from ccfindr_amd.parallel import cell_partition
    from oracle import mlnmf_oracle as O
    X = counts(n, m, 0.7, seed=n + m + r)
    if not integer:
        X = X * (np.median(X.sum(axis=0)) / X.sum(axis=0))[None, :]
    w, h = uniform_state(n, m, r, seed=11)
    kw = dict(prior=prior, gamma_a=2.5, gamma_b=0.7)
    M = C.CountMatrix(X)
    whole = C.VBEngine(M, r)
    whole.ml_set_state(w, h)
    cuts = list(cuts) if cuts else cell_partition(m, P)
    comm, parts = _group(M, r, cuts, m, w, h)
    for p in parts:                                              # the likelihood of the loaded pair, from the state exchange
        assert abs(p.ml_likelihood() / whole.ml_likelihood() - 1) <= 1e-10
        assert abs(p.ml_likelihood() / O.likelihood_literal(X, w, h) - 1) <= 1e-10
    reds = [p.reduce_tensor() for p in parts]
    want = {"ew": w, "eh": h}
    for _ in range(3):
        lks = _host_step(parts, reds, **kw)
        lk1 = whole.ml_step(**kw)
        want = O.nmf_update_literal(X, want["ew"], want["eh"], prior, 2.5, 0.7)
        assert all(v == lks[0] for v in lks)                     # the same bits on every partition
        assert abs(lks[0] / lk1 - 1) <= 1e-10
        assert abs(lks[0] / O.likelihood_literal(X, want["ew"], want["eh"]) - 1) <= 1e-10
    ref = whole.ml_get_state()
    st = [p.ml_get_state() for p in parts]
    for q in st[1:]:
        assert np.array_equal(st[0]["ew"], q["ew"])              # w replicated bit for bit
    eh = np.concatenate([q["eh"] for q in st], axis=1)
    assert [q["eh"].shape[1] for q in st] == [e - b for b, e in cuts]
    for got, single, oracle in ((st[0]["ew"], ref["ew"], want["ew"]), (eh, ref["eh"], want["eh"])):
        assert relerr(got, single) <= 1e-12 and relerr(got, oracle) <= 1e-12
    assert all(p.ml_likelihood() == lks[0] for p in parts)
    _close(*parts, whole, comm, M)


@pytest.mark.parametrize("itmax,P", [(1, 3), (8, 3), (37, 3), (11, 1)])
def test_local_group_device_loop_equals_single_engine(itmax, P):
    """Tol = 0 never converges: reason 4 inside, exactly at and across the queued batches of eight.  P = 1: a group of one
    partition that covers every cell is an unpartitioned engine driven through the group's protocol (exchanges with itself)."""
    import ccfindr_amd as C
    from ccfindr_amd.parallel import cell_partition
    n, m, r = 120, 260, 4
    X = counts(n, m, 0.3, seed=7)
    w, h = uniform_state(n, m, r, seed=2)
    M = C.CountMatrix(X)
    whole = C.VBEngine(M, r)
    whole.ml_set_state(w, h)
    want = whole.ml_run(Itmax=itmax, Tol=0.0, history=True)
    ref = whole.ml_get_state()
    comm, parts = _group(M, r, cell_partition(m, P), m, w, h)
    got = comm.ml_run(Itmax=itmax, Tol=0.0, history=True)
    assert got["it"] == want["it"] == itmax and got["reason"] == want["reason"] == 4
    assert relerr(got["history"], want["history"]) <= 1e-10
    assert abs(got["lk"] / want["lk"] - 1) <= 1e-10
    st = [p.ml_get_state() for p in parts]
    for q in st[1:]:
        assert np.array_equal(st[0]["ew"], q["ew"])
    assert relerr(st[0]["ew"], ref["ew"]) <= 1e-9
    assert relerr(np.concatenate([q["eh"] for q in st], axis=1), ref["eh"]) <= 1e-9
    assert all(p.ml_likelihood() == got["lk"] for p in parts)
    # the host-stepped protocol goes on from the loop's end state
    reds = [p.reduce_tensor() for p in parts]
    lks = _host_step(parts, reds)
    assert all(v == lks[0] for v in lks) and abs(lks[0] / whole.ml_step() - 1) <= 1e-10
    # ... and so does a second loop
    again, want2 = comm.ml_run(Itmax=3, Tol=0.0, history=True), whole.ml_run(Itmax=3, Tol=0.0, history=True)
    assert again["it"] == 3 and relerr(again["history"], want2["history"]) <= 1e-10
    _close(*parts, whole, comm, M)


def test_local_group_loop_stops_inside_a_batch_and_queued_steps_change_nothing():
    """A convergence break (R/factorize.R:211) inside a queued batch, at the single engine's step; afterwards the state is
    that of as many host-stepped partitioned steps, so the kernels AND the all-reduces queued past the stop were no-ops.

    Matrix counts(60, 90, 0.8, seed=103), start uniform_state(seed=3), Tol = 1e-4: the oracle stops at step 85 (85 % 8 = 5)
    with |lkold - lk| / |lkold| = 0.956 Tol there and 1.009 Tol one step earlier -- both a factor 1 -+ 1e-3 away from Tol and
    more, checked below, so the rounding differences between the sums' orders (1e-10 at most) cannot move the stop."""
    import ccfindr_amd as C
    from ccfindr_amd.parallel import cell_partition
    from oracle import mlnmf_oracle as O
    n, m, r, P, tol = 60, 90, 3, 3, 1e-4
    X = counts(n, m, 0.8, seed=103)
    w, h = uniform_state(n, m, r, seed=3)
    lkold, cur, ratios = -np.inf, {"ew": w, "eh": h}, []
    for it in range(1, 200):
        cur = O.nmf_update_literal(X, cur["ew"], cur["eh"])
        lk = O.likelihood_literal(X, cur["ew"], cur["eh"])
        ratios.append(abs(lkold - lk) / abs(lkold) if np.isfinite(lkold) else np.inf)
        if ratios[-1] < tol:
            break
        lkold = lk
    assert it == 85 and it % 8 != 0
    assert ratios[-1] <= tol * (1 - 1e-3) and ratios[-2] >= tol * (1 + 1e-3)
    M = C.CountMatrix(X)
    whole = C.VBEngine(M, r)
    whole.ml_set_state(w, h)
    want = whole.ml_run(Itmax=2000, Tol=tol)
    assert want["it"] == it and want["reason"] == 2
    cuts = cell_partition(m, P)
    comm, parts = _group(M, r, cuts, m, w, h)
    got = comm.ml_run(Itmax=2000, Tol=tol, history=True)
    assert got["it"] == it and got["reason"] == 2 and len(got["history"]) == it
    assert abs(got["lk"] / want["lk"] - 1) <= 1e-9
    st = [p.ml_get_state() for p in parts]
    comm2, stepped = _group(M, r, cuts, m, w, h)
    reds = [p.reduce_tensor() for p in stepped]
    for _ in range(it):
        lks = _host_step(stepped, reds)
    assert abs(lks[0] / got["lk"] - 1) <= 1e-12
    for a, b in zip(st, (p.ml_get_state() for p in stepped)):
        assert relerr(a["ew"], b["ew"]) <= 1e-12 and relerr(a["eh"], b["eh"]) <= 1e-12
    # the next host-stepped step of both groups agrees too: the loop left the statistics of ITS last step behind
    a, b = _host_step(parts, [p.reduce_tensor() for p in parts]), _host_step(stepped, reds)
    assert abs(a[0] / b[0] - 1) <= 1e-12
    _close(*parts, *stepped, whole, comm, comm2, M)


def test_nan_in_w_runs_to_itmax_on_every_partition():
    """A NaN likelihood never satisfies the test (as in R): the loop ends at Itmax, reason 4, like the single engine's; the
    group call itself fails if the partitions do not report the same step and reason."""
    import ccfindr_amd as C
    from ccfindr_amd.parallel import cell_partition
    n, m, r, P = 40, 70, 3, 2
    X = counts(n, m, 0.6, seed=9)
    w, h = uniform_state(n, m, r, seed=4)
    w[5, 1] = np.nan
    M = C.CountMatrix(X)
    whole = C.VBEngine(M, r)
    whole.ml_set_state(w, h)
    want = whole.ml_run(Itmax=11, Tol=1e-5)
    comm, parts = _group(M, r, cell_partition(m, P), m, w, h)
    got = comm.ml_run(Itmax=11, Tol=1e-5, history=True)
    assert np.isnan(got["lk"]) and np.isnan(want["lk"]) and np.all(np.isnan(got["history"]))
    assert got["it"] == want["it"] == 11 and got["reason"] == want["reason"] == 4
    assert all(np.isnan(p.ml_likelihood()) for p in parts)
    _close(*parts, whole, comm, M)


def test_rccl_communicator_one_rank_ml_loop():
    """The RCCL form of the loop with a 1-rank communicator: the engine owns every cell but is declared one partition of a
    matrix twice as wide, which only halves the likelihood."""
    import ccfindr_amd as C
    n, m, r = 90, 140, 5
    X = counts(n, m, 0.5, seed=31)
    w, h = uniform_state(n, m, r, seed=6)
    M = C.CountMatrix(X)
    whole = C.VBEngine(M, r)
    whole.ml_set_state(w, h)
    lk_loaded = whole.ml_likelihood()
    want = whole.ml_run(Itmax=19, Tol=0.0, history=True)
    comm = C.Communicator.rccl(C.Communicator.unique_id(), 1, 0, 0)
    part = C.VBEngine(M, r, cols=(0, m), m_global=2 * m)
    part.attach_comm(comm)
    part.ml_set_state(w, h)                                      # finish=True: the library's all-reduce and ml_state_finish inside
    assert abs(2.0 * part.ml_likelihood() / lk_loaded - 1) <= 1e-10
    part.ml_set_state(w, h, finish=False)                        # ... or by hand
    part.allreduce()
    part.ml_state_finish()
    got = part.ml_run(Itmax=19, Tol=0.0, history=True)
    assert got["it"] == 19 and got["reason"] == 4
    assert relerr(2.0 * got["history"], want["history"]) <= 1e-10
    a, b = part.ml_get_state(), whole.ml_get_state()
    for k in a:
        assert relerr(a[k], b[k]) <= 1e-9, k
    # host-stepped with the library's all-reduce
    part.ml_step_local(); part.allreduce(); part.ml_step_local(); part.allreduce()
    assert abs(2.0 * part.ml_step_finish() / whole.ml_step() - 1) <= 1e-10
    _close(part, whole, comm, M)


def test_refusals():
    import ccfindr_amd as C
    n, m, r = 30, 50, 3
    X = counts(n, m, 0.8, seed=12)
    w, h = uniform_state(n, m, r, seed=1)
    M = C.CountMatrix(X)
    comm, parts = _group(M, r, [(0, 20), (20, 50)], m, w, h)
    p = parts[0]
    with pytest.raises(C.VBNMFError, match="ml_step_local"):
        p.ml_step()
    with pytest.raises(C.VBNMFError, match="connectivity"):
        p.ml_run(criterion="connectivity")
    with pytest.raises(C.VBNMFError, match="without ml_step_local"):
        p.ml_step_finish()
    p.ml_step_local()
    with pytest.raises(C.VBNMFError, match="without ml_step_local"):       # one half is not a step
        p.ml_step_finish()
    with pytest.raises(C.VBNMFError, match="RCCL communicator"):           # a local group's engine alone has no loop
        p.ml_run(Itmax=2)
    with pytest.raises(C.VBNMFError, match="ml_state_finish"):
        p.ml_state_finish()
    _close(*parts, comm, M)


def test_cell_partitioned_engine_refuses_the_connectivity_loop():
    import ccfindr_amd as C
    from ccfindr_amd.parallel import CellPartitionedEngine
    X = counts(30, 40, 0.8, seed=2)
    M = C.CountMatrix(X)
    eng = CellPartitionedEngine(M, 2)
    with pytest.raises(ValueError):
        eng.ml_run(criterion="connectivity")
    _close(eng, M)


def test_factorize_over_a_cell_partitioned_engine():
    """The call the drivers make.  A world of one builds an unpartitioned engine, so this covers the ml_* SURFACE factorize()
    needs of a CellPartitionedEngine, not the partitioned step (the tests above do that)."""
    import ccfindr_amd as C
    from ccfindr_amd.parallel import CellPartitionedEngine
    X = counts(60, 80, 0.9, seed=55)
    kw = dict(ranks=[2, 3], nrun=3, verbose=0, seed=7)
    plain = C.factorize(X, **kw)
    part = C.factorize(X, engine_factory=lambda M, r: CellPartitionedEngine(M, r), **kw)
    assert part.nsteps == plain.nsteps
    assert relerr(np.asarray(part.measure["likelihood"]), np.asarray(plain.measure["likelihood"])) <= 1e-9
    for a, b in zip(part.basis + part.coeff, plain.basis + plain.coeff):
        assert relerr(a, b) <= 1e-9


def _problem():
    n, m, r = 120, 260, 4
    return counts(n, m, 0.3, seed=7), n, m, r, uniform_state(n, m, r, seed=2)


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ["VBNMF_RCCL_LIB"] = FAKE
    os.environ["FAKE_RCCL_TIMEOUT_S"] = "20"
    os.environ["FAKE_RCCL_KERNEL"] = "0"
    os.environ["VBNMF_WAIT_TIMEOUT_S"] = "30"                # bounded waits: a lost peer ends in an error, not a hang
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import ccfindr_amd as C
        from ccfindr_amd.parallel import CellPartitionedEngine
        X, n, m, r, (w, h) = _problem()
        M = C.CountMatrix(X)
        eng = CellPartitionedEngine(M, r, device=0, native=True)          # the library's communicator, 2 ranks
        eng.ml_set_state(w, h)
        lk0 = eng.ml_likelihood()
        out = eng.ml_run(Itmax=5, Tol=0.0, history=True)
        full = eng.ml_get_state()                                         # w replicated, h all-gathered
        lk_next = eng.ml_step()                                           # host-stepped, the library's all-reduce
        q.put((rank, lk0, out, lk_next, full))
        eng.close()
    finally:
        dist.destroy_process_group()


def test_two_ranks_through_the_rccl_stand_in():
    import torch.multiprocessing as mp
    import ccfindr_amd as C
    assert os.path.exists(FAKE), "tests/fake_rccl is not built (make, or __graft_entry__.build())"
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35100 + (os.getpid() % 1500)
    procs = [ctx.Process(target=_worker, args=(k, 2, port, q)) for k in range(2)]
    for p in procs:
        p.start()
    outs = sorted([q.get(timeout=120) for _ in procs], key=lambda o: o[0])
    for p in procs:
        p.join(timeout=60)
        if p.is_alive():                                                    # a stuck child must not keep the GPU open
            p.terminate()
        assert p.exitcode == 0
    X, n, m, r, (w, h) = _problem()
    M = C.CountMatrix(X)
    whole = C.VBEngine(M, r)
    whole.ml_set_state(w, h)
    lk0 = whole.ml_likelihood()
    want = whole.ml_run(Itmax=5, Tol=0.0, history=True)
    ref = whole.ml_get_state()
    lk_next = whole.ml_step()
    a, b = outs[0][2], outs[1][2]
    assert a["it"] == b["it"] == 5 and a["reason"] == b["reason"] == 4
    assert np.array_equal(a["history"], b["history"])                       # the same history on both ranks
    assert relerr(a["history"], want["history"]) <= 1e-10
    for o in outs:
        assert abs(o[1] / lk0 - 1) <= 1e-10 and abs(o[3] / lk_next - 1) <= 1e-10
        assert o[4]["eh"].shape == (r, m)                                   # all-gathered to full width
        assert relerr(o[4]["ew"], ref["ew"]) <= 1e-9 and relerr(o[4]["eh"], ref["eh"]) <= 1e-9
    assert np.array_equal(outs[0][4]["ew"], outs[1][4]["ew"])
    _close(whole, M)
