"""criterion = 'connectivity' (reference R/factorize.R:198-208) in the device-driven loop of a cell-partitioned ML-NMF: the
partitions' (r+1) x (r+1) label tables travel as doubles inside the step's second exchange, the control step counts the
changed pairs of ALL cells on their sum, and every partition takes the same decision.

The yardstick of every exact comparison is the CPU oracle (util_ml_connectivity.oracle_loop), never the code under test.
The partitioned loop agrees with it to ~1e-9 in the state, not bit for bit, so integer counts are compared only where no
label sits on a near-tie: each test first asserts that the smallest relative gap between a cell's two largest h entries over
the oracle's trajectory is >= 1e-6.

ONE test GPU: local groups (partition engines side by side in this process), real RCCL with one rank, two ranks through
tests/fake_rccl's stand-in.  Tolerances: histories 1e-10, the state after a loop 1e-9 (test_gpu_ml_partitioned.py)."""
import os
import sys

import numpy as np
import pytest

import util_ml_connectivity as U
from util_ml_connectivity import counts

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FAKE = os.path.join(HERE, "fake_rccl", "_build", "libfake_rccl.so")


def relerr(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


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


def _host_step(parts, reds):
    for p in parts:
        p.ml_step_local()
    _exchange(parts, reds, False)
    for p in parts:
        p.ml_step_local()
    _exchange(parts, reds, True)
    return [p.ml_step_finish() for p in parts]


def _close(*things):
    for t in things:
        t.close()


def _oracle(case, stop=None):
    o = U.oracle_run(*case)
    assert o["gap"] >= U.MIN_GAP, o["gap"]           # the condition of every integer comparison below
    assert o["reason"] == 2 and (stop is None or o["it"] == stop)
    return o


def _check_against_oracle(got, o, parts, cuts, m):
    assert got["it"] == o["it"] and got["reason"] == 2
    assert got["changes"].dtype == np.int64 and np.array_equal(got["changes"], o["changes"])
    assert got["changes"][0] == m * (m - 1) // 2                    # the pairs of ALL cells, not of a partition's
    assert relerr(got["history"], o["history"]) <= 1e-10
    assert abs(got["lk"] / o["history"][-1] - 1) <= 1e-10
    st = [p.ml_get_state() for p in parts]
    for q in st[1:]:
        assert np.array_equal(st[0]["ew"], q["ew"])                 # w replicated bit for bit
    assert [q["eh"].shape[1] for q in st] == [e - b for b, e in cuts]
    assert relerr(st[0]["ew"], o["ew"]) <= 1e-9
    assert relerr(np.concatenate([q["eh"] for q in st], axis=1), o["eh"]) <= 1e-9
    # every partition's labels of the last step are its own cells' (conn_finish covers every member)
    ids = np.concatenate([p.cluster_ids() for p in parts])
    assert np.array_equal(ids, o["labels"])
    return st


@pytest.mark.parametrize("P", [1, 2, 3])
@pytest.mark.parametrize("row", range(len(U.TABLE)))
def test_local_group_connectivity_loop_equals_the_oracle(row, P):
    import ccfindr_amd as C
    from ccfindr_amd.parallel import cell_partition
    case = U.TABLE[row]
    n, m, r, ncnn = case[0], case[1], case[2], case[6]
    o = _oracle(case, U.STOPS[row])
    M = C.CountMatrix(o["X"])
    cuts = cell_partition(m, P)
    comm, parts = _group(M, r, cuts, m, o["w"], o["h"])
    got = comm.ml_run_connectivity(Itmax=400, ncnn_step=ncnn, history=True, changes=True)
    _check_against_oracle(got, o, parts, cuts, m)
    whole = C.VBEngine(M, r)
    whole.ml_set_state(o["w"], o["h"])
    single = whole.ml_run(Itmax=400, criterion="connectivity", ncnn_step=ncnn, changes=True)
    assert single["it"] == got["it"] and np.array_equal(single["changes"], got["changes"])
    _close(*parts, whole, comm, M)


def test_a_two_cell_partition_next_to_a_wide_one():
    """((0, 2), (2, 300)) on 64 x 300, r = 4: fewer majors than update blocks on partition 0, and nearly every changed pair
    has a cell in each partition.  X seed 7, state seed 4: the oracle stops at step 104, smallest gap 1.2e-4."""
    import ccfindr_amd as C
    n, m, r, ncnn = U.UNEVEN[0], U.UNEVEN[1], U.UNEVEN[2], U.UNEVEN[6]
    o = _oracle(U.UNEVEN, 104)
    assert o["gap"] >= 1e-4
    cuts = [(0, 2), (2, 300)]
    M = C.CountMatrix(o["X"])
    comm, parts = _group(M, r, cuts, m, o["w"], o["h"])
    got = comm.ml_run_connectivity(Itmax=400, ncnn_step=ncnn, history=True, changes=True)
    _check_against_oracle(got, o, parts, cuts, m)
    _close(*parts, comm, M)


def test_itmax_before_the_stop_then_a_stop_inside_a_batch_and_queued_steps_change_nothing():
    """64 x 96, r = 10 on three partitions.  Itmax = 20 ends the loop first (reason 4); a second loop from that state restarts
    the rule (its first count is npair again) and stops where the oracle, continued from ITS step-20 state, stops: step 39 of
    that loop, 39 % 8 = 7, strictly inside a queued batch of eight.  Afterwards the state is that of 20 + 39 host-stepped
    partitioned steps, so the kernels and the exchanges queued past the stop -- the table's stretch included -- changed nothing."""
    import ccfindr_amd as C
    from ccfindr_amd.parallel import cell_partition
    case = U.TABLE[1]
    n, m, r, ncnn, P = case[0], case[1], case[2], case[6], 3
    full = _oracle(case, 59)
    first = U.oracle_run(*case, itmax=20)
    assert first["it"] == 20 and first["reason"] == 4 and np.array_equal(first["changes"], full["changes"][:20])
    second = U.oracle_loop(first["X"], first["ew"], first["eh"], ncnn)
    assert second["gap"] >= U.MIN_GAP and second["reason"] == 2
    assert second["it"] == 39 and second["it"] % 8 not in (0, 1)
    M = C.CountMatrix(full["X"])
    cuts = cell_partition(m, P)
    comm, parts = _group(M, r, cuts, m, full["w"], full["h"])
    a = comm.ml_run_connectivity(Itmax=20, ncnn_step=ncnn, history=True, changes=True)
    assert a["it"] == 20 and a["reason"] == 4 and len(a["changes"]) == 20 and len(a["history"]) == 20
    assert np.array_equal(a["changes"], first["changes"])
    b = comm.ml_run_connectivity(Itmax=400, ncnn_step=ncnn, history=True, changes=True)
    assert b["it"] == second["it"] and b["reason"] == 2
    assert b["changes"][0] == m * (m - 1) // 2 and np.array_equal(b["changes"], second["changes"])
    assert relerr(b["history"], second["history"]) <= 1e-10
    st = [p.ml_get_state() for p in parts]
    comm2, stepped = _group(M, r, cuts, m, full["w"], full["h"])
    reds = [p.reduce_tensor() for p in stepped]
    for _ in range(a["it"] + b["it"]):
        lks = _host_step(stepped, reds)
    assert abs(lks[0] / b["lk"] - 1) <= 1e-12
    for x, y in zip(st, (p.ml_get_state() for p in stepped)):
        assert relerr(x["ew"], y["ew"]) <= 1e-12 and relerr(x["eh"], y["eh"]) <= 1e-12
    # the next host-stepped step of both groups agrees too: the loop left the statistics of ITS last step behind
    x, y = _host_step(parts, [p.reduce_tensor() for p in parts]), _host_step(stepped, reds)
    assert abs(x[0] / y[0] - 1) <= 1e-12
    _close(*parts, *stepped, comm, comm2, M)


def test_the_likelihood_loop_is_untouched():
    """Tol = 0, eight steps on a group of three: bit-identical histories before a connectivity run, after one on fresh groups,
    and on the very engines that ran the connectivity loop (reloaded) -- both exchanges are back to today's lengths."""
    import ccfindr_amd as C
    from ccfindr_amd.parallel import cell_partition
    case = U.TABLE[0]
    n, m, r = case[0], case[1], case[2]
    X, (w, h) = counts(n, m, case[3], case[4]), U.uniform_state(n, m, r, case[5])
    M = C.CountMatrix(X)
    cuts = cell_partition(m, 3)

    def likelihood_history(comm):
        out = comm.ml_run(Itmax=8, Tol=0.0, history=True)
        assert out["it"] == 8 and out["reason"] == 4
        return out["history"]

    comm_a, parts_a = _group(M, r, cuts, m, w, h)
    before = likelihood_history(comm_a)
    comm_b, parts_b = _group(M, r, cuts, m, w, h)
    conn = comm_b.ml_run_connectivity(Itmax=11, ncnn_step=5, changes=True)
    assert conn["it"] == 11 and conn["changes"][0] == m * (m - 1) // 2
    comm_c, parts_c = _group(M, r, cuts, m, w, h)
    after = likelihood_history(comm_c)
    for p, (b, e) in zip(parts_b, cuts):
        p.ml_set_state(w, h[:, b:e])
    comm_b.ml_state_finish()
    same_engines = likelihood_history(comm_b)
    assert before.tobytes() == after.tobytes() == same_engines.tobytes()
    _close(*parts_a, *parts_b, *parts_c, comm_a, comm_b, comm_c, M)


def test_rccl_communicator_one_rank_connectivity_loop():
    """The RCCL form with a 1-rank communicator: the engine owns every cell but is declared one partition of a matrix twice as
    wide.  The labels are its own cells', so every count behind the first equals the whole engine's; the first is the pair
    count of the declared width."""
    import ccfindr_amd as C
    case = U.TABLE[4]
    n, m, r, ncnn = case[0], case[1], case[2], case[6]
    o = _oracle(case, U.STOPS[4])
    M = C.CountMatrix(o["X"])
    whole = C.VBEngine(M, r)
    whole.ml_set_state(o["w"], o["h"])
    want = whole.ml_run(Itmax=400, criterion="connectivity", ncnn_step=ncnn, history=True, changes=True)
    comm = C.Communicator.rccl(C.Communicator.unique_id(), 1, 0, 0)
    part = C.VBEngine(M, r, cols=(0, m), m_global=2 * m)
    part.attach_comm(comm)
    part.ml_set_state(o["w"], o["h"])
    got = part.ml_run(Itmax=400, criterion="connectivity", ncnn_step=ncnn, history=True, changes=True)
    assert got["changes"][0] == 2 * m * (2 * m - 1) // 2
    assert got["it"] == want["it"] == o["it"] and got["reason"] == 2
    assert np.array_equal(got["changes"][1:], want["changes"][1:]) and np.array_equal(got["changes"][1:], o["changes"][1:])
    assert relerr(2.0 * got["history"], want["history"]) <= 1e-10
    _close(part, whole, comm, M)


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT); sys.path.insert(0, HERE)
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
        import util_ml_connectivity as W
        case = W.TABLE[0]
        n, m, r = case[0], case[1], case[2]
        X, (w, h) = W.counts(n, m, case[3], case[4]), W.uniform_state(n, m, r, case[5])
        M = C.CountMatrix(X)
        eng = CellPartitionedEngine(M, r, device=0, native=True)          # the library's communicator, 2 ranks
        eng.ml_set_state(w, h)
        out = eng.ml_run_connectivity(Itmax=400, ncnn_step=case[6], history=True, changes=True)
        ids = eng.cluster_ids()                                           # all 260 cells, on both ranks
        q.put((rank, out, ids))
        eng.close()
    finally:
        dist.destroy_process_group()


def test_two_ranks_through_the_rccl_stand_in():
    import torch.multiprocessing as mp
    assert os.path.exists(FAKE), "tests/fake_rccl is not built (make, or __graft_entry__.build())"
    o = _oracle(U.TABLE[0], U.STOPS[0])
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 37900 + (os.getpid() % 1500)
    procs = [ctx.Process(target=_worker, args=(k, 2, port, q)) for k in range(2)]
    for p in procs:
        p.start()
    try:
        outs = sorted([q.get(timeout=120) for _ in procs], key=lambda x: x[0])
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():                                                # a stuck child must not keep the GPU open
                p.terminate()
    assert all(p.exitcode == 0 for p in procs)
    a, b = outs[0][1], outs[1][1]
    assert a["it"] == b["it"] == o["it"] and a["reason"] == b["reason"] == 2
    assert np.array_equal(a["changes"], b["changes"]) and np.array_equal(a["changes"], o["changes"])
    assert np.array_equal(a["history"], b["history"])                       # the same history on both ranks
    assert relerr(a["history"], o["history"]) <= 1e-10
    for _, _, ids in outs:
        assert ids.dtype == np.int32 and np.array_equal(ids, o["labels"])


def test_a_local_groups_member_alone_is_refused():
    import ccfindr_amd as C
    n, m, r = 30, 50, 3
    X = counts(n, m, 0.8, seed=12)
    w, h = U.uniform_state(n, m, r, seed=1)
    M = C.CountMatrix(X)
    comm, parts = _group(M, r, [(0, 20), (20, 50)], m, w, h)
    with pytest.raises(C.VBNMFError, match="connectivity") as ei:
        parts[0].ml_run(Itmax=5, criterion="connectivity", ncnn_step=2)
    assert ei.value.code == 5 and "vbnmf_group_ml_run_connectivity" in str(ei.value)
    _close(*parts, comm, M)


def test_factorize_connectivity_over_a_cell_partitioned_engine():
    """The call the drivers make; a world of one builds an unpartitioned engine, so this covers factorize()'s dispatch to
    ``ml_run_connectivity``, not the partitioned step (the tests above do that)."""
    import ccfindr_amd as C
    from ccfindr_amd.parallel import CellPartitionedEngine
    X = counts(60, 80, 0.9, seed=55)
    kw = dict(ranks=[2, 3], nrun=2, verbose=0, seed=7, criterion="connectivity", ncnn_step=5, Itmax=300)
    plain = C.factorize(X, **kw)
    part = C.factorize(X, engine_factory=lambda M, r: CellPartitionedEngine(M, r), **kw)
    assert part.nsteps == plain.nsteps and all(s < 300 for runs in plain.nsteps for s in runs)      # (the rule stopped every run)
    for a, b in zip(part.basis + part.coeff, plain.basis + plain.coeff):
        assert relerr(a, b) <= 1e-9
