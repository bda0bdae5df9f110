#!/usr/bin/env python3
"""tests/manual_tsne_knn_times.py -- the neighbour-limited t-SNE of csrc/tsne_knn.h timed on one MI355X next to the dense path
of csrc/tsne.h on the same data, in the same call, alternating.  Run by hand, like the other manual_* files:

    python tests/manual_tsne_knn_times.py [output file, default profiles/tsne_knn_times.txt] [small]

Per size (n = 5 000, 20 000, 50 000 cells; d = 10 and 20 coordinates; perplexity 30, K = 90): the search with the bisection
(device events), the search by itself (vbnmf_knn, device events; the bisection is the difference), the pattern (host clock:
read-back, build, upload), nnz and the longest row; then, alternating, a run of the neighbour handle and a run of the dense
handle: ms per iteration of each and the last iteration's launches each by itself (device events).  Each new kernel stands next
to its floor: the search and the repulsion against ordered pairs x counted fp64 operations / the fp64 vector peak, the
attraction against the bytes of the stored rows / the HBM peak.  No number is asserted.  ``small`` stops after n = 5 000.
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import util_tsne as T  # noqa: E402

import ccfindr_amd as C  # noqa: E402

FP64_PEAK = 78.6e12          # flop / s, the MI355X's specified fp64 vector peak (an FMA counts 2)
HBM_PEAK = 8.0e12            # bytes / s, the specified HBM3E peak
REPS = 5
REPULSE_OPS = 2 + 2 + 2 + 10 + 1 + 2 + 3      # d0 d1; their squares; 1 + . + .; the IEEE division at about 10; w w; two products; three additions
LINES = []


def say(*a):
    line = " ".join(str(v) for v in a)
    LINES.append(line)
    print(line)
    sys.stdout.flush()


def med(v):
    v = sorted(v)
    return "median %8.3f  min %8.3f  max %8.3f" % (v[len(v) // 2], v[0], v[-1])


def mid(v):
    return sorted(v)[len(v) // 2]


def one_size(n, d, iters):
    X, _ = T.clusters(n, d, 5, seed=1)
    Xn = T.normalise(X)
    C.knn(Xn, 90)                                        # warm-up: the code object, the buffer pool
    t = time.perf_counter()
    hk = C.TSNE(X, perplexity=30.0, neighbors="auto")
    wall = time.perf_counter() - t
    ki = hk.knn_info()
    K, nnz = ki["neighbors"], ki["nnz"]
    C.knn(Xn, K)
    alone = C.tsne_knn_info()["times_ms"]["search"]
    pairs = float(n) * (n - 1)
    floor_s = pairs * 3 * d / FP64_PEAK * 1e3
    say(f"n={n} d={d} K={K}: create {wall * 1e3:.1f} ms wall; search with the bisection (device events) {ki['times_ms']['search']:.2f} ms, the search "
        f"by itself (vbnmf_knn) {alone:.2f} ms: the difference, the bisection, is {ki['times_ms']['search'] - alone:+.2f} ms (inside the spread of "
        f"two launches where it is negative); pattern on the host "
        f"{ki['times_ms']['pattern']:.1f} ms; nnz {nnz} ({nnz / n:.1f} a row), longest row {ki['longest_row']}; trips mean {hk.trips.mean():.1f} max {hk.trips.max()}")
    say(f"    floor of the search: {pairs:.3g} ordered pairs x {3 * d} fp64 operations of D (the selection is integer work) / {FP64_PEAK / 1e12:.1f} Tflop/s "
        f"= {floor_s:.3f} ms -> the kernel runs at {100.0 * floor_s / ki['times_ms']['search']:.2f} % of it")
    t = time.perf_counter()
    hd = C.TSNE(X, perplexity=30.0)
    say(f"    dense handle: create {(time.perf_counter() - t) * 1e3:.1f} ms wall, affinities (device events) {hd.info()['times_ms']['affinities']:.2f} ms")
    Y0 = T.start(n, 0)
    for h in (hk, hd):
        h.set_state(Y0)
        h.run(2, cost_every=0)                           # warm-up: code objects
    loop_k, loop_d, att, rep, upd, force_d = [], [], [], [], [], []
    for _ in range(REPS):                                # alternating: the two paths see the same state of the part
        hk.set_state(Y0)
        hk.run(iters, cost_every=0)
        loop_k.append(hk.info()["times_ms"]["loop"] / iters)
        tm = hk.knn_info()["times_ms"]
        att.append(tm["last_attract"])
        rep.append(tm["last_repulse"])
        upd.append(tm["last_update"])
        hd.set_state(Y0)
        hd.run(iters, cost_every=0)
        tm = hd.info()["times_ms"]
        loop_d.append(tm["loop"] / iters)
        force_d.append(tm["last_force"])
    floor_r = pairs * REPULSE_OPS / FP64_PEAK * 1e3
    floor_a = (nnz * 12.0 + (n + 1) * 8.0) / HBM_PEAK * 1e3
    say(f"    {iters} iterations, {REPS} runs each, alternating, ms per iteration:")
    say(f"      neighbour path: {med(loop_k)}")
    say(f"      dense path:     {med(loop_d)}   -> neighbour / dense = {mid(loop_k) / mid(loop_d):.3f}")
    say(f"    last iteration's launches (device events): attraction {med(att)}")
    say(f"                                               repulsion  {med(rep)}")
    say(f"                                               update     {med(upd)}")
    say(f"                                               dense force {med(force_d)}")
    say(f"    floor of the repulsion: {pairs:.3g} ordered pairs x {REPULSE_OPS} counted fp64 operations / {FP64_PEAK / 1e12:.1f} Tflop/s = {floor_r:.3f} ms "
        f"-> the kernel runs at {100.0 * floor_r / mid(rep):.1f} % of it")
    say(f"    floor of the attraction: {nnz} stored entries x 12 bytes + the row pointers / {HBM_PEAK / 1e12:.0f} TB/s = {floor_a * 1e3:.2f} us "
        f"-> the kernel runs at {100.0 * floor_a / mid(att):.1f} % of it")
    hk.close()
    hd.close()


def main():
    args = [a for a in sys.argv[1:] if a != "small"]
    small = "small" in sys.argv[1:]
    out = args[0] if args else os.path.join(ROOT, "profiles", "tsne_knn_times.txt")
    say("profiles/tsne_knn_times.txt -- neighbour-limited t-SNE (csrc/tsne_knn.h: k_tsne_knn, k_tsne_attract, k_tsne_repulse) next to the dense")
    say("path (csrc/tsne.h) on one MI355X, one visit.  Written by tests/manual_tsne_knn_times.py.  Times by device events around the launches of")
    say("one stream unless a host clock is named.")
    say(f"kernel constants: { {k: v for k, v in C.tsne_knn_info().items() if k != 'times_ms'} }")
    say("")
    for n, iters in ((5000, 50), (20000, 10), (50000, 4)):
        for d in (10, 20):
            one_size(n, d, iters)
        say("")
        if small:
            break
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
