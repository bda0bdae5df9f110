#!/usr/bin/env python3
"""tests/manual_tsne_times.py -- the exact t-SNE of csrc/tsne.h (ccfindr_amd/embed.py) timed on one MI355X.  Run by hand, like
the other manual_* files:

    python tests/manual_tsne_times.py [output file, default profiles/tsne_times.txt] [small]

Per size (n = 5 000, 20 000, 50 000 cells; d = 10 and 20 coordinates): the affinity launch (device events), then a run's time
per iteration and the last iteration's force and update launch each by itself (device events, vbnmf_tsne_info), after a
warm-up run.  Each force time stands next to its floor: ordered pairs x counted fp64 operations / the part's fp64 vector peak.
Last, the numpy restatement of tests/util_tsne.py per iteration at n = 2 000 on the same host.  No number is asserted.
``small`` stops after n = 5 000.
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

FP64_PEAK = 78.6e12          # flop / s, the MI355X's specified fp64 vector peak (an FMA counts 2: 39.3e12 instructions' worth)
HBM_PEAK = 8.0e12            # bytes / s, the specified HBM3E peak
REPS = 5
LINES = []


def say(*a):
    line = " ".join(str(v) for v in a)
    LINES.append(line)
    print(line)
    sys.stdout.flush()


def med(v):
    v = sorted(v)
    return "median %8.3f  min %8.3f  max %8.3f" % (v[len(v) // 2], v[0], v[-1])


def counted_ops(d):
    """fp64 operations of one ordered pair in k_tsne_force, cost sums off.  D: d subtractions, d products, d additions (no
    contraction: -ffp-contract=off).  Two exponentials at about 25 operations each (argument product, reduction, an 11-term
    polynomial, scaling), 2 products with 1/S, 1 addition, 1 product with 1/(2n); w: 2 subtractions, 2 products, 2 additions,
    a division at about 10; P w, w w, 4 products, 5 additions."""
    width = 8 if d <= 8 else 16 if d <= 16 else 32 if d <= 32 else d
    return 3 * width + 2 * 25 + 4 + 6 + 10 + 2 + 4 + 5


def one_size(n, d, iters):
    X, _ = T.clusters(n, d, 5, seed=1)
    t = time.perf_counter()
    h = C.TSNE(X, perplexity=30.0)
    wall = time.perf_counter() - t
    info = h.info()
    tm = info["times_ms"]
    say(f"n={n} d={d}: create {wall * 1e3:.1f} ms wall: normalise {tm['normalise']:.2f}, upload {tm['upload']:.2f}, affinities (device events) "
        f"{tm['affinities']:.2f} ms; trips mean {h.trips.mean():.1f} max {h.trips.max()}; affinity grid {info['affinity_grid']}, force grid {info['force_grid']}")
    h.set_state(T.start(n, 0))
    h.run(2, cost_every=0)                               # warm-up: code objects
    loop, force, upd = [], [], []
    for _ in range(REPS):
        h.set_state(T.start(n, 0))
        h.run(iters, cost_every=0)
        tm = h.info()["times_ms"]
        loop.append(tm["loop"] / iters)
        force.append(tm["last_force"])
        upd.append(tm["last_update"])
    pairs = float(n) * (n - 1)
    ops = counted_ops(d)
    floor = pairs * ops / FP64_PEAK * 1e3
    fm = sorted(force)[REPS // 2]
    say(f"    {iters} iterations, {REPS} runs, ms per iteration: {med(loop)}")
    say(f"    force launch of the last iteration (device events): {med(force)}")
    say(f"    update launch of the last iteration:                {med(upd)}")
    say(f"    floor of the force kernel: {pairs:.3g} ordered pairs x {ops} counted fp64 operations / {FP64_PEAK / 1e12:.1f} Tflop/s = {floor:.3f} ms "
        f"-> the kernel runs at {100.0 * floor / fm:.1f} % of it; a stored fp64 P would be {pairs * 8 / 1e9:.2f} GB read per iteration, "
        f"{pairs * 8 / HBM_PEAK * 1e3:.3f} ms at the {HBM_PEAK / 1e12:.0f} TB/s HBM peak")
    h.close()


def numpy_statement(n, d):
    c = T.case(n, d, 5, 1)
    t = time.perf_counter()
    D = T.sq_dist(c["Xn"])
    beta, S, trips, _ = T.affinities(c["Xn"], 30.0, D)
    t_aff = time.perf_counter() - t
    P = T.joint_p(D, beta, S)
    t = time.perf_counter()
    T.run(P, T.start(n, 0), 5, cost_every=0)
    t_it = (time.perf_counter() - t) / 6                 # five iterations and the closing cost evaluation
    say(f"numpy restatement (tests/util_tsne.py) on this box's host, n={n} d={d}: affinities {t_aff:.2f} s, {t_it * 1e3:.0f} ms per iteration "
        f"(P stored: {n * n * 8 / 1e6:.0f} MB)")


def main():
    args = [a for a in sys.argv[1:] if a != "small"]
    small = "small" in sys.argv[1:]
    out = args[0] if args else os.path.join(ROOT, "profiles", "tsne_times.txt")
    say("profiles/tsne_times.txt -- exact t-SNE (csrc/tsne.h: k_tsne_affinity, k_tsne_force, k_tsne_update) on one MI355X, one visit.")
    say("Written by tests/manual_tsne_times.py.  Times by device events around the launches of one stream.")
    say(f"kernel constants: { {k: v for k, v in C.tsne_info().items() if k != 'times_ms'} }")
    say("")
    for n, iters in ((5000, 50), (20000, 10), (50000, 4)):
        for d in (10, 20):
            one_size(n, d, iters)
        say("")
        if small:
            break
    numpy_statement(2000, 10)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
