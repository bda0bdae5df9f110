"""Seeded engine configurations for the option sweep (tests/test_config_sweep_cpu.py, tests/test_gpu_config_sweep.py).

``draw_config(seed, **pins)`` is a pure function of its arguments (numpy ``default_rng``): one case -- a matrix, a rank and its
row width, hyper-parameters, a fudge, the engine's options (pad_rank, grid, a planned geometry class, cell order, a forced
geometry) and a path (resident steps, the device loop, a batch, a partitioned group, the ML step / loop / batch, or device
initialisation followed by steps).  ``pins`` fix some dimensions; the seed draws the others.  Combinations the API refuses are
never drawn: ML, SVD and batches on partitioned engines, batches wider than 16 columns.

``CASES`` is the committed list: a covering set in which every tuple of ``REQUIRED`` has a case of its own.

The comparison helpers hold a device result to the oracle's: NaN positions must agree, and with fudge = 0 the factors lw / lh
are held to max(bound, 2e-15 |psi(alpha)|) per element (tests/util_special.py: the device digamma's absolute error is a relative
error of exp(psi), and |psi| grows without bound as alpha -> 0); every other bound is the caller's.
"""
import os
from contextlib import contextmanager

import numpy as np

EPS = float(np.finfo(np.float64).eps)
PADDED_WIDTHS = tuple(range(2, 33, 2)) + (40, 48, 56, 64, 80, 96, 112, 128)
NS = (1, 2, 7, 33, 64, 65, 130, 257, 400)
MS = (1, 3, 16, 63, 64, 65, 129, 300, 700)
LAMBDAS = (0.05, 0.3, 1.0, 4.0)
HYPER_VALUES = (0.05, 0.5, 1.0, 3.0, 40.0)            # test_gpu_random_cases.draw
KINDS = ("counts", "binary", "twos", "ones_twos", "ones_big", "noninteger", "split")
STRETCH_KINDS = ("binary", "twos", "ones_twos", "ones_big")
FUDGES = (EPS, 1e-3, 0.0)
VB_PATHS = ("steps", "run", "batch", "group", "init")
ML_PATHS = ("ml_steps", "ml_run", "batch_ml")
PATHS = VB_PATHS + ML_PATHS
BATCH_PATHS = ("batch", "batch_ml")
BATCH_MAX_WIDTH = 16                                   # rank.h kBatchMaxPaddedRank
# forced geometries (VBNMF_LDS_KB, VBNMF_NWG, VBNMF_MAX_LEN): small LDS blocks, few workgroups (not a multiple of 8), short tasks
FORCED = ((32, 5, 16), (48, 3, 8), (64, 9, 32))
FORCED_KEYS = ("VBNMF_LDS_KB", "VBNMF_NWG", "VBNMF_MAX_LEN")


def padded_rank(r):
    """common.h padded_rank: even up to 32, then multiples of 8 (to 64) and of 16 (to 128)."""
    return (r + 1) & ~1 if r <= 32 else ((r + 7) & ~7 if r <= 64 else (r + 15) & ~15)


def lane_share(R):
    """common.h rank_shares: lanes of the sweep that share one task at row width R."""
    return 1 if R <= 32 else (2 if R <= 64 else 4)


def layout_of(kind):
    """How the sweep stores the values: 'packed' (14-bit counts), 'wide' (fp64 values), 'split' (counts beyond 16 383, packed
    in pieces)."""
    return "wide" if kind == "noninteger" else ("split" if kind == "split" else "packed")


def _rank_of_width(rng, W):
    lo = 1 if W == 2 else (W - 1 if W <= 32 else (W - 7 if W <= 64 else W - 15))
    return int(rng.integers(lo, W + 1))


def _matrix(rng, n, m, kind, lam, extra):
    if kind == "binary":
        X = (rng.random((n, m)) < 0.3).astype(np.float64)
        base = 1.0
    elif kind == "twos":
        X = 2.0 * (rng.random((n, m)) < 0.3)
        base = 2.0
    elif kind == "ones_twos":                          # ones and twos in a proportion that varies by gene
        p2 = rng.uniform(0.05, 0.9, size=(n, 1))
        X = (rng.random((n, m)) < 0.3) * (1.0 + (rng.random((n, m)) < p2))
        base = 1.0
    elif kind == "ones_big":                           # mostly ones, a heavy tail
        X = (rng.random((n, m)) < 0.3).astype(np.float64)
        big = rng.random((n, m)) < 0.05
        X[big] = rng.integers(2, 60, size=int(big.sum())).astype(np.float64)
        base = 1.0
    elif kind == "noninteger":
        X = rng.poisson(lam, size=(n, m)) * rng.uniform(0.5, 1.5, size=(1, m))
        base = 0.75
    else:                                              # "counts" or "split" (one each of 16 383, 16 384 and beyond, below)
        X = rng.poisson(lam, size=(n, m)).astype(np.float64)
        base = 1.0
    X = np.array(X, dtype=np.float64)
    X[X.sum(axis=1) == 0, int(rng.integers(0, m))] = base       # no empty gene or cell unless the case asks for one
    X[int(rng.integers(0, n)), X.sum(axis=0) == 0] = base
    if kind == "split":
        for v in (16383.0, 16384.0, float(16385 + rng.integers(0, 200000))):
            X[int(rng.integers(0, n)), int(rng.integers(0, m))] = v
    if extra == "dense_gene":
        X[int(rng.integers(0, n)), :] = base
    elif extra == "zero_gene" and n > 1:
        X[int(rng.integers(0, n)), :] = 0.0
    elif extra == "zero_cell" and m > 1:
        X[:, int(rng.integers(0, m))] = 0.0
    if not X.any():
        X[0, 0] = base
    return np.asfortranarray(X)


def _cuts(rng, m, P):
    """P consecutive column ranges covering [0, m), one of them a single cell."""
    one = int(rng.integers(0, P))
    sizes = np.ones(P, dtype=np.int64)
    others = [q for q in range(P) if q != one]
    sizes[others] += rng.multinomial(m - P, np.full(len(others), 1.0 / len(others)))
    ends = np.cumsum(sizes)
    return [(int(e - s), int(e)) for s, e in zip(sizes, ends)]


def draw_config(seed, **pins):
    """One case: a dict of plain Python values (the matrix itself is ``case_matrix(case)``)."""
    rng = np.random.default_rng([20261016, int(seed)])
    c = {"seed": int(seed)}

    def pick(key, choices, p=None):
        if key in pins:
            c[key] = pins[key]
        else:
            v = choices[int(rng.choice(len(choices), p=p))]
            c[key] = v.item() if isinstance(v, np.generic) else v
        return c[key]

    path = pick("path", PATHS)
    batch, ml = path in BATCH_PATHS, path in ML_PATHS
    pick("kind", KINDS)
    pick("lam", LAMBDAS)
    pick("extra", (None, "dense_gene", "zero_gene", "zero_cell") if path in ("steps", "run", "init", "ml_steps")
         else (None, "dense_gene"))
    pick("n", NS)
    pick("m", MS if path != "group" else tuple(v for v in MS if v >= 16))
    # the row width: every padded width equally likely (a batch: at most 16), then a rank of that width
    W = pick("width", tuple(w for w in PADDED_WIDTHS if not batch or w <= BATCH_MAX_WIDTH))
    c["rank"] = int(pins["rank"]) if "rank" in pins else _rank_of_width(rng, W)
    pad = batch or (path != "group" and rng.random() < 0.3)
    c["pad_rank"] = W if pad else None
    c["width"] = W if pad else padded_rank(c["rank"])
    c["hyper"] = {k: float(rng.choice(HYPER_VALUES)) for k in ("aw", "bw", "ah", "bh")}
    pick("fudge", FUDGES)
    if ml:
        c["fudge"] = EPS
    c["ml"] = {"prior": bool(rng.random() < 0.5), "gamma_a": float(rng.choice([0.5, 1.7, 2.5])),
               "gamma_b": float(rng.choice([0.6, 0.7, 1.0]))}
    pick("order", (0, 1))
    forced = pick("forced", (None,) + FORCED, p=[0.6, 0.4 / 3, 0.4 / 3, 0.4 / 3])
    c["forced"] = tuple(forced) if forced is not None else None
    # a narrow grid (a batch: engine.batch_grid) and a planned geometry class (a padded width >= the case's own)
    grid = None
    if batch:
        pick("B", (2, 3, 16))
        g = max(8, (256 // c["B"]) // 8 * 8)
        grid = (g, g)
    elif path != "group" and c["forced"] is None and rng.random() < 0.3:
        grid = (int(rng.choice([8, 16, 64])), int(rng.choice([8, 16, 64])))
    c["grid"] = grid
    geo = None
    if path != "group" and rng.random() < 0.25:
        above = [w for w in PADDED_WIDTHS if w >= c["width"]]
        geo = int(above[int(rng.integers(0, len(above)))])
    c["geometry_rank"] = geo
    if batch:                                           # mixed ranks of one width, the case's rank first
        c["ranks"] = [c["rank"]] + [int(rng.integers(1, W + 1)) for _ in range(c["B"] - 1)]
    if path == "group":
        c["cuts"] = _cuts(rng, c["m"], pick("P", (2, 3, 8)))
    if path in ("run", "batch", "group"):
        c["loop"] = {"Itmax": 12 if path == "group" else int(rng.integers(1, 13)), "n0": int(rng.choice([0, 1, 3, 5])),
                     "dn": int(rng.choice([1, 2, 3])), "flags": tuple(bool(v) for v in rng.random(4) < 0.6)}
    if path in ("ml_run", "batch_ml"):
        c["loop"] = {"Itmax": int(rng.integers(1, 13))}
    c["state_seed"] = int(rng.integers(0, 2 ** 31))
    c["init_seed"] = int(rng.integers(0, 2 ** 63))
    c["matrix_seed"] = int(rng.integers(0, 2 ** 31))
    return c


def case_matrix(c):
    return _matrix(np.random.default_rng(c["matrix_seed"]), c["n"], c["m"], c["kind"], c["lam"], c["extra"])


def case_env(c):
    """The environment switches a case's layouts are cut under."""
    env = {"VBNMF_CELL_ORDER": str(c["order"])}
    if c["forced"] is not None:
        env.update({k: str(v) for k, v in zip(FORCED_KEYS, c["forced"])})
    return env


@contextmanager
def switches(env):
    """Sets ``env`` for the block (the layout switches are read when a layout is cut) and restores it after."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def engine_kw(c):
    kw = {}
    if c["pad_rank"]:
        kw["pad_rank"] = c["pad_rank"]
    if c["grid"]:
        kw["grid"] = c["grid"]
    if c["geometry_rank"]:
        kw["geometry_rank"] = c["geometry_rank"]
    return kw


def layout_rank(c):
    """The rank whose geometry the case's layouts are cut for."""
    return max(c["width"], c["geometry_rank"] or 0)


def case_id(c):
    parts = [c["path"], f"n{c['n']}m{c['m']}", f"r{c['rank']}w{c['width']}", c["kind"]]
    if c["extra"]:
        parts.append(c["extra"])
    if c["order"]:
        parts.append("ordered")
    if c["forced"]:
        parts.append("forced" + "-".join(map(str, c["forced"])))
    if c["fudge"] != EPS:
        parts.append(f"fudge{c['fudge']:g}")
    return "_".join(parts) + f"_s{c['seed']}"


# ---- the covering set ----------------------------------------------------------------------------------------------------
def _required():
    req = []
    vb_cycle = ("steps", "run", "group", "init")
    for q, W in enumerate(PADDED_WIDTHS):                                   # every row width on a VB path
        req.append(("width", dict(width=W, path=vb_cycle[q % 4])))
    for R in (16, 48, 96):                                                  # every lane-sharing mode x value layout
        for q, kind in enumerate(("counts", "noninteger", "split")):
            req.append(("sp_layout", dict(width=R, kind=kind, path=("steps", "ml_steps", "run")[q])))
    for path in PATHS:                                                      # every path, ordered and not
        for order in (0, 1):
            req.append(("path_order", dict(path=path, order=order)))
    for q, forced in enumerate(FORCED):                                     # forced geometries on batch, group and ML paths
        for path in ("batch", "group", ML_PATHS[q]):
            req.append(("forced", dict(forced=forced, path=path)))
    for fudge in (0.0, 1e-3):                                               # the fudge edges on loops
        for path in ("run", "batch", "group"):
            req.append(("fudge", dict(fudge=fudge, path=path)))
    for kind in STRETCH_KINDS:                                              # stretch-shaped values on VB and ML
        for path in ("steps", "ml_run"):
            req.append(("stretch", dict(kind=kind, path=path)))
    return req


REQUIRED = _required()
CASES = [draw_config(1000 + q, **pins) for q, (_, pins) in enumerate(REQUIRED)]


# ---- comparison helpers --------------------------------------------------------------------------------------------------
def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300), initial=0.0))


def nan_relerr(a, b):
    """Relative error over the non-NaN entries; NaN positions must agree."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), f"NaN at different positions: {np.argwhere(na != nb)[:5].tolist()}"
    return relerr(a[~na], b[~na])


def psi_bound(ref, name, fudge, bound):
    """Per-element relative bound of factor ``name`` of the oracle's state ``ref``: ``bound``, or with fudge = 0 for lw / lh
    max(bound, 2e-15 |psi(alpha)|), alpha = ew / bew = ew^2 / dw (resp. eh^2 / dh)."""
    if fudge != 0.0 or name not in ("lw", "lh"):
        return bound
    from scipy.special import digamma
    e, d = (ref["ew"], ref["dw"]) if name == "lw" else (ref["eh"], ref["dh"])
    with np.errstate(divide="ignore", invalid="ignore"):
        b = np.maximum(bound, 2e-15 * np.abs(digamma(e * e / d)))
    return np.where(np.isfinite(b), b, bound)


def check_factors(got, ref, bound, fudge, what):
    """Every factor of ``got`` within the (fudge-aware) relative bound of the oracle's ``ref``; NaN positions equal."""
    for k in ("lw", "lh", "ew", "eh", "dw", "dh"):
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        na, nb = np.isnan(a), np.isnan(b)
        assert np.array_equal(na, nb), (what, k, "NaN positions differ")
        with np.errstate(invalid="ignore"):
            err = np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
        lim = np.broadcast_to(psi_bound(ref, k, fudge, bound), b.shape)
        bad = ~na & (err > lim)
        assert not bad.any(), (what, k, float(np.max(err[~na], initial=0.0)), np.argwhere(bad)[:3].tolist())
