"""The map of the cells: mirror of the reference's ``visualize_clusters`` (R/utils.R:692-712) without the drawing.

The reference hands ``t(h)`` to ``Rtsne`` (:700), a CPU package that is Barnes-Hut by default.  Here the t-SNE authors' EXACT
algorithm (``theta = 0``) runs on the device in fp64 with fixed summation trees (csrc/tsne.h): the affinities at
creation, then per iteration a force launch that recomputes every ``P_ij`` and an update launch.  No n x n array exists.  No CPU
fallback: without a device ``TSNE`` raises ``VBNMFError`` (status 2).

``neighbors="auto"`` or an int selects the neighbour-limited path instead (csrc/tsne_knn.h): an exact k-nearest-
neighbour search on the device, ``P`` supported on that graph and stored sparse, the attraction a sum over the stored rows, the
repulsion still exact over all pairs of ``Y``.  The dense path is the default.

Deviations: the start ``Y`` comes from ``numpy.random.default_rng(seed)`` (or ``Y_init=``), not from R's stream; no PCA (for
d <= 50 ``Rtsne``'s is a rotation and leaves the distances unchanged).  ``Rtsne`` is not pinned: it cannot run where this does.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np

from . import _native as N
from .post import cluster_id

DEFAULTS = dict(max_iter=1000, eta=200.0, exaggeration=12.0, stop_lying_iter=250, mom_switch_iter=250, momentum=0.5,
                final_momentum=0.8, min_gain=0.01, cost_every=50)
_INFO = ("wave_width", "workgroup_size", "i_block", "j_tile", "lds_row_capacity", "affinity_grid", "force_grid", "update_workgroup_size")
_TIMES = ("normalise", "upload", "affinities", "loop", "read_back", "last_force", "last_update")
_KNN_INFO = ("neighbor_limit", "workgroup_size", "lds_row_capacity", "repulse_tile", "repulse_i_block", "attract_rows", "neighbors", "nnz",
             "longest_row", "attract_grid")
_KNN_TIMES = ("search", "pattern", "last_attract", "last_repulse", "last_update")


def _i32p(a):
    return a.ctypes.data_as(N.c_int32_p)


def _i64p(a):
    return a.ctypes.data_as(N.c_int64_p)


def _pairs(a, n, what):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != (n, 2):
        raise ValueError(f"{what} must be {n} x 2, not {a.shape}")
    return a


def _info(call, handle, names, ints, intp, time_names):
    times = np.zeros(len(time_names), dtype=np.float64)
    N.check(call(handle._h if handle is not None else None, intp(ints), N.dptr(times)))
    out = {k: int(v) for k, v in zip(names, ints)}
    out["times_ms"] = dict(zip(time_names, (float(v) for v in times)))
    return out


def tsne_info(handle=None):
    """Constants of the kernels (``vbnmf_tsne_info``), with the grids and ``times_ms`` of ``handle`` (a ``TSNE``) if given."""
    return _info(N.load().vbnmf_tsne_info, handle, _INFO, np.zeros(len(_INFO), dtype=np.int32), _i32p, _TIMES)


def _neighbors_arg(neighbors):
    """None -> None (dense); "auto" -> 0 (floor(3 perplexity), resolved by the library); an int -> itself."""
    if neighbors is None:
        return None
    if isinstance(neighbors, str):
        if neighbors != "auto":
            raise TypeError(f"neighbors must be None, 'auto' or an int, not {neighbors!r}")
        return 0
    if isinstance(neighbors, (bool, np.bool_)) or not isinstance(neighbors, (int, np.integer)):
        raise TypeError(f"neighbors must be None, 'auto' or an int, not {neighbors!r}")
    if int(neighbors) < 1:
        raise N.VBNMFError(N.ERR_BAD_ARG, f"neighbors = {int(neighbors)} is outside [1, n - 1]")
    return int(neighbors)


def tsne_knn_info(handle=None):
    """Constants of the neighbour kernels (``vbnmf_tsne_knn_info``), with K, nnz, the longest row, the attraction grid and
    ``times_ms`` of ``handle`` (a ``TSNE`` with neighbours) if given; without one ``times_ms["search"]`` is the calling thread's
    last search."""
    return _info(N.load().vbnmf_tsne_knn_info, handle, _KNN_INFO, np.zeros(len(_KNN_INFO), dtype=np.int64), _i64p, _KNN_TIMES)


def knn(x, k, device=None):
    """The exact ``k`` nearest neighbours of every row of ``x`` (points x coordinates, as given) on the device -> (idx, dist),
    n x k each: the indices j != i with the smallest (squared distance, j), in that order, and the squared distances."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("x must be a matrix: points x coordinates")
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
        raise TypeError(f"k must be an int, not {k!r}")
    n, d = x.shape
    shape = (n, min(max(int(k), 1), max(n, 1)))          # (a k out of range: the library says so before it writes)
    idx, dist = np.zeros(shape, dtype=np.int32), np.zeros(shape)
    N.check(N.load().vbnmf_knn(0 if device is None else int(device), n, d, N.dptr(x), int(k), _i32p(idx), N.dptr(dist)))
    return idx, dist


class TSNE:
    """The resident handle: ``x`` (n points x d) and its affinities on the device.  ``beta``, ``sum_p``, ``trips`` are the
    bisection's results per point; ``set_state`` / ``state`` move ``Y``, ``uY``, ``gains``; ``forces`` evaluates the current
    ``Y`` and changes nothing; ``run`` iterates.  ``neighbors``: None is the dense handle, ``"auto"`` (floor(3 perplexity)) or
    an int the neighbour-limited one, which also has ``knn()``, ``sparse_p()`` and ``knn_info()``."""

    def __init__(self, x, perplexity=30.0, normalize=True, device=None, neighbors=None):
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 2:
            raise ValueError("x must be a matrix: points x coordinates")
        self.n, self.d = x.shape
        self._h = None
        self.neighbors = None
        k = _neighbors_arg(neighbors)
        h = ctypes.c_void_p()
        dev = 0 if device is None else int(device)
        args = (dev, self.n, self.d, N.dptr(x), float(perplexity), 1 if normalize else 0)
        N.check(N.load().vbnmf_tsne_create(*args, ctypes.byref(h)) if k is None else N.load().vbnmf_tsne_create_knn(*args, k, ctypes.byref(h)))
        self._h = h
        if k is not None:
            self.neighbors = tsne_knn_info(self)["neighbors"]
        self.beta = np.zeros(self.n)
        self.sum_p = np.zeros(self.n)
        self.trips = np.zeros(self.n, dtype=np.int32)
        N.check(N.load().vbnmf_tsne_affinity(self._h, N.dptr(self.beta), N.dptr(self.sum_p), _i32p(self.trips)))
        self.iteration = 0                    # iterations run since the last set_state

    def close(self):
        if self._h is not None:
            N.load().vbnmf_tsne_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass

    def info(self):
        return tsne_info(self)

    def _need_neighbors(self):
        if self.neighbors is None:
            raise N.VBNMFError(N.ERR_STATE, "a dense handle has no neighbour lists: create it with neighbors='auto' or an int")

    def knn_info(self):
        self._need_neighbors()
        return tsne_knn_info(self)

    def knn(self):
        """-> (idx, dist), n x K each: every point's neighbours by ascending (squared distance, index) and those distances."""
        self._need_neighbors()
        idx, dist = np.zeros((self.n, self.neighbors), dtype=np.int32), np.zeros((self.n, self.neighbors))
        N.check(N.load().vbnmf_tsne_neighbors(self._h, _i32p(idx), N.dptr(dist)))
        return idx, dist

    def sparse_p(self):
        """-> the stored ``P`` as a ``scipy.sparse.csr_matrix`` (n x n, sorted indices, symmetric bit for bit)."""
        import scipy.sparse as sp
        self._need_neighbors()
        nnz, indptr = ctypes.c_int64(0), np.zeros(self.n + 1, dtype=np.int64)
        N.check(N.load().vbnmf_tsne_sparse_p(self._h, ctypes.byref(nnz), _i64p(indptr), None, None))
        indices, values = np.zeros(nnz.value, dtype=np.int32), np.zeros(nnz.value)
        N.check(N.load().vbnmf_tsne_sparse_p(self._h, None, None, _i32p(indices), N.dptr(values)))
        return sp.csr_matrix((values, indices, indptr), shape=(self.n, self.n))

    def set_state(self, Y, uY=None, gains=None):
        """``uY`` None: 0, ``gains`` None: 1 (the start of the descent).  Resets the iteration count."""
        Y, uY, gains = _pairs(Y, self.n, "Y"), _pairs(uY, self.n, "uY"), _pairs(gains, self.n, "gains")
        N.check(N.load().vbnmf_tsne_set_state(self._h, N.dptr(Y), N.dptr(uY), N.dptr(gains)))
        self.iteration = 0

    def state(self):
        """-> (Y, uY, gains), n x 2 each."""
        out = [np.zeros((self.n, 2)) for _ in range(3)]
        N.check(N.load().vbnmf_tsne_get_state(self._h, *(N.dptr(a) for a in out)))
        return tuple(out)

    def forces(self, exaggeration=1.0):
        """-> dict A (n x 2, times ``exaggeration``), R (n x 2), z (n), cost_i (n) on the current ``Y``."""
        A, R, z, c = np.zeros((self.n, 2)), np.zeros((self.n, 2)), np.zeros(self.n), np.zeros(self.n)
        N.check(N.load().vbnmf_tsne_forces(self._h, float(exaggeration), N.dptr(A), N.dptr(R), N.dptr(z), N.dptr(c)))
        return {"A": A, "R": R, "z": z, "cost_i": c}

    def run(self, n_iter, first_iter=None, eta=200.0, exaggeration=12.0, stop_lying_iter=250, mom_switch_iter=250, momentum=0.5,
            final_momentum=0.8, min_gain=0.01, cost_every=50):
        """Iterations ``first_iter`` (default: where the last ``run`` stopped) ``.. first_iter + n_iter - 1`` of the schedule.
        -> (iterations, costs): the cost after every iteration divisible by ``cost_every`` and after the last."""
        first = self.iteration + 1 if first_iter is None else int(first_iter)
        cap = max(int(n_iter), 1)
        costs, iters, cnt = np.zeros(cap), np.zeros(cap, dtype=np.int32), ctypes.c_int32(0)
        N.check(N.load().vbnmf_tsne_run(self._h, first, int(n_iter), float(exaggeration), int(stop_lying_iter), int(mom_switch_iter),
                                        float(momentum), float(final_momentum), float(eta), float(min_gain), int(cost_every),
                                        N.dptr(costs), _i32p(iters), ctypes.byref(cnt)))
        self.iteration = first + int(n_iter) - 1
        return iters[:cnt.value].copy(), costs[:cnt.value].copy()


@dataclass
class Embedding:
    Y: np.ndarray                       # n x 2
    itercosts: np.ndarray               # the cost after the iterations ``cost_iters``
    cost_iters: np.ndarray
    costs: np.ndarray                   # per point, of the final Y; sums to itercosts[-1] up to rounding
    beta: np.ndarray
    trips: np.ndarray
    info: dict = field(default_factory=dict)
    neighbors: object = None            # K of the neighbour-limited path, None for the dense one


def tsne(x, perplexity=30.0, normalize=True, device=None, seed=None, Y_init=None, max_iter=1000, neighbors=None, **schedule):
    """Exact t-SNE of the rows of ``x`` into the plane.  ``schedule``: eta, exaggeration, stop_lying_iter, mom_switch_iter,
    momentum, final_momentum, min_gain, cost_every (``DEFAULTS``).  The start is ``1e-4 * standard_normal`` from
    ``numpy.random.default_rng(seed)``, or ``Y_init``.  ``neighbors``: as for ``TSNE``; None is the dense path."""
    bad = set(schedule) - (set(DEFAULTS) - {"max_iter"})
    if bad:
        raise TypeError(f"unknown t-SNE arguments: {sorted(bad)}")
    with TSNE(x, perplexity=perplexity, normalize=normalize, device=device, neighbors=neighbors) as T:
        Y0 = 1e-4 * np.random.default_rng(seed).standard_normal((T.n, 2)) if Y_init is None else Y_init
        T.set_state(Y0)
        iters, costs = T.run(int(max_iter), **schedule)
        Y = T.state()[0]
        per_point = T.forces(1.0)["cost_i"]
        return Embedding(Y=Y, itercosts=costs, cost_iters=iters, costs=per_point, beta=T.beta, trips=T.trips, info=T.info(),
                         neighbors=T.neighbors)


@dataclass
class ClusterMap:
    rank: int
    Y: np.ndarray                       # cells x 2 (tsne$Y of R/utils.R:700)
    cid: np.ndarray                     # 1-based cluster of every cell (:701)
    counts: dict                        # table(cid) (:708): cluster -> cells, over the clusters that occur, ascending
    names: list                         # rownames(h) (:708): the clusters' labels, "1" .. "r"
    embedding: object = None


def visualize_clusters(result, rank=None, embed=None, **tsne_args):
    """``visualize_clusters(object, rank, ...)``; reference R/utils.R:692-712 without the two plots (:705-710).  ``result`` is a
    ``VBResult``, ``MLResult``, ``Projection`` or ``VBProjection``; ``tsne_args`` go to ``tsne`` as ``...`` goes to ``Rtsne``.
    ``embed`` replaces ``tsne`` (anything that maps a cells x r matrix to an object with ``Y``)."""
    if rank is None:                                                                # :695-698
        rank = result.ranks[0]
    cid = cluster_id(result, rank)                                                  # :699 (IndexError if absent), :701
    h = np.asarray(result.coeff[[i for i, r in enumerate(result.ranks) if r == rank][0]], dtype=np.float64)
    emb = (tsne if embed is None else embed)(np.ascontiguousarray(h.T), **tsne_args)    # :700
    ids, cnt = np.unique(cid, return_counts=True)                                   # :708 table(cid)
    return ClusterMap(rank=int(rank), Y=np.asarray(emb.Y), cid=cid, counts={int(k): int(v) for k, v in zip(ids, cnt)},
                      names=[str(k + 1) for k in range(h.shape[0])], embedding=emb)
