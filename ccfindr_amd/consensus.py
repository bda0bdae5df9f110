"""Consensus measures of ``factorize()`` (reference R/factorize.R:62-78, :218-230) from the label vectors of the runs,
at any cell count: the device accumulator behind ``vbnmf_consensus_*`` (include/vbnmf.h, csrc/consensus.h) keeps the
labels of every run and the integer sums the dispersion follows from; the cophenetic correlation is computed on the
distinct label tuples, on the host (csrc/consensus.cpp) up to ``DEFAULT_MAX_GROUPS`` of them and on the device
(csrc/cophenet.h) up to ``DEVICE_MAX_GROUPS``.  The O(m^2) pair vector of the reference is never formed.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N
from .engine import VBEngine

METHODS = ("average", "single", "complete")     # the linkages the grouped cophenetic serves
DEFAULT_MAX_GROUPS = 4096                       # distinct label tuples served on the host: a 128 MB distance matrix
DEVICE_MAX_GROUPS = 32768                       # ... on the device: two matrices, 17 GB of device memory
WHERE = {None: -1, "auto": -1, "host": 0, "device": 1}


def cophenetic_grouped(tuples, sizes, method="average", device=None):
    """Cophenetic correlation of ``G`` groups of cells: ``tuples`` [G][R] labels of each group in the R runs, ``sizes`` [G]
    cells per group; distance = Hamming distance of the tuples / R.  ``device``: None = on the host, else the HIP device
    that runs the agglomeration (the host's dendrogram, up to ``DEVICE_MAX_GROUPS`` groups).  NaN when either side has no
    variance."""
    L = N.load()
    T = np.ascontiguousarray(tuples, dtype=np.uint8)
    if T.ndim != 2:
        raise ValueError("tuples must be a G x R array")
    s = np.ascontiguousarray(sizes, dtype=np.int64)
    if s.shape != (T.shape[0],):
        raise ValueError("sizes must hold one count per group")
    out = ctypes.c_double()
    args = (T.shape[0], T.shape[1], T.ctypes.data_as(N.c_uint8_p), s.ctypes.data_as(N.c_int64_p), str(method).encode(), ctypes.byref(out))
    if device is None:
        N.check(L.vbnmf_cophenetic_grouped(*args))
    else:
        N.check(L.vbnmf_cophenetic_grouped_device(int(device), *args))
    return out.value


class Consensus:
    """Accumulator of the runs of one rank: ``add`` a run's labels, read ``dispersion()`` after any run and
    ``cophenetic()`` at the end.  ``max_runs`` rows of ``m`` labels live on device ``device``."""

    def __init__(self, m, rank, max_runs, device=0):
        L = N.load()
        self._lib = L
        self._h = ctypes.c_void_p()
        N.check(L.vbnmf_consensus_create(int(m), int(rank), int(max_runs), int(device), ctypes.byref(self._h)))
        self.m, self.rank, self.max_runs, self.device = int(m), int(rank), int(max_runs), int(device)

    def add(self, engine_or_labels):
        """The next run: a ``VBEngine`` (its arg-max labels are taken on the device, nothing is downloaded) or ``m`` host
        labels, 1-based, 0 = no label."""
        if isinstance(engine_or_labels, VBEngine):
            N.check(self._lib.vbnmf_consensus_add_engine(self._h, engine_or_labels._h))
            return
        ids = np.ascontiguousarray(engine_or_labels, dtype=np.int32)
        if ids.shape != (self.m,):
            raise ValueError(f"labels must hold {self.m} entries")
        N.check(self._lib.vbnmf_consensus_add_labels(self._h, ids.ctypes.data_as(N.c_int32_p)))

    def sums(self):
        """``{"runs", "s1", "s2", "unlabelled"}``: the integers behind the dispersion (Python ints)."""
        runs, unl = ctypes.c_int32(), ctypes.c_int32()
        s1, s2 = ctypes.c_uint64(), ctypes.c_uint64()
        N.check(self._lib.vbnmf_consensus_sums(self._h, ctypes.byref(runs), ctypes.byref(s1), ctypes.byref(s2), ctypes.byref(unl)))
        return {"runs": runs.value, "s1": s1.value, "s2": s2.value, "unlabelled": bool(unl.value)}

    def dispersion(self):
        """``dispersion(conav / runs, m)`` (R/factorize.R:62-67); NaN if any label was 0."""
        out = ctypes.c_double()
        N.check(self._lib.vbnmf_consensus_dispersion(self._h, ctypes.byref(out)))
        return out.value

    def cophenetic(self, method="average", max_groups=None, with_groups=False, where=None):
        """``cophenet(conav / runs, m, method)`` (R/factorize.R:69-78) on the distinct label tuples.  ``where``: 'host',
        'device', or None = by size: up to ``DEFAULT_MAX_GROUPS`` groups on the host, above that on the accumulator's
        device.  NaN past ``max_groups`` groups (None: ``DEFAULT_MAX_GROUPS`` on the host, ``DEVICE_MAX_GROUPS``
        otherwise; the device never serves more than ``DEVICE_MAX_GROUPS``).  ``with_groups``: return ``(coefficient,
        number of groups)``."""
        if where not in WHERE:
            raise ValueError("where must be None, 'host' or 'device'")
        out, groups = ctypes.c_double(), ctypes.c_int64()
        N.check(self._lib.vbnmf_consensus_cophenetic_on(self._h, str(method).encode(), 0 if max_groups is None else int(max_groups),
                                                        WHERE[where], ctypes.byref(out), ctypes.byref(groups)))
        return (out.value, groups.value) if with_groups else out.value

    def labels(self, run):
        """The labels of run ``run`` (0-based): ``m`` int32, 1-based, 0 = no label."""
        ids = np.empty(self.m, dtype=np.int32)
        N.check(self._lib.vbnmf_consensus_labels(self._h, int(run), ids.ctypes.data_as(N.c_int32_p)))
        return ids

    def reset(self):
        N.check(self._lib.vbnmf_consensus_reset(self._h))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.vbnmf_consensus_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass
