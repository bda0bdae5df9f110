"""The C ABI of the device-driven connectivity stopping rule (reference R/factorize.R:198-208) on a machine without a GPU:
vbnmf_engine_ml_run_connectivity and vbnmf_batch_ml_run_connectivity are exported, bound in ccfindr_amd/_native.py with the
header's arity, and refuse bad arguments with a status and a message before touching any device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"vbnmf_engine_ml_run_connectivity": 13, "vbnmf_batch_ml_run_connectivity": 14}


def _header_arity(name):
    text = open(os.path.join(ROOT, "include", "vbnmf.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
    assert m, f"{name} is not declared in include/vbnmf.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_entries_are_exported_and_bound_with_the_headers_arity(name):
    from ccfindr_amd import _native as N
    L = N.load()
    assert hasattr(L, name)
    restype, argtypes = N.SIGNATURES[name]
    assert restype is ctypes.c_int
    assert len(argtypes) == ENTRIES[name] == _header_arity(name)
    assert getattr(L, name).argtypes == argtypes


def test_header_cites_the_reference_rule():
    text = open(os.path.join(ROOT, "include", "vbnmf.h")).read()
    for name in ENTRIES:
        comment = text[:text.index("int " + name)].rsplit("/*", 1)[1]
        assert "R/factorize.R" in comment and "198-208" in comment, name


def test_null_handle_is_a_bad_argument_with_a_message():
    from ccfindr_amd import _native as N
    L = N.load()
    it, reason, lk = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double()
    rc = L.vbnmf_engine_ml_run_connectivity(None, 0, 1.0, 1.0, 10, 5, ctypes.byref(it), ctypes.byref(lk), ctypes.byref(reason),
                                            None, 0, None, 0)
    assert rc == N.ERR_BAD_ARG and b"NULL" in L.vbnmf_last_error()
    rc = L.vbnmf_batch_ml_run_connectivity(None, 1, 0, 1.0, 1.0, 10, 5, None, None, None, None, 0, None, 0)
    assert rc == N.ERR_BAD_ARG and b"NULL" in L.vbnmf_last_error()
    # a NULL handle inside the batch: the admission's answer, as for vbnmf_batch_ml_run
    hs = (ctypes.c_void_p * 2)(None, None)
    rc = L.vbnmf_batch_ml_run_connectivity(hs, 2, 0, 1.0, 1.0, 10, 5, None, None, None, None, 0, None, 0)
    assert rc == N.ERR_BAD_ARG and b"NULL" in L.vbnmf_last_error()
    # count, max_it and ncnn_step are checked before any handle is read
    for count, max_it, ncnn in ((0, 10, 5), (1, 0, 5), (1, 10, 0)):
        rc = L.vbnmf_batch_ml_run_connectivity(hs, count, 0, 1.0, 1.0, max_it, ncnn, None, None, None, None, 0, None, 0)
        assert rc == N.ERR_BAD_ARG and L.vbnmf_last_error()


def test_python_refuses_an_unknown_criterion_before_any_call():
    from ccfindr_amd.engine import run_batch_ml

    class NoEngine:                                      # reading its handle would be a call into the library
        @property
        def _lib(self):
            raise AssertionError("the library was reached")
        _h = None

    with pytest.raises(ValueError, match="Unknown stopping criterion"):
        run_batch_ml([NoEngine()], criterion="stability")
    with pytest.raises(ValueError, match="empty batch"):
        run_batch_ml([], criterion="connectivity")


def test_stand_in_engine_with_todays_ml_run_keeps_working_under_the_likelihood_rule():
    """Under criterion = 'likelihood' factorize() calls ml_run(Itmax=, Tol=) and nothing more, as before."""
    import numpy as np
    from oracle import mlnmf_oracle as O
    from tests.fake_ml_engine import OracleMLEngine
    from ccfindr_amd.factorize import factorize

    class WithRun(OracleMLEngine):
        def ml_run(self, Itmax, Tol):                    # no criterion, no ncnn_step
            lkold, it, lk = -np.inf, 0, np.nan
            for it in range(1, Itmax + 1):
                lk = self.ml_step()
                if abs(lkold - lk) < Tol * abs(lkold):
                    break
                lkold = lk
            return {"it": it, "lk": lk, "reason": 2}

    rng = np.random.default_rng(3)
    X = rng.poisson(0.9, size=(30, 40)).astype(np.float64)
    X[np.arange(30), rng.integers(0, 40, 30)] += 1
    X[rng.integers(0, 30, 40), np.arange(40)] += 1
    kw = dict(ranks=[2], nrun=2, verbose=0, seed=4, Itmax=200, Tol=1e-5)
    a = factorize(X, engine_factory=lambda M, rank: WithRun(M.host, rank), **kw)
    b = factorize(X, engine_factory=lambda M, rank: OracleMLEngine(M.host, rank), **kw)
    assert a.nsteps == b.nsteps and np.array_equal(a.basis[0], b.basis[0])
