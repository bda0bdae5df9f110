"""GPU: the sweep's pair form -- one fp64 reciprocal per pair of entries (csrc/kernels.h: sweep_pair_head, sweep_pairs;
csrc/special.h: dev_div_pair).

One vbnmf_update step against oracle/vbnmf_oracle (reference src/vbnmf_update.cpp:33-90) at the tolerances of
tests/test_gpu_parity.py (factors 1e-12, lkh 1e-10), on shapes that run every form of the paired trip: the leading ones, the
ones-or-twos behind them and the general mode; odd group counts; pairs cut into merged pieces; the wide (non-integer) trip;
512 threads; ranks shared between two lanes; the one-buffer loop, which stays per entry.  A scale test puts wth near
2^-480 and 2^+480: the oracle's step is exactly scale-invariant there, so the tolerances are the same.  The pair form itself
is held on the device against its host twin (tests/test_pair_recip_cpu.py holds that one to mpmath)."""
import numpy as np
import pytest

from util_pair_recip import BOUND, quads
from util_piece_merge import layout_view
from util_special import evaluate

pytestmark = pytest.mark.gpu

FACT = ("lw", "lh", "ew", "eh", "dw", "dh")
HY1 = {"aw": 1.0, "bw": 1.0, "ah": 1.0, "bh": 1.0}


def relerr(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def check_step(got, want, lkh=None):
    for k in FACT:
        print(k, relerr(got[k], want[k]))
        assert relerr(got[k], want[k]) <= 1e-12, (k, relerr(got[k], want[k]))
    lkh = got["lkh"] if lkh is None else lkh
    print("lkh", lkh, want["lkh"])
    assert np.isfinite(lkh) and abs(lkh / want["lkh"] - 1) <= 1e-10, (lkh, want["lkh"])


def counts(n, m, lam, seed):
    rng = np.random.default_rng(seed)
    X = rng.poisson(lam, size=(n, m)).astype(np.float64)
    X[np.arange(n), rng.integers(0, m, n)] += 1      # no empty rows
    X[rng.integers(0, n, m), np.arange(m)] += 1      # no empty columns
    return np.asfortranarray(X)


def step_case(X, r, seed):
    import ccfindr_amd as C
    from ccfindr_amd import synth
    from oracle import vbnmf_oracle as O
    n, m = X.shape
    wh = synth.random_state(n, m, r, HY1, seed=seed)
    check_step(C.vbnmf_update(X, wh, HY1, C.EPS), O.update_dense(X, wh, HY1, C.EPS))


def test_ones_twos_and_larger_counts_rank_10():
    """96 x 160, Poisson 0.6: of the stored entries about 72 % are ones, 22 % twos, 5 % larger -- all three trip modes."""
    X = counts(96, 160, 0.6, seed=266)
    stored = X[X > 0]
    assert 0.6 < np.mean(stored == 1) < 0.8 and 0.15 < np.mean(stored == 2) < 0.3 and np.mean(stored > 2) > 0.03
    step_case(X, 10, seed=7)


def test_odd_group_counts_rank_10():
    step_case(counts(97, 211, 0.3, seed=318), 10, seed=7)


def test_pairs_cut_into_merged_pieces_through_an_engine(monkeypatch):
    """64 x 700 with four fully dense rows, tasks of 16 entries at the most: the dense rows are cut into runs of pieces that
    the wave adds up behind the paired trip."""
    import ccfindr_amd as C
    from ccfindr_amd import synth
    from oracle import vbnmf_oracle as O
    monkeypatch.setenv("VBNMF_MAX_LEN", "16")
    rng = np.random.default_rng(64700)
    X = counts(64, 700, 0.05, seed=764)
    X[[3, 17, 40, 63], :] = rng.integers(1, 4, size=(4, 700))
    X = np.asfortranarray(X)
    r = 10
    wh = synth.random_state(64, 700, r, HY1, seed=7)
    M = C.CountMatrix(X)
    v = layout_view(M, 0, r)
    assert v["merge"] == 1 and v["n_rows"] < v["n_tasks"]             # runs of more than one piece
    eng = C.VBEngine(M, r)
    eng.set_state(wh["lw"], wh["lh"], wh["eh"])
    lkh, _stats = eng.step(HY1)
    got = eng.get_state()
    eng.close(); M.close()
    check_step(got, O.update_dense(X, wh, HY1, C.EPS), lkh=lkh)


@pytest.mark.parametrize("n,m,r", [(80, 150, 5),
                                   (40, 45, 40)])         # two lanes share a task: the form of shared ranks that pairs
def test_wide_trip_non_integer(n, m, r):
    X = counts(n, m, 0.7, seed=5)
    X = np.asfortranarray(X * (np.median(X.sum(axis=0)) / X.sum(axis=0))[None, :])
    step_case(X, r, seed=9)


@pytest.mark.parametrize("n,m,r", [(50, 60, 16),          # 512 threads (per entry: no measured gain at this rank)
                                   (50, 60, 20),          # 512 threads, paired
                                   (40, 45, 40),          # two lanes share a task (packed entries: per entry, the pair would spill)
                                   (40, 45, 30)])         # the one-buffer loop: per entry, as it was
def test_other_rank_shapes(n, m, r):
    step_case(counts(n, m, 1.0, seed=n + m + r), r, seed=7)


@pytest.mark.parametrize("log2_scale", [-240, 240])
def test_factors_scaled_to_the_ends_of_the_domain(log2_scale):
    """lw and lh each times 2^-240, then 2^+240: wth near 2^-480 / 2^+480, the product of two divisors near 2^-+960."""
    import ccfindr_amd as C
    from ccfindr_amd import synth
    from oracle import vbnmf_oracle as O
    X = counts(96, 160, 0.6, seed=266)
    wh = dict(synth.random_state(96, 160, 10, HY1, seed=7))
    for k in ("lw", "lh"):
        wh[k] = np.asfortranarray(wh[k] * 2.0 ** log2_scale)
    want = O.update_dense(X, wh, HY1, C.EPS)
    assert all(np.all(np.isfinite(want[k])) for k in FACT) and np.isfinite(want["lkh"])
    check_step(C.vbnmf_update(X, wh, HY1, C.EPS), want)


@pytest.mark.parametrize("log2_scale", [0, -480, 480])
def test_pair_form_on_the_device_against_the_host_twin(log2_scale):
    """Both builds return (x / w)(1 - e^2) up to four roundings, e the relative error of their seed: at most 2^-46 below the
    quotient on the host (24-bit seed) and 2^-48 on the device, so they differ by less than the host form's own bound."""
    q = quads(2.0 ** log2_scale)
    host = evaluate(8, q, device=False).reshape(-1, 4)
    dev = evaluate(8, q, device=True).reshape(-1, 4)
    assert np.all(np.isfinite(dev))
    err = np.max(np.abs(dev[:, :3] / host[:, :3] - 1))
    print(f"scale 2^{log2_scale}: device against host 2^{np.log2(max(err, 1e-300)):.2f}")
    assert err <= BOUND, np.log2(err)
    pad = q.reshape(-1, 4).copy()
    pad[:, 2] = 0.0
    got = evaluate(8, np.ascontiguousarray(pad.ravel()), device=True).reshape(-1, 4)
    assert np.all(got[:, 0] == 0.0) and np.array_equal(got[:, 1], dev[:, 1])
