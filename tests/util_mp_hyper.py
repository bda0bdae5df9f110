"""hyper_update in 50-digit arithmetic (mpmath): an independent statement of reference R/bayesian.R:2-53 with the values
vb_iterate passes (Niter = 100, Tol = 1e-3, :343-344), used to hold the library's Newton update -- the host build and the
two-lane device routine -- to the exact value of the formulas, one iteration at a time.  Test infrastructure only.  Every
block cites the reference lines it follows.

Two things are not "exact":
  * R's functions return doubles: a value beyond the fp64 range is +-Inf there.  psigamma(a, 1) ~ 1/a^2 overflows below
    a ~ 7.5e-155, which makes the step -0 (:19-20).  _r_double() states that.
  * the project's one disclosed deviation: a non-finite step, or more than 1100 halvings, is a failed update where the
    reference's halving loops (:28-35) would spin for ever.
"""
import ctypes

import mpmath as mp
import numpy as np

mp.mp.dps = 50

NITER = 100                       # :343
TOL = mp.mpf(1e-3)                # :344 (the double 1e-3)
EPS = 2.0 ** -52
DBL_MAX = mp.mpf(1.7976931348623157e308)
FLAG_SETS = [tuple((q >> s) & 1 for s in range(4)) for q in range(16)]

# ---- the constants of the per-iteration tolerance (see step_tolerance) -------------------------------------------------
LN_BOUND = 4e-16                  # tests/util_special.py: relative bound on ln away from 1
PSI_BOUND = 1.8e-15               # tests/util_special.py: digamma, absolute, times max(1, |psi|) (the device build's)
# numerator (log a - psi(a) - em/b + 1 + lm - log b) / g: digamma's bound, two logarithms, the quotient em/b, five
# additions (each rounds a partial sum that S bounds) and the final quotient, one ulp each              -> 18.7
C_F = PSI_BOUND / EPS + 2 * LN_BOUND / EPS + 7


def _r_double(v):
    """An R function's result is a double: beyond the fp64 range it is +-Inf."""
    if mp.isnan(v) or mp.isinf(v):
        return v
    return mp.inf * mp.sign(v) if abs(v) > DBL_MAX else v


def _f(x):
    return mp.mpf(float(x))


def trigamma_series(x):
    """The library's series in plain Python floats (csrc/special.h dev_trigamma, term by term): the yardstick its bound is
    taken from, NOT what it is compared with (that is mpmath.psi(1, x))."""
    if not (x > 0.0) or x == float("inf"):
        return float("nan")
    s = 0.0
    while x < 10.0:
        s += (1.0 / (x * x)) if x * x != 0.0 else float("inf")
        x += 1.0
    xi = 1.0 / x
    y = xi * xi
    ser = xi * y * (1.0 / 6 - y * (1.0 / 30 - y * (1.0 / 42 - y * (1.0 / 30 - y * (5.0 / 66 - y * (691.0 / 2730 - y * (7.0 / 6)))))))
    return s + xi + 0.5 * y + ser


def trigamma_grid():
    from util_special import grid
    seam = np.concatenate([[9.0, 9.09, 9.999, 10.001, np.nextafter(10.0, 0.0), np.nextafter(10.0, 11.0)],
                           np.linspace(9.999, 10.001, 201), np.linspace(8.9, 9.3, 81)])
    tail = np.array([1e25, 1.1e25, 1e28, 7e30, 1e40, 1e100, 1e150, 1e300])
    return np.ascontiguousarray(np.concatenate([grid(), seam, tail]), dtype=np.float64)


def trigamma_rel_err(xs, ys):
    ref = [mp.psi(1, _f(x)) for x in xs]
    return np.array([float(abs(_f(y) - r) / r) for y, r in zip(ys, ref)])


_TRI = {}


def trigamma_bound():
    """2 x the worst relative error of the plain-float series on trigamma_grid() (the factor 2: contraction and reciprocal
    differences between builds, as util_special.py allows the device build).  Measured: 7.2e-16 -> bound 1.44e-15."""
    if "b" not in _TRI:
        xs = trigamma_grid()
        _TRI["worst"] = float(np.max(trigamma_rel_err(xs, [trigamma_series(float(x)) for x in xs])))
        _TRI["b"] = 2.0 * _TRI["worst"]
    return _TRI["b"]


def c_g():
    """Denominator 1/a - psi'(a): trigamma's bound, the reciprocal and the subtraction, in units of eps (1/a + psi'(a))."""
    return trigamma_bound() / EPS + 2


# ---- one Newton step of one side --------------------------------------------------------------------------------------
_STEP = {}


def newton_step(a0, b0, lm, em, fa):
    """One side of one iteration (:18-35) from the fp64 a0.  Returns a dict:
    d0 (the raw step, :19-25), d (after the halvings), a1 (mpf), halvings, bad (non-finite step or > 1100 halvings),
    tol (the fp64 tolerance on d0, see step_tolerance), near_zero (a halving decision within tolerance of a1 = 0)."""
    key = (float(a0), float(b0), float(lm), float(em), int(bool(fa)))
    if key in _STEP:
        return _STEP[key]
    # log(a) - psi(a) ~ 1/(2a) and 1/a - psi'(a) ~ -1/(2a^2) are differences of nearly equal terms: they cost log10(a) and
    # 2 log10(a) digits, which the working precision is raised by (the runaway iterates of a pair without a root)
    big = np.isfinite(float(a0)) and float(a0) > 1.0
    with mp.workdps(mp.mp.dps + (2 * int(np.ceil(np.log10(float(a0)))) if big else 0)):
        out = _newton_step(_f(a0), _f(b0), _f(lm), _f(em), a0, fa)
    _STEP[key] = out
    return out


def _newton_step(a, b, l, e, a0, fa):
    out = {"halvings": 0, "bad": False, "near_zero": False, "tol": mp.mpf(0)}
    if not fa:
        out.update(d0=mp.mpf(0), d=mp.mpf(0), a1=a)                              # :21, :25
    elif not (np.isfinite(float(a0)) and float(a0) > 0.0):
        # log / digamma / psigamma of a shape that is no positive number: NaN (or a pole), i.e. a non-finite step
        out.update(bad=True, d0=mp.nan, d=mp.nan, a1=mp.nan)
    else:
        tri = mp.psi(1, a)
        terms = [mp.log(a), -_r_double(mp.digamma(a)), -e / b, mp.mpf(1), l, -mp.log(b)]
        g = _r_double(1 / a) - _r_double(tri)                                    # :20 / :24
        d0 = mp.fsum(terms) / g                                                  # :19 / :23
        out["d0"] = d0
        if mp.isnan(d0) or mp.isinf(d0):
            out.update(bad=True, d=d0, a1=mp.nan)
        else:
            if not mp.isinf(g):
                S = mp.fsum(abs(t) for t in terms)
                out["tol"] = (C_F * EPS * S) / abs(g) + abs(d0) * c_g() * EPS * (1 / a + tri) / abs(g)
            d, a1, h = d0, a - d0, 0
            floor = 2 * EPS * a
            determined = out["tol"] <= max(abs(d0), a) / 2                       # (else: ill_conditioned below)
            while True:                                                          # :28-35
                if determined and abs(a1) <= mp.ldexp(out["tol"], -h) + floor:
                    out["near_zero"] = True
                if not a1 <= 0:
                    break
                d = d / 2
                a1 = a - d
                h += 1
                if h > 1100:
                    out["bad"] = True
                    break
            out.update(d=d, a1=a1, halvings=h)
    return out


def step_tolerance(st, a0):
    """Tolerance on d = a_prev - a_next of an fp64 evaluation of the step `st` (a newton_step result):
        (c_f eps S) / |g|  +  |d| c_g eps (1/a + psi'(a)) / |g|  +  2 eps |a_prev|
    S: the sum of the absolute values of the numerator's six terms, g: the exact denominator.  The first two scale with
    the halvings, the last (the rounding of a0 - d, twice) does not."""
    return mp.ldexp(st["tol"], -st["halvings"]) + 2 * EPS * abs(_f(a0))


def ill_conditioned(st, a0):
    """fp64 determines neither this step nor the new shape to within a factor of two: the derived tolerance exceeds half
    of the larger of |d| and a (1/a - psi'(a) ~ -1/(2 a^2) against terms of size 1/a has lost every bit from a ~ 1e14
    on -- the runaway iterates of a pair of statistics without a root, which fail in any arithmetic)."""
    return (not st["bad"]) and st["tol"] > max(abs(st["d0"]), abs(_f(a0))) / 2


# ---- the whole update -------------------------------------------------------------------------------------------------
def update(flags, stats, hyper):
    """hyper_update (:2-53) from fp64 flags[4], stats = (lwm, lhm, ewm, ehm), hyper = (aw, bw, ah, bh).
    Returns dict(hyper [4 mpf], failed, iters, trace [list of (aw1, ah1) mpf], near_tol, near_zero, ill) -- the last three:
    some iteration's df within 1e-9 relative of Tol / a halving decision within tolerance / an ill-conditioned step."""
    flags = [int(bool(f)) for f in flags]
    h = [_f(v) for v in hyper]
    out = {"hyper": list(h), "failed": False, "iters": 0, "trace": [], "near_tol": False, "near_zero": False, "ill": False}
    if sum(flags) == 0:                                                          # :4
        return out
    lwm, lhm, ewm, ehm = stats                                                   # :8-11
    aw0, ah0 = float(hyper[0]), float(hyper[2])                                  # :6-7
    aw1, ah1 = h[0], h[2]
    if flags[0] + flags[2] > 0:                                                  # :15
        i = 1
        while i < NITER:                                                         # :17
            sw = newton_step(aw0, hyper[1], lwm, ewm, flags[0])                  # :18-21, :26, :28-31
            sh = newton_step(ah0, hyper[3], lhm, ehm, flags[2])                  # :22-25, :27, :32-35
            out["iters"] += 1
            out["trace"].append((sw["a1"], sh["a1"]))
            out["near_zero"] |= sw["near_zero"] or sh["near_zero"]
            out["ill"] |= ill_conditioned(sw, aw0) or ill_conditioned(sh, ah0)
            if sw["bad"] or sh["bad"]:
                out["failed"] = True
                break
            aw1, ah1 = sw["a1"], sh["a1"]
            df = (1 - aw1 / _f(aw0)) ** 2 + (1 - ah1 / _f(ah0)) ** 2             # :37
            # within 1e-9 relative of Tol, or within what the steps' fp64 tolerances move df by: another arithmetic may stop
            # one iteration apart by right
            reach = 2 * (abs(1 - aw1 / _f(aw0)) * step_tolerance(sw, aw0) / _f(aw0)
                         + abs(1 - ah1 / _f(ah0)) * step_tolerance(sh, ah0) / _f(ah0))
            if not out["ill"]:
                out["near_tol"] |= abs(df / TOL - 1) < 1e-9 or abs(df - TOL) <= reach
            if df < TOL:                                                         # :38
                break
            # the next iteration starts from the fp64 value, as every implementation's does
            aw0, ah0 = _to_double(aw1), _to_double(ah1)                          # :39-40
            i += 1                                                               # :41
        if i == NITER:                                                           # :43
            out["failed"] = True
    if not out["failed"]:
        bw1 = _f(stats[2]) if flags[1] else h[1]                                 # :48-49
        bh1 = _f(stats[3])                                                       # :50-51: both branches assign ehm
        out["hyper"] = [aw1, bw1, ah1, bh1]                                      # :52
    return out


def _to_double(v):
    return float(v) if abs(v) <= DBL_MAX else float("inf") * (1 if v > 0 else -1)


# ---- the case grid ----------------------------------------------------------------------------------------------------
_GRID = {}


def _gamma_stats(k, b0, delta):
    """E log and E of a Gamma of shape k and mean b0, the mean off by the factor 1 + delta."""
    k = _f(k)
    return float(mp.digamma(k) - mp.log(k / _f(b0))), float(b0) * (1.0 + delta)


def case_grid():
    """The seeded case list: dict(flags [N,4] int32, stats [N,4], hyper [N,4], stratum [N] of str).  Built once."""
    if _GRID:
        return _GRID
    rng = np.random.default_rng(20240607)
    F, S, H, T = [], [], [], []

    def side(kind, a0=None, k=None):
        """(a0, b0, lm, em) of one side."""
        b0 = 10.0 ** rng.uniform(-3, 3)
        if a0 is None:
            a0 = 10.0 ** rng.uniform(-4, 6)
        if k is None:
            k = 10.0 ** rng.uniform(-3, 5)
        if kind == "consistent":
            lm, em = _gamma_stats(k, b0, rng.uniform(-0.1, 0.1))
        elif kind == "exact":
            lm, em = _gamma_stats(k, b0, 0.0)
        else:                                             # no root: 1 + lm - log b0 - em/b0 = c > 0
            c = 10.0 ** rng.uniform(-1.3, 0.7)
            em = b0 * 10.0 ** rng.uniform(-1, 1)
            lm = c - 1.0 + float(np.log(b0)) + em / b0
        return a0, b0, lm, em

    def add(flags, w, h, stratum):
        F.append(flags); T.append(stratum)
        S.append([w[2], h[2], w[3], h[3]]); H.append([w[0], w[1], h[0], h[1]])

    for flags in FLAG_SETS:                               # every flag combination, 90 cases each
        for j in range(90):
            kinds = ["consistent" if rng.random() < 0.85 else "noroot" for _ in range(2)]
            add(flags, side(kinds[0]), side(kinds[1]), "general")
    for j in range(150):                                  # the first step halves: start far above a small root
        fl = [(1, 1, 1, 1), (1, 0, 0, 0), (0, 0, 1, 1)][j % 3]
        mk = lambda: side("consistent", a0=10.0 ** rng.uniform(3, 6), k=10.0 ** rng.uniform(-3, -1))
        add(fl, mk(), mk(), "halving")
    for j in range(100):                                  # converges in one iteration: start at the root, off by <= 1e-3
        fl = [(1, 1, 1, 1), (1, 0, 1, 0), (1, 1, 0, 0), (0, 0, 1, 0)][j % 4]
        def mk():
            k = 10.0 ** rng.uniform(-3, 5)
            return side("exact", a0=k * (1.0 + rng.uniform(-1e-3, 1e-3)), k=k)
        add(fl, mk(), mk(), "one_iteration")
    for j in range(100):                                  # one lane's flag on, the other side's d = 0
        fl = [(1, 0, 0, 0), (0, 0, 1, 0), (1, 1, 0, 1), (0, 1, 1, 1)][j % 4]
        add(fl, side("consistent"), side("consistent"), "one_lane")
    for j in range(40):                                   # lm = -inf (fudge = 0 and exp(psi) underflowed): a failure
        fl = [(1, 1, 1, 1), (1, 0, 0, 0), (0, 0, 1, 0), (1, 0, 1, 1)][j % 4]
        w, h = list(side("consistent")), list(side("consistent"))
        if fl[0] and (j % 8 < 4 or not fl[2]):
            w[2] = -np.inf
        else:
            h[2] = -np.inf
        add(fl, w, h, "minus_inf")
    seam = [10.0, np.nextafter(10.0, 0.0), np.nextafter(10.0, 11.0), 9.999, 10.001]
    for j in range(100):                                  # the seam of the trigamma shift
        a = seam[j] if j < len(seam) else rng.uniform(9.999, 10.001)
        fl = [(1, 1, 1, 1), (1, 0, 0, 0), (0, 0, 1, 0)][j % 3]
        add(fl, side("consistent", a0=a), side("consistent", a0=rng.uniform(9.999, 10.001)), "seam")
    for j in range(20):                                   # 1 / (x x) overflows: the step is -0
        fl = [(1, 1, 1, 1), (1, 0, 0, 0), (0, 0, 1, 0), (1, 0, 1, 0)][j % 4]
        add(fl, side("consistent", a0=1e-300), side("consistent", a0=1e-300 if j % 2 else None), "tiny")
    _GRID.update(flags=np.ascontiguousarray(F, dtype=np.int32), stats=np.ascontiguousarray(S, dtype=np.float64),
                 hyper=np.ascontiguousarray(H, dtype=np.float64), stratum=np.array(T))
    return _GRID


_REF = {}


def reference():
    """update() on every case of the grid, computed once and shared."""
    if "r" not in _REF:
        G = case_grid()
        _REF["r"] = [update(G["flags"][c], G["stats"][c], G["hyper"][c]) for c in range(len(G["flags"]))]
    return _REF["r"]


def decade(a0):
    return int(np.floor(np.log10(float(a0))))


def comparable(R):
    """A 50-digit whole update another implementation's whole update can be compared with value for value: it converged,
    and none of its decisions (stop, halving) sat within rounding of its threshold, none of its steps was ill-conditioned."""
    return not (R["failed"] or R["ill"] or R["near_tol"] or R["near_zero"])


def oracle_errors():
    """oracle.vbnmf_oracle.hyper_update (fp64, SciPy's digamma / polygamma: the committed reference side) against update()
    on the comparable cases of the grid -> {decade of the start shape: worst relative error of the final shape}.  The oracle
    states the reference's loops literally, the unbounded halving of a non-finite step included, so it is run only where
    the 50-digit update converges.  It forms its statistics from matrices: a 1 x 1 `lw` of exp(lm) gives it log(exp(lm)),
    and that double -- not lm -- is what the 50-digit side is given here."""
    if "oe" in _REF:
        return _REF["oe"]
    from oracle import vbnmf_oracle as O
    G, ref = case_grid(), reference()
    worst, count = {}, 0
    for c in range(len(ref)):
        if not (np.all(np.isfinite(G["stats"][c])) and np.all(G["stats"][c][:2] > -700.0)):   # (exp(lm) must not underflow)
            continue
        if not comparable(ref[c]):
            continue
        fl, st, hy = G["flags"][c], G["stats"][c], G["hyper"][c]
        wh = {"lw": np.exp(st[0:1]), "lh": np.exp(st[1:2]), "ew": st[2:3], "eh": st[3:4]}
        st2 = np.array([np.log(wh["lw"])[0], np.log(wh["lh"])[0], st[2], st[3]])     # (finite: the update converged)
        R = ref[c] if np.array_equal(st2, st) else update(fl, st2, hy)
        if not comparable(R):
            continue
        got = O.hyper_update(fl, wh, dict(zip(("aw", "bw", "ah", "bh"), (float(v) for v in hy))), Niter=NITER, Tol=1e-3)
        count += 1
        for s, key in ((0, "aw"), (2, "ah")):
            err = float(abs(_f(got[key]) - R["hyper"][s]) / R["hyper"][s])
            dec = decade(hy[s])
            worst[dec] = max(worst.get(dec, 0.0), err)
        assert got["bw"] == float(R["hyper"][1]) and got["bh"] == float(R["hyper"][3]), (c, got)
    _REF["oe"] = (worst, count)
    return _REF["oe"]


def whole_update_tolerance(a0):
    """Relative tolerance on a whole update's final shape that started at a0: 10 x the oracle's own worst error against
    50-digit math in a0's decade (oracle_errors), floor 1e-12."""
    return max(1e-12, 10.0 * oracle_errors()[0].get(decade(a0), 0.0))


# ---- the library's hooks ----------------------------------------------------------------------------------------------
def run_hook(flags, stats, hyper, device):
    """vbnmf_test_hyper_update_host / _device -> dict(hyper [N,4], failed [N], iters [N], trace [N,2,100])."""
    from ccfindr_amd import _native as N
    L = N.load()
    flags = np.ascontiguousarray(flags, dtype=np.int32).reshape(-1, 4)
    stats = np.ascontiguousarray(stats, dtype=np.float64).reshape(-1, 4)
    hyper = np.ascontiguousarray(hyper, dtype=np.float64).reshape(-1, 4)
    n = flags.shape[0]
    out = np.full((n, 4), np.nan)
    failed, iters = np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    trace = np.zeros((n, 2, 100))
    fn = L.vbnmf_test_hyper_update_device if device else L.vbnmf_test_hyper_update_host
    i32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    N.check(fn(n, i32(flags), N.dptr(stats), N.dptr(hyper), N.dptr(out), i32(failed), i32(iters), N.dptr(trace)))
    return {"hyper": out, "failed": failed, "iters": iters, "trace": trace}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_hook(got, G=None, ref=None):
    """Every assertion of the hook's results on the grid against 50-digit math; returns the figures it measured:
    dict(skipped_tol, skipped_zero, ill, worst [per-iteration error / tolerance], transitions)."""
    G = G or case_grid()
    ref = ref or reference()
    n = len(G["flags"])
    skipped_tol = skipped_zero = ill = transitions = 0
    worst = worst_whole = 0.0
    for c in range(n):
        fl, st, hy = G["flags"][c], G["stats"][c], G["hyper"][c]
        it, failed, tr, ho = int(got["iters"][c]), int(got["failed"][c]), got["trace"][c], got["hyper"][c]
        tag = (c, G["stratum"][c], tuple(fl), tuple(hy), tuple(st))
        newton = fl[0] + fl[2] > 0
        # the trace holds exactly `iters` iterates per side
        assert 0 <= it <= 99, tag
        assert np.all(np.isnan(tr[:, it:])), tag
        if not newton:
            assert it == 0 and failed == 0, tag
        # ---- every iteration from the hook's own iterates
        a_prev = [float(hy[0]), float(hy[2])]
        skip = None                                    # a decision was within its tolerance: nothing after it is comparable
        ended = None
        for k in range(it):
            steps = [newton_step(a_prev[s], hy[2 * s + 1], st[s], st[2 + s], fl[2 * s]) for s in range(2)]
            if any(ill_conditioned(steps[s], a_prev[s]) for s in range(2)):
                ill += 1
                skip = "ill"                           # fp64 does not determine this step: only `failed` is held below
                break
            if steps[0]["bad"] or steps[1]["bad"]:
                ended = "failed"
                assert k == it - 1 and failed == 1, tag + (k, "a non-finite step is the last, and a failure")
                break
            u2 = mp.mpf(0)
            for s in range(2):
                a_next = float(tr[s, k])
                assert np.isfinite(a_next) and a_next > 0.0, tag + (k, s, a_next)
                d_got = _f(a_prev[s]) - _f(a_next)
                tol = step_tolerance(steps[s], a_prev[s])
                err = abs(d_got - steps[s]["d"])
                if err > tol and steps[s]["near_zero"]:
                    skip = "zero"                      # the halving count may differ by right: a1 within tolerance of 0
                    continue
                assert err <= tol, tag + (k, s, a_prev[s], a_next, float(steps[s]["d"]), float(err), float(tol))
                if steps[s]["halvings"]:               # the count itself: d_got = d0 / 2^h
                    h_got = int(mp.nint(mp.log(steps[s]["d0"] / d_got, 2)))
                    assert h_got == steps[s]["halvings"], tag + (k, s, h_got, steps[s]["halvings"])
                if tol > 0:
                    worst = max(worst, float(err / tol))
                transitions += 1
                u2 += (1 - _f(a_next) / _f(a_prev[s])) ** 2
            if skip:
                skipped_zero += 1
                break
            if abs(u2 / TOL - 1) < 1e-9:
                skipped_tol += 1
                skip = "tol"
                break
            if u2 < TOL:
                ended = "converged"
                assert k == it - 1 and failed == 0, tag + (k, "df < Tol ends the iteration", float(u2))
                break
            assert k < it - 1 or it == 99, tag + (k, "df >= Tol goes on", float(u2))
            a_prev = [float(tr[0, k]), float(tr[1, k])]
        if not skip and newton:
            if ended is None:                          # ran out: i == 100
                assert it == 99 and failed == 1, tag
            assert failed == (0 if ended == "converged" else 1), tag
        # ---- outputs
        if failed:
            assert np.array_equal(_bits(ho), _bits(hy)), tag + ("a failed update leaves all four untouched",)
        elif sum(fl) == 0:
            assert np.array_equal(_bits(ho), _bits(hy)) and np.all(np.isnan(tr)), tag
        else:
            assert np.all(np.isfinite(tr[:, :it])), tag
            want = [tr[0, it - 1] if newton else hy[0], st[2] if fl[1] else hy[1], tr[1, it - 1] if newton else hy[2], st[3]]
            assert np.array_equal(_bits(ho), _bits(want)), tag + (ho, want)
        # ---- against the whole 50-digit update
        R = ref[c]
        near = skip in ("zero", "tol") or R["near_tol"] or R["near_zero"]
        if not near:
            # (a pair of statistics without a root fails in every arithmetic: by i == 100 in exact math, by a non-finite
            # step once the iterates have run away in fp64)
            assert failed == int(R["failed"]), tag + (failed, R["failed"])
        if not near and skip != "ill" and not R["ill"]:
            assert it == R["iters"], tag + (it, R["iters"])
            if not failed:
                for s in (0, 2):
                    rel = float(abs(_f(ho[s]) - R["hyper"][s]) / R["hyper"][s])
                    assert rel <= whole_update_tolerance(hy[s]), tag + (s, rel, whole_update_tolerance(hy[s]))
                    worst_whole = max(worst_whole, rel)
                assert ho[1] == float(R["hyper"][1]) and ho[3] == float(R["hyper"][3]), tag
    return {"skipped_tol": skipped_tol, "skipped_zero": skipped_zero, "ill": ill, "worst": worst, "transitions": transitions,
            "worst_whole": worst_whole}
