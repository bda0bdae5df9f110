"""Host build of the sweep's pair form (csrc/special.h: dev_div_pair -- two quotients from one reciprocal of the product
of their divisors) against mpmath, through kind 8 of vbnmf_test_special_host: quads wa, wb, xa, xb in; qa, qb, r, 0 out.

Bound: 2^-45 relative on both quotients -- dev_div_fast's bound with the host's deliberately coarsened 24-bit seed (2^-46:
the square of the seed's 2^-23) plus one bit.  Divisors: the grid the other divisions of special.h are held on, at the
scales 2^0, 2^-480 and 2^+480 (both divisors: the product reaches 2^+-960), cut to the form's documented domain (either
divisor within 2^+-500, so that the product and its reciprocal stay normal doubles)."""
import mpmath
import numpy as np
import pytest

from util_pair_recip import BOUND, quads
from util_special import evaluate

mpmath.mp.dps = 50


def relative_errors(q, out):
    err = []
    for (wa, wb, xa, xb), (qa, qb) in zip(q.reshape(-1, 4), out.reshape(-1, 4)[:, :2]):
        ta, tb = mpmath.mpf(float(xa)) / mpmath.mpf(float(wa)), mpmath.mpf(float(xb)) / mpmath.mpf(float(wb))
        err.append(max(float(abs(mpmath.mpf(float(qa)) / ta - 1)), float(abs(mpmath.mpf(float(qb)) / tb - 1))))
    return np.array(err)


@pytest.mark.parametrize("log2_scale", [0, -480, 480])
def test_both_quotients_against_mpmath(log2_scale):
    q = quads(2.0 ** log2_scale)
    assert q.size // 4 > 1500                                        # the domain cut keeps most of the grid
    out = evaluate(8, q, device=False)
    assert np.all(np.isfinite(out))
    err = relative_errors(q, out)
    print(f"scale 2^{log2_scale}: {err.size} pairs, max relative error 2^{np.log2(err.max()):.2f}")
    assert err.max() <= BOUND, (log2_scale, np.log2(err.max()), q.reshape(-1, 4)[np.argmax(err)])
    # the shared reciprocal itself: 1 / (wa wb) to the same bound
    wa, wb, r = q.reshape(-1, 4)[:, 0], q.reshape(-1, 4)[:, 1], out.reshape(-1, 4)[:, 2]
    rerr = max(float(abs(mpmath.mpf(float(c)) * mpmath.mpf(float(a)) * mpmath.mpf(float(b)) - 1)) for a, b, c in zip(wa, wb, r))
    assert rerr <= BOUND, np.log2(rerr)


@pytest.mark.parametrize("log2_scale", [0, -480, 480])
def test_padding_beside_a_live_entry(log2_scale):
    """A padding slot (x = 0) gives an exact 0 and leaves its partner's quotient as it is, on either side of the pair."""
    live = quads(2.0 ** log2_scale).reshape(-1, 4)
    want = evaluate(8, np.ascontiguousarray(live.ravel()), device=False).reshape(-1, 4)
    for side in (0, 1):
        pad = live.copy()
        pad[:, 2 + side] = 0.0
        got = evaluate(8, np.ascontiguousarray(pad.ravel()), device=False).reshape(-1, 4)
        assert np.all(got[:, side] == 0.0) and not np.any(np.signbit(got[:, side]))
        assert np.array_equal(got[:, 1 - side], want[:, 1 - side])
        assert np.array_equal(got[:, 2], want[:, 2])
