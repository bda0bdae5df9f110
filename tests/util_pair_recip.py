"""The pair form's test inputs (csrc/special.h: dev_div_pair), shared by the host and the device test."""
import mpmath
import numpy as np

from util_special import grid

mpmath.mp.dps = 50
BOUND = 2.0 ** -45


def quads(scale):
    rng = np.random.default_rng(19)
    wa = grid() * scale
    wb = rng.permutation(grid()) * scale
    keep = (np.abs(np.log2(wa)) <= 500) & (np.abs(np.log2(wb)) <= 500)
    wa, wb = wa[keep], wb[keep]
    n = wa.size
    # stored counts (ones, twos, larger) on half of the grid, non-integer values (the wide layout's) on the other half
    xa = np.where(np.arange(n) % 2 == 0, rng.integers(1, 40, n).astype(np.float64), rng.uniform(0.01, 30.0, n))
    xb = np.where(np.arange(n) % 3 == 0, 1.0, rng.uniform(0.01, 30.0, n))
    return np.ascontiguousarray(np.stack([wa, wb, xa, xb], axis=1).ravel())
