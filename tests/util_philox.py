"""numpy restatement of the device's Gamma initial state (csrc/init.h: philox4x32, u53, gamma_draw, k_gamma_init), written from
the published algorithms (Salmon et al. 2011 for Philox4x32-10, Box-Muller, Marsaglia & Tsang 2000 with the a + 1 boost for
a < 1) and the keying the engine documents: attempt t of element e of factor f uses counters (e lo, e hi, f, 2 t) and
(e lo, e hi, f, 2 t + 1) under key (seed lo, seed hi); W[i, k] is element i r + k of factor 0, H[k, j] element j r + k of factor
1 with j the cell's GLOBAL column.  Used by tests/test_gpu_config_sweep.py; tests/test_config_sweep_cpu.py holds the generator to
its published answers."""
import numpy as np

_MASK = np.uint64(0xFFFFFFFF)
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_S32, _S21, _S11 = np.uint64(32), np.uint64(21), np.uint64(11)


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of counters (arrays of 32-bit values) under key (k0, k1) -> four uint64 arrays of 32-bit words."""
    c = [np.asarray(v, dtype=np.uint64) & _MASK for v in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0) & _MASK, np.uint64(k1) & _MASK
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]                 # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _MASK, (p0 >> _S32) ^ c[3] ^ k1, p0 & _MASK]
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c


def u53(hi, lo):
    v = (hi << _S21) ^ (lo >> _S11)
    return (v.astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def gamma_draws(a, scale, element, factor, seed):
    """Gamma(shape a, scale) of every element index in ``element`` (uint64 array) for ``factor`` under the 64-bit ``seed``."""
    element = np.asarray(element, dtype=np.uint64).ravel()
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    lo, hi = element & _MASK, element >> _S32
    a1 = a + 1.0 if a < 1.0 else a
    d = a1 - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    g = np.zeros(element.size)
    todo = np.arange(element.size)
    for t in range(64):
        if todo.size == 0:
            break
        f = np.full(todo.size, factor, dtype=np.uint64)
        r = philox4x32(lo[todo], hi[todo], f, np.full(todo.size, 2 * t, dtype=np.uint64), k0, k1)
        u1, u2 = u53(r[0], r[1]), u53(r[2], r[3])
        x = np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586476925 * u2)
        r = philox4x32(lo[todo], hi[todo], f, np.full(todo.size, 2 * t + 1, dtype=np.uint64), k0, k1)
        u = u53(r[0], r[1])
        v1 = 1.0 + c * x
        v = v1 * v1 * v1
        with np.errstate(invalid="ignore", divide="ignore"):
            acc = (v1 > 0.0) & (np.log(u) < 0.5 * x * x + d - d * v + d * np.log(v))
        val = d * v
        if a < 1.0:
            val = val * np.power(u53(r[2], r[3]), 1.0 / a)
        g[todo[acc]] = val[acc]
        todo = todo[~acc]
    return g * scale


def normal_draws(nmaj, r, seed):
    """The [nmaj, r] standard normal block of the truncated SVD's range finder (k_normal_init): element el = M r + k uses
    the single counter (el lo, el hi, 7, 0); Box-Muller's cosine branch from the uniforms of words (0, 1) and (2, 3)."""
    el = np.arange(nmaj, dtype=np.uint64)[:, None] * np.uint64(r) + np.arange(r, dtype=np.uint64)[None, :]
    el = el.ravel()
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    q = philox4x32(el & _MASK, el >> _S32, np.full(el.size, 7, dtype=np.uint64), np.zeros(el.size, dtype=np.uint64), k0, k1)
    x = np.sqrt(-2.0 * np.log(u53(q[0], q[1]))) * np.cos(6.283185307179586476925 * u53(q[2], q[3]))
    return x.reshape(nmaj, r)


def random_state(n, m, r, hyper, seed, col_begin=0):
    """(W [n, r], H [r, m]) the engine's ``random_state(hyper, seed)`` draws; H holds the cells col_begin .. col_begin + m - 1."""
    i = np.arange(n, dtype=np.uint64)[:, None] * np.uint64(r) + np.arange(r, dtype=np.uint64)[None, :]
    W = gamma_draws(hyper["aw"], hyper["bw"] / hyper["aw"], i, 0, seed).reshape(n, r)
    j = (np.uint64(col_begin) + np.arange(m, dtype=np.uint64))[None, :] * np.uint64(r) + np.arange(r, dtype=np.uint64)[:, None]
    H = gamma_draws(hyper["ah"], hyper["bh"] / hyper["ah"], j, 1, seed).reshape(r, m)
    return W, H
