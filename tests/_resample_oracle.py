"""The gather + nudge of a resample (include/obe_hip.h: obe_resample_particles) in exact arithmetic, on the CPU only.

The contract is the chain of operations itself, each of them one correctly rounded double operation:

    s = 0.0;  s = fma(z[p, j], F[i, j], s)  for j = 0 .. D-1        (one rounding per step)
    v = old[i, clamp(idx[p])] + s
    if scale:  v = v*a + mean[i]*(1 - a)                            (two products and a sum, three roundings)

— not the bits of whichever BLAS NumPy was built with.  ``fma`` is DEFINED in rational arithmetic (``fma_exact``); the
C maths library's ``fma`` stands in for it once it has agreed with the definition on ``FMA_TABLE`` (``fma``,
``fast_fma_checked``).  Additions and multiplications of whole arrays are NumPy's elementwise ones: IEEE operations, one
rounding each, never contracted.

The three neighbouring chains a kernel could compute instead (``nudge_mul_then_add``, ``nudge_reversed_j``,
``nudge_from_old``) and the contracted scale step (``scale_contracted``) are here for tests/test_resample_oracle_host.py,
which shows that the inputs of tests/test_gpu_resample_exact.py (``general_case``) tell the contract from each of them.
"""
import ctypes
import ctypes.util
import functools
from fractions import Fraction

import numpy as np

import _constraint_oracle as co

A_PARAM = 0.98


def fma_exact(x, y, c):
    """x*y + c with ONE rounding (to nearest, ties to even), for finite doubles: the definition."""
    return float(Fraction(x) * Fraction(y) + Fraction(c))


def _fma_table():
    g = np.random.default_rng(20240611)
    rows = [tuple(t) for t in g.standard_normal((300, 3)).tolist()]
    rows += [tuple(t) for t in (g.standard_normal((100, 3)) * 10.0 ** g.integers(-8, 9, (100, 3))).tolist()]
    # crafted: the low half of the product, which a multiplication rounded on its own throws away, decides
    for k in range(27, 52):
        x = 1.0 + 2.0 ** -k
        p = x * x                                       # (rounded: the 2^-2k term is lost for 2k > 52)
        rows.append((x, x, 2.0 ** -53))                 # the product's tail lifts the sum above the tie
        rows.append((x, x, -2.0 ** -53))
        rows.append((x, x, -p))                         # the tail alone is left
        rows.append((-x, x, p))
        rows.append((x, 1.0 - 2.0 ** -k, -1.0))         # exact product 1 - 2^-2k
    rows += [(3.0, 5.0, 7.0), (0.0, 5.0, 0.0), (-0.0, 5.0, 0.0), (2.0 ** -537, 2.0 ** -537, 0.0), (0.1, 10.0, -1.0)]
    return rows


FMA_TABLE = _fma_table()


def _libm_fma():
    for name in ("libm.so.6", ctypes.util.find_library("m")):
        try:
            f = ctypes.CDLL(name).fma
        except (OSError, AttributeError, TypeError):
            continue
        f.restype = ctypes.c_double
        f.argtypes = [ctypes.c_double] * 3
        return f
    return None


def _same(a, b):
    return np.float64(a).view(np.int64) == np.float64(b).view(np.int64)


@functools.lru_cache(maxsize=None)
def fast_fma_checked():
    """The C library's fma if it is there and equals ``fma_exact`` bit for bit on every row of FMA_TABLE, else None."""
    f = _libm_fma()
    if f is None or not all(_same(f(*t), fma_exact(*t)) for t in FMA_TABLE):
        return None
    return f


def fma(x, y, c):
    f = fast_fma_checked()
    return f(x, y, c) if f is not None else fma_exact(x, y, c)


def clamp(idx, n):
    """The source particle of a draw: an index outside the cloud reads its nearest end."""
    return np.clip(np.asarray(idx, dtype=np.int64), 0, n - 1)


def _chain(z, F, start=None, order=None, fused=True):
    """(D, n): the D-term sum of z[p, :] * F[i, :] for every (i, p), from ``start`` (default 0.0) in ``order``."""
    f = fast_fma_checked() or fma_exact
    n, d = z.shape
    js = list(range(d)) if order is None else list(order)
    zl, Fl = z.tolist(), F.tolist()
    s0 = None if start is None else start.tolist()
    out = np.empty((d, n))
    for p in range(n):
        zp = zl[p]
        for i in range(d):
            Fi = Fl[i]
            s = 0.0 if s0 is None else s0[i][p]
            if fused:
                for j in js:
                    s = f(zp[j], Fi[j], s)
            else:
                for j in js:
                    s = s + zp[j] * Fi[j]                # (Python floats: each operation rounded on its own)
            out[i, p] = s
    return out


def scale_two_roundings(v, mean, a):
    """v*a + mean*(1 - a): the two products and the sum rounded separately, 1 - a computed in double."""
    one_minus_a = 1.0 - a
    va = v * a
    mc = (np.asarray(mean, dtype=np.float64) * one_minus_a)[:, None]
    return va + mc


def scale_contracted(v, mean, a):
    """The wrong form fma(v, a, mean*(1 - a)): the product v*a is not rounded."""
    one_minus_a = 1.0 - a
    mc = (np.asarray(mean, dtype=np.float64) * one_minus_a).tolist()
    f = fast_fma_checked() or fma_exact
    out = np.empty_like(v)
    for i, row in enumerate(v.tolist()):
        out[i] = [f(x, a, mc[i]) for x in row]
    return out


def _finish(v, mean, a, scale):
    return scale_two_roundings(v, mean, a) if scale else v


def unscaled_exact(old, idx, z, F):
    """old[:, clamp(idx)] + the FMA chain from zero in j order: the result before the scale step."""
    old, z, F = (np.asarray(x, dtype=np.float64) for x in (old, z, F))
    return old[:, clamp(idx, old.shape[1])] + _chain(z, F)


def nudge_exact(old, idx, z, F, mean, a, scale):
    """The (D, n) array obe_resample_particles documents, from ``old`` (D, n), ``idx`` (n,), ``z`` (n, D), ``F`` (D, D)."""
    return _finish(unscaled_exact(old, idx, z, F), mean, a, scale)


# ---- the neighbours of the contract: each differs from it in the last bit or two on general doubles
def nudge_mul_then_add(old, idx, z, F, mean, a, scale):
    """s = s + z*F: the product rounded before the addition."""
    old, z, F = (np.asarray(x, dtype=np.float64) for x in (old, z, F))
    return _finish(old[:, clamp(idx, old.shape[1])] + _chain(z, F, fused=False), mean, a, scale)


def nudge_reversed_j(old, idx, z, F, mean, a, scale):
    """The FMA chain from zero, j = D-1 .. 0."""
    old, z, F = (np.asarray(x, dtype=np.float64) for x in (old, z, F))
    return _finish(old[:, clamp(idx, old.shape[1])] + _chain(z, F, order=range(z.shape[1] - 1, -1, -1)), mean, a, scale)


def nudge_from_old(old, idx, z, F, mean, a, scale):
    """The FMA chain started from old[i, idx[p]] instead of zero (no addition of its own)."""
    old, z, F = (np.asarray(x, dtype=np.float64) for x in (old, z, F))
    return _finish(_chain(z, F, start=np.ascontiguousarray(old[:, clamp(idx, old.shape[1])])), mean, a, scale)


WRONG_CHAINS = {"mul-then-add": nudge_mul_then_add, "reversed j": nudge_reversed_j, "started from old": nudge_from_old}


def nudge_integers(old, idx, z, F, mean, scale):
    """The same array for INTEGER inputs (|old| <= 2^20, |z|, |F| <= 8, integer mean) and a = 0.5, in NumPy integer
    arithmetic: every operation of the contract is exact on such data, so every evaluation order gives these bits."""
    old, z, F, mean = (np.asarray(x) for x in (old, z, F, mean))
    for x in (old, z, F, mean):
        assert np.array_equal(x, np.rint(x))
    oi, zi, Fi, mi = (x.astype(np.int64) for x in (old, z, F, mean))
    v = oi[:, clamp(idx, oi.shape[1])] + Fi @ zi.T
    if not scale:
        return v.astype(np.float64)
    return (v + mi[:, None]).astype(np.float64) * 0.5          # v/2 + mean/2: halves of integers below 2^22, exact


def violators(new, rows, lo, hi, open_flags):
    """bool (n,): the particle is outside some entry's bounds.  Entry k bounds row rows[k] of ``new`` to lo[k] .. hi[k];
    bit 0 / bit 1 of open_flags[k] make the lower / upper end exclusive (include/obe_hip.h: obe_mask_bounds)."""
    rows, flags = np.asarray(rows, dtype=np.int64), np.asarray(open_flags, dtype=np.int64)
    return co.violators(np.asarray(new)[rows], np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64),
                        (flags & 1) != 0, (flags & 2) != 0)


# ---- the inputs of the GPU file
def general_case(d, n, seed=None):
    """General doubles: rows of ``old`` of scale 1 .. D, F ~ N(0, 0.1), z ~ N(0, 1), indices with repeats, the mean of
    the rows.  (old, idx, z, F, mean), C-contiguous."""
    g = np.random.default_rng(11000 + 100 * d + n if seed is None else seed)
    old = g.normal(0.0, 1.0, (d, n)) * np.arange(1, d + 1)[:, None]
    idx = g.integers(0, n, n)
    z = g.standard_normal((n, d))
    F = g.normal(0.0, 0.1, (d, d))
    mean = old.mean(axis=1)
    return tuple(np.ascontiguousarray(x) for x in (old, idx, z, F, mean))


def integer_case(d, n, seed=None):
    """Data on which every operation is exact (with a = 0.5): integers, idx a permutation."""
    g = np.random.default_rng(9000 + 100 * d + n % 9973 if seed is None else seed)
    old = g.integers(-2 ** 20, 2 ** 20 + 1, (d, n)).astype(np.float64)
    idx = g.permutation(n).astype(np.int64)
    z = g.integers(-8, 9, (n, d)).astype(np.float64)
    F = g.integers(-8, 9, (d, d)).astype(np.float64)
    mean = g.integers(-1000, 1001, d).astype(np.float64)
    return old, idx, z, F, mean
