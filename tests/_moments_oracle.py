"""Two references for the K3 moment block (csrc/obe_moments.{h,hip}, the update's normalisation pass and the
constraint mask's second half), NumPy and the standard library only.  tests/test_moments_oracle_host.py pins both on
the CPU (against fractions.Fraction, the oracle package and np.cov) and shows that the inputs of the GPU file tell a
wrong kernel from a right one; tests/test_gpu_moments_exact.py compares the device with them.

The block of a cloud of d rows (include/obe_hip.h: obe_moments):
    [0] W = sum w   [1] W2 = sum w*w   [2, 2+d) mean   [2+d, 2+2d) m1 = sum x*w   [2+2d, 2+3d) m2 = sum (x*x)*w
    [2+3d, 2+4d) std   [2+4d, 2+4d+d*d) covariance, row-major, both triangles

(a) EXACT CLOUDS.  Integer particle values and weights q * 2^(shift - k) with sum q = 2^k, every row mirrored about
an integer centre: every sum the kernels form is a sum of integers times one power of two and stays below 2^53 units,
so it is exact in ANY order of additions — per thread, over the wave, over the waves, over the rows of the fold — and
the mean is the integer centre, so every deviation is an integer as well.  What remains are the single roundings the
kernels document (obe_moments.h: derive_first_moments, derive_covariance), applied here by the same IEEE operations
in float64: the device build has no contraction and no fast-math.  The whole block is therefore defined bit for bit.

(b) GENERAL DOUBLES.  longdouble_block() forms the block in two passes in np.longdouble; block_bounds() gives, value
by value, how far a kernel that follows the documented arithmetic may be from it.  The derivation is in its docstring:
nothing in it is fitted to what the device returns.
"""
import math

import numpy as np

U = 2.0 ** -53                 # unit roundoff of float64
ETA = 2.0 ** -1022             # what a product that underflows can lose (gradual underflow loses less)
U_REF = float(np.finfo(np.longdouble).eps)      # long double: one ulp of 1.0 (2^-63 on x86), taken whole
ROWS_PER_STRIDE = 65536        # 256 workgroups of 256 threads: the smallest grid stride of any producer
TREE_DEPTH = 32                # wave tree 6 + four waves 4 + 12 rows per lane of the fold 12 + its tree 6 = 28, rounded up
TILE = 8
Q_MAX = 2 ** 10
X_MAX = 512                    # |centre| <= 256, |deviation| <= 256


def block_len(d):
    return 2 + 4 * d + d * d


def sections(d):
    """Slices of the block by name."""
    return dict(W=slice(0, 1), W2=slice(1, 2), mean=slice(2, 2 + d), m1=slice(2 + d, 2 + 2 * d),
                m2=slice(2 + 2 * d, 2 + 3 * d), std=slice(2 + 3 * d, 2 + 4 * d), cov=slice(2 + 4 * d, block_len(d)))


# ------------------------------------------------------------------------------------------------ (a) exact clouds
def exact_cloud(g, d, n, shift=0):
    """(x, q, k): x d x n integers as float64, q int64 with sum q == 2^k and every q <= 2^10; the weights are
    w = q * 2^(shift - k) (exact_weights).  Each row is a half cloud of integer deviations |dev| <= 256 about an
    integer centre |c| <= 256 with weights q, its mirror image with the same q and, for odd n, a particle at the centre;
    then the particles are permuted.  sum x q = c 2^k exactly: the mean is c."""
    h, odd = n // 2, n % 2
    k = int(math.floor(math.log2(n))) + 8                  # n 2^7 < 2^k <= n 2^8: the average q is at most 256
    total = 1 << k
    c = g.integers(-256, 257, size=(d, 1))
    dev = g.integers(-256, 257, size=(d, h))
    qh = g.integers(1, 128, size=h).astype(np.int64)       # 2 sum qh <= 254 h < 2^k: something is always left to top up
    qc = np.zeros(0, dtype=np.int64)
    if odd:
        qc = np.array([total if h == 0 else 2 * int(g.integers(0, 64))], dtype=np.int64)     # (even: 2^k and 2 sum qh are)
    if h:
        rest = total - 2 * int(qh.sum()) - int(qc.sum())
        assert rest >= 0 and rest % 2 == 0
        each, extra = divmod(rest // 2, h)                 # the top-up spread over the pairs, not parked on one of them
        qh += each
        qh[:extra] += 1
    x = np.concatenate([c + dev, c - dev, np.broadcast_to(c, (d, odd))], axis=1)
    q = np.concatenate([qh, qh, qc])
    order = g.permutation(n)
    x, q = np.ascontiguousarray(x[:, order].astype(np.float64)), np.ascontiguousarray(q[order])
    assert int(q.sum()) == total and q.min() >= 0 and q.max() <= Q_MAX, (n, int(q.max()))
    assert np.abs(x).max() <= X_MAX
    return x, q, k


def exact_weights(q, k, shift=0):
    """w = q * 2^(shift - k): exact in float64."""
    return np.ldexp(q.astype(np.float64), shift - k)


def with_zero_weights(g, x, q, at, count):
    """The cloud with `count` more particles of weight zero (and arbitrary integer values) inserted before column
    `at`: they add exact zeros to every sum."""
    d = x.shape[0]
    extra = g.integers(-X_MAX, X_MAX + 1, size=(d, count)).astype(np.float64)
    return (np.ascontiguousarray(np.concatenate([x[:, :at], extra, x[:, at:]], axis=1)),
            np.concatenate([q[:at], np.zeros(count, dtype=np.int64), q[at:]]))


def exact_sums(x, q, k):
    """The integer sums behind the block, in int64: (Q2, M1, M2, c, S) with Q2 = sum q^2, M1 = sum x q = c 2^k,
    M2 = sum x^2 q, S = sum (x_i - c_i)(x_j - c_j) q.  Asserts what makes the device's sums exact in any order: sum q
    == 2^k, M1 a multiple of 2^k (an integer mean), and every sum OF MAGNITUDES below 2^53."""
    xi = np.asarray(x).astype(np.int64)
    assert np.array_equal(xi.astype(np.float64), x), "integer particle values"
    q = np.asarray(q, dtype=np.int64)
    total = 1 << k
    lim = 1 << 53
    assert int(q.sum()) == total and q.min() >= 0 and q.max() <= Q_MAX
    q2 = int((q * q).sum())
    m1 = xi @ q
    m2 = (xi * xi) @ q
    assert q2 < lim and int((np.abs(xi) @ q).max()) < lim and int(m2.max()) < lim
    assert np.all(m1 % total == 0), "the mean is an integer"
    c = m1 // total
    dev = xi - c[:, None]
    s = (dev * q) @ dev.T
    assert int(((np.abs(dev) * q) @ np.abs(dev).T).max()) < lim
    assert int(np.abs(c).max()) ** 2 < lim                  # m1 * m1 = c^2 2^(2 shift) is exact too
    return q2, m1, m2, c, s


def derive_block(w_sum, w2, m1, m2, s):
    """The documented single roundings, in float64, from the folded sums (obe_moments.h):
    mean = m1 / W, var = m2 - m1 * m1, std = sqrt(var), fact = W - W2 / W, cov = S * (1 / fact)."""
    d = len(m1)
    out = np.empty(block_len(d))
    sec = sections(d)
    w_sum, w2 = np.float64(w_sum), np.float64(w2)
    m1, m2, s = np.asarray(m1, dtype=np.float64), np.asarray(m2, dtype=np.float64), np.asarray(s, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        out[0], out[1] = w_sum, w2
        out[sec["mean"]] = m1 / w_sum
        out[sec["m1"]], out[sec["m2"]] = m1, m2
        out[sec["std"]] = np.sqrt(m2 - m1 * m1)
        fact = w_sum - w2 / w_sum
        scale = np.float64(1.0) / fact
        out[sec["cov"]] = (s * scale).reshape(-1)
    return out


def exact_block(x, q, k, shift=0):
    """The K3 block of an exact cloud, bit for bit: the sums in int64 (exact_sums asserts that none reaches 2^53),
    scaled by their power of two, then derive_block's roundings.  A cloud with fact == 0 (one particle carries all the
    weight) has NumPy's 0 * inf = NaN covariance."""
    q2, m1, m2, c, s = exact_sums(x, q, k)
    e = shift - k
    return derive_block(np.ldexp(1.0, shift), np.ldexp(float(q2), 2 * e), np.ldexp(m1.astype(np.float64), e),
                        np.ldexp(m2.astype(np.float64), e), np.ldexp(s.astype(np.float64), e))


# --------------------------------------------------------------------------------------------- (b) general doubles
def _ld(a):
    return np.asarray(a, dtype=np.longdouble)


def longdouble_sums(x, w):
    """(W, W2, m1, m2, mean, S) in long double, two passes: S about the long double mean."""
    x, w = np.atleast_2d(_ld(x)), _ld(w)
    w_sum, w2 = w.sum(), (w * w).sum()
    m1, m2 = (x * w).sum(axis=1), (x * x * w).sum(axis=1)
    mean = m1 / w_sum
    dev = x - mean[:, None]
    s = (dev * w) @ dev.T
    return w_sum, w2, m1, m2, mean, (s + s.T) / 2          # (bit-symmetric, as the device's two triangles are)


def longdouble_derive(w_sum, w2, m1, m2, s, mean=None):
    d = len(m1)
    out = np.empty(block_len(d), dtype=np.longdouble)
    sec = sections(d)
    with np.errstate(invalid="ignore", divide="ignore"):
        out[0], out[1] = w_sum, w2
        out[sec["mean"]] = m1 / w_sum if mean is None else mean
        out[sec["m1"]], out[sec["m2"]] = m1, m2
        out[sec["std"]] = np.sqrt(m2 - m1 * m1)
        out[sec["cov"]] = (s * (1 / (w_sum - w2 / w_sum))).reshape(-1)
    return out


def longdouble_block(x, w):
    """The K3 block in np.longdouble (returned as such: compare before rounding it)."""
    w_sum, w2, m1, m2, mean, s = longdouble_sums(x, w)
    return longdouble_derive(w_sum, w2, m1, m2, s)


def _gamma(m, u=U):
    return m * u / (1.0 - m * u)


def block_bounds(x, w, n=None):
    """Per value of the block, how far a device result may be from longdouble_block(x, w).  float64 array.

    Model of the device (obe_moments.h / .hip): every sum is  sum_p t_p  over the particles, t_p a product of the
    inputs with r roundings, added up in some tree in which no term passes through more than h additions:
        h = ceil(n / 65 536) + 32
    (the run of one thread at the smallest grid stride of any producer, then the wave tree 6, the four waves 4, the 12
    rows a lane of the fold adds 12, its tree 6).  The standard bound (Higham, Accuracy and Stability, 4.2) is then
        |computed - exact| <= gamma(h + r) sum |t_p| + n_r ETA,     gamma(m) = m u / (1 - m u),  u = 2^-53,
    ETA = 2^-1022 per product that can underflow (n_r of them, times the factor it is then multiplied by).

      W   = sum w              r = 0      bW  = gamma(h) sum |w|
      W2  = sum w*w            r = 1      bW2 = gamma(h + 1) sum w^2 + n ETA
      m1  = sum x*w            r = 1      bm1 = gamma(h + 1) sum |x| w + n ETA
      m2  = sum (x*x)*w        r = 2      bm2 = gamma(h + 2) sum x^2 w + n ETA
      mean = fl(m1 / W):  m1^/W^ - m1/W = (dm1 - mean dW) / W^, so
                               bmean = (bm1 + |mean| bW) / (W - bW), then + u (|mean| + bmean) for the division
      var = fl(m2^ - fl(m1^ m1^)):
                               bvar = bm2 + (2 |m1| + bm1) bm1 + u (|m1| + bm1)^2 + u (|var| + all of the former)
      std = fl(sqrt(var^)):    |sqrt a - sqrt b| <= min(|a - b| / sqrt b, sqrt |a - b|), then + 2 u std for a square
                               root good to one ulp
      S_ij: the device adds fma(d^_i, fl(d^_j w), .) with d^_i = fl(x_i - mean^_i) = dev_i + c_i + r_i, where dev is
        the deviation from the TRUE mean, c_i = mean_i - mean^_i (|c_i| <= bmean_i, the same for every particle) and
        r_i the rounding of the subtraction, |r_i| <= u (|dev_i| + bmean_i).  Multiplying out,
            sum d^_i d^_j w - S_ij = c_i sum dev_j w + c_j sum dev_i w + c_i c_j W + sum (r_i dev_j + r_j dev_i) w
                                     + sum (c_i r_j + c_j r_i + r_i r_j) w
        and the first two vanish: sum dev w = 0 about the true mean.  With A_i = sum |dev_i| w, B_ij = sum |dev_i dev_j| w
            |...| <= bmean_i bmean_j W + u (2 B_ij + bmean_i A_j + bmean_j A_i)
                     + u (bmean_i (A_j + bmean_j W) + bmean_j (A_i + bmean_i W)) + u^2 B'_ij
        B'_ij = sum (|dev_i| + bmean_i)(|dev_j| + bmean_j) w.  The summation itself (r = 1: the product d^_j w; the
        fma rounds once with the addition) costs gamma(h + 1) sum |d^_i d^_j| w <= gamma(h + 1) (1 + u)^2 B'_ij, and the
        underflow of d^_j w at most n ETA max|d^_i|.  bS_ij is the sum of these.
      fact = fl(W^ - fl(W2^ / W^)):  with R = W2 / W,
                               bR = (bW2 + R bW) / (W - bW) + u (R + that),  bfact = bW + bR + u (|fact| + bW + bR)
      scale = fl(1 / fact^):   bscale = bfact / (|fact| (|fact| - bfact)) + u (1/|fact| + that)
      cov = fl(S^ scale^):     bcov = bS (|scale| + bscale) + |S| bscale, then + u (|cov| + bcov)

    The reference's own error — long double sums of at most 2 + log2 n pairwise levels plus NumPy's 128-element
    leaves, taken as 256 u_ld sum |t| — and half an ulp for rounding nothing (the comparison is made in long double) are
    added: 256 u_ld times the same sums of magnitudes.
    """
    x, w = np.atleast_2d(_ld(x)), _ld(w)
    d, n_x = x.shape
    n = n_x if n is None else n
    h = -(-n // ROWS_PER_STRIDE) + TREE_DEPTH
    g0, g1, g2 = (_gamma(h + r) for r in (0, 1, 2))
    ref = 256 * U_REF
    w_sum, w2, m1, m2, mean, s = longdouble_sums(x, w)
    aw = np.abs(w)
    sw, sw2 = aw.sum(), (w * w).sum()
    sx, sx2 = (np.abs(x) * aw).sum(axis=1), (x * x * aw).sum(axis=1)
    xmax = np.abs(x).max(axis=1)
    b_w = g0 * sw
    b_w2 = g1 * sw2 + n * ETA
    b_m1 = g1 * sx + n * ETA
    b_m2 = g2 * sx2 + n * ETA * xmax * xmax
    amean = np.abs(mean)
    b_mean = (b_m1 + amean * b_w) / (w_sum - b_w)
    b_mean = b_mean + U * (amean + b_mean)
    var = m2 - m1 * m1
    am1 = np.abs(m1)
    b_var = b_m2 + (2 * am1 + b_m1) * b_m1 + U * (am1 + b_m1) ** 2
    b_var = b_var + U * (np.abs(var) + b_var)
    std = np.sqrt(np.maximum(var, 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        b_std = np.minimum(np.where(std > 0, b_var / std, np.inf), np.sqrt(b_var))
    b_std = b_std + 2 * U * (std + b_std)
    dev = np.abs(x - mean[:, None])
    a = (dev * aw).sum(axis=1)
    b = (dev * aw) @ dev.T
    devp = dev + b_mean[:, None]
    bp = (devp * aw) @ devp.T
    bm_a = np.outer(b_mean, a)
    bm_bm = np.outer(b_mean, b_mean) * sw
    b_s = (bm_bm + U * (2 * b + bm_a + bm_a.T) + U * (bm_a + bm_a.T + 2 * bm_bm) + U * U * bp
           + g1 * (1 + U) ** 2 * bp + n * ETA * np.add.outer(devp.max(axis=1), devp.max(axis=1)))
    r = w2 / w_sum
    b_r = (b_w2 + r * b_w) / (w_sum - b_w)
    b_r = b_r + U * (r + b_r)
    fact = w_sum - r
    afact = np.abs(fact)
    b_fact = b_w + b_r + U * (afact + b_w + b_r)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = 1 / afact
        b_scale = b_fact / (afact * (afact - b_fact))
        b_scale = b_scale + U * (scale + b_scale)
        b_cov = b_s * (scale + b_scale) + np.abs(s) * b_scale
        b_cov = b_cov + U * (np.abs(s) * scale + b_cov)
    if not afact > b_fact:
        b_cov = np.full((d, d), np.inf)
    out = np.empty(block_len(d), dtype=np.longdouble)
    sec = sections(d)
    out[0], out[1] = b_w + ref * sw, b_w2 + ref * sw2
    out[sec["mean"]] = b_mean + ref * (sx / w_sum + amean)
    out[sec["m1"]], out[sec["m2"]] = b_m1 + ref * sx, b_m2 + ref * sx2
    out[sec["std"]] = b_std + ref * np.where(std > 0, (sx2 + am1 * sx) / np.where(std > 0, std, 1), 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        out[sec["cov"]] = (b_cov + ref * (b * scale + np.abs(s) * scale * (1 + r / afact))).reshape(-1)
    return out.astype(np.float64)


def worst_fraction(got, ref, bound, d):
    """max |got - ref| / bound per quantity (name -> fraction) of a block, or of its first-moment part; a NaN, or an
    error where the bound is 0, counts as inf."""
    got, ref, bound = _ld(got), _ld(ref), _ld(bound)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(err == 0, 0.0, err / bound)
    frac = np.where(np.isnan(frac), np.inf, frac).astype(np.float64)
    return {name: float(frac[sl].max()) for name, sl in sections(d).items() if sl.stop <= len(got)}


# -------------------------------------------------------------------- the general inputs of the GPU file, and mutants
def special_columns(n):
    """The particles a kernel is most likely to lose: the last one, the first of the second workgroup and of the last
    workgroup, the first of the second grid stride."""
    cols = {n - 1}
    if n > 256:
        cols |= {256, 256 * ((n - 1) // 256)}
    if n > ROWS_PER_STRIDE:
        cols.add(ROWS_PER_STRIDE)
    return sorted(cols)


def general_cloud(g, d, n, total=0.8125):
    """(x, w): rows of distinct scale (10^-3 ... 10^3) with mean / sd from 0 up to 10^6, weights spanning 300 decades
    (a fifth of them within three decades of the largest), one particle that carries a third of the weight, the
    special_columns at the top of the range — and sum w = `total`, not 1: a kernel that takes sum w for granted
    shows."""
    sd = 10.0 ** g.uniform(-3, 3, size=(d, 1))
    ratio = np.concatenate([[1e6, 0.0], 10.0 ** g.uniform(-1, 6, size=d)])[:d].reshape(d, 1) * g.choice([-1, 1], (d, 1))
    x = sd * (g.standard_normal((d, n)) + ratio)
    if d > 1:                                              # neighbouring rows are correlated
        x[1:] += 0.5 * (x[:-1] - sd[:-1] * ratio[:-1]) * (sd[1:] / sd[:-1])
    w = 10.0 ** (-300.0 * g.random(n) ** 3)
    cols = special_columns(n)
    w[cols] = 1.0
    if n > 2:
        heavy = int(g.integers(1, n - 1))
        while heavy in cols:
            heavy = (heavy + 1) % (n - 1)
        w[heavy] = 0.0
        w[heavy] = 0.5 * w.sum()
    w *= total / w.sum()
    return np.ascontiguousarray(x), w


def _replay_tiles(d, first, cov, pad_first=None, pad_cov=None, swap=False):
    """The block the tiled launches of obe_moments.hip leave when they store `first` (a dict mean / m1 / m2 / std of
    per-row values) and `cov` through the kernels' own index expressions, in launch order.  pad_first / pad_cov: values
    of d rounded up to whole tiles of rows, which a kernel whose row guard works in whole tiles would store too —
    wherever in the block (or beyond: dropped here) the index expressions then point.  swap: the 8 x 8 block of a pair
    of different tiles stored transposed."""
    out = np.full(block_len(d), np.nan, dtype=np.longdouble)
    d_rows = d if pad_first is None else -(-d // TILE) * TILE
    src = first if pad_first is None else pad_first
    scov = cov if pad_cov is None else pad_cov
    base = 2 + 4 * d
    for d0 in range(0, d, TILE):
        for r in range(d0, min(d0 + TILE, d_rows)):
            for slot, name in enumerate(("mean", "m1", "m2", "std")):
                out[2 + slot * d + r] = src[name][r]
    for i0 in range(0, d, TILE):
        for j0 in range(i0, d, TILE):
            for e in range(TILE * TILE):
                i, j = i0 + e // TILE, j0 + e % TILE
                if i < d_rows and j < d_rows and (i0 != j0 or i <= j):
                    c = scov[i, j]
                    if swap and i0 != j0:                  # (a padded row's sums are zero)
                        si, sj = i0 + e % TILE, j0 + e // TILE
                        c = scov[si, sj] if si < len(scov) and sj < len(scov) else 0.0
                    for at in (i * d + j, j * d + i):
                        if at < d * d:
                            out[base + at] = c
    return out


def mutants(x, w):
    """name -> block (long double) of a reference with one plausible kernel mistake built in; only the mistakes that
    apply to the cloud's shape are returned.  tests/test_moments_oracle_host.py requires every one of them to differ
    from longdouble_block(x, w) by more than block_bounds(x, w) in at least one value, on every general case of the GPU
    file: the comparison there can then tell such a kernel from a right one."""
    d, n = x.shape
    out = {}

    def dropped(col):
        keep = np.arange(n) != col
        return longdouble_block(x[:, keep], w[keep])

    if n > 1:
        out["the last particle dropped"] = dropped(n - 1)
    if n > 256:
        out["particle 256 dropped"] = dropped(256)
        out["the last workgroup's first particle dropped"] = dropped(256 * ((n - 1) // 256))
    if n > ROWS_PER_STRIDE:
        out["particle 65 536 dropped"] = dropped(ROWS_PER_STRIDE)
    w_sum, w2, m1, m2, mean, s = longdouble_sums(x, w)
    out["W = 1 used for sum w"] = longdouble_derive(np.longdouble(1), w2, m1, m2, s)
    out["W = 1 used for sum w"][:2] = w_sum, w2
    no_w2 = longdouble_derive(w_sum, w2, m1, m2, s)
    no_w2[sections(d)["cov"]] = (s * (1 / w_sum)).reshape(-1)
    out["the W2 / W term left out"] = no_w2
    if d > 16:
        good = longdouble_derive(w_sum, w2, m1, m2, s)
        sec = sections(d)
        first = {name: good[sec[name]] for name in ("mean", "m1", "m2", "std")}
        cov = good[sec["cov"]].reshape(d, d)

        def replay(**kw):
            blk = _replay_tiles(d, first, cov, **kw)
            blk[:2] = good[:2]
            return blk

        assert np.array_equal(replay(), good)                   # the replay itself reproduces the block
        out["a tile pair's i and j swapped"] = replay(swap=True)
        shift = np.zeros(d, dtype=np.longdouble)
        shift[TILE:] = mean[TILE:] - mean[:-TILE]               # deviations taken from the previous tile's means
        stale = longdouble_derive(w_sum, w2, m1, m2, s + np.outer(shift, shift) * w_sum)
        out["a mean taken from the previous tile"] = stale
        if d % TILE:
            d_pad = -(-d // TILE) * TILE
            xp = np.concatenate([x, np.repeat(x[-1:], d_pad - d, axis=0)])
            padded = longdouble_block(xp, w)
            psec = sections(d_pad)
            out["row d - 1 read in place of a short tile's zero padding"] = replay(
                pad_first={name: padded[psec[name]] for name in first}, pad_cov=padded[psec["cov"]].reshape(d_pad, d_pad))
    return out


# the general cases of tests/test_gpu_moments_exact.py (tests/test_moments_oracle_host.py runs the mutants on them)
GENERAL_CASES = ([(d, n) for n in (293, 65537) for d in range(1, 17)] + [(d, 5000) for d in (17, 33, 40)]
                 + [(4, 2 ** 21 + 293)])


def general_case(d, n):
    """(x, w) of one general case: the same arrays wherever they are asked for."""
    return general_cloud(np.random.default_rng(7000003 * d + n), d, n)
