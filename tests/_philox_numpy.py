"""A numpy twin of the problem generator (csrc/kernels.hpp: struct Philox, k_gen_X, k_gen_y; cdhip.hip: cdh_generate).

Philox4x32-10 and the map from its words to two uniforms are integer arithmetic plus exactly rounded IEEE operations, so
the twin reproduces them bit for bit.  Box-Muller is not: log, sqrt, cos and sin come from a math library, and the device's
differs from numpy's.  So every normal is returned twice: the fp64 value numpy computes, and a np.longdouble REFERENCE
that runs log, sqrt, cos, sin and the product in 64-bit-mantissa arithmetic on the same fp64 u1 and the same fp64 angle
2 pi u2 -- the value the device's fp64 chain approximates.  `rad` = sqrt(-2 log u1) comes with it: it is the scale of the
error a log/sqrt/sincos chain can make (|cos|, |sin| <= 1), and the unit the comparisons below are written in.

`Variant` restates the generator with one thing wrong (tests/test_philox_host.py shows that each such mistake fails the
comparison tests/test_gpu_generator.py makes).
"""
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

assert np.finfo(np.longdouble).nmant >= 63, "the reference needs an extended-precision long double (x86-64)"

M32 = np.uint64(0xFFFFFFFF)
SH32 = np.uint64(32)
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
TWO_PI = 6.283185307179586476925286766559        # the literal of kernels.hpp; rounds to fp64 2 pi
assert TWO_PI == 2.0 * math.pi
X_ABS_MAX = 8.66                                 # u1 >= 2^-54: |x| <= sqrt(108 ln 2) = 8.652...
assert math.sqrt(108.0 * math.log(2.0)) < X_ABS_MAX
U64 = 2.0 ** -53
ULPS = 8                                         # ceiling for the device's log, sqrt, sincos chain, in 2^-53 rad

STREAM_X, STREAM_NOISE, STREAM_BETA = 0, 1, 2
GEN_X_MAX_BLOCKS, GEN_Y_MAX_BLOCKS, GEN_BLOCK, GEN_COL_SLICE = 2048, 4096, 256, 32768

# the generator with one mistake in it; the default is the generator
Variant = namedtuple("Variant", "m0 rounds swap col_mask drop_ctr_hi", defaults=(PHILOX_M0, 10, False, None, False))
EXACT = Variant()


def _u64(a):
    return np.asarray(a, dtype=np.uint64)


def philox4x32_10(c0, c1, c2, c3, k0, k1, rounds=10, m0=PHILOX_M0, m1=PHILOX_M1):
    """Philox4x32 (Salmon et al., Random123) over arrays of 32-bit words held in uint64; returns the four output words."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_u64(a) & M32 for a in (c0, c1, c2, c3, k0, k1)))
    m0, m1, w0, w1 = np.uint64(m0), np.uint64(m1), np.uint64(PHILOX_W0), np.uint64(PHILOX_W1)
    for _ in range(rounds):
        p0, p1 = m0 * c0, m1 * c2                 # 32 x 32 bits: no overflow in 64
        hi0, lo0, hi1, lo1 = p0 >> SH32, p0 & M32, p1 >> SH32, p1 & M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + w0) & M32, (k1 + w1) & M32
    return c0, c1, c2, c3


def _to_uniform(hi_word, lo_word):
    """((w0 >> 5) 2^26 + (w1 >> 6) + 0.5) 2^-53 in fp64: k + 0.5 needs 54 bits once k >= 2^52 and rounds to even."""
    k = (hi_word >> np.uint64(5)).astype(np.float64) * 67108864.0 + (lo_word >> np.uint64(6)).astype(np.float64)
    return (k + 0.5) * (1.0 / 9007199254740992.0)


def uniform_of_k(k):
    """The uniform of the 53-bit integer k = (w0 >> 5) 2^26 + (w1 >> 6); k = 0 and k = 2^53 - 1 are the ends."""
    k = int(k)
    assert 0 <= k < 1 << 53
    return _to_uniform(_u64((k >> 26) << 5), _u64((k & ((1 << 26) - 1)) << 6))


def uniforms(seed, ctr, col, stream, v=EXACT):
    """Philox::uniforms: two fp64 uniforms in (0, 1] of (seed, 64-bit counter, column, stream).  ctr, col: arrays."""
    seed = int(seed) & ((1 << 64) - 1)
    ctr, col = _u64(ctr), _u64(col)
    if v.col_mask is not None:
        col = col % np.uint64(v.col_mask)
    chi = np.zeros_like(ctr) if v.drop_ctr_hi else ctr >> SH32
    w = philox4x32_10(ctr & M32, chi, col, np.uint64(stream), np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32),
                      rounds=v.rounds, m0=v.m0)
    return _to_uniform(w[0], w[1]), _to_uniform(w[2], w[3])


def box_muller(u1, u2):
    """(cos member, sin member), each as (fp64 value, longdouble reference), and rad (fp64), of fp64 uniforms."""
    u1, u2 = np.asarray(u1, dtype=np.float64), np.asarray(u2, dtype=np.float64)
    th = TWO_PI * u2                                            # one fp64 product, as on the device
    rad = np.sqrt(-2.0 * np.log(u1))
    L = np.longdouble
    radL = np.sqrt(L(-2.0) * np.log(u1.astype(L)))
    thL = th.astype(L)
    return (rad * np.cos(th), radL * np.cos(thL)), (rad * np.sin(th), radL * np.sin(thL)), radL.astype(np.float64)


def normal(seed, gi, col, stream, v=EXACT):
    """Philox::normal: number gi of (col, stream) is member gi & 1 of pair gi >> 1.  -> (fp64, longdouble, rad)."""
    gi = _u64(gi)
    gi, col = np.broadcast_arrays(gi, _u64(col))
    u1, u2 = uniforms(seed, gi >> np.uint64(1), col, stream, v)
    (c, cL), (s, sL), rad = box_muller(u1, u2)
    odd = (gi & np.uint64(1)).astype(bool) ^ bool(v.swap)
    return np.where(odd, s, c), np.where(odd, sL, cL), rad


def x_entry(seed, rows, cols, v=EXACT):
    """X[row, col] of the GLOBAL row index: (row >> 1, col, stream 0), even rows cos, odd rows sin."""
    return normal(seed, rows, cols, STREAM_X, v)


def x_matrix(seed, row0, n, col0, p, v=EXACT, stream=STREAM_X):
    """x_entry over rows [row0, row0 + n) x columns [col0, col0 + p), one Box-Muller per row pair (as k_gen_X forms it)."""
    row0, n = int(row0), int(n)
    gp0, gp1 = row0 >> 1, (row0 + n + 1) >> 1
    gp = np.arange(gp0, gp1, dtype=np.uint64)[:, None]
    col = np.arange(col0, col0 + p, dtype=np.uint64)[None, :]
    u1, u2 = uniforms(seed, gp, col, stream, v)
    (c, cL), (s, sL), rad = box_muller(u1, u2)
    if v.swap:
        c, cL, s, sL = s, sL, c, cL
    lo, hi = row0 - 2 * gp0, row0 - 2 * gp0 + n

    def weave(a, b):
        out = np.empty((2 * a.shape[0], a.shape[1]), dtype=a.dtype)
        out[0::2], out[1::2] = a, b
        return out[lo:hi]
    return weave(c, s), weave(cL, sL), weave(rad, rad)


def noise(seed, rows, v=EXACT):
    """e[row]: (row >> 1, column 0, stream 1), the member by the row's parity."""
    return normal(seed, rows, 0, STREAM_NOISE, v)


def noise_vector(seed, row0, n, v=EXACT):
    """noise over rows [row0, row0 + n), one Box-Muller per row pair."""
    return tuple(a[:, 0] for a in x_matrix(seed, row0, n, 0, 1, v, stream=STREAM_NOISE))


def beta_star(seed, s, v=EXACT):
    """beta*_j = z (1 + u), z the cos member of (ctr j, col 0, stream 2), u the first uniform of (ctr j, col 1, stream 2).
    -> (fp64, longdouble reference, |z| (1 + u) in fp64)."""
    j = np.arange(int(s), dtype=np.uint64)
    z, zL, _ = normal(seed, 2 * j, 0, STREAM_BETA, v)
    u, _ = uniforms(seed, j, 1, STREAM_BETA, v)
    ref = zL * (np.longdouble(1.0) + u.astype(np.longdouble))
    return z * (1.0 + u), ref, np.abs(ref).astype(np.float64)


def _fma(a, b, c):
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    return float(Fraction(a) * Fraction(b) + Fraction(c))       # Fraction -> float rounds to nearest even


def y_exact(Xs, bstar, noise_term=None):
    """k_gen_y's chain acc = fma(x_j, b_j, acc), j < s, from acc = 0, with every fma rounded once; then + noise_term in
    fp64 when there is one.  Xs: n x s (any float dtype; widened exactly).  A Python loop: small n only."""
    Xs = np.asarray(Xs, dtype=np.float64)
    n, s = Xs.shape
    assert len(bstar) == s
    out = np.zeros(n)
    for i in range(n):
        acc = 0.0
        for j in range(s):
            acc = _fma(float(Xs[i, j]), float(bstar[j]), acc)
        out[i] = acc
    return out if noise_term is None else out + np.asarray(noise_term, dtype=np.float64)


# ---- the launch arithmetic of cdh_generate, restated -----------------------------------------------------------------
def gen_x_grid(n):
    """(blocks of k_gen_X along x, row pairs one trip of its grid-stride loop covers)."""
    gx = max(1, min(GEN_X_MAX_BLOCKS, -(-((n + 3) // 2) // GEN_BLOCK)))
    return gx, gx * GEN_BLOCK


def gen_y_grid(n):
    gy = max(1, min(GEN_Y_MAX_BLOCKS, -(-n // GEN_BLOCK)))
    return gy, gy * GEN_BLOCK


def x_trip_of_row(n, row0=0):
    """The trip of k_gen_X's grid-stride loop that writes each local row."""
    _, stride = gen_x_grid(n)
    i = np.arange(n, dtype=np.int64)
    return (((row0 + i) >> 1) - (row0 >> 1)) // stride


# ---- the comparisons tests/test_gpu_generator.py makes ---------------------------------------------------------------
def x_errors(dev, ref, rad):
    """|dev - ref| in units of 2^-53 rad, elementwise in fp64 (0 where both are exactly equal, inf where rad = 0 and they
    are not); non-finite or out-of-range device values count as inf."""
    dev = np.asarray(dev, dtype=np.float64)
    d = np.abs(dev.astype(np.longdouble) - ref).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(d == 0.0, 0.0, d / (U64 * rad))
    e[~(np.isfinite(dev) & (np.abs(dev) < X_ABS_MAX))] = np.inf
    return e


def check_f64(dev, ref, rad):
    """-> (mask of entries that break |dev - ref| <= ULPS 2^-53 rad, or are not finite with |x| < 8.66; the largest error
    in 2^-53 rad)."""
    e = x_errors(dev, ref, rad)
    return e > ULPS, float(e.max()) if e.size else 0.0


def f32_expected(ref, rad):
    """What (float)(fp64 value) may be when the fp64 value lies within ULPS 2^-53 rad of the longdouble `ref`:
    -> (np.float32(ref), the other admissible float where ref lies that close to an fp32 rounding boundary else the
    same float, the mask of such entries).  Decided from the reference alone."""
    L = np.longdouble
    f = ref.astype(np.float32)
    up, dn = np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))
    tol = (ULPS * U64) * rad.astype(L)
    mid_up, mid_dn = (f.astype(L) + up.astype(L)) / 2, (f.astype(L) + dn.astype(L)) / 2
    near_up, near_dn = np.abs(ref - mid_up) <= tol, np.abs(ref - mid_dn) <= tol
    alt = np.where(near_up, up, np.where(near_dn, dn, f))
    return f, alt, near_up | near_dn


def check_f32(dev, ref, rad):
    """-> (mask of entries that are neither np.float32(ref) nor its admitted neighbour, or not finite with |x| < 8.66;
    the number of entries with an admitted neighbour)."""
    dev = np.asarray(dev)
    assert dev.dtype == np.float32
    f, alt, near = f32_expected(ref, rad)
    bad = ~((dev == f) | (dev == alt)) | ~(np.isfinite(dev) & (np.abs(dev) < X_ABS_MAX))
    return bad, int(near.sum())


F32_EXCEPTION_SHARE = 1e-6


def check_x(dev, ref, rad):
    """The comparison of a downloaded X (or noise vector) with the twin, by its dtype.  -> (bad mask, dict of figures)."""
    dev = np.asarray(dev)
    if dev.dtype == np.float64:
        bad, worst = check_f64(dev, ref, rad)
        return bad, {"max_err_in_2^-53_rad": worst}
    bad, near = check_f32(dev, ref, rad)
    assert near <= F32_EXCEPTION_SHARE * dev.size, (near, dev.size)
    return bad, {"f32_boundary_exceptions": near}
