"""The context shift's arithmetic (csrc/common/tk_kv_shift.h) restated in NumPy, exactly.

A key row that moves down by d positions is re-rotated by -d: for every adjacent pair (a, b) of the row, widened from f16 to fp32, with
c = rope_cos[d][i], s = rope_sin[d][i]:
    k'[2i]     = f16( fma( b, s, a * c) )
    k'[2i + 1] = f16( fma(-a, s, b * c) )
the product rounded to fp32 first, then ONE rounding of the fma; a value row is a bit copy.

fma(x, y, z) for an f16 x and fp32 y, z is computed without an fma instruction: x * y has at most 11 + 24 significant bits, so it is exact in
float64; t = x * y + z is then rounded to float64 once, the rounding error err = exact - t is recovered exactly (Knuth's TwoSum), and t is
rounded to fp32.  The two roundings differ from one only when t sits exactly half way between two neighbouring fp32 values while the exact sum does
not (a float64 rounding can land ON such a midpoint but never jump over one): there err says on which side the exact sum lies.  fma_scalar is the
same thing by rational arithmetic, for the tests to hold the vector form against."""
import math
from fractions import Fraction

import numpy as np

# f16 bit patterns with a history: infinities, NaNs with payloads, the smallest and largest denormals, zeros, the largest normal, the smallest
# normal (tests/test_prefix_cache_gpu.py fills its caches with the same)
SPECIAL_F16 = np.array([0x7C00, 0xFC00, 0x7E00, 0xFE01, 0x7FFF, 0xFFFF, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0000, 0x8000, 0x7BFF, 0x0400], np.uint16)


def rope_table(max_ctx, head_dim, rope_theta):
    """(cos, sin) float32 [max_ctx][head_dim / 2] the way TkLlmSession::init computes them: float64 pow, cos and sin of p * theta_i, rounded to fp32"""
    half = head_dim // 2
    base = float(np.float32(rope_theta))
    cs, sn = np.empty((max_ctx, half), np.float32), np.empty((max_ctx, half), np.float32)
    for i in range(half):
        theta = math.pow(base, -2.0 * i / float(head_dim))
        for p in range(max_ctx):
            a = float(p) * theta
            cs[p, i] = np.float32(math.cos(a))
            sn[p, i] = np.float32(math.sin(a))
    return cs, sn


def _round_once(t, err):
    """float64 t = the rounded sum, err = exact sum - t: the fp32 nearest (ties to even) to the EXACT sum"""
    f = t.astype(np.float32)
    fd = f.astype(np.float64)
    toward = np.where(t > fd, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
    other = np.nextafter(f, toward)
    od = other.astype(np.float64)
    tie = np.isfinite(t) & (t != fd) & (np.abs(t - fd) == np.abs(od - t))
    moved = tie & np.isfinite(err) & (err != 0.0)
    to_other = moved & (np.sign(err) == np.sign(od - fd))
    # t lies half way between f (where ties-to-even sent it) and other; the exact sum lies on one side of t and decides instead
    return np.where(to_other, other, f).astype(np.float32)


def fma_f16_f32(x, y, z):
    """fma(x, y, z) rounded once to fp32; x holds f16 values (as float32), y and z are float32 arrays"""
    with np.errstate(all="ignore"):
        prod = x.astype(np.float64) * y.astype(np.float64)  # exact: 11 x 24 bits
        zd = z.astype(np.float64)
        t = prod + zd
        bb = t - prod                                       # TwoSum: err = (prod - (t - bb)) + (zd - bb), exact
        err = (prod - (t - bb)) + (zd - bb)
        return _round_once(t, err)


def _f32_from_fraction(q):
    """the fp32 nearest (ties to even) to the rational q != 0, normal range"""
    sign = -1 if q < 0 else 1
    q = abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    scaled = q / Fraction(2) ** (e - 23)  # in [2^23, 2^24)
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    return np.float32(sign * math.ldexp(n, e - 23))


def fma_scalar(x, y, z):
    """fma of three finite floats (held exactly by float64), ONE rounding to fp32, by rational arithmetic (math.fma, where an interpreter has it,
    rounds to float64: rounding that again to fp32 is the double rounding the vector form avoids)"""
    q = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
    if q == 0:
        return np.float32(float(x) * float(y) + float(z))  # the sign of an exact zero: what IEEE addition gives
    return _f32_from_fraction(q)


def shift_key_rows(k_bits, cos_d, sin_d):
    """k_bits: uint16 [..., head_dim] key rows; cos_d / sin_d: float32 [head_dim / 2], the table's row d.  The rows re-rotated by -d, as uint16"""
    k = np.ascontiguousarray(k_bits, np.uint16)
    a = k[..., 0::2].view(np.float16).astype(np.float32)
    b = k[..., 1::2].view(np.float16).astype(np.float32)
    c = np.ascontiguousarray(cos_d, np.float32)
    s = np.ascontiguousarray(sin_d, np.float32)
    with np.errstate(all="ignore"):
        ac = a * c  # one fp32 rounding each
        bc = b * c
        even = fma_f16_f32(b, np.broadcast_to(s, b.shape), ac)
        odd = fma_f16_f32(-a, np.broadcast_to(s, a.shape), bc)
        out = np.empty(k.shape, np.float16)
        out[..., 0::2] = even.astype(np.float16)
        out[..., 1::2] = odd.astype(np.float16)
    return out.view(np.uint16)


def kv_shift_ref(kcache, vcache, rope_cos, rope_sin, seq, p0, p1, delta):
    """caches uint16 [n_layer][max_seq][n_kv_head][max_ctx][head_dim]; returns the shifted copies: rows [p0, p1) of `seq` at [p0 + delta, p1 + delta)"""
    assert delta < 0 <= p0 + delta and p0 < p1 <= kcache.shape[3]
    d = -delta
    k, v = kcache.copy(), vcache.copy()
    k[:, seq, :, p0 - d:p1 - d] = shift_key_rows(kcache[:, seq, :, p0:p1], rope_cos[d], rope_sin[d])
    v[:, seq, :, p0 - d:p1 - d] = vcache[:, seq, :, p0:p1]
    return k, v


def kv_shift_rows_ref(k_rows, v_rows, rope_cos, rope_sin, p0, p1, delta):
    """one (layer, sequence) in kv_read's layout uint16 [max_ctx][n_kv_head][head_dim]; returns the shifted copies"""
    d = -delta
    k, v = k_rows.copy(), v_rows.copy()
    k[p0 - d:p1 - d] = shift_key_rows(k_rows[p0:p1], rope_cos[d], rope_sin[d])
    v[p0 - d:p1 - d] = v_rows[p0:p1]
    return k, v


def same_f16_bits(got, want):
    """uint16 arrays equal bit for bit, a NaN comparing equal to any NaN"""
    g, w = np.asarray(got, np.uint16), np.asarray(want, np.uint16)
    gn, wn = (g & 0x7FFF) > 0x7C00, (w & 0x7FFF) > 0x7C00
    return g.shape == w.shape and bool(np.array_equal(gn, wn)) and bool(np.array_equal(g[~gn], w[~wn]))


def seeded_caches(shape, seed, finite=False):
    """(k, v) uint16 of `shape` = [n_layer][max_seq][n_kv_head][max_ctx][head_dim]: seeded bit patterns, the special ones scattered in and one for
    certain in every row; finite: normal-range finite values only (|x| < 256)"""
    rng = np.random.default_rng(seed)
    if finite:
        k = (rng.standard_normal(shape) * 8).clip(-255, 255).astype(np.float16).view(np.uint16)
        v = (rng.standard_normal(shape) * 8).clip(-255, 255).astype(np.float16).view(np.uint16)
        return k, v
    k = rng.integers(0, 65536, shape).astype(np.uint16)
    v = rng.integers(0, 65536, shape).astype(np.uint16)
    for a in (k, v):
        flat = a.reshape(-1)
        flat[rng.integers(0, flat.size, max(16, flat.size // 50))] = rng.choice(SPECIAL_F16, max(16, flat.size // 50))
    rows = k.reshape(-1, shape[-1])
    rows[:, 0] = SPECIAL_F16[np.arange(rows.shape[0]) % len(SPECIAL_F16)]
    rows[:, 1] = SPECIAL_F16[(np.arange(rows.shape[0]) // len(SPECIAL_F16)) % len(SPECIAL_F16)]  # the pair's other half varies against it
    return k, v
