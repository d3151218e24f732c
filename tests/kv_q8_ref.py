"""The Q8_0 KV cache's quantiser (csrc/common/tk_kv_q8.h) restated in float32 NumPy, for tests/test_kv_q8_cpu.py and tests/test_kv_q8_gpu.py.

A cached row is the f16-rounded key or value widened to fp32; per block of 32, ggml's quantize_row_q8_0_ref value for value:
    amax = max |x|;  d = amax / 127;  id = d ? 1 / d : 0;  q[i] = roundf(x[i] * id);  stored scale = f16(d)
roundf rounds halves away from zero.  Every step is one correctly rounded float32 operation, which NumPy's float32 arithmetic is too.  The value of
an element is f16_to_f32(scale) * q, exact in fp32.

lossless_rows() makes rows that the quantiser keeps exactly: per block x = n * 2^e with integer |n| <= 127, one |n| = 127, e in -10 .. -4 unless the
caller names another range; then amax = 127 * 2^e, d = 2^e, id = 2^-e, q = n and d * q = x.

The general (lossy) rows and the passes of the deep-window probe tests are below the quantiser."""
import functools

import numpy as np

import attention_geometry_cases as G

BLOCK = 32


def roundf(v):
    """roundf on float32 values below 2^23: the integer part and the remainder are exact, so halves go away from zero and nothing else moves"""
    v = np.asarray(v, np.float32)
    t = np.trunc(v)
    r = v - t
    return (t + (r >= np.float32(0.5)).astype(np.float32) - (r <= np.float32(-0.5)).astype(np.float32)).astype(np.float32)


def quantize(rows_f16_bits):
    """uint16 f16 bits [..., head_dim] -> (int8 [..., head_dim], uint16 scale bits [..., head_dim / 32])"""
    bits = np.asarray(rows_f16_bits, np.uint16)
    assert bits.shape[-1] % BLOCK == 0
    x = bits.view(np.float16).astype(np.float32).reshape(bits.shape[:-1] + (bits.shape[-1] // BLOCK, BLOCK))
    amax = np.abs(x).max(axis=-1)
    with np.errstate(divide="ignore", over="ignore"):
        d = (amax / np.float32(127.0)).astype(np.float32)
        inv = np.where(d != 0, np.float32(1.0) / np.where(d != 0, d, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
    q = roundf(x * inv[..., None]).astype(np.int8)
    return q.reshape(bits.shape), d.astype(np.float16).view(np.uint16)


def value(q, scale_bits):
    """the float32 value of every cached element"""
    q = np.asarray(q, np.int8)
    d = np.asarray(scale_bits, np.uint16).view(np.float16).astype(np.float32)
    return (np.repeat(d, BLOCK, axis=-1) * q.astype(np.float32)).astype(np.float32)


def inverse_overflows(rows_f16_bits):
    """True where a block's amax is so small that 1 / d overflows float32 (such blocks are left out of the tests, as llm_step_cases.py does)"""
    bits = np.asarray(rows_f16_bits, np.uint16)
    x = bits.view(np.float16).astype(np.float32).reshape(bits.shape[:-1] + (bits.shape[-1] // BLOCK, BLOCK))
    d = (np.abs(x).max(axis=-1) / np.float32(127.0)).astype(np.float32)
    with np.errstate(divide="ignore", over="ignore"):
        return (d != 0) & ~np.isfinite(np.float32(1.0) / np.where(d != 0, d, np.float32(1.0)))


def lossless_rows(shape, seed, exponents=(-10, -4)):
    """f16 bits of rows the quantiser keeps exactly; shape[-1] % 32 == 0.  exponents: the inclusive range the blocks' e is drawn from, within
    -14 .. 8: n * 2^e is then a normal f16 number (|n| * 2^e >= 2^-14, 127 * 2^8 < 65504), and 127 * 2^e / 127, 1 / 2^e and n * 2^e * 2^-e are
    exact in float32.  Key rows of a deep window take a lower range: their scores must not collapse the softmax onto a few positions"""
    lo, hi = exponents
    assert -14 <= lo <= hi <= 8
    rng = np.random.default_rng([91, seed])
    nb = shape[-1] // BLOCK
    n = rng.integers(-127, 128, shape[:-1] + (nb, BLOCK))
    at = rng.integers(0, BLOCK, shape[:-1] + (nb,))
    np.put_along_axis(n, at[..., None], rng.choice([-127, 127], shape[:-1] + (nb, 1)), axis=-1)
    e = rng.integers(lo, hi + 1, shape[:-1] + (nb, 1))
    x = (n * np.exp2(e.astype(np.float64))).astype(np.float16)
    return x.reshape(shape).view(np.uint16)


# ---- deep windows: the probe passes of tests/test_kv_q8_deep_gpu.py; tests/test_kv_q8_cpu.py checks on the host loop that their deep positions count ----

MISTRAL = (32, 8, 128)           # a group of 4 at head_dim 128, which attention_geometry_cases.GEOMETRIES does not hold
DEEP_K_SCALE = G.K_SCALE         # the key scale of the general rows: test_deep_probe_rows_depend_on_their_deep_positions holds at it, unshrunk
DEEP_SEQS = 3                    # sequences 0 and 1 take the rows of a pass in turn; sequence 2 is nobody's
DEEP_PROBE = {                   # name -> (geometry, window)
    "g4_d256_w6144": (G.GEOMETRIES["g4_d256"], 6144),
    "g2_d128_w8448": (G.GEOMETRIES["g2_d128"], 8448),
    "g4_d64_w8448": (G.GEOMETRIES["g4_d64"], 8448),
    "g4_d192_w4099": (G.GEOMETRIES["g4_d192"], 4099),   # an odd window
    "g1_d256_w4100": (G.GEOMETRIES["g1_d256"], 4100),
    "g2_d128_w32768": (G.GEOMETRIES["g2_d128"], 32768),
}
# windows of 260 positions for the instantiations no deep pass reaches: name -> (geometry, width)
SMALL_PROBE = {"g2_d256_6kv_rows171": (G.GEOMETRIES["g2_d256_6kv"], 171), "mistral_rows64": (MISTRAL, 64), "mistral_rows129": (MISTRAL, 129)}
SMALL_WINDOW = 260


@functools.lru_cache(maxsize=None)
def _general_pool(nkv, hd):
    """G.POOL general (lossy) rows, quantised: seeded normal rows times DEEP_K_SCALE / G.V_SCALE, rounded to f16, then quantize()"""
    rng = np.random.default_rng([37, nkv, hd])
    k = (rng.standard_normal((G.POOL, nkv, hd), dtype=np.float32) * np.float32(DEEP_K_SCALE)).astype(np.float16).view(np.uint16)
    v = (rng.standard_normal((G.POOL, nkv, hd), dtype=np.float32) * np.float32(G.V_SCALE)).astype(np.float16).view(np.uint16)
    return tuple(np.ascontiguousarray(a.transpose(1, 0, 2)) for a in quantize(k) + quantize(v))   # kq, kd, vq, vd as [n_kv_head][POOL][.]


def general_run(geometry, window, seq):
    """one sequence's (kq, kd, vq, vd), [n_kv_head][window][head_dim | head_dim / 32]: a run of the pool (a prime number of rows) from the
    sequence's own offset"""
    _, nkv, hd = geometry
    idx = (211 * seq + 17 + np.arange(window)) % G.POOL
    return tuple(a[:, idx] for a in _general_pool(nkv, hd))


def general_cache(geometry, window, nseq=DEEP_SEQS):
    """(kq, kd, vq, vd) of one layer and nseq sequences, [1][nseq][n_kv_head][window][.]"""
    runs = [general_run(geometry, window, s) for s in range(nseq)]
    return tuple(np.ascontiguousarray(np.stack([r[i] for r in runs])[None]) for i in range(4))


def deep_edge(window):
    """a position deep inside at which a 64-position slot and a 32-position slot both begin: slot 61 (122) or, in the wider windows, slot 90 (180)"""
    return 64 * (90 if window > 6000 else 61)


def probe_passes(name):
    """the passes of one DEEP_PROBE or SMALL_PROBE case: [(seq, pos)] int32 arrays; row r reads sequence r % 2.  Host cost of a row at position p:
    n_head * (p + 1) * head_dim * 2 fused multiply-adds (counted per case in tests/test_kv_q8_deep_gpu.py)"""
    if name in SMALL_PROBE:
        _, width = SMALL_PROBE[name]
        lengths = G.WINDOWS[SMALL_WINDOW]
        lists = [[lengths[(r + width) % len(lengths)] for r in range(width)]]
    else:
        _, W = DEEP_PROBE[name]
        E = deep_edge(W)
        if W == 32768:
            lists = [[W - 1, 31]]
        else:
            short = [G.LENGTHS[r % len(G.LENGTHS)] for r in range(256)]     # all below 300
            wide = list(short)
            wide[0], wide[85], wide[170], wide[255] = W - 1, E - 1, E, E + 1
            lists = [[W - 1], [E], [64],
                     [W - 1, E - 1, E, E + 1, 0, 1, 63, 64, 65], [W - 2, 65, 0, 1, 63, 64, 31, 32, 33],
                     wide]
    return [((np.arange(len(p)) % 2).astype(np.int32), np.array(p, np.int32)) for p in lists]


def probe_q(name, i, width, n_head, head_dim):
    """the queries of pass i of a case"""
    return np.random.default_rng([43, sum(map(ord, name)), i]).standard_normal((width, n_head, head_dim), dtype=np.float32)


def hd_class(head_dim):
    return head_dim if head_dim in (64, 128) else 0
