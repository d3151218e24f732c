"""The Q8_0 KV cache's quantiser (csrc/common/tk_kv_q8.h) restated in float32 NumPy, for tests/test_kv_q8_cpu.py and tests/test_kv_q8_gpu.py.

A cached row is the f16-rounded key or value widened to fp32; per block of 32, ggml's quantize_row_q8_0_ref value for value:
    amax = max |x|;  d = amax / 127;  id = d ? 1 / d : 0;  q[i] = roundf(x[i] * id);  stored scale = f16(d)
roundf rounds halves away from zero.  Every step is one correctly rounded float32 operation, which NumPy's float32 arithmetic is too.  The value of
an element is f16_to_f32(scale) * q, exact in fp32.

lossless_rows() makes rows that the quantiser keeps exactly: per block x = n * 2^e with integer |n| <= 127, one |n| = 127, e in -10 .. -4; then
amax = 127 * 2^e, d = 2^e, id = 2^-e, q = n and d * q = x."""
import numpy as np

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


def lossless_rows(shape, seed):
    """f16 bits of rows the quantiser keeps exactly; shape[-1] % 32 == 0"""
    rng = np.random.default_rng([91, seed])
    nb = shape[-1] // BLOCK
    n = rng.integers(-127, 128, shape[:-1] + (nb, BLOCK))
    at = rng.integers(0, BLOCK, shape[:-1] + (nb,))
    np.put_along_axis(n, at[..., None], rng.choice([-127, 127], shape[:-1] + (nb, 1)), axis=-1)
    e = rng.integers(-10, -3, shape[:-1] + (nb, 1))
    x = (n * np.exp2(e.astype(np.float64))).astype(np.float16)
    return x.reshape(shape).view(np.uint16)
