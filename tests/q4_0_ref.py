"""Q4_0 and Q5_0 blocks (GGML types 2 and 6, 18 / 22 B per 32 weights) in NumPy: the codecs, ggml's published quantisers, the Q8_0 twin
that pins both types to what tests/q8_0_ref.py pins, and the dot contract, which is Q8_0's.

  * Q4_0: f16 d, qs[16].  Weight j (0..15) = qs[j] & 15, weight j + 16 = qs[j] >> 4.  w = d (q - 8), q in 0..15.
  * Q5_0: f16 d, qh[4] (one little-endian u32), qs[16].  Weight j = (qs[j] & 15) | ((qh >> j) & 1) << 4, weight j + 16 =
    (qs[j] >> 4) | ((qh >> (j + 16)) & 1) << 4.  w = d (q - 16), q in 0..31.
    Both products are exact in binary32 (11 significant bits times at most 5).
  * quantise (quantize_row_q4_0_ref / quantize_row_q5_0_ref), all in binary32: max = the element of largest magnitude with its sign, the
    first one on ties; d = max / -z; id = d ? 1 / d : 0 from the unrounded d; d stored as f16; q = min(2 z - 1, (int8_t)(x id + z + 0.5)):
    one multiply, one add, truncation.
  * Q8_0 twin: the Q8_0 block with the same d bits and q8 = q - z decodes to the same bits, and the dot contract of the two types IS
    q8_0_ref.gemv on the twins: per 256-k run b and 32-block j ascending, acc = fmaf(d[b][j] d8[b], (float)P[b][j], acc) with
    P = sum_k (q_k - z) a_k, slabs added in ascending order.  -8..7 and -16..15 lie inside -32..31, so a twin-sparse run (one live block,
    seven with d = +0) is, through q8_0_ref.to_q6k, a Q6_K block the oracle runs."""
import numpy as np

import q8_0_ref as Q8

Q4_0, Q5_0 = 2, 6
BYTES = {Q4_0: 18, Q5_0: 22}
Z = {Q4_0: 8, Q5_0: 16}
QS_AT = {Q4_0: 2, Q5_0: 6}   # offset of the sixteen nibble bytes
CHUNK = 1 << 15


def _blocks(ttype, buf):
    return np.frombuffer(np.ascontiguousarray(buf).tobytes(), np.uint8).reshape(-1, BYTES[ttype])


def quants(ttype, blocks):
    """the stored q (n, 32): 0..15 / 0..31"""
    b = _blocks(ttype, blocks)
    qs = b[:, QS_AT[ttype]:QS_AT[ttype] + 16].astype(np.int64)
    q = np.concatenate([qs & 15, qs >> 4], axis=1)
    if ttype == Q5_0:
        qh = b[:, 2:6].copy().view("<u4")[:, 0].astype(np.int64)
        q |= ((qh[:, None] >> np.arange(32)[None, :]) & 1) << 4
    return q


def d_bits(ttype, blocks):
    return _blocks(ttype, blocks)[:, 0:2].copy().view(np.uint16)[:, 0]


def d_of(ttype, blocks):
    return d_bits(ttype, blocks).view(np.float16).astype(np.float32)


def dequant(ttype, blocks):
    """w = d (q - z) in binary32 (tk_q4_0_dequant / tk_q5_0_dequant's expression); (n, 32)"""
    b = _blocks(ttype, blocks)
    if b.shape[0] > 8 * CHUNK:
        return np.concatenate([dequant(ttype, b[i:i + 8 * CHUNK]) for i in range(0, b.shape[0], 8 * CHUNK)])
    with np.errstate(all="ignore"):
        return (d_of(ttype, b)[:, None] * (quants(ttype, b) - Z[ttype]).astype(np.float32)).astype(np.float32)


def make_blocks(ttype, q, d):
    """blocks (n, 18 | 22) from the stored q (n, 32) and d (n,): floats stored as f16, or uint16 f16 bit patterns taken as they are"""
    q = np.asarray(q).reshape(-1, 32).astype(np.int64)
    assert q.min() >= 0 and q.max() < 2 * Z[ttype]
    d = np.asarray(d).reshape(-1)
    b = np.zeros((q.shape[0], BYTES[ttype]), np.uint8)
    b[:, 0:2] = (d if d.dtype == np.uint16 else d.astype(np.float32).astype(np.float16)).view(np.uint8).reshape(-1, 2)
    b[:, QS_AT[ttype]:QS_AT[ttype] + 16] = ((q[:, :16] & 15) | ((q[:, 16:] & 15) << 4)).astype(np.uint8)
    if ttype == Q5_0:
        qh = (((q >> 4) & 1) << np.arange(32)[None, :]).sum(axis=1).astype("<u4")
        b[:, 2:6] = qh.view(np.uint8).reshape(-1, 4)
    return b


def quantize(ttype, x):
    """float weights (..., 32 n) -> blocks (n, 18 | 22): quantize_row_q4_0_ref / quantize_row_q5_0_ref in binary32, operation for
    operation"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 32)
    z = Z[ttype]
    n = x.shape[0]
    with np.errstate(all="ignore"):
        first = np.abs(x).argmax(axis=1)                                 # the first of equal magnitudes: `if (amax < fabsf(v))`
        mx = x[np.arange(n), first]
        d = (mx / np.float32(-z)).astype(np.float32)
        inv = np.where(d != 0, np.float32(1.0) / np.where(d != 0, d, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
        v = ((x * inv[:, None]).astype(np.float32) + np.float32(z + 0.5)).astype(np.float32)
    q = np.minimum(2 * z - 1, np.trunc(v.astype(np.float64)).astype(np.int64).astype(np.int8).astype(np.int64))
    return make_blocks(ttype, q, d)


def to_q8_0(ttype, blocks):
    """the Q8_0 twins (n, 34): the same d bits, q8 = q - z"""
    return Q8.make_blocks(quants(ttype, blocks) - Z[ttype], d_bits(ttype, blocks))


def gemv(ttype, blocks, rows, K, ks, q8, d8):
    """y [nrows][rows] of the dot contract: q8_0_ref.gemv on the Q8_0 twins"""
    return Q8.gemv(to_q8_0(ttype, blocks), rows, K, ks, q8, d8)


def quantize_twin_sparse(ttype, w, seed=0):
    """float weights (..., 256 n) -> twin-able blocks (8 n, 18 | 22): per 256-k run one live block at a position that walks with the run
    (all eight occur), quantised by the type's own quantiser, so q - z takes the type's whole range; the other seven blocks get d = +0 and
    random quants, which must not matter.  A test's own encoder: it only has to keep the model's weights sensible"""
    x = np.ascontiguousarray(w, np.float32).reshape(-1, 8, 32)
    n = x.shape[0]
    rng = np.random.default_rng(seed)
    live = (np.arange(n) * 3 + seed) % 8
    lb = quantize(ttype, x[np.arange(n), live])
    dead = (d_bits(ttype, lb) & 0x7FFF) == 0                                        # an all-zero live block still gets a live (non-zero) d
    lb[dead, 0:2] = np.array([0x0400], np.uint16).view(np.uint8)
    b = rng.integers(0, 256, (n, 8, BYTES[ttype]), dtype=np.uint8)
    b[:, :, 0:2] = 0
    b[np.arange(n), live] = lb
    return b.reshape(-1, BYTES[ttype])


def to_q6k(ttype, blocks):
    """twin-able runs -> the Q6_K blocks the oracle runs, through the Q8_0 twins"""
    return Q8.to_q6k(to_q8_0(ttype, blocks))
