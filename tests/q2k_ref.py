"""Q2_K blocks (GGML type 10, 84 B per 256 weights: scales[16] with the scale in the low and the min in the high nibble, qs[64], f16 d,
f16 dmin) in NumPy: the decode the HIP path implements, the two exact twins that pin it to the oracle, and the dot contract restated.

  * Q4_K twin: a block whose groups 2 j and 2 j + 1 share (sc, m) is the Q4_K block with the same d and dmin, 6-bit pair j = (sc, m) and
    q4 = q: the same integers P and M, the same float expression, the same dequantised bits.
  * Q6_K twin: a block with dmin = +0 is the Q6_K block with the same d, scales[g] = sc_g and q6 = q + 32.
  * gemv: per block and slab acc = fmaf(d d8, P, acc); acc = fmaf(-(dmin d8), M, acc) with P = sum_g sc_g sum_{k in g} q_k a_k and
    M = sum_g m_g sum_{k in g} a_k, blocks and slabs in ascending order."""
import numpy as np

from q5k_ref import fmaf

Q2K_BYTES, Q4K_BYTES, Q6K_BYTES = 84, 144, 210


def _blocks(buf):
    return np.frombuffer(np.ascontiguousarray(buf).tobytes(), np.uint8).reshape(-1, Q2K_BYTES)


def quants(blocks):
    """q (n, 256) int in 0..3: weight 128 n + 32 j + l = (qs[32 n + l] >> 2 j) & 3"""
    qs = _blocks(blocks)[:, 16:80].astype(np.int64)
    q = np.zeros((qs.shape[0], 256), np.int64)
    for n in range(2):
        for j in range(4):
            q[:, 128 * n + 32 * j:128 * n + 32 * j + 32] = (qs[:, 32 * n:32 * n + 32] >> (2 * j)) & 3
    return q


def scales(blocks):
    """sc (n, 16) int in 0..15: the low nibble of scales[g]"""
    return _blocks(blocks)[:, 0:16].astype(np.int64) & 15


def mins(blocks):
    """m (n, 16) int in 0..15: the high nibble of scales[g]"""
    return _blocks(blocks)[:, 0:16].astype(np.int64) >> 4


def d_of(blocks):
    return _blocks(blocks)[:, 80:82].copy().view(np.float16).astype(np.float32)[:, 0]


def dmin_of(blocks):
    return _blocks(blocks)[:, 82:84].copy().view(np.float16).astype(np.float32)[:, 0]


CHUNK = 1 << 14  # blocks per pass of the bulk functions below: whole Mistral-7B matrices go through them


def dequant(blocks):
    """w = (d sc_g) q - dmin m_g in binary32, one rounding per operation (tk_q2k_dequant's expression); (n, 256)"""
    b = _blocks(blocks)
    if b.shape[0] > CHUNK:
        return np.concatenate([dequant(b[i:i + CHUNK]) for i in range(0, b.shape[0], CHUNK)])
    with np.errstate(all="ignore"):
        ds = (d_of(b)[:, None] * scales(b).astype(np.float32)).astype(np.float32)     # (n, 16)
        mm = (dmin_of(b)[:, None] * mins(b).astype(np.float32)).astype(np.float32)
        a = (np.repeat(ds, 16, axis=1) * quants(b).astype(np.float32)).astype(np.float32)
        return (a - np.repeat(mm, 16, axis=1)).astype(np.float32)


def make_blocks(q, sc, m, d, dmin):
    """Q2_K blocks (n, 84) from q (n, 256) in 0..3, sc and m (n, 16) in 0..15, d and dmin (n,) floats stored as f16: the encoder of the
    layout above"""
    q, sc, m = np.asarray(q, np.int64).reshape(-1, 256), np.asarray(sc, np.int64).reshape(-1, 16), np.asarray(m, np.int64).reshape(-1, 16)
    b = np.zeros((q.shape[0], Q2K_BYTES), np.uint8)
    b[:, 0:16] = (sc | (m << 4)).astype(np.uint8)
    for n in range(2):
        for j in range(4):
            b[:, 16 + 32 * n:16 + 32 * n + 32] |= (q[:, 128 * n + 32 * j:128 * n + 32 * j + 32] << (2 * j)).astype(np.uint8)
    b[:, 80:82] = np.asarray(d, np.float32).reshape(-1).astype(np.float16).view(np.uint8).reshape(-1, 2)
    b[:, 82:84] = np.asarray(dmin, np.float32).reshape(-1).astype(np.float16).view(np.uint8).reshape(-1, 2)
    return b


def make_block(q, sc, m, d, dmin):
    return make_blocks(np.asarray(q)[None], np.asarray(sc)[None], np.asarray(m)[None], [d], [dmin])[0]


def pair_groups(blocks):
    """the blocks with (sc, m) of group 2 j copied to group 2 j + 1: Q4_K-twin-able"""
    b = _blocks(blocks).copy()
    b[:, 1:16:2] = b[:, 0:16:2]
    return b


def quantize_paired(w):
    """float weights (..., 256 n) -> Q2_K blocks (n, 84) with paired groups: per 32-wide sub-block a non-negative min and a scale, both
    4-bit fractions of dmin and d.  A test's own encoder — any valid block would do; it only has to keep the model's weights sensible"""
    x = np.asarray(w, np.float32).reshape(-1, 8, 32)
    if x.shape[0] > CHUNK:
        return np.concatenate([quantize_paired(x[i:i + CHUNK]) for i in range(0, x.shape[0], CHUNK)])
    x = x.astype(np.float64)
    mn = np.minimum(x.min(axis=2), 0.0)
    scale = (x.max(axis=2) - mn) / 3.0
    d = (scale.max(axis=1) / 15.0).astype(np.float16).astype(np.float64)
    dmin = ((-mn).max(axis=1) / 15.0).astype(np.float16).astype(np.float64)
    with np.errstate(all="ignore"):
        sc = np.where(d[:, None] > 0, np.rint(scale / d[:, None]), 0.0).clip(0, 15)
        m = np.where(dmin[:, None] > 0, np.rint(-mn / dmin[:, None]), 0.0).clip(0, 15)
        dl, ml = d[:, None] * sc, dmin[:, None] * m
        q = np.where(dl[:, :, None] > 0, np.rint((x + ml[:, :, None]) / dl[:, :, None]), 0.0).clip(0, 3)
    return make_blocks(q.reshape(-1, 256), np.repeat(sc, 2, axis=1), np.repeat(m, 2, axis=1), d, dmin)


def is_paired(blocks):
    b = _blocks(blocks)
    return (b[:, 1:16:2] == b[:, 0:16:2]).all(axis=1)


def to_q4k(blocks):
    """paired-group Q2_K blocks -> their Q4_K twins (n x 144 bytes, flat): d, dmin verbatim, 6-bit pair j = (sc_2j, m_2j) in Q4_K's
    packing (the high two bits of every pair are 0), q4 = q in the low / high nibbles of qs[32 (j / 2) + l]"""
    b = _blocks(blocks)
    assert is_paired(b).all()
    if b.shape[0] > CHUNK:
        return np.concatenate([to_q4k(b[i:i + CHUNK]) for i in range(0, b.shape[0], CHUNK)])
    sc, m = scales(b)[:, 0::2], mins(b)[:, 0::2]
    out = np.zeros((b.shape[0], Q4K_BYTES), np.uint8)
    out[:, 0:4] = b[:, 80:84]
    out[:, 4:8] = sc[:, 0:4]
    out[:, 8:12] = m[:, 0:4]
    out[:, 12:16] = sc[:, 4:8] | (m[:, 4:8] << 4)
    for n in range(2):       # sub-blocks 4 n + 2 e and 4 n + 2 e + 1 share the Q4_K bytes qs[32 (2 n + e) + l]: bit pairs 2 e, 2 e + 1 of a Q2_K byte
        qs = b[:, 16 + 32 * n:16 + 32 * n + 32]
        for e in range(2):
            out[:, 16 + 32 * (2 * n + e):16 + 32 * (2 * n + e) + 32] = ((qs >> (4 * e)) & 3) | (((qs >> (4 * e + 2)) & 3) << 4)
    return out.reshape(-1)


def to_q6k(blocks):
    """Q2_K blocks with dmin = +0 -> their Q6_K twins (n x 210 bytes, flat): d verbatim, scales[g] = sc_g, q6 = q + 32 in Q6_K's packing
    (weight 128 n + 32 c + l: low nibble in ql[64 n + 32 (c & 1) + l] (high half of the byte for c >= 2), bits 2c, 2c + 1 of qh[32 n + l])"""
    b = _blocks(blocks)
    assert not b[:, 82:84].any()
    if b.shape[0] > CHUNK:
        return np.concatenate([to_q6k(b[i:i + CHUNK]) for i in range(0, b.shape[0], CHUNK)])
    q6 = (quants(b) + 32).astype(np.uint8)
    out = np.zeros((b.shape[0], Q6K_BYTES), np.uint8)
    for n in range(2):
        for c in range(4):
            v = q6[:, 128 * n + 32 * c:128 * n + 32 * c + 32]
            lo = slice(64 * n + 32 * (c & 1), 64 * n + 32 * (c & 1) + 32)
            out[:, lo] |= (v & 15) << (4 * (c >> 1))
            out[:, 128 + 32 * n:128 + 32 * n + 32] |= (v >> 4) << (2 * c)
    out[:, 192:208] = scales(b).astype(np.uint8)
    out[:, 208:210] = b[:, 80:82]
    return out.reshape(-1)


def gemv(blocks, rows, K, ks, q8, d8):
    """y [nrows][rows] of the Q2_K dot contract.  q8 [nrows][K] int8 and d8 [nrows][K / 256] as oracle_lib.q8k_quantize gives them per
    row; the 16-wide sums of M are taken from q8 itself.  (The integer sums run as binary64 matrix products: every partial sum is an
    integer below 2^53, so they are exact.)"""
    nb = K // 256
    flat = _blocks(blocks)
    assert flat.shape[0] == rows * nb
    sq = (quants(flat).reshape(-1, 16, 16) * scales(flat)[:, :, None]).reshape(rows, nb, 256).astype(np.float64)   # sc_g q_k
    mk = np.repeat(mins(flat), 16, axis=1).reshape(rows, nb, 256).astype(np.float64)                              # m_g(k)
    d, dmin = d_of(flat).reshape(rows, nb), dmin_of(flat).reshape(rows, nb)
    nrows = q8.shape[0]
    a = q8.astype(np.float64).reshape(nrows, nb, 256)
    y = None
    per = nb // ks
    for s in range(ks):
        acc = np.zeros((nrows, rows), np.float32)
        for blk in range(s * per, (s + 1) * per):
            P = a[:, blk, :] @ sq[:, blk, :].T
            M = a[:, blk, :] @ mk[:, blk, :].T
            dd = d8[:, blk, None].astype(np.float32)
            acc = fmaf(d[None, :, blk] * dd, P.astype(np.float32), acc)
            acc = fmaf(-(dmin[None, :, blk] * dd), M.astype(np.float32), acc)
        y = acc if y is None else (y + acc).astype(np.float32)
    return y
