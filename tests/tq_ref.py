"""TQ1_0 and TQ2_0 blocks (GGML types 34 and 35, the ternary types) in NumPy, written from the published format description: the codecs,
ggml's one-pass reference quantisers, the dot contract restated, and the twins that pin both types to what the project already trusts.

  * TQ2_0: 66 B per 256 weights, qs[64], f16 d LAST.  Weight 128 h + 32 l + m (h 0..1, l 0..3, m 0..31) has the code
    c = (qs[32 h + m] >> 2 l) & 3 and the value (float)(c - 1) d.  The quantiser writes 0..2; code 3 is a valid byte and is +2 d.
  * TQ1_0: 54 B per 256 weights, qs[48], qh[4], f16 d LAST.  Trit n of byte b is t = ((uint16)(uint8)(b 3^n) * 3) >> 8, in 0..2 for every
    one of the 256 byte values; weights 0..159 at 32 n + m = trit n (0..4) of qs[m], m 0..31; 160..239 at 160 + 16 n + m = trit n (0..4) of
    qs[32 + m], m 0..15; 240..255 at 240 + 4 n + j = trit n (0..3) of qh[j]; the fifth trit of a qh byte is unused.  Value (float)(t - 1) d.
  Below "code" means c for TQ2_0 and t for TQ1_0: the weight is (code - 1) d for both.
  * quantise (quantize_row_tq2_0_ref / quantize_row_tq1_0_ref), all in binary32: amax = max |x| over the 256 values, d = amax stored as
    f16, id = amax ? 1 / amax : 0 from the f32 amax, xi = lroundf(x id) + 1 (halves away from zero; x id clamped to +-1 and NaN
    taken as -1, which only matters where an amax below 2^-128 makes id infinite).  TQ2_0: qs[32 h + m] |= xi << 2 l.
    TQ1_0: per byte q = 0, for n ascending q = 3 q + xi_n (a qh byte takes four trits and one more q *= 3), byte = (256 q + 242) / 243.
  * gemv, the contract: per weight row and K-split slab, over the 256-k runs b ascending from +0,
        acc = fmaf(d[b] d8[b], (float)S[b], acc),    S[b] = sum_k (code_k - 1) a_k  (exact, |S| <= 256 * 2 * 127 < 2^23),
    the product d d8 rounded once to binary32; slabs added in ascending order.  This is ggml_vec_dot_tq*_q8_K per run.
  * Q6_K twin: EVERY block of either type is the Q6_K block with the same d, all sixteen scales 1 and q6 = 32 + (code - 1): the same
    integer, the same float expression (dot_q6k_range computes fmaf(d_w d8, (float)P, acc)), the same dequantised bits."""
import numpy as np

from q5k_ref import fmaf

TQ1_0, TQ2_0 = 34, 35
BYTES = {TQ1_0: 54, TQ2_0: 66}
D_AT = {TQ1_0: 52, TQ2_0: 64}   # d is the block's last field
Q6K_BYTES = 210
POW3 = (1, 3, 9, 27, 81)
CHUNK = 1 << 14  # blocks per pass of the bulk functions below: whole Mistral-7B matrices go through them


def _blocks(ttype, buf):
    return np.frombuffer(np.ascontiguousarray(buf).tobytes(), np.uint8).reshape(-1, BYTES[ttype])


def trits(byte):
    """the five trits of TQ1_0 bytes (..., 5): ((uint16)(uint8)(b 3^n) * 3) >> 8"""
    b = np.asarray(byte).astype(np.int64)[..., None]
    return ((((b * np.array(POW3, np.int64)) & 0xFF) * 3) >> 8)


def codes(ttype, blocks):
    """(n, 256) int in 0..3 (TQ2_0) / 0..2 (TQ1_0): the weight is (code - 1) d"""
    b = _blocks(ttype, blocks).astype(np.int64)
    q = np.zeros((b.shape[0], 256), np.int64)
    if ttype == TQ2_0:
        for h in range(2):
            for l in range(4):
                q[:, 128 * h + 32 * l:128 * h + 32 * l + 32] = (b[:, 32 * h:32 * h + 32] >> (2 * l)) & 3
        return q
    t = trits(b[:, 0:52])                                                # (n, 52, 5)
    for n in range(5):
        q[:, 32 * n:32 * n + 32] = t[:, 0:32, n]
        q[:, 160 + 16 * n:160 + 16 * n + 16] = t[:, 32:48, n]
    for n in range(4):
        q[:, 240 + 4 * n:240 + 4 * n + 4] = t[:, 48:52, n]
    return q


def d_bits(ttype, blocks):
    return _blocks(ttype, blocks)[:, D_AT[ttype]:D_AT[ttype] + 2].copy().view(np.uint16)[:, 0]


def d_of(ttype, blocks):
    return d_bits(ttype, blocks).view(np.float16).astype(np.float32)


def dequant(ttype, blocks):
    """w = (float)(code - 1) d in binary32 (exact); (n, 256)"""
    b = _blocks(ttype, blocks)
    if b.shape[0] > CHUNK:
        return np.concatenate([dequant(ttype, b[i:i + CHUNK]) for i in range(0, b.shape[0], CHUNK)])
    with np.errstate(all="ignore"):
        return ((codes(ttype, b) - 1).astype(np.float32) * d_of(ttype, b)[:, None]).astype(np.float32)


def _d_bytes(d):
    d = np.asarray(d).reshape(-1)
    with np.errstate(all="ignore"):
        return (d if d.dtype == np.uint16 else d.astype(np.float32).astype(np.float16)).view(np.uint8).reshape(-1, 2)


def pack_tq1(q):
    """canonical TQ1_0 bytes (n, 52) of trits q (n, 256) in 0..2"""
    q = np.asarray(q, np.int64).reshape(-1, 256)
    assert q.min() >= 0 and q.max() <= 2
    v = np.zeros((q.shape[0], 52), np.int64)
    for n in range(5):
        v[:, 0:32] = 3 * v[:, 0:32] + q[:, 32 * n:32 * n + 32]
        v[:, 32:48] = 3 * v[:, 32:48] + q[:, 160 + 16 * n:160 + 16 * n + 16]
    for n in range(4):
        v[:, 48:52] = 3 * v[:, 48:52] + q[:, 240 + 4 * n:240 + 4 * n + 4]
    v[:, 48:52] *= 3
    return ((v * 256 + 242) // 243).astype(np.uint8)


def make_blocks(ttype, trits_or_codes, d):
    """blocks (n, 54 | 66) from the codes (n, 256) — 0..3 for TQ2_0, trits 0..2 for TQ1_0, which get their canonical bytes — and d per block
    (floats stored as f16, or uint16 bit patterns taken as they are)"""
    q = np.asarray(trits_or_codes, np.int64).reshape(-1, 256)
    b = np.zeros((q.shape[0], BYTES[ttype]), np.uint8)
    if ttype == TQ2_0:
        assert q.min() >= 0 and q.max() <= 3
        for h in range(2):
            for l in range(4):
                b[:, 32 * h:32 * h + 32] |= (q[:, 128 * h + 32 * l:128 * h + 32 * l + 32] << (2 * l)).astype(np.uint8)
    else:
        b[:, 0:52] = pack_tq1(q)
    b[:, D_AT[ttype]:D_AT[ttype] + 2] = _d_bytes(d)
    return b


def quantize(ttype, x):
    """float weights (..., 256 n) -> blocks: ggml's reference quantisers in binary32, operation for operation"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 256)
    if x.shape[0] > CHUNK:
        return np.concatenate([quantize(ttype, x[i:i + CHUNK]) for i in range(0, x.shape[0], CHUNK)])
    with np.errstate(all="ignore"):
        amax = np.abs(x).max(axis=1).astype(np.float32)
        iid = np.where(amax != 0, np.float32(1.0) / np.where(amax != 0, amax, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
        v = (x * iid[:, None]).astype(np.float32)
        v = np.where(v >= -1, v, np.float32(-1.0))       # an amax below 2^-128: id is inf, v +-inf or NaN; NaN counts as -1, +-inf as +-1
        v = np.where(v <= 1, v, np.float32(1.0)).astype(np.float32)
        xi = (np.sign(v) * np.floor(np.abs(v).astype(np.float64) + 0.5)).astype(np.int64) + 1    # lroundf: halves away from zero
        return make_blocks(ttype, xi, amax)


def to_q6k(ttype, blocks):
    """any block -> its Q6_K twin (n x 210 bytes, flat): d verbatim, all sixteen scales 1, q6 = 32 + (code - 1) in Q6_K's packing
    (weight 128 n + 32 c + l: low nibble in ql[64 n + 32 (c & 1) + l] (high half of the byte for c >= 2), bits 2c, 2c + 1 of qh[32 n + l])"""
    b = _blocks(ttype, blocks)
    if b.shape[0] > CHUNK:
        return np.concatenate([to_q6k(ttype, b[i:i + CHUNK]) for i in range(0, b.shape[0], CHUNK)])
    q6 = (codes(ttype, b) + 31).astype(np.uint8)
    out = np.zeros((q6.shape[0], Q6K_BYTES), np.uint8)
    for n in range(2):
        for c in range(4):
            v = q6[:, 128 * n + 32 * c:128 * n + 32 * c + 32]
            lo = slice(64 * n + 32 * (c & 1), 64 * n + 32 * (c & 1) + 32)
            out[:, lo] |= (v & 15) << (4 * (c >> 1))
            out[:, 128 + 32 * n:128 + 32 * n + 32] |= (v >> 4) << (2 * c)
    out[:, 192:208] = 1
    out[:, 208:210] = b[:, D_AT[ttype]:D_AT[ttype] + 2]
    return out.reshape(-1)


def tq1_to_tq2(blocks):
    """TQ1_0 blocks -> the TQ2_0 blocks with the same weights: the trits as codes, d verbatim"""
    return make_blocks(TQ2_0, codes(TQ1_0, blocks), d_bits(TQ1_0, blocks))


def gemv(ttype, blocks, rows, K, ks, q8, d8):
    """y [nrows][rows] of the dot contract.  q8 [nrows][K] int8 and d8 [nrows][K / 256] as oracle_lib.q8k_quantize gives them per row.
    (The integer sums run as binary64 matrix products: every partial sum is an integer below 2^53, so they are exact.)"""
    nb = K // 256
    t = (codes(ttype, blocks) - 1).astype(np.float64)
    assert t.shape[0] == rows * nb
    t = t.reshape(rows, nb, 256)
    d = d_of(ttype, blocks).reshape(rows, nb)
    nrows = q8.shape[0]
    a = q8.astype(np.float64).reshape(nrows, nb, 256)
    y = None
    per = nb // ks
    with np.errstate(all="ignore"):
        for s in range(ks):
            acc = np.zeros((nrows, rows), np.float32)
            for blk in range(s * per, (s + 1) * per):
                S = a[:, blk, :] @ t[:, blk, :].T
                dd = d8[:, blk, None].astype(np.float32)
                acc = fmaf((d[None, :, blk] * dd).astype(np.float32), S.astype(np.float32), acc)
            y = acc if y is None else (y + acc).astype(np.float32)
    return y
