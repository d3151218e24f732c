"""Q4_1 and Q5_1 blocks (GGML types 3 and 7, 20 / 24 B per 32 weights) in NumPy: the codecs, ggml's published quantisers, the dot contract
with its min term, and the twins that pin it to what the project already trusts.

  * Q4_1: f16 d, f16 m, qs[16].  Weight j (0..15) = qs[j] & 15, weight j + 16 = qs[j] >> 4.  w = d q + m, q in 0..15.
  * Q5_1: f16 d, f16 m, qh[4] (one little-endian u32), qs[16].  Weight j = (qs[j] & 15) | ((qh >> j) & 1) << 4, weight j + 16 =
    (qs[j] >> 4) | ((qh >> (j + 16)) & 1) << 4.  w = d q + m, q in 0..31.
    d q is exact in binary32 (11 significant bits times at most 5) and the add rounds once: the decode is fmaf(d, (float)q, m).
  * quantise (quantize_row_q4_1_ref / quantize_row_q5_1_ref), all in binary32, L = 15 / 31: min and max the block's smallest and largest
    element; d = (max - min) / L; id = d ? 1 / d : 0 from the unrounded d; d and m = min stored as f16;
    q = min(15, (int8_t)((x - min) id + 0.5f)) for Q4_1, (uint8_t)((x - min) id + 0.5f) for Q5_1 (no clamp: the sum stays below 32).
  * the dot contract, per weight row and K-split slab, runs b of 256 k ascending and within a run the eight 32-blocks j ascending:
        acc = fmaf(fl(d[b][j] d8[b]), (float)P[b][j], acc)      P = sum_k q_k a_k
        acc = fmaf(fl(m[b][j] d8[b]), (float)S[b][j], acc)      S = sum_k a_k
    on the Q8_K activation image (a, d8, and the per-32 sums S the image carries); slabs added in ascending order.
  * twins: a run with one live block (the other seven d = +0 and m = +0) is the Q4_K block with d, dmin = -m (an exact f16 negation),
    sc = mn = 1 on the live sub-block and 0 elsewhere (to_q4k; q <= 15) or the Q5_K block of the same construction (to_q5k); a block
    with m = +-0 is the Q8_0 block with the same d and q8 = q (to_q8_0)."""
import numpy as np

import q5k_ref as Q5K
import q8_0_ref as Q8

Q4_1, Q5_1 = 3, 7
BYTES = {Q4_1: 20, Q5_1: 24}
L = {Q4_1: 15, Q5_1: 31}
QS_AT = {Q4_1: 4, Q5_1: 8}   # offset of the sixteen nibble bytes
fmaf = Q5K.fmaf


def _blocks(ttype, buf):
    return np.frombuffer(np.ascontiguousarray(buf).tobytes(), np.uint8).reshape(-1, BYTES[ttype])


def quants(ttype, blocks):
    """the stored q (n, 32): 0..15 / 0..31"""
    b = _blocks(ttype, blocks)
    qs = b[:, QS_AT[ttype]:QS_AT[ttype] + 16].astype(np.int64)
    q = np.concatenate([qs & 15, qs >> 4], axis=1)
    if ttype == Q5_1:
        qh = b[:, 4:8].copy().view("<u4")[:, 0].astype(np.int64)
        q |= ((qh[:, None] >> np.arange(32)[None, :]) & 1) << 4
    return q


def d_bits(ttype, blocks):
    return _blocks(ttype, blocks)[:, 0:2].copy().view(np.uint16)[:, 0]


def m_bits(ttype, blocks):
    return _blocks(ttype, blocks)[:, 2:4].copy().view(np.uint16)[:, 0]


def d_of(ttype, blocks):
    return d_bits(ttype, blocks).view(np.float16).astype(np.float32)


def m_of(ttype, blocks):
    return m_bits(ttype, blocks).view(np.float16).astype(np.float32)


def dequant(ttype, blocks):
    """w = fmaf(d, q, m) in binary32 (tk_q4_1_dequant / tk_q5_1_dequant's expression); (n, 32)"""
    b = _blocks(ttype, blocks)
    q = quants(ttype, b).astype(np.float32)
    with np.errstate(all="ignore"):
        return fmaf(np.broadcast_to(d_of(ttype, b)[:, None], q.shape), q, np.broadcast_to(m_of(ttype, b)[:, None], q.shape))


def make_blocks(ttype, q, d, m):
    """blocks (n, 20 | 24) from the stored q (n, 32), d (n,) and m (n,): floats stored as f16, or uint16 f16 bit patterns taken as they are"""
    q = np.asarray(q).reshape(-1, 32).astype(np.int64)
    assert q.min() >= 0 and q.max() <= L[ttype]
    b = np.zeros((q.shape[0], BYTES[ttype]), np.uint8)
    for at, v in ((0, d), (2, m)):
        v = np.asarray(v).reshape(-1)
        b[:, at:at + 2] = (v if v.dtype == np.uint16 else v.astype(np.float32).astype(np.float16)).view(np.uint8).reshape(-1, 2)
    b[:, QS_AT[ttype]:QS_AT[ttype] + 16] = ((q[:, :16] & 15) | ((q[:, 16:] & 15) << 4)).astype(np.uint8)
    if ttype == Q5_1:
        qh = (((q >> 4) & 1) << np.arange(32)[None, :]).sum(axis=1).astype("<u4")
        b[:, 4:8] = qh.view(np.uint8).reshape(-1, 4)
    return b


def quantize_values(ttype, x):
    """the float (x - min) id + 0.5f of every element, before truncation: (n, 32) float32, and d, min"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 32)
    with np.errstate(all="ignore"):
        mn, mx = x.min(axis=1), x.max(axis=1)
        d = ((mx - mn).astype(np.float32) / np.float32(L[ttype])).astype(np.float32)
        inv = np.where(d != 0, np.float32(1.0) / np.where(d != 0, d, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
        v = (((x - mn[:, None]).astype(np.float32) * inv[:, None]).astype(np.float32) + np.float32(0.5)).astype(np.float32)
    return v, d, mn


def quantize(ttype, x):
    """float weights (..., 32 n) -> blocks (n, 20 | 24): quantize_row_q4_1_ref / quantize_row_q5_1_ref in binary32, operation for operation"""
    v, d, mn = quantize_values(ttype, x)
    t = np.trunc(v.astype(np.float64)).astype(np.int64)
    if ttype == Q4_1:
        q = np.minimum(15, t.astype(np.int8).astype(np.int64))
    else:
        q = t.astype(np.uint8).astype(np.int64)
        assert q.max() <= 31
    return make_blocks(ttype, q, d, mn)


def gemv(ttype, blocks, rows, K, ks, q8, d8, bsum):
    """y [nrows][rows] of the dot contract.  q8 [nrows][K] int8, d8 [nrows][K / 256] and bsum [nrows][K / 32] as oracle_lib.q8k_quantize
    gives them per row.  (The integer sums run as binary64 matrix products: every partial sum is an integer below 2^53, so exact.)"""
    nb = K // 256
    flat = _blocks(ttype, blocks)
    assert flat.shape[0] == rows * nb * 8
    q = quants(ttype, flat).reshape(rows, nb, 8, 32).astype(np.float64)
    d = d_of(ttype, flat).reshape(rows, nb, 8)
    m = m_of(ttype, flat).reshape(rows, nb, 8)
    nrows = q8.shape[0]
    a = q8.astype(np.float64).reshape(nrows, nb, 8, 32)
    S = np.asarray(bsum).astype(np.int64).reshape(nrows, nb, 8)
    assert np.array_equal(S, q8.astype(np.int64).reshape(nrows, nb, 8, 32).sum(axis=3))      # the image's sums are the sums of its int8
    y = None
    per = nb // ks
    with np.errstate(all="ignore"):
        for s in range(ks):
            acc = np.zeros((nrows, rows), np.float32)
            for blk in range(s * per, (s + 1) * per):
                dd = d8[:, blk, None].astype(np.float32)
                for j in range(8):
                    P = a[:, blk, j, :] @ q[:, blk, j, :].T
                    acc = fmaf((d[None, :, blk, j] * dd).astype(np.float32), P.astype(np.float32), acc)
                    Sj = np.broadcast_to(S[:, blk, j, None].astype(np.float32), acc.shape)
                    acc = fmaf((m[None, :, blk, j] * dd).astype(np.float32), Sj, acc)
            y = acc if y is None else (y + acc).astype(np.float32)
    return y


def live_of(ttype, blocks):
    """per 256-k run (eight blocks) of twin-able blocks: the index of the one block whose d or m is not +0 (0 when all eight are)"""
    b = _blocks(ttype, blocks)
    on = ((d_bits(ttype, b) != 0) | (m_bits(ttype, b) != 0)).reshape(-1, 8)
    assert (on.sum(axis=1) <= 1).all()
    return on.argmax(axis=1)


def _twin_parts(ttype, blocks):
    b = _blocks(ttype, blocks)
    live = live_of(ttype, b)
    runs = b.reshape(-1, 8, BYTES[ttype])
    n = runs.shape[0]
    pick = runs[np.arange(n), live]
    head = np.zeros((n, 16), np.uint8)
    head[:, 0:2] = pick[:, 0:2]
    head[:, 2:4] = (m_bits(ttype, pick) ^ np.uint16(0x8000)).view(np.uint8).reshape(-1, 2)     # dmin = -m
    on = ((pick[:, 0:4] != 0).any(axis=1)).astype(np.uint8)
    # 6-bit (scale, min) pairs: j < 4 in bytes j and j + 4; j >= 4 in the two nibbles of byte j + 4 (the high two bits are zero for 1)
    sc = head[:, 4:16]
    lo = live < 4
    sc[np.arange(n)[lo], live[lo]] = on[lo]
    sc[np.arange(n)[lo], live[lo] + 4] = on[lo]
    sc[np.arange(n)[~lo], live[~lo] + 4] = on[~lo] * 0x11
    ql = quants(ttype, pick)                                             # (n, 32)
    return n, live, head, ql


def _pack_nibbles(n, live, ql):
    """the 128 qs bytes of a Q4_K / Q5_K block: sub-block j = the low (even j) or high (odd j) nibbles of qs[32 (j / 2) .. + 31]"""
    qs = np.zeros((n, 128), np.uint8)
    cols = 32 * (live // 2)[:, None] + np.arange(32)[None, :]
    qs[np.arange(n)[:, None], cols] = ((ql & 15) << (4 * (live % 2))[:, None]).astype(np.uint8)
    return qs


def to_q4k(ttype, blocks):
    """twin-able runs whose live q are <= 15 -> the Q4_K blocks (n / 8 x 144 bytes, flat) the oracle runs"""
    n, live, head, ql = _twin_parts(ttype, blocks)
    assert ql.max() <= 15
    return np.concatenate([head, _pack_nibbles(n, live, ql)], axis=1).reshape(-1)


def to_q5k(ttype, blocks):
    """twin-able runs -> their Q5_K twins (n / 8 x 176 bytes, flat): bit j of qh[l] = bit 4 of weight l of the live sub-block j"""
    n, live, head, ql = _twin_parts(ttype, blocks)
    qh = (((ql >> 4) & 1) << live[:, None]).astype(np.uint8)
    return np.concatenate([head, qh, _pack_nibbles(n, live, ql)], axis=1).reshape(-1)


def to_q8_0(ttype, blocks):
    """blocks with m = +-0 -> the Q8_0 twins (n, 34): the same d bits, q8 = q"""
    assert ((m_bits(ttype, blocks) & 0x7FFF) == 0).all()
    return Q8.make_blocks(quants(ttype, blocks), d_bits(ttype, blocks))


def quantize_twin_sparse(ttype, w, seed=0, q4_only=False):
    """float weights (..., 256 n) -> twin-able blocks (8 n, 20 | 24): per 256-k run one live block at a position that walks with the run
    (all eight occur), quantised by the type's own quantiser; the other seven blocks get d = +0, m = +0 and random quants, which must not
    matter.  q4_only (Q5_1): the live blocks are quantised to 0..15 (Q4_1's step) and qh = 0, so the runs have Q4_K twins.  A test's
    own encoder: it only has to keep the model's weights sensible"""
    x = np.ascontiguousarray(w, np.float32).reshape(-1, 8, 32)
    n = x.shape[0]
    rng = np.random.default_rng(seed)
    live = (np.arange(n) * 3 + seed) % 8
    xl = x[np.arange(n), live]
    if q4_only and ttype == Q5_1:
        b4 = quantize(Q4_1, xl)
        lb = make_blocks(Q5_1, quants(Q4_1, b4), d_bits(Q4_1, b4), m_bits(Q4_1, b4))
    else:
        lb = quantize(ttype, xl)
    dead = ((d_bits(ttype, lb) & 0x7FFF) == 0) & ((m_bits(ttype, lb) & 0x7FFF) == 0)     # an all-zero live block still gets a live d
    lb[dead, 0:2] = np.array([0x0400], np.uint16).view(np.uint8)
    b = rng.integers(0, 256, (n, 8, BYTES[ttype]), dtype=np.uint8)
    b[:, :, 0:4] = 0
    b[np.arange(n), live] = lb
    return b.reshape(-1, BYTES[ttype])
