"""Q5_K blocks (GGML type 13, 176 B per 256 weights) in NumPy: the decode the HIP path implements, and the re-encoding of Q4_K blocks
as Q5_K blocks with zero high bits (same d, dmin, scales, qs: the same weights, so the oracle's Q4_K results are the expected ones)."""
import numpy as np

Q4K_BYTES, Q5K_BYTES = 144, 176


def q4k_to_q5k(buf):
    """Q4_K blocks (bytes, n x 144) -> Q5_K blocks (n x 176) with qh = 0"""
    b = np.frombuffer(np.ascontiguousarray(buf).tobytes(), np.uint8).reshape(-1, Q4K_BYTES)
    out = np.zeros((b.shape[0], Q5K_BYTES), np.uint8)
    out[:, :16] = b[:, :16]      # d, dmin, scales[12]
    out[:, 48:] = b[:, 16:]      # qs[128] after qh[32]
    return out.reshape(-1)


def scale_min(scales, j):
    """6-bit (scale, min) pair j of the 12 packed bytes, for every block: arrays of int"""
    s = scales.astype(np.int64)
    if j < 4:
        return s[:, j] & 63, s[:, j + 4] & 63
    return (s[:, j + 4] & 0x0F) | ((s[:, j - 4] >> 6) << 4), (s[:, j + 4] >> 4) | ((s[:, j] >> 6) << 4)


def quants(blocks):
    """q5 (n, 256) int: low | high << 4 with low = (qs[32 (j / 2) + l] >> 4 (j % 2)) & 15, high = (qh[l] >> j) & 1"""
    b = np.frombuffer(np.ascontiguousarray(blocks).tobytes(), np.uint8).reshape(-1, Q5K_BYTES)
    qh, qs = b[:, 16:48].astype(np.int64), b[:, 48:].astype(np.int64)
    q = np.zeros((b.shape[0], 256), np.int64)
    for j in range(8):
        low = (qs[:, 32 * (j // 2):32 * (j // 2) + 32] >> (4 * (j % 2))) & 15
        q[:, 32 * j:32 * j + 32] = low | (((qh >> j) & 1) << 4)
    return q


def dequant(blocks):
    """w = (d sc_j) q - dmin m_j in binary32, one rounding per operation (tk_q5k_dequant's expression)"""
    b = np.frombuffer(np.ascontiguousarray(blocks).tobytes(), np.uint8).reshape(-1, Q5K_BYTES)
    d = b[:, 0:2].copy().view(np.float16).astype(np.float32)[:, 0]
    dmin = b[:, 2:4].copy().view(np.float16).astype(np.float32)[:, 0]
    q = quants(b)
    w = np.zeros(q.shape, np.float32)
    for j in range(8):
        sc, m = scale_min(b[:, 4:16], j)
        a = (d * sc.astype(np.float32))[:, None] * q[:, 32 * j:32 * j + 32].astype(np.float32)
        w[:, 32 * j:32 * j + 32] = a - (dmin * m.astype(np.float32))[:, None]
    return w


def fmaf(a, b, c):
    """binary32 fma, one rounding: a, b, c float32 arrays.  a*b is exact in binary64; TwoSum gives the exact s + e = a*b + c; rounding s
    to binary32 is the correct result except where s sits exactly on a binary32 midpoint and e != 0, where e decides the side"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c64 = c.astype(np.float64)
    s = p + c64
    bb = s - p
    e = (p - (s - bb)) + (c64 - bb)
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    diff = s - r64
    nxt = np.nextafter(r, np.where(diff > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    tie = (diff != 0) & (2.0 * diff == nxt.astype(np.float64) - r64)
    away = tie & (e != 0) & (np.sign(e) == np.sign(diff))
    return np.where(away, nxt, r).astype(np.float32)


def gemv(blocks, rows, K, ks, q8, d8, bsum):
    """y [nrows][rows] of the Q5_K dot contract: per slab acc = fmaf(d d8, P, acc); acc = fmaf(-(dmin d8), M, acc) over its blocks in
    ascending order with P, M exact integers; y = acc_0 + acc_1 + ... .  q8 [nrows][K] int8, d8 [nrows][K / 256], bsum [nrows][K / 32]
    as oracle_lib.q8k_quantize gives them per row"""
    nb = K // 256
    b = np.frombuffer(np.ascontiguousarray(blocks).tobytes(), np.uint8).reshape(rows, nb, Q5K_BYTES)
    flat = b.reshape(-1, Q5K_BYTES)
    q = quants(flat).reshape(rows, nb * 8, 32)
    sc = np.stack([scale_min(flat[:, 4:16], j)[0] for j in range(8)], 1).reshape(rows, nb * 8)
    mn = np.stack([scale_min(flat[:, 4:16], j)[1] for j in range(8)], 1).reshape(rows, nb * 8)
    d = flat[:, 0:2].copy().view(np.float16).astype(np.float32).reshape(rows, nb)
    dmin = flat[:, 2:4].copy().view(np.float16).astype(np.float32).reshape(rows, nb)
    nrows = q8.shape[0]
    a = q8.astype(np.int64).reshape(nrows, nb * 8, 32)
    bs = bsum.astype(np.int64).reshape(nrows, nb * 8)
    y = None
    per = nb // ks
    for s in range(ks):
        acc = np.zeros((nrows, rows), np.float32)
        for blk in range(s * per, (s + 1) * per):
            P = np.zeros((nrows, rows), np.int64)
            M = np.zeros((nrows, rows), np.int64)
            for j in range(8):
                t = 8 * blk + j
                P += (a[:, t, :] @ q[:, t, :].T) * sc[None, :, t]
                M += bs[:, t, None] * mn[None, :, t]
            dd = d8[:, blk, None].astype(np.float32)
            acc = fmaf(d[None, :, blk] * dd, P.astype(np.float32), acc)
            acc = fmaf(-(dmin[None, :, blk] * dd), M.astype(np.float32), acc)
        y = acc if y is None else (y + acc).astype(np.float32)
    return y
