"""Q3_K blocks (GGML type 11, 110 B per 256 weights: hmask[32], qs[64], scales[12], f16 d) in NumPy: the decode the HIP path implements,
and the exact Q6_K twin of a Q3_K block (same d, scales[g] = sc6_g - 32, q6 = q + 32): the same weights bit for bit and the same integer
block sum, so the oracle's Q6_K results on the twins are the expected Q3_K results."""
import numpy as np

Q3K_BYTES, Q6K_BYTES = 110, 210


def _blocks(buf):
    return np.frombuffer(np.ascontiguousarray(buf).tobytes(), np.uint8).reshape(-1, Q3K_BYTES)


def quants(blocks):
    """q (n, 256) int in -4..3: weight i = 128 n + 32 j + l has low = (qs[32 n + l] >> 2 j) & 3, high = (hmask[l] >> (4 n + j)) & 1,
    q = low + 4 high - 4"""
    b = _blocks(blocks)
    hm, qs = b[:, 0:32].astype(np.int64), b[:, 32:96].astype(np.int64)
    q = np.zeros((b.shape[0], 256), np.int64)
    for n in range(2):
        for j in range(4):
            low = (qs[:, 32 * n:32 * n + 32] >> (2 * j)) & 3
            high = (hm >> (4 * n + j)) & 1
            q[:, 128 * n + 32 * j:128 * n + 32 * j + 32] = low + 4 * high - 4
    return q


def scales(blocks):
    """s (n, 16) int in -32..31: sc6_g - 32 with the low 4 bits of sc6_g in scales[g] & 15 (g < 8) or scales[g - 8] >> 4, and the high
    2 bits in (scales[8 + (g & 3)] >> 2 (g >> 2)) & 3"""
    sc = _blocks(blocks)[:, 96:108].astype(np.int64)
    s = np.zeros((sc.shape[0], 16), np.int64)
    for g in range(16):
        low = sc[:, g] & 15 if g < 8 else sc[:, g - 8] >> 4
        high = (sc[:, 8 + (g & 3)] >> (2 * (g >> 2))) & 3
        s[:, g] = (low | (high << 4)) - 32
    return s


def d_of(blocks):
    return _blocks(blocks)[:, 108:110].copy().view(np.float16).astype(np.float32)[:, 0]


CHUNK = 1 << 14  # blocks per pass of the two bulk functions below: whole Mistral-7B matrices go through them


def dequant(blocks):
    """w = (d s_g) q in binary32, one rounding per operation (tk_q3k_dequant's expression); (n, 256)"""
    b = _blocks(blocks)
    if b.shape[0] > CHUNK:
        return np.concatenate([dequant(b[i:i + CHUNK]) for i in range(0, b.shape[0], CHUNK)])
    with np.errstate(all="ignore"):
        ds = d_of(blocks)[:, None] * scales(blocks).astype(np.float32)           # (n, 16)
        return (np.repeat(ds, 16, axis=1) * quants(blocks).astype(np.float32)).astype(np.float32)


def q3k_to_q6k(blocks):
    """Q3_K blocks -> their Q6_K twins (n x 210 bytes, flat): d verbatim, scales[g] = s_g as int8, q6 = q + 32 in Q6_K's packing
    (weight 128 n + 32 c + l: low nibble in ql[64 n + 32 (c & 1) + l] (high half of the byte for c >= 2), bits 2c, 2c + 1 of qh[32 n + l])"""
    b = _blocks(blocks)
    if b.shape[0] > CHUNK:
        return np.concatenate([q3k_to_q6k(b[i:i + CHUNK]) for i in range(0, b.shape[0], CHUNK)])
    q6 = (quants(b) + 32).astype(np.uint8)
    out = np.zeros((b.shape[0], Q6K_BYTES), np.uint8)
    for n in range(2):
        for c in range(4):
            v = q6[:, 128 * n + 32 * c:128 * n + 32 * c + 32]
            lo = slice(64 * n + 32 * (c & 1), 64 * n + 32 * (c & 1) + 32)
            out[:, lo] |= (v & 15) << (4 * (c >> 1))
            out[:, 128 + 32 * n:128 + 32 * n + 32] |= (v >> 4) << (2 * c)
    out[:, 192:208] = scales(b).astype(np.int8).view(np.uint8)
    out[:, 208:210] = b[:, 108:110]
    return out.reshape(-1)


def make_block(q, s, d):
    """one Q3_K block from q (256 ints in -4..3), s (16 ints in -32..31) and d (float, stored as f16): the encoder of the layout above"""
    b = np.zeros(Q3K_BYTES, np.uint8)
    u = np.asarray(q, np.int64) + 4
    for i in range(256):
        n, j, l = i >> 7, (i & 127) >> 5, i & 31
        b[32 + 32 * n + l] |= (u[i] & 3) << (2 * j)
        b[l] |= (u[i] >> 2) << (4 * n + j)
    for g in range(16):
        v = int(s[g]) + 32
        if g < 8:
            b[96 + g] |= v & 15
        else:
            b[96 + g - 8] |= (v & 15) << 4
        b[96 + 8 + (g & 3)] |= (v >> 4) << (2 * (g >> 2))
    b[108:110] = np.array([d], np.float16).view(np.uint8)
    return b
