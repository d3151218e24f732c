"""Q8_0 blocks (GGML type 8, 34 B per 32 weights: f16 d, 32 int8 quants) in NumPy: the codec, ggml's published quantiser, the Q6_K twin
that pins the type to the oracle, and the dot contract restated.

  * decode: w = d q, d the block's f16 widened to binary32 and q any int8 (-128 included); the product is exact in binary32.
  * quantise (quantize_row_q8_0_ref): d = amax / 127, id = d ? 1 / d : 0, q = roundf(x id) (halves away from zero), d stored as f16.
  * gemv: per weight row and K-split slab, over the 256-k runs b ascending and inside a run the eight 32-blocks j ascending,
        acc = fmaf(d[b][j] d8[b], (float)P[b][j], acc),    P[b][j] = sum_{k < 32} q_k a_k  (exact, |P| < 2^23),
    d8[b] the activation row's Q8_K scale of run b, the product of the two scales rounded once to binary32; slabs added in ascending order.
  * Q6_K twin: a 256-k run with seven of its eight d equal to +0 and the live block's q in -32..31 is the Q6_K block with the same d,
    scales = 1 on the live block's two groups and 0 elsewhere, q6 = q + 32 there: the zero blocks' fmaf(+-0, P, acc) leave acc as it is
    (acc starts at +0 and a binary32 sum is -0 only when both terms are), so the run contributes the oracle's one fmaf(d d8, P, acc)."""
import numpy as np

from q5k_ref import fmaf

Q8_0_BYTES, Q6K_BYTES = 34, 210
CHUNK = 1 << 15  # 256-k runs per pass of the bulk functions: whole Mistral-7B matrices go through them


def _blocks(buf):
    return np.frombuffer(np.ascontiguousarray(buf).tobytes(), np.uint8).reshape(-1, Q8_0_BYTES)


def quants(blocks):
    """q (n, 32) int in -128..127"""
    return _blocks(blocks)[:, 2:34].copy().view(np.int8).astype(np.int64)


def d_of(blocks):
    return _blocks(blocks)[:, 0:2].copy().view(np.float16).astype(np.float32)[:, 0]


def dequant(blocks):
    """w = d q in binary32 (tk_q8_0_dequant's expression); (n, 32)"""
    b = _blocks(blocks)
    if b.shape[0] > 8 * CHUNK:
        return np.concatenate([dequant(b[i:i + 8 * CHUNK]) for i in range(0, b.shape[0], 8 * CHUNK)])
    with np.errstate(all="ignore"):
        return (d_of(blocks)[:, None] * quants(blocks).astype(np.float32)).astype(np.float32)


def make_blocks(q, d):
    """Q8_0 blocks (n, 34) from q (n, 32) in -128..127 and d (n,): floats stored as f16, or uint16 f16 bit patterns taken as they are"""
    q = np.asarray(q).reshape(-1, 32)
    d = np.asarray(d).reshape(-1)
    b = np.zeros((q.shape[0], Q8_0_BYTES), np.uint8)
    b[:, 0:2] = (d if d.dtype == np.uint16 else d.astype(np.float32).astype(np.float16)).view(np.uint8).reshape(-1, 2)
    b[:, 2:34] = q.astype(np.int8).view(np.uint8)
    return b


def quantize(x):
    """float weights (..., 32 n) -> Q8_0 blocks (n, 34): quantize_row_q8_0_ref in binary32, operation for operation"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 32)
    with np.errstate(all="ignore"):
        amax = np.abs(x).max(axis=1)
        d = (amax / np.float32(127.0)).astype(np.float32)
        inv = np.where(d != 0, np.float32(1.0) / np.where(d != 0, d, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
        v = (x * inv[:, None]).astype(np.float32).astype(np.float64)
    q = np.sign(v) * np.floor(np.abs(v) + 0.5)        # roundf: exact in binary64, |v| <= 128
    return make_blocks(q, d)


def live_of(blocks):
    """per 256-k run (eight blocks) of twin-able blocks: the index of the one block whose d is not +0 (0 when all eight are)"""
    dbits = _blocks(blocks)[:, 0:2].copy().view(np.uint16).reshape(-1, 8)
    assert ((dbits != 0).sum(axis=1) <= 1).all()
    return (dbits != 0).argmax(axis=1)


def to_q6k(blocks):
    """twin-able Q8_0 runs -> their Q6_K twins (n / 8 x 210 bytes, flat): d of the live block, scales[2 j] = scales[2 j + 1] = 1 for the
    live block j and 0 elsewhere, q6 = q + 32 on the live block and 32 elsewhere, in Q6_K's packing (weight 128 n + 32 c + l: low nibble in
    ql[64 n + 32 (c & 1) + l] (high half of the byte for c >= 2), bits 2c, 2c + 1 of qh[32 n + l])"""
    b = _blocks(blocks)
    if b.shape[0] > 8 * CHUNK:
        return np.concatenate([to_q6k(b[i:i + 8 * CHUNK]) for i in range(0, b.shape[0], 8 * CHUNK)])
    live = live_of(b)
    runs = b.reshape(-1, 8, Q8_0_BYTES)
    n = runs.shape[0]
    pick = runs[np.arange(n), live]                                      # (n, 34): the live blocks
    ql = quants(pick)
    assert ql.min() >= -32 and ql.max() <= 31
    q6 = np.full((n, 256), 32, np.uint8)
    cols = live[:, None] * 32 + np.arange(32)[None, :]
    q6[np.arange(n)[:, None], cols] = (ql + 32).astype(np.uint8)
    out = np.zeros((n, Q6K_BYTES), np.uint8)
    for h in range(2):
        for c in range(4):
            v = q6[:, 128 * h + 32 * c:128 * h + 32 * c + 32]
            lo = slice(64 * h + 32 * (c & 1), 64 * h + 32 * (c & 1) + 32)
            out[:, lo] |= (v & 15) << (4 * (c >> 1))
            out[:, 128 + 32 * h:128 + 32 * h + 32] |= (v >> 4) << (2 * c)
    has_live = (pick[:, 0:2] != 0).any(axis=1)
    sc = np.zeros((n, 16), np.uint8)
    sc[np.arange(n), 2 * live] = has_live
    sc[np.arange(n), 2 * live + 1] = has_live
    out[:, 192:208] = sc
    out[:, 208:210] = pick[:, 0:2]
    return out.reshape(-1)


def quantize_twin_sparse(w, seed=0):
    """float weights (..., 256 n) -> twin-able Q8_0 blocks (8 n, 34): per 256-k run one live block, at a position that changes from run to
    run (all eight occur), quantised to -32..31 with d = amax / 31; the other seven blocks get d = +0 and random quants, which must not
    matter.  A test's own encoder — any twin-able run would do; it only has to keep the model's weights sensible"""
    x = np.ascontiguousarray(w, np.float32).reshape(-1, 8, 32)
    if x.shape[0] > CHUNK:
        return np.concatenate([quantize_twin_sparse(x[i:i + CHUNK], seed + 1 + i // CHUNK) for i in range(0, x.shape[0], CHUNK)])
    n = x.shape[0]
    rng = np.random.default_rng(seed)
    live = rng.integers(0, 8, n)
    xl = x[np.arange(n), live].astype(np.float64)                        # (n, 32)
    d = (np.abs(xl).max(axis=1) / 31.0).astype(np.float16)
    d[d == 0] = np.float16(2.0 ** -14)                                   # an all-zero live block still gets a live (non-zero) d
    with np.errstate(all="ignore"):
        ql = np.rint(xl / d.astype(np.float64)[:, None]).clip(-32, 31)
    q = rng.integers(-128, 128, (n, 8, 32), dtype=np.int8)
    q[np.arange(n), live] = ql.astype(np.int8)
    dd = np.zeros((n, 8), np.float16)
    dd[np.arange(n), live] = d
    return make_blocks(q.reshape(-1, 32), dd.reshape(-1).view(np.uint16))


def gemv(blocks, rows, K, ks, q8, d8):
    """y [nrows][rows] of the Q8_0 dot contract.  q8 [nrows][K] int8 and d8 [nrows][K / 256] as oracle_lib.q8k_quantize gives them per
    row.  (The integer sums run as binary64 matrix products: every partial sum is an integer below 2^53, so they are exact.)"""
    nb = K // 256
    flat = _blocks(blocks)
    assert flat.shape[0] == rows * nb * 8
    q = quants(flat).reshape(rows, nb, 8, 32).astype(np.float64)
    d = d_of(flat).reshape(rows, nb, 8)
    nrows = q8.shape[0]
    a = q8.astype(np.float64).reshape(nrows, nb, 8, 32)
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
            y = acc if y is None else (y + acc).astype(np.float32)
    return y
