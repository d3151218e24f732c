"""IQ4_NL and IQ4_XS blocks (GGML types 20 and 23) in NumPy: the codecs, the build's one-pass quantisers, the dot contract restated, and the
twins that pin both types to what the project already trusts.

  * code book KV[16] (ggml's published kvalues_iq4nl), indexed by the stored nibble.
  * IQ4_NL: 18 B per 32 weights, f16 d, qs[16].  Weight j (0..15) = d KV[qs[j] & 15], weight j + 16 = d KV[qs[j] >> 4].
  * IQ4_XS: 136 B per 256 weights, f16 d, u16 scales_h (little endian), scales_l[4], qs[128].  Sub-block j (0..7, 32 weights) has
    ls_j = ((scales_l[j / 2] >> 4 (j % 2)) & 15) | ((scales_h >> 2 j) & 3) << 4, s_j = ls_j - 32, nibbles qs[16 j .. 16 j + 15] ordered as in
    an IQ4_NL block, w = (d s_j) KV[q].  Both products are exact in binary32 (11 bits times 6, then 17 times 7).
  Everything below works on 32-weight sub-blocks: n IQ4_NL blocks are n sub-blocks, n IQ4_XS blocks are 8 n, in order.
  * quantise (the build's own, not ggml's search), all in binary32.  IQ4_NL: max = the element of largest magnitude with its sign, the
    first one on ties; d = max / -127; id = d ? 1 / d : 0 from the unrounded d; d stored as f16; index = the number of k in 0..14 with
    x id > (KV[k] + KV[k + 1]) / 2.  IQ4_XS: r_j = max_j / -127 per sub-block, d = max |r_j| / 31 stored as f16, dq its value,
    s_j = clamp(rint(r_j / dq), -32, 31) (0 when dq == 0), dl = dq s_j, idl = dl ? 1 / dl : 0, indices as above with x idl.
  * gemv, the contract: per weight row and K-split slab, over the 256-k runs b ascending and inside a run its eight sub-blocks j ascending,
        acc = fmaf(D[b][j] d8[b], (float)P[b][j], acc),    P[b][j] = sum_{k < 32} KV[q_k] a_k  (exact, |P| <= 32 127 128 < 2^23),
    D = d (IQ4_NL) or d (float)s_j (IQ4_XS), the product D d8 rounded once to binary32; slabs added in ascending order.  This is
    q8_0_ref.gemv with D in place of the Q8_0 block's d and KV[q] in place of its q.
  * Q8_0 twin: the Q8_0 block with d = D and q8 = KV[q], wherever D is an f16 (every IQ4_NL block; an IQ4_XS sub-block whose d s_j is one).
  * Q6_K twin: a 256-k run with seven dead sub-blocks (IQ4_NL: d = +0; IQ4_XS: ls = 32, so s = 0) and one live one whose indices lie in
    6..10 (KV -22..25, q6 = KV + 32 in 10..57) — and for IQ4_XS whose s_j is +- a power of two, because only then
    fl((d s) d8) = s fl(d d8) — is the Q6_K block with the same d, scales = s_j (1 for IQ4_NL) on the live sub-block's two groups and 0
    elsewhere: fmaf(s X, P, acc) and fmaf(X, s P, acc) round the same exact value."""
import numpy as np

import q8_0_ref as Q8
from q5k_ref import fmaf

IQ4_NL, IQ4_XS = 20, 23
BYTES = {IQ4_NL: 18, IQ4_XS: 136}
ELEMS = {IQ4_NL: 32, IQ4_XS: 256}
SUBS = {IQ4_NL: 1, IQ4_XS: 8}   # 32-weight sub-blocks per block
QS_AT = {IQ4_NL: 2, IQ4_XS: 8}  # offset of the nibble bytes
KV = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], np.int64)
MID = ((KV[:-1] + KV[1:]).astype(np.float32) * np.float32(0.5)).astype(np.float32)
TWIN_LO, TWIN_HI = 6, 10         # the indices of a Q6_K-twin-able live sub-block: KV -22 .. 25


def _blocks(ttype, buf):
    return np.frombuffer(np.ascontiguousarray(buf).tobytes(), np.uint8).reshape(-1, BYTES[ttype])


def indices(ttype, blocks):
    """the stored nibbles (n sub-blocks, 32): 0..15"""
    qs = _blocks(ttype, blocks)[:, QS_AT[ttype]:].reshape(-1, 16).astype(np.int64)
    return np.concatenate([qs & 15, qs >> 4], axis=1)


def d_bits(ttype, blocks):
    """the f16 d of every block, as bits (n blocks,)"""
    return _blocks(ttype, blocks)[:, 0:2].copy().view(np.uint16)[:, 0]


def d_of(ttype, blocks):
    return d_bits(ttype, blocks).view(np.float16).astype(np.float32)


def ls_of(blocks):
    """the stored 6-bit scales of IQ4_XS blocks (n, 8): 0..63"""
    b = _blocks(IQ4_XS, blocks)
    sh = b[:, 2:4].copy().view("<u2")[:, 0].astype(np.int64)
    sl = b[:, 4:8].astype(np.int64)
    j = np.arange(8)
    return ((sl[:, j // 2] >> (4 * (j % 2))) & 15) | (((sh[:, None] >> (2 * j)) & 3) << 4)


def sub_scales(ttype, blocks):
    """D of every sub-block in binary32 (n sub-blocks,): d, or d (float)s_j — exact"""
    d = d_of(ttype, blocks)
    if ttype == IQ4_NL:
        return d
    with np.errstate(all="ignore"):
        return (d[:, None] * (ls_of(blocks) - 32).astype(np.float32)).astype(np.float32).reshape(-1)


def dequant(ttype, blocks):
    """w = D KV[q] in binary32 (tk_iq4nl_dequant / tk_iq4xs_dequant's expression); (n sub-blocks, 32)"""
    with np.errstate(all="ignore"):
        return (sub_scales(ttype, blocks)[:, None] * KV[indices(ttype, blocks)].astype(np.float32)).astype(np.float32)


def make_blocks(ttype, idx, d, ls=None):
    """blocks from the indices (n sub-blocks, 32), d per block (floats stored as f16, or uint16 bit patterns taken as they are) and, for
    IQ4_XS, the stored scales ls (n blocks, 8) in 0..63"""
    idx = np.asarray(idx).reshape(-1, 32).astype(np.int64)
    assert idx.min() >= 0 and idx.max() < 16 and idx.shape[0] % SUBS[ttype] == 0
    n = idx.shape[0] // SUBS[ttype]
    d = np.asarray(d).reshape(-1)
    b = np.zeros((n, BYTES[ttype]), np.uint8)
    b[:, 0:2] = (d if d.dtype == np.uint16 else d.astype(np.float32).astype(np.float16)).view(np.uint8).reshape(-1, 2)
    b[:, QS_AT[ttype]:] = ((idx[:, :16]) | (idx[:, 16:] << 4)).astype(np.uint8).reshape(n, -1)
    if ttype == IQ4_XS:
        ls = np.asarray(ls).reshape(n, 8).astype(np.int64)
        assert ls.min() >= 0 and ls.max() < 64
        b[:, 2:4] = ((ls >> 4) << (2 * np.arange(8))).sum(axis=1).astype("<u2").view(np.uint8).reshape(n, 2)
        b[:, 4:8] = ((ls[:, 0::2] & 15) | ((ls[:, 1::2] & 15) << 4)).astype(np.uint8)
    return b


def _signed_max(x):
    first = np.abs(x).argmax(axis=1)                                     # the first of equal magnitudes: `if (amax < fabsf(v))`
    return x[np.arange(x.shape[0]), first]


def _inv(d):
    return np.where(d != 0, np.float32(1.0) / np.where(d != 0, d, np.float32(1.0)), np.float32(0.0)).astype(np.float32)


def _index(v):
    return (v[:, :, None] > MID[None, None, :]).sum(axis=2)


def quantize(ttype, x):
    """float weights (..., 32 n | 256 n) -> blocks: tk_quantize_iq4_nl / tk_quantize_iq4_xs in binary32, operation for operation"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 32)
    with np.errstate(all="ignore"):
        r = (_signed_max(x) / np.float32(-127.0)).astype(np.float32)
        if ttype == IQ4_NL:
            return make_blocks(ttype, _index((x * _inv(r)[:, None]).astype(np.float32)), r)
        r = r.reshape(-1, 8)
        d = (np.abs(r).max(axis=1) / np.float32(31.0)).astype(np.float32).astype(np.float16)
        dq = d.astype(np.float32)[:, None]
        s = np.where(dq != 0, np.rint((r / np.where(dq != 0, dq, np.float32(1.0))).astype(np.float32)), np.float32(0.0)).clip(-32, 31)
        dl = (dq * s.astype(np.float32)).astype(np.float32).reshape(-1)
        idx = _index((x * _inv(dl)[:, None]).astype(np.float32))
    return make_blocks(ttype, idx, d.view(np.uint16), s.astype(np.int64) + 32)


def q8_0_twinable(ttype, blocks):
    """per sub-block: D is an f16, so the sub-block is a Q8_0 block"""
    D = sub_scales(ttype, blocks)
    with np.errstate(all="ignore"):
        return D.astype(np.float16).astype(np.float32).view(np.uint32) == D.view(np.uint32)


def to_q8_0(ttype, blocks):
    """the Q8_0 twins (n sub-blocks, 34): d = D (which must be an f16), q8 = KV[q]"""
    assert q8_0_twinable(ttype, blocks).all()
    return Q8.make_blocks(KV[indices(ttype, blocks)], sub_scales(ttype, blocks).astype(np.float16).view(np.uint16))


def gemv(ttype, blocks, rows, K, ks, q8, d8):
    """y [nrows][rows] of the dot contract.  q8 [nrows][K] int8 and d8 [nrows][K / 256] as oracle_lib.q8k_quantize gives them per row.
    (The integer sums run as binary64 matrix products: every partial sum is an integer below 2^53, so they are exact.)"""
    nb = K // 256
    q = KV[indices(ttype, blocks)].astype(np.float64)
    assert q.shape[0] == rows * nb * 8
    q = q.reshape(rows, nb, 8, 32)
    D = sub_scales(ttype, blocks).reshape(rows, nb, 8)
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
                    acc = fmaf((D[None, :, blk, j] * dd).astype(np.float32), P.astype(np.float32), acc)
            y = acc if y is None else (y + acc).astype(np.float32)
    return y


def quantize_twin_sparse(ttype, w, seed=0):
    """float weights (..., 256 n) -> Q6_K-twin-able blocks: per 256-k run one live sub-block at a position that walks with the run (all
    eight occur) with indices in 6..10 — the nearest of KV[6..10] to x / D, D = +- amax / 22 with both signs occurring, and for IQ4_XS
    D = d s with s walking over +-1, +-2, ... +-16, -32 —; the other seven are dead (IQ4_NL: d = +0, IQ4_XS: ls = 32) with random nibbles,
    which must not matter.  A test's own encoder: it only has to keep the model's weights sensible"""
    x = np.ascontiguousarray(w, np.float32).reshape(-1, 8, 32)
    n = x.shape[0]
    rng = np.random.default_rng(seed)
    live = (np.arange(n) * 3 + seed) % 8
    xl = x[np.arange(n), live].astype(np.float64)
    sign = np.where((np.arange(n) + seed) % 2 == 0, 1.0, -1.0)
    pows = np.array([1, -1, 2, -2, 4, -4, 8, -8, 16, -16, -32], np.int64)
    s = pows[(np.arange(n) * 5 + seed) % len(pows)] if ttype == IQ4_XS else np.ones(n, np.int64)
    d = (sign * np.abs(xl).max(axis=1) / 22.0 / np.abs(s)).astype(np.float16)
    d[(d.view(np.uint16) & 0x7FFF) < 0x0400] = np.float16(2.0 ** -14)    # an all-zero live sub-block still gets a live (normal) d
    D = d.astype(np.float64) * s
    il = np.abs(xl[:, :, None] / D[:, None, None] - KV[None, None, TWIN_LO:TWIN_HI + 1]).argmin(axis=2) + TWIN_LO
    idx = rng.integers(0, 16, (n, 8, 32))
    idx[np.arange(n), live] = il
    if ttype == IQ4_NL:
        dd = np.zeros((n, 8), np.float16)
        dd[np.arange(n), live] = d
        return make_blocks(ttype, idx.reshape(-1, 32), dd.reshape(-1).view(np.uint16))
    ls = np.full((n, 8), 32, np.int64)
    ls[np.arange(n), live] = s + 32
    return make_blocks(ttype, idx.reshape(-1, 32), d.view(np.uint16), ls)


def to_q6k(ttype, blocks):
    """twin-able runs -> the Q6_K blocks the oracle runs (flat bytes): q8_0_ref.to_q6k on Q8_0 blocks holding d on the live sub-block
    and +0 on the dead ones, then scales = s_j in place of 1 for IQ4_XS"""
    idx = indices(ttype, blocks)
    if ttype == IQ4_NL:
        return Q8.to_q6k(Q8.make_blocks(KV[idx], d_bits(ttype, blocks)))
    s = ls_of(blocks) - 32                                               # (n, 8)
    assert ((s != 0).sum(axis=1) <= 1).all()
    sl = s[np.arange(s.shape[0]), (s != 0).argmax(axis=1)]
    assert np.isin(np.abs(sl), [0, 1, 2, 4, 8, 16, 32]).all()
    d = np.where(s != 0, d_bits(ttype, blocks)[:, None], 0).astype(np.uint16)
    q6 = Q8.to_q6k(Q8.make_blocks(KV[idx], d.reshape(-1))).reshape(-1, Q8.Q6K_BYTES).copy()
    sc = q6[:, 192:208].view(np.int8).astype(np.int64) * sl[:, None]
    q6[:, 192:208] = sc.astype(np.int8).view(np.uint8)
    return q6.reshape(-1)
