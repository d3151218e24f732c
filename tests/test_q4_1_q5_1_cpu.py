"""CPU: Q4_1 and Q5_1 (GGML types 3 and 7) — the constants, the NumPy codecs against the formula written out by hand, the host quantiser
entries against the NumPy quantisers byte for byte, the round-trip bound, the refused arguments, the restated dot contract (with its min
term) against the oracle on Q4_K twins, its error bound against the float64 dot, and the GGUF reader's size checks for files of the types."""
import ctypes as C
import struct

import numpy as np
import pytest

import gguf_util as G
import oracle_lib as O
import q4_1_ref as R
import q5k_ref as Q5K
import q8_0_ref as Q8

TYPES = [R.Q4_1, R.Q5_1]
ENTRY = {R.Q4_1: "tk_mi355x_quantize_blocks_q4_1", R.Q5_1: "tk_mi355x_quantize_blocks_q5_1"}


@pytest.fixture(autouse=True)
def restated_types_are_the_librarys():
    """every test of this file restates types the library has to know: the restatement's type ids and block sizes are the library's"""
    import trackiellm_amd as tk
    assert {tk.TYPE_Q4_1: tk.llm.BLOCK_BYTES[tk.TYPE_Q4_1], tk.TYPE_Q5_1: tk.llm.BLOCK_BYTES[tk.TYPE_Q5_1]} == R.BYTES


def probe(path):
    import trackiellm_amd as tk
    hp = tk.LlmHParams()
    nv = C.c_int32(0)
    return tk.lib().tk_mi355x_gguf_probe(path.encode(), C.byref(hp), C.byref(nv))


def test_constants_and_struct_sizes():
    import trackiellm_amd as tk
    assert (tk.TYPE_Q4_1, tk.TYPE_Q5_1, tk.FTYPE_Q4_1, tk.FTYPE_Q5_1) == (3, 7, 3, 9)
    assert (tk.llm.BLOCK_BYTES[3], tk.llm.BLOCK_BYTES[7]) == (20, 24)
    assert 3 in tk.llm.TYPES_OF_32 and 7 in tk.llm.TYPES_OF_32
    # the entries write exactly 20 / 24 bytes per block: the bytes after the last block stay as they were
    x = np.arange(96, dtype=np.float32).reshape(3, 32)
    for t, nb in ((3, 20), (7, 24)):
        fn = getattr(tk.lib(), ENTRY[t])
        fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        out = np.full(3 * nb + 8, 0xA5, np.uint8)
        assert fn(x.ctypes.data_as(C.c_void_p), 3, out.ctypes.data_as(C.c_void_p)) == 0
        assert (out[3 * nb:] == 0xA5).all() and not (out[:3 * nb] == 0xA5).all()


def f16_bits(rng, n):
    """n finite f16 bit patterns of both signs: normal, subnormal and zero ones among them"""
    v = rng.integers(0, 1 << 16, n).astype(np.uint16)
    v[(v & 0x7C00) == 0x7C00] &= 0xBBFF                                    # no inf / nan
    v[0:4] = [0x0001, 0x83FF, 0x0000, 0x8000]                              # the smallest subnormal, the largest negative one, +0, -0
    return v


@pytest.mark.parametrize("ttype", TYPES)
def test_dequant_equals_the_hand_formula_on_random_bytes(ttype):
    """every byte of the block random (d and m finite, of both signs, subnormals among them), so every nibble and every qh bit position
    is distinguished; the formula of the format description per weight: d q exactly (binary64 holds it), plus m, rounded once"""
    rng = np.random.default_rng(40 + ttype)
    n = 96
    b = rng.integers(0, 256, (n, R.BYTES[ttype]), dtype=np.uint8)
    b[:, 0:2] = f16_bits(rng, n).view(np.uint8).reshape(n, 2)
    b[:, 2:4] = f16_bits(rng, n)[::-1].copy().view(np.uint8).reshape(n, 2)
    b[8:40, 0:2] = (rng.uniform(1e-3, 1e-2, 32) * rng.choice([-1.0, 1.0], 32)).astype(np.float16).view(np.uint8).reshape(32, 2)
    b[8:40, 2:4] = (rng.uniform(1e-3, 1e-1, 32) * rng.choice([-1.0, 1.0], 32)).astype(np.float16).view(np.uint8).reshape(32, 2)
    got_q, got_w = R.quants(ttype, b), R.dequant(ttype, b)
    seen = set()
    for i in range(n):
        raw = bytes(b[i])
        d = float(np.frombuffer(raw[0:2], np.float16)[0])
        m = float(np.frombuffer(raw[2:4], np.float16)[0])
        if ttype == R.Q4_1:
            qs = raw[4:20]
            q = [qs[j] & 15 for j in range(16)] + [qs[j] >> 4 for j in range(16)]
        else:
            qh = struct.unpack("<I", raw[4:8])[0]
            qs = raw[8:24]
            q = [(qs[j] & 15) | (((qh >> j) & 1) << 4) for j in range(16)] + [(qs[j] >> 4) | (((qh >> (j + 16)) & 1) << 4) for j in range(16)]
        seen |= set(q)
        assert [int(v) for v in got_q[i]] == q
        want = np.array([np.float32(d * v + m) for v in q], np.float32)   # d v is exact in binary64 and the sum of two binary64 rounds to binary32 as the fma does: 53 bits hold it
        assert np.array_equal(got_w[i].view(np.uint32), want.view(np.uint32)), i
    assert seen == set(range(R.L[ttype] + 1))
    # the codec round-trips
    assert np.array_equal(R.make_blocks(ttype, got_q, R.d_bits(ttype, b), R.m_bits(ttype, b)), b)
    # m = 0: the Q8_0 twin decodes to the same bits
    z = b.copy()
    z[:, 2:4] = 0
    z[1::2, 3] = 0x80                                                   # -0 as well
    w0, w8 = R.dequant(ttype, z), Q8.dequant(R.to_q8_0(ttype, z))
    assert np.array_equal(np.abs(w0).view(np.uint32), np.abs(w8).view(np.uint32)) and np.array_equal(w0 == 0, w8 == 0)
    # single qh bits and single nibbles, by hand
    if ttype == R.Q5_1:
        for bit in range(32):
            one = np.zeros(24, np.uint8)
            one[0:2] = np.array([1.0], np.float16).view(np.uint8)
            one[2:4] = np.array([-3.0], np.float16).view(np.uint8)
            one[4:8] = np.array([1 << bit], "<u4").view(np.uint8)
            w = R.dequant(ttype, one)[0]
            assert w[bit] == 13.0 and (np.delete(w, bit) == -3.0).all()
    one = np.zeros(R.BYTES[ttype], np.uint8)
    one[0:2] = np.array([1.0], np.float16).view(np.uint8)
    one[2:4] = np.array([0.5], np.float16).view(np.uint8)
    one[R.QS_AT[ttype] + 3] = 0xC5                                       # weight 3 = 5, weight 19 = 12
    w = R.dequant(ttype, one)[0]
    assert w[3] == 5.5 and w[19] == 12.5 and w.sum() == 17 + 16
    # the add rounds once: d q + m with d q = 15 * 2^-10 (exact) and m = 1 needs more than f16's bits but fits binary32
    one[0:2] = np.array([2.0 ** -10], np.float16).view(np.uint8)
    one[2:4] = np.array([1.0], np.float16).view(np.uint8)
    one[R.QS_AT[ttype]] = 0x0F
    assert R.dequant(ttype, one)[0, 0] == np.float32(1.0 + 15 * 2.0 ** -10)


def quantiser_inputs(ttype):
    lv = R.L[ttype]
    rng = np.random.default_rng(50 + ttype)
    x = [(rng.standard_normal((256, 32)) * 0.02).astype(np.float32), rng.standard_normal((64, 32)).astype(np.float32) * 1e3,
         (rng.standard_normal((64, 32)) * 1e-4).astype(np.float32), np.zeros((2, 32), np.float32), np.full((2, 32), -0.37, np.float32),
         np.full((2, 32), 1.25, np.float32)]
    t = (rng.standard_normal((8, 32)) * 0.1).astype(np.float32)         # ties for the minimum and for the maximum
    t[:, 3], t[:, 20], t[:, 31] = 3.0, 3.0, 3.0
    t[:, 0], t[:, 7], t[:, 16] = -2.0, -2.0, -2.0
    x.append(t)
    pos = np.abs(rng.standard_normal((16, 32))).astype(np.float32) + np.float32(0.5)      # blocks of one sign
    x += [pos, -pos]
    h = rng.integers(0, lv, (64, 32)).astype(np.float32) + 0.5          # min = 0, max = L: d = 1, id = 1, (x - min) id + 0.5 lands on integers
    h[:, 0], h[:, 1] = 0.0, lv
    x.append(h)
    x.append((h - np.float32(7.0)).astype(np.float32))                  # ... with a negative minimum: x - min is exact
    x.append((h * np.float32(0.75)).astype(np.float32))                 # id = fl(1 / 0.75) is inexact: products beside a half
    return np.concatenate(x)


@pytest.mark.parametrize("ttype", TYPES)
def test_host_quantiser_equals_the_numpy_quantiser_byte_for_byte(ttype):
    import trackiellm_amd as tk
    lv = R.L[ttype]
    x = quantiser_inputs(ttype)
    got = tk.quantize_blocks(ttype, x)
    assert got.shape == (x.shape[0], R.BYTES[ttype]) and got.dtype == np.uint8
    want = R.quantize(ttype, x)
    bad = np.argwhere((got != want).any(axis=1))
    assert bad.size == 0, (bad[:4].tolist(), got[bad[0, 0]], want[bad[0, 0]])
    # Q5_1 takes no clamp: on these inputs the value that is truncated stays below 32 (and Q4_1's below 16, so its clamp is idle too)
    v, _, _ = R.quantize_values(ttype, x)
    assert v.min() >= 0.5 and v.max() < lv + 1
    assert R.quants(ttype, got).max() == lv and R.quants(ttype, got).min() == 0
    # all-zero and constant blocks: d = +0, id = 0, every q = (int)0.5 = 0, m = x
    for c in (0.0, -0.37, 1.25):
        cb = R.quantize(ttype, np.full(32, c, np.float32))
        assert (R.d_bits(ttype, cb) == 0).all() and (R.quants(ttype, cb) == 0).all()
        assert R.m_of(ttype, cb)[0] == np.float32(np.float16(c)) and (R.dequant(ttype, cb) == np.float32(np.float16(c))).all()
    # ties: every element equal to the minimum gets 0, every one equal to the maximum gets L
    t = np.zeros((1, 32), np.float32)
    t[0, [3, 20, 31]], t[0, [0, 7, 16]] = 3.0, -2.0
    tb = R.quantize(ttype, t)
    q = R.quants(ttype, tb)[0]
    assert (q[[3, 20, 31]] == lv).all() and (q[[0, 7, 16]] == 0).all()
    assert float(R.m_of(ttype, tb)[0]) == -2.0 and float(R.d_of(ttype, tb)[0]) == float(np.float16(np.float32(5.0) / np.float32(lv)))
    # halves: with min = 0 and d = 1 the sum x + 0.5 is an integer and truncation keeps it: q = x + 0.5
    h = np.zeros(32, np.float32)
    h[1], h[2], h[3], h[4] = lv, 0.5, 1.5, lv - 0.5
    assert [int(v) for v in R.quants(ttype, R.quantize(ttype, h))[0, :5]] == [0, lv, 1, 2, lv]
    # a row of 256 n weights is n / 32 blocks, in order
    assert np.array_equal(tk.quantize_blocks(ttype, x[:16].reshape(2, 256)), want[:16])


@pytest.mark.parametrize("ttype", TYPES)
def test_decode_of_quantise_stays_within_the_bound_of_the_construction(ttype):
    """A bound, not a measurement.  mn, mx = the block's extremes, d = (mx - mn) / L (unrounded), t = (x - mn) / d in [0, L].
      * the truncated value is t + 0.5 up to three binary32 roundings of numbers below 32 (the subtraction, id = fl(1 / d), the product)
        and the add's: less than L 2^-21 together, so |t - q| <= 0.5 + L 2^-21 (t <= L (1 + 2^-22): Q4_1's clamp changes nothing) and
        |x - (mn + d q)| <= (0.5 + L 2^-21) d;
      * the stored scale: |f16(d) - d| <= 2^-11 d for a normal f16 (d >= 2^-14, true of this data), times q <= L;
      * the stored minimum: |f16(mn) - mn| <= max(2^-11 |mn|, 2^-25);
      * the decode's one rounding: 2^-24 |w|.
    Together |x - w| <= (0.5 + L 2^-21 + L 2^-11) d + max(2^-11 |mn|, 2^-25) + 2^-24 |w|."""
    lv = R.L[ttype]
    rng = np.random.default_rng(60 + ttype)
    x = np.concatenate([(rng.standard_normal((4096, 32)) * 0.02).astype(np.float32), rng.standard_normal((512, 32)).astype(np.float32),
                        (rng.standard_normal((512, 32)) * 0.02 + 3.0).astype(np.float32)])
    b = R.quantize(ttype, x)
    w = R.dequant(ttype, b).astype(np.float64)
    x64 = x.astype(np.float64)
    mn = x64.min(axis=1)
    d = (x64.max(axis=1) - mn) / lv
    assert (d >= 2.0 ** -14).all()
    bound = ((0.5 + lv * 2.0 ** -21 + lv * 2.0 ** -11) * d + np.maximum(2.0 ** -11 * np.abs(mn), 2.0 ** -25))[:, None] + 2.0 ** -24 * np.abs(w)
    err = np.abs(x64 - w)
    print(f"type {ttype}: largest |x - w| / bound = {(err / bound).max():.6f}; largest |x - w| / d = {(err / d[:, None]).max():.6f}")
    assert (err <= bound).all()
    assert (err / d[:, None]).max() > 0.45                               # the half step is in the sample


def test_refused_arguments():
    import trackiellm_amd as tk
    x = np.zeros(256, np.float32)
    out = np.zeros(8 * 34, np.uint8)
    xp, op = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for name in ENTRY.values():
        fn = getattr(tk.lib(), name)
        fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        assert fn(xp, 8, op) == 0 and fn(xp, 0, op) == 0
        assert fn(None, 1, op) != 0 and fn(xp, 1, None) != 0 and fn(xp, -1, op) != 0
    old = tk.lib().tk_mi355x_quantize_blocks
    old.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    for bad in (3, 7):
        assert old(bad, xp, 1, op) != 0
    # fill_synthetic_type takes a model and one of the two tensor types, nothing else (no GPU is needed to be refused)
    fst = tk.lib().tk_mi355x_llm_model_fill_synthetic_type
    fst.argtypes = [C.c_void_p, C.c_uint64, C.c_int]
    assert fst(None, 4, 3) != 0


def activations(rng, n, K):
    x = rng.standard_normal((n, K)).astype(np.float32)
    x[0, 256:512] = 0.0
    x[1, 0] = -7.0
    x[2, 0] = 7.0
    return x


def q8_rows(x):
    qs, ds, bs = zip(*[O.q8k_quantize(r) for r in x])
    return np.stack(qs), np.stack(ds).reshape(len(x), -1), np.stack(bs)


@pytest.mark.parametrize("ks", [1, 7])
@pytest.mark.parametrize("ttype", TYPES)
def test_restated_contract_equals_the_oracle_on_twin_rows(ttype, ks):
    """q4_1_ref.gemv on twin-sparse rows (Q5_1: live q <= 15, qh = 0) is oracle_lib.gemv_q8 on their Q4_K twins, bit for bit; and on
    Q5_1 rows with high bits q5k_ref.gemv on their Q5_K twins, which is the Q4_K arithmetic with a fifth bit"""
    rng = np.random.default_rng(70 + ttype)
    rows, K = 64, 1792
    w = (rng.standard_normal((rows, K)) * 0.02 + rng.choice([-0.05, 0.0, 0.05], (rows, 1))).astype(np.float32)
    b = R.quantize_twin_sparse(ttype, w, seed=5, q4_only=True)
    live = ((R.d_bits(ttype, b) != 0) | (R.m_bits(ttype, b) != 0)).reshape(-1, 8)
    assert (live.sum(axis=1) == 1).all() and set(live.argmax(axis=1).tolist()) == set(range(8))
    ml = R.m_of(ttype, b)
    assert (ml < 0).any() and (ml > 0).any() and (R.d_of(ttype, b) > 0).any()
    ql = R.quants(ttype, b)[live.reshape(-1)]
    assert ql.min() == 0 and ql.max() == 15
    x = activations(rng, 6, K)
    q8, d8, bs = q8_rows(x)
    assert (d8 < 0).any() and (d8 > 0).any() and (d8 == 0).any()
    twin = R.to_q4k(ttype, b)
    want = np.stack([O.gemv_q8(O.TYPE_Q4_K, twin, rows, K, ks, r) for r in x])
    got = R.gemv(ttype, b, rows, K, ks, q8, d8, bs)
    assert np.isfinite(want).all() and want.any()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (ks, np.abs(got - want).max())
    # the Q4_K twin re-encoded as Q5_K with zero high bits is the Q5_K twin, and q5k_ref agrees with both
    assert np.array_equal(R.to_q5k(ttype, b), Q5K.q4k_to_q5k(twin))
    got5 = Q5K.gemv(R.to_q5k(ttype, b), rows, K, ks, q8, d8, bs)
    assert np.array_equal(got5.view(np.uint32), want.view(np.uint32))
    if ttype == R.Q5_1:
        b5 = R.quantize_twin_sparse(ttype, w, seed=6)
        assert R.quants(ttype, b5).max() == 31
        got = R.gemv(ttype, b5, rows, K, ks, q8, d8, bs)
        want5 = Q5K.gemv(R.to_q5k(ttype, b5), rows, K, ks, q8, d8, bs)
        assert np.array_equal(got.view(np.uint32), want5.view(np.uint32))


@pytest.mark.parametrize("ttype", TYPES)
def test_contract_stays_within_the_activation_rounding_bound(ttype):
    """A bound, not a measurement: tests/test_q8_0_cpu.py's, with the min term.  With w = fl(d q + m) the dequantised weights, x the
    unquantised activations and a, d8 their Q8_K image:
      * the contract's exact-arithmetic value is E' = sum_k (d q_k + m) (d8_b a_k): the unrounded weights.  |w_k - (d q_k + m)| <=
        2^-24 |w_k| (1 + 2^-24), so |E' - sum_k w_k d8_b a_k| <= 2^-23 S with S = sum_k |w_k| |d8_b a_k|;
      * the activation rounding, as for Q8_0: |sum_k w_k (d8_b a_k - x_k)| <= sum_b (0.5 + 2^-15) |d8_b| sum_k |w_k|;
      * the binary32 evaluation makes one rounding per scale product and one per fmaf, 2 n = K / 16 of each per slab, then ks - 1 adds.
        The partial sums are bounded by T = sum_k (|d| q_k + |m|) |d8_b a_k| >= S (d q and m may cancel in w, not in the two chains):
        |R - E'| <= (2 n + ks + 1) 2^-24 T (1 + O(n 2^-24)); the test allows (2 n + ks + 1) 2^-23 T.
    So err <= 0.5 sum_b |d8_b| sum_k |w_k| + [2^-15 sum_b |d8_b| sum_k |w_k| + 2^-23 S + (K / 16 + ks + 1) 2^-23 T]."""
    rng = np.random.default_rng(84 + ttype)
    rows, K = 32, 4096
    w = (rng.standard_normal((rows, K)) * 0.02 + rng.choice([-0.03, 0.0, 0.03], (rows, 1))).astype(np.float32)
    b = R.quantize(ttype, w)
    wq = R.dequant(ttype, b).reshape(rows, K).astype(np.float64)
    mag = (np.abs(R.d_of(ttype, b).astype(np.float64))[:, None] * R.quants(ttype, b) + np.abs(R.m_of(ttype, b).astype(np.float64))[:, None]).reshape(rows, K)
    x = rng.standard_normal((8, K)).astype(np.float32)
    q8, d8, bs = q8_rows(x)
    for ks in (1, 4):
        got = R.gemv(ttype, b, rows, K, ks, q8, d8, bs).astype(np.float64)
        exact = x.astype(np.float64) @ wq.T
        absw = np.abs(wq).reshape(rows, K // 256, 256).sum(axis=2)                       # (rows, nb)
        bound = 0.5 * np.abs(d8).astype(np.float64) @ absw.T                            # (nrows, rows)
        xq = (q8.astype(np.float64).reshape(8, K // 256, 256) * d8.astype(np.float64)[:, :, None]).reshape(8, K)
        S = np.abs(xq) @ np.abs(wq).T
        T = np.abs(xq) @ mag.T
        slack = 2.0 ** -15 * 2 * bound + 2.0 ** -23 * S + (K // 16 + ks + 1) * 2.0 ** -23 * T
        err = np.abs(got - exact)
        assert (err <= bound + slack).all(), (ks, float((err / (bound + slack)).max()))
        assert err.max() > 0


def source(base, down0=None):
    """a tiny llama GGUF source whose every layer matrix and token_embd are `base` (the host quantiser's blocks), output Q6_K, norms F32;
    down0: the type of blk.0.ffn_down instead (the importance-matrix mix of llama.cpp's quantiser)"""
    import trackiellm_amd as tk
    cfg = O.tiny_config()
    orc = O.OracleLlm(cfg, seed=4)
    D, FF, QD, KVD = cfg.d_model, cfg.d_ff, cfg.n_head * cfg.head_dim, cfg.n_kv_head * cfg.head_dim
    shape = {1: (QD, D), 2: (KVD, D), 3: (KVD, D), 4: (D, QD), 6: (FF, D), 7: (FF, D), 8: (D, FF)}

    class Src(object):
        def get_tensor(self, layer, which):
            t, buf = orc.get_tensor(layer, which)
            if layer < 0 and which == O.T_OUTPUT:
                return O.TYPE_Q6_K, O.quantize_rows(O.TYPE_Q6_K, orc.dequant(layer, which, cfg.vocab, D))
            if (layer < 0 and which == O.T_TOKEN_EMBD) or (layer >= 0 and which in shape):
                w = orc.dequant(layer, which, *((cfg.vocab, D) if layer < 0 else shape[which]))
                ttype = down0 if (down0 is not None and layer == 0 and which == 8) else base
                return ttype, tk.quantize_blocks(ttype, w).reshape(-1)
            return t, buf
    return Src(), cfg


def type_of(raw, name):
    at = raw.index(G._s(name)) + len(G._s(name))
    ndim = struct.unpack_from("<I", raw, at)[0]
    return struct.unpack_from("<I", raw, at + 4 + 8 * ndim)[0]


@pytest.mark.parametrize("ttype", TYPES)
def test_gguf_of_one_type_passes_the_probe_and_short_data_is_refused(tmp_path, ttype):
    """an all-Q4_1 / all-Q5_1 file (output Q6_K): the probe accepts it; a file that ends one block early, whose ffn_down claims a K
    running past the end of the file or wrapping the element count, is refused; a K of whole blocks that is no multiple of 256 is sized
    block by block"""
    src, cfg = source(ttype)
    p = str(tmp_path / "whole.gguf")
    G.write_llama_gguf(p, src, cfg)
    raw = bytearray(open(p, "rb").read())
    for name, want in (("token_embd.weight", ttype), ("output.weight", 14), ("blk.0.attn_q.weight", ttype), ("blk.1.ffn_down.weight", ttype)):
        assert type_of(raw, name) == want, name
    assert probe(p) == 0
    # the last tensor of the file is blk.1.ffn_down
    (tmp_path / "one_short.gguf").write_bytes(bytes(raw[:-R.BYTES[ttype]]))
    assert probe(str(tmp_path / "one_short.gguf")) == 3004
    name = G._s("blk.0.ffn_down.weight")
    dims_at = raw.index(name) + len(name) + 4
    b = bytearray(raw)
    struct.pack_into("<QQ", b, dims_at, 512 * 64, 256)
    (tmp_path / "past_end.gguf").write_bytes(bytes(b))
    assert probe(str(tmp_path / "past_end.gguf")) == 3004
    b = bytearray(raw)
    struct.pack_into("<QQ", b, dims_at, 1 << 63, 4)        # element count wraps
    (tmp_path / "wrap.gguf").write_bytes(bytes(b))
    assert probe(str(tmp_path / "wrap.gguf")) == 3004
    b = bytearray(raw)
    assert struct.unpack_from("<QQ", b, dims_at) == (cfg.d_ff, cfg.d_model)
    # K = d_ff - 32: whole 32-blocks, K % 256 = 224.  The reader sizes a tensor in blocks of its own type and this one lies inside the file,
    # so the reader passes it; that K must be a multiple of 256 is the loader's check (tests/test_q4_1_q5_1_gpu.py).  One block more than the
    # file holds (the last tensor, K = d_ff + 32) is the reader's to refuse
    struct.pack_into("<QQ", b, dims_at, cfg.d_ff - 32, cfg.d_model)
    (tmp_path / "k_not_256.gguf").write_bytes(bytes(b))
    assert probe(str(tmp_path / "k_not_256.gguf")) == 0
    name = G._s("blk.1.ffn_down.weight")
    b = bytearray(raw)
    struct.pack_into("<QQ", b, raw.index(name) + len(name) + 4, cfg.d_ff + 32, cfg.d_model)
    (tmp_path / "k_not_256_long.gguf").write_bytes(bytes(b))
    assert probe(str(tmp_path / "k_not_256_long.gguf")) == 3004


def test_gguf_of_q4_0_with_a_q4_1_ffn_down_passes_the_probe(tmp_path):
    """the importance-matrix mix: a Q4_0 file whose blk.0.ffn_down is Q4_1 — each tensor is sized by its own type"""
    src, cfg = source(2, down0=R.Q4_1)
    p = str(tmp_path / "mix.gguf")
    G.write_llama_gguf(p, src, cfg)
    raw = bytearray(open(p, "rb").read())
    assert (type_of(raw, "blk.0.ffn_down.weight"), type_of(raw, "blk.1.ffn_down.weight"), type_of(raw, "blk.0.ffn_up.weight")) == (R.Q4_1, 2, 2)
    assert probe(p) == 0
    # the last tensor, blk.1.ffn_down, is Q4_0: 18 bytes per block.  Claimed as Q4_1 (20 per block) its data runs past the end of the file
    name = G._s("blk.1.ffn_down.weight")
    at = raw.index(name) + len(name)
    ndim = struct.unpack_from("<I", raw, at)[0]
    b = bytearray(raw)
    struct.pack_into("<I", b, at + 4 + 8 * ndim, R.Q4_1)                 # 20 bytes per block claimed, 18 present
    (tmp_path / "claims_q4_1.gguf").write_bytes(bytes(b))
    assert probe(str(tmp_path / "claims_q4_1.gguf")) == 3004
