"""CPU: Q3_K (GGML type 11) — the NumPy codec against a hand-computed block, the Q6_K twin against the oracle's Q6_K decode, the host
quantiser entry (tk_mi355x_quantize_blocks) and the GGUF reader's size checks for the type."""
import ctypes as C
import struct

import numpy as np

import gguf_util as G
import oracle_lib as O
import q3k_ref as R


def probe(path):
    import trackiellm_amd as tk
    hp = tk.LlmHParams()
    nv = C.c_int32(0)
    return tk.lib().tk_mi355x_gguf_probe(path.encode(), C.byref(hp), C.byref(nv))


def hand_block():
    """bytes: hmask 0..31, qs 32..95, scales 96..107, d 108..109.  Every field carries a value whose neighbours would give another result"""
    b = np.zeros(110, np.uint8)
    b[0] = 0xA5          # hmask[0]: high bits of weights 0, 64 (bits 0, 2) and 160, 224 (bits 5, 7); clear for 32, 96, 128, 192
    b[31] = 0x80         # hmask[31]: weight 255
    b[32 + 0] = 0xE4     # qs[0]: weights 0, 32, 64, 96 low = 0, 1, 2, 3
    b[32 + 32] = 0x1B    # qs[32]: weights 128, 160, 192, 224 low = 3, 2, 1, 0
    b[32 + 63] = 0xC0    # qs[63]: weight 255 low = 3
    b[96 + 0] = 0xF7     # low 4 bits: group 0 = 7, group 8 = 15
    b[96 + 1] = 0x01     # group 1 = 1, group 9 = 0
    b[96 + 2] = 0x05     # group 2 = 5, group 10 = 0
    b[96 + 4] = 0x30     # group 4 = 0, group 12 = 3
    b[96 + 6] = 0x9C     # group 6 = 12, group 14 = 9
    b[96 + 7] = 0xA0     # group 7 = 0, group 15 = 10
    b[96 + 8] = 0x9C     # high 2 bits of groups 0, 4, 8, 12 = 0, 3, 1, 2
    b[96 + 9] = 0x02     # groups 1, 5, 9, 13 = 2, 0, 0, 0
    b[96 + 10] = 0x72    # groups 2, 6, 10, 14 = 2, 0, 3, 1
    b[96 + 11] = 0xC0    # groups 3, 7, 11, 15 = 0, 0, 0, 3
    b[108:110] = np.array([0.5], np.float16).view(np.uint8)
    return b


def test_codec_decodes_hand_computed_block():
    b = hand_block()
    q = R.quants(b)[0]
    assert [int(q[i]) for i in (0, 32, 64, 96, 128, 160, 192, 224, 255, 1, 16)] == [0, -3, 2, -1, -1, 2, -3, 0, 3, -4, -4]
    s = R.scales(b)[0]
    assert [int(v) for v in s] == [-25, 1, 5, -32, 16, -32, -20, -32, -1, -32, 16, -32, 3, -32, -7, 26]
    w = R.dequant(b)[0]
    want = {0: 0.0, 1: 50.0, 16: -2.0, 32: -7.5, 64: 16.0, 96: 10.0, 112: 64.0, 128: 0.5, 160: 16.0, 192: -4.5, 224: 0.0, 255: 39.0}
    for i, v in want.items():
        assert w[i] == v, (i, w[i], v)
    assert np.array_equal(R.make_block(q, s, 0.5), b)


def random_q3k(rng, n):
    """n Q3_K blocks with every field random and d of both signs"""
    b = rng.integers(0, 256, (n, 110), dtype=np.uint8)
    b[:, 108:110] = (rng.uniform(1e-3, 1e-2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float16).view(np.uint8).reshape(n, 2)
    return b


def test_q6k_twin_dequantises_to_the_same_bits_in_the_oracle():
    """the oracle's Q6_K decode of q3k_to_q6k(b) is the NumPy Q3_K decode of b, bit for bit, on random-byte blocks"""
    rng = np.random.default_rng(31)
    rows, nb = 64, 48
    b = random_q3k(rng, rows * nb)
    got = O.dequant_rows(O.TYPE_Q6_K, R.q3k_to_q6k(b), rows, nb * 256)
    want = R.dequant(b).reshape(rows, nb * 256)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (R.quants(b).min(), R.quants(b).max(), R.scales(b).min(), R.scales(b).max()) == (-4, 3, -32, 31)


def quantiser_inputs():
    rng = np.random.default_rng(32)
    x = {"normal": (rng.standard_normal((64, 256)) * 0.02).astype(np.float32)}
    o = (rng.standard_normal((16, 256)) * 0.01).astype(np.float32)
    o[:, ::16] = rng.choice([-1.0, 1.0], (16, 16)).astype(np.float32) * rng.uniform(0.5, 4.0, (16, 16)).astype(np.float32)
    x["one outlier per group"] = o
    x["all equal"] = np.repeat(np.array([[0.37], [-0.37], [1e-2], [-250.0]], np.float32), 256, axis=1)
    x["all zero"] = np.zeros((2, 256), np.float32)
    m = (rng.standard_normal((16, 256)) * 0.3).astype(np.float32)
    m[:, 0::16] = 1.0
    m[:, 1::16] = -1.0          # the group maximum occurs with both signs: the first one decides the scale's sign
    m[8:, 0::16] = -1.0
    m[8:, 1::16] = 1.0
    x["sign-mixed maxima"] = m
    return x


def test_host_quantiser_error_bound_per_block():
    """tk_mi355x_quantize_blocks(11, ...): decode(quantise(x)) stays within the bound of the construction, asserted per weight of every
    block.

    Construction (tk_quantize_q3_K): per group g of 16, a = max |x| and the real group scale t_g = -x_max / 4, so the step is a / 4 (eight
    levels -4..3, the largest weight on -4).  d = max_g |t_g| / 31 rounded to f16 (dq); the stored scale is s_g = rint(t_g / dq), a 6-bit
    integer, so |dq s_g - t_g| <= dq / 2; q = rint(x / (dq s_g)) clamped to -4..3.
    Error of one weight, with e = dq |s_g| the realised step (a/4 - dq/2 <= e <= a/4 + dq/2):
      * rounding inside the range: e / 2 <= a/8 + dq/4;
      * clipping at +3 (the range is asymmetric: a weight near -x_max wants level +4): at most a - 3 e <= a/4 + 1.5 dq;
      * clipping at -4 when the scale was rounded down: at most a - 4 e <= 2 dq;
      * s_g = 0 (|t_g| < dq / 2): every weight of the group decodes to 0, error <= a = 4 |t_g| < 2 dq.
    All four are below  a_g / 4 + 2 dq.  The f32 operations of quantiser and decode add relative 2^-22 terms, covered by a factor
    1 + 2^-10.  (f16 under- or overflow of d is outside the construction: inputs here keep d a normal f16.)"""
    import trackiellm_amd as tk
    for name, x in quantiser_inputs().items():
        b = tk.quantize_blocks(tk.TYPE_Q3_K, x)
        assert b.shape == (x.shape[0], 110)
        w = R.dequant(b)
        dq = np.abs(R.d_of(b)).astype(np.float64)
        a = np.abs(x.astype(np.float64)).reshape(-1, 16, 16).max(axis=2)                # (n, 16)
        bound = (a / 4 + 2 * dq[:, None]) * (1 + 2.0 ** -10)
        err = np.abs(w.astype(np.float64) - x).reshape(-1, 16, 16).max(axis=2)
        for blk in range(x.shape[0]):
            assert (err[blk] <= bound[blk]).all(), (name, blk, err[blk].max(), bound[blk])
        if name == "all zero":
            assert not w.any() and not R.d_of(b).any()
        if name != "all zero":
            # the largest-magnitude weight of every group sits on level -4 when its scale survived the rounding
            q, s = R.quants(b).reshape(-1, 16, 16), R.scales(b)
            first = np.abs(x).reshape(-1, 16, 16).argmax(axis=2)
            qmax = np.take_along_axis(q, first[:, :, None], axis=2)[:, :, 0]
            assert (qmax[np.abs(s) >= 4] == -4).all(), name


def test_host_quantiser_is_deterministic_and_matches_the_oracle_for_q4k_and_q6k():
    import trackiellm_amd as tk
    rng = np.random.default_rng(33)
    x = (rng.standard_normal((32, 512)) * 0.02).astype(np.float32)
    for ttype in (O.TYPE_Q4_K, O.TYPE_Q6_K):
        assert np.array_equal(tk.quantize_blocks(ttype, x).reshape(-1), O.quantize_rows(ttype, x))
    assert np.array_equal(tk.quantize_blocks(tk.TYPE_Q3_K, x), tk.quantize_blocks(tk.TYPE_Q3_K, x.copy()))
    assert tk.quantize_blocks(tk.TYPE_Q5_K, x).shape == (64, 176)
    out = np.zeros(110, np.uint8)
    rc = tk.lib().tk_mi355x_quantize_blocks(10, x.ctypes.data_as(C.c_void_p), C.c_int64(1), out.ctypes.data_as(C.c_void_p))
    assert rc != 0


def q3k_gguf(path):
    """a tiny llama GGUF in the Q3_K_M pattern: Q3_K matrices and token_embd beside Q4_K / Q6_K tensors"""
    import trackiellm_amd as tk
    cfg = O.tiny_config()
    orc = O.OracleLlm(cfg, seed=4)

    D, FF = cfg.d_model, cfg.d_ff
    shape = {1: (cfg.n_head * cfg.head_dim, D), 2: (cfg.n_kv_head * cfg.head_dim, D), 6: (FF, D), 7: (FF, D), 8: (D, FF)}

    class Q3(object):
        def get_tensor(self, layer, which):
            t, buf = orc.get_tensor(layer, which)
            if t == 12 and (layer < 0 or which in shape):
                w = orc.dequant(layer, which, *((cfg.vocab, D) if layer < 0 else shape[which]))
                return 11, tk.quantize_blocks(tk.TYPE_Q3_K, w).reshape(-1)
            return t, buf
    G.write_llama_gguf(path, Q3(), cfg)


def test_gguf_with_q3k_tensors_passes_the_probe(tmp_path):
    p = str(tmp_path / "q3k.gguf")
    q3k_gguf(p)
    assert probe(p) == 0


def test_gguf_reader_refuses_short_q3k_data(tmp_path):
    p = str(tmp_path / "short.gguf")
    q3k_gguf(p)
    raw = bytearray(open(p, "rb").read())
    # the last tensor of the file is blk.1.ffn_down; make layer 0's Q3_K ffn_down claim a K that runs past the end of the file
    name = G._s("blk.0.ffn_down.weight")
    at = raw.index(name) + len(name)
    assert struct.unpack_from("<I", raw, at)[0] == 2
    dims_at, type_at = at + 4, at + 4 + 16
    assert struct.unpack_from("<I", raw, type_at)[0] == 11
    b = bytearray(raw)
    struct.pack_into("<QQ", b, dims_at, 512 * 64, 256)   # 64x the columns: the block count times 110 B exceeds the data region
    (tmp_path / "short_q3k.gguf").write_bytes(bytes(b))
    assert probe(str(tmp_path / "short_q3k.gguf")) == 3004
    b = bytearray(raw)
    struct.pack_into("<QQ", b, dims_at, 1 << 63, 4)       # element count wraps
    (tmp_path / "wrap_q3k.gguf").write_bytes(bytes(b))
    assert probe(str(tmp_path / "wrap_q3k.gguf")) == 3004
    b = bytearray(raw)
    struct.pack_into("<QQ", b, dims_at, 1 << 40, 1 << 8)  # does not wrap, describes far more than the file holds
    (tmp_path / "huge_q3k.gguf").write_bytes(bytes(b))
    assert probe(str(tmp_path / "huge_q3k.gguf")) == 3004
