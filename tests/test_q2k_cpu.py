"""CPU: Q2_K (GGML type 10) — the NumPy codec against a hand-written block, the Q4_K and Q6_K twins and the restated dot contract against
the oracle, the host quantiser entry (tk_mi355x_quantize_blocks_q2k) and the GGUF reader's size checks for the type."""
import ctypes as C
import struct

import numpy as np
import pytest

import gguf_util as G
import oracle_lib as O
import q2k_ref as R


def probe(path):
    import trackiellm_amd as tk
    hp = tk.LlmHParams()
    nv = C.c_int32(0)
    return tk.lib().tk_mi355x_gguf_probe(path.encode(), C.byref(hp), C.byref(nv))


def hand_block():
    """bytes: scales 0..15, qs 16..79, d 80..81, dmin 82..83.  Every field carries a value whose neighbours would give another result"""
    b = np.zeros(84, np.uint8)
    b[0] = 0x21          # group 0: scale 1, min 2
    b[1] = 0x0F          # group 1: scale 15, min 0
    b[2] = 0xF3          # group 2 (weights 32..47): scale 3, min 15
    b[8] = 0x45          # group 8 (weights 128..143): scale 5, min 4
    b[15] = 0x97         # group 15 (weights 240..255): scale 7, min 9
    b[16 + 0] = 0xE4     # qs[0]: weights 0, 32, 64, 96 = 0, 1, 2, 3
    b[16 + 16] = 0x03    # qs[16]: weight 16 (group 1) = 3
    b[16 + 32] = 0x1B    # qs[32]: weights 128, 160, 192, 224 = 3, 2, 1, 0
    b[16 + 63] = 0xC0    # qs[63]: weight 255 = 3
    b[80:82] = np.array([0.5], np.float16).view(np.uint8)
    b[82:84] = np.array([0.25], np.float16).view(np.uint8)
    return b


def test_codec_decodes_hand_written_block():
    b = hand_block()
    q = R.quants(b)[0]
    assert [int(q[i]) for i in (0, 32, 64, 96, 16, 128, 160, 192, 224, 255, 1)] == [0, 1, 2, 3, 3, 3, 2, 1, 0, 3, 0]
    assert [int(v) for v in R.scales(b)[0]] == [1, 15, 3, 0, 0, 0, 0, 0, 5, 0, 0, 0, 0, 0, 0, 7]
    assert [int(v) for v in R.mins(b)[0]] == [2, 0, 15, 0, 0, 0, 0, 0, 4, 0, 0, 0, 0, 0, 0, 9]
    assert (R.d_of(b)[0], R.dmin_of(b)[0]) == (0.5, 0.25)
    w = R.dequant(b)[0]
    # w = 0.5 sc q - 0.25 m
    want = {0: -0.5, 1: -0.5, 16: 22.5, 32: 1.5 - 3.75, 33: -3.75, 64: 0.0, 128: 7.5 - 1.0, 129: -1.0, 255: 10.5 - 2.25, 254: -2.25}
    for i, v in want.items():
        assert w[i] == v, (i, w[i], v)
    assert np.array_equal(R.make_block(q, R.scales(b)[0], R.mins(b)[0], 0.5, 0.25), b)


def random_q2k(rng, n):
    """n Q2_K blocks with every field random and d, dmin of both signs"""
    b = rng.integers(0, 256, (n, 84), dtype=np.uint8)
    b[:, 80:82] = (rng.uniform(1e-3, 1e-2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float16).view(np.uint8).reshape(n, 2)
    b[:, 82:84] = (rng.uniform(1e-3, 1e-2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float16).view(np.uint8).reshape(n, 2)
    return b


def twinable(rng, rows, nb):
    """(paired-group blocks, dmin = +0 blocks), [rows][nb] each, random otherwise"""
    p = R.pair_groups(random_q2k(rng, rows * nb))
    z = random_q2k(rng, rows * nb)
    z[:, 82:84] = 0
    return p, z


def activations(rng, n, K):
    """rows whose Q8_K scales take both signs (the oracle's scale carries the sign of the largest-magnitude value), one with an all-zero
    block"""
    x = rng.standard_normal((n, K)).astype(np.float32)
    x[0, 256:512] = 0.0
    x[1, 0] = -7.0
    x[2, 0] = 7.0
    return x


def q8_rows(x):
    qs, ds, _ = zip(*[O.q8k_quantize(r) for r in x])
    return np.stack(qs), np.stack(ds)


def test_twins_dequantise_to_the_same_bits_in_the_oracle():
    rng = np.random.default_rng(41)
    rows, nb = 64, 7
    p, z = twinable(rng, rows, nb)
    got = O.dequant_rows(O.TYPE_Q4_K, R.to_q4k(p), rows, nb * 256)
    assert np.array_equal(got.view(np.uint32), R.dequant(p).reshape(rows, nb * 256).view(np.uint32))
    got = O.dequant_rows(O.TYPE_Q6_K, R.to_q6k(z), rows, nb * 256)
    assert np.array_equal(got.view(np.uint32), R.dequant(z).reshape(rows, nb * 256).view(np.uint32))
    assert (R.quants(p).min(), R.quants(p).max(), R.scales(z).min(), R.scales(z).max(), R.mins(p).max()) == (0, 3, 0, 15, 15)


@pytest.mark.parametrize("ks", [1, 7])
def test_restated_contract_equals_the_oracle_on_both_twins(ks):
    """q2k_ref.gemv on twin-able Q2_K blocks is oracle_lib.gemv_q8 on their Q4_K / Q6_K twins, bit for bit: the restatement the GPU tests
    hold general blocks against is the oracle's contract"""
    rng = np.random.default_rng(42)
    rows, K = 64, 1792
    p, z = twinable(rng, rows, K // 256)
    x = activations(rng, 6, K)
    q8, d8 = q8_rows(x)
    assert (d8 < 0).any() and (d8 > 0).any() and (d8 == 0).any()
    for blocks, ttype, twin in ((p, O.TYPE_Q4_K, R.to_q4k(p)), (z, O.TYPE_Q6_K, R.to_q6k(z))):
        want = np.stack([O.gemv_q8(ttype, twin, rows, K, ks, r) for r in x])
        got = R.gemv(blocks, rows, K, ks, q8, d8)
        assert np.isfinite(want).all()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (ttype, ks, np.abs(got - want).max())


def quantiser_inputs():
    rng = np.random.default_rng(43)
    x = {"normal": (rng.standard_normal((64, 256)) * 0.02).astype(np.float32)}
    x["positive"] = np.abs(rng.standard_normal((16, 256)) * 0.02).astype(np.float32) + 0.01   # min clamps to 0
    x["negative"] = -x["positive"]
    o = (rng.standard_normal((16, 256)) * 0.01).astype(np.float32)
    o[:, ::16] = rng.choice([-1.0, 1.0], (16, 16)).astype(np.float32) * rng.uniform(0.5, 4.0, (16, 16)).astype(np.float32)
    x["one outlier per group"] = o
    x["all equal"] = np.repeat(np.array([[0.37], [-0.37], [1e-2], [-250.0]], np.float32), 256, axis=1)
    x["all zero"] = np.zeros((2, 256), np.float32)
    return x


def test_host_quantiser_error_bound_per_block():
    """the host Q2_K quantiser (tk.quantize_blocks(10, ...) = tk_mi355x_quantize_blocks_q2k): decode(quantise(x)) stays within the bound the block's own fields imply, per group.

    Construction (tk_quantize_q2_K): per group g of 16, lo = min(x, 0), hi = max(x); the real step is t = (hi - lo) / 3 and the real min
    is -lo.  The block stores sc = rint(t / d) and m = rint(-lo / dmin) as 4-bit integers, d and dmin being f16, so the realised step
    e = d sc and min ml = dmin m satisfy |e - t| <= d / 2 and |ml + lo| <= dmin / 2 (no clamp bites: d >= max t / 15 up to f16 rounding,
    which the factor below covers).  q = rint((x + ml) / e) clamped to 0..3.  With u = x + ml in [-dmin/2, 3 t + dmin/2]:
      * inside 0..3 the rounding error is e / 2;
      * below 0 (u < 0): at most dmin / 2; above 3 e: u - 3 e <= 3 (t - e) + dmin / 2 <= 1.5 d + dmin / 2.
    Every case is below  e / 2 + 1.5 d + dmin / 2  — half a step, plus the scale and min rounding.  sc = 0 (t < d / 2): every weight
    decodes to -ml, error <= 3 t + dmin / 2 < 1.5 d + dmin / 2, inside the same bound.  f16 rounding of d and dmin (relative 2^-11, times 15
    levels, times 3 for the clipped case: 45 * 2^-11 d < 1.5 d * 2^-5) and the f32 operations are covered by a factor 1 + 2^-5."""
    import trackiellm_amd as tk
    for name, x in quantiser_inputs().items():
        b = tk.quantize_blocks(tk.TYPE_Q2_K, x)
        assert b.shape == (x.shape[0], 84)
        w = R.dequant(b).astype(np.float64)
        d, dmin = R.d_of(b).astype(np.float64), R.dmin_of(b).astype(np.float64)
        assert (d >= 0).all() and (dmin >= 0).all()
        e = d[:, None] * R.scales(b)                                                    # (n, 16)
        bound = (e / 2 + 1.5 * d[:, None] + dmin[:, None] / 2) * (1 + 2.0 ** -5)
        err = np.abs(w - x).reshape(-1, 16, 16).max(axis=2)
        for blk in range(x.shape[0]):
            assert (err[blk] <= bound[blk]).all(), (name, blk, err[blk].max(), bound[blk])
        if name == "all zero":
            assert not b.any()
        if name == "positive":
            assert not R.mins(b).any() and not dmin.any()
    x = quantiser_inputs()["normal"]
    assert np.array_equal(tk.quantize_blocks(tk.TYPE_Q2_K, x), tk.quantize_blocks(tk.TYPE_Q2_K, x.copy()))
    assert (tk.TYPE_Q2_K, tk.FTYPE_Q2_K, tk.FTYPE_Q2_K_S, tk.llm.BLOCK_BYTES[10]) == (10, 10, 21, 84)


def test_quantize_blocks_refuses_bad_arguments():
    """null pointers and a negative count are refused; tk_mi355x_quantize_blocks keeps its own set of types (type 10 stays an invalid
    argument there, as tests/test_q3k_cpu.py pins it): Q2_K has the entry of its own"""
    import trackiellm_amd as tk
    fn = tk.lib().tk_mi355x_quantize_blocks_q2k
    fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    x = np.zeros(256, np.float32)
    out = np.zeros(256, np.uint8)
    xp, op = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert fn(xp, 1, op) == 0
    assert fn(xp, 0, op) == 0
    assert fn(None, 1, op) != 0
    assert fn(xp, 1, None) != 0
    assert fn(xp, -1, op) != 0
    old = tk.lib().tk_mi355x_quantize_blocks
    old.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    for bad in (9, 10, 15, 2, 0):
        assert old(bad, xp, 1, op) != 0
    with pytest.raises(KeyError):
        tk.quantize_blocks(9, x)


def q2k_gguf(path):
    """a tiny llama GGUF in the Q2_K pattern: Q2_K matrices and token_embd beside Q4_K / Q6_K tensors"""
    import trackiellm_amd as tk
    cfg = O.tiny_config()
    orc = O.OracleLlm(cfg, seed=4)

    D, FF = cfg.d_model, cfg.d_ff
    shape = {1: (cfg.n_head * cfg.head_dim, D), 2: (cfg.n_kv_head * cfg.head_dim, D), 6: (FF, D), 7: (FF, D), 8: (D, FF)}

    class Q2(object):
        def get_tensor(self, layer, which):
            t, buf = orc.get_tensor(layer, which)
            if (layer < 0 and which == 0) or (layer >= 0 and which in shape):   # v, o and output keep the oracle's Q4_K / Q6_K
                w = orc.dequant(layer, which, *((cfg.vocab, D) if layer < 0 else shape[which]))
                return 10, tk.quantize_blocks(tk.TYPE_Q2_K, w).reshape(-1)
            return t, buf
    G.write_llama_gguf(path, Q2(), cfg)


def test_gguf_with_q2k_tensors_passes_the_probe(tmp_path):
    p = str(tmp_path / "q2k.gguf")
    q2k_gguf(p)
    raw = open(p, "rb").read()
    name = G._s("blk.0.ffn_down.weight")
    at = raw.index(name) + len(name)
    assert struct.unpack_from("<I", raw, at + 4 + 16)[0] == 10
    assert probe(p) == 0


def test_gguf_reader_refuses_short_q2k_data(tmp_path):
    p = str(tmp_path / "short.gguf")
    q2k_gguf(p)
    raw = bytearray(open(p, "rb").read())
    # the last tensor of the file is blk.1.ffn_down, Q2_K: a file that ends one 84-byte block early is refused
    name = G._s("blk.1.ffn_down.weight")
    at = raw.index(name) + len(name)
    assert struct.unpack_from("<I", raw, at + 4 + 16)[0] == 10
    (tmp_path / "one_short.gguf").write_bytes(bytes(raw[:-84]))
    assert probe(str(tmp_path / "one_short.gguf")) == 3004
    # layer 0's ffn_down claims a K that runs past the end of the file
    name = G._s("blk.0.ffn_down.weight")
    at = raw.index(name) + len(name)
    dims_at, type_at = at + 4, at + 4 + 16
    assert struct.unpack_from("<I", raw, type_at)[0] == 10
    b = bytearray(raw)
    struct.pack_into("<QQ", b, dims_at, 512 * 64, 256)
    (tmp_path / "short_q2k.gguf").write_bytes(bytes(b))
    assert probe(str(tmp_path / "short_q2k.gguf")) == 3004
    b = bytearray(raw)
    struct.pack_into("<QQ", b, dims_at, 1 << 63, 4)       # element count wraps
    (tmp_path / "wrap_q2k.gguf").write_bytes(bytes(b))
    assert probe(str(tmp_path / "wrap_q2k.gguf")) == 3004
