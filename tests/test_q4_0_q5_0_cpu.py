"""CPU: Q4_0 and Q5_0 (GGML types 2 and 6) — the constants, the NumPy codecs against the formula written out by hand, the host quantiser
entries against the NumPy quantisers byte for byte, the round-trip bound, the refused arguments, the restated dot contract against the
oracle on Q6_K twins, and the GGUF reader's size checks for files of the two types."""
import ctypes as C
import struct

import numpy as np
import pytest

import gguf_util as G
import oracle_lib as O
import q4_0_ref as R
import q8_0_ref as Q8

TYPES = [R.Q4_0, R.Q5_0]


@pytest.fixture(autouse=True)
def restated_types_are_the_librarys():
    """every test of this file restates types the library has to know: the restatement's type ids and block sizes are the library's"""
    import trackiellm_amd as tk
    assert {tk.TYPE_Q4_0: tk.llm.BLOCK_BYTES[tk.TYPE_Q4_0], tk.TYPE_Q5_0: tk.llm.BLOCK_BYTES[tk.TYPE_Q5_0]} == R.BYTES


def probe(path):
    import trackiellm_amd as tk
    hp = tk.LlmHParams()
    nv = C.c_int32(0)
    return tk.lib().tk_mi355x_gguf_probe(path.encode(), C.byref(hp), C.byref(nv))


def test_constants_and_struct_sizes():
    import trackiellm_amd as tk
    assert (tk.TYPE_Q4_0, tk.TYPE_Q5_0, tk.FTYPE_Q4_0, tk.FTYPE_Q5_0) == (2, 6, 2, 8)
    assert (tk.llm.BLOCK_BYTES[2], tk.llm.BLOCK_BYTES[6]) == (18, 22)
    # the entries write exactly 18 / 22 bytes per block: the bytes after the last block stay as they were
    x = np.ones((3, 32), np.float32)
    for t, nb in ((2, 18), (6, 22)):
        fn = getattr(tk.lib(), "tk_mi355x_quantize_blocks_q4_0" if t == 2 else "tk_mi355x_quantize_blocks_q5_0")
        fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        out = np.full(3 * nb + 8, 0xA5, np.uint8)
        assert fn(x.ctypes.data_as(C.c_void_p), 3, out.ctypes.data_as(C.c_void_p)) == 0
        assert (out[3 * nb:] == 0xA5).all() and not (out[:3 * nb] == 0xA5).all()


@pytest.mark.parametrize("ttype", TYPES)
def test_dequant_equals_the_hand_formula_on_random_bytes(ttype):
    """every byte of the block random, so every nibble and every qh bit position is distinguished; the formula of the format description
    written out per weight in Python integers"""
    rng = np.random.default_rng(40 + ttype)
    n = 64
    b = rng.integers(0, 256, (n, R.BYTES[ttype]), dtype=np.uint8)
    b[:, 0:2] = (rng.uniform(1e-3, 1e-2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float16).view(np.uint8).reshape(n, 2)
    got_q, got_w = R.quants(ttype, b), R.dequant(ttype, b)
    for i in range(n):
        raw = bytes(b[i])
        d = np.float32(np.frombuffer(raw[0:2], np.float16)[0])
        if ttype == R.Q4_0:
            qs = raw[2:18]
            q = [qs[j] & 15 for j in range(16)] + [qs[j] >> 4 for j in range(16)]
            z = 8
        else:
            qh = struct.unpack("<I", raw[2:6])[0]
            qs = raw[6:22]
            q = [(qs[j] & 15) | (((qh >> j) & 1) << 4) for j in range(16)] + [(qs[j] >> 4) | (((qh >> (j + 16)) & 1) << 4) for j in range(16)]
            z = 16
        assert [int(v) for v in got_q[i]] == q
        want = np.array([d * np.float32(v - z) for v in q], np.float32)
        assert np.array_equal(got_w[i].view(np.uint32), want.view(np.uint32))
    # the codec round-trips, and the Q8_0 twin decodes to the same bits
    assert np.array_equal(R.make_blocks(ttype, got_q, R.d_bits(ttype, b)), b)
    assert np.array_equal(Q8.dequant(R.to_q8_0(ttype, b)).view(np.uint32), got_w.view(np.uint32))
    # single qh bits and single nibbles, by hand
    if ttype == R.Q5_0:
        for bit in range(32):
            one = np.zeros(22, np.uint8)
            one[0:2] = np.array([1.0], np.float16).view(np.uint8)
            one[2:6] = np.array([1 << bit], "<u4").view(np.uint8)
            w = R.dequant(ttype, one)[0]
            assert w[bit] == 0.0 and (np.delete(w, bit) == -16.0).all()
    one = np.zeros(R.BYTES[ttype], np.uint8)
    one[0:2] = np.array([1.0], np.float16).view(np.uint8)
    one[R.QS_AT[ttype] + 3] = 0xC5                                       # weight 3 = 5, weight 19 = 12
    w = R.dequant(ttype, one)[0] + R.Z[ttype]
    assert w[3] == 5 and w[19] == 12 and w.sum() == 17


def quantiser_inputs(ttype):
    z = R.Z[ttype]
    rng = np.random.default_rng(50 + ttype)
    x = [(rng.standard_normal((256, 32)) * 0.02).astype(np.float32), rng.standard_normal((64, 32)).astype(np.float32) * 1e4,
         (rng.standard_normal((64, 32)) * 1e-4).astype(np.float32), np.zeros((2, 32), np.float32), np.full((2, 32), -0.37, np.float32)]
    t = (rng.standard_normal((8, 32)) * 0.1).astype(np.float32)         # +- ties for the maximum: the first one wins
    t[0:4, 3], t[0:4, 20] = 3.0, -3.0
    t[4:8, 3], t[4:8, 20] = -3.0, 3.0
    x.append(t)
    m = (rng.standard_normal((8, 32)) * 0.1).astype(np.float32)         # a maximum of each sign, first and last position
    m[0, 0], m[1, 0], m[2, 31], m[3, 31] = 5.0, -5.0, 5.0, -5.0
    x.append(m)
    h = rng.integers(-z, z, (64, 32)).astype(np.float32) + 0.5          # d = 1, id = 1: x id + z + 0.5 lands on integers
    h[:, 0] = -z
    x.append(h)
    h2 = h.copy()                                                        # ... and d = -1 (max = +z): x id = -x
    h2[:, 0] = z
    x.append(h2)
    h3 = (h * np.float32(0.75)).astype(np.float32)                       # id = fl(1 / 0.75) is inexact: products beside a half
    x.append(h3)
    return np.concatenate(x)


@pytest.mark.parametrize("ttype", TYPES)
def test_host_quantiser_equals_the_numpy_quantiser_byte_for_byte(ttype):
    import trackiellm_amd as tk
    x = quantiser_inputs(ttype)
    got = tk.quantize_blocks(ttype, x)
    assert got.shape == (x.shape[0], R.BYTES[ttype]) and got.dtype == np.uint8
    want = R.quantize(ttype, x)
    bad = np.argwhere((got != want).any(axis=1))
    assert bad.size == 0, (bad[:4].tolist(), got[bad[0, 0]], want[bad[0, 0]])
    z = R.Z[ttype]
    # all-zero blocks: d = 0 / -z = -0 (f16 0x8000, as ggml stores it), id = 0, every q = (int)(z + 0.5) = z: every weight decodes to 0
    zero = R.quantize(ttype, np.zeros(32, np.float32))
    assert (R.d_bits(ttype, zero) == 0x8000).all() and (R.quants(ttype, zero) == z).all() and not R.dequant(ttype, zero).any()
    # ties: the first of +3 / -3 is the maximum, so d = -+3 / z, and the element of the other sign clips at 2 z - 1
    t = np.zeros((2, 32), np.float32)
    t[0, 3], t[0, 20], t[1, 3], t[1, 20] = 3.0, -3.0, -3.0, 3.0
    tb = R.quantize(ttype, t)
    assert [float(v) for v in R.d_of(ttype, tb)] == [float(np.float16(-3.0 / z)), float(np.float16(3.0 / z))]
    q = R.quants(ttype, tb)
    assert (q[0, 3], q[0, 20], q[1, 3], q[1, 20]) == (0, 2 * z - 1, 0, 2 * z - 1)
    # halves: with d = 1 the sum x + z + 0.5 is an integer and truncation keeps it: q = x + z + 0.5, the top one clipped
    h = np.zeros(32, np.float32)
    h[0], h[1], h[2], h[3] = -z, -0.5, 0.5, z - 0.5
    assert [int(v) for v in R.quants(ttype, R.quantize(ttype, h))[0, :5]] == [0, z, z + 1, 2 * z - 1, z]
    # a row of 256 n weights is n / 32 blocks, in order
    assert np.array_equal(tk.quantize_blocks(ttype, x[:16].reshape(2, 256)), want[:16])


@pytest.mark.parametrize("ttype", TYPES)
def test_decode_of_quantise_stays_within_the_bound_of_the_construction(ttype):
    """A bound, not a measurement.  M = the block's element of largest magnitude, d = -M / z (unrounded), dh = f16(d), id = fl(1 / d).
      * an element with x / d < z - 0.5 is not clipped: q - z = trunc(x id + z + 0.5) - z is x / d rounded to an integer up to the two
        binary32 roundings of the sum, so |x - d (q - z)| <= (0.5 + z 2^-21) |d|;
      * an element with x / d >= z - 0.5 (the one opposite the maximum, x = -M, among them: x / d = z) is clipped to q = 2 z - 1, so
        |x - d (q - z)| <= |d| there;
      * the stored scale: |dh - d| <= 2^-11 |d| for a normal f16 (|d| >= 2^-14, true of this data), times |q - z| <= z.
    Together |x - dh (q - z)| <= (1 + z 2^-11 + z 2^-21) |d|.  (A sample of the construction gave 1.0008 |d| for Q4_0.)"""
    z = R.Z[ttype]
    rng = np.random.default_rng(60 + ttype)
    x = np.concatenate([(rng.standard_normal((4096, 32)) * 0.02).astype(np.float32), rng.standard_normal((512, 32)).astype(np.float32)])
    x[:64, 7] = -x[np.arange(64), np.abs(x[:64]).argmax(axis=1)]         # an element exactly opposite the maximum
    b = R.quantize(ttype, x)
    w = R.dequant(ttype, b).astype(np.float64)
    d = np.abs(x).max(axis=1).astype(np.float64) / z
    assert (d >= 2.0 ** -14).all()
    err = np.abs(x.astype(np.float64) - w) / d[:, None]
    bound = 1.0 + z * 2.0 ** -11 + z * 2.0 ** -21
    print(f"type {ttype}: largest |x - w| / |d| = {err.max():.6f}, bound {bound:.6f}")
    assert err.max() <= bound
    assert err.max() > 0.9                                               # the clipped element is in the sample
    q = R.quants(ttype, b)
    free = q < 2 * z - 1
    assert (err[free] <= 0.5 + z * 2.0 ** -11 + z * 2.0 ** -21).all()


def test_refused_arguments():
    import trackiellm_amd as tk
    x = np.zeros(256, np.float32)
    out = np.zeros(8 * 34, np.uint8)
    xp, op = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for name in ("tk_mi355x_quantize_blocks_q4_0", "tk_mi355x_quantize_blocks_q5_0"):
        fn = getattr(tk.lib(), name)
        fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        assert fn(xp, 8, op) == 0 and fn(xp, 0, op) == 0
        assert fn(None, 1, op) != 0 and fn(xp, 1, None) != 0 and fn(xp, -1, op) != 0
    old = tk.lib().tk_mi355x_quantize_blocks
    old.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    for bad in (2, 6):
        assert old(bad, xp, 1, op) != 0


def activations(rng, n, K):
    x = rng.standard_normal((n, K)).astype(np.float32)
    x[0, 256:512] = 0.0
    x[1, 0] = -7.0
    x[2, 0] = 7.0
    return x


def q8_rows(x):
    qs, ds, _ = zip(*[O.q8k_quantize(r) for r in x])
    return np.stack(qs), np.stack(ds).reshape(len(x), -1)


@pytest.mark.parametrize("ks", [1, 7])
@pytest.mark.parametrize("ttype", TYPES)
def test_restated_contract_equals_the_oracle_on_twin_rows(ttype, ks):
    """q4_0_ref.gemv on twin-sparse rows is oracle_lib.gemv_q8 on their Q6_K twins, bit for bit"""
    rng = np.random.default_rng(70 + ttype)
    rows, K = 64, 1792
    b = R.quantize_twin_sparse(ttype, (rng.standard_normal((rows, K)) * 0.02).astype(np.float32), seed=5)
    live = R.d_bits(ttype, b).reshape(-1, 8) != 0
    assert (live.sum(axis=1) == 1).all() and set(live.argmax(axis=1).tolist()) == set(range(8))
    dl = R.d_of(ttype, b)
    assert (dl < 0).any() and (dl > 0).any()
    ql = R.quants(ttype, b)[R.d_bits(ttype, b) != 0]
    assert ql.min() == 0 and ql.max() == 2 * R.Z[ttype] - 1             # q - z over the type's whole range
    x = activations(rng, 6, K)
    q8, d8 = q8_rows(x)
    assert (d8 < 0).any() and (d8 > 0).any() and (d8 == 0).any()
    twin = R.to_q6k(ttype, b)
    want = np.stack([O.gemv_q8(O.TYPE_Q6_K, twin, rows, K, ks, r) for r in x])
    got = R.gemv(ttype, b, rows, K, ks, q8, d8)
    assert np.isfinite(want).all() and want.any()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (ks, np.abs(got - want).max())


def all_of(ttype):
    """a tiny llama GGUF source whose every layer matrix and token_embd are `ttype` (the host quantiser's blocks), output Q6_K, norms F32"""
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
                return ttype, tk.quantize_blocks(ttype, w).reshape(-1)
            return t, buf
    return Src(), cfg


@pytest.mark.parametrize("ttype", TYPES)
def test_gguf_of_one_type_passes_the_probe_and_short_data_is_refused(tmp_path, ttype):
    """an all-Q4_0 / all-Q5_0 file (output Q6_K): the probe accepts it; a file that ends one block early, or whose ffn_down claims a K
    running past the end of the file or wrapping the element count, comes back 3004"""
    src, cfg = all_of(ttype)
    p = str(tmp_path / "whole.gguf")
    G.write_llama_gguf(p, src, cfg)
    raw = bytearray(open(p, "rb").read())
    for name, want in (("token_embd.weight", ttype), ("output.weight", 14), ("blk.0.attn_q.weight", ttype), ("blk.1.ffn_down.weight", ttype)):
        at = raw.index(G._s(name)) + len(G._s(name))
        ndim = struct.unpack_from("<I", raw, at)[0]
        assert struct.unpack_from("<I", raw, at + 4 + 8 * ndim)[0] == want, name
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
