"""CPU: IQ4_NL and IQ4_XS (GGML types 20 and 23) — the constants, the NumPy codecs against the formula written out by hand, the host
quantiser entries against the NumPy quantisers byte for byte, the round-trip bound, the refused arguments, the restated dot contract
against the oracle on Q6_K twins, and the GGUF reader's size checks for files of the two types."""
import ctypes as C
import struct

import numpy as np
import pytest

import gguf_util as G
import iq4_ref as R
import oracle_lib as O
import q8_0_ref as Q8

TYPES = [R.IQ4_NL, R.IQ4_XS]
ENTRY = {R.IQ4_NL: "tk_mi355x_quantize_blocks_iq4_nl", R.IQ4_XS: "tk_mi355x_quantize_blocks_iq4_xs"}
KV = [-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113]


@pytest.fixture(autouse=True)
def restated_types_are_the_librarys():
    """every test of this file restates types the library has to know: the restatement's type ids and block sizes are the library's"""
    import trackiellm_amd as tk
    assert {tk.TYPE_IQ4_NL: tk.llm.BLOCK_BYTES[tk.TYPE_IQ4_NL], tk.TYPE_IQ4_XS: tk.llm.BLOCK_BYTES[tk.TYPE_IQ4_XS]} == R.BYTES


def probe(path):
    import trackiellm_amd as tk
    hp = tk.LlmHParams()
    nv = C.c_int32(0)
    return tk.lib().tk_mi355x_gguf_probe(path.encode(), C.byref(hp), C.byref(nv))


def test_constants_and_struct_sizes():
    import trackiellm_amd as tk
    assert (tk.TYPE_IQ4_NL, tk.TYPE_IQ4_XS, tk.FTYPE_IQ4_NL, tk.FTYPE_IQ4_XS) == (20, 23, 25, 30)
    assert (tk.llm.BLOCK_BYTES[20], tk.llm.BLOCK_BYTES[23]) == (18, 136)
    assert R.KV.tolist() == KV
    # the entries write exactly 18 / 136 bytes per block: the bytes after the last block stay as they were
    for t in TYPES:
        nb = R.BYTES[t]
        x = np.ones((3, R.ELEMS[t]), np.float32)
        fn = getattr(tk.lib(), ENTRY[t])
        fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        out = np.full(3 * nb + 8, 0xA5, np.uint8)
        assert fn(x.ctypes.data_as(C.c_void_p), 3, out.ctypes.data_as(C.c_void_p)) == 0
        assert (out[3 * nb:] == 0xA5).all() and not (out[:3 * nb] == 0xA5).all()


def hand_weights(ttype, raw):
    """the format description written out per weight in Python integers: (indices, [d, s, kv] factors) of one block"""
    d = np.float32(np.frombuffer(raw[0:2], np.float16)[0])
    if ttype == R.IQ4_NL:
        qs = raw[2:18]
        q = [qs[j] & 15 for j in range(16)] + [qs[j] >> 4 for j in range(16)]
        return q, np.array([d * np.float32(KV[v]) for v in q], np.float32)
    sh = struct.unpack("<H", raw[2:4])[0]
    sl, qs = raw[4:8], raw[8:136]
    q, w = [], []
    for j in range(8):
        ls = ((sl[j // 2] >> (4 * (j % 2))) & 15) | (((sh >> (2 * j)) & 3) << 4)
        dl = np.float32(d * np.float32(ls - 32))
        sub = [qs[16 * j + i] & 15 for i in range(16)] + [qs[16 * j + i] >> 4 for i in range(16)]
        q += sub
        w += [dl * np.float32(KV[v]) for v in sub]
    return q, np.array(w, np.float32)


@pytest.mark.parametrize("ttype", TYPES)
def test_dequant_equals_the_hand_formula_on_random_bytes(ttype):
    """every byte of the block random, so every nibble and every scales_h / scales_l bit is distinguished; plus ls = 0, 32 and 63"""
    rng = np.random.default_rng(40 + ttype)
    n = 64
    b = rng.integers(0, 256, (n, R.BYTES[ttype]), dtype=np.uint8)
    b[:, 0:2] = (rng.uniform(1e-3, 1e-2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float16).view(np.uint8).reshape(n, 2)
    if ttype == R.IQ4_XS:
        b[0, 2:8] = 0                                                    # ls = 0: s = -32
        b[1, 2:8] = 0xFF                                                 # ls = 63: s = 31
        b[2, 2:4] = np.array([0xAAAA], "<u2").view(np.uint8)             # ls = 32: s = 0
        b[2, 4:8] = 0
        assert (R.ls_of(b[:3]) == np.array([[0], [63], [32]])).all()
    got_q, got_w = R.indices(ttype, b).reshape(n, -1), R.dequant(ttype, b).reshape(n, -1)
    for i in range(n):
        q, want = hand_weights(ttype, bytes(b[i]))
        assert [int(v) for v in got_q[i]] == q
        assert np.array_equal(got_w[i].view(np.uint32), want.view(np.uint32))
    assert set(got_q.reshape(-1).tolist()) == set(range(16))
    # the codec round-trips
    ls = R.ls_of(b) if ttype == R.IQ4_XS else None
    assert np.array_equal(R.make_blocks(ttype, got_q.reshape(-1, 32), R.d_bits(ttype, b), ls), b)
    if ttype == R.IQ4_XS:
        assert set(ls.reshape(-1).tolist()) == set(range(64))
        assert not got_w[2].any() and np.array_equal(got_w[0, :32], (R.d_of(ttype, b[:1]) * np.float32(-32)) * R.KV[got_q[0, :32]].astype(np.float32))
        # every single bit of scales_h and scales_l, by hand: bit k of scales_h is bit 4 + (k & 1) of ls_{k / 2}, bit k of scales_l[m] is bit
        # k & 3 of ls_{2 m + k / 4}
        for k in range(16):
            one = np.zeros(136, np.uint8)
            one[2:4] = np.array([1 << k], "<u2").view(np.uint8)
            want = np.zeros(8, np.int64)
            want[k // 2] = 16 << (k & 1)
            assert np.array_equal(R.ls_of(one)[0], want)
        for m in range(4):
            for k in range(8):
                one = np.zeros(136, np.uint8)
                one[4 + m] = 1 << k
                want = np.zeros(8, np.int64)
                want[2 * m + k // 4] = 1 << (k & 3)
                assert np.array_equal(R.ls_of(one)[0], want)
    # the Q8_0 twin (where D is an f16: every IQ4_NL block) decodes to the same bits
    ok = R.q8_0_twinable(ttype, b)
    assert ok.all() if ttype == R.IQ4_NL else ok.any()
    sub = b if ttype == R.IQ4_NL else b[ok.reshape(n, 8).all(axis=1)]
    if len(sub):
        assert np.array_equal(Q8.dequant(R.to_q8_0(ttype, sub)).view(np.uint32), R.dequant(ttype, sub).view(np.uint32))
    # single nibbles, by hand
    one = np.zeros(R.BYTES[ttype], np.uint8)
    one[0:2] = np.array([1.0], np.float16).view(np.uint8)
    one[2:R.QS_AT[ttype]] = [0xFF, 0xFF, 0x33, 0x33, 0x33, 0x33][:R.QS_AT[ttype] - 2]   # IQ4_XS: ls = 51, s = 19
    one[R.QS_AT[ttype] + 3] = 0xC5                                      # weight 3 = kv[5], weight 19 = kv[12], the rest kv[0]
    w = R.dequant(ttype, one).reshape(-1) / (1 if ttype == R.IQ4_NL else 19)
    assert w[3] == -35 and w[19] == 53 and (np.delete(w, [3, 19]) == -127).all()


def midpoint_run(scale):
    """eight sub-blocks whose scaled values land exactly on code-book midpoints.  Sub-block 0 holds one element -127 * 31 * scale, so an
    IQ4_XS block gets d = scale exactly and s_0 = 31; sub-blocks 1..7 have the maximum -127 * scale (D = scale, s = 1, id = 1 / scale exact
    for a power of two) and the fifteen midpoints (kv[k] + kv[k + 1]) / 2 times scale, once as they are and once one ulp towards kv[k + 1]"""
    mids = ((R.KV[:-1] + R.KV[1:]) / 2.0).astype(np.float32) * np.float32(scale)
    h = np.zeros((8, 32), np.float32)
    h[0, 5] = -127.0 * 31 * scale
    h[1:, :15] = mids
    h[1:, 15:30] = np.nextafter(mids, np.float32(1e6 * scale))
    h[1:, 31] = -127.0 * scale
    return h


def quantiser_inputs(ttype):
    rng = np.random.default_rng(50 + ttype)
    x = [(rng.standard_normal((256, 32)) * 0.02).astype(np.float32), rng.standard_normal((64, 32)).astype(np.float32) * 1e4,
         (rng.standard_normal((64, 32)) * 1e-4).astype(np.float32), np.zeros((8, 32), np.float32), np.full((8, 32), -0.37, np.float32)]
    t = (rng.standard_normal((8, 32)) * 0.1).astype(np.float32)         # +- ties for the maximum: the first one wins
    t[0:4, 3], t[0:4, 20] = 3.0, -3.0
    t[4:8, 3], t[4:8, 20] = -3.0, 3.0
    x.append(t)
    m = (rng.standard_normal((8, 32)) * 0.1).astype(np.float32)         # a maximum of each sign, first and last position
    m[0, 0], m[1, 0], m[2, 31], m[3, 31] = 5.0, -5.0, 5.0, -5.0
    x.append(m)
    for scale in (1.0, 0.5, -2.0):
        x.append(midpoint_run(scale))
    x.append((rng.standard_normal((64, 32)) * np.repeat(10.0 ** rng.uniform(-4, 0, 8), 8)[:, None]).astype(np.float32))   # sub-block scales far apart
    return np.concatenate(x)


@pytest.mark.parametrize("ttype", TYPES)
def test_host_quantiser_equals_the_numpy_quantiser_byte_for_byte(ttype):
    import trackiellm_amd as tk
    x = quantiser_inputs(ttype)
    assert x.shape[0] % 8 == 0
    got = tk.quantize_blocks(ttype, x)
    assert got.shape == (x.shape[0] // R.SUBS[ttype], R.BYTES[ttype]) and got.dtype == np.uint8
    want = R.quantize(ttype, x)
    bad = np.argwhere((got != want).any(axis=1))
    assert bad.size == 0, (bad[:4].tolist(), got[bad[0, 0]], want[bad[0, 0]])
    # all-zero blocks: d = 0 / -127 = -0 (IQ4_NL stores it; IQ4_XS stores max |r| / 31 = +0), id = 0, and 0 lies between the midpoints
    # -4.5 and 7, eight midpoints below it: index 8 (kv = 1); every weight decodes to 0.  IQ4_XS: s = 0, ls = 32
    zero = R.quantize(ttype, np.zeros(256, np.float32))
    assert (R.d_bits(ttype, zero) == (0x8000 if ttype == R.IQ4_NL else 0)).all() and (R.indices(ttype, zero) == 8).all()
    assert not R.dequant(ttype, zero).any()
    if ttype == R.IQ4_XS:
        assert (R.ls_of(zero) == 32).all()
    # ties: the first of +3 / -3 is the maximum and lands on kv[0] = -127: D = -+3 / 127; the element of the other sign is x / D = 127,
    # nearest kv[15] = 113
    t = np.zeros((16, 32), np.float32)
    t[0::2, 3], t[0::2, 20], t[1::2, 3], t[1::2, 20] = 3.0, -3.0, -3.0, 3.0
    tb = R.quantize(ttype, t)
    D = R.sub_scales(ttype, tb)
    assert (D[0::2] < 0).all() and (D[1::2] > 0).all() and np.allclose(np.abs(D), 3.0 / 127, rtol=2e-3)
    q = R.indices(ttype, tb)
    assert (q[:, 3] == 0).all() and (q[:, 20] == 15).all()
    # midpoints: a scaled value exactly on (kv[k] + kv[k + 1]) / 2 is not above it: the lower index k; one ulp further: k + 1
    for scale in (1.0, 0.5, -2.0):
        hb = tk.quantize_blocks(ttype, midpoint_run(scale))
        assert np.array_equal(hb, R.quantize(ttype, midpoint_run(scale)))
        assert (R.sub_scales(ttype, hb)[1:] == np.float32(scale)).all()
        hq = R.indices(ttype, hb)[1:]
        assert (hq[:, :15] == np.arange(15)).all() and (hq[:, 15:30] == np.arange(1, 16)).all() and (hq[:, 31] == 0).all()
    # a row of 256 n weights is its blocks, in order
    assert np.array_equal(tk.quantize_blocks(ttype, x[:16].reshape(2, 256)), want[:16 // R.SUBS[ttype]])


@pytest.mark.parametrize("ttype", TYPES)
def test_decode_of_quantise_stays_within_the_bound_of_the_construction(ttype):
    """A bound, not a measurement.  Per sub-block M = the element of largest magnitude, r = -M / 127, Dl the stored sub-block scale
    (IQ4_NL: f16(r); IQ4_XS: dq s_j), idl = fl(1 / Dl from the unrounded value), v = fl(x idl).
      * The index picked is that of the code-book value nearest to v.  Inside the code book, v in [-127, 113], |v - kv[q]| is at most
        half the widest gap (89 .. 113, 24): 12.  The code book is one-sided: the element opposite the maximum has v = +127, past
        kv[15] = 113, so for v in (113, 127] the distance is up to 14.  In units of |Dl|: 12 |Dl| for elements with x / Dl <= 113,
        14 |Dl| over all.
      * IQ4_NL picks with id = 1 / r and decodes with Dl = f16(r), |Dl - r| <= 2^-11 |r| (normal f16, asserted): x / Dl and the value the
        index was picked for differ by at most 127 |Dl - r| / |Dl|, which enters twice (the pick, and which side of 113 an element is on):
        + 2 * 127 |Dl - r|, 0.125 |r| at the most.
      * IQ4_XS picks and decodes with the same Dl = dq s_j, s_j = rint(r / dq), |r| <= 31.008 dq, so |Dl - r| <= dq / 2 (asserted) and
        there is no such drift.  But where |Dl| < |r| the scaled values run past +-127, up to 127 |r| / |Dl|: below -127 the error is
        |x| - 127 |Dl| <= 127 (|r| - |Dl|), above 113 it is 14 |Dl| + 127 (|r| - |Dl|).  So the term is 127 max(0, |r| - |Dl|): nothing for a
        sub-block whose scale was rounded up, and a wrong s_j (off by one: |Dl - r| >= dq / 2 on the wrong side, or an error of order
        |Dl| for small s_j) is not covered by it.
      * binary32 roundings of idl and v: 127 * 2^-22 in v; 1e-3 |Dl| covers it.
    Sub-blocks with s_j = 0 (an IQ4_XS sub-block 62 times smaller than the block's largest) decode to 0: |x - w| <= |M| there."""
    rng = np.random.default_rng(60 + ttype)
    x = np.concatenate([(rng.standard_normal((4096, 32)) * 0.02).astype(np.float32), rng.standard_normal((512, 32)).astype(np.float32)])
    x[:64, 7] = -x[np.arange(64), np.abs(x[:64]).argmax(axis=1)]         # an element exactly opposite the maximum: x / D = 127
    b = R.quantize(ttype, x)
    w = R.dequant(ttype, b).astype(np.float64)
    Dl = R.sub_scales(ttype, b).astype(np.float64)
    M = x[np.arange(x.shape[0]), np.abs(x).argmax(axis=1)].astype(np.float64)
    r = M / -127.0
    assert (np.abs(r) >= 2.0 ** -14).all()
    live = Dl != 0
    assert live.mean() > 0.99
    err = np.abs(x.astype(np.float64) - w)
    if ttype == R.IQ4_NL:
        assert (np.abs(Dl - r) <= 2.0 ** -11 * np.abs(r)).all()
        drift = 2 * 127.0 * np.abs(Dl - r) + 1e-3 * np.abs(Dl)
    else:
        drift = 127.0 * np.maximum(0.0, np.abs(r) - np.abs(Dl)) + 1e-3 * np.abs(Dl)
        dq = np.repeat(R.d_of(ttype, b).astype(np.float64), 8)
        assert (np.abs(Dl - r)[live] <= 0.5 * dq[live] * (1 + 1e-6)).all()
    with np.errstate(all="ignore"):
        v = x.astype(np.float64) / Dl[:, None]
    inside = live[:, None] & (v <= 113.0)
    all_bound = (14.0 * np.abs(Dl) + drift)[:, None] * np.ones_like(err)
    in_bound = (12.0 * np.abs(Dl) + drift)[:, None] * np.ones_like(err)
    rel = (err / np.abs(Dl)[:, None])[live]
    print(f"type {ttype}: largest |x - w| / |Dl| = {rel.max():.4f} (inside the code book {(err / np.abs(Dl)[:, None])[inside].max():.4f})")
    assert (err[live] <= all_bound[live]).all()
    assert (err[inside] <= in_bound[inside]).all()
    assert (err[~live] <= np.abs(M)[~live, None]).all()
    assert rel.max() > 11.0                                              # the widest gap is in the sample


def test_refused_arguments():
    import trackiellm_amd as tk
    x = np.zeros(2048, np.float32)
    out = np.zeros(8 * 136, np.uint8)
    xp, op = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for name in ENTRY.values():
        fn = getattr(tk.lib(), name)
        fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        assert fn(xp, 8, op) == 0 and fn(xp, 0, op) == 0
        assert fn(None, 1, op) != 0 and fn(xp, 1, None) != 0 and fn(xp, -1, op) != 0
    old = tk.lib().tk_mi355x_quantize_blocks
    old.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    for bad in (20, 23):
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
    """iq4_ref.gemv on twin-sparse rows is oracle_lib.gemv_q8 on their Q6_K twins, bit for bit"""
    rng = np.random.default_rng(70 + ttype)
    rows, K = 64, 1792
    b = R.quantize_twin_sparse(ttype, (rng.standard_normal((rows, K)) * 0.02).astype(np.float32), seed=5)
    D = R.sub_scales(ttype, b).reshape(-1, 8)
    live = D != 0
    assert (live.sum(axis=1) == 1).all() and set(live.argmax(axis=1).tolist()) == set(range(8))
    assert (D < 0).any() and (D > 0).any()
    ql = R.indices(ttype, b)[live.reshape(-1)]
    assert ql.min() == R.TWIN_LO and ql.max() == R.TWIN_HI
    if ttype == R.IQ4_XS:
        assert set((R.ls_of(b) - 32)[live].tolist()) == {1, -1, 2, -2, 4, -4, 8, -8, 16, -16, -32}
    x = activations(rng, 6, K)
    q8, d8 = q8_rows(x)
    assert (d8 < 0).any() and (d8 > 0).any() and (d8 == 0).any()
    twin = R.to_q6k(ttype, b)
    want = np.stack([O.gemv_q8(O.TYPE_Q6_K, twin, rows, K, ks, r) for r in x])
    got = R.gemv(ttype, b, rows, K, ks, q8, d8)
    assert np.isfinite(want).all() and want.any()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (ks, np.abs(got - want).max())
    # the twins dequantise to the oracle's values, on the live sub-blocks to its bits (a dead one is +-0 on both sides)
    w6 = O.dequant_rows(O.TYPE_Q6_K, twin, rows, K).reshape(-1, 32)
    mine = R.dequant(ttype, b)
    assert np.array_equal(w6, mine) and not mine[~live.reshape(-1)].any()
    assert np.array_equal(w6[live.reshape(-1)].view(np.uint32), mine[live.reshape(-1)].view(np.uint32))


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
    """an all-IQ4_NL / all-IQ4_XS file (output Q6_K): the probe accepts it; a file that ends one block early, or whose ffn_down claims a K
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
