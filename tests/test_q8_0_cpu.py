"""CPU: Q8_0 (GGML type 8) — the NumPy codec and quantiser against hand-computed blocks and the host quantiser entry, the Q6_K twin and the
restated dot contract against the oracle, the constants, the GGUF reader's size checks for the type (and for an all-Q6_K file whose
token_embd is Q6_K), and an error bound of the contract against the unquantised dot."""
import ctypes as C
import struct

import numpy as np
import pytest

import gguf_util as G
import oracle_lib as O
import q8_0_ref as R


def probe(path):
    import trackiellm_amd as tk
    hp = tk.LlmHParams()
    nv = C.c_int32(0)
    return tk.lib().tk_mi355x_gguf_probe(path.encode(), C.byref(hp), C.byref(nv))


def hand_inputs():
    """three blocks of 32 weights: one whose extreme is positive, one whose extreme is negative, one all zero"""
    x = np.zeros((3, 32), np.float32)
    x[0, :6] = [127.0, -63.5, 1.5, 2.5, -0.49, 0.5]        # d = 1: halves round away from zero
    x[1, :5] = [-254.0, 254.0 * 126.5 / 127.0, 3.0, -1.0, 1.0]   # amax from a negative value, d = 2
    return x


def test_codec_and_quantiser_on_hand_computed_blocks():
    x = hand_inputs()
    b = R.quantize(x)
    assert b.shape == (3, 34)
    assert [float(v) for v in R.d_of(b)] == [1.0, 2.0, 0.0]
    q = R.quants(b)
    assert [int(v) for v in q[0, :7]] == [127, -64, 2, 3, 0, 1, 0]
    # block 1: id = fl(1 / 2) = 0.5 exactly, so q = roundf(x / 2): -127, roundf(126.5) = 127, roundf(1.5) = 2, roundf(-0.5) = -1, 1
    assert [int(v) for v in q[1, :6]] == [-127, 127, 2, -1, 1, 0]
    assert not b[2].any()                                   # all zero: d = +0 and every q = 0
    w = R.dequant(b)
    assert [float(v) for v in w[0, :4]] == [127.0, -64.0, 2.0, 3.0] and [float(v) for v in w[1, :3]] == [-254.0, 254.0, 4.0]
    # the decode alone, on bytes written by hand: d = -0.5 (f16 0xB800), q = -128, 127, -1
    raw = np.zeros(34, np.uint8)
    raw[0:2] = [0x00, 0xB8]
    raw[2:5] = [0x80, 0x7F, 0xFF]
    assert [int(v) for v in R.quants(raw)[0, :4]] == [-128, 127, -1, 0]
    assert [float(v) for v in R.dequant(raw)[0, :4]] == [64.0, -63.5, 0.5, -0.0]
    assert np.array_equal(R.make_blocks(R.quants(raw), R.d_of(raw)), raw[None])


def quantiser_inputs():
    rng = np.random.default_rng(81)
    x = [hand_inputs(), (rng.standard_normal((256, 32)) * 0.02).astype(np.float32), rng.standard_normal((64, 32)).astype(np.float32) * 1e4,
         (rng.standard_normal((64, 32)) * 1e-6).astype(np.float32), np.full((2, 32), -0.37, np.float32)]
    h = rng.integers(-127, 128, (64, 32)).astype(np.float32) + 0.5       # many products x * id near a half
    h[:, 0] = 127.0
    x.append(h)
    return np.concatenate(x)


def test_host_quantiser_equals_the_numpy_quantiser_byte_for_byte():
    import trackiellm_amd as tk
    x = quantiser_inputs()
    got = tk.quantize_blocks(tk.TYPE_Q8_0, x)
    assert got.shape == (x.shape[0], 34) and got.dtype == np.uint8
    want = R.quantize(x)
    bad = np.argwhere((got != want).any(axis=1))
    assert bad.size == 0, (bad[:4].tolist(), got[bad[0, 0]], want[bad[0, 0]])
    # a row of 256 n weights is n / 32 blocks, in order
    assert np.array_equal(tk.quantize_blocks(tk.TYPE_Q8_0, x[:16].reshape(2, 256)), want[:16])


def test_constants_and_refused_quantiser_types():
    import trackiellm_amd as tk
    assert (tk.TYPE_Q8_0, tk.FTYPE_Q8_0, tk.llm.BLOCK_BYTES[8]) == (8, 7, 34)
    fn = tk.lib().tk_mi355x_quantize_blocks
    fn.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    x = np.zeros(256, np.float32)
    out = np.zeros(8 * 34, np.uint8)                       # 256 weights = eight 34-byte blocks
    xp, op = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert fn(8, xp, 8, op) == 0 and fn(8, xp, 0, op) == 0
    assert fn(8, None, 1, op) != 0 and fn(8, xp, 1, None) != 0 and fn(8, xp, -1, op) != 0
    for bad in (0, 2, 9, 10, 15):
        assert fn(bad, xp, 1, op) != 0


def twin_runs(rng, rows, nb):
    """[rows][nb] twin-able 256-k runs: one live block per run at a random position, q in -32..31 and d of both signs there; +0 d and
    random quants in the other seven"""
    n = rows * nb
    live = rng.integers(0, 8, n)
    q = rng.integers(-128, 128, (n, 8, 32))
    q[np.arange(n), live] = rng.integers(-32, 32, (n, 32))
    d = np.zeros((n, 8), np.float16)
    d[np.arange(n), live] = (rng.uniform(1e-3, 1e-2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float16)
    b = R.make_blocks(q.reshape(-1, 32), d.reshape(-1).view(np.uint16))
    assert set(R.live_of(b).tolist()) == set(range(8))
    return b


def activations(rng, n, K):
    """rows whose Q8_K scales take both signs (the oracle's scale carries the sign of the largest-magnitude value), one with an all-zero
    run"""
    x = rng.standard_normal((n, K)).astype(np.float32)
    x[0, 256:512] = 0.0
    x[1, 0] = -7.0
    x[2, 0] = 7.0
    return x


def q8_rows(x):
    qs, ds, _ = zip(*[O.q8k_quantize(r) for r in x])
    return np.stack(qs), np.stack(ds).reshape(len(x), -1)


def test_twins_dequantise_to_the_oracles_bits():
    """the live block of every run: the oracle's bits.  The seven zero blocks decode to +-0 on both sides (+0 q against (d 0) 0: the sign
    of a zero follows q here and d there), equal as numbers"""
    rng = np.random.default_rng(82)
    rows, nb = 64, 7
    b = twin_runs(rng, rows, nb)
    got = O.dequant_rows(O.TYPE_Q6_K, R.to_q6k(b), rows, nb * 256)
    mine = R.dequant(b).reshape(rows, nb * 256)
    assert np.array_equal(got, mine)
    live = np.repeat(R.d_of(b) != 0, 32).reshape(rows, nb * 256)
    assert live.sum() == rows * nb * 32
    assert np.array_equal(got[live].view(np.uint32), mine[live].view(np.uint32))
    assert not mine[~live].any()


@pytest.mark.parametrize("ks", [1, 7])
def test_restated_contract_equals_the_oracle_on_twin_rows(ks):
    """q8_0_ref.gemv on twin-able runs is oracle_lib.gemv_q8 on their Q6_K twins, bit for bit: the restatement the GPU tests hold general
    blocks against is the oracle's contract"""
    rng = np.random.default_rng(83)
    rows, K = 64, 1792
    b = twin_runs(rng, rows, K // 256)
    x = activations(rng, 6, K)
    q8, d8 = q8_rows(x)
    assert (d8 < 0).any() and (d8 > 0).any() and (d8 == 0).any()
    twin = R.to_q6k(b)
    want = np.stack([O.gemv_q8(O.TYPE_Q6_K, twin, rows, K, ks, r) for r in x])
    got = R.gemv(b, rows, K, ks, q8, d8)
    assert np.isfinite(want).all() and want.any()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (ks, np.abs(got - want).max())


def test_contract_stays_within_the_activation_rounding_bound():
    """A bound, not a measurement.  With w the dequantised weights, x the unquantised activations and a, d8 their Q8_K image:
      * the contract's exact-arithmetic value is E' = sum_k w_k (d8_b a_k); the Q8_K quantiser rounds iscale x to the nearest integer and
        never clips (|iscale x| <= 127 (1 + 2^-24)), so |x_k - d8_b a_k| <= 0.5 |d8_b| up to d8_b = fl(1 / fl(-127 / mx)) not being the
        exact inverse of iscale: 127 |d8_b| 2^-22 < 2^-15 |d8_b| more.  Hence |E' - sum w x| <= sum_b (0.5 + 2^-15) |d8_b| sum_k |w_k|;
      * the binary32 evaluation makes one rounding per scale product and one per fmaf, n = K / 32 of each per slab, then ks - 1 adds:
        |R - E'| <= (n + ks + 1) 2^-24 S (1 + O(n 2^-24)), S = sum_k |w_k| |d8_b a_k| bounding every partial sum; the test allows
        (n + ks + 1) 2^-23 S.
    So the slack beside the stated bound sum_b 0.5 |d8_b| sum_k |w_k| is  2^-15 sum_b |d8_b| sum_k |w_k| + (K / 32 + ks + 1) 2^-23 S."""
    rng = np.random.default_rng(84)
    rows, K = 32, 4096
    w = (rng.standard_normal((rows, K)) * 0.02).astype(np.float32)
    b = R.quantize(w)
    wq = R.dequant(b).reshape(rows, K).astype(np.float64)
    x = rng.standard_normal((8, K)).astype(np.float32)
    q8, d8 = q8_rows(x)
    for ks in (1, 4):
        got = R.gemv(b, rows, K, ks, q8, d8).astype(np.float64)
        exact = x.astype(np.float64) @ wq.T
        absw = np.abs(wq).reshape(rows, K // 256, 256).sum(axis=2)                       # (rows, nb)
        bound = 0.5 * np.abs(d8).astype(np.float64) @ absw.T                            # (nrows, rows)
        xq = (q8.astype(np.float64).reshape(8, K // 256, 256) * d8.astype(np.float64)[:, :, None]).reshape(8, K)
        S = np.abs(xq) @ np.abs(wq).T
        slack = 2.0 ** -15 * 2 * bound + (K // 32 + ks + 1) * 2.0 ** -23 * S
        err = np.abs(got - exact)
        assert (err <= bound + slack).all(), (ks, float((err / (bound + slack)).max()))
        assert err.max() > 0


def all_of(ttype):
    """a tiny llama GGUF source whose every matrix, token_embd and output are `ttype` (8: the host quantiser's Q8_0 blocks; 14: the
    oracle's Q6_K quantiser), norms F32"""
    import trackiellm_amd as tk
    cfg = O.tiny_config()
    orc = O.OracleLlm(cfg, seed=4)
    D, FF, QD, KVD = cfg.d_model, cfg.d_ff, cfg.n_head * cfg.head_dim, cfg.n_kv_head * cfg.head_dim
    shape = {1: (QD, D), 2: (KVD, D), 3: (KVD, D), 4: (D, QD), 6: (FF, D), 7: (FF, D), 8: (D, FF)}

    class Src(object):
        def get_tensor(self, layer, which):
            t, buf = orc.get_tensor(layer, which)
            if (layer < 0 and which != O.T_OUT_NORM) or (layer >= 0 and which in shape):
                w = orc.dequant(layer, which, *((cfg.vocab, D) if layer < 0 else shape[which]))
                if ttype == 8:
                    return 8, tk.quantize_blocks(tk.TYPE_Q8_0, w).reshape(-1)
                return O.TYPE_Q6_K, O.quantize_rows(O.TYPE_Q6_K, w)
            return t, buf
    return Src(), cfg


@pytest.mark.parametrize("ttype,block_bytes", [(8, 34), (14, 210)])
def test_gguf_of_one_type_passes_the_probe_and_short_data_is_refused(tmp_path, ttype, block_bytes):
    """an all-Q8_0 file, and an all-Q6_K file whose token_embd is Q6_K too: the probe accepts them; a file that ends one block early, or
    whose ffn_down claims a K running past the end of the file or wrapping the element count, comes back 3004"""
    src, cfg = all_of(ttype)
    p = str(tmp_path / "whole.gguf")
    G.write_llama_gguf(p, src, cfg)
    raw = bytearray(open(p, "rb").read())
    for name in ("token_embd.weight", "output.weight", "blk.0.attn_q.weight", "blk.1.ffn_down.weight"):
        at = raw.index(G._s(name)) + len(G._s(name))
        ndim = struct.unpack_from("<I", raw, at)[0]
        assert struct.unpack_from("<I", raw, at + 4 + 8 * ndim)[0] == ttype, name
    assert probe(p) == 0
    # the last tensor of the file is blk.1.ffn_down
    (tmp_path / "one_short.gguf").write_bytes(bytes(raw[:-block_bytes]))
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
