"""GPU: Q5_K weights (GGML type 13) on the W4A8 kernels.  The oracle has no Q5_K, so parity rests on re-encoding its Q4_K tensors as Q5_K
blocks with zero high bits (the same weights: logits and ids must stay the oracle's, bit for bit, at every pass width), and on width / batch
invariance of synthetic Q5_K_M and Q4_K_S models whose high bits are live."""
import ctypes as C

import numpy as np
import pytest

import gguf_util
import oracle_lib as O
import q5k_ref as R
from kquant_gpu_util import install, logits_in_passes, oracle_cfg_from, WIDTHS

pytestmark = pytest.mark.gpu


class Reencoded:
    """the oracle's tensors with the Q4_K ones for which pick(layer, which) holds re-encoded as Q5_K (qh = 0)"""

    def __init__(self, orc, pick):
        self.orc, self.pick = orc, pick

    def get_tensor(self, layer, which):
        t, buf = self.orc.get_tensor(layer, which)
        if t == 12 and self.pick(layer, which):
            return 13, R.q4k_to_q5k(buf)
        return t, buf


Q5_K_M = lambda layer, which: True                                 # every Q4_K tensor, token_embd included
Q4_K_S = lambda layer, which: (which == 3 and layer == 0) or (which == 8 and layer == 1)   # attn_v / ffn_down of chosen layers


@pytest.mark.parametrize("mix", ["q5_k_m", "q4_k_s"])
def test_q5k_reencoded_oracle_model_bit_exact_at_every_width(gpu, mix, monkeypatch):
    pick = Q5_K_M if mix == "q5_k_m" else Q4_K_S
    hp = gpu.TINY()
    model = gpu.LlmModel(hp)
    hp = model.hparams
    orc = O.OracleLlm(oracle_cfg_from(hp, 8, 256), seed=4)
    install(model, Reencoded(orc, pick), hp.n_layer)
    check_widths(gpu, model, hp, orc, monkeypatch, mix)


def check_widths(gpu, model, hp, orc, monkeypatch, tag):
    """logits and ids bit-identical to the oracle at every width in WIDTHS (and at 1, 2 rows with the producers as launches of their own),
    two positions through the KV cache"""
    rng = np.random.default_rng(11)
    for no_fuse in ("0", "1"):
        monkeypatch.setenv("TK_MI355X_NO_FUSE", no_fuse)
        for n in (WIDTHS if no_fuse == "0" else [1, 2]):
            sess = gpu.LlmSession(model, n, 8)
            orc.reset()
            seq = np.arange(n, dtype=np.int32)
            for p in range(2):
                tok = rng.integers(3, hp.vocab, n).astype(np.int32)
                pos = np.full(n, p, np.int32)
                want, wam = orc.forward(seq, pos, tok)
                got, gam = sess.forward(seq, pos, tok)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (tag, n, p, np.abs(got - want).max())
                assert np.array_equal(gam, wam), (tag, n, p)
            sess.close()


def test_q5k_gguf_checkpoint_end_to_end(gpu, tmp_path):
    """a Q5_K_M-layout GGUF through tk_mi355x_llm_model_load_gguf's path (tk_model_loader + tk_llm_runner): the oracle's token ids"""
    cfg = O.tiny_config()
    orc = O.OracleLlm(cfg, seed=4)
    path = str(tmp_path / "tiny_q5k.gguf")
    gguf_util.write_llama_gguf(path, Reencoded(orc, Q5_K_M), cfg)
    loader = gpu.ModelLoader()
    h = loader.load(path)
    hp = gpu.LlmHParams()
    gpu.lib().tk_mi355x_llm_model_get_hparams(h, C.byref(hp))
    orc2 = O.OracleLlm(oracle_cfg_from(hp, 64, 1), seed=4)
    runner = gpu.LlmRunner(h, context_size=64)
    runner.prepare("hello world")
    ids = [1, 263, 273]
    _, am = orc2.forward([0, 0, 0], [0, 1, 2], ids, want_logits=False)
    cur = int(am[-1])
    for i in range(6):
        piece = runner.next_token()
        if cur == 2:
            assert piece is None
            break
        assert piece == gguf_util.expected_piece(cfg.vocab, cur), (i, cur, piece)
        _, am = orc2.forward([0], [3 + i], [cur], want_logits=False)
        cur = int(am[0])
    runner.close()
    loader.unload(h)
    loader.close()


def test_q4k_s_mix_gguf_logits_bit_exact_at_every_width(gpu, tmp_path, monkeypatch):
    """a Q4_K_S-layout GGUF (Q5_K attn_v / ffn_down beside Q4_K and Q6_K tensors) loaded by tk_mi355x_llm_model_load_gguf: the Q5_K tensors
    keep their 176-byte blocks through the reader, and the logits are the oracle's at every width"""
    cfg = O.tiny_config()
    orc = O.OracleLlm(cfg, seed=4)
    path = str(tmp_path / "tiny_q4ks.gguf")
    gguf_util.write_llama_gguf(path, Reencoded(orc, Q4_K_S), cfg)
    model = gpu.LlmModel(gguf=path)
    hp = model.hparams
    check_widths(gpu, model, hp, O.OracleLlm(oracle_cfg_from(hp, 8, 256), seed=4), monkeypatch, "gguf q4_k_s")


def random_q5k(rng, n):
    """n Q5_K blocks with every field random: live high bits, all scales / mins, d / dmin of both signs"""
    b = rng.integers(0, 256, (n, 176), dtype=np.uint8)
    b[:, 0:2] = (rng.uniform(1e-3, 1e-2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float16).view(np.uint8).reshape(n, 2)
    b[:, 2:4] = (rng.uniform(1e-3, 1e-2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float16).view(np.uint8).reshape(n, 2)
    return b


def test_q5k_embedding_with_live_high_bits_bit_exact(gpu):
    """token_embd as Q5_K blocks with random high bits on the GPU; the oracle gets the same rows as F32 values from the NumPy decode
    (tests/q5k_ref.py, pinned to the spec on the CPU): k_embed's Q5_K decode must give the same bits"""
    hp = gpu.TINY()
    model = gpu.LlmModel(hp)
    hp = model.hparams
    orc = O.OracleLlm(oracle_cfg_from(hp, 8, 16), seed=4)
    install(model, orc, hp.n_layer)
    emb = random_q5k(np.random.default_rng(3), hp.vocab * hp.d_model // 256)
    model.set_tensor(-1, O.T_TOKEN_EMBD, 13, emb.reshape(-1))
    orc.set_tensor(-1, O.T_TOKEN_EMBD, O.TYPE_F32, R.dequant(emb).reshape(-1))
    sess = gpu.LlmSession(model, 16, 8)
    seq = np.arange(16, dtype=np.int32)
    tok = np.random.default_rng(4).integers(3, hp.vocab, 16).astype(np.int32)
    want, wam = orc.forward(seq, np.zeros(16, np.int32), tok)
    got, gam = sess.forward(seq, np.zeros(16, np.int32), tok)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.abs(got - want).max()
    assert np.array_equal(gam, wam)


def q8_rows(x):
    qs, ds, bs = zip(*[O.q8k_quantize(r) for r in x])
    return np.stack(qs), np.stack(ds), np.stack(bs)


PROBE_K = {1: 512, 4: 3072, 7: 3584}  # 2, 3 and 2 blocks per K-range: both tile depths of the mat-vec
PROBE_NROWS = [1, 2, 16, 32, 33, 64, 128, 192, 193, 256]


def test_gemv_probe_equals_the_oracle_on_q4k_and_q6k(gpu):
    """the probe's plumbing (repack, production Q8_K kernel, launcher, slab sum) against oracle_lib.gemv_q8"""
    rng = np.random.default_rng(21)
    rows = 128
    for ttype in (O.TYPE_Q4_K, O.TYPE_Q6_K):
        for ks in (1, 4):
            K = PROBE_K[ks]
            blocks = O.quantize_rows(ttype, (rng.standard_normal((rows, K)) * 0.02).astype(np.float32))
            x = rng.standard_normal((193, K)).astype(np.float32)
            want = np.stack([O.gemv_q8(ttype, blocks, rows, K, ks, r) for r in x])
            for n in (1, 2, 16, 33, 193):
                got = gpu.gemv_probe(ttype, blocks, rows, K, ks, x[:n])
                assert np.array_equal(got.view(np.uint32), want[:n].view(np.uint32)), (ttype, ks, n)


def edge_q5k(rng, rows, nb):
    """[rows][nb] Q5_K blocks: random, then whole rows of edge cases"""
    b = random_q5k(rng, rows * nb).reshape(rows, nb, 176)
    b[0, :, 16:48] = 0xFF                                              # every high bit set
    b[1, :, 16:48] = 0                                                 # none
    b[2, :, 4:16] = 0xFF                                               # sc = m = 63 for every sub-block
    b[3, :, 4:16] = 0                                                  # zero scales and mins
    b[4, :, 0:4] = np.array([-0.0078, -0.0042], np.float16).view(np.uint8)        # negative d, dmin
    b[5, :, 0:4] = np.array([0x0001, 0x03FF], np.uint16).view(np.uint8)           # subnormal d, dmin
    b[6, :, 0:4] = np.array([0x83FF, 0x8010], np.uint16).view(np.uint8)           # negative subnormals
    b[7, :, 4:16] = 0xFF; b[7, :, 16:48] = 0xFF; b[7, :, 48:] = 0xFF    # q = 31, sc = m = 63: v = 1953 everywhere
    return b.reshape(-1)


def test_gemv_probe_q5k_equals_the_numpy_restatement(gpu):
    """Q5_K with live high bits and edge-case blocks through every W4A8 family (1..32 rows: mat-vec, 33..192: GEMM, 193..256: 32x32x32 GEMM)
    and K-split 1 / 4 / 7, against the NumPy decode and dot (q5k_ref.gemv, fmaf emulated with one rounding): bit for bit"""
    rng = np.random.default_rng(22)
    rows = 128
    for ks in (1, 4, 7):
        K = PROBE_K[ks]
        blocks = edge_q5k(rng, rows, K // 256)
        x = rng.standard_normal((256, K)).astype(np.float32)
        want = R.gemv(blocks, rows, K, ks, *q8_rows(x))
        assert np.isfinite(want).all()
        for n in PROBE_NROWS:
            got = gpu.gemv_probe(13, blocks, rows, K, ks, x[:n])
            assert np.array_equal(got.view(np.uint32), want[:n].view(np.uint32)), (ks, n, np.abs(got - want[:n]).max())


@pytest.mark.parametrize("nrows", [16, 256])
def test_q5k_mistral_shape_layer_bit_exact(gpu, nrows):
    """one Mistral-7B-shaped layer (production K-split plan 4/4/1/7) with its Q4_K tensors as Q5_K, against the oracle (256 rows: the
    32x32x32 kernel with the fused SwiGLU epilogue)"""
    hp = gpu.MISTRAL_7B()
    hp.n_layer = 1
    model = gpu.LlmModel(hp)
    hp = model.hparams
    assert (hp.ks_qkv, hp.ks_o, hp.ks_gateup, hp.ks_down) == (4, 4, 1, 7)
    orc = O.OracleLlm(oracle_cfg_from(hp, 4, nrows), seed=4)
    install(model, Reencoded(orc, Q5_K_M), 1)
    sess = gpu.LlmSession(model, nrows, 4)
    seq = np.arange(nrows, dtype=np.int32)
    tok = np.random.default_rng(2).integers(3, hp.vocab, nrows).astype(np.int32)
    want, wam = orc.forward(seq, np.zeros(nrows, np.int32), tok)
    got, gam = sess.forward(seq, np.zeros(nrows, np.int32), tok)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.abs(got - want).max()
    assert np.array_equal(gam, wam)


@pytest.mark.parametrize("ftype", [17, 14])
def test_q5k_synthetic_width_and_batch_invariance(gpu, ftype):
    """high bits live: a 2-layer Mistral-shaped Q5_K_M / Q4_K_S model gives the same logits bits as 1 x 256, 2 x 128, 8 x 32, 16 x 16 and
    256 x 1 passes (every kernel family, fused producers at one row), over two positions through the KV cache"""
    hp = gpu.MISTRAL_7B()
    hp.n_layer = 2
    model = gpu.LlmModel(hp).fill_synthetic(4, ftype=ftype)
    hp = model.hparams
    rng = np.random.default_rng(7)
    toks = [rng.integers(3, hp.vocab, 256).astype(np.int32) for _ in range(2)]
    ref = logits_in_passes(gpu, model, hp, 256, toks)
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()
    for width in (128, 32, 16, 1):
        got = logits_in_passes(gpu, model, hp, width, toks)
        for p in range(2):
            assert np.array_equal(got[p].view(np.uint32), ref[p].view(np.uint32)), (ftype, width, p)
    # two fills with one seed are identical
    again = gpu.LlmModel(hp).fill_synthetic(4, ftype=ftype)
    got = logits_in_passes(gpu, again, hp, 256, toks)
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32))


def test_ftype_15_is_fill_synthetic_and_other_ftypes_are_refused(gpu):
    hp = gpu.TINY()
    a = gpu.LlmModel(hp).fill_synthetic(9)
    b = gpu.LlmModel(hp).fill_synthetic(9, ftype=gpu.FTYPE_Q4_K_M)
    toks = np.arange(3, 19, dtype=np.int32)
    seq, pos = np.arange(16, dtype=np.int32), np.zeros(16, np.int32)
    la, _ = gpu.LlmSession(a, 16, 4).forward(seq, pos, toks)
    lb, _ = gpu.LlmSession(b, 16, 4).forward(seq, pos, toks)
    assert np.array_equal(la.view(np.uint32), lb.view(np.uint32))
    lc, _ = gpu.LlmSession(gpu.LlmModel(hp).fill_synthetic(9, ftype=gpu.FTYPE_Q5_K_M), 16, 4).forward(seq, pos, toks)
    assert not np.array_equal(la, lc)
    for bad in (0, 13, 18):
        with pytest.raises(gpu.TkError):
            gpu.LlmModel(hp).fill_synthetic(9, ftype=bad)


def test_lora_into_a_q5k_matrix_fails_the_load(gpu, tmp_path):
    hp = gpu.TINY()
    orc = O.OracleLlm(O.tiny_config(), seed=4)
    rng = np.random.default_rng(1)
    D = hp.d_model
    factors = {(0, 3): (rng.standard_normal((4, D)).astype(np.float32) * 0.01,
                        rng.standard_normal((hp.n_kv_head * hp.head_dim, 4)).astype(np.float32) * 0.01)}
    ad = str(tmp_path / "v.gguf")
    gguf_util.write_lora_gguf(ad, 8.0, factors)
    model = gpu.LlmModel(hp)
    model.set_lora(ad)
    src = Reencoded(orc, Q5_K_M)
    with pytest.raises(gpu.TkError) as ei:
        model.set_tensor(0, 3, *src.get_tensor(0, 3))
    assert "Q5_K" in str(ei.value)
