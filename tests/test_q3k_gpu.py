"""GPU: Q3_K weights (GGML type 11) on the W4A8 kernels, bit for bit against the oracle.  The oracle has no Q3_K; every Q3_K block has an
exact Q6_K twin (tests/q3k_ref.py: same d, scales[g] = sc6_g - 32, q6 = q + 32 — the same weights and the same integer block sum, pinned
on the CPU by tests/test_q3k_cpu.py), so the oracle holds the twins and its logits, ids and mat-vec results are the expected ones."""
import ctypes as C

import numpy as np
import pytest

import gguf_util
import oracle_lib as O
import q3k_ref as R
import q5k_ref as R5
from kquant_gpu_util import check_widths, install, logits_in_passes, oracle_cfg_from, shapes, WIDTHS

pytestmark = pytest.mark.gpu

Q3, Q4, Q5, Q6 = 11, 12, 13, 14


# which GGML type a tensor takes in a mix: layout(layer, which, n_layer); layer -1 / which 0 is token_embd
def q3_k_s(layer, which, n_layer):
    return Q3


def q3_k_m(layer, which, n_layer):
    if layer >= 0 and which == 3:
        return Q5 if layer < 2 else Q4
    if layer >= 0 and which == 4:
        return Q4
    if layer >= 0 and which == 8:
        return Q5 if layer < n_layer // 16 else Q4
    return Q3


def q3_k_l(layer, which, n_layer):
    return Q5 if layer >= 0 and which in (3, 4, 8) else Q3


def q3_matrices(layer, which, n_layer):
    """every matrix of the layers Q3_K; token_embd stays the oracle's (None = keep)"""
    return Q3 if layer >= 0 else None


class Mixed:
    """The tensors of an oracle model under a mix, as the device takes them; the ORACLE IS CHANGED to hold exactly the same weights:
    a Q3_K tensor is made by the host quantiser from the oracle's dequantised weights and the oracle gets its Q6_K twins (token_embd: the
    NumPy-decoded F32 rows); a Q4_K choice keeps the oracle's Q4_K blocks (a Q6_K original is re-quantised to Q4_K on both sides); a Q5_K
    choice is the Q4_K blocks re-encoded with zero high bits, as in tests/test_q5k_gpu.py.  output and the norms stay as they are."""

    def __init__(self, tk, orc, cfg, layout):
        self.orc, self.t = orc, {}
        todo = [(-1, 0, cfg.vocab, cfg.d_model)] + [(l, w, r, c) for l in range(cfg.n_layer) for w, (r, c) in shapes(cfg).items()]
        for layer, which, rows, cols in todo:
            want = layout(layer, which, cfg.n_layer)
            if want is None:
                continue
            t, buf = orc.get_tensor(layer, which)
            if want == Q3:
                b3 = tk.quantize_blocks(Q3, orc.dequant(layer, which, rows, cols))
                if layer < 0:
                    orc.set_tensor(layer, which, O.TYPE_F32, R.dequant(b3).reshape(-1))
                else:
                    orc.set_tensor(layer, which, O.TYPE_Q6_K, R.q3k_to_q6k(b3))
                self.t[(layer, which)] = (Q3, b3.reshape(-1))
            else:
                if t != Q4:
                    buf = O.quantize_rows(O.TYPE_Q4_K, orc.dequant(layer, which, rows, cols))
                    orc.set_tensor(layer, which, O.TYPE_Q4_K, buf)
                self.t[(layer, which)] = (Q4, buf) if want == Q4 else (Q5, R5.q4k_to_q5k(buf))

    def get_tensor(self, layer, which):
        return self.t[(layer, which)] if (layer, which) in self.t else self.orc.get_tensor(layer, which)


@pytest.mark.parametrize("mix", ["q3_k_s", "q3_k_m", "q3_k_l"])
def test_q3k_oracle_model_bit_exact_at_every_width(gpu, mix, monkeypatch):
    layout = {"q3_k_s": q3_k_s, "q3_k_m": q3_k_m, "q3_k_l": q3_k_l}[mix]
    hp = gpu.TINY()
    model = gpu.LlmModel(hp)
    hp = model.hparams
    cfg = oracle_cfg_from(hp, 8, 256)
    orc = O.OracleLlm(cfg, seed=4)
    src = Mixed(gpu, orc, cfg, layout)
    types = {src.get_tensor(l, w)[0] for l in range(hp.n_layer) for w in (1, 2, 3, 4, 6, 7, 8)} | {src.get_tensor(-1, 2)[0]}
    assert types == {"q3_k_s": {Q3, Q6}, "q3_k_m": {Q3, Q4, Q5, Q6}, "q3_k_l": {Q3, Q5, Q6}}[mix]
    install(model, src, hp.n_layer)
    check_widths(gpu, model, hp, orc, monkeypatch, mix)


def random_q3k(rng, n):
    """n Q3_K blocks with every field random and d of both signs"""
    b = rng.integers(0, 256, (n, 110), dtype=np.uint8)
    b[:, 108:110] = (rng.uniform(1e-3, 1e-2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float16).view(np.uint8).reshape(n, 2)
    return b


def edge_q3k(rng, rows, nb):
    """[rows][nb] Q3_K blocks: random, then whole rows of edge cases"""
    b = random_q3k(rng, rows * nb).reshape(rows, nb, 110)
    b[0, :, 0:32] = 0xFF                                               # every hmask bit set: q in 0..3
    b[1, :, 0:32] = 0                                                  # none: q in -4..-1
    b[2, :, 96:108] = 0xFF                                             # sc6 = 63: s = 31 in every group
    b[3, :, 96:108] = 0                                                # sc6 = 0: s = -32
    b[4, :, 0:108] = 0                                                 # s = -32 and q = -4 in every weight: s q = +128
    b[5, :, 108:110] = np.array([-0.0078], np.float16).view(np.uint8)  # negative d
    b[6, :, 108:110] = np.array([0x0001], np.uint16).view(np.uint8)    # subnormal d
    b[7, :, 108:110] = np.array([0x83FF], np.uint16).view(np.uint8)    # negative subnormal d
    b[8, :, 0:96] = 0xFF; b[8, :, 96:108] = 0xFF                       # q = 3, s = 31
    b[9, :, 0:96] = 0xFF; b[9, :, 96:108] = 0                          # q = 3, s = -32: s q = -96
    return b.reshape(-1)


PROBE_K = {1: 512, 4: 3072, 7: 3584}  # 2, 3 and 2 blocks per K-range: both tile depths of the mat-vec
PROBE_NROWS = [1, 2, 16, 32, 33, 64, 128, 192, 193, 256]


def test_gemv_probe_q3k_equals_the_oracle_on_the_q6k_twins(gpu):
    """Q3_K random and edge-case blocks through every W4A8 family (1..32 rows: mat-vec, 33..192: GEMM, 193..256: 32x32x32 GEMM) and
    K-split 1 / 4 / 7, against oracle_lib.gemv_q8 on the Q6_K twins: bit for bit"""
    rng = np.random.default_rng(23)
    rows = 128
    for ks in (1, 4, 7):
        K = PROBE_K[ks]
        blocks = edge_q3k(rng, rows, K // 256)
        twins = R.q3k_to_q6k(blocks)
        x = rng.standard_normal((256, K)).astype(np.float32)
        want = np.stack([O.gemv_q8(O.TYPE_Q6_K, twins, rows, K, ks, r) for r in x])
        assert np.isfinite(want).all()
        for n in PROBE_NROWS:
            got = gpu.gemv_probe(Q3, blocks, rows, K, ks, x[:n])
            assert np.array_equal(got.view(np.uint32), want[:n].view(np.uint32)), (ks, n, np.abs(got - want[:n]).max())


@pytest.mark.parametrize("nrows", [16, 256])
def test_q3k_mistral_shape_layer_bit_exact(gpu, nrows):
    """one Mistral-7B-shaped layer (production K-split plan 4/4/1/7) with all seven matrices Q3_K, against the oracle (256
    rows: the 32x32x32 kernel with the fused SwiGLU epilogue)"""
    hp = gpu.MISTRAL_7B()
    hp.n_layer = 1
    model = gpu.LlmModel(hp)
    hp = model.hparams
    assert (hp.ks_qkv, hp.ks_o, hp.ks_gateup, hp.ks_down) == (4, 4, 1, 7)
    cfg = oracle_cfg_from(hp, 4, nrows)
    orc = O.OracleLlm(cfg, seed=4)
    install(model, Mixed(gpu, orc, cfg, q3_matrices), 1)
    sess = gpu.LlmSession(model, nrows, 4)
    seq = np.arange(nrows, dtype=np.int32)
    tok = np.random.default_rng(2).integers(3, hp.vocab, nrows).astype(np.int32)
    want, wam = orc.forward(seq, np.zeros(nrows, np.int32), tok)
    got, gam = sess.forward(seq, np.zeros(nrows, np.int32), tok)
    assert np.isfinite(want).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.abs(got - want).max()
    assert np.array_equal(gam, wam)


def test_q3k_embedding_with_random_live_bits_bit_exact(gpu):
    """token_embd as Q3_K blocks of random bytes on the GPU; the oracle gets the same rows as F32 values from the NumPy decode
    (tests/q3k_ref.py, pinned to the spec on the CPU): k_embed's Q3_K decode must give the same bits"""
    hp = gpu.TINY()
    model = gpu.LlmModel(hp)
    hp = model.hparams
    orc = O.OracleLlm(oracle_cfg_from(hp, 8, 16), seed=4)
    install(model, orc, hp.n_layer)
    emb = random_q3k(np.random.default_rng(3), hp.vocab * hp.d_model // 256)
    model.set_tensor(-1, O.T_TOKEN_EMBD, Q3, emb.reshape(-1))
    orc.set_tensor(-1, O.T_TOKEN_EMBD, O.TYPE_F32, R.dequant(emb).reshape(-1))
    sess = gpu.LlmSession(model, 16, 8)
    seq = np.arange(16, dtype=np.int32)
    tok = np.random.default_rng(4).integers(3, hp.vocab, 16).astype(np.int32)
    want, wam = orc.forward(seq, np.zeros(16, np.int32), tok)
    got, gam = sess.forward(seq, np.zeros(16, np.int32), tok)
    assert np.isfinite(want).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.abs(got - want).max()
    assert np.array_equal(gam, wam)


def test_q3k_m_gguf_logits_bit_exact_at_every_width(gpu, tmp_path, monkeypatch):
    """a Q3_K_M-layout GGUF (Q3_K beside Q4_K, Q5_K and Q6_K tensors) loaded by tk_mi355x_llm_model_load_gguf: the Q3_K tensors keep their
    110-byte blocks through the reader, and the logits are the oracle's at every width"""
    cfg = O.tiny_config()
    path = str(tmp_path / "tiny_q3km.gguf")
    gguf_util.write_llama_gguf(path, Mixed(gpu, O.OracleLlm(cfg, seed=4), cfg, q3_k_m), cfg)
    model = gpu.LlmModel(gguf=path)
    hp = model.hparams
    cfg2 = oracle_cfg_from(hp, 8, 256)  # the K-split plan the loader chose
    orc = O.OracleLlm(cfg2, seed=4)
    Mixed(gpu, orc, cfg2, q3_k_m)       # the same seed and mix: the oracle now holds the file's weights
    check_widths(gpu, model, hp, orc, monkeypatch, "gguf q3_k_m")


def test_q3k_m_gguf_checkpoint_end_to_end(gpu, tmp_path):
    """the same file through tk_model_loader + tk_llm_runner: the oracle's token ids"""
    cfg = O.tiny_config()
    path = str(tmp_path / "tiny_q3km.gguf")
    gguf_util.write_llama_gguf(path, Mixed(gpu, O.OracleLlm(cfg, seed=4), cfg, q3_k_m), cfg)
    loader = gpu.ModelLoader()
    h = loader.load(path)
    hp = gpu.LlmHParams()
    gpu.lib().tk_mi355x_llm_model_get_hparams(h, C.byref(hp))
    cfg2 = oracle_cfg_from(hp, 64, 1)
    orc = O.OracleLlm(cfg2, seed=4)
    Mixed(gpu, orc, cfg2, q3_k_m)
    runner = gpu.LlmRunner(h, context_size=64)
    runner.prepare("hello world")
    ids = [1, 263, 273]
    _, am = orc.forward([0, 0, 0], [0, 1, 2], ids, want_logits=False)
    cur = int(am[-1])
    for i in range(6):
        piece = runner.next_token()
        if cur == 2:
            assert piece is None
            break
        assert piece == gguf_util.expected_piece(cfg.vocab, cur), (i, cur, piece)
        _, am = orc.forward([0], [3 + i], [cur], want_logits=False)
        cur = int(am[0])
    runner.close()
    loader.unload(h)
    loader.close()


@pytest.mark.parametrize("ftype", [11, 12])
def test_q3k_synthetic_width_and_batch_invariance(gpu, ftype):
    """a 2-layer Mistral-shaped Q3_K_S / Q3_K_M model gives the same logits bits as 1 x 256, 2 x 128, 8 x 32, 16 x 16 and 256 x 1 passes
    (every kernel family, fused producers at one row), over two positions through the KV cache; two fills with one seed are identical;
    the logits are not the Q4_K_M model's"""
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
    again = gpu.LlmModel(hp).fill_synthetic(4, ftype=ftype)
    got = logits_in_passes(gpu, again, hp, 256, toks)
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32))
    q4km = gpu.LlmModel(hp).fill_synthetic(4, ftype=gpu.FTYPE_Q4_K_M)
    other = logits_in_passes(gpu, q4km, hp, 256, toks)
    assert not np.array_equal(other[0], ref[0])


def test_ftype_constants_and_weight_bytes(gpu):
    assert (gpu.FTYPE_Q3_K_S, gpu.FTYPE_Q3_K_M, gpu.TYPE_Q3_K) == (11, 12, 11)
    hp = gpu.TINY()
    s = gpu.LlmModel(hp).fill_synthetic(9, ftype=gpu.FTYPE_Q3_K_S)
    m = gpu.LlmModel(hp).fill_synthetic(9, ftype=gpu.FTYPE_Q3_K_M)
    k = gpu.LlmModel(hp).fill_synthetic(9, ftype=gpu.FTYPE_Q4_K_M)
    assert s.weight_bytes < m.weight_bytes < k.weight_bytes


def test_lora_into_a_q3k_matrix_fails_the_load(gpu, tmp_path):
    hp = gpu.TINY()
    rng = np.random.default_rng(1)
    D = hp.d_model
    kvd = hp.n_kv_head * hp.head_dim
    factors = {(0, 3): (rng.standard_normal((4, D)).astype(np.float32) * 0.01, rng.standard_normal((kvd, 4)).astype(np.float32) * 0.01)}
    ad = str(tmp_path / "v.gguf")
    gguf_util.write_lora_gguf(ad, 8.0, factors)
    model = gpu.LlmModel(hp)
    model.set_lora(ad)
    blocks = gpu.quantize_blocks(Q3, (rng.standard_normal((kvd, D)) * 0.02).astype(np.float32))
    with pytest.raises(gpu.TkError) as ei:
        model.set_tensor(0, 3, Q3, blocks.reshape(-1))
    assert "Q3_K" in str(ei.value)
