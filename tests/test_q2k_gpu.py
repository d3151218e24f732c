"""GPU: Q2_K weights (GGML type 10) on the W4A8 kernels, bit for bit against the oracle.  The oracle has no Q2_K.  Two exact twins and a
NumPy restatement pin it (tests/q2k_ref.py, held against the oracle on the CPU by tests/test_q2k_cpu.py): a block whose groups 2 j and
2 j + 1 share (sc, m) is a Q4_K block, a block with dmin = +0 is a Q6_K block, and general blocks — sixteen independent scales and mins —
are held against q2k_ref.gemv, the contract restated with an exact fmaf."""
import ctypes as C

import numpy as np
import pytest

import gguf_util
import oracle_lib as O
import q2k_ref as R
import q3k_ref as R3
from kquant_gpu_util import check_widths, install, logits_in_passes, oracle_cfg_from, shapes, WIDTHS

pytestmark = pytest.mark.gpu

Q2, Q3, Q4, Q6 = 10, 11, 12, 14
BLOCK_BYTES_INSTALLED = {Q2: 84, Q3: 114, Q4: 144, Q6: 210}   # Q3_K matrices are held as 1824-byte tiles: 114 B per block


# which GGML type a tensor takes in a mix: layout(layer, which, cfg); layer -1 / which 0 is token_embd.  The two ftype layouts restate
# fill_synthetic_ftype's recipes 10 and 21 (output stays the oracle's Q6_K in all of them)
def all_q2k(layer, which, cfg):
    return Q2


def ftype_10(layer, which, cfg):
    if layer >= 0 and which == 3:
        return Q4 if cfg.n_head // cfg.n_kv_head >= 4 else Q3
    if layer >= 0 and which in (4, 8):
        return Q3
    return Q2


def ftype_21(layer, which, cfg):
    if layer >= 0 and which == 3 and cfg.n_head // cfg.n_kv_head >= 4:
        return Q4
    if layer >= 0 and which == 8 and layer < cfg.n_layer // 8:
        return Q4
    return Q2


def q2_matrices(layer, which, cfg):
    """every matrix of the layers Q2_K; token_embd stays the oracle's (None = keep)"""
    return Q2 if layer >= 0 else None


class Mixed:
    """The tensors of an oracle model under a mix, as the device takes them; the ORACLE IS CHANGED to hold exactly the same weights:
    a Q2_K tensor is built in NumPy from the oracle's dequantised weights with paired groups and the oracle gets its Q4_K twins
    (token_embd: the NumPy-decoded F32 rows); a Q3_K tensor is made by the host quantiser and the oracle gets its Q6_K twins, as in
    tests/test_q3k_gpu.py; a Q4_K choice keeps the oracle's Q4_K blocks (a Q6_K original is re-quantised to Q4_K on both sides).
    output and the norms stay as they are."""

    def __init__(self, tk, orc, cfg, layout, encode=R.quantize_paired):
        self.orc, self.t = orc, {}
        todo = [(-1, 0, cfg.vocab, cfg.d_model)] + [(l, w, r, c) for l in range(cfg.n_layer) for w, (r, c) in shapes(cfg).items()]
        for layer, which, rows, cols in todo:
            want = layout(layer, which, cfg)
            if want is None:
                continue
            t, buf = orc.get_tensor(layer, which)
            if want == Q2:
                b2 = encode(orc.dequant(layer, which, rows, cols))
                if layer < 0:
                    orc.set_tensor(layer, which, O.TYPE_F32, R.dequant(b2).reshape(-1))
                else:
                    orc.set_tensor(layer, which, O.TYPE_Q4_K, R.to_q4k(b2))
                self.t[(layer, which)] = (Q2, b2.reshape(-1))
            elif want == Q3:
                b3 = tk.quantize_blocks(Q3, orc.dequant(layer, which, rows, cols))
                orc.set_tensor(layer, which, O.TYPE_Q6_K, R3.q3k_to_q6k(b3))
                self.t[(layer, which)] = (Q3, b3.reshape(-1))
            else:
                if t != Q4:
                    buf = O.quantize_rows(O.TYPE_Q4_K, orc.dequant(layer, which, rows, cols))
                    orc.set_tensor(layer, which, O.TYPE_Q4_K, buf)
                self.t[(layer, which)] = (Q4, buf)

    def get_tensor(self, layer, which):
        return self.t[(layer, which)] if (layer, which) in self.t else self.orc.get_tensor(layer, which)


@pytest.mark.parametrize("mix", ["all_q2k", "ftype_10", "ftype_21"])
def test_q2k_oracle_model_bit_exact_at_every_width(gpu, mix, monkeypatch):
    layout = {"all_q2k": all_q2k, "ftype_10": ftype_10, "ftype_21": ftype_21}[mix]
    hp = gpu.TINY()
    model = gpu.LlmModel(hp)
    hp = model.hparams
    cfg = oracle_cfg_from(hp, 8, 256)
    orc = O.OracleLlm(cfg, seed=4)
    src = Mixed(gpu, orc, cfg, layout)
    types = {src.get_tensor(l, w)[0] for l in range(hp.n_layer) for w in (1, 2, 3, 4, 6, 7, 8)} | {src.get_tensor(-1, 2)[0]}
    assert types == {"all_q2k": {Q2, Q6}, "ftype_10": {Q2, Q3, Q4, Q6}, "ftype_21": {Q2, Q4, Q6}}[mix]
    assert src.get_tensor(-1, 0)[0] == Q2
    install(model, src, hp.n_layer)
    check_widths(gpu, model, hp, orc, monkeypatch, mix)


def random_q2k(rng, n):
    """n Q2_K blocks with every field random and d, dmin of both signs"""
    b = rng.integers(0, 256, (n, 84), dtype=np.uint8)
    b[:, 80:82] = (rng.uniform(1e-3, 1e-2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float16).view(np.uint8).reshape(n, 2)
    b[:, 82:84] = (rng.uniform(1e-3, 1e-2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float16).view(np.uint8).reshape(n, 2)
    return b


PAIRED_ROWS, ZERO_DMIN_ROWS = slice(32, 64), slice(64, 96)   # the Q4_K- and the Q6_K-twin-able weight rows of edge_q2k


def edge_q2k(rng, rows, nb):
    """[rows][nb] Q2_K blocks: random, whole rows of edge cases, 32 rows with paired groups and 32 rows with dmin = +0"""
    b = random_q2k(rng, rows * nb).reshape(rows, nb, 84)
    b[0, :, 16:80] = 0xFF; b[0, :, 0:16] |= 0x0F                       # q = 3 and sc = 15 everywhere: operand byte 45
    b[1, :, 16:80] = 0                                                 # q = 0
    b[2, :, 0:16] &= 0xF0                                              # sc = 0
    b[3, :, 0:16] |= 0xF0                                              # m = 15
    b[4, :, 80:82] = 0                                                 # d = 0
    b[5, :, 82:84] = 0                                                 # dmin = 0
    b[6, :, 0:16:2] = 0x51; b[6, :, 1:16:2] = 0x5F                     # scales 1 | 15 in the two halves of every sub-block, one min
    b[7, :, 0:16:2] = 0x07; b[7, :, 1:16:2] = 0xF7                     # mins 0 | 15 in the two halves, one scale
    b[8, :, 0:16:2] = 0xF0; b[8, :, 1:16:2] = 0x0F                     # (sc, m) = (0, 15) | (15, 0)
    b[9, :, 80:84] = np.array([-0.0078, -0.0042], np.float16).view(np.uint8)      # negative d, dmin
    b[10, :, 80:84] = np.array([0x0001, 0x03FF], np.uint16).view(np.uint8)        # subnormal d, dmin
    b[11, :, :80] = 0xFF                                               # q = 3, sc = m = 15
    b[PAIRED_ROWS] = R.pair_groups(b[PAIRED_ROWS].reshape(-1, 84)).reshape(32, nb, 84)
    b[ZERO_DMIN_ROWS, :, 82:84] = 0
    return b.reshape(rows, nb, 84)


def q8_rows(x):
    qs, ds, _ = zip(*[O.q8k_quantize(r) for r in x])
    return np.stack(qs), np.stack(ds)


PROBE_NROWS = [1, 2, 16, 17, 32, 33, 192, 193, 256]


@pytest.fixture(scope="module")
def probe_case():
    """the probe's blocks, activations and expected results, computed once: K = 7168, 128 weight rows, 256 activation rows"""
    rng = np.random.default_rng(24)
    rows, K = 128, 7168
    b = edge_q2k(rng, rows, K // 256)
    x = rng.standard_normal((256, K)).astype(np.float32)
    x[3, 512:768] = 0.0
    q8, d8 = q8_rows(x)
    want = {ks: R.gemv(b.reshape(-1), rows, K, ks, q8, d8) for ks in (1, 4, 7)}
    return rows, K, b, x, want


@pytest.mark.parametrize("ks", [1, 4, 7])
def test_gemv_probe_q2k_equals_the_restated_contract_and_the_oracle(gpu, probe_case, ks):
    """Q2_K random and edge-case blocks through every W4A8 family and its edges (1..32 rows: mat-vec with one and two M-tiles, 33..192:
    GEMM, 193..256: 32x32x32 GEMM) and K-split 1 / 4 / 7 (28, 7 and 4 blocks per K-range: both tile depths of the mat-vec): bit for
    bit q2k_ref.gemv, and on the twin-able weight rows bit for bit oracle_lib.gemv_q8 on the Q4_K / Q6_K twins"""
    rows, K, b, x, want = probe_case
    want = want[ks]
    assert np.isfinite(want).all()
    for sl, ttype, twin in ((PAIRED_ROWS, O.TYPE_Q4_K, R.to_q4k(b[PAIRED_ROWS].reshape(-1))), (ZERO_DMIN_ROWS, O.TYPE_Q6_K, R.to_q6k(b[ZERO_DMIN_ROWS].reshape(-1)))):
        orc = np.stack([O.gemv_q8(ttype, twin, 32, K, ks, r) for r in x])
        assert np.array_equal(orc.view(np.uint32), want[:, sl].view(np.uint32)), (ttype, ks)
    for n in PROBE_NROWS:
        got = gpu.gemv_probe(Q2, b.reshape(-1), rows, K, ks, x[:n])
        bad = np.argwhere(got.view(np.uint32) != want[:n].view(np.uint32))
        assert bad.size == 0, (ks, n, len(bad), bad[:8].tolist(), np.abs(got - want[:n]).max())


class Held:
    """tensors already encoded, over an oracle that holds their twins"""

    def __init__(self, orc, t):
        self.orc, self.t = orc, t
        for (layer, which), (_, b2) in t.items():
            orc.set_tensor(layer, which, O.TYPE_Q4_K, R.to_q4k(b2))

    get_tensor = Mixed.get_tensor


_layer = {}


@pytest.mark.parametrize("nrows", [16, 256])
def test_q2k_mistral_shape_layer_bit_exact(gpu, nrows):
    """one Mistral-7B-shaped layer (production K-split plan 4/4/1/7) with all seven matrices Q2_K, against the oracle (256 rows: the
    32x32x32 kernel with the fused SwiGLU epilogue).  The 218 M weights are encoded once for both widths, by the host quantiser with
    the (scale, min) of every even group copied to its odd neighbour: valid paired-group blocks at a fraction of the NumPy encoder's time"""
    hp = gpu.MISTRAL_7B()
    hp.n_layer = 1
    model = gpu.LlmModel(hp)
    hp = model.hparams
    assert (hp.ks_qkv, hp.ks_o, hp.ks_gateup, hp.ks_down) == (4, 4, 1, 7)
    cfg = oracle_cfg_from(hp, 4, nrows)
    orc = O.OracleLlm(cfg, seed=4)
    if not _layer:
        _layer.update(Mixed(gpu, orc, cfg, q2_matrices, encode=lambda w: R.pair_groups(gpu.quantize_blocks(Q2, w))).t)
    src = Held(orc, _layer)
    assert {src.get_tensor(0, w)[0] for w in (1, 2, 3, 4, 6, 7, 8)} == {Q2}
    install(model, src, 1)
    sess = gpu.LlmSession(model, nrows, 4)
    seq = np.arange(nrows, dtype=np.int32)
    tok = np.random.default_rng(2).integers(3, hp.vocab, nrows).astype(np.int32)
    want, wam = orc.forward(seq, np.zeros(nrows, np.int32), tok)
    got, gam = sess.forward(seq, np.zeros(nrows, np.int32), tok)
    assert np.isfinite(want).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.abs(got - want).max()
    assert np.array_equal(gam, wam)


def test_q2k_embedding_with_random_bytes_bit_exact(gpu):
    """token_embd as Q2_K blocks of random bytes on the GPU; the oracle gets the same rows as F32 values from the NumPy decode
    (tests/q2k_ref.py, pinned to the layout on the CPU): k_embed's Q2_K decode must give the same bits"""
    hp = gpu.TINY()
    model = gpu.LlmModel(hp)
    hp = model.hparams
    orc = O.OracleLlm(oracle_cfg_from(hp, 8, 16), seed=4)
    install(model, orc, hp.n_layer)
    emb = random_q2k(np.random.default_rng(3), hp.vocab * hp.d_model // 256)
    model.set_tensor(-1, O.T_TOKEN_EMBD, Q2, emb.reshape(-1))
    orc.set_tensor(-1, O.T_TOKEN_EMBD, O.TYPE_F32, R.dequant(emb).reshape(-1))
    sess = gpu.LlmSession(model, 16, 8)
    seq = np.arange(16, dtype=np.int32)
    tok = np.random.default_rng(4).integers(3, hp.vocab, 16).astype(np.int32)
    want, wam = orc.forward(seq, np.zeros(16, np.int32), tok)
    got, gam = sess.forward(seq, np.zeros(16, np.int32), tok)
    assert np.isfinite(want).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.abs(got - want).max()
    assert np.array_equal(gam, wam)


def test_q2k_gguf_logits_bit_exact_at_every_width(gpu, tmp_path, monkeypatch):
    """a Q2_K-layout GGUF (Q2_K beside Q3_K, Q4_K and Q6_K tensors) loaded by tk_mi355x_llm_model_load_gguf: the Q2_K tensors keep their
    84-byte blocks through the reader, and the logits are the oracle's at every width"""
    cfg = O.tiny_config()
    path = str(tmp_path / "tiny_q2k.gguf")
    gguf_util.write_llama_gguf(path, Mixed(gpu, O.OracleLlm(cfg, seed=4), cfg, ftype_10), cfg)
    model = gpu.LlmModel(gguf=path)
    hp = model.hparams
    cfg2 = oracle_cfg_from(hp, 8, 256)  # the K-split plan the loader chose
    orc = O.OracleLlm(cfg2, seed=4)
    Mixed(gpu, orc, cfg2, ftype_10)     # the same seed and mix: the oracle now holds the file's weights
    check_widths(gpu, model, hp, orc, monkeypatch, "gguf q2_k")


def test_q2k_gguf_checkpoint_end_to_end(gpu, tmp_path):
    """the same file through tk_model_loader + tk_llm_runner: the oracle's token ids"""
    cfg = O.tiny_config()
    path = str(tmp_path / "tiny_q2k.gguf")
    gguf_util.write_llama_gguf(path, Mixed(gpu, O.OracleLlm(cfg, seed=4), cfg, ftype_10), cfg)
    loader = gpu.ModelLoader()
    h = loader.load(path)
    hp = gpu.LlmHParams()
    gpu.lib().tk_mi355x_llm_model_get_hparams(h, C.byref(hp))
    cfg2 = oracle_cfg_from(hp, 64, 1)
    orc = O.OracleLlm(cfg2, seed=4)
    Mixed(gpu, orc, cfg2, ftype_10)
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


def recipe_bytes(hp, layout):
    """the matrix bytes a decode step streams under a layout: every layer matrix plus output (Q6_K), at the installed bytes per block"""
    cfg = oracle_cfg_from(hp, 4, 1)
    total = hp.vocab * hp.d_model // 256 * BLOCK_BYTES_INSTALLED[Q6]
    for l in range(hp.n_layer):
        for w, (r, c) in shapes(cfg).items():
            total += r * c // 256 * BLOCK_BYTES_INSTALLED[layout(l, w, cfg)]
    return total


@pytest.fixture(scope="module")
def q4km_logits():
    return {}


@pytest.mark.parametrize("ftype", [10, 21])
def test_q2k_synthetic_width_and_batch_invariance(gpu, ftype, q4km_logits):
    """a 2-layer Mistral-shaped Q2_K / Q2_K_S model gives the same logits bits as 1 x 256, 2 x 128, 8 x 32, 16 x 16 and 256 x 1 passes
    (every kernel family, fused producers at one row), over two positions through the KV cache; two fills with one seed are identical;
    the logits are not the Q4_K_M model's; weight_bytes is the sum the recipe implies"""
    hp = gpu.MISTRAL_7B()
    hp.n_layer = 2
    model = gpu.LlmModel(hp).fill_synthetic(4, ftype=ftype)
    hp = model.hparams
    assert model.weight_bytes == recipe_bytes(hp, {10: ftype_10, 21: ftype_21}[ftype])
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
    if "q4km" not in q4km_logits:
        q4km_logits["q4km"] = logits_in_passes(gpu, gpu.LlmModel(hp).fill_synthetic(4, ftype=gpu.FTYPE_Q4_K_M), hp, 256, toks)[0]
    assert not np.array_equal(q4km_logits["q4km"], ref[0])


def test_q2k_ftype_constants_loader_names_and_refused_ftypes(gpu):
    assert (gpu.FTYPE_Q2_K, gpu.FTYPE_Q2_K_S, gpu.TYPE_Q2_K) == (10, 21, 10)
    hp = gpu.TINY()
    a = gpu.LlmModel(hp).fill_synthetic(9, ftype=gpu.FTYPE_Q2_K)
    s = gpu.LlmModel(hp).fill_synthetic(9, ftype=gpu.FTYPE_Q2_K_S)
    k = gpu.LlmModel(hp).fill_synthetic(9, ftype=gpu.FTYPE_Q4_K_M)
    assert a.weight_bytes == recipe_bytes(a.hparams, ftype_10) and s.weight_bytes == recipe_bytes(s.hparams, ftype_21)
    assert s.weight_bytes < a.weight_bytes < k.weight_bytes
    for bad in (13, 9, 20, 22):
        with pytest.raises(gpu.TkError):
            gpu.LlmModel(hp).fill_synthetic(9, ftype=bad)
    # synthetic://tiny-q2k and -q2ks are the loader's names for the two recipes
    loader = gpu.ModelLoader()
    for name, want in (("synthetic://tiny-q2k?seed=9", a), ("synthetic://tiny-q2ks?seed=9", s)):
        h = loader.load(name)
        wb = gpu.lib().tk_mi355x_llm_model_weight_bytes
        wb.restype = C.c_uint64
        assert wb(h) == want.weight_bytes
        loader.unload(h)
    loader.close()


def test_lora_into_a_q2k_matrix_fails_the_load(gpu, tmp_path):
    hp = gpu.TINY()
    rng = np.random.default_rng(1)
    D = hp.d_model
    kvd = hp.n_kv_head * hp.head_dim
    factors = {(0, 3): (rng.standard_normal((4, D)).astype(np.float32) * 0.01, rng.standard_normal((kvd, 4)).astype(np.float32) * 0.01)}
    ad = str(tmp_path / "v.gguf")
    gguf_util.write_lora_gguf(ad, 8.0, factors)
    model = gpu.LlmModel(hp)
    model.set_lora(ad)
    blocks = gpu.quantize_blocks(Q2, (rng.standard_normal((kvd, D)) * 0.02).astype(np.float32))
    with pytest.raises(gpu.TkError) as ei:
        model.set_tensor(0, 3, Q2, blocks.reshape(-1))
    assert "Q2_K" in str(ei.value)
