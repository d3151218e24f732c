"""GPU: Q8_0 weights (GGML type 8) on the W4A8 kernels, and Q6_K token embeddings, bit for bit.  The oracle has no Q8_0, and its Q6_K
does one fmaf per 256 weights where Q8_0 does eight.  One restatement and one twin pin the type (tests/q8_0_ref.py, held against the
oracle on the CPU by tests/test_q8_0_cpu.py): general blocks are held against q8_0_ref.gemv, the contract restated with an exact fmaf,
and a 256-k run with seven of its eight d equal to +0 and the live block's quants in -32..31 is a Q6_K block the oracle runs."""
import ctypes as C

import numpy as np
import pytest

import gguf_util
import oracle_lib as O
import q8_0_ref as R
from kquant_gpu_util import check_widths, install, logits_in_passes, oracle_cfg_from, shapes

pytestmark = pytest.mark.gpu

Q8, Q6 = 8, 14
INSTALLED_BYTES_PER_256 = 272   # a Q8_0 matrix is held as 4352-byte tiles of 16 rows x 256 k: eight 34-byte blocks per row and run


class TwinSparse:
    """Every matrix, output and token_embd of an oracle model as twin-able Q8_0 blocks made from the oracle's dequantised weights; the
    ORACLE IS CHANGED to hold exactly the same weights: the Q6_K twins (token_embd: the NumPy-decoded F32 rows).  Norms stay."""

    def __init__(self, orc, cfg, with_embd=True, with_output=True):
        self.orc, self.t = orc, {}
        todo = [(l, w, r, c) for l in range(cfg.n_layer) for w, (r, c) in shapes(cfg).items()]
        if with_output:
            todo.append((-1, O.T_OUTPUT, cfg.vocab, cfg.d_model))
        if with_embd:
            todo.append((-1, O.T_TOKEN_EMBD, cfg.vocab, cfg.d_model))
        for layer, which, rows, cols in todo:
            b = R.quantize_twin_sparse(orc.dequant(layer, which, rows, cols), seed=1000 * (layer + 1) + which)
            self.t[(layer, which)] = (Q8, b.reshape(-1))
        hold_twins(orc, self.t)

    def get_tensor(self, layer, which):
        return self.t[(layer, which)] if (layer, which) in self.t else self.orc.get_tensor(layer, which)


def hold_twins(orc, t):
    for (layer, which), (_, b) in t.items():
        if layer < 0 and which == O.T_TOKEN_EMBD:
            orc.set_tensor(layer, which, O.TYPE_F32, R.dequant(b).reshape(-1))
        else:
            orc.set_tensor(layer, which, O.TYPE_Q6_K, R.to_q6k(b))


def test_q8_0_twin_sparse_model_bit_exact_at_every_width(gpu, monkeypatch):
    """a whole tiny model with every matrix, output and token_embd Q8_0 (twin-sparse), against the oracle holding the Q6_K twins: every
    width of WIDTHS, both fuse settings"""
    hp = gpu.TINY()
    model = gpu.LlmModel(hp)
    hp = model.hparams
    cfg = oracle_cfg_from(hp, 8, 256)
    orc = O.OracleLlm(cfg, seed=4)
    src = TwinSparse(orc, cfg)
    assert {src.get_tensor(l, w)[0] for l in range(hp.n_layer) for w in (1, 2, 3, 4, 6, 7, 8)} | {src.get_tensor(-1, 0)[0], src.get_tensor(-1, 2)[0]} == {Q8}
    install(model, src, hp.n_layer)
    check_widths(gpu, model, hp, orc, monkeypatch, "twin-sparse q8_0")


def random_q8_0(rng, n):
    """n Q8_0 blocks with random quant bytes (every int8 value) and d of both signs"""
    b = rng.integers(0, 256, (n, 34), dtype=np.uint8)
    b[:, 0:2] = (rng.uniform(1e-3, 1e-2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float16).view(np.uint8).reshape(n, 2)
    return b


TWIN_ROWS = slice(32, 64)   # the Q6_K-twin-able weight rows of edge_q8_0


def edge_q8_0(rng, rows, nb):
    """[rows][nb runs][8 blocks] Q8_0: random, whole rows of edge cases, and 32 twin-able rows"""
    b = random_q8_0(rng, rows * nb * 8).reshape(rows, nb, 8, 34)
    f16 = lambda v: np.array(v, np.float16).view(np.uint8)
    b[0, :, :, 2:] = 0x7F                                               # q = 127 everywhere
    b[1, :, :, 2:] = 0x80                                               # q = -128 everywhere
    b[2, :, :, 2:] = 0                                                  # q = 0
    b[3, :, :, 0:2] = 0                                                 # d = 0
    b[4, :, :, 0:2] = f16([-0.0078])                                    # negative d
    b[5, :, :, 0:2] = np.array([0x0001], np.uint16).view(np.uint8)      # subnormal d
    b[5, :, 1::2, 0:2] = np.array([0x83FF], np.uint16).view(np.uint8)   # ... and a negative one
    # d alternating in sign and by 2^10 in magnitude between neighbouring 32-blocks: a scale taken 64 or 256 wide gives other bits
    b[6, :, 0::2, 0:2] = f16([2.0 ** -4])
    b[6, :, 1::2, 0:2] = f16([-(2.0 ** -14)])
    b[7, :, :, 0:2] = 0                                                 # one live block per run, at a position that walks with the run
    for r in range(nb):
        b[7, r, (3 * r + 1) % 8, 0:2] = f16([0.0061])
    n = 32 * nb
    live = rng.integers(0, 8, n)
    t = b[TWIN_ROWS].reshape(n, 8, 34)
    t[:, :, 0:2] = 0
    t[np.arange(n), live, 0:2] = (rng.uniform(1e-3, 1e-2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float16).view(np.uint8).reshape(n, 2)
    t[np.arange(n), live, 2:] = rng.integers(-32, 32, (n, 32)).astype(np.int8).view(np.uint8)
    b[TWIN_ROWS] = t.reshape(32, nb, 8, 34)
    return b


def q8_rows(x):
    qs, ds, _ = zip(*[O.q8k_quantize(r) for r in x])
    return np.stack(qs), np.stack(ds).reshape(len(x), -1)


PROBE_NROWS = [1, 2, 16, 17, 32, 33, 192, 193, 256]


@pytest.fixture(scope="module")
def probe_case():
    """the probe's blocks, activations and expected results, computed once: K = 7168, 128 weight rows, 256 activation rows"""
    rng = np.random.default_rng(80)
    rows, K = 128, 7168
    b = edge_q8_0(rng, rows, K // 256)
    x = rng.standard_normal((256, K)).astype(np.float32)
    x[3, 512:768] = 0.0                                                 # one activation run all zero
    q8, d8 = q8_rows(x)
    want = {ks: R.gemv(b.reshape(-1), rows, K, ks, q8, d8) for ks in (1, 4, 7)}
    return rows, K, b, x, want


@pytest.mark.parametrize("ks", [1, 4, 7])
def test_gemv_probe_q8_0_equals_the_restated_contract_and_the_oracle(gpu, probe_case, ks):
    """Q8_0 random and edge-case blocks through every W4A8 family and its edges (1..32 rows: mat-vec with one and two M-tiles — K-split 1
    has 28 runs per range and takes the K-streamed kernel —, 33..192: GEMM, 193..256: 32x32x32 GEMM) and K-split 1 / 4 / 7: bit for bit
    q8_0_ref.gemv, and on the twin-able weight rows bit for bit oracle_lib.gemv_q8 on the Q6_K twins"""
    rows, K, b, x, want = probe_case
    want = want[ks]
    assert np.isfinite(want).all()
    twin = R.to_q6k(b[TWIN_ROWS].reshape(-1))
    orc = np.stack([O.gemv_q8(O.TYPE_Q6_K, twin, 32, K, ks, r) for r in x])
    assert np.array_equal(orc.view(np.uint32), want[:, TWIN_ROWS].view(np.uint32)), ks
    for n in PROBE_NROWS:
        got = gpu.gemv_probe(Q8, b.reshape(-1), rows, K, ks, x[:n])
        bad = np.argwhere(got.view(np.uint32) != want[:n].view(np.uint32))
        assert bad.size == 0, (ks, n, len(bad), bad[:8].tolist(), np.abs(got - want[:n]).max())


def test_q8_0_synthetic_width_invariance_and_recipe(gpu):
    """synthetic ftype 7 on the tiny geometry — general Q8_0 blocks from the host quantiser's device twin in every matrix, output and
    token_embd: the same logits bits as 1 x 256, 2 x 128, 8 x 32, 16 x 16 and 256 x 1 passes (every kernel family, fused producers at one
    row), two positions through the KV cache; two fills with one seed are identical; the logits are not the Q4_K_M model's; weight_bytes
    is the sum the recipe implies; synthetic://tiny-q80 is the loader's name for it; the other ftypes stay refused"""
    assert (gpu.FTYPE_Q8_0, gpu.TYPE_Q8_0) == (7, 8)
    hp = gpu.TINY()
    model = gpu.LlmModel(hp).fill_synthetic(4, ftype=gpu.FTYPE_Q8_0)
    hp = model.hparams
    cfg = oracle_cfg_from(hp, 4, 1)
    want_bytes = (hp.vocab * hp.d_model + sum(r * c for r, c in shapes(cfg).values()) * hp.n_layer) // 256 * INSTALLED_BYTES_PER_256
    assert model.weight_bytes == want_bytes
    rng = np.random.default_rng(7)
    toks = [rng.integers(3, hp.vocab, 256).astype(np.int32) for _ in range(2)]
    ref = logits_in_passes(gpu, model, hp, 256, toks)
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()
    for width in (128, 32, 16, 1):
        got = logits_in_passes(gpu, model, hp, width, toks)
        for p in range(2):
            assert np.array_equal(got[p].view(np.uint32), ref[p].view(np.uint32)), (width, p)
    again = gpu.LlmModel(hp).fill_synthetic(4, ftype=gpu.FTYPE_Q8_0)
    got = logits_in_passes(gpu, again, hp, 256, toks)
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32))
    q4km = logits_in_passes(gpu, gpu.LlmModel(hp).fill_synthetic(4, ftype=gpu.FTYPE_Q4_K_M), hp, 256, toks)[0]
    assert not np.array_equal(q4km, ref[0])
    for bad in (0, 9, 13, 18, 20, 22):
        with pytest.raises(gpu.TkError):
            gpu.LlmModel(hp).fill_synthetic(9, ftype=bad)
    loader = gpu.ModelLoader()
    h = loader.load("synthetic://tiny-q80?seed=4")
    wb = gpu.lib().tk_mi355x_llm_model_weight_bytes
    wb.restype = C.c_uint64
    assert wb(h) == want_bytes
    loader.unload(h)
    loader.close()


class Held:
    """tensors already encoded, over an oracle that is given their twins"""

    def __init__(self, orc, t):
        self.orc, self.t = orc, t
        hold_twins(orc, t)

    get_tensor = TwinSparse.get_tensor


_layer = {}


@pytest.mark.parametrize("nrows", [16, 256])
def test_q8_0_mistral_shape_layer_bit_exact(gpu, nrows):
    """one Mistral-7B-shaped layer (production K-split plan 4/4/1/7) with all seven matrices Q8_0 (twin-sparse), against the oracle (256
    rows: the 32x32x32 kernel with the fused SwiGLU epilogue).  The 218 M weights are encoded once for both widths"""
    hp = gpu.MISTRAL_7B()
    hp.n_layer = 1
    model = gpu.LlmModel(hp)
    hp = model.hparams
    assert (hp.ks_qkv, hp.ks_o, hp.ks_gateup, hp.ks_down) == (4, 4, 1, 7)
    cfg = oracle_cfg_from(hp, 4, nrows)
    orc = O.OracleLlm(cfg, seed=4)
    if not _layer:
        _layer.update(TwinSparse(orc, cfg, with_embd=False, with_output=False).t)
    src = Held(orc, _layer)
    assert {src.get_tensor(0, w)[0] for w in (1, 2, 3, 4, 6, 7, 8)} == {Q8}
    install(model, src, 1)
    sess = gpu.LlmSession(model, nrows, 4)
    seq = np.arange(nrows, dtype=np.int32)
    tok = np.random.default_rng(2).integers(3, hp.vocab, nrows).astype(np.int32)
    want, wam = orc.forward(seq, np.zeros(nrows, np.int32), tok)
    got, gam = sess.forward(seq, np.zeros(nrows, np.int32), tok)
    assert np.isfinite(want).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.abs(got - want).max()
    assert np.array_equal(gam, wam)


def test_q8_0_embedding_with_random_bytes_bit_exact(gpu):
    """token_embd as Q8_0 blocks of random bytes on the GPU; the oracle gets the same rows as F32 values from the NumPy decode
    (tests/q8_0_ref.py, pinned on the CPU): k_embed's Q8_0 decode must give the same bits"""
    hp = gpu.TINY()
    model = gpu.LlmModel(hp)
    hp = model.hparams
    orc = O.OracleLlm(oracle_cfg_from(hp, 8, 16), seed=4)
    install(model, orc, hp.n_layer)
    emb = random_q8_0(np.random.default_rng(3), hp.vocab * hp.d_model // 32)
    model.set_tensor(-1, O.T_TOKEN_EMBD, Q8, emb.reshape(-1))
    orc.set_tensor(-1, O.T_TOKEN_EMBD, O.TYPE_F32, R.dequant(emb).reshape(-1))
    sess = gpu.LlmSession(model, 16, 8)
    seq = np.arange(16, dtype=np.int32)
    tok = np.random.default_rng(4).integers(3, hp.vocab, 16).astype(np.int32)
    want, wam = orc.forward(seq, np.zeros(16, np.int32), tok)
    got, gam = sess.forward(seq, np.zeros(16, np.int32), tok)
    assert np.isfinite(want).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.abs(got - want).max()
    assert np.array_equal(gam, wam)


class AllQ6K:
    """every matrix, output and token_embd re-quantised to Q6_K by the oracle's quantiser; the ORACLE IS CHANGED to hold the same blocks
    (a Q6_K token_embd too)"""

    def __init__(self, orc, cfg):
        self.orc = orc
        todo = [(-1, O.T_TOKEN_EMBD, cfg.vocab, cfg.d_model), (-1, O.T_OUTPUT, cfg.vocab, cfg.d_model)]
        todo += [(l, w, r, c) for l in range(cfg.n_layer) for w, (r, c) in shapes(cfg).items()]
        for layer, which, rows, cols in todo:
            if orc.get_tensor(layer, which)[0] != O.TYPE_Q6_K:
                orc.set_tensor(layer, which, O.TYPE_Q6_K, O.quantize_rows(O.TYPE_Q6_K, orc.dequant(layer, which, rows, cols)))

    def get_tensor(self, layer, which):
        return self.orc.get_tensor(layer, which)


def mix_of(kind, orc, cfg):
    return TwinSparse(orc, cfg) if kind == "q8_0" else AllQ6K(orc, cfg)


@pytest.mark.parametrize("kind", ["q8_0", "q6_k"])
def test_gguf_of_one_type_logits_bit_exact_at_every_width(gpu, tmp_path, monkeypatch, kind):
    """an all-Q8_0 GGUF (twin-sparse) and an all-Q6_K GGUF whose token_embd is Q6_K, loaded by tk_mi355x_llm_model_load_gguf: the logits
    are those of the oracle holding the same weights, at every width"""
    cfg = O.tiny_config()
    path = str(tmp_path / f"tiny_{kind}.gguf")
    src = mix_of(kind, O.OracleLlm(cfg, seed=4), cfg)
    want_type = Q8 if kind == "q8_0" else Q6
    assert {src.get_tensor(-1, 0)[0], src.get_tensor(-1, 2)[0]} | {src.get_tensor(l, w)[0] for l in range(cfg.n_layer) for w in (1, 2, 3, 4, 6, 7, 8)} == {want_type}
    gguf_util.write_llama_gguf(path, src, cfg)
    model = gpu.LlmModel(gguf=path)
    hp = model.hparams
    cfg2 = oracle_cfg_from(hp, 8, 256)  # the K-split plan the loader chose
    orc = O.OracleLlm(cfg2, seed=4)
    mix_of(kind, orc, cfg2)             # the same seed and mix: the oracle now holds the file's weights
    check_widths(gpu, model, hp, orc, monkeypatch, f"gguf {kind}")


@pytest.mark.parametrize("kind", ["q8_0", "q6_k"])
def test_gguf_of_one_type_end_to_end(gpu, tmp_path, kind):
    """the same files through tk_model_loader + tk_llm_runner: the oracle's token ids"""
    cfg = O.tiny_config()
    path = str(tmp_path / f"tiny_{kind}.gguf")
    gguf_util.write_llama_gguf(path, mix_of(kind, O.OracleLlm(cfg, seed=4), cfg), cfg)
    loader = gpu.ModelLoader()
    h = loader.load(path)
    hp = gpu.LlmHParams()
    gpu.lib().tk_mi355x_llm_model_get_hparams(h, C.byref(hp))
    cfg2 = oracle_cfg_from(hp, 64, 1)
    orc = O.OracleLlm(cfg2, seed=4)
    mix_of(kind, orc, cfg2)
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


def test_lora_into_a_q8_0_matrix_fails_the_load(gpu, tmp_path):
    hp = gpu.TINY()
    rng = np.random.default_rng(1)
    D = hp.d_model
    kvd = hp.n_kv_head * hp.head_dim
    factors = {(0, 3): (rng.standard_normal((4, D)).astype(np.float32) * 0.01, rng.standard_normal((kvd, 4)).astype(np.float32) * 0.01)}
    ad = str(tmp_path / "v.gguf")
    gguf_util.write_lora_gguf(ad, 8.0, factors)
    model = gpu.LlmModel(hp)
    model.set_lora(ad)
    blocks = gpu.quantize_blocks(Q8, (rng.standard_normal((kvd, D)) * 0.02).astype(np.float32))
    with pytest.raises(gpu.TkError) as ei:
        model.set_tensor(0, 3, Q8, blocks.reshape(-1))
    assert "LoRA merge" in str(ei.value) and "Q8_0 matrix is not built" in str(ei.value)
