"""GPU: Q4_0 and Q5_0 weights (GGML types 2 and 6) on the W4A8 kernels, bit for bit.  A block of either type IS the Q8_0 block with the
same d and q8 = q - 8 / q - 16, so both are pinned to what the project already trusts (tests/q4_0_ref.py, held against the oracle on the
CPU by tests/test_q4_0_q5_0_cpu.py): general blocks against the restated contract and against the probe's own output for their Q8_0
twins, twin-sparse runs (one live block, seven with d = +0) against the oracle running their Q6_K twins."""
import ctypes as C

import numpy as np
import pytest

import gguf_util
import oracle_lib as O
import q4_0_ref as R
from kquant_gpu_util import check_widths, install, logits_in_passes, oracle_cfg_from, shapes

pytestmark = pytest.mark.gpu

TYPES = [R.Q4_0, R.Q5_0]
NAME = {R.Q4_0: "Q4_0", R.Q5_0: "Q5_0"}
FTYPE = {R.Q4_0: 2, R.Q5_0: 8}
INSTALLED_BYTES_PER_256 = {R.Q4_0: 144, R.Q5_0: 176, 14: 210}   # tiles of 16 rows x 256 k: eight 18- / 22-byte blocks per row and run


class TwinSparse:
    """Every layer matrix and token_embd of an oracle model as twin-sparse blocks of `ttype` made from the oracle's dequantised weights;
    output stays the oracle's Q6_K.  The ORACLE IS CHANGED to hold exactly the same weights: the Q6_K twins (token_embd: the
    NumPy-decoded F32 rows).  Norms stay."""

    def __init__(self, ttype, orc, cfg):
        self.orc, self.t = orc, {}
        assert orc.get_tensor(-1, O.T_OUTPUT)[0] == O.TYPE_Q6_K
        todo = [(l, w, r, c) for l in range(cfg.n_layer) for w, (r, c) in shapes(cfg).items()]
        todo.append((-1, O.T_TOKEN_EMBD, cfg.vocab, cfg.d_model))
        for layer, which, rows, cols in todo:
            b = R.quantize_twin_sparse(ttype, orc.dequant(layer, which, rows, cols), seed=1000 * (layer + 1) + which)
            self.t[(layer, which)] = (ttype, b.reshape(-1))
        for (layer, which), (_, b) in self.t.items():
            if layer < 0:
                orc.set_tensor(layer, which, O.TYPE_F32, R.dequant(ttype, b).reshape(-1))
            else:
                orc.set_tensor(layer, which, O.TYPE_Q6_K, R.to_q6k(ttype, b))

    def get_tensor(self, layer, which):
        return self.t[(layer, which)] if (layer, which) in self.t else self.orc.get_tensor(layer, which)

    def types(self, n_layer):
        return {self.get_tensor(l, w)[0] for l in range(n_layer) for w in (1, 2, 3, 4, 6, 7, 8)} | {self.get_tensor(-1, 0)[0]}


@pytest.mark.parametrize("ttype", TYPES)
def test_twin_sparse_model_bit_exact_at_every_width(gpu, monkeypatch, ttype):
    """a whole tiny model with every layer matrix and token_embd twin-sparse in the type and output Q6_K, against the oracle holding the
    twins: every width of WIDTHS, both fuse settings"""
    hp = gpu.TINY()
    model = gpu.LlmModel(hp)
    hp = model.hparams
    cfg = oracle_cfg_from(hp, 8, 256)
    orc = O.OracleLlm(cfg, seed=4)
    src = TwinSparse(ttype, orc, cfg)
    assert src.types(hp.n_layer) == {ttype} and src.get_tensor(-1, O.T_OUTPUT)[0] == 14
    install(model, src, hp.n_layer)
    check_widths(gpu, model, hp, orc, monkeypatch, f"twin-sparse {NAME[ttype]}")


def random_blocks(ttype, rng, n):
    """n blocks with random quant bytes (every nibble, every qh bit) and d of both signs"""
    b = rng.integers(0, 256, (n, R.BYTES[ttype]), dtype=np.uint8)
    b[:, 0:2] = (rng.uniform(1e-3, 1e-2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float16).view(np.uint8).reshape(n, 2)
    return b


TWIN_ROWS = slice(32, 64)   # the twin-sparse weight rows of edge_blocks


def edge_blocks(ttype, rng, rows, nb):
    """[rows][nb runs][8 blocks]: random, whole rows of edge cases, and 32 twin-sparse rows"""
    nbytes, qs = R.BYTES[ttype], R.QS_AT[ttype]
    b = random_blocks(ttype, rng, rows * nb * 8).reshape(rows, nb, 8, nbytes)
    f16 = lambda v: np.array(v, np.float16).view(np.uint8)
    b[0, :, :, 2:] = 0                                                  # q = 0 everywhere
    b[1, :, :, 2:] = 0xFF                                               # q = 15 / 31 everywhere
    if ttype == R.Q4_0:
        b[2, :, :, 2:] = 0x88                                           # q = z = 8: every weight 0
    else:
        b[2, :, :, 2:6] = 0xFF                                          # q = z = 16: the high bit alone
        b[2, :, :, 6:] = 0
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
    b[8, :, :, qs:] = 0xF0                                              # weights 0..15 = 0, weights 16..31 = 15: nibble order
    b[9, :, :, qs:] = 0x0F
    b[10, :, :, qs:qs + 8] = 0x21                                       # ... and the order inside each half
    b[10, :, :, qs + 8:] = 0x43
    if ttype == R.Q5_0:
        u32 = lambda v: np.array([v], "<u4").view(np.uint8)
        b[11, :, :, 2:6] = u32(0x0000FFFF)
        b[12, :, :, 2:6] = u32(0xFFFF0000)
        b[13, :, :, 2:6] = u32(0xAAAAAAAA)
        for r in range(nb):
            for j in range(8):
                b[14, r, j, 2:6] = u32(1 << ((8 * r + j) % 32))        # a single walking bit
        b[8, :, :, 2:6] = u32(0x0000FFFF)                               # rows 8, 9: the two halves differ in the high bit too
        b[9, :, :, 2:6] = u32(0xFFFF0000)
    w = (rng.standard_normal((32, nb * 256)) * 0.02).astype(np.float32)
    b[TWIN_ROWS] = R.quantize_twin_sparse(ttype, w, seed=9).reshape(32, nb, 8, nbytes)
    return b


def q8_rows(x):
    qs, ds, _ = zip(*[O.q8k_quantize(r) for r in x])
    return np.stack(qs), np.stack(ds).reshape(len(x), -1)


PROBE_NROWS = [1, 2, 16, 17, 32, 33, 192, 193, 256]
_probe = {}


def probe_case(ttype):
    """the probe's blocks, activations and expected results, computed once per type: K = 7168, 128 weight rows, 256 activation rows"""
    if ttype not in _probe:
        rng = np.random.default_rng(40 + ttype)
        rows, K = 128, 7168
        b = edge_blocks(ttype, rng, rows, K // 256)
        x = rng.standard_normal((256, K)).astype(np.float32)
        x[3, 512:768] = 0.0                                             # one activation run all zero
        q8, d8 = q8_rows(x)
        want = {ks: R.gemv(ttype, b.reshape(-1), rows, K, ks, q8, d8) for ks in (1, 4, 7)}
        _probe[ttype] = (rows, K, b, x, want)
    return _probe[ttype]


@pytest.mark.parametrize("ks", [1, 4, 7])
@pytest.mark.parametrize("ttype", TYPES)
def test_gemv_probe_equals_the_restated_contract_the_oracle_and_the_q8_0_twin(gpu, ttype, ks):
    """random and edge-case blocks through every W4A8 family and its edges (1..32 rows: mat-vec with one and two M-tiles — K-split 1 has
    28 runs per range and takes the K-streamed kernel —, 33..192: GEMM, 193..256: 32x32x32 GEMM) and K-split 1 / 4 / 7: bit for bit the
    restatement, on the twin-sparse rows bit for bit oracle_lib.gemv_q8 on the Q6_K twins, and bit for bit the probe's own output for the
    Q8_0 twin blocks (type 8) at the same shapes"""
    rows, K, b, x, want = probe_case(ttype)
    want = want[ks]
    assert np.isfinite(want).all()
    twin6 = R.to_q6k(ttype, b[TWIN_ROWS].reshape(-1))
    orc = np.stack([O.gemv_q8(O.TYPE_Q6_K, twin6, 32, K, ks, r) for r in x])
    assert np.array_equal(orc.view(np.uint32), want[:, TWIN_ROWS].view(np.uint32)), ks
    twin8 = R.to_q8_0(ttype, b.reshape(-1))
    for n in PROBE_NROWS:
        got = gpu.gemv_probe(ttype, b.reshape(-1), rows, K, ks, x[:n])
        bad = np.argwhere(got.view(np.uint32) != want[:n].view(np.uint32))
        assert bad.size == 0, (ks, n, len(bad), bad[:8].tolist(), np.abs(got - want[:n]).max())
        got8 = gpu.gemv_probe(8, twin8.reshape(-1), rows, K, ks, x[:n])
        assert np.array_equal(got.view(np.uint32), got8.view(np.uint32)), (ks, n)


def recipe_bytes(hp, cfg, ttype):
    return (hp.vocab * hp.d_model // 256 * INSTALLED_BYTES_PER_256[14] +
            sum(r * c for r, c in shapes(cfg).values()) * hp.n_layer // 256 * INSTALLED_BYTES_PER_256[ttype])


@pytest.mark.parametrize("ttype", TYPES)
def test_synthetic_width_invariance_and_recipe(gpu, ttype):
    """synthetic ftype 2 / 8 on the tiny geometry — general blocks from the host quantiser's device twin in every layer matrix and
    token_embd, output Q6_K: the same logits bits as 1 x 256, 2 x 128, 8 x 32, 16 x 16 and 256 x 1 passes (every kernel family, fused
    producers at one row), two positions through the KV cache; two fills with one seed are identical; the logits are not the Q4_K_M
    model's nor the other type's; weight_bytes is the sum the recipe implies; synthetic://tiny-q40 / -q50 is the loader's name for it;
    the other ftypes stay refused"""
    assert (gpu.FTYPE_Q4_0, gpu.TYPE_Q4_0, gpu.FTYPE_Q5_0, gpu.TYPE_Q5_0) == (2, 2, 8, 6)
    hp = gpu.TINY()
    model = gpu.LlmModel(hp).fill_synthetic(4, ftype=FTYPE[ttype])
    hp = model.hparams
    cfg = oracle_cfg_from(hp, 4, 1)
    want_bytes = recipe_bytes(hp, cfg, ttype)
    assert model.weight_bytes == want_bytes
    rng = np.random.default_rng(7)
    toks = [rng.integers(3, hp.vocab, 256).astype(np.int32) for _ in range(2)]
    ref = logits_in_passes(gpu, model, hp, 256, toks)
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()
    for width in (128, 32, 16, 1):
        got = logits_in_passes(gpu, model, hp, width, toks)
        for p in range(2):
            assert np.array_equal(got[p].view(np.uint32), ref[p].view(np.uint32)), (width, p)
    again = gpu.LlmModel(hp).fill_synthetic(4, ftype=FTYPE[ttype])
    got = logits_in_passes(gpu, again, hp, 256, toks)
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32))
    q4km = logits_in_passes(gpu, gpu.LlmModel(hp).fill_synthetic(4, ftype=gpu.FTYPE_Q4_K_M), hp, 256, toks)[0]
    assert not np.array_equal(q4km, ref[0])
    other = R.Q5_0 if ttype == R.Q4_0 else R.Q4_0
    om = gpu.LlmModel(hp).fill_synthetic(4, ftype=FTYPE[other])
    assert om.weight_bytes == recipe_bytes(hp, cfg, other) != want_bytes
    assert not np.array_equal(logits_in_passes(gpu, om, hp, 256, toks)[0], ref[0])
    for bad in (0, 3, 9, 13, 18, 20, 22):
        with pytest.raises(gpu.TkError):
            gpu.LlmModel(hp).fill_synthetic(9, ftype=bad)
    loader = gpu.ModelLoader()
    h = loader.load("synthetic://tiny-q40?seed=4" if ttype == R.Q4_0 else "synthetic://tiny-q50?seed=4")
    wb = gpu.lib().tk_mi355x_llm_model_weight_bytes
    wb.restype = C.c_uint64
    assert wb(h) == want_bytes
    loader.unload(h)
    loader.close()


@pytest.mark.parametrize("ttype", TYPES)
def test_embedding_with_random_bytes_bit_exact(gpu, ttype):
    """token_embd as blocks of random bytes on the GPU; the oracle gets the same rows as F32 values from the NumPy decode
    (tests/q4_0_ref.py, pinned on the CPU): k_embed's decode must give the same bits"""
    hp = gpu.TINY()
    model = gpu.LlmModel(hp)
    hp = model.hparams
    orc = O.OracleLlm(oracle_cfg_from(hp, 8, 16), seed=4)
    install(model, orc, hp.n_layer)
    emb = random_blocks(ttype, np.random.default_rng(3), hp.vocab * hp.d_model // 32)
    model.set_tensor(-1, O.T_TOKEN_EMBD, ttype, emb.reshape(-1))
    orc.set_tensor(-1, O.T_TOKEN_EMBD, O.TYPE_F32, R.dequant(ttype, emb).reshape(-1))
    sess = gpu.LlmSession(model, 16, 8)
    seq = np.arange(16, dtype=np.int32)
    tok = np.random.default_rng(4).integers(3, hp.vocab, 16).astype(np.int32)
    want, wam = orc.forward(seq, np.zeros(16, np.int32), tok)
    got, gam = sess.forward(seq, np.zeros(16, np.int32), tok)
    assert np.isfinite(want).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.abs(got - want).max()
    assert np.array_equal(gam, wam)


@pytest.mark.parametrize("ttype", TYPES)
def test_gguf_logits_bit_exact_at_every_width(gpu, tmp_path, monkeypatch, ttype):
    """an all-Q4_0 / all-Q5_0 GGUF (twin-sparse, output Q6_K) loaded by tk_mi355x_llm_model_load_gguf: the logits are those of the oracle
    holding the same weights, at every width"""
    cfg = O.tiny_config()
    path = str(tmp_path / f"tiny_{NAME[ttype]}.gguf")
    src = TwinSparse(ttype, O.OracleLlm(cfg, seed=4), cfg)
    assert src.types(cfg.n_layer) == {ttype}
    gguf_util.write_llama_gguf(path, src, cfg)
    model = gpu.LlmModel(gguf=path)
    hp = model.hparams
    cfg2 = oracle_cfg_from(hp, 8, 256)  # the K-split plan the loader chose
    orc = O.OracleLlm(cfg2, seed=4)
    TwinSparse(ttype, orc, cfg2)        # the same seed and encoder: the oracle now holds the file's weights
    check_widths(gpu, model, hp, orc, monkeypatch, f"gguf {NAME[ttype]}")


@pytest.mark.parametrize("ttype", TYPES)
def test_gguf_end_to_end(gpu, tmp_path, ttype):
    """the same file through tk_model_loader + tk_llm_runner: the oracle's token ids"""
    cfg = O.tiny_config()
    path = str(tmp_path / f"tiny_{NAME[ttype]}.gguf")
    gguf_util.write_llama_gguf(path, TwinSparse(ttype, O.OracleLlm(cfg, seed=4), cfg), cfg)
    loader = gpu.ModelLoader()
    h = loader.load(path)
    hp = gpu.LlmHParams()
    gpu.lib().tk_mi355x_llm_model_get_hparams(h, C.byref(hp))
    cfg2 = oracle_cfg_from(hp, 64, 1)
    orc = O.OracleLlm(cfg2, seed=4)
    TwinSparse(ttype, orc, cfg2)
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


@pytest.mark.parametrize("ttype", TYPES)
def test_lora_into_such_a_matrix_fails_the_load(gpu, tmp_path, ttype):
    hp = gpu.TINY()
    rng = np.random.default_rng(1)
    D = hp.d_model
    kvd = hp.n_kv_head * hp.head_dim
    factors = {(0, 3): (rng.standard_normal((4, D)).astype(np.float32) * 0.01, rng.standard_normal((kvd, 4)).astype(np.float32) * 0.01)}
    ad = str(tmp_path / "v.gguf")
    gguf_util.write_lora_gguf(ad, 8.0, factors)
    model = gpu.LlmModel(hp)
    model.set_lora(ad)
    blocks = gpu.quantize_blocks(ttype, (rng.standard_normal((kvd, D)) * 0.02).astype(np.float32))
    with pytest.raises(gpu.TkError) as ei:
        model.set_tensor(0, 3, ttype, blocks.reshape(-1))
    assert "LoRA merge" in str(ei.value) and f"{NAME[ttype]} matrix is not built" in str(ei.value)
