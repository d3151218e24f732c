"""GPU: IQ4_NL and IQ4_XS weights (GGML types 20 and 23) on the W4A8 kernels, bit for bit.  A 32-weight sub-block of either type IS the
Q8_0 block with scale D = d (IQ4_NL) or d (float)s_j (IQ4_XS) and q8 = kv[q], so both are pinned to what the project already trusts
(tests/iq4_ref.py, held against the oracle on the CPU by tests/test_iq4_cpu.py): general blocks against the restated contract,
twin-sparse runs (one live sub-block, seven dead) against the oracle running their Q6_K twins, and the sub-blocks whose D is an f16
against the probe's own output for their Q8_0 twins."""
import ctypes as C

import numpy as np
import pytest

import gguf_util
import iq4_ref as R
import oracle_lib as O
from kquant_gpu_util import check_widths, install, logits_in_passes, oracle_cfg_from, shapes

pytestmark = pytest.mark.gpu

TYPES = [R.IQ4_NL, R.IQ4_XS]
NAME = {R.IQ4_NL: "IQ4_NL", R.IQ4_XS: "IQ4_XS"}
FTYPE = {R.IQ4_NL: 25, R.IQ4_XS: 30}
LOADER = {R.IQ4_NL: "synthetic://tiny-iq4nl?seed=4", R.IQ4_XS: "synthetic://tiny-iq4xs?seed=4"}
INSTALLED_BYTES_PER_256 = {R.IQ4_NL: 144, R.IQ4_XS: 144, 14: 210}   # tiles of 16 rows x 256 k: both IQ4 tiles are 2304 B


class TwinSparse:
    """Every layer matrix and token_embd of an oracle model as twin-sparse blocks of `ttype` made from the oracle's dequantised weights;
    output stays the oracle's Q6_K, and with v_q6k attn_v becomes a general Q6_K tensor (the mixed q | k | v launch of real IQ4_XS
    files).  The ORACLE IS CHANGED to hold exactly the same weights: the Q6_K twins (token_embd: the NumPy-decoded F32 rows)."""

    def __init__(self, ttype, orc, cfg, v_q6k=False):
        self.orc, self.t = orc, {}
        assert orc.get_tensor(-1, O.T_OUTPUT)[0] == O.TYPE_Q6_K
        todo = [(l, w, r, c) for l in range(cfg.n_layer) for w, (r, c) in shapes(cfg).items()]
        todo.append((-1, O.T_TOKEN_EMBD, cfg.vocab, cfg.d_model))
        for layer, which, rows, cols in todo:
            w = orc.dequant(layer, which, rows, cols)
            if v_q6k and layer >= 0 and which == 3:
                self.t[(layer, which)] = (O.TYPE_Q6_K, O.quantize_rows(O.TYPE_Q6_K, w))
            else:
                self.t[(layer, which)] = (ttype, R.quantize_twin_sparse(ttype, w, seed=1000 * (layer + 1) + which).reshape(-1))
        for (layer, which), (t, b) in self.t.items():
            if t == O.TYPE_Q6_K:
                orc.set_tensor(layer, which, O.TYPE_Q6_K, b)
            elif layer < 0:
                orc.set_tensor(layer, which, O.TYPE_F32, R.dequant(ttype, b).reshape(-1))
            else:
                orc.set_tensor(layer, which, O.TYPE_Q6_K, R.to_q6k(ttype, b))

    def get_tensor(self, layer, which):
        return self.t[(layer, which)] if (layer, which) in self.t else self.orc.get_tensor(layer, which)

    def types(self, n_layer):
        return {self.get_tensor(l, w)[0] for l in range(n_layer) for w in (1, 2, 3, 4, 6, 7, 8)} | {self.get_tensor(-1, 0)[0]}


@pytest.mark.parametrize("v_q6k", [False, True])
@pytest.mark.parametrize("ttype", TYPES)
def test_twin_sparse_model_bit_exact_at_every_width(gpu, monkeypatch, ttype, v_q6k):
    """a whole tiny model with every layer matrix and token_embd twin-sparse in the type and output Q6_K, against the oracle holding the
    twins: every width of WIDTHS, both fuse settings; and the same with attn_v Q6_K, so that q | k | v is a mixed-type launch"""
    hp = gpu.TINY()
    model = gpu.LlmModel(hp)
    hp = model.hparams
    cfg = oracle_cfg_from(hp, 8, 256)
    orc = O.OracleLlm(cfg, seed=4)
    src = TwinSparse(ttype, orc, cfg, v_q6k)
    assert src.types(hp.n_layer) == ({ttype, 14} if v_q6k else {ttype}) and src.get_tensor(-1, O.T_OUTPUT)[0] == 14
    install(model, src, hp.n_layer)
    check_widths(gpu, model, hp, orc, monkeypatch, f"twin-sparse {NAME[ttype]} v_q6k={v_q6k}")


def rand_d(rng, n, five):
    """f16 d of both signs in 0.004 .. 0.01, as bits; five: at most five significant bits, so that d s_j is an f16 for every s_j"""
    sign = rng.choice([-1.0, 1.0], n)
    mag = rng.integers(16, 32, n) * 2.0 ** -12 if five else rng.uniform(1e-3, 1e-2, n)
    return (mag * sign).astype(np.float16).view(np.uint16)


def random_blocks(ttype, rng, n):
    """n blocks of random bytes (every nibble, every scale bit) with d of both signs"""
    b = rng.integers(0, 256, (n, R.BYTES[ttype]), dtype=np.uint8)
    b[:, 0:2] = rand_d(rng, n, False).view(np.uint8).reshape(n, 2)
    return b


HALF = 64                    # edge_rows makes 64 weight rows
TWIN_ROWS = slice(32, 64)    # its twin-sparse rows


def edge_rows(ttype, rng, nb, five):
    """64 weight rows x nb runs: whole rows of edge cases (0..17), random rows, and 32 twin-sparse rows.  five: every d has at most five
    significant bits (IQ4_XS rows that are Q8_0 blocks)"""
    xs = ttype == R.IQ4_XS
    idx = rng.integers(0, 16, (HALF, nb, 8, 32))
    d = rand_d(rng, HALF * nb * (1 if xs else 8), five).reshape((HALF, nb) if xs else (HALF, nb, 8))
    ls = rng.integers(0, 64, (HALF, nb, 8))
    f16 = lambda v: np.array([v], np.float16).view(np.uint16)[0]
    idx[0], idx[1], idx[2] = 0, 15, 8                                    # kv = -127, 113, 1 everywhere
    d[3] = 0                                                             # d = 0
    d[4] = f16(-(2.0 ** -7) if five else -0.0078)                        # negative d
    d[5] = 0x0001                                                        # subnormal d
    d[5, 1::2] = 0x8003 if five else 0x83FF                              # ... and a negative one, in every other run
    # one live sub-block per run, at a position that walks with the run
    walk = (3 * np.arange(nb) + 1) % 8
    if xs:
        d[7] = f16(25 * 2.0 ** -12 if five else 0.0061)
        ls[7] = 32
        ls[7, np.arange(nb), walk] = rng.integers(0, 64, nb)
    else:
        d[7] = 0
        d[7, np.arange(nb), walk] = f16(0.0061)
    idx[8, :, :, :16], idx[8, :, :, 16:] = 0, 15                         # nibble bytes 0xF0: weights 0..15 / 16..31
    idx[9, :, :, :16], idx[9, :, :, 16:] = 15, 0                         # 0x0F
    idx[10, :, :, 0:8], idx[10, :, :, 16:24] = 1, 2                      # bytes 0..7 = 0x21, bytes 8..15 = 0x43: the order inside each half
    idx[10, :, :, 8:16], idx[10, :, :, 24:32] = 3, 4
    if xs:
        ls[11, :, 0::2], ls[11, :, 1::2] = 63, 0                         # s alternating +31 / -32 between neighbouring sub-blocks
        ls[12], ls[13], ls[14] = 0, 63, 32
        ls[15] = 32                                                      # scales_l = 0, scales_h = 0xAAAA
        ls[16] = 0                                                       # scales_h alone: a walking pair of set bits
        ls[16, np.arange(nb), (5 * np.arange(nb) + 2) % 8] = 48
        ls[17] = rng.integers(0, 16, (nb, 8))                            # scales_l alone: scales_h = 0
    else:
        # d alternating in sign and by 2^10 in magnitude between neighbouring blocks: a scale taken 64 or 256 wide gives other bits
        d[6, :, 0::2], d[6, :, 1::2] = f16(2.0 ** -4), f16(-(2.0 ** -14))
    b = R.make_blocks(ttype, idx.reshape(-1, 32), d.reshape(-1), ls.reshape(-1, 8) if xs else None).reshape(HALF, nb, -1)
    if xs:
        raw = b.reshape(HALF, nb, R.BYTES[ttype])
        assert (raw[15, :, 4:8] == 0).all() and (raw[15, :, 2:4] == 0xAA).all() and (raw[16, :, 4:8] == 0).all() and (raw[17, :, 2:4] == 0).all()
    assert (b.reshape(HALF, -1, R.BYTES[ttype])[8, :, R.QS_AT[ttype]:] == 0xF0).all()
    assert (b.reshape(HALF, -1, R.BYTES[ttype])[10, :, R.QS_AT[ttype]:].reshape(-1, 16) == [0x21] * 8 + [0x43] * 8).all()
    w = (rng.standard_normal((32, nb * 256)) * 0.02).astype(np.float32)
    b[TWIN_ROWS] = R.quantize_twin_sparse(ttype, w, seed=9).reshape(32, nb, -1)
    return b


def q8_rows(x):
    qs, ds, _ = zip(*[O.q8k_quantize(r) for r in x])
    return np.stack(qs), np.stack(ds).reshape(len(x), -1)


PROBE_NROWS = [1, 2, 16, 17, 32, 33, 192, 193, 256]
_probe = {}


def probe_case(ttype):
    """the probe's blocks, activations and expected results, computed once per type: K = 7168, 128 weight rows (the first 64 general, the
    last 64 the same cases with five-bit d: Q8_0 blocks for IQ4_XS too), 256 activation rows"""
    if ttype not in _probe:
        rng = np.random.default_rng(40 + ttype)
        rows, K = 2 * HALF, 7168
        b = np.concatenate([edge_rows(ttype, rng, K // 256, False), edge_rows(ttype, rng, K // 256, True)])
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
    restatement, on the twin-sparse rows bit for bit oracle_lib.gemv_q8 on the Q6_K twins, and on the Q8_0-twin-able rows (all of IQ4_NL;
    the 64 five-bit-d rows of IQ4_XS) bit for bit the probe's own output for the Q8_0 twin blocks (type 8) at the same shapes"""
    rows, K, b, x, want = probe_case(ttype)
    want = want[ks]
    assert np.isfinite(want).all()
    twin6 = R.to_q6k(ttype, b[TWIN_ROWS].reshape(-1))
    orc = np.stack([O.gemv_q8(O.TYPE_Q6_K, twin6, 32, K, ks, r) for r in x])
    assert np.array_equal(orc.view(np.uint32), want[:, TWIN_ROWS].view(np.uint32)), ks
    r8 = slice(0, rows) if ttype == R.IQ4_NL else slice(HALF, rows)
    assert not R.q8_0_twinable(ttype, b[:HALF].reshape(-1)).all() or ttype == R.IQ4_NL
    twin8 = R.to_q8_0(ttype, b[r8].reshape(-1))
    for n in PROBE_NROWS:
        got = gpu.gemv_probe(ttype, b.reshape(-1), rows, K, ks, x[:n])
        bad = np.argwhere(got.view(np.uint32) != want[:n].view(np.uint32))
        assert bad.size == 0, (ks, n, len(bad), bad[:8].tolist(), np.abs(got - want[:n]).max())
        got8 = gpu.gemv_probe(8, twin8.reshape(-1), r8.stop - r8.start, K, ks, x[:n])
        assert np.array_equal(got[:, r8].view(np.uint32), got8.view(np.uint32)), (ks, n)


def recipe_bytes(hp, cfg, ttype):
    return (hp.vocab * hp.d_model // 256 * INSTALLED_BYTES_PER_256[14] +
            sum(r * c for r, c in shapes(cfg).values()) * hp.n_layer // 256 * INSTALLED_BYTES_PER_256[ttype])


@pytest.mark.parametrize("ttype", TYPES)
def test_synthetic_width_invariance_and_recipe(gpu, ttype):
    """synthetic ftype 25 / 30 on the tiny geometry — general blocks from the host quantiser's device twin in every layer matrix and
    token_embd, output Q6_K: the same logits bits as 1 x 256, 2 x 128, 8 x 32, 16 x 16 and 256 x 1 passes (every kernel family, fused
    producers at one row), two positions through the KV cache; two fills with one seed are identical; the logits are not the Q4_K_M
    model's nor the other type's; weight_bytes is the sum the recipe implies; synthetic://tiny-iq4nl / -iq4xs is the loader's name for
    it; the other ftypes stay refused"""
    assert (gpu.FTYPE_IQ4_NL, gpu.TYPE_IQ4_NL, gpu.FTYPE_IQ4_XS, gpu.TYPE_IQ4_XS) == (25, 20, 30, 23)
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
    other = R.IQ4_XS if ttype == R.IQ4_NL else R.IQ4_NL
    om = gpu.LlmModel(hp).fill_synthetic(4, ftype=FTYPE[other])
    assert om.weight_bytes == recipe_bytes(hp, cfg, other)
    assert not np.array_equal(logits_in_passes(gpu, om, hp, 256, toks)[0], ref[0])
    for bad in (0, 3, 9, 13, 18, 20, 22, 23, 24, 26, 29, 31):
        with pytest.raises(gpu.TkError):
            gpu.LlmModel(hp).fill_synthetic(9, ftype=bad)
    loader = gpu.ModelLoader()
    h = loader.load(LOADER[ttype])
    wb = gpu.lib().tk_mi355x_llm_model_weight_bytes
    wb.restype = C.c_uint64
    assert wb(h) == want_bytes
    loader.unload(h)
    loader.close()


@pytest.mark.parametrize("ttype", TYPES)
def test_embedding_with_random_bytes_bit_exact(gpu, ttype):
    """token_embd as blocks of random bytes on the GPU; the oracle gets the same rows as F32 values from the NumPy decode
    (tests/iq4_ref.py, pinned on the CPU): k_embed's decode must give the same bits"""
    hp = gpu.TINY()
    model = gpu.LlmModel(hp)
    hp = model.hparams
    orc = O.OracleLlm(oracle_cfg_from(hp, 8, 16), seed=4)
    install(model, orc, hp.n_layer)
    emb = random_blocks(ttype, np.random.default_rng(3), hp.vocab * hp.d_model // R.ELEMS[ttype])
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
    """an all-IQ4_NL / all-IQ4_XS GGUF (twin-sparse, output Q6_K) loaded by tk_mi355x_llm_model_load_gguf: the logits are those of the
    oracle holding the same weights, at every width"""
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
