"""GPU: Q4_1 and Q5_1 weights (GGML types 3 and 7) on the W4A8 kernels, bit for bit.  w = d q + m per block of 32, so each block adds to
Q8_0's product term a min term m_j d8 S_j on the block's activation sum.  The contract is restated in tests/q4_1_ref.py and held against
the oracle on the CPU by tests/test_q4_1_q5_1_cpu.py; here the kernels are held to it: general and edge-case blocks against the
restatement, twin-sparse runs (one live block, seven with d = m = +0) against the oracle running their Q4_K twins and against the probe's own
Q5_K output for their Q5_K twins, and blocks with m = 0 against the probe's own Q8_0 output for their Q8_0 twins."""
import ctypes as C
import struct

import numpy as np
import pytest

import gguf_util
import oracle_lib as O
import q4_0_ref as R40
import q4_1_ref as R
from kquant_gpu_util import check_widths, install, logits_in_passes, oracle_cfg_from, shapes

pytestmark = pytest.mark.gpu

TYPES = [R.Q4_1, R.Q5_1]
NAME = {R.Q4_1: "Q4_1", R.Q5_1: "Q5_1"}
INSTALLED_BYTES_PER_256 = {R.Q4_1: 160, R.Q5_1: 192, 14: 210}   # tiles of 16 rows x 256 k: eight 20- / 24-byte blocks per row and run


class TwinSparse:
    """Every layer matrix and token_embd of an oracle model as twin-sparse blocks made from the oracle's dequantised weights; output stays
    the oracle's Q6_K.  type_of(layer, which) names the type of each: Q4_1 / Q5_1 (live q <= 15, so the run has a Q4_K twin) or Q4_0
    (tests/q4_0_ref.py, Q6_K twins).  The ORACLE IS CHANGED to hold exactly the same weights: the twins (token_embd: the NumPy-decoded
    F32 rows).  Norms stay."""

    def __init__(self, type_of, orc, cfg):
        self.orc, self.t = orc, {}
        assert orc.get_tensor(-1, O.T_OUTPUT)[0] == O.TYPE_Q6_K
        todo = [(l, w, r, c) for l in range(cfg.n_layer) for w, (r, c) in shapes(cfg).items()]
        todo.append((-1, O.T_TOKEN_EMBD, cfg.vocab, cfg.d_model))
        for layer, which, rows, cols in todo:
            ttype = type_of(layer, which)
            w = orc.dequant(layer, which, rows, cols)
            seed = 1000 * (layer + 1) + which
            b = R40.quantize_twin_sparse(ttype, w, seed=seed) if ttype == R40.Q4_0 else R.quantize_twin_sparse(ttype, w, seed=seed, q4_only=True)
            self.t[(layer, which)] = (ttype, b.reshape(-1))
        for (layer, which), (ttype, b) in self.t.items():
            if layer < 0:
                orc.set_tensor(layer, which, O.TYPE_F32, (R40.dequant(ttype, b) if ttype == R40.Q4_0 else R.dequant(ttype, b)).reshape(-1))
            elif ttype == R40.Q4_0:
                orc.set_tensor(layer, which, O.TYPE_Q6_K, R40.to_q6k(ttype, b))
            else:
                orc.set_tensor(layer, which, O.TYPE_Q4_K, R.to_q4k(ttype, b))

    def get_tensor(self, layer, which):
        return self.t[(layer, which)] if (layer, which) in self.t else self.orc.get_tensor(layer, which)

    def types(self, n_layer):
        return {self.get_tensor(l, w)[0] for l in range(n_layer) for w in (1, 2, 3, 4, 6, 7, 8)} | {self.get_tensor(-1, 0)[0]}


def imatrix_mix(layer, which):
    """llama.cpp's quantiser with an importance matrix, as the issue recalls it: a Q4_0 file whose first layers' ffn_down are Q4_1"""
    return R.Q4_1 if (layer == 0 and which == 8) else R40.Q4_0


KINDS = {"Q4_1": lambda layer, which: R.Q4_1, "Q5_1": lambda layer, which: R.Q5_1, "Q4_0+Q4_1": imatrix_mix}
KIND_TYPES = {"Q4_1": {R.Q4_1}, "Q5_1": {R.Q5_1}, "Q4_0+Q4_1": {R40.Q4_0, R.Q4_1}}


@pytest.mark.parametrize("kind", list(KINDS))
def test_twin_sparse_model_bit_exact_at_every_width(gpu, monkeypatch, kind):
    """a whole tiny model with every layer matrix and token_embd twin-sparse in the type (or Q4_0 with a Q4_1 ffn_down, the
    importance-matrix mix) and output Q6_K, against the oracle holding the twins: every width of WIDTHS, both fuse settings"""
    hp = gpu.TINY()
    model = gpu.LlmModel(hp)
    hp = model.hparams
    cfg = oracle_cfg_from(hp, 8, 256)
    orc = O.OracleLlm(cfg, seed=4)
    src = TwinSparse(KINDS[kind], orc, cfg)
    assert src.types(hp.n_layer) == KIND_TYPES[kind] and src.get_tensor(-1, O.T_OUTPUT)[0] == 14
    if kind == "Q4_0+Q4_1":
        assert (src.get_tensor(0, 8)[0], src.get_tensor(1, 8)[0], src.get_tensor(0, 7)[0]) == (R.Q4_1, R40.Q4_0, R40.Q4_0)
    install(model, src, hp.n_layer)
    check_widths(gpu, model, hp, orc, monkeypatch, f"twin-sparse {kind}")


def random_blocks(ttype, rng, n):
    """n blocks with random quant bytes (every nibble, every qh bit) and d, m of both signs"""
    b = rng.integers(0, 256, (n, R.BYTES[ttype]), dtype=np.uint8)
    b[:, 0:2] = (rng.uniform(1e-3, 1e-2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float16).view(np.uint8).reshape(n, 2)
    b[:, 2:4] = (rng.uniform(1e-3, 1e-1, n) * rng.choice([-1.0, 1.0], n)).astype(np.float16).view(np.uint8).reshape(n, 2)
    return b


def edge_blocks(ttype, rng, rows, nb):
    """[rows][nb runs][8 blocks]: whole rows of edge cases, the rest random"""
    nbytes, qs = R.BYTES[ttype], R.QS_AT[ttype]
    b = random_blocks(ttype, rng, rows * nb * 8).reshape(rows, nb, 8, nbytes)
    f16 = lambda v: np.array(v, np.float16).view(np.uint8)
    u16 = lambda v: np.array([v], np.uint16).view(np.uint8)
    b[0, :, :, 4:] = 0                                                  # q = 0 everywhere: the min term alone
    b[1, :, :, 4:] = 0xFF                                               # q = 15 / 31 everywhere
    b[2, :, :, 2:4] = 0                                                 # m = +0: the product term alone
    b[3, :, :, 2:4] = u16(0x8000)                                       # m = -0
    b[4, :, :, 0:2] = 0                                                 # d = 0 with m != 0
    b[5, :, :, 0:2] = f16([-0.0078])                                    # negative d and m
    b[5, :, :, 2:4] = f16([-0.0421])
    b[6, :, :, 0:2] = u16(0x0001)                                       # subnormal d and m, of both signs
    b[6, :, 1::2, 0:2] = u16(0x83FF)
    b[6, :, :, 2:4] = u16(0x8003)
    b[6, :, 1::2, 2:4] = u16(0x03FF)
    # d alternating in sign and by 2^10 in magnitude between neighbouring 32-blocks (m constant): a scale taken 64 or 256 wide gives other bits
    b[7, :, 0::2, 0:2] = f16([2.0 ** -4])
    b[7, :, 1::2, 0:2] = f16([-(2.0 ** -14)])
    b[7, :, :, 2:4] = f16([0.0137])
    # ... and m likewise (d constant): an S_j paired with the wrong j, or an m taken 64 or 256 wide
    b[8, :, 0::2, 2:4] = f16([-(2.0 ** -3)])
    b[8, :, 1::2, 2:4] = f16([2.0 ** -13])
    b[8, :, :, 0:2] = f16([0.0059])
    # ... and both at once, the large d beside the small m
    b[9, :, 0::2, 0:2], b[9, :, 1::2, 0:2] = f16([2.0 ** -4]), f16([-(2.0 ** -14)])
    b[9, :, 0::2, 2:4], b[9, :, 1::2, 2:4] = f16([2.0 ** -13]), f16([-(2.0 ** -3)])
    b[10, :, :, 0:4] = 0                                                # one live block per run, at a position that walks with the run
    b[11, :, :, 0:4] = 0                                                # ... and another walk in the next row
    for r in range(nb):
        b[10, r, (3 * r + 1) % 8, 0:2], b[10, r, (3 * r + 1) % 8, 2:4] = f16([0.0061]), f16([-0.0205])
        b[11, r, (5 * r + 2) % 8, 0:2], b[11, r, (5 * r + 2) % 8, 2:4] = f16([-0.0047]), f16([0.0311])
    b[12, :, :, qs:] = 0xF0                                             # weights 0..15 = 0, weights 16..31 = 15: nibble order
    b[13, :, :, qs:] = 0x0F
    b[14, :, :, qs:qs + 8] = 0x21                                       # ... and the order inside each half
    b[14, :, :, qs + 8:] = 0x43
    if ttype == R.Q5_1:
        u32 = lambda v: np.array([v], "<u4").view(np.uint8)
        b[15, :, :, 4:8] = u32(0x0000FFFF)
        b[16, :, :, 4:8] = u32(0xFFFF0000)
        b[17, :, :, 4:8] = u32(0xAAAAAAAA)
        for r in range(nb):
            for j in range(8):
                b[18, r, j, 4:8] = u32(1 << ((8 * r + j) % 32))        # a single walking bit
        b[12, :, :, 4:8] = u32(0x0000FFFF)                              # rows 12, 13: the two halves differ in the high bit too
        b[13, :, :, 4:8] = u32(0xFFFF0000)
    return b


def edge_activations(rng, n, K):
    """[n][K]: whole rows of edge cases for the sums S_j, the rest random"""
    x = rng.standard_normal((n, K)).astype(np.float32)
    x[0] = 0.75                                                         # all equal: every a = +-127, |S| = 4064
    x[1] = -0.75
    x[2] = np.tile(np.array([0.5, -0.5], np.float32), K // 2)           # +-x alternating: S = 0 in every block, a != 0
    x[3] = x[2]
    for r in range(K // 256):                                           # ... but for one block of each run, at a position that walks
        j = (3 * r + 2) % 8
        x[3, 256 * r + 32 * j:256 * r + 32 * j + 32] = 0.5 * (1 if r % 2 else -1)
    x[4] = -np.abs(x[4]) - np.float32(0.01)                             # one sign: every sum far below zero, odd ones among them (the
    x[5] = np.abs(x[5]) + np.float32(0.01)                              # element of largest magnitude maps to -127, whatever its sign)
    x[5, ::256] = -5.0                                                  # ... and far above zero: the run's largest element has the other sign
    x[6, 512:768] = 0.0                                                 # one activation run all zero
    return x


def q8_rows(x):
    qs, ds, bs = zip(*[O.q8k_quantize(r) for r in x])
    return np.stack(qs), np.stack(ds).reshape(len(x), -1), np.stack(bs)


PROBE_NROWS = [1, 2, 16, 17, 32, 33, 192, 193, 256]
ROWS, K = 64, 7168          # the smallest K that splits 1, 4 and 7 ways into whole 256-k runs
Q4K_TWIN_ROWS = slice(0, 32)
_probe = {}


def probe_case(ttype):
    """the probe's three weight matrices (edge cases; twin-sparse; the edge cases with m = 0), the activations and the expected results,
    computed once per type"""
    if ttype not in _probe:
        rng = np.random.default_rng(40 + ttype)
        nb = K // 256
        edge = edge_blocks(ttype, rng, ROWS, nb).reshape(-1, R.BYTES[ttype])
        w = (rng.standard_normal((ROWS, K)) * 0.02 + rng.choice([-0.05, 0.0, 0.05], (ROWS, 1))).astype(np.float32)
        twin = R.quantize_twin_sparse(ttype, w, seed=9, q4_only=True)
        if ttype == R.Q5_1:                                             # rows 32..63: live blocks over Q5_1's whole range, high bits set
            twin = twin.reshape(ROWS, -1)
            twin[32:] = R.quantize_twin_sparse(ttype, w[32:], seed=10).reshape(32, -1)
            first = twin[:32].reshape(-1, R.BYTES[ttype])
            on = (R.d_bits(ttype, first) != 0) | (R.m_bits(ttype, first) != 0)
            assert R.quants(ttype, twin[32:]).max() == 31 and R.quants(ttype, first)[on].max() == 15 and not first[on][:, 4:8].any()
            twin = twin.reshape(-1, R.BYTES[ttype])
        live = R.live_of(ttype, twin).reshape(ROWS, nb)
        assert all(len(set(live[r].tolist())) == 8 for r in range(ROWS)) and (live[0] != live[1]).any()   # every j, another walk per row
        m0 = edge.copy()
        m0[:, 2:4] = 0
        m0[1::2, 3] = 0x80                                              # m = -0 in every other block
        x = edge_activations(rng, 256, K)
        q8, d8, bs = q8_rows(x)
        assert (np.abs(bs[0]) == 4064).all() and (np.abs(bs[1]) == 4064).all() and d8[0, 0] * d8[1, 0] < 0   # the element of largest magnitude maps to -127: the sign is d8's
        assert not bs[2].any() and (q8[2] != 0).all()
        assert ((bs[3].reshape(-1, 8) != 0).sum(axis=1) == 1).all() and len(set((bs[3].reshape(-1, 8) != 0).argmax(axis=1).tolist())) == 8
        lo, hi = bs[4], bs[5].reshape(-1, 8)[:, 1:]
        assert lo.max() < -64 and (lo % 2 == 1).any() and (lo % 64 != 0).any() and hi.min() > 64      # the l / h split below zero
        assert not q8[6, 512:768].any() and d8[6, 2] == 0
        assert (d8 < 0).any() and (d8 > 0).any()
        want = {name: {ks: R.gemv(ttype, blk, ROWS, K, ks, q8, d8, bs) for ks in (1, 4, 7)} for name, blk in (("edge", edge), ("twin", twin), ("m0", m0))}
        _probe[ttype] = ({"edge": edge, "twin": twin, "m0": m0}, x, want)
    return _probe[ttype]


@pytest.mark.parametrize("ks", [1, 4, 7])
@pytest.mark.parametrize("ttype", TYPES)
def test_gemv_probe_equals_the_restated_contract_the_oracle_and_the_twins(gpu, ttype, ks):
    """edge-case, random and twin-sparse blocks through every W4A8 family and its edges (1..32 rows: mat-vec with one and two M-tiles —
    K-split 1 has 28 runs per range and takes the K-streamed kernel —, 33..192: GEMM, 193..256: 32x32x32 GEMM) and K-split 1 / 4 / 7:
    bit for bit the restatement; on the twin-sparse rows with q <= 15 bit for bit oracle_lib.gemv_q8 on the Q4_K twins; on all twin-sparse
    rows bit for bit the probe's own output for the Q5_K twins (type 13); with m = 0 bit for bit the probe's own output for the Q8_0 twins
    (type 8)"""
    blocks, x, want = probe_case(ttype)
    for name in want:
        assert np.isfinite(want[name][ks]).all() and want[name][ks].any()
    rows4 = ROWS if ttype == R.Q4_1 else 32
    twin4 = R.to_q4k(ttype, blocks["twin"].reshape(ROWS, -1)[:rows4].reshape(-1, R.BYTES[ttype]))
    orc = np.stack([O.gemv_q8(O.TYPE_Q4_K, twin4, rows4, K, ks, r) for r in x])
    assert np.array_equal(orc.view(np.uint32), want["twin"][ks][:, :rows4].view(np.uint32)), ks
    twin5 = R.to_q5k(ttype, blocks["twin"])
    twin8 = R.to_q8_0(ttype, blocks["m0"])
    for n in PROBE_NROWS:
        for name in ("edge", "twin", "m0"):
            got = gpu.gemv_probe(ttype, blocks[name].reshape(-1), ROWS, K, ks, x[:n])
            w = want[name][ks][:n]
            bad = np.argwhere(got.view(np.uint32) != w.view(np.uint32))
            assert bad.size == 0, (name, ks, n, len(bad), bad[:8].tolist(), np.abs(got - w).max())
            if name == "twin":
                got5 = gpu.gemv_probe(13, twin5, ROWS, K, ks, x[:n])
                assert np.array_equal(got.view(np.uint32), got5.view(np.uint32)), (ks, n)
            if name == "m0":
                got8 = gpu.gemv_probe(8, twin8.reshape(-1), ROWS, K, ks, x[:n])
                assert np.array_equal(got.view(np.uint32), got8.view(np.uint32)), (ks, n)


def recipe_bytes(hp, cfg, ttype):
    return (hp.vocab * hp.d_model // 256 * INSTALLED_BYTES_PER_256[14] +
            sum(r * c for r, c in shapes(cfg).values()) * hp.n_layer // 256 * INSTALLED_BYTES_PER_256[ttype])


@pytest.mark.parametrize("ttype", TYPES)
def test_synthetic_width_invariance_and_recipe(gpu, ttype):
    """fill_synthetic_type(3 | 7) on the tiny geometry — general blocks from the host quantiser's device twin in every layer matrix and
    token_embd, output Q6_K: the same logits bits as 1 x 256, 2 x 128, 8 x 32, 16 x 16 and 256 x 1 passes (every kernel family, fused
    producers at one row), two positions through the KV cache; two fills with one seed are identical; the logits are not the Q4_K_M
    model's nor the other type's; weight_bytes is the sum the recipe implies; synthetic://tiny-q41 / -q51 is the loader's name for it;
    file types 3 and 9 stay refused by fill_synthetic, and fill_synthetic_type takes nothing but the two"""
    assert (gpu.FTYPE_Q4_1, gpu.TYPE_Q4_1, gpu.FTYPE_Q5_1, gpu.TYPE_Q5_1) == (3, 3, 9, 7)
    hp = gpu.TINY()
    model = gpu.LlmModel(hp).fill_synthetic_type(4, ttype)
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
    again = gpu.LlmModel(hp).fill_synthetic_type(4, ttype)
    got = logits_in_passes(gpu, again, hp, 256, toks)
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32))
    q4km = logits_in_passes(gpu, gpu.LlmModel(hp).fill_synthetic(4, ftype=gpu.FTYPE_Q4_K_M), hp, 256, toks)[0]
    assert not np.array_equal(q4km, ref[0])
    other = R.Q5_1 if ttype == R.Q4_1 else R.Q4_1
    om = gpu.LlmModel(hp).fill_synthetic_type(4, other)
    assert om.weight_bytes == recipe_bytes(hp, cfg, other) != want_bytes
    assert not np.array_equal(logits_in_passes(gpu, om, hp, 256, toks)[0], ref[0])
    for bad in (gpu.FTYPE_Q4_1, gpu.FTYPE_Q5_1):
        with pytest.raises(gpu.TkError):
            gpu.LlmModel(hp).fill_synthetic(9, ftype=bad)
    for bad in (-3, 0, 1, 2, 6, 8, 9, 12, 14, 20, 23):
        with pytest.raises(gpu.TkError):
            gpu.LlmModel(hp).fill_synthetic_type(9, bad)
    loader = gpu.ModelLoader()
    h = loader.load("synthetic://tiny-q41?seed=4" if ttype == R.Q4_1 else "synthetic://tiny-q51?seed=4")
    wb = gpu.lib().tk_mi355x_llm_model_weight_bytes
    wb.restype = C.c_uint64
    assert wb(h) == want_bytes
    loader.unload(h)
    loader.close()


@pytest.mark.parametrize("ttype", TYPES)
def test_embedding_with_random_bytes_bit_exact(gpu, ttype):
    """token_embd as blocks of random bytes on the GPU; the oracle gets the same rows as F32 values from the NumPy decode
    (tests/q4_1_ref.py, pinned on the CPU): k_embed's decode, fmaf(d, q, m), must give the same bits"""
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


@pytest.mark.parametrize("kind", list(KINDS))
def test_gguf_logits_bit_exact_at_every_width(gpu, tmp_path, monkeypatch, kind):
    """an all-Q4_1 / all-Q5_1 GGUF and a Q4_0 one with a Q4_1 ffn_down (twin-sparse, output Q6_K) loaded by
    tk_mi355x_llm_model_load_gguf: the logits are those of the oracle holding the same weights, at every width"""
    cfg = O.tiny_config()
    path = str(tmp_path / "tiny.gguf")
    src = TwinSparse(KINDS[kind], O.OracleLlm(cfg, seed=4), cfg)
    assert src.types(cfg.n_layer) == KIND_TYPES[kind]
    gguf_util.write_llama_gguf(path, src, cfg)
    model = gpu.LlmModel(gguf=path)
    hp = model.hparams
    cfg2 = oracle_cfg_from(hp, 8, 256)  # the K-split plan the loader chose
    orc = O.OracleLlm(cfg2, seed=4)
    TwinSparse(KINDS[kind], orc, cfg2)  # the same seed and encoder: the oracle now holds the file's weights
    check_widths(gpu, model, hp, orc, monkeypatch, f"gguf {kind}")


@pytest.mark.parametrize("kind", list(KINDS))
def test_gguf_end_to_end(gpu, tmp_path, kind):
    """the same files through tk_model_loader + tk_llm_runner: the oracle's token ids"""
    cfg = O.tiny_config()
    path = str(tmp_path / "tiny.gguf")
    gguf_util.write_llama_gguf(path, TwinSparse(KINDS[kind], O.OracleLlm(cfg, seed=4), cfg), cfg)
    loader = gpu.ModelLoader()
    h = loader.load(path)
    hp = gpu.LlmHParams()
    gpu.lib().tk_mi355x_llm_model_get_hparams(h, C.byref(hp))
    cfg2 = oracle_cfg_from(hp, 64, 1)
    orc = O.OracleLlm(cfg2, seed=4)
    TwinSparse(KINDS[kind], orc, cfg2)
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


def test_gguf_whose_k_is_no_multiple_of_256_fails_the_load(gpu, tmp_path):
    """a Q4_1 file that claims d_ff = 480 (whole 32-blocks, not whole 256-k runs): the reader's size checks pass, the load is refused"""
    cfg = O.tiny_config()
    path = str(tmp_path / "tiny.gguf")
    gguf_util.write_llama_gguf(path, TwinSparse(KINDS["Q4_1"], O.OracleLlm(cfg, seed=4), cfg), cfg)
    raw = bytearray(open(path, "rb").read())
    key = gguf_util._s("llama.feed_forward_length")
    at = raw.index(key) + len(key) + 4
    assert struct.unpack_from("<I", raw, at)[0] == cfg.d_ff
    struct.pack_into("<I", raw, at, cfg.d_ff - 32)
    for w in ("ffn_gate", "ffn_up", "ffn_down"):
        for l in range(cfg.n_layer):
            name = gguf_util._s(f"blk.{l}.{w}.weight")
            dims_at = raw.index(name) + len(name) + 4
            dims = list(struct.unpack_from("<QQ", raw, dims_at))
            dims[dims.index(cfg.d_ff)] = cfg.d_ff - 32
            struct.pack_into("<QQ", raw, dims_at, *dims)
    bad = str(tmp_path / "k480.gguf")
    open(bad, "wb").write(bytes(raw))
    hp = gpu.LlmHParams()
    assert gpu.lib().tk_mi355x_gguf_probe(bad.encode(), C.byref(hp), None) == 0 and hp.d_ff == cfg.d_ff - 32
    with pytest.raises(gpu.TkError) as ei:
        gpu.LlmModel(gguf=bad)
    assert "256" in str(ei.value)


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
