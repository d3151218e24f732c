"""GPU: TQ1_0 and TQ2_0 weights (GGML types 34 and 35, the ternary types) on the W4A8 kernels, bit for bit.  EVERY block of either type is
the Q6_K block with the same d, all sixteen scales 1 and q6 = 32 + (code - 1), so the unchanged oracle pins every bit of the new path
(tests/tq_ref.py, held against the oracle on the CPU by tests/test_tq_cpu.py): general blocks against the restated contract AND against
the oracle running their Q6_K twins, on all rows.  A TQ1_0 matrix is installed as the TQ2_0 tile: its results are also held against the
probe's own output for the TQ2_0 blocks with the same weights."""
import ctypes as C
import struct

import numpy as np
import pytest

import gguf_util
import oracle_lib as O
import tq_ref as R
from kquant_gpu_util import check_widths, install, logits_in_passes, oracle_cfg_from, shapes

pytestmark = pytest.mark.gpu

TQ1, TQ2 = R.TQ1_0, R.TQ2_0
TYPES = [TQ1, TQ2]
NAME = {TQ1: "TQ1_0", TQ2: "TQ2_0"}
FTYPE = {TQ1: 36, TQ2: 37}
LOADER = {TQ1: "synthetic://tiny-tq10?seed=4", TQ2: "synthetic://tiny-tq20?seed=4"}
# bytes per 256 weights as a decode step streams them: the W4A8 tiles of 16 rows x 256 k over 16 (TK_TQ2_0_TILE_BYTES = 1056 for BOTH
# types: a TQ1_0 matrix is installed as the TQ2_0 tile; TK_Q6K_TILE_BYTES = 3360)
TILE_BYTES_PER_256 = {TQ1: 1056 // 16, TQ2: 1056 // 16, 14: 3360 // 16}


class Twins:
    """Every layer matrix of an oracle model in `ttype` — ggml's reference quantiser (tests/tq_ref.py) on the oracle's dequantised weights —
    with token_embd (Q4_K) and output (Q6_K) as the oracle has them: llama.cpp's recipe for the two file types.  v_q6k: attn_v becomes a
    general Q6_K tensor (the mixed q | k | v launch); embd: token_embd in the type too.  The ORACLE IS CHANGED to hold exactly the same
    weights: the Q6_K twins (token_embd: the NumPy-decoded F32 rows)."""

    def __init__(self, ttype, orc, cfg, v_q6k=False, embd=False, encode=None):
        self.orc, self.t = orc, {}
        encode = encode or (lambda w: R.quantize(ttype, w))
        assert orc.get_tensor(-1, O.T_OUTPUT)[0] == O.TYPE_Q6_K and orc.get_tensor(-1, O.T_TOKEN_EMBD)[0] == O.TYPE_Q4_K
        todo = [(l, w, r, c) for l in range(cfg.n_layer) for w, (r, c) in shapes(cfg).items()]
        if embd:
            todo.append((-1, O.T_TOKEN_EMBD, cfg.vocab, cfg.d_model))
        for layer, which, rows, cols in todo:
            w = orc.dequant(layer, which, rows, cols)
            if v_q6k and layer >= 0 and which == 3:
                self.t[(layer, which)] = (O.TYPE_Q6_K, O.quantize_rows(O.TYPE_Q6_K, w))
            else:
                self.t[(layer, which)] = (ttype, encode(w).reshape(-1))
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
        return {self.get_tensor(l, w)[0] for l in range(n_layer) for w in (1, 2, 3, 4, 6, 7, 8)}


@pytest.mark.parametrize("variant", ["recipe", "v_q6k", "embd"])
@pytest.mark.parametrize("ttype", TYPES)
def test_whole_model_bit_exact_at_every_width(gpu, monkeypatch, ttype, variant):
    """a whole tiny model with every layer matrix in the type, token_embd Q4_K and output Q6_K, against the oracle holding the Q6_K twins:
    every width of WIDTHS, both fuse settings; the same with attn_v Q6_K, so that q | k | v is a mixed-type launch; and with token_embd
    in the type itself (k_embed's decode; the oracle is given the decoded F32 rows)"""
    hp = gpu.TINY()
    model = gpu.LlmModel(hp)
    hp = model.hparams
    cfg = oracle_cfg_from(hp, 8, 256)
    orc = O.OracleLlm(cfg, seed=4)
    src = Twins(ttype, orc, cfg, v_q6k=variant == "v_q6k", embd=variant == "embd")
    assert src.types(hp.n_layer) == ({ttype, 14} if variant == "v_q6k" else {ttype})
    assert src.get_tensor(-1, O.T_OUTPUT)[0] == 14 and src.get_tensor(-1, O.T_TOKEN_EMBD)[0] == (ttype if variant == "embd" else 12)
    install(model, src, hp.n_layer)
    check_widths(gpu, model, hp, orc, monkeypatch, f"{NAME[ttype]} {variant}")


ROWS, K = 128, 7168
NB = K // 256
WALK = [(41 * r + 3) % 256 for r in range(NB)]   # the live weight of run r in the one-live-weight row


def f16_bits(v):
    return np.array([v], np.float16).view(np.uint16)[0]


def rand_d(rng, shape):
    """f16 d of both signs in 0.001 .. 0.01, as bits"""
    return (rng.uniform(1e-3, 1e-2, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float16).view(np.uint16)


def probe_rows(ttype, rng):
    """128 weight rows x 28 runs as raw blocks: random bytes (rows 16..63: TQ2_0 all four codes, TQ1_0 all 256 byte values, the
    non-canonical ones and arbitrary fifth trits in qh among them), whole rows of edge cases (0..12), rows quantised from normal data
    (64..127)"""
    nbytes, d_at = R.BYTES[ttype], R.D_AT[ttype]
    b = rng.integers(0, 256, (ROWS, NB, nbytes), dtype=np.uint8)
    d = rand_d(rng, (ROWS, NB))
    ones = np.ones((NB, 256), np.int64)

    def put(row, codes):
        b[row] = R.make_blocks(ttype, codes, np.zeros(NB, np.uint16))

    put(0, 0 * ones)                                                     # all code 0: every weight -d
    put(1, 2 * ones)                                                     # all code 2: +d
    put(2, ones)                                                         # all code 1: zero weights
    if ttype == TQ2:
        put(3, 3 * ones)                                                 # all code 3: +2 d
    d[4] = 0                                                             # d = 0
    d[5] = f16_bits(-0.0078)                                             # negative d
    d[6] = 0x0001                                                        # subnormal d
    d[6, 1::2] = 0x83FF                                                  # ... and the largest negative one, in every other run
    d[7, 0::2], d[7, 1::2] = f16_bits(2.0 ** -4), f16_bits(-(2.0 ** -14))   # alternating in sign and by 2^10 between neighbouring runs
    live = ones.copy()                                                   # one live weight per run, at a walking position
    live[np.arange(NB), WALK] = np.where(np.arange(NB) % 3 == 0, 0, 2)
    put(8, live)
    if ttype == TQ2:
        b[9, :, 0:64:2], b[9, :, 1:64:2] = 0x1B, 0xE4                    # codes 3, 2, 1, 0 / 0, 1, 2, 3 over l, alternating over m
        b[10, :, 0:32], b[10, :, 32:64] = 0x00, 0xAA                     # h: the first 128 weights -d, the last 128 +d
        b[11, :, 0:64] = np.arange(64) * 4 + 3                           # every byte another value: m and h from the byte index
    else:
        b[9, :, 0:52:2], b[9, :, 1:52:2] = 187, 81                       # trits (2, 0, 1, 2, 0) / (0, 2, 2, 1, 1), alternating over m
        b[10, :, 0:32], b[10, :, 32:48], b[10, :, 48:52] = 0, 255, 128   # the three segments: -d, +d (a non-canonical byte), zero
        b[11, :, 0:52] = np.arange(52) * 4 + 48                          # every byte another value, the non-canonical 244, 248, 252 among them
        b[12, :, 0:52] = rng.integers(243, 256, (NB, 52))                # non-canonical bytes alone
    w = (rng.standard_normal((64, K)) * 0.02).astype(np.float32)
    b[64:128] = R.quantize(ttype, w).reshape(64, NB, nbytes)
    keep = np.ones(ROWS, bool)
    keep[64:128] = False                                                 # the quantised rows keep their own d (amax of the data)
    b[keep, :, d_at:d_at + 2] = d[keep].reshape(-1, NB, 1).view(np.uint8)
    return b


def q8_rows(x):
    qs, ds, _ = zip(*[O.q8k_quantize(r) for r in x])
    return np.stack(qs), np.stack(ds).reshape(len(x), -1)


PROBE_NROWS = [1, 2, 16, 17, 32, 33, 192, 193, 256]
_probe = {}


def probe_case(ttype):
    """the probe's blocks, activations and expected results, computed once per type and left unchanged"""
    if ttype not in _probe:
        rng = np.random.default_rng(40 + ttype)
        b = probe_rows(ttype, rng)
        x = rng.standard_normal((256, K)).astype(np.float32)
        x[3, 512:768] = 0.0                                             # one activation run all zero
        q8, d8 = q8_rows(x)
        want = {ks: R.gemv(ttype, b.reshape(-1), ROWS, K, ks, q8, d8) for ks in (1, 4, 7)}
        _probe[ttype] = (b, x, want, R.to_q6k(ttype, b.reshape(-1)))
    return _probe[ttype]


@pytest.mark.parametrize("ttype", TYPES)
def test_probe_rows_are_what_they_are_meant_to_be(gpu, ttype):
    b, _, _, _ = probe_case(ttype)
    c = R.codes(ttype, b.reshape(-1)).reshape(ROWS, NB, 256)
    assert (c[0] == 0).all() and (c[1] == 2).all() and (c[2] == 1).all()
    assert set(WALK) == set(np.nonzero((c[8] != 1).any(axis=0))[0].tolist()) and ((c[8] != 1).sum(axis=1) == 1).all()
    assert {(p % 128) // 32 for p in WALK} == {0, 1, 2, 3} and {p // 128 for p in WALK} == {0, 1}        # all four TQ2_0 shifts, both halves
    assert any(p < 160 for p in WALK) and any(160 <= p < 240 for p in WALK) and any(p >= 240 for p in WALK)   # all three TQ1_0 segments
    raw = b[16:64, :, :R.D_AT[ttype]]
    if ttype == TQ2:
        assert (c[3] == 3).all() and set(np.unique(c[16:64]).tolist()) == {0, 1, 2, 3}
        assert (c[9, :, 0::2][:, :16] == 3).all() and (c[9, :, 1::2][:, :16] == 0).all() and (c[10, :, :128] == 0).all() and (c[10, :, 128:] == 2).all()
    else:
        assert len(np.unique(raw[:, :, :48])) == 256 and len(np.unique(raw[:, :, 48:52])) == 256
        assert (b[12, :, :52] >= 243).all() and c.max() == 2
        assert (c[10, :, :160] == 0).all() and (c[10, :, 160:240] == 2).all() and (c[10, :, 240:] == 1).all()
    db = R.d_bits(ttype, b.reshape(-1)).reshape(ROWS, NB)
    assert (db[4] == 0).all() and (db[5] & 0x8000).all() and set(db[6].tolist()) == {0x0001, 0x83FF}
    assert (R.codes(ttype, b[64:128].reshape(-1)) <= 2).all()


@pytest.mark.parametrize("ks", [1, 4, 7])
@pytest.mark.parametrize("ttype", TYPES)
def test_gemv_probe_equals_the_restated_contract_the_oracle_and_the_tq2_0_image(gpu, ttype, ks):
    """random and edge-case blocks through every W4A8 family and its edges (1..32 rows: mat-vec with one and two M-tiles — K-split 1 has
    28 runs per range and takes the K-streamed kernel —, 33..192: GEMM, 193..256: 32x32x32 GEMM) and K-split 1 / 4 / 7: bit for bit the
    restatement, which is bit for bit oracle_lib.gemv_q8 on the Q6_K twins of ALL rows; for TQ1_0 also bit for bit the probe's own output
    for the TQ2_0 blocks with the same weights (the tile it is installed as)"""
    b, x, want, twin6 = probe_case(ttype)
    want = want[ks]
    assert np.isfinite(want).all()
    orc = np.stack([O.gemv_q8(O.TYPE_Q6_K, twin6, ROWS, K, ks, r) for r in x])
    assert np.array_equal(orc.view(np.uint32), want.view(np.uint32)), ks
    as_tq2 = R.tq1_to_tq2(b.reshape(-1)) if ttype == TQ1 else None
    for n in PROBE_NROWS:
        got = gpu.gemv_probe(ttype, b.reshape(-1), ROWS, K, ks, x[:n])
        bad = np.argwhere(got.view(np.uint32) != want[:n].view(np.uint32))
        assert bad.size == 0, (ks, n, len(bad), bad[:8].tolist(), np.abs(got - want[:n]).max())
        if ttype == TQ1:
            got2 = gpu.gemv_probe(TQ2, as_tq2.reshape(-1), ROWS, K, ks, x[:n])
            assert np.array_equal(got.view(np.uint32), got2.view(np.uint32)), (ks, n)


def recipe_bytes(hp, cfg, ttype):
    """output (Q6_K tiles) + the layer matrices (the type's tiles); token_embd is not a matrix a decode step streams"""
    return (hp.vocab * hp.d_model // 256 * TILE_BYTES_PER_256[14] +
            sum(r * c for r, c in shapes(cfg).values()) * hp.n_layer // 256 * TILE_BYTES_PER_256[ttype])


class Loaded:
    """a handle from tk_model_loader_load_model where the helpers want an LlmModel"""

    def __init__(self, gpu, h):
        self.h = h
        self.hparams = gpu.LlmHParams()
        gpu.lib().tk_mi355x_llm_model_get_hparams(h, C.byref(self.hparams))


def synth_toks(hp):
    rng = np.random.default_rng(7)
    return [rng.integers(3, hp.vocab, 256).astype(np.int32) for _ in range(2)]


@pytest.mark.parametrize("ttype", TYPES)
def test_synthetic_width_invariance_and_recipe_bytes(gpu, ttype):
    """synthetic ftype 36 / 37 on the tiny geometry: the same logits bits in passes of 256, 64 and 16 rows (every kernel family), two
    positions through the KV cache; two fills with one seed are identical; the logits are not the Q4_K_M model's; weight_bytes is the sum
    the recipe implies — output in Q6_K tiles, the layer matrices in the type's — with TQ1_0 counting TQ2_0's tile; the loader's
    synthetic://tiny-tq10 / -tq20 has the same bytes and the same logits"""
    assert (gpu.FTYPE_TQ1_0, gpu.TYPE_TQ1_0, gpu.FTYPE_TQ2_0, gpu.TYPE_TQ2_0) == (36, 34, 37, 35)
    hp = gpu.TINY()
    model = gpu.LlmModel(hp).fill_synthetic(4, ftype=FTYPE[ttype])
    hp = model.hparams
    cfg = oracle_cfg_from(hp, 4, 1)
    want_bytes = recipe_bytes(hp, cfg, ttype)
    assert TILE_BYTES_PER_256[TQ1] == TILE_BYTES_PER_256[TQ2] == 66 and want_bytes == recipe_bytes(hp, cfg, TQ2)
    assert model.weight_bytes == want_bytes
    toks = synth_toks(hp)
    ref = logits_in_passes(gpu, model, hp, 256, toks)
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()
    for width in (64, 16):
        got = logits_in_passes(gpu, model, hp, width, toks)
        for p in range(2):
            assert np.array_equal(got[p].view(np.uint32), ref[p].view(np.uint32)), (width, p)
    again = gpu.LlmModel(hp).fill_synthetic(4, ftype=FTYPE[ttype])
    got = logits_in_passes(gpu, again, hp, 256, toks)
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32))
    q4km = logits_in_passes(gpu, gpu.LlmModel(hp).fill_synthetic(4, ftype=gpu.FTYPE_Q4_K_M), hp, 256, toks)[0]
    assert not np.array_equal(q4km, ref[0])
    loader = gpu.ModelLoader()
    h = loader.load(LOADER[ttype])
    wb = gpu.lib().tk_mi355x_llm_model_weight_bytes
    wb.restype = C.c_uint64
    assert wb(h) == want_bytes
    got = logits_in_passes(gpu, Loaded(gpu, h), hp, 256, toks)
    for p in range(2):
        assert np.array_equal(got[p].view(np.uint32), ref[p].view(np.uint32)), p
    loader.unload(h)
    loader.close()


def test_synthetic_recipe_tensor_types(gpu):
    """the tensor types of ftypes 36 / 37, seen from outside.  token_embd is Q4_K and output Q6_K: both are the seeded blocks the oracle
    holds for seed 4 (the Q4_K_M recipe's, same stream and type), so putting the oracle's blocks in their place changes no logits bit,
    while token_embd in the type itself — what the 32-block recipes do — gives other logits at the same weight_bytes.  The layer matrices
    are ternary in both (weight_bytes: 66 bytes per 256 weights), and the two recipes hold the SAME weights: ggml's two quantisers make
    the same trits of the same stream and a TQ1_0 matrix is installed as the TQ2_0 tile, so ftype 36 equals ftype 37 bit for bit — which
    holds the device TQ1_0 quantiser and the base-3 repack to the TQ2_0 path on synthetic data"""
    hp = gpu.TINY()
    m36 = gpu.LlmModel(hp).fill_synthetic(4, ftype=36)
    hp = m36.hparams
    toks = synth_toks(hp)
    ref = logits_in_passes(gpu, m36, hp, 256, toks)
    m37 = gpu.LlmModel(hp).fill_synthetic(4, ftype=37)
    got = logits_in_passes(gpu, m37, hp, 256, toks)
    for p in range(2):
        assert np.array_equal(got[p].view(np.uint32), ref[p].view(np.uint32)), p
    orc = O.OracleLlm(oracle_cfg_from(hp, 4, 1), seed=4)
    emb_t, emb = orc.get_tensor(-1, O.T_TOKEN_EMBD)
    out_t, out = orc.get_tensor(-1, O.T_OUTPUT)
    assert (emb_t, out_t) == (O.TYPE_Q4_K, O.TYPE_Q6_K)
    for ttype in TYPES:
        model = gpu.LlmModel(hp).fill_synthetic(4, ftype=FTYPE[ttype])
        model.set_tensor(-1, O.T_TOKEN_EMBD, O.TYPE_Q4_K, emb)
        got = logits_in_passes(gpu, model, hp, 256, toks)
        assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32))
        model.set_tensor(-1, O.T_OUTPUT, O.TYPE_Q6_K, out)
        got = logits_in_passes(gpu, model, hp, 256, toks)
        assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32))
        before = model.weight_bytes
        own = gpu.quantize_blocks(ttype, orc.dequant(-1, O.T_TOKEN_EMBD, hp.vocab, hp.d_model))
        model.set_tensor(-1, O.T_TOKEN_EMBD, ttype, own.reshape(-1))
        got = logits_in_passes(gpu, model, hp, 256, toks)
        assert model.weight_bytes == before and np.isfinite(got[0]).all() and not np.array_equal(got[0], ref[0])


def test_refused_file_types_and_probe_arguments(gpu):
    """file types other than 36 / 37 are taken or refused as before (34 and 35, the tensor types' own numbers, are no file types); the
    probe takes both types and refuses a K that is no multiple of 256 ks.  (Columns that are no multiple of 256 cannot reach set_tensor:
    the model geometry is held to multiples of 256 when the handle is made.  The next test refuses them on the GGUF path.)"""
    hp = gpu.TINY()
    for bad in (0, 3, 9, 13, 18, 20, 22, 23, 24, 26, 29, 31, 34, 35, 38, 39):
        with pytest.raises(gpu.TkError):
            gpu.LlmModel(hp).fill_synthetic(9, ftype=bad)
    for ok in (36, 37, 25, 10):
        gpu.LlmModel(hp).fill_synthetic(9, ftype=ok).close()
    x = np.zeros((1, 512), np.float32)
    for ttype in TYPES:
        blocks = np.zeros(64 * 2 * R.BYTES[ttype], np.uint8)
        assert np.isfinite(gpu.gemv_probe(ttype, blocks, 64, 512, 1, x)).all()
        with pytest.raises(gpu.TkError):
            gpu.gemv_probe(ttype, blocks, 64, 512, 4, x)               # K % (256 ks) != 0


@pytest.mark.parametrize("ttype", TYPES)
def test_gguf_whose_k_is_no_multiple_of_256_fails_the_load(gpu, tmp_path, ttype):
    """a file that claims d_ff = 384 for its TQ ffn tensors (whole bytes of the data section, not whole 256-k runs): the load is refused"""
    cfg = O.tiny_config()
    path = str(tmp_path / "tiny.gguf")
    gguf_util.write_llama_gguf(path, Twins(ttype, O.OracleLlm(cfg, seed=4), cfg), cfg)
    raw = bytearray(open(path, "rb").read())
    key = gguf_util._s("llama.feed_forward_length")
    at = raw.index(key) + len(key) + 4
    assert struct.unpack_from("<I", raw, at)[0] == cfg.d_ff
    struct.pack_into("<I", raw, at, cfg.d_ff - 128)
    for w in ("ffn_gate", "ffn_up", "ffn_down"):
        for l in range(cfg.n_layer):
            name = gguf_util._s(f"blk.{l}.{w}.weight")
            dims_at = raw.index(name) + len(name) + 4
            dims = list(struct.unpack_from("<QQ", raw, dims_at))
            dims[dims.index(cfg.d_ff)] = cfg.d_ff - 128
            struct.pack_into("<QQ", raw, dims_at, *dims)
    bad = str(tmp_path / "k384.gguf")
    open(bad, "wb").write(bytes(raw))
    with pytest.raises(gpu.TkError) as ei:
        gpu.LlmModel(gguf=bad)
    assert "256" in str(ei.value)


@pytest.mark.parametrize("ttype", TYPES)
def test_embedding_with_random_bytes_bit_exact(gpu, ttype):
    """token_embd as blocks of random bytes on the GPU (TQ1_0: every byte value, decoded per weight by k_embed; TQ2_0: code 3 among them);
    the oracle gets the same rows as F32 values from the NumPy decode (tests/tq_ref.py, pinned on the CPU): the same bits"""
    hp = gpu.TINY()
    model = gpu.LlmModel(hp)
    hp = model.hparams
    orc = O.OracleLlm(oracle_cfg_from(hp, 8, 16), seed=4)
    install(model, orc, hp.n_layer)
    rng = np.random.default_rng(3)
    n = hp.vocab * hp.d_model // 256
    emb = rng.integers(0, 256, (n, R.BYTES[ttype]), dtype=np.uint8)
    emb[:, R.D_AT[ttype]:] = rand_d(rng, n).view(np.uint8).reshape(n, 2)
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
    """a GGUF in the 36 / 37 recipe (every layer matrix in the type, token_embd Q4_K, output Q6_K) loaded by
    tk_mi355x_llm_model_load_gguf: the logits are those of the oracle holding the same weights, at every width"""
    cfg = O.tiny_config()
    path = str(tmp_path / f"tiny_{NAME[ttype]}.gguf")
    src = Twins(ttype, O.OracleLlm(cfg, seed=4), cfg)
    assert src.types(cfg.n_layer) == {ttype}
    gguf_util.write_llama_gguf(path, src, cfg)
    model = gpu.LlmModel(gguf=path)
    hp = model.hparams
    cfg2 = oracle_cfg_from(hp, 8, 256)  # the K-split plan the loader chose
    orc = O.OracleLlm(cfg2, seed=4)
    Twins(ttype, orc, cfg2)             # the same seed and encoder: the oracle now holds the file's weights
    assert model.weight_bytes == recipe_bytes(hp, cfg2, ttype)
    check_widths(gpu, model, hp, orc, monkeypatch, f"gguf {NAME[ttype]}")


@pytest.mark.parametrize("ttype", TYPES)
def test_gguf_end_to_end(gpu, tmp_path, ttype):
    """the same file through tk_model_loader + tk_llm_runner: prompt and greedy ids are the oracle's"""
    cfg = O.tiny_config()
    path = str(tmp_path / f"tiny_{NAME[ttype]}.gguf")
    gguf_util.write_llama_gguf(path, Twins(ttype, O.OracleLlm(cfg, seed=4), cfg), cfg)
    ids = np.zeros(16, np.int32)
    n_ids = gpu.lib().tk_mi355x_gguf_tokenize(path.encode(), b"hello world", 1, ids.ctypes.data_as(C.c_void_p), 16)
    assert ids[:n_ids].tolist() == [1, 263, 273]
    loader = gpu.ModelLoader()
    h = loader.load(path)
    hp = gpu.LlmHParams()
    gpu.lib().tk_mi355x_llm_model_get_hparams(h, C.byref(hp))
    cfg2 = oracle_cfg_from(hp, 64, 1)
    orc = O.OracleLlm(cfg2, seed=4)
    Twins(ttype, orc, cfg2)
    runner = gpu.LlmRunner(h, context_size=64)
    runner.prepare("hello world")
    _, am = orc.forward([0, 0, 0], [0, 1, 2], ids[:3], want_logits=False)
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
    assert "LoRA merge needs a Q4_K, Q6_K, F16, BF16 or F32 matrix" in str(ei.value) and f"{NAME[ttype]} matrix is not built" in str(ei.value)


_layer = {}


def mistral_layer(gpu, ttype, cfg):
    """the seven matrices of one Mistral-7B-shaped layer, encoded once per type for both widths by the host quantiser (byte for byte
    tests/tq_ref.py's, tests/test_tq_cpu.py), with their Q6_K twins"""
    if ttype not in _layer:
        orc = O.OracleLlm(cfg, seed=4)
        t = {}
        for which, (rows, cols) in shapes(cfg).items():
            b = gpu.quantize_blocks(ttype, orc.dequant(0, which, rows, cols)).reshape(-1)
            t[which] = (b, R.to_q6k(ttype, b))
        orc.close()
        _layer.clear()      # one type's 218 M weights at a time
        _layer[ttype] = t
    return _layer[ttype]


@pytest.mark.parametrize("nrows", [16, 256])
@pytest.mark.parametrize("ttype", TYPES)
def test_mistral_shape_layer_bit_exact(gpu, ttype, nrows):
    """one Mistral-7B-shaped layer (4096 / 1024 / 14336 dims, the production K-split plan 4 / 4 / 1 / 7, a small vocabulary) with all seven
    matrices in the type, against the oracle holding their Q6_K twins (256 rows: the 32x32x32 kernel with the fused SwiGLU epilogue)"""
    hp = gpu.MISTRAL_7B()
    hp.n_layer = 1
    hp.vocab = 512
    model = gpu.LlmModel(hp)
    hp = model.hparams
    assert (hp.ks_qkv, hp.ks_o, hp.ks_gateup, hp.ks_down) == (4, 4, 1, 7)
    cfg = oracle_cfg_from(hp, 4, nrows)
    layer = mistral_layer(gpu, ttype, cfg)
    orc = O.OracleLlm(cfg, seed=4)
    install(model, orc, 1)
    for which, (b, twin) in layer.items():
        model.set_tensor(0, which, ttype, b)
        orc.set_tensor(0, which, O.TYPE_Q6_K, twin)
    assert model.weight_bytes == recipe_bytes(hp, cfg, ttype)
    sess = gpu.LlmSession(model, nrows, 4)
    seq = np.arange(nrows, dtype=np.int32)
    tok = np.random.default_rng(2).integers(3, hp.vocab, nrows).astype(np.int32)
    want, wam = orc.forward(seq, np.zeros(nrows, np.int32), tok)
    got, gam = sess.forward(seq, np.zeros(nrows, np.int32), tok)
    assert np.isfinite(want).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.abs(got - want).max()
    assert np.array_equal(gam, wam)
