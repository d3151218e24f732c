"""CPU: TQ1_0 and TQ2_0 (GGML types 34 and 35, the ternary types) — the constants, the NumPy codecs against hand-written blocks and literal
expected arrays, every TQ1_0 byte value in both positions, the host quantiser entries against the NumPy quantisers byte for byte, the round
trip, the Q6_K twins against the oracle (dequantised bits and the dot contract), the refused arguments, and the GGUF reader and tokenizer
entries on a file with TQ tensors.  (The refusals that need a model handle — columns that are no multiple of 256, the file types
fill_synthetic_ftype does not take — are in tests/test_tq_gpu.py: a handle needs a device.)"""
import ctypes as C
import struct

import numpy as np
import pytest

import gguf_util as G
import oracle_lib as O
import tq_ref as R

TQ1, TQ2 = R.TQ1_0, R.TQ2_0
TYPES = [TQ1, TQ2]
ENTRY = {TQ1: "tk_mi355x_quantize_blocks_tq1_0", TQ2: "tk_mi355x_quantize_blocks_tq2_0"}


@pytest.fixture(autouse=True)
def restated_types_are_the_librarys():
    """every test of this file restates types the library has to know: the restatement's type ids and block sizes are the library's"""
    import trackiellm_amd as tk
    assert {tk.TYPE_TQ1_0: tk.llm.BLOCK_BYTES[tk.TYPE_TQ1_0], tk.TYPE_TQ2_0: tk.llm.BLOCK_BYTES[tk.TYPE_TQ2_0]} == R.BYTES


def probe(path):
    import trackiellm_amd as tk
    hp = tk.LlmHParams()
    nv = C.c_int32(0)
    return tk.lib().tk_mi355x_gguf_probe(path.encode(), C.byref(hp), C.byref(nv))


def f16_bytes(v):
    return list(np.array([v], np.float16).view(np.uint8))


def test_constants_and_struct_sizes():
    import trackiellm_amd as tk
    assert (tk.TYPE_TQ1_0, tk.TYPE_TQ2_0, tk.FTYPE_TQ1_0, tk.FTYPE_TQ2_0) == (34, 35, 36, 37)
    assert (tk.llm.BLOCK_BYTES[34], tk.llm.BLOCK_BYTES[35]) == (54, 66)
    # the entries write exactly 54 / 66 bytes per block: the bytes after the last block stay as they were
    for t in TYPES:
        nb = R.BYTES[t]
        x = np.ones((3, 256), np.float32)
        fn = getattr(tk.lib(), ENTRY[t])
        fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        out = np.full(3 * nb + 8, 0xA5, np.uint8)
        assert fn(x.ctypes.data_as(C.c_void_p), 3, out.ctypes.data_as(C.c_void_p)) == 0
        assert (out[3 * nb:] == 0xA5).all() and not (out[:3 * nb] == 0xA5).all()


def test_tq2_0_hand_written_block_decodes_to_the_literal_array():
    """byte 0 = 0xE4 (codes 0, 1, 2, 3 at l = 0..3), byte 1 = 0x1B (3, 2, 1, 0), byte 33 = 0x02 (h = 1, m = 1, l = 0: code 2), every other
    byte 0x55 (code 1: zero); d = 0.5 LAST"""
    raw = np.full(66, 0x55, np.uint8)
    raw[0], raw[1], raw[33] = 0xE4, 0x1B, 0x02
    raw[64:66] = f16_bytes(0.5)
    want = np.zeros(256, np.float32)
    want[[0, 32, 64, 96]] = [-0.5, 0.0, 0.5, 1.0]          # m = 0: weights 32 l
    want[[1, 33, 65, 97]] = [1.0, 0.5, 0.0, -0.5]          # m = 1
    want[[129, 161, 193, 225]] = [0.5, -0.5, -0.5, -0.5]   # h = 1, m = 1: 128 + 32 l + 1; 0x02 has code 0 at l = 1..3
    got = R.dequant(TQ2, raw)[0]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert R.codes(TQ2, raw)[0, [0, 32, 64, 96]].tolist() == [0, 1, 2, 3]


def test_tq1_0_hand_written_block_decodes_to_the_literal_array():
    """canonical bytes by hand: trits (t0 .. t4) -> q = ((((t0 3 + t1) 3 + t2) 3 + t3) 3 + t4), byte = ceil(256 q / 243).
    qs[0] = (2, 0, 1, 2, 0) -> q = 177 -> 187; qs[32] = (0, 2, 2, 1, 1) -> q = 76 -> 81; qh[3] = (2, 1, 0, 2, pad 0) -> q = 195 -> 206; every
    other byte (1, 1, 1, 1, 1) -> q = 121 -> 128 (all zero weights); d = -2 LAST"""
    assert (177 * 256 + 242) // 243 == 187 and (76 * 256 + 242) // 243 == 81 and (195 * 256 + 242) // 243 == 206 and (121 * 256 + 242) // 243 == 128
    raw = np.full(54, 128, np.uint8)
    raw[0], raw[32], raw[51] = 187, 81, 206
    raw[52:54] = f16_bytes(-2.0)
    want = np.zeros(256, np.float32)
    want[[0, 32, 64, 96, 128]] = [-2.0, 2.0, -0.0, -2.0, 2.0]                  # (t - 1) * -2 for t = 2, 0, 1, 2, 0
    want[[160, 176, 192, 208, 224]] = [2.0, -2.0, -2.0, -0.0, -0.0]            # qs[32]: 160 + 16 n
    want[[243, 247, 251, 255]] = [-2.0, -0.0, 2.0, -2.0]                       # qh[3]: 240 + 4 n + 3
    want[want == 0] = -0.0                                                     # (float)0 * -2 = -0
    got = R.dequant(TQ1, raw)[0]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("ttype", TYPES)
def test_walking_single_live_weight_names_each_of_the_256_positions_once(ttype):
    """256 blocks, block i with weight i alone at code 2 (+d) and every other weight at code 1 (zero), written byte by byte from the format
    description: the decode is the identity matrix times d"""
    raw = np.zeros((256, R.BYTES[ttype]), np.uint8)
    for i in range(256):
        if ttype == TQ2:
            raw[i, 0:64] = 0x55
            h, l, m = i // 128, (i % 128) // 32, i % 32
            raw[i, 32 * h + m] = (0x55 & ~(3 << (2 * l))) | (2 << (2 * l))
        else:
            raw[i, 0:48] = 128                                                   # (1, 1, 1, 1, 1): q = 121
            raw[i, 48:52] = 127                                                  # (1, 1, 1, 1) and the pad digit 0: q = 120
            if i < 160:
                at, n = i % 32, i // 32
            elif i < 240:
                at, n = 32 + (i - 160) % 16, (i - 160) // 16
            else:
                at, n = 48 + (i - 240) % 4, (i - 240) // 4
            q = (121 if at < 48 else 120) + 3 ** (4 - n)                         # trit n goes from 1 to 2
            raw[i, at] = (q * 256 + 242) // 243
        raw[i, R.D_AT[ttype]:] = f16_bytes(0.25)
    got = R.dequant(ttype, raw)
    assert np.array_equal(got, np.eye(256, dtype=np.float32) * np.float32(0.25))
    assert np.array_equal(R.make_blocks(ttype, np.eye(256, dtype=np.int64) + 1, np.full(256, 0.25)), raw)


def test_every_tq1_0_byte_value_in_the_qs_and_the_qh_position():
    """all 256 byte values decode to trits in {0, 1, 2}, the 13 non-canonical ones 243..255 included; in a qs byte the five trits are five
    weights, in a qh byte the first four are and the fifth is not read"""
    by_hand = [[(((b * p) & 0xFF) * 3) >> 8 for p in (1, 3, 9, 27, 81)] for b in range(256)]
    assert by_hand[255] == [2, 2, 2, 2, 2] and by_hand[243] == [2, 2, 1, 1, 2]
    assert all(0 <= t <= 2 for row in by_hand for t in row)
    assert R.trits(np.arange(256)).tolist() == by_hand
    # the 243 canonical bytes are the 243 five-trit strings, in order
    canon = [(q * 256 + 242) // 243 for q in range(243)]
    assert [by_hand[c] for c in canon] == [[q // 81 % 3, q // 27 % 3, q // 9 % 3, q // 3 % 3, q % 3] for q in range(243)]
    raw = np.full((256, 54), 128, np.uint8)
    raw[:, 5] = np.arange(256)
    raw[:, 38] = np.arange(256)
    raw[:, 50] = np.arange(256)
    raw[:, 52:54] = f16_bytes(1.0)
    c = R.codes(TQ1, raw)
    t = np.array(by_hand)
    assert np.array_equal(c[:, [5, 37, 69, 101, 133]], t)                       # qs[5]: 32 n + 5
    assert np.array_equal(c[:, [166, 182, 198, 214, 230]], t)                   # qs[38]: 160 + 16 n + 6
    assert np.array_equal(c[:, [242, 246, 250, 254]], t[:, :4])                 # qh[2]: 240 + 4 n + 2
    rest = np.ones(256, bool)
    rest[[5, 37, 69, 101, 133, 166, 182, 198, 214, 230, 242, 246, 250, 254]] = False
    assert (c[:, rest] == 1).all()
    # the fifth trit of a qh byte is unused: bytes that differ in it alone decode alike
    a, b = raw[0].copy(), raw[0].copy()
    a[49], b[49] = (120 * 256 + 242) // 243, (122 * 256 + 242) // 243          # (1, 1, 1, 1, 0) and (1, 1, 1, 1, 2)
    assert a[49] != b[49] and np.array_equal(R.codes(TQ1, a), R.codes(TQ1, b))
    assert np.array_equal(R.dequant(TQ1, raw), (c - 1).astype(np.float32))


def special_rows(rng):
    x = (rng.standard_normal((8, 256)) * 0.02).astype(np.float32)
    x[0] = 0.0                                                                  # all zero: d = 0, id = 0, every trit 1
    x[1, 17] = -3.0                                                             # the extreme is negative
    x[2] = rng.choice(np.array([0.125, -0.125, 0.25, -0.25, 0.0], np.float32), 256)   # values exactly on +-amax / 2: lroundf's tie
    x[2, 0] = 0.25
    x[3] = np.clip(rng.standard_normal(256) * 1e6, -2e6, 2e6).astype(np.float32)   # amax above the f16 range: d = inf, id from the f32 amax
    x[3, 9] = 2e6
    x[4] = -0.0
    x[5, :] = np.float32(0.3)                                                   # constant
    x[6] = np.where(np.arange(256) % 2 == 0, np.float32(1.0), np.float32(-1.0)) * np.float32(0.7)
    x[7] = 0.0                                                                  # amax below 2^-128: id = inf, x id = +-inf or NaN (0 inf);
    x[7, 0::3], x[7, 1::3] = np.float32(1e-40), np.float32(-5e-41)              # defined here as +-1 and -1; d = +0
    return x


@pytest.mark.parametrize("ttype", TYPES)
def test_host_quantiser_equals_the_numpy_quantiser_byte_for_byte(ttype):
    import trackiellm_amd as tk
    rng = np.random.default_rng(50 + ttype)
    x = np.concatenate([(rng.standard_normal((512, 256)) * 0.02).astype(np.float32), rng.standard_normal((64, 256)).astype(np.float32) * 40,
                        special_rows(rng)])
    want = R.quantize(ttype, x)
    got = tk.quantize_blocks(ttype, x)
    assert got.shape == want.shape == (x.shape[0], R.BYTES[ttype])
    bad = np.argwhere((got != want).any(axis=1))
    assert bad.size == 0, bad[:8].tolist()
    sp = want[-8:]
    c = R.codes(ttype, sp)
    assert (c[0] == 1).all() and R.d_bits(ttype, sp)[0] == 0
    assert c[1, 17] == 0 and R.d_of(ttype, sp)[1] == 3.0
    tie = x[-6]
    assert np.array_equal(c[2], np.where(tie > 0, 2, np.where(tie < 0, 0, 1)))   # +-0.5 rounds away from zero
    assert R.d_bits(ttype, sp)[3] == 0x7C00 and set(c[3].tolist()) == {0, 1, 2} and c[3, 9] == 2
    assert (c[4] == 1).all() and (c[5] == 2).all() and set(c[6].tolist()) == {0, 2}
    assert R.d_bits(ttype, sp)[7] == 0 and np.array_equal(c[7], np.where(np.arange(256) % 3 == 0, 2, 0))
    assert c.max() <= 2                                                          # the quantiser never writes code 3


@pytest.mark.parametrize("ttype", TYPES)
def test_decode_of_quantise_is_the_identity_on_canonical_blocks(ttype):
    """a block of trits and an f16 d, decoded and quantised again, is the same bytes: the extreme is exactly d (some weight is +-d), every
    other weight 0 or +-d; all 243 + 81 byte round trips of TQ1_0 are in the sample"""
    import trackiellm_amd as tk
    rng = np.random.default_rng(3)
    q = rng.integers(0, 3, (400, 256))
    n = np.arange(243)
    five = np.stack([n // 81 % 3, n // 27 % 3, n // 9 % 3, n // 3 % 3, n % 3], axis=1)      # every five-trit string, in the first qs byte
    q[:243, [0, 32, 64, 96, 128]] = five
    q[:81, [240, 244, 248, 252]] = five[::3, :4]                                            # every four-trit string, in qh[0]
    q[:, 7] = 2                                                                              # a live weight: amax = |d|
    d = np.abs(rng.standard_normal(400)).astype(np.float16) + np.float16(0.01)
    b = R.make_blocks(ttype, q, d.astype(np.float32))
    assert np.array_equal(R.codes(ttype, b), q)
    w = R.dequant(ttype, b)
    assert np.array_equal(tk.quantize_blocks(ttype, w), b)
    assert np.array_equal(R.quantize(ttype, w), b)


@pytest.mark.parametrize("ttype", TYPES)
def test_tq1_to_tq2_and_the_q6k_twin_hold_the_same_weights(ttype):
    """random bytes (TQ2_0: code 3 among them; TQ1_0: the non-canonical bytes among them): the Q6_K twin dequantises through the oracle to
    tq_ref.dequant's bits, and a TQ1_0 block's TQ2_0 image decodes to the same bits"""
    rng = np.random.default_rng(8 + ttype)
    rows, K = 32, 1024
    b = rng.integers(0, 256, (rows * K // 256, R.BYTES[ttype]), dtype=np.uint8)
    b[:, R.D_AT[ttype]:] = (rng.uniform(1e-3, 1e-2, b.shape[0]) * rng.choice([-1.0, 1.0], b.shape[0])).astype(np.float16).view(np.uint8).reshape(-1, 2)
    c = R.codes(ttype, b)
    assert c.max() == (3 if ttype == TQ2 else 2) and c.min() == 0
    if ttype == TQ1:
        assert (b[:, :52] >= 243).any()
        assert np.array_equal(R.dequant(TQ2, R.tq1_to_tq2(b)).view(np.uint32), R.dequant(TQ1, b).view(np.uint32))
    w6 = O.dequant_rows(O.TYPE_Q6_K, R.to_q6k(ttype, b), rows, K).reshape(-1, 256)
    mine = R.dequant(ttype, b)
    assert np.array_equal(w6.view(np.uint32), mine.view(np.uint32))


def q8_rows(x):
    qs, ds, _ = zip(*[O.q8k_quantize(r) for r in x])
    return np.stack(qs), np.stack(ds).reshape(len(x), -1)


_case = {}


def contract_case(ttype):
    if ttype not in _case:
        rng = np.random.default_rng(70 + ttype)
        rows, K = 64, 1792
        b = rng.integers(0, 256, (rows * K // 256, R.BYTES[ttype]), dtype=np.uint8)
        d = (rng.uniform(1e-3, 1e-2, b.shape[0]) * rng.choice([-1.0, 1.0], b.shape[0])).astype(np.float16)
        d[5], d[6], d[7] = 0.0, np.float16(6e-8), -np.float16(6e-5)                         # zero and subnormal d
        b[:, R.D_AT[ttype]:] = d.view(np.uint8).reshape(-1, 2)
        b[32:64] = R.quantize(ttype, (rng.standard_normal((32, 256)) * 0.02).astype(np.float32))
        x = rng.standard_normal((6, K)).astype(np.float32)
        x[0, 256:512] = 0.0
        x[1, 0], x[2, 0] = -7.0, 7.0
        _case[ttype] = (rows, K, b, x, q8_rows(x))
    return _case[ttype]


@pytest.mark.parametrize("ks", [1, 4, 7])
@pytest.mark.parametrize("ttype", TYPES)
def test_restated_contract_equals_the_oracle_on_the_q6k_twins(ttype, ks):
    """tq_ref.gemv on ANY blocks is oracle_lib.gemv_q8 on their Q6_K twins, bit for bit: K-split 1 / 4 / 7"""
    rows, K, b, x, (q8, d8) = contract_case(ttype)
    K = K if ks != 4 else 1024
    nb = K // 256
    bb = b.reshape(rows, -1, R.BYTES[ttype])[:, :nb].reshape(-1, R.BYTES[ttype])
    xs = x[:, :K]
    if ks == 4:
        q8, d8 = q8_rows(xs)
    assert (d8 < 0).any() and (d8 > 0).any() and (d8 == 0).any()
    want = np.stack([O.gemv_q8(O.TYPE_Q6_K, R.to_q6k(ttype, bb), rows, K, ks, r) for r in xs])
    got = R.gemv(ttype, bb, rows, K, ks, q8, d8)
    assert np.isfinite(want).all() and want.any()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (ks, np.abs(got - want).max())


def test_refused_arguments():
    import trackiellm_amd as tk
    x = np.zeros(2048, np.float32)
    out = np.zeros(8 * 66, np.uint8)
    xp, op = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for name in ENTRY.values():
        fn = getattr(tk.lib(), name)
        fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        assert fn(xp, 8, op) == 0 and fn(xp, 0, op) == 0
        assert fn(None, 1, op) != 0 and fn(xp, 1, None) != 0 and fn(xp, -1, op) != 0
    old = tk.lib().tk_mi355x_quantize_blocks
    old.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    for bad in (34, 35):
        assert old(bad, xp, 1, op) != 0
    assert old(14, xp, 1, op) == 0                                               # the pinned set is as it was


def all_of(ttype):
    """a tiny llama GGUF source whose every layer matrix is `ttype` (the host quantiser's blocks), token_embd Q4_K, output Q6_K, norms F32:
    llama.cpp's recipe for file types 36 / 37"""
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
            if layer < 0 and which == O.T_TOKEN_EMBD:
                return O.TYPE_Q4_K, O.quantize_rows(O.TYPE_Q4_K, orc.dequant(layer, which, cfg.vocab, D))
            if layer >= 0 and which in shape:
                return ttype, tk.quantize_blocks(ttype, orc.dequant(layer, which, *shape[which])).reshape(-1)
            return t, buf
    return Src(), cfg


@pytest.mark.parametrize("ttype", TYPES)
def test_gguf_with_tq_tensors_passes_the_probe_and_the_tokenizer_and_short_data_is_refused(tmp_path, ttype):
    """a file in the 36 / 37 recipe: the probe accepts it and reads its geometry, the tokenizer entry reads its vocabulary; a file that ends
    one block early, or whose ffn_down claims a K running past the end of the file or wrapping the element count, comes back 3004"""
    import trackiellm_amd as tk
    src, cfg = all_of(ttype)
    p = str(tmp_path / "whole.gguf")
    G.write_llama_gguf(p, src, cfg)
    raw = bytearray(open(p, "rb").read())
    for name, want in (("token_embd.weight", 12), ("output.weight", 14), ("blk.0.attn_q.weight", ttype), ("blk.1.ffn_down.weight", ttype)):
        at = raw.index(G._s(name)) + len(G._s(name))
        ndim = struct.unpack_from("<I", raw, at)[0]
        assert struct.unpack_from("<I", raw, at + 4 + 8 * ndim)[0] == want, name
    hp = tk.LlmHParams()
    nv = C.c_int32(0)
    assert tk.lib().tk_mi355x_gguf_probe(p.encode(), C.byref(hp), C.byref(nv)) == 0
    assert (hp.n_layer, hp.d_model, hp.d_ff, hp.vocab, nv.value) == (cfg.n_layer, cfg.d_model, cfg.d_ff, cfg.vocab, cfg.vocab)
    ids = np.zeros(16, np.int32)
    n_ids = tk.lib().tk_mi355x_gguf_tokenize(p.encode(), b"hello world", 1, ids.ctypes.data_as(C.c_void_p), 16)
    assert ids[:n_ids].tolist() == [1, 263, 273]
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
