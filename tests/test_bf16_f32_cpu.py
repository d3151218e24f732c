"""CPU: BF16 and F32 float matrices (GGML types 30 and 0) — the build's bfloat16 rounding against the formula restated in NumPy (tests/bf16_ref.py) byte
for byte and against torch on everything that is no NaN, the restated matmul contract against the float64 dot, the GGUF reader's size checks for
files of the two types, and the refusals of the new entry points and loader names, none of which needs a GPU."""
import ctypes as C
import struct

import numpy as np
import pytest

import bf16_ref as R
import gguf_util as G
import oracle_lib as O


def probe(path):
    import trackiellm_amd as tk
    hp = tk.LlmHParams()
    nv = C.c_int32(0)
    return tk.lib().tk_mi355x_gguf_probe(path.encode(), C.byref(hp), C.byref(nv)), hp


def edge_bits():
    """ties at the 8th mantissa bit (both parities of the kept half), one above and below a tie, the carry into the next binade and into
    infinity, subnormals (fp32's and bf16's own, smallest and largest), max-finite, infinities, zeros, NaNs with payload — both signs"""
    pos = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF, 0x3FFF8000, 0x3FFFFFFF, 0x3FFF7FFF,
           0x7F7F8000, 0x7F7F7FFF, 0x7F7FFFFF, 0x7F7F0000, 0x7F800000, 0x00000000, 0x00000001, 0x00007FFF, 0x00008000, 0x00008001,
           0x00010000, 0x00018000, 0x007F0000, 0x007F8000, 0x007FFFFF, 0x00800000, 0x00808000,
           0x7F800001, 0x7FC00000, 0x7FFFFFFF, 0x7F80FFFF, 0x7F812345, 0x7FBF0000, 0x7F800040, 0x7FABCDEF]
    return np.array(pos + [b | 0x80000000 for b in pos], np.uint32)


def test_convert_bf16_is_the_restated_formula_and_torchs_rounding():
    import torch
    import trackiellm_amd as tk
    assert (tk.TYPE_BF16, tk.TYPE_F32, tk.TYPE_F16) == (R.BF16, R.F32, R.F16) == (30, 0, 1)
    rng = np.random.default_rng(30)
    bits = np.concatenate([edge_bits(), rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32),
                           # every kept half with the dropped half exactly on, just under and just over the tie
                           (np.arange(1 << 16, dtype=np.uint32) << 16) | 0x8000, (np.arange(1 << 16, dtype=np.uint32) << 16) | 0x7FFF,
                           (np.arange(1 << 16, dtype=np.uint32) << 16) | 0x8001])
    x = bits.view(np.float32)
    got = tk.convert_bf16(x)
    want = R.f32_to_bf16(x)
    assert got.dtype == np.uint16 and np.array_equal(got, want)
    # by hand: ties go to the even kept half, 0x7f7f8000 rounds to +inf, subnormals are kept, a NaN keeps its upper payload and gains bit 6
    by_hand = {0x3F808000: 0x3F80, 0x3F818000: 0x3F82, 0x3F808001: 0x3F81, 0x3FFF8000: 0x4000, 0x7F7F8000: 0x7F80, 0x7F7F7FFF: 0x7F7F,
               0x00008000: 0x0000, 0x00008001: 0x0001, 0x00018000: 0x0002, 0x007F8000: 0x0080, 0x80000000: 0x8000, 0xFF800000: 0xFF80,
               0x7F800001: 0x7FC0, 0x7F812345: 0x7FC1, 0xFFABCDEF: 0xFFEB, 0x7FBF0000: 0x7FFF}
    for b, h in by_hand.items():
        assert int(tk.convert_bf16(np.array([b], np.uint32).view(np.float32))[0]) == h, hex(b)
    nan = np.isnan(x)
    assert nan.sum() > 100 and (np.isnan(R.bf16_to_f32(got[nan]))).all()
    tb = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(tb[~nan], got[~nan])
    # widening is exact and the rounding is idempotent
    assert np.array_equal(tk.convert_bf16(R.bf16_to_f32(got[~nan])), got[~nan])
    fn = tk.lib().tk_mi355x_convert_bf16
    fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    out = np.full(4, 0xAAAA, np.uint16)
    one = np.ones(4, np.float32)
    assert fn(one.ctypes.data, 2, out.ctypes.data) == 0 and out.tolist() == [0x3F80, 0x3F80, 0xAAAA, 0xAAAA]
    assert fn(None, 1, out.ctypes.data) != 0 and fn(one.ctypes.data, 1, None) != 0 and fn(one.ctypes.data, -1, out.ctypes.data) != 0
    assert fn(one.ctypes.data, 0, out.ctypes.data) == 0


@pytest.mark.parametrize("ttype", [R.BF16, R.F32, R.F16])
@pytest.mark.parametrize("ks", [1, 4])
def test_restated_matmul_is_within_the_running_error_bound_of_the_float64_dot(ttype, ks):
    """the restatement's slab chains against float64 sums of the same decoded operands: |y - y64| <= (K + ks) 2^-24 sum |a w|"""
    rng = np.random.default_rng(5)
    K, rows, n = 1024, 32, 5
    stored = R.encode(ttype, (0.02 * rng.standard_normal((rows, K))).astype(np.float32))
    x = rng.standard_normal((n, K)).astype(np.float32)
    y = R.matmul(ttype, stored, x, ks)
    w64, a64 = R.decode(ttype, stored).astype(np.float64), R.round_act(ttype, x).astype(np.float64)
    assert np.all(np.abs(y - a64 @ w64.T) <= (K + ks) * 2.0 ** -24 * (np.abs(a64) @ np.abs(w64).T))
    if ttype == R.BF16:
        assert not np.array_equal(R.round_act(ttype, x), x) and np.array_equal(R.decode(ttype, stored).view(np.uint32) & 0xFFFF, np.zeros((rows, K), np.uint32))
    if ttype == R.F32:
        assert np.array_equal(R.round_act(ttype, x), x)


@pytest.mark.parametrize("ttype", [R.BF16, R.F32])
def test_gguf_of_the_type_passes_the_probe_and_damaged_ones_do_not(tmp_path, ttype):
    """a whole file of the type is sized like any known type: one element short of the last tensor, a tensor claimed larger than the file and an
    element count that wraps are the reader's to refuse"""
    cfg = O.tiny_config()
    p = str(tmp_path / "whole.gguf")
    G.write_llama_gguf(p, R.FloatSource(ttype, cfg), cfg)
    raw = bytearray(open(p, "rb").read())
    for name in ("token_embd.weight", "output.weight", "blk.0.attn_q.weight", "blk.1.ffn_down.weight"):
        key = G._s(name)
        at = raw.index(key) + len(key)
        ndim = struct.unpack_from("<I", raw, at)[0]
        assert struct.unpack_from("<I", raw, at + 4 + 8 * ndim)[0] == ttype, name
    rc, hp = probe(p)
    assert rc == 0 and (hp.n_layer, hp.d_model, hp.d_ff, hp.vocab) == (cfg.n_layer, cfg.d_model, cfg.d_ff, cfg.vocab)
    # the last tensor of the file is blk.1.ffn_down, d_model x d_ff elements: a multiple of the alignment, so the file ends with its last element
    assert (cfg.d_model * cfg.d_ff * R.BYTES[ttype]) % 32 == 0
    (tmp_path / "one_short.gguf").write_bytes(bytes(raw[:-R.BYTES[ttype]]))
    assert probe(str(tmp_path / "one_short.gguf"))[0] == 3004
    name = G._s("blk.0.ffn_down.weight")
    dims_at = raw.index(name) + len(name) + 4
    assert struct.unpack_from("<QQ", raw, dims_at) == (cfg.d_ff, cfg.d_model)
    b = bytearray(raw)
    struct.pack_into("<QQ", b, dims_at, 1 << 20, 1 << 12)
    (tmp_path / "past_end.gguf").write_bytes(bytes(b))
    assert probe(str(tmp_path / "past_end.gguf"))[0] == 3004
    b = bytearray(raw)
    struct.pack_into("<QQ", b, dims_at, 1 << 63, 4)        # element count wraps
    (tmp_path / "wrap.gguf").write_bytes(bytes(b))
    assert probe(str(tmp_path / "wrap.gguf"))[0] == 3004
    b = bytearray(raw)
    struct.pack_into("<QQ", b, dims_at, 1 << 62, 2)        # elements fit 64 bits, their bytes do not
    (tmp_path / "wrap_bytes.gguf").write_bytes(bytes(b))
    assert probe(str(tmp_path / "wrap_bytes.gguf"))[0] == 3004


def test_new_entry_points_refuse_null_pointers_and_other_types():
    import trackiellm_amd as tk
    L = tk.lib()
    fsf = L.tk_mi355x_llm_model_fill_synthetic_float
    fsf.argtypes = [C.c_void_p, C.c_uint64, C.c_int]
    assert fsf(None, 4, 30) == 1001 and fsf(None, 4, 0) == 1001
    mp = L.tk_mi355x_llm_matmul_float_probe
    mp.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    w = np.zeros((16, 256), np.uint16)
    x = np.zeros((1, 256), np.float32)
    y = np.zeros((1, 16), np.float32)
    seg = (C.c_int32 * 3)(16, 0, 0)
    args = lambda t, wp=w.ctypes.data, sp=seg, xp=x.ctypes.data, yp=y.ctypes.data: mp(0, t, wp, 16, 256, 1, 1, sp, 1, xp, yp)
    assert args(30, wp=None) == 1001 and args(30, sp=None) == 1001 and args(30, xp=None) == 1001 and args(30, yp=None) == 1001
    for bad in (-1, 2, 8, 12, 14, 29, 31):
        assert args(bad) == 1001, bad
    # shapes are checked before the device is touched
    assert mp(0, 30, w.ctypes.data, 16, 256, 2, 1, seg, 1, x.ctypes.data, y.ctypes.data) == 1001      # K % (256 ks)
    assert mp(0, 30, w.ctypes.data, 16, 256, 1, 1, seg, 257, x.ctypes.data, y.ctypes.data) == 1001    # nrows
    assert mp(0, 0, w.ctypes.data, 16, 256, 1, 4, seg, 1, x.ctypes.data, y.ctypes.data) == 1001       # nseg
    assert mp(0, 1, w.ctypes.data, 32, 256, 1, 1, seg, 1, x.ctypes.data, y.ctypes.data) == 1001       # segments do not add up to rows
    seg8 = (C.c_int32 * 3)(8, 8, 0)
    assert mp(0, 30, w.ctypes.data, 16, 256, 1, 2, seg8, 1, x.ctypes.data, y.ctypes.data) == 1001     # segment rows % 16
    big = (C.c_int32 * 3)(131072, 0, 0)
    assert mp(0, 30, w.ctypes.data, 131072, 256, 1, 1, big, 1, x.ctypes.data, y.ctypes.data) == 1001  # rows > 65536: refused before w is read
    big = (C.c_int32 * 3)(32768, 0, 0)
    assert mp(0, 0, w.ctypes.data, 32768, 4096, 1, 1, big, 1, x.ctypes.data, y.ctypes.data) == 1001   # rows x K > 2^26
    # the k-quant probe keeps its set of types
    gp = L.tk_mi355x_llm_gemv_probe
    gp.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    w64 = np.zeros((64, 256), np.float32)
    y64 = np.zeros((1, 64), np.float32)
    for t in (30, 0, 1):
        assert gp(0, t, w64.ctypes.data, 64, 256, 1, 1, x.ctypes.data, y64.ctypes.data) != 0


def test_loader_names_parse():
    """-bf16 and -f32 are suffixes of the synthetic names like -f16: with an unknown base name the loader reports the base it parsed"""
    import trackiellm_amd as tk
    loader = tk.ModelLoader()
    for name, base in (("nosuch-bf16", "nosuch"), ("nosuch-f32", "nosuch"), ("nosuch-f16", "nosuch"), ("nosuch-bf16-f16", "nosuch-bf16"),
                       ("nosuch-bf17", "nosuch-bf17")):
        with pytest.raises(tk.TkError) as ei:
            loader.load(f"synthetic://{name}?seed=4")
        assert ei.value.detail == "unknown synthetic model: " + base, name
    loader.close()
