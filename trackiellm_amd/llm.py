"""LLM stream: tk_model_loader_* / tk_llm_runner_* and the batched tk_mi355x_llm_* extension."""
import ctypes as C

import numpy as np

from ._lib import check, lib


# GGUF tensor types the LLM path loads (the rows of tk_type_desc_of in csrc/common/tk_ggml_blocks.h), and llama.cpp's k-quant file types (fill_synthetic(ftype=...))
TYPE_F32, TYPE_F16, TYPE_Q4_0, TYPE_Q5_0, TYPE_Q8_0, TYPE_Q2_K, TYPE_Q3_K, TYPE_Q4_K, TYPE_Q5_K, TYPE_Q6_K = 0, 1, 2, 6, 8, 10, 11, 12, 13, 14
TYPE_IQ4_NL, TYPE_IQ4_XS = 20, 23
TYPE_Q4_1, TYPE_Q5_1 = 3, 7
TYPE_TQ1_0, TYPE_TQ2_0 = 34, 35  # the ternary types; a TQ1_0 matrix is installed as TQ2_0 tiles (66 resident bytes per 256 weights, not the file's 54)
TYPE_BF16 = 30  # with TYPE_F32 and TYPE_F16 the float matrix types; a model's matrices hold at most one of the three
FTYPE_Q4_1, FTYPE_Q5_1 = 3, 9  # GGUF metadata only: fill_synthetic refuses them, fill_synthetic_type(TYPE_Q4_1 / TYPE_Q5_1) makes such models
FTYPE_IQ4_NL, FTYPE_IQ4_XS = 25, 30
FTYPE_TQ1_0, FTYPE_TQ2_0 = 36, 37  # every layer matrix in the base type, token_embd Q4_K, output Q6_K
FTYPE_Q4_0, FTYPE_Q5_0, FTYPE_Q8_0 = 2, 8, 7
TYPES_OF_32 = (TYPE_Q4_0, TYPE_Q4_1, TYPE_Q5_0, TYPE_Q5_1, TYPE_Q8_0, TYPE_IQ4_NL)  # blocks of 32 weights; every other quantised type has blocks of 256
FTYPE_Q2_K, FTYPE_Q2_K_S = 10, 21
FTYPE_Q3_K_S, FTYPE_Q3_K_M, FTYPE_Q4_K_S, FTYPE_Q4_K_M, FTYPE_Q5_K_S, FTYPE_Q5_K_M = 11, 12, 14, 15, 16, 17
BLOCK_BYTES = {TYPE_Q4_0: 18, TYPE_Q5_0: 22, TYPE_Q8_0: 34, TYPE_Q2_K: 84, TYPE_Q3_K: 110, TYPE_Q4_K: 144, TYPE_Q5_K: 176, TYPE_Q6_K: 210, TYPE_IQ4_NL: 18, TYPE_IQ4_XS: 136, TYPE_Q4_1: 20, TYPE_Q5_1: 24, TYPE_TQ1_0: 54, TYPE_TQ2_0: 66}


def prefix_match(toks, records, self_slot=-1, cursor=-1):
    """the prefix cache's matching rules on hand-written records (lists of token ids, one per slot), no GPU involved: (rows of `toks` kept from
    self_slot's own record, donor slot or -1, position the donor's match ends at); cursor -1 = the kept count (tk_mi355x_prefix_match)"""
    toks = np.ascontiguousarray(toks, dtype=np.int32)
    stride = max([len(r) for r in records] + [1])
    tab = np.zeros((len(records), stride), np.int32)
    lens = np.zeros(len(records), np.int32)
    for s, r in enumerate(records):
        tab[s, :len(r)] = r
        lens[s] = len(r)
    out = (C.c_int32 * 3)()
    if lib().tk_mi355x_prefix_match(_p(toks), len(toks), _p(tab), _p(lens), len(records), stride, int(self_slot), int(cursor), out) != 0:
        raise ValueError("prefix_match: bad arguments")
    return out[0], out[1], out[2]


def lookup_draft(ctx, pred, ngram_min, ngram_max, n_draft):
    """lookup decoding's draft rule, no GPU involved (tk_mi355x_lookup_draft): the ids drafted behind the last id of `ctx` from the prediction `pred`
    (may be empty), then from `ctx` itself"""
    ctx = np.ascontiguousarray(ctx, dtype=np.int32).reshape(-1)
    pred = np.ascontiguousarray(pred, dtype=np.int32).reshape(-1)
    out = np.zeros(max(int(n_draft), 1), np.int32)
    n = lib().tk_mi355x_lookup_draft(_p(ctx) if ctx.size else None, int(ctx.size), _p(pred) if pred.size else None, int(pred.size), int(ngram_min), int(ngram_max),
                                     int(n_draft), _p(out))
    if n < 0:
        raise ValueError("lookup_draft: bad arguments")
    return out[:n].tolist()


def lookup_accept(toks, picks, eos):
    """lookup decoding's accept rule, no GPU involved (tk_mi355x_lookup_accept): the ids a verify pass that fed `toks` and picked `picks` hands out"""
    toks = np.ascontiguousarray(toks, dtype=np.int32).reshape(-1)
    picks = np.ascontiguousarray(picks, dtype=np.int32).reshape(-1)
    if toks.size != picks.size:
        raise ValueError("lookup_accept: toks and picks must have one length")
    out = np.zeros(max(int(toks.size), 1), np.int32)
    n = lib().tk_mi355x_lookup_accept(_p(toks) if toks.size else None, _p(picks) if picks.size else None, int(toks.size), int(eos), _p(out))
    if n < 0:
        raise ValueError("lookup_accept: bad arguments")
    return out[:n].tolist()


class LlmHParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_layer", "d_model", "n_head", "n_kv_head", "head_dim", "d_ff", "vocab")] + \
               [("rms_eps", C.c_float), ("rope_theta", C.c_float)] + \
               [(n, C.c_int32) for n in ("ks_qkv", "ks_o", "ks_gateup", "ks_down", "ks_out")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def lora_probe(path):
    """(rank, alpha, tensor pairs) of a LoRA adapter file; no GPU involved"""
    r, a, n = C.c_int32(0), C.c_float(0), C.c_int32(0)
    check(lib().tk_mi355x_lora_probe(path.encode(), C.byref(r), C.byref(a), C.byref(n)))
    return r.value, a.value, n.value


# the types with a host quantiser entry of their own, tk_mi355x_quantize_blocks_<name>; tk_mi355x_quantize_blocks(type, ...) takes the others
QUANTIZE_ENTRY = {TYPE_Q2_K: "q2k", TYPE_Q4_0: "q4_0", TYPE_Q5_0: "q5_0", TYPE_Q4_1: "q4_1", TYPE_Q5_1: "q5_1", TYPE_IQ4_NL: "iq4_nl", TYPE_IQ4_XS: "iq4_xs",
                  TYPE_TQ1_0: "tq1_0", TYPE_TQ2_0: "tq2_0"}


def quantize_blocks(ttype, x):
    """the build's own block quantiser on the host, no GPU (tk_mi355x_quantize_blocks; tk_mi355x_quantize_blocks_q2k for TYPE_Q2_K,
    tk_mi355x_quantize_blocks_q4_0 / _q5_0 / _q4_1 / _q5_1 / _iq4_nl / _iq4_xs / _tq1_0 / _tq2_0 for TYPE_Q4_0 / TYPE_Q5_0 / TYPE_Q4_1 / TYPE_Q5_1 / TYPE_IQ4_NL / TYPE_IQ4_XS / TYPE_TQ1_0 / TYPE_TQ2_0):
    x [..., 256 n] float32 -> uint8 [n_blocks][block bytes] of k-quant `ttype`; TYPE_Q4_0 / TYPE_Q5_0 / TYPE_Q8_0 / TYPE_IQ4_NL: blocks of 32 weights,
    [n / 32][18 / 22 / 34 / 18]"""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 32 if ttype in TYPES_OF_32 else 256)
    out = np.empty((x.shape[0], BLOCK_BYTES[ttype]), np.uint8)
    if ttype in QUANTIZE_ENTRY:
        fn = getattr(lib(), "tk_mi355x_quantize_blocks_" + QUANTIZE_ENTRY[ttype])
        fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        check(fn(_p(x), x.shape[0], _p(out)))
        return out
    lib().tk_mi355x_quantize_blocks.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    check(lib().tk_mi355x_quantize_blocks(ttype, _p(x), x.shape[0], _p(out)))
    return out


def gemv_probe(ttype, blocks, rows, K, ks, x, device=0):
    """one production mat-vec (tk_mi355x_llm_gemv_probe): raw GGUF blocks [rows][K / 256] of `ttype` ([rows][K / 32] for the TYPES_OF_32) against x [nrows][K] with K split ks
    ways; returns y [nrows][rows] float32"""
    blocks = np.ascontiguousarray(blocks).view(np.uint8).reshape(-1)
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, K)
    y = np.empty((x.shape[0], rows), np.float32)
    lib().tk_mi355x_llm_gemv_probe.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    check(lib().tk_mi355x_llm_gemv_probe(device, ttype, _p(blocks), rows, K, ks, x.shape[0], _p(x), _p(y)))
    return y


# tk_mi355x_llm_step_probe's ops
STEP_EMBED, STEP_RMSNORM, STEP_RESIDUAL_FOLD, STEP_SWIGLU, STEP_QUANT, STEP_ROPE_APPEND, STEP_PV_JOIN, STEP_ATT_TILES, STEP_FUSED_NORM, STEP_FUSED_SWIGLU, STEP_WIDE_SWIGLU = range(11)
STEP_IMAGE_OPS = (STEP_RMSNORM, STEP_SWIGLU, STEP_QUANT, STEP_PV_JOIN, STEP_WIDE_SWIGLU)
ROUND_NONE, ROUND_F16, ROUND_BF16 = 0, 1, 2


class LlmStepProbe(C.Structure):  # tk_mi355x_llm_step_probe_t
    _fields_ = [(n, C.c_int32) for n in ("op", "nrows", "K", "ks", "n_total", "af_round", "type", "vocab", "n_head", "n_kv_head", "head_dim", "n_layer", "max_seq",
                                          "max_ctx", "layer")] + [("eps", C.c_float)] + \
               [(n, C.c_void_p) for n in ("x", "partial", "w", "embd", "tok", "seq", "pos", "rope_cos", "rope_sin", "qbuf", "kcache", "vcache", "pv_part", "l_part",
                                           "tiles", "aq", "ad", "abs", "abs16", "af")] + \
               [(n, C.c_int64) for n in ("n_x", "n_partial", "n_w", "n_embd", "n_rows", "n_rope", "n_qbuf", "n_cache", "n_pv", "n_l", "n_tiles", "n_aq", "n_ad", "n_abs",
                                          "n_abs16", "n_af")] + \
               [(n, C.c_void_p) for n in ("wblocks", "y_a", "y_b", "x_b", "aq_b", "ad_b", "abs_b", "abs16_b")] + \
               [(n, C.c_int64) for n in ("n_wblocks", "n_y", "n_xb")] + [(n, C.c_int32) for n in ("wtype", "wrows", "fks", "reserved")]


_STEP_ARRAYS = {"x": (np.float32, "n_x"), "partial": (np.float32, "n_partial"), "w": (np.float32, "n_w"), "embd": (np.uint8, "n_embd"), "tok": (np.int32, "n_rows"),
                "seq": (np.int32, "n_rows"), "pos": (np.int32, "n_rows"), "rope_cos": (np.float32, "n_rope"), "rope_sin": (np.float32, "n_rope"),
                "qbuf": (np.float32, "n_qbuf"), "kcache": (np.uint16, "n_cache"), "vcache": (np.uint16, "n_cache"), "pv_part": (np.float32, "n_pv"),
                "l_part": (np.float32, "n_l"), "tiles": (np.int32, "n_tiles"), "aq": (np.int8, "n_aq"), "ad": (np.float32, "n_ad"), "abs": (np.int8, "n_abs"),
                "abs16": (np.uint16, "n_abs16"), "af": (np.float32, "n_af"), "wblocks": (np.uint8, "n_wblocks"), "y_a": (np.float32, "n_y"), "y_b": (np.float32, "n_y"),
                "x_b": (np.float32, "n_xb"), "aq_b": (np.int8, None), "ad_b": (np.float32, None), "abs_b": (np.int8, None), "abs16_b": (np.uint16, None)}
_STEP_OUT = ("x", "qbuf", "kcache", "vcache", "tiles", "aq", "ad", "abs", "abs16", "af", "y_a", "y_b", "x_b", "aq_b", "ad_b", "abs_b", "abs16_b")
_STEP_SCALARS = ("nrows", "K", "ks", "n_total", "af_round", "type", "vocab", "n_head", "n_kv_head", "head_dim", "n_layer", "max_seq", "max_ctx", "layer", "wtype", "wrows", "fks")


def llm_step_probe(op, device=0, image_fill=None, **kw):
    """ONE launch of a step launcher of the LLM stream (tk_mi355x_llm_step_probe).  Keywords: the struct's scalars (nrows, K, ks, n_total, af_round, type, vocab,
    n_head, n_kv_head, head_dim, n_layer, max_seq, max_ctx, layer, wtype, wrows, fks, eps) and its arrays by name; COPIES of the in/out arrays (x, qbuf, kcache, vcache, tiles
    the raw image aq / ad / abs / abs16 / af, and the twins' y_a, y_b, x_b and second image) come back in a dict, None where not given.  image_fill: a byte (0..255) — the image arrays not given are
    made here, every byte of them that value: aq, ad, abs, abs16, and with want_af the float image af.  device < 0 validates only"""
    p = LlmStepProbe()
    p.op = op
    keep = {}
    if image_fill is not None and op in STEP_IMAGE_OPS:
        K, M = int(kw.get("wrows" if op == STEP_WIDE_SWIGLU else "K", 0)), lib().tk_mi355x_llm_max_rows()
        if 0 < K <= 65536:
            for suffix in ("", "_b") if op == STEP_WIDE_SWIGLU else ("",):
                for name, n in (("aq", M * K), ("ad", K), ("abs", M // 16 * K), ("abs16", M // 16 * K)):
                    kw.setdefault(name + suffix, np.frombuffer(bytes([image_fill]) * (n * np.dtype(_STEP_ARRAYS[name][0]).itemsize), _STEP_ARRAYS[name][0]))
            if kw.get("want_af", False):
                kw.setdefault("af", np.frombuffer(bytes([image_fill]) * (M * K * 4), np.float32))
    kw.pop("want_af", None)
    for name, v in kw.items():
        if name in _STEP_ARRAYS:
            if v is None:
                continue
            dt, cnt = _STEP_ARRAYS[name]
            a = np.array(v, dtype=dt).reshape(-1) if name in _STEP_OUT else np.ascontiguousarray(v, dtype=dt).reshape(-1)
            keep[name] = a
            setattr(p, name, a.ctypes.data)
            if cnt is None:                                               # the second image: the counts of the first
                continue
            if cnt in ("n_rows", "n_rope", "n_cache", "n_y"):              # shared counts: the shortest array given
                have = getattr(p, cnt)
                setattr(p, cnt, a.size if have == 0 else min(have, a.size))
            else:
                setattr(p, cnt, a.size)
        elif name == "eps":
            p.eps = float(v)
        elif name in _STEP_SCALARS:
            setattr(p, name, int(v))
        else:
            raise TypeError("llm_step_probe: no field %r" % name)
    lib().tk_mi355x_llm_step_probe.argtypes = [C.c_int, C.POINTER(LlmStepProbe)]
    check(lib().tk_mi355x_llm_step_probe(device, C.byref(p)))
    return {k: keep.get(k) for k in _STEP_OUT}


# bytes of one W4A8 tile, 16 rows x 256 k (csrc/llm/tk_llm_layout.h): 16 x the bytes of a row's run, but for Q3_K and IQ4_XS, whose tiles hold
# their scales unpacked, and TQ1_0, which is installed as TQ2_0 tiles
TILE_BYTES = {t: 16 * (256 // (32 if t in TYPES_OF_32 else 256)) * b for t, b in BLOCK_BYTES.items()}
TILE_BYTES.update({TYPE_Q3_K: 16 * 114, TYPE_IQ4_XS: 16 * 144, TYPE_TQ1_0: 16 * 66})


def repack_probe(ttype, blocks, rows, K, device=0):
    """the load-time repack alone (tk_mi355x_llm_repack_probe): raw GGUF blocks [rows][K / 256] of `ttype` ([rows][K / 32] for the TYPES_OF_32) ->
    uint8 tiles [rows / 16][K / 256][TILE_BYTES[ttype]]; device < 0 runs the same lane function on the host, no GPU touched"""
    blocks = np.ascontiguousarray(blocks).view(np.uint8).reshape(-1)
    if ttype in BLOCK_BYTES and blocks.size != rows * K // (32 if ttype in TYPES_OF_32 else 256) * BLOCK_BYTES[ttype]:
        raise ValueError("repack_probe: blocks is not rows x K weights of this type")
    tiles = np.empty((max(rows // 16, 0), max(K // 256, 0), TILE_BYTES.get(ttype, 0)), np.uint8)
    lib().tk_mi355x_llm_repack_probe.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    check(lib().tk_mi355x_llm_repack_probe(device, ttype, _p(blocks), rows, K, _p(tiles)))
    return tiles


def convert_bf16(x):
    """the build's float32 -> bfloat16 rounding on the host, no GPU (tk_mi355x_convert_bf16): uint16 bits, x's shape"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty(x.shape, np.uint16)
    lib().tk_mi355x_convert_bf16.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    check(lib().tk_mi355x_convert_bf16(_p(x), x.size, _p(out)))
    return out


def matmul_float_probe(ttype, w, K, ks, x, seg_rows=None, device=0):
    """one production float matmul (tk_mi355x_llm_matmul_float_probe): w [rows][K] as uint16 bits (TYPE_F16, TYPE_BF16) or float32 (TYPE_F32), split into
    the segments seg_rows (default: one) that ride side by side in one launch, against x [nrows][K] with K split ks ways; returns y [nrows][rows] float32"""
    w = np.ascontiguousarray(w, dtype=np.float32 if ttype == TYPE_F32 else np.uint16).reshape(-1, K)
    rows = w.shape[0]
    seg = np.asarray([rows] if seg_rows is None else list(seg_rows), np.int32)
    segs = (C.c_int32 * 3)(*([int(v) for v in seg] + [0] * (3 - len(seg))))
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, K)
    y = np.empty((x.shape[0], rows), np.float32)
    lib().tk_mi355x_llm_matmul_float_probe.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                       C.c_void_p, C.c_void_p]
    check(lib().tk_mi355x_llm_matmul_float_probe(device, ttype, _p(w), rows, K, ks, len(seg), segs, x.shape[0], _p(x), _p(y)))
    return y


KV_F16, KV_Q8_0 = 0, 1


def attention_plan(nrows, n_head, n_kv_head, head_dim, max_ctx, fused=True, device=0, top_position=None, kv_type=0):
    """the attention launch a pass takes on `device`: (kernel, query heads per workgroup, positions per slot / resident chunk, slots);
    kernel 0 = k_attention, 1 = k_attention_narrow, 2 = k_attention_prefill, 3 = the long-context decode form, 5 = k_attention_far (tk_mi355x_attention_plan;
    with top_position — the pass's highest position — tk_mi355x_attention_plan_at: the session's per-pass choice); kv_type = KV_Q8_0: kernel 6, the far
    form over a Q8_0 cache, for every pass of such a session (tk_mi355x_attention_plan_kv)"""
    out = (C.c_int32 * 4)()
    if kv_type != 0:
        check(lib().tk_mi355x_attention_plan_kv(device, nrows, n_head, n_kv_head, head_dim, max_ctx, 1 if fused else 0, int(kv_type), out))
    elif top_position is None:
        check(lib().tk_mi355x_attention_plan(device, nrows, n_head, n_kv_head, head_dim, max_ctx, 1 if fused else 0, out))
    else:
        check(lib().tk_mi355x_attention_plan_at(device, nrows, n_head, n_kv_head, head_dim, max_ctx, 1 if fused else 0, int(top_position), out))
    return tuple(out)


def attention_resident_limit(n_head, n_kv_head, head_dim):
    """the largest session window whose attention keeps its score rows in LDS (kernels 0 and 1); a wider window, up to 32768 positions, runs
    kernel 5 = k_attention_far in their place (tk_mi355x_attention_resident_limit; host only, needs no device)"""
    fn = lib().tk_mi355x_attention_resident_limit
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_int, C.c_int]
    return int(fn(n_head, n_kv_head, head_dim))


def attention_plan_verify(nrows, n_head, n_kv_head, head_dim, max_ctx, top_position, device=0):
    """attention_plan for a verify pass of lookup decoding (LlmSession.forward_verify, form -1): kernel 4 = the run form of the long-context
    attention, else 2 or 0 (tk_mi355x_attention_plan_verify)"""
    out = (C.c_int32 * 4)()
    check(lib().tk_mi355x_attention_plan_verify(device, nrows, n_head, n_kv_head, head_dim, max_ctx, int(top_position), out))
    return tuple(out)


class Sampling(C.Structure):  # tk_mi355x_sampling_t
    _fields_ = [("temperature", C.c_float), ("top_p", C.c_float), ("min_p", C.c_float), ("top_k", C.c_int32), ("seed", C.c_uint64),
                ("counter", C.c_uint32), ("reserved", C.c_uint32)]


LOGPROB_MAX_TOP = 20


class TokenLogprob(C.Structure):  # tk_mi355x_token_logprob_t
    _fields_ = [("logprob", C.c_float), ("n_top", C.c_int32), ("top_ids", C.c_int32 * LOGPROB_MAX_TOP), ("top_logprobs", C.c_float * LOGPROB_MAX_TOP)]


# the same record as a NumPy dtype: arrays of records go to the library as they are, sentinels included
TOKEN_LOGPROB_DTYPE = np.dtype([("logprob", np.float32), ("n_top", np.int32), ("top_ids", np.int32, (LOGPROB_MAX_TOP,)), ("top_logprobs", np.float32, (LOGPROB_MAX_TOP,))])
assert TOKEN_LOGPROB_DTYPE.itemsize == C.sizeof(TokenLogprob)


def token_logprobs_probe(logits, rows, cols, ids, n_top, records=None, ld=None, device=0, n_logits=None):
    """ONE launch of k_token_logprobs (tk_mi355x_token_logprobs_probe): logits float32, `rows` rows of `cols` floats `ld` (default cols) apart; ids [rows]
    the chosen id of every row; n_top [rows] (-1 = the row is off).  records: a C-contiguous TOKEN_LOGPROB_DTYPE array of `rows` entries that is
    filled IN PLACE (whatever the launch does not write keeps the caller's bytes), or None for a zeroed one.  device < 0: the same row function in a
    host loop, no GPU touched.  Returns the records; a refusal raises TkError with nothing written"""
    logits = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1)
    ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
    n_top = np.ascontiguousarray(n_top, dtype=np.int32).reshape(-1)
    if records is None:
        records = np.zeros(max(int(rows), 1), TOKEN_LOGPROB_DTYPE)
    if records.dtype != TOKEN_LOGPROB_DTYPE or not records.flags.c_contiguous:
        raise ValueError("token_logprobs_probe: records must be a C-contiguous TOKEN_LOGPROB_DTYPE array")
    if ids.size < rows or n_top.size < rows or records.size < rows:
        raise ValueError("token_logprobs_probe: ids, n_top and records need one entry per row")
    f = lib().tk_mi355x_token_logprobs_probe
    f.argtypes = [C.c_int, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    check(f(int(device), int(rows), int(cols), int(cols if ld is None else ld), _p(logits), int(logits.size if n_logits is None else n_logits), _p(ids), _p(n_top),
            _p(records)))
    return records


def _vocab_image(pieces):
    """pieces (bytes each) -> (offsets uint32 [n + 1], the bytes back to back as uint8)"""
    pieces = [bytes(p) for p in pieces]
    offsets = np.zeros(len(pieces) + 1, np.uint32)
    offsets[1:] = np.cumsum([len(p) for p in pieces], dtype=np.int64)
    data = np.frombuffer(b"".join(pieces) or b"\0", dtype=np.uint8).copy()
    return offsets, data


def grammar_mask_probe(gbnf, prefixes, pieces, eos=-1, bits=None, undecided=None, device=0, vocab=None, offsets=None):
    """ONE launch of k_grammar_mask (tk_mi355x_grammar_mask_probe).  gbnf: GBNF text or None for the tool-call grammar; prefixes: one per mask row,
    bytes / str, or None for a row that is off; pieces: the vocabulary's pieces as bytes (an empty piece is never allowed); eos: the token allowed iff the
    state is complete (-1: none).  bits: uint32 [rows][(vocab + 31) // 32] filled IN PLACE (None: zeros); undecided: int32 [rows] IN PLACE (None: zeros).
    device < 0: the same walk in a host loop, no GPU touched.  vocab / offsets override what the pieces give (the refusal tests).  Returns
    (bits, undecided); a refusal raises TkError with nothing written"""
    offs, data = _vocab_image(pieces)
    if offsets is not None:
        offs = np.ascontiguousarray(offsets, dtype=np.uint32)
    n = len(pieces) if vocab is None else int(vocab)
    rows = len(prefixes)
    words = (max(n, 1) + 31) // 32
    if bits is None:
        bits = np.zeros((max(rows, 1), words), np.uint32)
    if undecided is None:
        undecided = np.zeros(max(rows, 1), np.int32)
    if bits.dtype != np.uint32 or not bits.flags.c_contiguous or undecided.dtype != np.int32 or not undecided.flags.c_contiguous:
        raise ValueError("grammar_mask_probe: bits must be C-contiguous uint32 and undecided C-contiguous int32")
    if bits.size < rows * words or undecided.size < rows or offs.size < n + 1:
        raise ValueError("grammar_mask_probe: bits, undecided or offsets are too short")
    pre = (C.c_char_p * max(rows, 1))(*[None if p is None else (p.encode() if isinstance(p, str) else bytes(p)) for p in prefixes])
    f = lib().tk_mi355x_grammar_mask_probe
    f.argtypes = [C.c_int, C.c_char_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    g = None if gbnf is None else (gbnf.encode() if isinstance(gbnf, str) else bytes(gbnf))
    check(f(int(device), g, rows, C.cast(pre, C.c_void_p), _p(data), _p(offs), n, int(eos), _p(bits), _p(undecided)))
    return bits, undecided


def time_grammar_mask(prefix, pieces, rows=1, eos=-1, iters=200, gbnf=None, device=0):
    """(ms of the state upload plus one k_grammar_mask launch over `rows` equal states, ms of the host trie walk for one row) after `prefix`
    (tk_mi355x_time_grammar_mask)"""
    offs, data = _vocab_image(pieces)
    d, h = C.c_float(0), C.c_float(0)
    f = lib().tk_mi355x_time_grammar_mask
    f.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    g = None if gbnf is None else (gbnf.encode() if isinstance(gbnf, str) else bytes(gbnf))
    check(f(int(device), g, prefix.encode() if isinstance(prefix, str) else bytes(prefix), int(rows), _p(data), _p(offs), len(pieces), int(eos), int(iters), C.byref(d),
            C.byref(h)))
    return d.value, h.value


def time_token_logprobs(rows, cols, n_top, iters=200, device=0):
    """average ms of one k_token_logprobs launch at rows x cols with every row asking for n_top alternatives (tk_mi355x_time_token_logprobs)"""
    ms = C.c_float(0)
    f = lib().tk_mi355x_time_token_logprobs
    f.argtypes = [C.c_int, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float)]
    check(f(int(device), int(rows), int(cols), int(n_top), int(iters), C.byref(ms)))
    return ms.value


def MISTRAL_7B():
    return LlmHParams(32, 4096, 32, 8, 128, 14336, 32000, 1e-5, 10000.0, 0, 0, 0, 0, 1)


def TINY():
    return LlmHParams(2, 256, 8, 2, 64, 512, 512, 1e-5, 10000.0, 0, 0, 0, 0, 1)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class LlmModel:
    def __init__(self, hparams=None, device=0, gguf=None, lora=None):
        self.h = C.c_void_p()
        if gguf is not None:
            check(lib().tk_mi355x_llm_model_load_gguf_lora(C.byref(self.h), gguf.encode(), lora.encode() if lora else None, device))
        else:
            check(lib().tk_mi355x_llm_model_create(C.byref(self.h), C.byref(hparams), device))

    @property
    def hparams(self):
        hp = LlmHParams()
        lib().tk_mi355x_llm_model_get_hparams(self.h, C.byref(hp))
        return hp

    @property
    def weight_bytes(self):
        lib().tk_mi355x_llm_model_weight_bytes.restype = C.c_uint64
        return lib().tk_mi355x_llm_model_weight_bytes(self.h)

    def fill_synthetic(self, seed, f16=False, ftype=None):
        """ftype (one of the FTYPE_* k-quant mixes) selects the recipe; None = Q4_K_M"""
        if ftype is not None:
            if f16:
                raise ValueError("fill_synthetic: f16 and ftype select different recipes; give one")
            check(lib().tk_mi355x_llm_model_fill_synthetic_ftype(self.h, C.c_uint64(seed), int(ftype)))
            return self
        fn = lib().tk_mi355x_llm_model_fill_synthetic_f16 if f16 else lib().tk_mi355x_llm_model_fill_synthetic
        check(fn(self.h, C.c_uint64(seed)))
        return self

    def fill_synthetic_float(self, seed, ttype):
        """the float checkpoint recipe in TYPE_BF16 or TYPE_F32 (fill_synthetic(f16=True) is the TYPE_F16 one): every matrix and token_embd `ttype`, norms F32"""
        check(lib().tk_mi355x_llm_model_fill_synthetic_float(self.h, C.c_uint64(seed), int(ttype)))
        return self

    def fill_synthetic_type(self, seed, ttype):
        """seeded weights by tensor type (TYPE_Q4_1, TYPE_Q5_1): every layer matrix and token_embd `ttype`, output Q6_K, norms F32"""
        check(lib().tk_mi355x_llm_model_fill_synthetic_type(self.h, C.c_uint64(seed), int(ttype)))
        return self

    def set_tensor(self, layer, which, ttype, data):
        data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        check(lib().tk_mi355x_llm_model_set_tensor(self.h, layer, which, ttype, _p(data), C.c_size_t(data.size)))

    def set_lora(self, adapter_path):
        """the adapter merged into every matrix installed from now on (set_tensor, fill_synthetic); None = none"""
        check(lib().tk_mi355x_llm_model_set_lora(self.h, adapter_path.encode() if adapter_path else None))
        return self

    @property
    def lora_merged(self):
        return lib().tk_mi355x_llm_model_lora_merged(self.h)

    def close(self):
        if self.h:
            lib().tk_mi355x_llm_model_destroy(C.byref(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LlmSession:
    def __init__(self, model, max_seq, max_ctx, kv_type=0):
        """kv_type: KV_F16, or KV_Q8_0 = the KV cache as ggml Q8_0 blocks, 17/32 of the bytes (tk_mi355x_llm_session_create_kv)"""
        self.model = model
        self.vocab = model.hparams.vocab
        self.kv_type = int(kv_type)
        self.h = C.c_void_p()
        if self.kv_type == 0:
            check(lib().tk_mi355x_llm_session_create(C.byref(self.h), model.h, max_seq, max_ctx))
        else:
            check(lib().tk_mi355x_llm_session_create_kv(C.byref(self.h), model.h, max_seq, max_ctx, self.kv_type))

    def kv_bytes(self):
        """bytes of the session's cache arrays, keys and values"""
        f = lib().tk_mi355x_llm_session_kv_bytes
        f.restype, f.argtypes = C.c_uint64, [C.c_void_p]
        return int(f(self.h))

    def kv_read_q8(self, layer, seq, pos0, n_pos):
        """the raw rows of a Q8_0 session: (k int8 [n_pos][n_kv_head][head_dim], k scale bits uint16 [n_pos][n_kv_head][head_dim / 32], v, v scales)"""
        hp = self.model.hparams
        kq = np.empty((n_pos, hp.n_kv_head, hp.head_dim), np.int8)
        kd = np.empty((n_pos, hp.n_kv_head, hp.head_dim // 32), np.uint16)
        vq, vd = np.empty_like(kq), np.empty_like(kd)
        check(lib().tk_mi355x_llm_session_kv_read_q8(self.h, layer, seq, pos0, n_pos, _p(kq), _p(kd), _p(vq), _p(vd)))
        return kq, kd, vq, vd

    def forward(self, seq, pos, tok, want_logits=True):
        seq = np.ascontiguousarray(seq, dtype=np.int32)
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        tok = np.ascontiguousarray(tok, dtype=np.int32)
        n = len(seq)
        logits = np.empty((n, self.vocab), dtype=np.float32) if want_logits else None
        am = np.empty(n, dtype=np.int32)
        check(lib().tk_mi355x_llm_forward(self.h, n, _p(seq), _p(pos), _p(tok), _p(logits), _p(am)))
        return logits, am

    def forward_sampled(self, seq, pos, tok, sampling, want_logits=True):
        """forward() with a sampling state per row: sampling = [(temperature, top_k, top_p, min_p, seed, counter), ...]; temperature <= 0
        takes the arg max for that row"""
        seq = np.ascontiguousarray(seq, dtype=np.int32)
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        tok = np.ascontiguousarray(tok, dtype=np.int32)
        n = len(seq)
        tab = (Sampling * n)()
        for r, (temp, top_k, top_p, min_p, seed, counter) in enumerate(sampling):
            tab[r] = Sampling(temp, top_p, min_p, top_k, seed, counter, 0)
        logits = np.empty((n, self.vocab), dtype=np.float32) if want_logits else None
        ids = np.empty(n, dtype=np.int32)
        check(lib().tk_mi355x_llm_forward_sampled(self.h, n, _p(seq), _p(pos), _p(tok), tab, _p(logits), _p(ids)))
        return logits, ids

    def forward_adjusted(self, seq, pos, tok, adjust, sampling=None, want_logits=True):
        """forward_sampled() with a logit adjustment per row (tk_mi355x_llm_forward_adjusted): adjust = the specs of pick.logit_adjust_rows, one per
        row (None = a neutral row); sampling as forward_sampled's, or None = every row greedy.  The logits returned are the ADJUSTED ones"""
        from .pick import logit_adjust_rows
        seq = np.ascontiguousarray(seq, dtype=np.int32)
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        tok = np.ascontiguousarray(tok, dtype=np.int32)
        n = len(seq)
        tab = None
        if sampling is not None:
            tab = (Sampling * n)()
            for r, (temp, top_k, top_p, min_p, seed, counter) in enumerate(sampling):
                tab[r] = Sampling(temp, top_p, min_p, top_k, seed, counter, 0)
        adj, keep = logit_adjust_rows(adjust)
        logits = np.empty((n, self.vocab), dtype=np.float32) if want_logits else None
        ids = np.empty(n, dtype=np.int32)
        check(lib().tk_mi355x_llm_forward_adjusted(self.h, n, _p(seq), _p(pos), _p(tok), tab, adj, _p(logits), _p(ids)))
        del keep
        return logits, ids

    def forward_logprobs(self, seq, pos, tok, n_top, adjust=None, sampling=None, want_logits=True, records=None):
        """forward_adjusted() plus log-probability records (tk_mi355x_llm_forward_logprobs): n_top [rows], -1 = that row is off; adjust and sampling as
        forward_adjusted's, or None.  records: a TOKEN_LOGPROB_DTYPE array filled in place (rows that are off and entries past a record's count keep
        the caller's bytes), or None for a zeroed one.  Returns (logits or None, ids, records)"""
        from .pick import logit_adjust_rows
        seq = np.ascontiguousarray(seq, dtype=np.int32)
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        tok = np.ascontiguousarray(tok, dtype=np.int32)
        n = len(seq)
        n_top = np.ascontiguousarray(n_top, dtype=np.int32).reshape(-1)
        if n_top.size != n:
            raise ValueError("forward_logprobs: one n_top per row")
        tab = None
        if sampling is not None:
            tab = (Sampling * n)()
            for r, (temp, top_k, top_p, min_p, seed, counter) in enumerate(sampling):
                tab[r] = Sampling(temp, top_p, min_p, top_k, seed, counter, 0)
        adj, keep = logit_adjust_rows(adjust) if adjust is not None else (None, None)
        if records is None:
            records = np.zeros(n, TOKEN_LOGPROB_DTYPE)
        if records.dtype != TOKEN_LOGPROB_DTYPE or not records.flags.c_contiguous or records.size < n:
            raise ValueError("forward_logprobs: records must be a C-contiguous TOKEN_LOGPROB_DTYPE array with one entry per row")
        logits = np.empty((n, self.vocab), dtype=np.float32) if want_logits else None
        ids = np.empty(n, dtype=np.int32)
        f = lib().tk_mi355x_llm_forward_logprobs
        f.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 9
        check(f(self.h, n, _p(seq), _p(pos), _p(tok), C.cast(tab, C.c_void_p) if tab is not None else None, C.cast(adj, C.c_void_p) if adj is not None else None,
                _p(n_top), _p(logits), _p(ids), _p(records)))
        del keep
        return logits, ids, records

    def forward_verify(self, seq, pos, tok, form=-1, want_logits=True):
        """the verify pass of lookup decoding (tk_mi355x_llm_forward_verify): greedy rows, the rows of a sequence at consecutive ascending positions
        and contiguous; every row is sampled.  form: 0 k_attention per row, 2 k_attention_prefill, 4 the run form of the long-context attention,
        -1 the session's choice.  Returns (logits or None, picks)"""
        seq = np.ascontiguousarray(seq, dtype=np.int32)
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        tok = np.ascontiguousarray(tok, dtype=np.int32)
        n = len(seq)
        logits = np.empty((n, self.vocab), dtype=np.float32) if want_logits else None
        picks = np.empty(n, dtype=np.int32)
        check(lib().tk_mi355x_llm_forward_verify(self.h, n, _p(seq), _p(pos), _p(tok), int(form), _p(logits), _p(picks)))
        return logits, picks

    def forward_rows(self, seq, pos, tok, masks=None, sampling=None, adjust=None, n_top=None, want_logits=True, records=None):
        """one sampling pass with every optional per-row table (tk_mi355x_llm_forward_rows): masks = [None | uint32 array of (vocab + 31) // 32 words]
        per row; sampling, adjust, n_top and records as forward_logprobs takes them, each None = not given.  The rows may be several consecutive
        positions of a sequence (the verify pass of a runner whose lookup scope is not 0).  Returns (logits or None, picks, records or None)"""
        from .pick import logit_adjust_rows
        seq = np.ascontiguousarray(seq, dtype=np.int32)
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        tok = np.ascontiguousarray(tok, dtype=np.int32)
        n = len(seq)
        if len(pos) != n or len(tok) != n:
            raise ValueError("forward_rows: seq, pos and tok need one entry per row")
        words = (self.vocab + 31) // 32
        mtab, mkeep = None, []
        if masks is not None:
            if len(masks) != n:
                raise ValueError("forward_rows: one mask (or None) per row")
            mtab = (C.c_void_p * n)()
            for r, m in enumerate(masks):
                if m is None:
                    continue
                m = np.ascontiguousarray(m, dtype=np.uint32).reshape(-1)
                if m.size != words:
                    raise ValueError("forward_rows: a mask holds (vocab + 31) // 32 words")
                mkeep.append(m)
                mtab[r] = m.ctypes.data
        tab = None
        if sampling is not None:
            if len(sampling) != n:
                raise ValueError("forward_rows: one sampling state per row")
            tab = (Sampling * n)()
            for r, (temp, top_k, top_p, min_p, seed, counter) in enumerate(sampling):
                tab[r] = Sampling(temp, top_p, min_p, top_k, seed, counter, 0)
        if adjust is not None and len(adjust) != n:
            raise ValueError("forward_rows: one adjustment (or None) per row")
        adj, keep = logit_adjust_rows(adjust) if adjust is not None else (None, None)
        if n_top is not None:
            n_top = np.ascontiguousarray(n_top, dtype=np.int32).reshape(-1)
            if n_top.size != n:
                raise ValueError("forward_rows: one n_top per row")
            if records is None:
                records = np.zeros(n, TOKEN_LOGPROB_DTYPE)
        if records is not None and (records.dtype != TOKEN_LOGPROB_DTYPE or not records.flags.c_contiguous or records.size < n):
            raise ValueError("forward_rows: records must be a C-contiguous TOKEN_LOGPROB_DTYPE array with one entry per row")
        logits = np.empty((n, self.vocab), dtype=np.float32) if want_logits else None
        picks = np.empty(n, dtype=np.int32)
        f = lib().tk_mi355x_llm_forward_rows
        f.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 10
        check(f(self.h, n, _p(seq), _p(pos), _p(tok), C.cast(mtab, C.c_void_p) if mtab is not None else None, C.cast(tab, C.c_void_p) if tab is not None else None,
                C.cast(adj, C.c_void_p) if adj is not None else None, _p(n_top), _p(logits), _p(picks), _p(records)))
        del keep, mkeep
        return logits, picks, records

    @property
    def last_pass_key(self):
        """the form key (csrc/llm/tk_pass_form.h) of the last pass this session ran, -1 before the first: with the head,
        5 + 4 * attention + 2 * adjusted + with records, attention 4 = the run form (tk_mi355x_llm_session_last_pass_key)"""
        k = C.c_int(-1)
        check(lib().tk_mi355x_llm_session_last_pass_key(self.h, C.byref(k)))
        return k.value

    def forward_stage(self, seq, pos, layer0, layer1, tok=None, x_in=None, x_out=None, head=False, on_host=True):
        """layers [layer0, layer1) of one pass (pipeline stage).  x_in / x_out: float32 [n][d_model] numpy arrays (on_host) or raw
        device addresses (ints, e.g. torch_tensor.data_ptr()) on this session's GPU.  Returns arg max ids when head."""
        seq = np.ascontiguousarray(seq, dtype=np.int32)
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        n = len(seq)
        if tok is not None:
            tok = np.ascontiguousarray(tok, dtype=np.int32)
        am = np.empty(n, dtype=np.int32) if head else None
        ptr = (lambda a: _p(a)) if on_host else (lambda a: None if a is None else C.c_void_p(int(a)))
        check(lib().tk_mi355x_llm_forward_stage(self.h, n, _p(seq), _p(pos), _p(tok), ptr(x_in), ptr(x_out), 1 if on_host else 0,
                                                layer0, layer1, 1 if head else 0, _p(am)))
        return am

    def kv_write(self, layer, seq, pos0, k, v):
        """k, v: uint16 (f16 bits) [n_pos][n_kv_head][head_dim]"""
        k = np.ascontiguousarray(k, dtype=np.uint16)
        v = np.ascontiguousarray(v, dtype=np.uint16)
        assert k.shape == v.shape and k.ndim == 3
        check(lib().tk_mi355x_llm_session_kv_write(self.h, layer, seq, pos0, k.shape[0], _p(k), _p(v)))

    def kv_read(self, layer, seq, pos0, n_pos):
        hp = self.model.hparams
        k = np.empty((n_pos, hp.n_kv_head, hp.head_dim), np.uint16)
        v = np.empty_like(k)
        check(lib().tk_mi355x_llm_session_kv_read(self.h, layer, seq, pos0, n_pos, _p(k), _p(v)))
        return k, v

    def kv_copy(self, src_seq, dst_seq, pos0, n_pos):
        """rows [pos0, pos0 + n_pos) of src_seq onto the same rows of dst_seq, every layer, on the device (tk_mi355x_llm_session_kv_copy)"""
        check(lib().tk_mi355x_llm_session_kv_copy(self.h, int(src_seq), int(dst_seq), int(pos0), int(n_pos)))

    def kv_shift(self, seq, p0, p1, delta):
        """rows [p0, p1) of seq become rows [p0 + delta, p1 + delta) (delta < 0) in every layer: values copied, keys re-rotated to the new positions
        (tk_mi355x_llm_session_kv_shift)"""
        check(lib().tk_mi355x_llm_session_kv_shift(self.h, int(seq), int(p0), int(p1), int(delta)))

    def time_kv_shift(self, seq, p0, p1, delta, iters):
        """(ms of one launch, bytes read + written) of that move, `iters` launches after a warm-up"""
        ms, nbytes = C.c_float(0), C.c_double(0)
        check(lib().tk_mi355x_llm_time_kv_shift(self.h, int(seq), int(p0), int(p1), int(delta), int(iters), C.byref(ms), C.byref(nbytes)))
        return ms.value, nbytes.value

    def prefill(self, tokens):
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        nseq, n_prompt = tokens.shape
        first = np.empty(nseq, dtype=np.int32)
        check(lib().tk_mi355x_llm_prefill(self.h, nseq, n_prompt, _p(tokens), _p(first)))
        return first

    def decode(self, nrows, n_steps):
        out = np.empty((n_steps, lib().tk_mi355x_llm_max_rows()), dtype=np.int32)
        ms = C.c_float(0)
        check(lib().tk_mi355x_llm_decode(self.h, nrows, n_steps, _p(out), C.byref(ms)))
        return out[:, :nrows].copy(), ms.value

    def time_gemv(self, layer, which, nrows, iters):
        ms = C.c_float(0)
        nbytes = C.c_double(0)
        check(lib().tk_mi355x_llm_time_gemv(self.h, layer, which, nrows, iters, C.byref(ms), C.byref(nbytes)))
        return ms.value, nbytes.value

    def time_attention(self, nrows, ctx, iters):
        ms = C.c_float(0)
        nbytes = C.c_double(0)
        check(lib().tk_mi355x_llm_time_attention(self.h, nrows, ctx, iters, C.byref(ms), C.byref(nbytes)))
        return ms.value, nbytes.value

    def time_kv_copy(self, n_pos, n_dst, iters):
        """(kernel ms, memcpy-form ms, bytes read + written) of copying rows [0, n_pos) of sequence 0 onto sequences 1 .. n_dst"""
        k, m, nbytes = C.c_float(0), C.c_float(0), C.c_double(0)
        check(lib().tk_mi355x_llm_time_kv_copy(self.h, n_pos, n_dst, iters, C.byref(k), C.byref(m), C.byref(nbytes)))
        return k.value, m.value, nbytes.value

    @property
    def graph_captures(self):
        """passes (and timing loops) this session has recorded into a graph so far (tk_mi355x_llm_session_graph_captures)"""
        n = C.c_uint64(0)
        check(lib().tk_mi355x_llm_session_graph_captures(self.h, C.byref(n)))
        return n.value

    def close(self):
        if self.h:
            lib().tk_mi355x_llm_session_destroy(C.byref(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KvQ8Probe(C.Structure):
    """tk_mi355x_kv_q8_probe_t (include/tk/tk_mi355x_ext.h)"""
    _fields_ = [(n, C.c_int32) for n in ("mode", "n_layer", "max_seq", "n_kv_head", "max_ctx", "head_dim", "layer", "nrows", "n_head")] + \
               [(n, C.c_void_p) for n in ("seq", "pos", "kq", "vq", "kd", "vd")] + [("n_values", C.c_int64), ("n_scales", C.c_int64)] + \
               [(n, C.c_void_p) for n in ("k16", "v16", "q", "out")] + [("n_rows_elems", C.c_int64)]


def kv_q8_probe_into(mode, kq, kd, vq, vd, seq, pos, layer=0, k16=None, v16=None, q=None, out=None, device=0, head_dim=None, n_values=None, n_scales=None,
                     n_rows_elems=None):
    """tk_mi355x_kv_q8_probe in place.  kq / vq: int8 [n_layer][max_seq][n_kv_head][max_ctx][head_dim], kd / vd: uint16 [...][max_ctx][head_dim / 32]
    (None passes NULL; the geometry then comes from the first array given).  mode 0: k16 / v16 uint16 [nrows][n_kv_head][head_dim] are quantised
    into the rows (seq[r], pos[r]) of `layer`.  mode 1: q float32 [nrows][n_head][head_dim] -> out, the attention over positions 0 .. pos[r].
    device >= 0: one production launch; device < 0: the host loops.  head_dim / n_values / n_scales / n_rows_elems override what the arrays say"""
    shape = next(a.shape for a in (kq, vq) if a is not None) if (kq is not None or vq is not None) else None
    if shape is None:
        sd = next(a.shape for a in (kd, vd) if a is not None)
        shape = sd[:4] + (sd[4] * 32,)
    for a, dt in ((kq, np.int8), (vq, np.int8), (kd, np.uint16), (vd, np.uint16), (k16, np.uint16), (v16, np.uint16), (q, np.float32), (out, np.float32)):
        if a is not None and (a.dtype != dt or not a.flags.c_contiguous):
            raise ValueError("kv_q8_probe_into: arrays must be C-contiguous and of their type")
    seq = np.ascontiguousarray(seq, dtype=np.int32)
    pos = np.ascontiguousarray(pos, dtype=np.int32)
    rows = k16 if mode == 0 else q
    p = KvQ8Probe()
    p.mode, p.layer, p.nrows = int(mode), int(layer), int(seq.size)
    p.n_layer, p.max_seq, p.n_kv_head, p.max_ctx = (int(x) for x in shape[:4])
    p.head_dim = int(shape[4] if head_dim is None else head_dim)
    p.n_head = int(q.shape[1]) if q is not None and q.ndim == 3 else int(shape[2])
    p.seq, p.pos = _p(seq), _p(pos)
    p.kq, p.vq, p.kd, p.vd = _p(kq), _p(vq), _p(kd), _p(vd)
    p.n_values = int(n_values if n_values is not None else min(a.size for a in (kq, vq) if a is not None) if (kq is not None or vq is not None) else 0)
    p.n_scales = int(n_scales if n_scales is not None else min(a.size for a in (kd, vd) if a is not None) if (kd is not None or vd is not None) else 0)
    p.k16, p.v16, p.q, p.out = _p(k16), _p(v16), _p(q), _p(out)
    p.n_rows_elems = int(n_rows_elems if n_rows_elems is not None else 0 if rows is None else rows.size)
    f = lib().tk_mi355x_kv_q8_probe
    f.argtypes = [C.c_int, C.POINTER(KvQ8Probe)]
    check(f(int(device), C.byref(p)))


def kv_q8_quantize_probe(kq, kd, vq, vd, seq, pos, k16, v16, layer=0, device=0):
    """mode 0 on COPIES of the cache arrays: returns (kq, kd, vq, vd) with the rows written"""
    c = [np.array(a, copy=True) for a in (kq, kd, vq, vd)]
    kv_q8_probe_into(0, c[0], c[1], c[2], c[3], seq, pos, layer=layer, k16=np.ascontiguousarray(k16, dtype=np.uint16), v16=np.ascontiguousarray(v16, dtype=np.uint16),
                     device=device)
    return tuple(c)


def kv_q8_attention_probe(kq, kd, vq, vd, seq, pos, q, layer=0, device=0, fill=np.nan):
    """mode 1: the attention of q [nrows][n_head][head_dim] over the cache arrays; returns out, pre-filled with `fill`"""
    q = np.ascontiguousarray(q, dtype=np.float32)
    out = np.full(q.shape, fill, np.float32)
    kv_q8_probe_into(1, kq, kd, vq, vd, seq, pos, layer=layer, q=q, out=out, device=device)
    return out


def kv_shift_probe(kcache, vcache, rope_cos, rope_sin, seq, p0, p1, delta, device=0):
    """ONE launch of k_kv_shift_rows (tk_mi355x_kv_shift_probe) on COPIES of kcache / vcache (uint16 f16 bits, [n_layer][max_seq][n_kv_head][max_ctx]
    [head_dim]), which are returned; rope_cos / rope_sin float32 [max_ctx][head_dim / 2]; device < 0: the same per-row function in a host loop.  A
    refusal raises with the copies untouched: pass arrays through kv_shift_probe_into to see that"""
    k = np.array(kcache, dtype=np.uint16, order="C", copy=True)
    v = np.array(vcache, dtype=np.uint16, order="C", copy=True)
    kv_shift_probe_into(k, v, rope_cos, rope_sin, seq, p0, p1, delta, device=device)
    return k, v


def kv_shift_probe_into(kcache, vcache, rope_cos, rope_sin, seq, p0, p1, delta, device=0, head_dim=None):
    """kv_shift_probe in place on C-contiguous uint16 arrays of 5 dimensions; None for an array passes NULL; head_dim overrides the arrays' last
    dimension (refusal tests)"""
    shape = next((a.shape for a in (kcache, vcache) if a is not None), (1, 1, 1, 1, 8))
    for a in (kcache, vcache):
        if a is not None and (a.dtype != np.uint16 or not a.flags["C_CONTIGUOUS"] or a.ndim != 5 or a.shape != shape):
            raise ValueError("kv_shift_probe_into: caches must be C-contiguous uint16 arrays of one 5-dimensional shape")
    n_layer, max_seq, n_kv_head, max_ctx, hd = shape
    for a in (rope_cos, rope_sin):
        if a is not None and (a.dtype != np.float32 or not a.flags["C_CONTIGUOUS"] or a.size < max_ctx * (hd // 2)):
            raise ValueError("kv_shift_probe_into: tables must be C-contiguous float32 arrays of [max_ctx][head_dim / 2]")
    check(lib().tk_mi355x_kv_shift_probe(int(device), n_layer, max_seq, n_kv_head, max_ctx, hd if head_dim is None else int(head_dim), _p(kcache), _p(vcache),
                                         _p(rope_cos), _p(rope_sin), int(seq), int(p0), int(p1), int(delta)))


class PipeHandle(C.Structure):
    _fields_ = [("ipc", C.c_uint8 * 64), ("bytes", C.c_uint64), ("device", C.c_int32), ("pid", C.c_int32)]

    def to_bytes(self):
        return bytes(memoryview(self))

    @classmethod
    def from_bytes(cls, b):
        return cls.from_buffer_copy(b)


class LlmPipe:
    """one stage of the layer-sharded LLM with the hand-off inside the library (tk_mi355x_pipe_*)"""

    def __init__(self, session, stage, n_stages, layer0, layer1, payload_f16=False):
        self.session, self.stage, self.n_stages = session, stage, n_stages
        self.h = C.c_void_p()
        self.handle = PipeHandle()
        check(lib().tk_mi355x_pipe_create(C.byref(self.h), session.h, stage, n_stages, layer0, layer1, 1 if payload_f16 else 0, C.byref(self.handle)))

    def connect(self, next_handle, prev_handle):
        check(lib().tk_mi355x_pipe_connect(self.h, C.byref(next_handle), C.byref(prev_handle)))

    def connect_local(self, nxt, prv):
        check(lib().tk_mi355x_pipe_connect_local(self.h, nxt.h, prv.h))

    @staticmethod
    def rccl_unique_id():
        """128 bytes naming a new RCCL communicator: made in ONE process, handed to every stage (tk_mi355x_pipe_rccl_unique_id)"""
        buf = (C.c_uint8 * 128)()
        check(lib().tk_mi355x_pipe_rccl_unique_id(buf))
        return bytes(buf)

    def connect_rccl(self, unique_id):
        """the collective transport (ncclSend / ncclRecv per boundary) instead of the mailboxes; needs one GPU per stage and FAILS otherwise"""
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        check(lib().tk_mi355x_pipe_connect_rccl(self.h, buf))

    def enqueue(self, seq, pos, tok=None, head=False):
        seq = np.ascontiguousarray(seq, dtype=np.int32)
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        if tok is not None:
            tok = np.ascontiguousarray(tok, dtype=np.int32)
        check(lib().tk_mi355x_pipe_pass(self.h, len(seq), _p(seq), _p(pos), _p(tok), 1 if head else 0))

    def decode(self, nrows, n_steps):
        check(lib().tk_mi355x_pipe_decode(self.h, nrows, n_steps))

    def sync(self, nrows=0, n_steps=0):
        out = np.zeros((max(n_steps, 1), lib().tk_mi355x_llm_max_rows()), dtype=np.int32) if n_steps else None
        check(lib().tk_mi355x_pipe_sync(self.h, _p(out), n_steps))
        return out[:n_steps, :nrows].copy() if n_steps else None

    def close(self):
        if self.h:
            lib().tk_mi355x_pipe_destroy(C.byref(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- reference surface (what trackie-core links against) ------------------------------------

class _Path(C.Structure):
    _fields_ = [("path_str", C.c_char_p), ("length", C.c_size_t), ("capacity", C.c_size_t)]


class _LoaderConfig(C.Structure):
    _fields_ = [("max_models", C.c_uint32), ("num_threads", C.c_uint32)]


class _LoadParams(C.Structure):
    _fields_ = [("model_path", C.POINTER(_Path)), ("model_type", C.c_uint32), ("force_reload", C.c_bool),
                ("gpu_layers", C.c_uint32), ("cpu_threads", C.c_uint32), ("use_mmap", C.c_bool), ("use_mlock", C.c_bool),
                ("numa", C.c_bool), ("seed", C.c_uint32), ("lora_adapter", C.c_char_p)]


class _LlmConfig(C.Structure):
    _fields_ = [("context_size", C.c_uint32), ("system_prompt", C.c_char_p), ("random_seed", C.c_uint32)]


class ModelLoader:
    def __init__(self, max_models=4):
        self.h = C.c_void_p()
        cfg = _LoaderConfig(max_models, 1)
        check(lib().tk_model_loader_create(C.byref(self.h), C.byref(cfg)))

    def load(self, path, lora_adapter=None, force_reload=False):
        """tk_model_loader_load_model; lora_adapter: a "ggla" or GGUF adapter file merged into the weights at load"""
        lib().tk_path_create.restype = C.POINTER(_Path)
        p = lib().tk_path_create(path.encode())
        params = _LoadParams(p, 1, bool(force_reload), 99, 1, True, False, False, 0, lora_adapter.encode() if lora_adapter else None)
        handle = C.c_void_p()
        try:
            check(lib().tk_model_loader_load_model(self.h, C.byref(params), C.byref(handle)))
        finally:
            lib().tk_path_destroy(C.byref(p))
        return handle

    def unload(self, handle):
        check(lib().tk_model_loader_unload_model(self.h, C.byref(handle)))

    @staticmethod
    def set_runner_slots(handle, slots):
        """sequences per shared decode session of the runners created on this model handle (before the first tk_llm_runner_create)"""
        check(lib().tk_mi355x_llm_model_set_runner_slots(handle, slots))

    @staticmethod
    def set_kv_cache_type(handle, kv_type):
        """the KV cache type of the sessions the runners of this model handle share: KV_F16 / KV_Q8_0, or llama.cpp's names "f16" / "q8_0"; before
        the first tk_llm_runner_create on the handle"""
        if isinstance(kv_type, str):
            f = lib().tk_mi355x_llm_model_set_kv_cache_type_by_name
            f.argtypes = [C.c_void_p, C.c_char_p]
            check(f(handle, kv_type.encode()))
        else:
            f = lib().tk_mi355x_llm_model_set_kv_cache_type
            f.argtypes = [C.c_void_p, C.c_int]
            check(f(handle, int(kv_type)))

    @staticmethod
    def batch_stats(handle):
        """(passes, rows, widest pass) of the continuous-batching schedulers of this model"""
        p, r, m = C.c_uint64(0), C.c_uint64(0), C.c_int32(0)
        lib().tk_mi355x_llm_model_batch_stats(handle, C.byref(p), C.byref(r), C.byref(m))
        return p.value, r.value, m.value

    @staticmethod
    def run_ahead_wasted(handle):
        """run-ahead rows of this model's schedulers that no owner came back for"""
        f = lib().tk_mi355x_llm_model_run_ahead_wasted
        f.restype = C.c_uint64
        f.argtypes = [C.c_void_p]
        return int(f(handle))

    @staticmethod
    def set_prefix_cache(handle, on):
        """prompt prefix cache of the runners of this model handle (off by default): prepare keeps the rows its slot already holds for the same
        leading tokens and copies rows another slot holds; same tokens either way"""
        check(lib().tk_mi355x_llm_model_set_prefix_cache(handle, 1 if on else 0))

    @staticmethod
    def prefix_cache_stats(handle):
        """(prompt rows asked for by prepare, of them kept, of them copied, copy launches) over this model's schedulers"""
        v = [C.c_uint64(0) for _ in range(4)]
        f = lib().tk_mi355x_llm_model_prefix_cache_stats
        f.restype = None
        f(handle, *[C.byref(x) for x in v])
        return tuple(x.value for x in v)

    def close(self):
        if self.h:
            lib().tk_model_loader_destroy(C.byref(self.h))
            self.h = C.c_void_p()


class LlmRunner:
    """tk_llm_runner_* exactly as the reference's Rust GgufRunner drives it."""

    def __init__(self, model_handle, context_size=4096, random_seed=0):
        self.h = C.c_void_p()
        cfg = _LlmConfig(context_size, None, random_seed)
        check(lib().tk_llm_runner_create(C.byref(self.h), model_handle, C.byref(cfg)))
        lib().tk_llm_runner_generate_next_token.restype = C.c_void_p

    def prepare(self, prompt, use_tool_grammar=False):
        check(lib().tk_llm_runner_prepare_generation(self.h, prompt.encode(), use_tool_grammar))

    def set_sampling(self, temperature, top_k=40, top_p=0.95, min_p=0.05):
        """the reference's default stochastic chain (llama_sampling_default_params) instead of greedy; temperature 0 = greedy again"""
        check(lib().tk_mi355x_llm_runner_set_sampling(self.h, C.c_float(temperature), top_k, C.c_float(top_p), C.c_float(min_p)))

    def set_penalties(self, last_n, repeat=1.0, freq=0.0, present=0.0):
        """repetition penalties over the last last_n accepted ids (llama_sample_repetition_penalties); last_n 0 = off; from the next sampled token"""
        check(lib().tk_mi355x_llm_runner_set_penalties(self.h, int(last_n), C.c_float(repeat), C.c_float(freq), C.c_float(present)))

    def set_logit_bias(self, ids, bias):
        """replaces the runner's bias list: logit[ids[j]] += bias[j] before everything else (-inf bans a token); empty lists clear it"""
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        bias = np.ascontiguousarray(bias, dtype=np.float32).reshape(-1)
        if ids.size != bias.size:
            raise ValueError("set_logit_bias: ids and bias must have one length")
        check(lib().tk_mi355x_llm_runner_set_logit_bias(self.h, int(ids.size), _p(ids) if ids.size else None, _p(bias) if bias.size else None))

    def recent_tokens(self):
        """the ids accepted since the last prepare(), oldest first (the most recent 256)"""
        f = lib().tk_mi355x_llm_runner_recent_tokens
        f.restype = C.c_int32
        out = np.zeros(256, np.int32)
        n = f(self.h, _p(out), 256)
        return out[:max(n, 0)].tolist()

    def add_tool_response(self, tool_name, tool_output):
        check(lib().tk_llm_runner_add_tool_response(self.h, tool_name.encode(), tool_output.encode()))

    def tool_call_text(self):
        """what the tool-call grammar has accepted since the last prepare(), as bytes (tk_mi355x_llm_runner_tool_call_text)"""
        f = lib().tk_mi355x_llm_runner_tool_call_text
        f.restype, f.argtypes = C.c_char_p, [C.c_void_p]
        return f(self.h) or b""

    def set_context_shift(self, on, n_keep=0):
        """llama.cpp's context shift instead of stopping at the end of the context (off by default): keep the first n_keep rows (-1 = the last prompt's
        token count), drop half of the rest, move the others down (tk_mi355x_llm_runner_set_context_shift)"""
        check(lib().tk_mi355x_llm_runner_set_context_shift(self.h, 1 if on else 0, int(n_keep)))

    def context_shifts(self):
        """(shifts, rows dropped by them) since the last prepare()"""
        n, d = C.c_int32(0), C.c_int64(0)
        check(lib().tk_mi355x_llm_runner_context_shifts(self.h, C.byref(n), C.byref(d)))
        return n.value, d.value

    def set_lookup(self, n_draft, ngram_min=1, ngram_max=3):
        """lookup decoding for a greedy runner (off by default; n_draft 0 = off): up to n_draft ids drafted per pass from the prediction, then from
        the context, by the longest n-gram of ngram_max .. ngram_min ids that ends the context (tk_mi355x_llm_runner_set_lookup)"""
        check(lib().tk_mi355x_llm_runner_set_lookup(self.h, int(n_draft), int(ngram_min), int(ngram_max)))

    def set_lookup_scope(self, sampled=False, grammar=False, adjusted=False, logprobs=False):
        """under which conditions a runner with lookup on still drafts (tk_mi355x_llm_runner_set_lookup_scope): with a temperature, under a grammar
        mask, with penalties or a logit bias, with log-probabilities on.  All False (the default): a greedy, unmasked, unadjusted runner only"""
        f = lib().tk_mi355x_llm_runner_set_lookup_scope
        f.argtypes = [C.c_void_p, C.c_uint32]
        check(f(self.h, (1 if sampled else 0) | (2 if grammar else 0) | (4 if adjusted else 0) | (8 if logprobs else 0)))

    def lookup_scope(self):
        """the scope's flag bits: 1 sampled, 2 grammar, 4 adjusted, 8 logprobs"""
        v = C.c_uint32(0)
        check(lib().tk_mi355x_llm_runner_get_lookup_scope(self.h, C.byref(v)))
        return v.value

    def lookup_host_ms(self):
        """(ms building the per-row masks of the verify requests, ms inside the verify requests) since the last prepare()"""
        a, b = C.c_double(0), C.c_double(0)
        check(lib().tk_mi355x_llm_runner_lookup_host_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_device_mask(self, on):
        """grammar masks built by k_grammar_mask inside the runner's passes instead of by the host's trie walk (off by default; same ids either way:
        tk_mi355x_llm_runner_set_device_mask)"""
        f = lib().tk_mi355x_llm_runner_set_device_mask
        f.argtypes = [C.c_void_p, C.c_int]
        check(f(self.h, 1 if on else 0))

    def mask_stats(self):
        """(mask rows built on the device, built on the host, requests submitted again after an undecided token) since the last prepare()"""
        d, h, r = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        f = lib().tk_mi355x_llm_runner_mask_stats
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        check(f(self.h, C.byref(d), C.byref(h), C.byref(r)))
        return d.value, h.value, r.value

    def set_grammar(self, gbnf):
        """the runner's grammar becomes this GBNF text (str or bytes), armed by prepare(..., use_tool_grammar=True); None restores the tool-call grammar
        (tk_mi355x_llm_runner_set_grammar).  A text that does not parse, or a call during a generation, raises TkError"""
        f = lib().tk_mi355x_llm_runner_set_grammar
        f.argtypes = [C.c_void_p, C.c_char_p]
        check(f(self.h, None if gbnf is None else (gbnf.encode() if isinstance(gbnf, str) else bytes(gbnf))))

    def set_lookup_scope_bits(self, flags):
        """set_lookup_scope by flag bits; unknown bits raise TkError"""
        f = lib().tk_mi355x_llm_runner_set_lookup_scope
        f.argtypes = [C.c_void_p, C.c_uint32]
        check(f(self.h, int(flags)))

    def set_logprobs(self, n_top):
        """log-probabilities of every sampled token (off by default): -1 = off, 0 = the produced id only, 1 .. 20 = that many alternatives
        (tk_mi355x_llm_runner_set_logprobs); from the next sampled token"""
        check(lib().tk_mi355x_llm_runner_set_logprobs(self.h, int(n_top)))

    def last_logprobs(self):
        """the record of the id the last prepare() / next_token() sampled, as (logprob, [(id, logprob), ...]); raises TkError while the setting is off or
        nothing has been sampled since it was switched on"""
        rec = TokenLogprob()
        check(lib().tk_mi355x_llm_runner_last_logprobs(self.h, C.byref(rec)))
        return rec.logprob, [(rec.top_ids[j], rec.top_logprobs[j]) for j in range(rec.n_top)]

    def set_prediction(self, ids):
        """the host's prediction of the reply, as token ids (copied; an empty list clears it; it survives prepare())"""
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        check(lib().tk_mi355x_llm_runner_set_prediction(self.h, _p(ids) if ids.size else None, int(ids.size)))

    def lookup_stats(self):
        """(passes that carried drafts, drafts fed, drafts accepted) since the last prepare()"""
        v, d, a = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        check(lib().tk_mi355x_llm_runner_lookup_stats(self.h, C.byref(v), C.byref(d), C.byref(a)))
        return v.value, d.value, a.value

    def last_prompt_rows(self):
        """(rows, of them kept in place, of them copied from another runner's slot) of the last prepare()"""
        n, k, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        check(lib().tk_mi355x_llm_runner_last_prompt_rows(self.h, C.byref(n), C.byref(k), C.byref(c)))
        return n.value, k.value, c.value

    def next_token(self):
        p = lib().tk_llm_runner_generate_next_token(self.h)
        if not p:
            return None
        if p == 1:
            return "<tool_call>"
        return C.string_at(p)

    def reset(self):
        check(lib().tk_llm_runner_reset_context(self.h))

    def close(self):
        if self.h:
            lib().tk_llm_runner_destroy(C.byref(self.h))
            self.h = C.c_void_p()
