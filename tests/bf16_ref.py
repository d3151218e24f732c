"""The BF16 / F32 (and F16) float-matrix contract restated for the tests, independent of the library: ggml's CPU arithmetic.
  BF16 (type 30): the weight is bits << 16 as fp32, exact; the activation row is rounded to bf16 (ggml_compute_fp32_to_bf16) and widened;
  F32  (type 0):  the weight as stored, the activation row unrounded;
  F16  (type 1):  the weight widened exactly, the activation row rounded through IEEE f16 (NumPy's astype, round to nearest even);
  all three: per K-split slab one fp32 fmaf chain over k ascending from +0 — oracle_lib.gemm, the oracle's C chain: bf16 x bf16 products are
  exact in fp32 only down to 2^-126, so `a * w + acc` in NumPy would round twice exactly where the edge cases live — and the slabs added in
  ascending order in np.float32."""
import numpy as np

import oracle_lib as O

F32, F16, BF16 = 0, 1, 30
NAME = {F32: "F32", F16: "F16", BF16: "BF16"}
BYTES = {F32: 4, F16: 2, BF16: 2}


def f32_to_bf16(x):
    """ggml_compute_fp32_to_bf16 on an array: uint16 bits"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return np.where(nan, (u >> 16) | 64, r).astype(np.uint16)


def bf16_to_f32(b):
    return (np.ascontiguousarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def encode(ttype, w):
    """fp32 values -> the type's stored form (uint16 bits or float32)"""
    w = np.ascontiguousarray(w, np.float32)
    if ttype == BF16:
        return f32_to_bf16(w)
    if ttype == F16:
        return w.astype(np.float16).view(np.uint16)
    return w.copy()


def decode(ttype, stored):
    if ttype == BF16:
        return bf16_to_f32(stored)
    if ttype == F16:
        return np.ascontiguousarray(stored, np.uint16).view(np.float16).astype(np.float32)
    return np.ascontiguousarray(stored, np.float32)


def round_act(ttype, x):
    """the activation operand: ggml's vec_dot_type of the weight type"""
    x = np.ascontiguousarray(x, np.float32)
    if ttype == BF16:
        return bf16_to_f32(f32_to_bf16(x))
    if ttype == F16:
        with np.errstate(over="ignore"):
            return x.astype(np.float16).astype(np.float32)
    return x


def matmul(ttype, stored, x, ks):
    """y [nrows][rows]: stored [rows][K] against x [nrows][K], K split ks ways"""
    w = decode(ttype, stored)
    a = round_act(ttype, x).reshape(-1, w.shape[1])
    K = w.shape[1]
    assert K % ks == 0
    kr = K // ks
    total = None
    for s in range(ks):
        acc = O.gemm(np.ascontiguousarray(a[:, s * kr:(s + 1) * kr]), np.ascontiguousarray(w[:, s * kr:(s + 1) * kr]))
        total = acc if total is None else (total + acc).astype(np.float32)
    return total


def lora_merge(ttype, stored, A, B, scale):
    """k_lora_merge's formula on a float matrix: delta = the fmaf chain over j from +0 (oracle_lib.gemm), w' = w + scale * delta (multiply, then
    add, each rounded once), stored back through the type's conversion"""
    w = decode(ttype, stored)
    delta = O.gemm(np.ascontiguousarray(B, np.float32), np.ascontiguousarray(A, np.float32), b_kn=True)
    merged = (w + (np.float32(scale) * delta).astype(np.float32)).astype(np.float32)
    return encode(ttype, merged)


def shapes(cfg):
    D, QD, KVD, FF = cfg.d_model, cfg.n_head * cfg.head_dim, cfg.n_kv_head * cfg.head_dim, cfg.d_ff
    return {1: (QD, D), 2: (KVD, D), 3: (KVD, D), 4: (D, QD), 6: (FF, D), 7: (FF, D), 8: (D, FF)}


class FloatSource:
    """a whole model in one float type, as tests/gguf_util.write_llama_gguf and kquant_gpu_util.install read one: every layer matrix, output and
    token_embd `ttype` (0.02 x normal values, stored through encode()), norms F32 (1 + 0.1 x normal).  type_of(layer, which) overrides a tensor's
    type.  values[(layer, which)] keeps the decoded fp32 values, row-major"""

    def __init__(self, ttype, cfg, seed=4, type_of=None):
        rng = np.random.default_rng(seed)
        self.cfg, self.t, self.values = cfg, {}, {}
        todo = [(-1, 0, cfg.vocab, cfg.d_model), (-1, 1, 1, cfg.d_model), (-1, 2, cfg.vocab, cfg.d_model)]
        for l in range(cfg.n_layer):
            todo += [(l, 0, 1, cfg.d_model), (l, 5, 1, cfg.d_model)] + [(l, w, r, c) for w, (r, c) in shapes(cfg).items()]
        for layer, which, rows, cols in todo:
            if rows == 1:
                v = (1.0 + 0.1 * rng.standard_normal(cols)).astype(np.float32)
                self.t[(layer, which)] = (F32, v.view(np.uint8).reshape(-1))
                self.values[(layer, which)] = v
                continue
            tt = ttype if type_of is None else type_of(layer, which)
            stored = encode(tt, (0.02 * rng.standard_normal((rows, cols))).astype(np.float32))
            self.t[(layer, which)] = (tt, stored.view(np.uint8).reshape(-1))
            self.values[(layer, which)] = decode(tt, stored)

    def get_tensor(self, layer, which):
        return self.t[(layer, which)]
