"""Perception kernels one launch at a time: the test hooks tk_mi355x_gemm_probe and tk_mi355x_attention_h3_probe."""
import ctypes as C

import numpy as np

from ._lib import check, lib

# tk_gemm_kernel_of's answer: family * 1000 + IM * 100 + PATH * 10 + NT
GEMM_F32, GEMM_F32_TALL, GEMM_F32_BIG, GEMM_H3_TALL, GEMM_H3_BIG = 0, 1, 2, 3, 4
ACT_NONE, ACT_SILU, ACT_GELU, ACT_SIGMOID = 0, 1, 2, 3


def gemm_code(family, im=False, path=1, nt=0):
    return family * 1000 + (100 if im else 0) + path * 10 + nt


class GemmProbe(C.Structure):  # tk_mi355x_gemm_probe_t
    _fields_ = [(n, C.c_int32) for n in ("M", "N", "K", "lda", "ldb", "ldc", "ldr", "b_kn", "act")] + [("alpha", C.c_float)] + \
               [(n, C.c_int32) for n in ("batch", "batch_inner")] + \
               [(n, C.c_int64) for n in ("sA", "sB", "sC", "sR", "sA2", "sB2", "sC2", "sR2")] + \
               [(n, C.c_int32) for n in ("b_f16", "im_C", "im_H", "im_W", "im_ldx", "im_kw", "im_stride", "im_pad", "im_Ho", "im_Wo", "fast",
                                         "a_offset", "b_offset", "kernel")] + \
               [(n, C.c_void_p) for n in ("a", "b", "bias", "residual", "c")] + \
               [(n, C.c_int64) for n in ("n_a", "n_b", "n_bias", "n_residual", "n_c")]


def _flat(x, dtype):
    return None if x is None else np.ascontiguousarray(x, dtype=dtype).reshape(-1)


def gemm_probe(a, b, c, M, N, K, lda=None, ldb=None, ldc=None, bias=None, residual=None, ldr=0, b_kn=False, act=0, alpha=1.0, batch=1, strides=(0, 0, 0, 0),
               batch_inner=0, strides2=(0, 0, 0, 0), b_f16=False, im=None, fast=False, a_offset=0, b_offset=0, device=0):
    """ONE tk_launch_gemm (tk_mi355x_gemm_probe).  a, b, bias, residual: arrays holding the operands as the descriptor addresses them (b: uint16
    f16 bits with b_f16); c: float32 array with the caller's initial content — a COPY is launched on and returned, in c's shape.
    strides / strides2 = (sA, sB, sC, sR) of the inner / outer batch level; im = dict(C, H, W, ldx, kw, stride, pad, Ho, Wo) for implicit im2col.
    device < 0: no launch, only validation and the launcher's answer.  Returns (c after the launch, kernel code)."""
    a, bias, residual = _flat(a, np.float32), _flat(bias, np.float32), _flat(residual, np.float32)
    b = _flat(b, np.uint16 if b_f16 else np.float32)
    out = np.array(c, dtype=np.float32, order="C", copy=True)
    p = GemmProbe()
    p.M, p.N, p.K = M, N, K
    p.lda = K if lda is None else lda
    p.ldb = (N if b_kn else K) if ldb is None else ldb
    p.ldc = N if ldc is None else ldc
    p.ldr, p.b_kn, p.act, p.alpha = ldr, int(b_kn), act, alpha
    p.batch, p.batch_inner = batch, batch_inner
    p.sA, p.sB, p.sC, p.sR = [int(v) for v in strides]
    p.sA2, p.sB2, p.sC2, p.sR2 = [int(v) for v in strides2]
    p.b_f16, p.fast, p.a_offset, p.b_offset = int(b_f16), int(fast), a_offset, b_offset
    if im is not None:
        p.im_C, p.im_H, p.im_W, p.im_ldx, p.im_kw = im["C"], im["H"], im["W"], im["ldx"], im["kw"]
        p.im_stride, p.im_pad, p.im_Ho, p.im_Wo = im["stride"], im["pad"], im["Ho"], im["Wo"]
    p.a, p.b, p.c = a.ctypes.data, b.ctypes.data, out.ctypes.data
    p.n_a, p.n_b, p.n_c = a.size, b.size, out.size
    if bias is not None:
        p.bias, p.n_bias = bias.ctypes.data, bias.size
    if residual is not None:
        p.residual, p.n_residual = residual.ctypes.data, residual.size
    lib().tk_mi355x_gemm_probe.argtypes = [C.c_int, C.POINTER(GemmProbe)]
    check(lib().tk_mi355x_gemm_probe(device, C.byref(p)))
    return out, int(p.kernel)


def attention_h3_probe(q, k, v, out, B, nh, Tq, Tk, d, scale, q_bstride=None, kv_bstride=None, device=0):
    """ONE tk_launch_attention_h3 (tk_mi355x_attention_h3_probe): q / out [B] x [Tq][d] rows q_bstride floats apart, k / v [B] x [Tk][d] rows
    kv_bstride apart, head h in columns [64 h, 64 h + 64).  out: the caller's initial content; a copy is launched on and returned."""
    q, k, v = _flat(q, np.float32), _flat(k, np.float32), _flat(v, np.float32)
    res = np.array(out, dtype=np.float32, order="C", copy=True)
    if res.size != q.size or k.size != v.size:
        raise ValueError("attention_h3_probe: out must have q's size and v k's")
    qb = Tq * d if q_bstride is None else q_bstride
    kb = Tk * d if kv_bstride is None else kv_bstride
    lib().tk_mi355x_attention_h3_probe.argtypes = [C.c_int] * 5 + [C.c_int64, C.c_int64, C.c_int, C.c_float] + [C.c_void_p] * 3 + [C.c_int64, C.c_int64, C.c_void_p]
    check(lib().tk_mi355x_attention_h3_probe(device, B, nh, Tq, Tk, qb, kb, d, scale, q.ctypes.data, k.ctypes.data, v.ctypes.data, q.size, k.size,
                                             res.ctypes.data))
    return res
