"""Perception kernels one launch at a time: the test hooks tk_mi355x_gemm_probe, tk_mi355x_attention_h3_probe, tk_mi355x_nn_row_probe and tk_mi355x_edge_probe."""
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


# tk_mi355x_nn_row_probe's ops, and the launchers' kernel codes it reports
ROW_CONV_STEM, ROW_IM2COL, ROW_IM2COL1D, ROW_MAXPOOL5, ROW_UPSAMPLE2X, ROW_COPY_COLS, ROW_LAYERNORM, ROW_SOFTMAX_ROWS, ROW_ADD_ROWS, ROW_EMBED_ROWS, ROW_ATTEND1 = range(11)
SOFTMAX_GENERIC, SOFTMAX_REG, SOFTMAX_WAVE = 0, 1, 2
IM2COL_ELEMENT, IM2COL_V4 = 0, 1


class NnRowProbe(C.Structure):  # tk_mi355x_nn_row_probe_t
    _fields_ = [(n, C.c_int32) for n in ("op", "B", "H", "W", "C", "ldx", "ldy", "rows", "N", "k", "stride", "pad", "act", "add_rows", "table_rows",
                                         "pos_rows")] + [("eps", C.c_float)] + [(n, C.c_int32) for n in ("a_offset", "y_offset", "kernel")] + \
               [(n, C.c_void_p) for n in ("a", "b", "c", "idx", "pos_idx", "y", "img")] + \
               [(n, C.c_int64) for n in ("n_a", "n_b", "n_c", "n_idx", "n_y", "n_img", "q_bstride", "kv_bstride")]


def nn_row_probe(op, y, a=None, b=None, c=None, idx=None, pos_idx=None, img=None, a_offset=0, y_offset=0, device=0, **geometry):
    """ONE launch of a row / layout launcher (tk_mi355x_nn_row_probe).  y (and img): float32 arrays with the caller's initial content; COPIES are
    launched on and returned.  a / b / c: float32 inputs, idx / pos_idx: int32, as the header's table assigns them per op; geometry: the
    struct's integer fields (B, H, W, C, ldx, ldy, rows, N, k, stride, pad, act, add_rows, table_rows, pos_rows, q_bstride, kv_bstride) and eps.
    device < 0: validation and the launcher's kernel code only.  Returns (y, img or None, kernel code)."""
    a, b, c = _flat(a, np.float32), _flat(b, np.float32), _flat(c, np.float32)
    idx, pos_idx = _flat(idx, np.int32), _flat(pos_idx, np.int32)
    out = np.array(y, dtype=np.float32, order="C", copy=True)
    image = None if img is None else np.array(img, dtype=np.float32, order="C", copy=True)
    p = NnRowProbe()
    p.op, p.a_offset, p.y_offset = op, a_offset, y_offset
    for name, value in geometry.items():
        if name not in dict(NnRowProbe._fields_) or name in ("op", "kernel", "a_offset", "y_offset") or name.startswith("n_"):
            raise TypeError("nn_row_probe: no geometry field %r" % name)
        setattr(p, name, value)
    if idx is not None and pos_idx is not None and idx.size != pos_idx.size:
        raise ValueError("nn_row_probe: idx and pos_idx must have the same length")
    for name, arr in (("a", a), ("b", b), ("c", c), ("y", out), ("img", image)):
        if arr is not None:
            setattr(p, name, arr.ctypes.data)
            setattr(p, "n_" + name, arr.size)
    if idx is not None:
        p.idx, p.n_idx = idx.ctypes.data, idx.size
    if pos_idx is not None:
        p.pos_idx = pos_idx.ctypes.data
    lib().tk_mi355x_nn_row_probe.argtypes = [C.c_int, C.POINTER(NnRowProbe)]
    check(lib().tk_mi355x_nn_row_probe(device, C.byref(p)))
    return out, image, int(p.kernel)


# tk_mi355x_edge_probe's ops, and the element type of each op's arrays (a, b, y); c and y2 are float32
EDGE_FRAMES, EDGE_POWER, EDGE_LOGMEL_FINISH, EDGE_VAD_HEAD, EDGE_PREPROCESS, EDGE_DEPTH_MINMAX, EDGE_DEPTH_METRIC, EDGE_POSTPROCESS_DEPTH, EDGE_DEPTH_TO_POINTS, \
    EDGE_BOX_ATTRIBUTES = range(10)
PREPROCESS_CANONICAL, PREPROCESS_SCALED = 0, 1
_EDGE_TYPES = {EDGE_FRAMES: (np.int16, np.float32, np.float32), EDGE_PREPROCESS: (np.uint8, np.float32, np.float32),
               EDGE_BOX_ATTRIBUTES: (np.uint8, np.int32, np.int32)}


class EdgeProbe(C.Structure):  # tk_mi355x_edge_probe_t
    _fields_ = [(n, C.c_int32) for n in ("op", "B", "n_samples", "pcm_stride", "n_total", "T", "rows", "nb", "per_b", "hidden", "in_w", "in_h", "in_stride", "bpp",
                                         "out_w", "out_h", "nhwc", "width", "height", "kernel")] + [("n", C.c_int64), ("mean", C.c_float * 3), ("std_dev", C.c_float * 3)] + \
               [(n, C.c_float) for n in ("scale", "shift", "min_depth", "max_depth", "fx", "fy", "cx", "cy")] + \
               [(n, C.c_void_p) for n in ("a", "b", "c", "y", "y2")] + [(n, C.c_int64) for n in ("n_a", "n_b", "n_c", "n_y", "n_y2")]


def edge_probe(op, y, a=None, b=None, c=None, y2=None, device=0, **geometry):
    """ONE launch of a front- or back-end launcher (tk_mi355x_edge_probe).  y (and y2): arrays with the caller's initial content; COPIES are launched
    on and returned.  a / b / c: inputs, of the element types the header's table names per op; geometry: the struct's integer and float fields,
    mean / std_dev as three floats.  device < 0: validation and the launcher's answer only.  Returns (y, y2 or None, kernel)."""
    ta, tb, ty = _EDGE_TYPES.get(op, (np.float32, np.float32, np.float32))
    a, b, c = _flat(a, ta), _flat(b, tb), _flat(c, np.float32)
    out = None if y is None else np.array(y, dtype=ty, order="C", copy=True)
    out2 = None if y2 is None else np.array(y2, dtype=np.float32, order="C", copy=True)
    p = EdgeProbe()
    p.op = op
    for name, value in geometry.items():
        if name not in dict(EdgeProbe._fields_) or name in ("op", "kernel", "a", "b", "c", "y", "y2") or name.startswith("n_") and name not in ("n_samples", "n_total"):
            raise TypeError("edge_probe: no geometry field %r" % name)
        setattr(p, name, (C.c_float * 3)(*value) if name in ("mean", "std_dev") else value)
    for name, arr in (("a", a), ("b", b), ("c", c), ("y", out), ("y2", out2)):
        if arr is not None:
            setattr(p, name, arr.ctypes.data)
            setattr(p, "n_" + name, arr.size)
    lib().tk_mi355x_edge_probe.argtypes = [C.c_int, C.POINTER(EdgeProbe)]
    check(lib().tk_mi355x_edge_probe(device, C.byref(p)))
    return out, out2, int(p.kernel)
