"""A plain NumPy float64 evaluation of the ONNX operators the graph executor (csrc/nn/tk_onnx_exec*.hip) implements, written from the
ONNX operator specification — loops where that is clearest — and the error bounds the per-op tests hold the executor to.

Nothing here knows the executor's accumulation order or shares code with the float32 oracle: the inputs are the float32 tensors of a case,
every value is computed in float64, and attributes are taken at their float32 value (that is what the file stores).  For contractions the
evaluation also yields S = sum |a_k| |b_k| (+ |bias|) per output element and n, the number of accumulated terms, for the bound
|got - ref| <= gamma(n + 2) S.

run(spec, feeds, floats, ints, opset) evaluates a list of node dicts ({"op", "in", "out", "attrs"}, as tests/onnx_util.spec_nodes takes
them) and returns name -> Ref(value, info)."""
import math

import numpy as np

U = 2.0 ** -24
FLT_MIN = 2.0 ** -126
TOL = 2e-5  # x max|ref|: tests/test_depth_gpu.py


def gamma(n):
    return n * U / (1.0 - n * U)


class Ref:
    def __init__(self, v, info=None):
        self.v = v              # float64 (or int64 / bool) ndarray
        self.info = info or {}  # "S", "n" of a contraction; "x", "z" of Pow; "n" of Softmax

    @property
    def shape(self):
        return tuple(self.v.shape)


def _attrs(nd):
    """attributes at the precision the file stores: floats are float32"""
    out = {}
    for k, v in nd["attrs"].items():
        if isinstance(v, float):
            out[k] = float(np.float32(v))
        elif isinstance(v, (list, tuple)) and len(v) and isinstance(v[0], float):
            out[k] = [float(np.float32(t)) for t in v]
        else:
            out[k] = v
    return out


# ------------------------------------------------------------------ convolutions

def _auto_pads(ap, in_, k, s, d):
    """SAME_UPPER / SAME_LOWER: output = ceil(in / stride); an odd total puts the extra cell at the end (UPPER) or the beginning (LOWER)"""
    out = -(-in_ // s)
    total = max(0, (out - 1) * s + (k - 1) * d + 1 - in_)
    begin = total // 2 if ap == "SAME_UPPER" else total - total // 2
    return begin, total - begin


def conv2d(x, w, b, strides=(1, 1), dilations=(1, 1), pads=(0, 0, 0, 0), group=1, auto_pad="NOTSET"):
    N, C, H, W = x.shape
    M, Cg, kh, kw = w.shape
    sh, sw = strides
    dh, dw = dilations
    pt, pl, pb, pr = pads
    if auto_pad in ("SAME_UPPER", "SAME_LOWER"):
        pt, pb = _auto_pads(auto_pad, H, kh, sh, dh)
        pl, pr = _auto_pads(auto_pad, W, kw, sw, dw)
    elif auto_pad == "VALID":
        pt = pl = pb = pr = 0
    assert C == Cg * group and M % group == 0
    Ho = (H + pt + pb - dh * (kh - 1) - 1) // sh + 1
    Wo = (W + pl + pr - dw * (kw - 1) - 1) // sw + 1
    xp = np.zeros((N, C, H + pt + pb, W + pl + pr))
    xp[:, :, pt:pt + H, pl:pl + W] = x
    y = np.zeros((N, M, Ho, Wo))
    mg = M // group
    for m in range(M):
        g = m // mg
        for i in range(kh):
            for j in range(kw):
                patch = xp[:, g * Cg:(g + 1) * Cg, i * dh:i * dh + (Ho - 1) * sh + 1:sh, j * dw:j * dw + (Wo - 1) * sw + 1:sw]
                y[:, m] += (patch * w[m, :, i, j][None, :, None, None]).sum(axis=1)
    if b is not None:
        y += b[None, :, None, None]
    return y


def conv_transpose2d(x, w, b, strides=(1, 1), pads=(0, 0, 0, 0), output_padding=(0, 0)):
    """every input pixel scatters its kernel-sized patch at (iy sh, ix sw); pads crop the borders, output_padding extends the far ones"""
    N, Ci, H, W = x.shape
    _, Co, kh, kw = w.shape
    sh, sw = strides
    pt, pl, pb, pr = pads
    fh, fw = (H - 1) * sh + kh + output_padding[0], (W - 1) * sw + kw + output_padding[1]
    full = np.zeros((N, Co, fh, fw))
    for iy in range(H):
        for ix in range(W):
            full[:, :, iy * sh:iy * sh + kh, ix * sw:ix * sw + kw] += np.einsum("nc,cokl->nokl", x[:, :, iy, ix], w)
    y = full[:, :, pt:fh - pb, pl:fw - pr].copy()
    if b is not None:
        y += b[None, :, None, None]
    return y


def _with_S(fn, arrays, n):
    """a contraction and its S: the same function over the absolute values"""
    v = fn(*arrays)
    S = fn(*[None if a is None else np.abs(a) for a in arrays])
    return v, {"S": S, "n": n}


# ------------------------------------------------------------------ pools

def pool_out_dim(in_, k, s, pa, pz, ceil_mode):
    num = in_ + pa + pz - k
    o = (-(-num // s) if ceil_mode else num // s) + 1
    if ceil_mode and (o - 1) * s >= in_ + pa:  # the last window must start inside the input or its leading pad
        o -= 1
    return o


def pool2d(x, kind, kernel, strides=(1, 1), pads=(0, 0, 0, 0), ceil_mode=0, count_include_pad=0, divisor=None):
    """MaxPool / AveragePool.  The divisor of an average with count_include_pad = 1 counts the cells of the window inside the PADDED
    extent [-pad_begin, in + pad_end): cells a ceil_mode window reaches beyond it are not counted (torch.avg_pool2d, which ONNX's
    operator tests follow).  divisor="khkw" is the deliberately wrong rule of the sensitivity test."""
    N, C, H, W = x.shape
    kh, kw = kernel
    sh, sw = strides
    pt, pl, pb, pr = pads
    Ho, Wo = pool_out_dim(H, kh, sh, pt, pb, ceil_mode), pool_out_dim(W, kw, sw, pl, pr, ceil_mode)
    y = np.zeros((N, C, Ho, Wo))
    S = np.zeros((N, C, Ho, Wo))
    for oh in range(Ho):
        hs = oh * sh - pt
        h0, h1 = max(hs, 0), min(hs + kh, H)
        for ow in range(Wo):
            ws = ow * sw - pl
            w0, w1 = max(ws, 0), min(ws + kw, W)
            win = x[:, :, h0:h1, w0:w1]
            if kind == "max":
                y[:, :, oh, ow] = win.max(axis=(2, 3))
                continue
            if divisor == "khkw":
                div = kh * kw
            elif count_include_pad:
                div = (min(hs + kh, H + pb) - hs) * (min(ws + kw, W + pr) - ws)
            else:
                div = (h1 - h0) * (w1 - w0)
            y[:, :, oh, ow] = win.sum(axis=(2, 3)) / div
            S[:, :, oh, ow] = np.abs(win).sum(axis=(2, 3)) / div
    return y, {"S": S, "n": kh * kw, "ulp": 1}


# ------------------------------------------------------------------ Resize

def resize_coords(in_, out, scale, ct, dtype=np.float64):
    """source coordinate of every output index along one axis (ONNX Resize, coordinate_transformation_mode)"""
    o = np.arange(out).astype(dtype)
    scale = dtype(scale)
    if ct == "align_corners":
        return o * dtype(in_ - 1) / dtype(out - 1) if out > 1 else np.zeros(out, dtype)
    if ct == "asymmetric":
        return o / scale
    if ct == "pytorch_half_pixel" and out <= 1:
        return np.zeros(out, dtype)
    return (o + dtype(0.5)) / scale - dtype(0.5)


def nearest_index(c, in_, nm):
    if nm == "floor":
        r = np.floor(c)
    elif nm == "ceil":
        r = np.ceil(c)
    elif nm == "round_prefer_ceil":
        r = np.floor(c + 0.5)
    else:  # round_prefer_floor
        r = np.ceil(c - 0.5)
    return np.clip(r.astype(np.int64), 0, in_ - 1)


def resize_geometry(H, W, scales=None, sizes=None):
    """(Ho, Wo, sh, sw): with scales the output is floor(in x scale) and the scale is used as given; with sizes the scale is out / in"""
    if sizes is not None:
        Ho, Wo = int(sizes[2]), int(sizes[3])
        return Ho, Wo, Ho / H, Wo / W
    sh, sw = float(np.float32(scales[2])), float(np.float32(scales[3]))
    return int(math.floor(H * sh)), int(math.floor(W * sw)), sh, sw


def resize(x, mode, ct, nm, scales=None, sizes=None):
    N, C, H, W = x.shape
    Ho, Wo, sh, sw = resize_geometry(H, W, scales, sizes)
    cy, cx = resize_coords(H, Ho, sh, ct), resize_coords(W, Wo, sw, ct)
    if mode == "nearest":
        iy, ix = nearest_index(cy, H, nm), nearest_index(cx, W, nm)
        return x[:, :, iy][:, :, :, ix]
    cy, cx = np.clip(cy, 0, H - 1), np.clip(cx, 0, W - 1)
    y0, x0 = np.floor(cy).astype(np.int64), np.floor(cx).astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    dy, dx = (cy - y0)[None, None, :, None], (cx - x0)[None, None, None, :]
    g = lambda a, b: x[:, :, a][:, :, :, b]
    return (1 - dy) * ((1 - dx) * g(y0, x0) + dx * g(y0, x1)) + dy * ((1 - dx) * g(y1, x0) + dx * g(y1, x1))


# ------------------------------------------------------------------ LSTM

def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def lstm(X, W, R, B=None, h0=None, c0=None):
    """ONNX LSTM, forward, default activations; gate rows of W / R / B in the order i, o, f, c.  X [T, batch, I] -> Y [T, 1, batch, H]"""
    T, nb, _ = X.shape
    H = R.shape[2]
    Wm, Rm = W[0], R[0]
    bias = np.zeros(4 * H) if B is None else B.reshape(-1)[:4 * H] + B.reshape(-1)[4 * H:]
    h = np.zeros((nb, H)) if h0 is None else h0.reshape(nb, H).copy()
    c = np.zeros((nb, H)) if c0 is None else c0.reshape(nb, H).copy()
    Y = np.zeros((T, 1, nb, H))
    for t in range(T):
        g = X[t] @ Wm.T + h @ Rm.T + bias
        i, o, f, cc = _sigmoid(g[:, :H]), _sigmoid(g[:, H:2 * H]), _sigmoid(g[:, 2 * H:3 * H]), np.tanh(g[:, 3 * H:])
        c = f * c + i * cc
        h = o * np.tanh(c)
        Y[t, 0] = h
    return Y, h[None], c[None]


# ------------------------------------------------------------------ the interpreter

_erf = np.vectorize(math.erf, otypes=[np.float64])


def _axes_arg(at, ins, idx, rank):
    axes = at.get("axes")
    if axes is None and len(ins) > idx and ins[idx] is not None:
        axes = [int(a) for a in np.asarray(ins[idx]).reshape(-1)]
    return None if axes is None else [a + rank if a < 0 else a for a in axes]


def _eval(nd, ins, at, opset):
    """-> list of outputs, each an array or (array, info)"""
    op = nd["op"]
    x = ins[0] if ins else None
    with np.errstate(all="ignore"):
        if op in ("Identity", "Dropout", "Cast"):
            return [x]
        if op == "Relu":
            return [np.maximum(x, 0.0)]
        if op == "Abs":
            return [np.abs(x)]
        if op == "Neg":
            return [-x]
        if op == "Sigmoid":
            return [_sigmoid(x)]
        if op == "Tanh":
            return [np.tanh(x)]
        if op == "Sqrt":
            return [np.sqrt(x)]
        if op == "Exp":
            return [np.exp(x)]
        if op == "Log":
            return [np.log(x)]
        if op == "Erf":
            return [_erf(x)]
        if op == "Gelu":
            if at.get("approximate", "none") == "tanh":
                return [0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))]
            return [0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))]
        if op == "LeakyRelu":
            return [np.where(x >= 0, x, x * at.get("alpha", float(np.float32(0.01))))]
        if op == "HardSigmoid":
            a, b = at.get("alpha", float(np.float32(0.2))), at.get("beta", 0.5)
            return [(np.clip(a * x + b, 0.0, 1.0), {"S": np.abs(a * x) + abs(b), "n": 1})]
        if op == "HardSwish":
            return [(x * np.clip(x / 6.0 + 0.5, 0.0, 1.0), {"S": np.abs(x) * (np.abs(x) / 6.0 + 0.5), "n": 2})]
        if op == "Clip":
            lo = at["min"] if "min" in at else -np.inf
            hi = at["max"] if "max" in at else np.inf
            if len(ins) > 1 and ins[1] is not None:
                lo = float(ins[1].reshape(-1)[0])
            if len(ins) > 2 and ins[2] is not None:
                hi = float(ins[2].reshape(-1)[0])
            return [np.minimum(np.maximum(x, lo), hi)]
        if op in ("Add", "Sub", "Mul", "Div", "Max", "Min"):
            f = {"Add": np.add, "Sub": np.subtract, "Mul": np.multiply, "Div": np.divide, "Max": np.maximum, "Min": np.minimum}[op]
            return [f(x, ins[1])]
        if op == "Pow":
            xb, zb = np.broadcast_arrays(x, ins[1])
            return [(np.power(xb, zb), {"x": xb, "z": zb})]
        if op in ("Greater", "Less", "Equal"):
            return [{"Greater": np.greater, "Less": np.less, "Equal": np.equal}[op](x, ins[1])]
        if op == "Where":
            return [np.where(np.asarray(x).astype(bool), ins[1], ins[2])]
        if op == "Expand":
            shape = [int(s) for s in ins[1].reshape(-1)]
            return [np.broadcast_to(x, np.broadcast_shapes(x.shape, tuple(shape))).copy()]
        if op == "MatMul":
            return [_with_S(np.matmul, [x, ins[1]], x.shape[-1])]
        if op == "Gemm":
            assert not at.get("transA", 0) and at.get("alpha", 1.0) == 1.0 and at.get("beta", 1.0) == 1.0
            c = ins[2] if len(ins) > 2 else None
            fn = lambda a, b, cc: a @ (b.T if at.get("transB", 0) else b) + (0.0 if cc is None else cc)
            return [_with_S(fn, [x, ins[1], c], x.shape[-1])]
        if op == "Conv":
            w, b = ins[1], ins[2] if len(ins) > 2 else None
            one_d = x.ndim == 3
            k = 1 if one_d else 2
            st, dl = at.get("strides", [1] * k), at.get("dilations", [1] * k)
            pd = at.get("pads", [0] * (2 * k))
            assert len(st) == k and len(dl) == k and len(pd) == 2 * k
            if one_d:  # [N, C, L] as an image of height 1
                fn = lambda xx, ww, bb: conv2d(xx[:, :, None, :], ww[:, :, None, :], bb, (1, st[0]), (1, dl[0]), (0, pd[0], 0, pd[1]), at.get("group", 1),
                                               at.get("auto_pad", "NOTSET"))[:, :, 0, :]
            else:
                fn = lambda xx, ww, bb: conv2d(xx, ww, bb, st, dl, pd, at.get("group", 1), at.get("auto_pad", "NOTSET"))
            return [_with_S(fn, [x, w, b], int(np.prod(w.shape[1:])))]
        if op == "ConvTranspose":
            w, b = ins[1], ins[2] if len(ins) > 2 else None
            st, pd, opd = at.get("strides", [1, 1]), at.get("pads", [0, 0, 0, 0]), at.get("output_padding", [0, 0])
            assert len(st) == 2 and len(pd) == 4 and len(opd) == 2
            fn = lambda xx, ww, bb: conv_transpose2d(xx, ww, bb, st, pd, opd)
            v, info = _with_S(fn, [x, w, b], int(w.shape[0] * w.shape[2] * w.shape[3]))
            if "output_shape" in at:
                assert list(v.shape[2:]) == list(at["output_shape"]), "output_shape disagrees with strides / pads: the executor must refuse this"
            return [(v, info)]
        if op in ("MaxPool", "AveragePool"):
            st, pd = at.get("strides", [1, 1]), at.get("pads", [0, 0, 0, 0])
            assert len(st) == 2 and len(pd) == 4
            v, info = pool2d(x, "max" if op == "MaxPool" else "avg", at["kernel_shape"], st, pd, at.get("ceil_mode", 0), at.get("count_include_pad", 0))
            return [v if op == "MaxPool" else (v, info)]
        if op == "GlobalAveragePool":
            hw = x.shape[2] * x.shape[3]
            return [(x.mean(axis=(2, 3), keepdims=True), {"S": np.abs(x).mean(axis=(2, 3), keepdims=True), "n": hw, "ulp": 1})]
        if op in ("Resize", "Upsample"):
            if op == "Upsample":
                sc = at.get("scales")
                sc = ins[1].reshape(-1) if sc is None else sc
                return [resize(x, at.get("mode", "nearest"), "asymmetric", "floor", scales=sc)]
            sizes = ins[3].reshape(-1) if len(ins) > 3 and ins[3] is not None else None
            sc = ins[1] if len(ins) == 2 else (ins[2] if len(ins) > 2 else None)
            return [resize(x, at.get("mode", "nearest"), at.get("coordinate_transformation_mode", "half_pixel"), at.get("nearest_mode", "round_prefer_floor"),
                           scales=None if sc is None or sizes is not None else sc.reshape(-1), sizes=sizes)]
        if op == "Pad":
            pads = at.get("pads")
            pads = [int(p) for p in ins[1].reshape(-1)] if pads is None else pads
            r = x.ndim
            width = [(pads[i], pads[r + i]) for i in range(r)]
            if at.get("mode", "constant") == "reflect":
                return [np.pad(x, width, mode="reflect")]
            cval = at.get("value", 0.0)
            if len(ins) > 2 and ins[2] is not None:
                cval = float(ins[2].reshape(-1)[0])
            return [np.pad(x, width, mode="constant", constant_values=cval)]
        if op == "Softmax":
            r = x.ndim
            if opset < 13:  # coerced to 2-D at `axis` (default 1): every row of [prod(shape[:axis]), prod(shape[axis:])] is normalised
                ax = at.get("axis", 1)
                ax = ax + r if ax < 0 else ax
                m = x.reshape(int(np.prod(x.shape[:ax], dtype=np.int64)), -1)
                e = np.exp(m - m.max(axis=1, keepdims=True))
                return [((e / e.sum(axis=1, keepdims=True)).reshape(x.shape), {"n": m.shape[1]})]
            ax = at.get("axis", -1)
            e = np.exp(x - x.max(axis=ax, keepdims=True))
            return [(e / e.sum(axis=ax, keepdims=True), {"n": x.shape[ax]})]
        if op in ("ReduceMean", "ReduceSum", "ReduceL2", "ReduceMax", "ReduceMin"):
            axes = _axes_arg(at, ins, 1, x.ndim)
            if not axes:
                if at.get("noop_with_empty_axes", 0):
                    return [(x, {"exact": True})]  # the identity
                axes = list(range(x.ndim))
            axes = tuple(axes)
            keep = bool(at.get("keepdims", 1))
            n = int(np.prod([x.shape[a] for a in axes]))
            if op == "ReduceMax":
                return [x.max(axis=axes, keepdims=keep)]
            if op == "ReduceMin":
                return [x.min(axis=axes, keepdims=keep)]
            if op == "ReduceSum":
                return [(x.sum(axis=axes, keepdims=keep), {"S": np.abs(x).sum(axis=axes, keepdims=keep), "n": n})]
            if op == "ReduceMean":
                return [(x.mean(axis=axes, keepdims=keep), {"S": np.abs(x).mean(axis=axes, keepdims=keep), "n": n})]
            # L2: the sum of squares carries gamma(n + 1) relative, the root halves it: gamma(n + 2) |result| holds, plus the root's own ulp
            v = np.sqrt((x * x).sum(axis=axes, keepdims=keep))
            return [(v, {"S": v, "n": n, "ulp": 1})]
        if op == "LayerNormalization":
            mu = x.mean(axis=-1, keepdims=True)
            var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
            y = (x - mu) / np.sqrt(var + at.get("epsilon", float(np.float32(1e-5)))) * ins[1]
            return [y + ins[2] if len(ins) > 2 and ins[2] is not None else y]
        if op == "BatchNormalization":
            sh = [1, -1] + [1] * (x.ndim - 2)
            sc, bi, mu, var = [a.reshape(sh) for a in ins[1:5]]
            d = np.sqrt(var + at.get("epsilon", float(np.float32(1e-5))))
            # x - mean, var + eps, the root (<= 1 ulp = 2u), the division and one fma: 5.5 u on the product, 1 u on the sum -> n = 4, gamma(6)
            return [((x - mu) / d * sc + bi, {"S": np.abs(x - mu) / d * np.abs(sc) + np.abs(bi), "n": 4})]
        if op == "Gather":
            return [np.take(x, np.asarray(ins[1]).astype(np.int64), axis=at.get("axis", 0))]
        if op == "Concat":
            return [np.concatenate(ins, axis=at["axis"])]
        if op == "Transpose":
            return [np.transpose(x, at.get("perm"))]
        if op == "Split":
            ax = at.get("axis", 0)
            sizes = at.get("split")
            if sizes is None and len(ins) > 1 and ins[1] is not None:
                sizes = [int(s) for s in ins[1].reshape(-1)]
            if sizes is None:  # equal parts, the last one smaller when the axis does not divide
                k = len(nd["out"])
                each = -(-x.shape[ax] // k)
                sizes = [each] * (k - 1) + [x.shape[ax] - each * (k - 1)]
            return list(np.split(x, np.cumsum(sizes)[:-1], axis=ax))
        if op == "Slice":
            starts = at["starts"] if "starts" in at else [int(v) for v in ins[1].reshape(-1)]
            ends = at["ends"] if "ends" in at else [int(v) for v in ins[2].reshape(-1)]
            axes = at.get("axes")
            if axes is None and len(ins) > 3 and ins[3] is not None:
                axes = [int(v) for v in ins[3].reshape(-1)]
            axes = list(range(len(starts))) if axes is None else axes
            steps = [int(v) for v in ins[4].reshape(-1)] if len(ins) > 4 and ins[4] is not None else [1] * len(starts)
            sl = [slice(None)] * x.ndim
            for s, e, a, st in zip(starts, ends, axes, steps):
                assert st > 0
                sl[a] = slice(s, e, st)  # Python's clamping of positive-step slices is ONNX's
            return [x[tuple(sl)]]
        if op == "Squeeze":
            axes = _axes_arg(at, ins, 1, x.ndim)
            return [np.squeeze(x) if axes is None else np.squeeze(x, axis=tuple(axes))]
        if op == "Unsqueeze":
            axes = at.get("axes")
            axes = [int(a) for a in ins[1].reshape(-1)] if axes is None else axes
            r = x.ndim + len(axes)
            shape = list(x.shape)
            for a in sorted(a + r if a < 0 else a for a in axes):
                shape.insert(a, 1)
            return [x.reshape(shape)]
        if op == "Flatten":
            ax = at.get("axis", 1)
            ax = ax + x.ndim if ax < 0 else ax
            return [x.reshape(int(np.prod(x.shape[:ax], dtype=np.int64)), -1)]
        if op == "Reshape":
            shape = [int(s) for s in ins[1].reshape(-1)]
            shape = [x.shape[i] if s == 0 else s for i, s in enumerate(shape)]
            return [x.reshape(shape)]
        if op == "LSTM":
            opt = lambda i: ins[i] if len(ins) > i and ins[i] is not None else None
            return list(lstm(x, ins[1], ins[2], opt(3), opt(5), opt(6)))
    raise NotImplementedError(op)


def run(spec, feeds, floats=None, ints=None, opset=17):
    vals = {k: np.asarray(v, np.float32).astype(np.float64) for k, v in {**(floats or {}), **feeds}.items()}
    for k, (v, dims) in (ints or {}).items():
        a = np.asarray(v).reshape(-1)
        a = a.astype(bool) if (k == "mask" or k.startswith("bool_")) else a.astype(np.int64)
        vals[k] = a.reshape(dims if dims is not None else [a.size])
    refs = {}
    for nd in spec:
        ins = [vals[i] if i else None for i in nd["in"]]
        outs = _eval(nd, ins, _attrs(nd), opset)
        for name, o in zip(nd["out"], outs):
            if not name:
                continue
            v, info = o if isinstance(o, tuple) else (o, {})
            v = np.asarray(v)
            vals[name] = v
            refs[name] = Ref(v, dict(info, op=nd["op"]))
    return refs


# ------------------------------------------------------------------ the bounds (derived, not measured)

EXACT = {"Transpose", "Slice", "Split", "Concat", "Pad", "Gather", "Expand", "Where", "Reshape", "Flatten", "Squeeze", "Unsqueeze", "Identity", "Dropout",
         "Cast", "Resize/nearest", "Upsample/nearest", "MaxPool", "ReduceMax", "ReduceMin", "Relu", "Clip", "LeakyRelu", "Abs", "Neg", "Max", "Min",
         "Add", "Sub", "Mul", "Div"}  # moves and selects; one correctly rounded operation (double rounding through binary64 is harmless for + - x /)
CHAIN = {"MatMul", "Gemm", "Conv", "ConvTranspose", "ReduceSum", "ReduceMean", "ReduceL2", "AveragePool", "GlobalAveragePool", "BatchNormalization",
         "HardSigmoid", "HardSwish"}
SCALE = {"Erf", "Gelu", "LayerNormalization", "Resize/linear", "Upsample/linear", "LSTM"}


def ulp32(v):
    """one float32 ulp at |v|; results under FLT_MIN count with the quantum of the normal range's floor, 2^-126 x 2^-23 being below what the
    shared exp resolves: it is defined on [-87, 88] and returns 0 under e^-87 = 1.6e-38, an absolute error below FLT_MIN"""
    a = np.abs(np.asarray(v, np.float64))
    return np.where(a < FLT_MIN, FLT_MIN, np.spacing(np.minimum(a, 3e38).astype(np.float32)).astype(np.float64))


def kind_of(nd):
    op = nd["op"]
    if op in ("Resize", "Upsample"):
        return op + "/" + nd["attrs"].get("mode", "nearest")
    return op


def bits_equal(got, ref64):
    with np.errstate(all="ignore"):
        want = np.asarray(ref64, np.float64).astype(np.float32)
    got = np.asarray(got, np.float32)
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))


def ulp_distance(got, ref64):
    want = np.asarray(ref64, np.float64).astype(np.float32)
    return np.abs(np.asarray(got, np.float32).view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))


def check(kind, got, ref):
    """-> (ok per element, error / bound per element): the criterion of `kind` applied to a float32 result `got` against ref.v (float64)"""
    got64 = np.asarray(got, np.float32).astype(np.float64)
    v, info = np.asarray(ref.v, np.float64), ref.info
    if kind in ("Exp", "Log", "Sqrt"):
        # where the float32 value of the true result is an infinity, a NaN or a zero (the edges of the domain, overflow, underflow) the
        # IEEE answer is required as it is; everywhere else the op's accuracy criterion
        with np.errstate(all="ignore"):
            want = v.astype(np.float32)
        edge = ~np.isfinite(want) | (want == 0)
        if edge.any():
            ok, ratio = np.ones(v.shape, bool), np.zeros(v.shape)
            ok[edge] = bits_equal(np.asarray(got, np.float32)[edge], v[edge])
            ratio[edge] = np.where(ok[edge], 0.0, np.inf)
            if (~edge).any():
                ok[~edge], ratio[~edge] = check(kind, np.asarray(got, np.float32)[~edge], Ref(v[~edge], info))
            return ok, ratio
    err = np.abs(got64 - v)
    if kind in EXACT or info.get("exact"):
        ok = bits_equal(got, v)
        return ok, np.where(ok, 0.0, np.inf)
    if kind == "Sqrt":
        d = ulp_distance(got, v)
        return d <= 1, d.astype(np.float64)
    if kind in CHAIN:
        bound = gamma(info["n"] + 2) * info["S"] + (ulp32(v) if info.get("ulp") else 0.0)
    elif kind == "Exp":
        bound = 4e-7 * v
    elif kind == "Log":
        bound = 3e-7 * np.maximum(1.0, np.abs(v))
    elif kind in ("Tanh", "Sigmoid"):
        bound = np.full(v.shape, 3e-7)
    elif kind == "Softmax":
        bound = (2 * 4e-7 + (info["n"] + 2) * U) * v + ulp32(v)
    elif kind == "Pow":
        x, z = info["x"], info["z"]
        with np.errstate(all="ignore"):
            lnx = np.abs(np.log(np.abs(x)))
        general = (4e-7 + 3e-7 * np.abs(z) * np.maximum(1.0, np.where(np.isfinite(lnx), lnx, 0.0)) + 2 * U) * np.abs(v)
        exact = bits_equal(got, v)
        root = ulp_distance(got, v) <= 1
        ok = np.where((z == 2.0) | (z == 1.0) | (z == 0.0), exact, np.where(z == 0.5, root, err <= general))
        ok = ok | ((np.isinf(v) | np.isnan(v) | (v == 0.0)) & exact)
        with np.errstate(all="ignore"):
            ratio = np.where(ok & ~(err > 0), 0.0, err / np.where(general > 0, general, 1.0))
        return ok, np.where(np.isfinite(ratio), ratio, np.where(ok, 0.0, np.inf))
    elif kind in SCALE:
        bound = np.full(v.shape, TOL * np.max(np.abs(v))) if v.size else np.zeros(v.shape)
    else:
        raise KeyError("no criterion for " + kind)
    bound = np.broadcast_to(bound, v.shape)
    with np.errstate(all="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    return err <= bound, ratio
