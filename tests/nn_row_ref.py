"""Reference B of the perception streams' row and layout kernels (csrc/nn/tk_nn_kernels.hip): NumPy written from the kernels' comments.  It never
imports the oracle.

expected(launch, mut) -> (y, y_bound, img, img_bound): the WHOLE in/out arrays a launch of tests/nn_row_cases.py must leave behind — what the kernel
writes, and the caller's content everywhere else (bound 0 there).  A bound of None means exact:
  im2col / im2col1d / maxpool5 / upsample2x / copy_cols   a gather: array_equal
  add_rows / embed_rows                                   one np.float32 add: array_equal
  layernorm / softmax_rows / conv_stem / attend1          float64 with bounds built term by term in the running-error form of tests/split_f16_ref.py

The bounds' constants come from csrc/common/tk_exact_math.h and IEEE arithmetic, not from a measurement of the kernels:
  U = 2^-24     one correctly rounded float32 operation (add, mul, fma, tk_divf), relative
  tk_expf       relative error <= 2^-22
  tk_sqrtf      <= 1 ulp = 2^-23 relative
  a sum of n terms in the kernels' order (256 strided partials, a 64-wide butterfly per wave, ((w0 + w1) + w2) + w3): every term passes through at most
  h = ceil(n / 256) + 8 additions, so |error| <= h U sum |term| (first order; SLACK covers the rest)

MUTATIONS: one plausible kernel error each; tests/test_nn_rows_cpu.py shows that each changes the answer of at least one GPU case by more than the bound."""
import numpy as np

U = 2.0 ** -24
EXPF_REL = 2.0 ** -22
SQRT_REL = 2.0 ** -23
SLACK = 1.01
MUTATIONS = ("softmax_max_over_255_partials", "softmax_pitch_columns_written", "layernorm_one_pass_variance", "layernorm_eps_outside_the_root",
             "layernorm_image_g_t_swapped", "layernorm_image_block_of_15_rows", "conv_stem_bias_after_activation", "im2col_tap_order_swapped",
             "maxpool_padding_is_zero", "add_rows_no_wrap", "embed_rows_position_ignored", "attend1_key_64c_read_as_64c_minus_1", "attend1_tk_minus_1_keys",
             "attend1_chunk_c_from_the_slot_of_c_minus_3", "attend1_tail_row_enters_the_chain", "attend1_wrong_scale", "attend1_head_offset_h_64",
             "attend1_image_block_of_15_rows")


def depth(n):
    return -(-n // 256) + 8


def gather_im2col(x, B, H, W, C, ldx, k, stride, pad, mut=()):
    """col[b Ho Wo + oy Wo + ox][(ky k + kx) C + c] = x[b][oy stride + ky - pad][ox stride + kx - pad][c], 0 outside"""
    x = np.asarray(x, np.float32).reshape(-1)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    img = np.zeros((B, H + 2 * pad, W + 2 * pad, C), np.float32)
    pix = np.lib.stride_tricks.as_strided(x, (B, H, W, C), (H * W * ldx * 4, W * ldx * 4, ldx * 4, 4))
    img[:, pad:pad + H, pad:pad + W] = pix
    col = np.zeros((B, Ho, Wo, k, k, C), np.float32)
    for ky in range(k):
        for kx in range(k):
            v = img[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride]
            if "im2col_tap_order_swapped" in mut:
                col[:, :, :, kx, ky] = v
            else:
                col[:, :, :, ky, kx] = v
    return col.reshape(B * Ho * Wo, k * k * C)


def image_index(rows, D, mut=()):
    """float index of element (row, k) in the tiled GEMM's operand image: k = 16 j + 4 t + g at [row / 16][j][g][row % 16][t]"""
    r, k = np.meshgrid(np.arange(rows), np.arange(D), indexing="ij")
    j, t, g = k >> 4, (k & 15) >> 2, k & 3
    if "layernorm_image_g_t_swapped" in mut:
        t, g = g, t
    blk = 15 if "layernorm_image_block_of_15_rows" in mut else 16
    return ((((r // blk) * (D // 16) + j) * 4 + g) * 16 + r % blk) * 4 + t


def layernorm64(x, w, b, eps, mut=()):
    """y = ((x - mean) * rstd) * w + b per row, float64, with the bound of the kernel's float32 evaluation"""
    x, w, b = (np.asarray(v, np.float32).astype(np.float64) for v in (x, w, b))
    D = x.shape[1]
    h = depth(D) * U
    mean = x.sum(axis=1, keepdims=True) / D
    mean_err = h * np.abs(x).sum(axis=1, keepdims=True) / D + np.abs(mean) * U
    d = x - mean
    d_err = mean_err + np.abs(d) * U
    var = (d * d).sum(axis=1, keepdims=True) / D
    if "layernorm_one_pass_variance" in mut:
        x32, m32 = x.astype(np.float32), mean.astype(np.float32)            # float32, as a kernel would: E[x^2] - mean^2 cancels
        var = np.maximum(((x32 * x32).sum(axis=1, keepdims=True, dtype=np.float32) / np.float32(D) - m32 * m32).astype(np.float64), 0.0)
    var_err = (2 * np.abs(d) * d_err).sum(axis=1, keepdims=True) / D + (h + 2 * U) * (d * d).sum(axis=1, keepdims=True) / D + var * U
    root = np.sqrt(var + eps)
    rstd = 1.0 / (np.sqrt(var) + eps) if "layernorm_eps_outside_the_root" in mut else 1.0 / root
    rstd_rel = 0.5 * (var_err + (var + eps) * U) / (var + eps) + SQRT_REL + U
    v = d * rstd
    v_err = d_err * rstd + np.abs(v) * (rstd_rel + U)
    y = v * w + b
    y_err = v_err * np.abs(w) + np.abs(v * w) * U + np.abs(y) * U
    return y, y_err * SLACK


def softmax64(x, mut=()):
    """softmax over axis 1, float64, with the bound of the kernels' float32 evaluation (all three kernels: the same operations in the same order)"""
    x = np.asarray(x, np.float32).astype(np.float64)
    n = x.shape[1]
    xm = x
    if "softmax_max_over_255_partials" in mut:
        xm = np.where(np.arange(n) % 256 == 255, -np.inf, x)
    m = xm.max(axis=1, keepdims=True)
    d = x - m
    e = np.exp(d)
    e_rel = EXPF_REL + np.abs(d) * U
    e = np.where(d < -87.0, 0.0, e)                                        # tk_expf returns 0 below -87
    tot = e.sum(axis=1, keepdims=True)
    tot_rel = (e * e_rel).sum(axis=1, keepdims=True) / tot + depth(n) * U
    p = e / tot
    # an entry whose exponent is within rounding of -87 may be flushed or not: its own size is its bound
    edge = np.abs(d + 87.0) <= 87.0 * U
    return p, np.where(edge, np.exp(-86.9) / tot, p * (e_rel + tot_rel + U)) * SLACK


def conv_stem64(x, B, H, W, ldx, w, bias, act, stride, pad, mut=()):
    """3x3 convolution of a 3-channel image into 16 channels: acc = fma chain over k = (ky 3 + kx) 3 + c from +0, padding taps as a = 0, then + bias, SiLU"""
    col = gather_im2col(x, B, H, W, 3, ldx, 3, stride, pad).astype(np.float64)
    wm = np.asarray(w, np.float32).astype(np.float64).reshape(16, 27)
    acc = col @ wm.T
    acc_err = 27 * U * (np.abs(col) @ np.abs(wm).T)
    bv = np.zeros(16) if bias is None else np.asarray(bias, np.float32).astype(np.float64)
    late = "conv_stem_bias_after_activation" in mut
    v = acc if late else acc + bv
    v_err = acc_err + np.abs(v) * U
    if act:
        sig = 1.0 / (1.0 + np.exp(-v))
        y = v * sig
        # d silu / dv lies in [-0.1, 1.1]; sigmoid = 1 / (1 + tk_expf(-v)): 2^-22 + two roundings; then the product
        y_err = 1.1 * v_err + np.abs(y) * (EXPF_REL + 3 * U)
    else:
        y, y_err = v, v_err
    if late:
        y = y + bv
    return y, y_err * SLACK


def attend1_64(q, k, v, B, Tk, q_bstride, kv_bstride, d, nh, mut=()):
    """k_attend1's comment, float64: per (sequence, head) score_t = (fma chain of q . k_t over the head dimension) * scale + 0, scale = 1 / sqrt(hd);
    softmax as k_softmax_rows; out_j = one fma chain of p_t v_tj over the keys in ascending order.  -> (out [B][d], bound [B][d])"""
    q, k, v = (np.asarray(x, np.float32).reshape(-1).astype(np.float64) for x in (q, k, v))
    hd = d // nh
    scale = 1.0 / np.sqrt(64.0 if "attend1_wrong_scale" in mut else float(hd))
    out, bound = np.zeros((B, d)), np.zeros((B, d))
    for b in range(B):
        K = k[b * kv_bstride:b * kv_bstride + Tk * d].reshape(Tk, d)
        V = v[b * kv_bstride:b * kv_bstride + Tk * d].reshape(Tk, d)
        for h in range(nh):
            c0 = (h * 64) % d if "attend1_head_offset_h_64" in mut else h * hd
            cols = (c0 + np.arange(hd)) % d
            qh, Kh, Vh = q[b * q_bstride + cols], K[:, cols], V[:, cols].copy()
            n = Tk - 1 if "attend1_tk_minus_1_keys" in mut and Tk > 1 else Tk
            if "attend1_key_64c_read_as_64c_minus_1" in mut:
                Vh[64::64] = Vh[63:Tk - 1:64]
            if "attend1_chunk_c_from_the_slot_of_c_minus_3" in mut and Tk > 192:
                Vh[192:] = Vh[:Tk - 192]
            s = (Kh[:n] @ qh) * scale
            # the chain: hd fmas; scale = tk_divf(1, tk_sqrtf(hd)) (<= 1 ulp + one division), the product, + 0.0f is exact
            s_err = hd * U * (np.abs(Kh[:n]) @ np.abs(qh)) * scale + np.abs(s) * (SQRT_REL + 2 * U)
            dlt = s - s.max()
            zero = dlt < -87.0
            e = np.where(zero, 0.0, np.exp(np.where(zero, 0.0, dlt)))
            e_rel = EXPF_REL + np.abs(dlt) * U + s_err + s_err[np.argmax(s)]
            tot = e.sum()
            tot_rel = (e * e_rel).sum() / tot + depth(n) * U
            p = e / tot
            p_err = np.where(np.abs(dlt + 87.0) <= 87.0 * U + s_err + s_err[np.argmax(s)], np.exp(-86.9) / tot, p * (e_rel + tot_rel + U))
            terms = np.abs(p)[:, None] * np.abs(Vh[:n])
            o = p @ Vh[:n]
            o_err = p_err @ np.abs(Vh[:n]) + n * U * terms.sum(axis=0)
            if "attend1_tail_row_enters_the_chain" in mut and Tk % 64:
                o = o + p[n - 1] * Vh[n - 1]
            out[b, h * hd:(h + 1) * hd], bound[b, h * hd:(h + 1) * hd] = o, o_err * SLACK
    return out, bound


def expected(l, mut=()):
    """the whole y (and img) a launch must leave behind -> (y, y_bound or None, img or None, img_bound or None); y / img float64 when bounded"""
    g, op = l["geometry"], l["op"]
    y0 = np.asarray(l["y"], np.float32).reshape(-1)
    exact = op not in ("layernorm", "softmax_rows", "conv_stem", "attend1")
    y = y0.copy() if exact else y0.astype(np.float64)
    bound = None if exact else np.zeros(y.size)
    img = img_bound = None

    def rows_view(arr, rows, ld, cols):
        return np.lib.stride_tricks.as_strided(arr, (rows, cols), (ld * arr.itemsize, arr.itemsize))
    if op == "im2col":
        col = gather_im2col(l["a"], g["B"], g["H"], g["W"], g["C"], g["ldx"], g["k"], g["stride"], g["pad"], mut)
        y[:col.size] = col.reshape(-1)
    elif op == "im2col1d":
        col = gather_im2col(l["a"], g["B"], g["H"], 1, g["C"], g["ldx"], 1, 1, 0)          # [B T][C] rows
        T, k, s, pad, C = g["H"], g["k"], g["stride"], g["pad"], g["C"]
        To = (T + 2 * pad - k) // s + 1
        seq = np.zeros((g["B"], T + 2 * pad, C), np.float32)
        seq[:, pad:pad + T] = col.reshape(g["B"], T, C)
        out = np.stack([seq[:, kx:kx + s * (To - 1) + 1:s] for kx in range(k)], axis=2)     # [B][To][k][C]
        y[:out.size] = out.reshape(-1)
    elif op in ("maxpool5", "upsample2x", "copy_cols"):
        if op == "copy_cols":
            src = rows_view(np.asarray(l["a"], np.float32).reshape(-1), g["rows"], g["ldx"], g["C"])
            rows_view(y, g["rows"], g["ldy"], g["C"])[:] = src
        else:
            B, H, W, C = g["B"], g["H"], g["W"], g["C"]
            src = rows_view(np.asarray(l["a"], np.float32).reshape(-1), B * H * W, g["ldx"], C).reshape(B, H, W, C)
            if op == "upsample2x":
                out = src.repeat(2, axis=1).repeat(2, axis=2)
            else:
                pad_value = 0.0 if "maxpool_padding_is_zero" in mut else -np.inf
                p = np.full((B, H + 4, W + 4, C), pad_value, np.float32)
                p[:, 2:2 + H, 2:2 + W] = src
                out = np.max(np.stack([p[:, dy:dy + H, dx:dx + W] for dy in range(5) for dx in range(5)]), axis=0)
            rows_view(y, out.shape[0] * out.shape[1] * out.shape[2], g["ldy"], C)[:] = out.reshape(-1, C)
    elif op == "add_rows":
        rows, D, n_add = g["rows"], g["C"], g["add_rows"]
        add = np.asarray(l["a"], np.float32).reshape(-1)[:n_add * D].reshape(n_add, D)
        pick = np.arange(rows) % n_add if "add_rows_no_wrap" not in mut else np.minimum(np.arange(rows), n_add - 1)
        y[:rows * D] = (y0[:rows * D].reshape(rows, D) + add[pick]).reshape(-1)
    elif op == "embed_rows":
        D = g["C"]
        table, pos = np.asarray(l["a"], np.float32).reshape(-1, D), np.asarray(l["b"], np.float32).reshape(-1, D)
        p = pos[np.asarray(l["pos_idx"])] if "embed_rows_position_ignored" not in mut else pos[np.zeros(len(l["idx"]), np.int64)]
        y[:len(l["idx"]) * D] = (table[np.asarray(l["idx"])] + p).reshape(-1)
    elif op == "layernorm":
        rows, D = g["rows"], g["C"]
        v, e = layernorm64(np.asarray(l["a"], np.float32).reshape(-1)[:rows * D].reshape(rows, D), l["b"], l["c"], g["eps"], mut)
        y[:rows * D], bound[:rows * D] = v.reshape(-1), e.reshape(-1)
        if l["img"] is not None:
            img = np.asarray(l["img"], np.float32).reshape(-1).astype(np.float64)
            img_bound = np.zeros(img.size)
            at = image_index(rows, D, mut) % img.size                       # (a mutant's index may leave the image; the kernel's never does)
            img[at], img_bound[at] = v, e
    elif op == "softmax_rows":
        rows, cols, ld = g["rows"], g["C"], g["ldy"]
        v, e = softmax64(rows_view(y0, rows, ld, cols), mut)
        rows_view(y, rows, ld, cols)[:] = v
        rows_view(bound, rows, ld, cols)[:] = e
        if "softmax_pitch_columns_written" in mut and ld > cols:
            rows_view(y, rows - 1, ld, ld)[:, cols:] = 0.0
    elif op == "conv_stem":
        v, e = conv_stem64(l["a"], g["B"], g["H"], g["W"], g["ldx"], l["b"], l["c"], g["act"], g["stride"], g["pad"], mut)
        rows_view(y, v.shape[0], g["ldy"], 16)[:] = v
        rows_view(bound, v.shape[0], g["ldy"], 16)[:] = e
    elif op == "attend1":
        B, d, qs = g["B"], g["C"], g["q_bstride"]
        v, e = attend1_64(l["a"], l["b"], l["c"], B, g["H"], qs, g["kv_bstride"], d, g["N"], mut)
        rows_view(y, B, qs, d)[:] = v
        rows_view(bound, B, qs, d)[:] = e
        if l["img"] is not None:
            img = np.asarray(l["img"], np.float32).reshape(-1).astype(np.float64)
            img_bound = np.zeros(img.size)
            at = image_index(B, d, ("layernorm_image_block_of_15_rows",) if "attend1_image_block_of_15_rows" in mut else ()) % img.size
            img[at], img_bound[at] = v, e
    else:
        raise ValueError(op)
    return y, bound, img, img_bound


def compare(got, want, bound):
    """-> worst error / bound over the entries with a bound; entries without one must be equal (bit for bit, NaN-free)"""
    got = np.asarray(got).reshape(-1)
    if bound is None:
        assert np.array_equal(got, want), "a gather / single add is exact"
        return 0.0
    free = bound > 0
    assert np.array_equal(got[~free].astype(np.float64), want[~free]), "an entry the kernel must not touch, or an exact one, differs"
    err = np.abs(got[free].astype(np.float64) - want[free])
    assert np.all(err <= bound[free]), ("outside the bound", float(np.max(err / bound[free])))
    return float(np.max(err / bound[free], initial=0.0))
