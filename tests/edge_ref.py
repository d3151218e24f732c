"""Reference B of the kernels at the two ends of the perception streams (k_frames, k_power, k_logmel_finish, k_vad_head, k_preprocess,
k_preprocess_scaled, k_depth_minmax, k_depth_metric, k_postprocess_depth, k_depth_to_points, k_box_attributes): NumPy written from the kernels'
comments and the reference's documented formulas.  It never imports the oracle.

expected(case, mut) -> {array name: (values, bound)}: the WHOLE in/out arrays a launch of tests/edge_cases.py must leave behind, what the kernel writes
and the caller's sentinel everywhere else (bound 0 there).  A bound of None means exact:
  frames             a division by 2^15 and ONE product: the float64 product of two float32 values is exact, so its rounding is the kernel's
  power              fma(re, re, round(im im)): the exact sum by TwoSum, rounded once (a float64 sum rounded again would round twice at a tie)
  depth min / max    a sequential scan
  depth_to_points    the branch d > 0 and z; x and y inside 3 roundings
  box_attributes     every output is an integer: the float32 / float64 operation order of the kernel's comment, evaluated with NumPy's IEEE operations
Everything else is float64 inside a bound built term by term, in the running-error form of tests/split_f16_ref.py, from the documented order:
  U = 2^-24          one correctly rounded float32 operation, relative
  tk_expf            relative error <= 2^-22 (csrc/common/tk_exact_math.h); its argument is clamped to 88 and it returns 0 below -87
  tk_log10f          documents no bound: tests/test_perception_edges_cpu.py measures the host build against float64 log10 over every argument the
                     cases send and over a dense sweep of [1e-10, 1e6], and asserts LOG10_ABS is twice the worst absolute error.
                     Measured: 1.1245e-06 at 1.3985307e-10 (|log10| close to 10, where half an ulp is 4.8e-7), so LOG10_ABS = 2.25e-06.
The bilinear stretch is continuous in its sampling coordinate (slope at most 255 per pixel), so the truncation (int)gx needs no abstention: the bound
carries the coordinate's two roundings through that slope.  No element of any case abstains.

MUTATIONS: one plausible kernel error each; tests/test_perception_edges_cpu.py shows that each changes what at least one GPU case leaves behind."""
import numpy as np

U = 2.0 ** -24
EXPF_REL = 2.0 ** -22
LOG10_ABS = 2.25e-06
SLACK = 1.01
NFFT, HOP = 400, 160
F32, F64 = np.float32, np.float64

MUTATIONS = ("frames_right_reflect_2n_minus_j", "frames_left_reflect_minus_j_minus_1", "frames_j_le_n_samples", "frames_divide_by_32767", "frames_window_by_frame",
             "frames_batch_offset_dropped", "power_im_at_pitch_nb", "logmel_max_over_first_1024", "logmel_one_max_for_the_batch", "logmel_floor_max_minus_80",
             "logmel_clamp_before_log", "vad_no_relu", "vad_b2_dropped", "preprocess_ratio_in_over_out", "preprocess_stride_ignored", "preprocess_bgra",
             "preprocess_layout_swapped", "preprocess_mean_after_std", "preprocess_scaled_ignores_scale", "depth_first_stride_only", "depth_min_max_exchanged",
             "depth_threshold_1e_5", "points_u_is_i_over_width", "points_cx_cy_exchanged", "points_d_ge_0", "points_second_trip_skipped", "box_border_in_edge_count",
             "box_tie_to_last_bin", "box_out_of_frame_counted", "box_density_over_in_frame", "box_luma_ge_100", "box_hue_le_30")


def hann():
    """periodic Hann window, rounded once to float32"""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NFFT) / NFFT)).astype(F32)


def frames(c, mut):
    B, ns, stride, nt, T = c["B"], c["n_samples"], c["pcm_stride"], c["n_total"], c["T"]
    pcm, w = c["a"].astype(F64), c["b"].astype(F64)
    out = c["y"].astype(F64).copy()
    for b in range(B):
        row = pcm[(0 if "frames_batch_offset_dropped" in mut else b) * stride:][:ns]
        x = np.zeros(nt)
        keep = min(ns + 1, nt) if "frames_j_le_n_samples" in mut else ns
        x[:len(row)] = row
        if keep > ns:
            x[ns] = pcm[b * stride + ns] if b * stride + ns < len(pcm) else 0.0
        x = x / (32767.0 if "frames_divide_by_32767" in mut else 32768.0)
        pad = np.pad(x, NFFT // 2, mode="reflect")                          # pad[i] = x at sample i - 200
        if "frames_right_reflect_2n_minus_j" in mut:
            j = np.arange(nt, nt + NFFT // 2)
            pad[NFFT // 2 + nt:] = x[np.clip(2 * nt - j, 0, nt - 1)]
        if "frames_left_reflect_minus_j_minus_1" in mut:
            j = np.arange(-(NFFT // 2), 0)
            pad[:NFFT // 2] = x[-j - 1]
        for t in range(T):
            win = w[np.full(NFFT, t % NFFT)] if "frames_window_by_frame" in mut else w
            seg = pad[t * HOP:t * HOP + NFFT]
            out[(b * T + t) * NFFT:(b * T + t + 1) * NFFT] = (seg * win).astype(F32)
    return {"y": (out.astype(F32), None)}


def round_sum_once(s, t):
    """float32(s + t) for float64 s, t whose exact sum needs more than 53 bits: TwoSum, then the float64 sum's rounding to float32 is corrected where
    it sat exactly on a float32 tie and the discarded part decides"""
    hi = s + t
    bb = hi - s
    lo = (s - (hi - bb)) + (t - bb)
    r = hi.astype(F32)
    r64 = r.astype(F64)
    with np.errstate(over="ignore"):
        other = np.nextafter(r, np.where(hi > r64, np.inf, -np.inf).astype(F32)).astype(F64)
    tie = (lo != 0) & (hi != r64) & ((hi - r64) == (other - hi))
    flip = tie & (np.sign(lo) == np.sign(hi - r64))
    return np.where(flip, other.astype(F32), r)


def power(c, mut):
    rows, nb = c["rows"], c["nb"]
    ri = c["a"].astype(F64)
    out = c["y"].copy()
    r = np.arange(rows)[:, None]
    f = np.arange(nb)[None, :]
    re = ri[r * 2 * nb + f]
    im = ri[r * 2 * nb + nb + f]
    if "power_im_at_pitch_nb" in mut:                                       # the imaginary half looked for one row pitch of nb further, not 2 nb
        im = ri[np.minimum(r * nb + nb + f, len(ri) - 1)]
    t = (im * im).astype(F32).astype(F64)
    out[:rows * nb] = round_sum_once(re * re, t).reshape(-1)
    return {"y": (out, None)}


def logmel(c, mut):
    B, per = c["B"], c["per_b"]
    x = c["y"].astype(F64)
    out, bound = x.copy(), np.zeros(len(x))
    m = x[:B * per].reshape(B, per)
    floor_arg = float(F32(1e-10))
    if "logmel_clamp_before_log" in mut:                                    # the clamp at max - 8 applied to the power, not to its logarithm
        m = np.maximum(m, m.max(axis=1, keepdims=True) - 8.0)
    v = np.log10(np.maximum(m, floor_arg))
    mx = v[:, :1024].max(axis=1, keepdims=True) if "logmel_max_over_first_1024" in mut else v.max(axis=1, keepdims=True)
    if "logmel_one_max_for_the_batch" in mut:
        mx = np.full_like(mx, v.max())
    fl = mx - (80.0 if "logmel_floor_max_minus_80" in mut else 8.0)
    fl_err = LOG10_ABS + np.abs(fl) * U
    cl = np.maximum(v, fl)
    cl_err = np.maximum(LOG10_ABS, fl_err) + 0 * cl
    y = (cl + 4.0) * 0.25
    out[:B * per] = y.reshape(-1)
    bound[:B * per] = ((cl_err + np.abs(cl + 4.0) * U) * 0.25 * SLACK).reshape(-1)
    return {"y": (out, bound)}


def vad(c, mut):
    n, hidden = c["rows"], c["hidden"]
    hid, w2, b2 = c["a"].astype(F64).reshape(n, hidden), c["b"].astype(F64), float(c["c"][0])
    out, bound = c["y"].astype(F64).copy(), np.zeros(len(c["y"]))
    act = hid if "vad_no_relu" in mut else np.maximum(hid, 0.0)
    terms = act * w2[None, :]
    acc = terms.sum(axis=1)
    acc_err = hidden * U * np.abs(terms).sum(axis=1)
    z = acc + (0.0 if "vad_b2_dropped" in mut else b2)
    z_err = acc_err + np.abs(z) * U
    arg = np.minimum(-z, 88.0)                                              # tk_expf clamps its argument at 88 ...
    e = np.where(arg < -87.0, 0.0, np.exp(arg))                             # ... and returns 0 below -87
    p = 1.0 / (1.0 + e)
    # dp/dz = p (1 - p); exp's relative error enters through e / (1 + e) = 1 - p; 1 + e and the division round once each; results this small
    # (p = 1 / (1 + exp(88)) = 6e-39) are subnormal: half a unit of 2^-149 more.  An argument within z_err of a clamp may fall on either side.
    p_err = p * (1.0 - p) * z_err + p * ((1.0 - p) * EXPF_REL + 2 * U) + 2.0 ** -149
    near = (np.abs(arg + 87.0) <= z_err) | ((np.abs(-z - 88.0) <= z_err) & (-z > 80.0))
    p_err = np.where(near, p_err + np.exp(-87.0), p_err)
    out[:n], bound[:n] = p, p_err * SLACK
    return {"y": (out, bound)}


def preprocess(c, mut):
    iw, ih, stride, bpp, ow, oh, nhwc = (c[k] for k in ("in_w", "in_h", "in_stride", "bpp", "out_w", "out_h", "nhwc"))
    mean, std, scale = np.asarray(c["mean"], F32).astype(F64), np.asarray(c["std_dev"], F32).astype(F64), float(F32(c["scale"]))
    canonical = scale == float(F32(1.0) / F32(255.0)) or scale == 0.0
    if "preprocess_stride_ignored" in mut:
        stride = iw * bpp
    src = c["a"].astype(F64)
    pix = np.zeros((ih, iw, 3))
    for ch in range(3):
        cc = 2 - ch if "preprocess_bgra" in mut else ch
        idx = np.arange(ih)[:, None] * stride + np.arange(iw)[None, :] * bpp + cc
        pix[:, :, ch] = src[np.minimum(idx, len(src) - 1)]
    less = 0.0 if "preprocess_ratio_in_over_out" in mut else 1.0
    gx, gy = (iw - less) / ow * np.arange(ow), (ih - less) / oh * np.arange(oh)
    x0, y0 = np.minimum(np.floor(gx).astype(int), iw - 1), np.minimum(np.floor(gy).astype(int), ih - 1)
    x1, y1 = np.minimum(x0 + 1, iw - 1), np.minimum(y0 + 1, ih - 1)
    dx, dy = (gx - x0)[None, :, None], (gy - y0)[:, None, None]
    v = (pix[y0][:, x0] * (1 - dx) + pix[y0][:, x1] * dx) * (1 - dy) + (pix[y1][:, x0] * (1 - dx) + pix[y1][:, x1] * dx) * dy
    # the coordinate is ratio * o after two roundings; the stretch's slope is at most 255 per pixel in either axis; the four products and three sums
    v_err = 255.0 * 2 * U * (gx[None, :, None] + gy[:, None, None]) + 16 * U * 255.0
    if canonical or "preprocess_scaled_ignores_scale" in mut:
        s, s_err = v / 255.0, v_err / 255.0 + np.abs(v / 255.0) * U
    else:
        s, s_err = v * scale, v_err * abs(scale) + np.abs(v * scale) * U
    if "preprocess_mean_after_std" in mut:
        o = s / std - mean
    else:
        o = (s - mean) / std
    o_err = (s_err + np.abs(s - mean) * U) / np.abs(std) + np.abs(o) * U
    if bool(nhwc) != ("preprocess_layout_swapped" in mut):
        o, o_err = o.reshape(-1), o_err.reshape(-1)
    else:
        o, o_err = o.transpose(2, 0, 1).reshape(-1), o_err.transpose(2, 0, 1).reshape(-1)
    out, bound = c["y"].astype(F64).copy(), np.zeros(len(c["y"]))
    out[:3 * ow * oh], bound[:3 * ow * oh] = o, o_err * SLACK
    return {"y": (out, bound)}


def minmax_seq(x, mut):
    if "depth_first_stride_only" in mut:
        x = x[:1024]
    lo = hi = x[0]
    for v in x[1:]:
        if v < lo:
            lo = v
        if v > hi:
            hi = v
    return lo, hi


def depth_minmax(c, mut):
    lo, hi = minmax_seq(c["a"], mut)
    out = c["y"].copy()
    out[:2] = (lo, hi)
    # min and max are order-independent except for the sign of a zero that occurs with both signs: compared as values (bound None), not by sign
    return {"y": (out, None)}


def depth_metric(c, mut):
    n, x = c["n"], c["a"].astype(F64)
    lo, hi = (float(v) for v in minmax_seq(c["a"], mut))
    mn, mxd = float(F32(c["min_depth"])), float(F32(c["max_depth"]))
    out, bound = c["y"].astype(F64).copy(), np.zeros(len(c["y"]))
    rng = float(F32(hi - lo))
    thr = float(F32(1e-5)) if "depth_threshold_1e_5" in mut else float(F32(1e-6))
    if rng < thr:
        out[:n] = mxd
    else:
        if "depth_min_max_exchanged" in mut:
            lo, hi = hi, lo
            rng = hi - lo
        d = x - lo
        q = d / rng
        q_err = np.abs(q) * 3 * U                                          # x - lo, the range, the division
        span = mxd - mn
        t = q * span
        t_err = q_err * abs(span) + np.abs(t) * 2 * U                      # the span's rounding and the product's
        y = mxd - t
        out[:n], bound[:n] = y, (t_err + np.abs(y) * U) * SLACK
    mm = c["y2"].copy()
    mm[:2] = minmax_seq(c["a"], mut)
    return {"y": (out, bound), "y2": (mm, None)}


def postprocess_depth(c, mut):
    n = c["width"] * c["height"]
    raw, scale, shift = c["a"].astype(F64), float(F32(c["scale"])), float(F32(c["shift"]))
    out, bound = c["y"].astype(F64).copy(), np.zeros(len(c["y"]))
    y = raw * scale + shift
    out[:n], bound[:n] = y, (np.abs(raw * scale) * U + np.abs(y) * U + 2.0 ** -149) * SLACK
    return {"y": (out, bound)}


def depth_to_points(c, mut, cap_threads):
    w, h = c["width"], c["height"]
    n = w * h
    d = c["a"].astype(F64)
    fx, fy, cx, cy = (float(F32(c[k])) for k in ("fx", "fy", "cx", "cy"))
    if "points_cx_cy_exchanged" in mut:
        cx, cy = cy, cx
    i = np.arange(n)
    u, v = i % w, i // w
    if "points_u_is_i_over_width" in mut:
        u, v = v, u
    on = d >= 0 if "points_d_ge_0" in mut else d > 0
    x, y = (u - cx) * d / fx, (v - cy) * d / fy
    pts = np.where(on[:, None], np.stack([x, y, d], axis=1), 0.0)
    err = np.where(on[:, None], np.stack([np.abs(x) * 3 * U + 2.0 ** -149, np.abs(y) * 3 * U + 2.0 ** -149, 0 * d], axis=1) * SLACK, 0.0)
    out, bound = c["y"].astype(F64).copy(), np.zeros(len(c["y"]))
    out[:3 * n], bound[:3 * n] = pts.reshape(-1), err.reshape(-1)
    if "points_second_trip_skipped" in mut:                                 # elements past the first trip of the grid-stride loop keep the caller's content
        keep = (np.repeat(i, 3) >= cap_threads) & (np.repeat(i, 3) < 2 * cap_threads)
        out[:3 * n] = np.where(keep, c["y"].astype(F64)[:3 * n], out[:3 * n])
    return {"y": (out, bound)}


def color_bins(rgb, mut=()):
    """bin of every pixel of a uint8 [..., 3] array, in the kernel comment's operation order: float32 except where the reference's double constants
    promote (2 + ., 4 + ., * 60, + 360 and every comparison with 0.1 / 0.9 / 0)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        c = (rgb.astype(F32) / F32(255.0)).astype(F32)
        r, g, b = c[..., 0], c[..., 1], c[..., 2]
        mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
        delta = (mx - mn).astype(F32)
        s = np.where(mx > 0, (delta / mx).astype(F32), F32(0))
        hr = ((g - b).astype(F32) / delta).astype(F32)
        hg = (2.0 + ((b - r).astype(F32) / delta).astype(F32).astype(F64)).astype(F32)
        hb = (4.0 + ((r - g).astype(F32) / delta).astype(F32).astype(F64)).astype(F32)
        h = np.where(r >= mx, hr, np.where(g >= mx, hg, hb))
        h = (h.astype(F64) * 60.0).astype(F32)
        h = np.where(h.astype(F64) < 0.0, (h.astype(F64) + 360.0).astype(F32), h)
        h = np.where(mx > 0, h, F32(0))
    gray = s.astype(F64) < 0.1
    v = mx.astype(F64)
    out = np.full(h.shape, -1, np.int32)
    first = h <= F32(30) if "box_hue_le_30" in mut else h < F32(30)
    for lim, k in ((330, 5), (270, 4), (210, 3), (150, 2), (90, 1)):
        out = np.where(h < F32(lim), k, out)
    out = np.where(first | (h >= F32(330)), 0, out)
    return np.where(gray, np.where(v < 0.1, 6, np.where(v > 0.9, 7, 8)), out).astype(np.int32)


def box_attributes(c, mut):
    W, H, n = c["in_w"], c["in_h"], c["rows"]
    frame = c["a"].reshape(H, W, 3)
    bins = color_bins(frame, mut)
    f = frame.astype(np.int64)
    luma = ((f[..., 0] * 299 + f[..., 1] * 587 + f[..., 2] * 114) // 1000) & 255
    strong = np.zeros((H, W), bool)
    diff = np.abs(luma[:-2] - luma[2:])
    strong[1:-1] = diff >= 100 if "box_luma_ge_100" in mut else diff > 100
    out = c["y"].copy()
    rects = c["b"].reshape(n, 4)
    for k in range(n):
        bx, by, bw, bh = (int(t) for t in rects[k])
        x0, x1, y0, y1 = max(bx, 0), min(bx + bw, W), max(by, 0), min(by + bh, H)
        counts = np.zeros(9, np.int64)
        edges = 0
        if x1 > x0 and y1 > y0:
            sub = bins[y0:y1, x0:x1]
            counts = np.bincount(sub[sub >= 0], minlength=9)
            if "box_out_of_frame_counted" in mut:                           # pixels outside the frame read as the clamped edge pixel
                ys, xs = np.clip(np.arange(by, by + bh), 0, H - 1), np.clip(np.arange(bx, bx + bw), 0, W - 1)
                sub = bins[ys][:, xs]
                counts = np.bincount(sub[sub >= 0], minlength=9)
            inner = 0 if "box_border_in_edge_count" in mut else 1
            ex0, ex1, ey0, ey1 = max(bx + inner, 0), min(bx + bw - inner, W), max(by + inner, 1), min(by + bh - inner, H - 1)
            if ex1 > ex0 and ey1 > ey0:
                edges = int(strong[ey0:ey1, ex0:ex1].sum())
        top = counts.max()
        out[2 * k] = int(np.flatnonzero(counts == top)[-1 if "box_tie_to_last_bin" in mut else 0])
        area = (x1 - x0) * (y1 - y0) if "box_density_over_in_frame" in mut else bw * bh
        with np.errstate(divide="ignore", invalid="ignore"):
            density = F32(edges) / F32(area)
        out[2 * k + 1] = 1 if float(density) > 0.1 else 0
    return {"y": (out, None)}


def expected(c, mut=(), cap_threads=2048 * 256):
    op = c["op"]
    if op == "depth_to_points":
        return depth_to_points(c, mut, cap_threads)
    return {"frames": frames, "power": power, "logmel_finish": logmel, "vad_head": vad, "preprocess": preprocess, "depth_minmax": depth_minmax,
            "depth_metric": depth_metric, "postprocess_depth": postprocess_depth, "box_attributes": box_attributes}[op](c, mut)


def compare(got, want, bound):
    """worst |got - want| / bound over the elements with a bound > 0; elements of bound 0 (and every element when bound is None) must be equal as values,
    NaN matching NaN (with a bound of 0 the sign of a zero counts too; with None it does not).  Raises AssertionError with the first offender."""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    if bound is None:
        bad = np.flatnonzero(~((got == want) | (np.isnan(got.astype(F64)) & np.isnan(want.astype(F64)))))
        assert bad.size == 0, "element %d: %r, exact answer %r (%d differ)" % (bad[0], got[bad[0]], want[bad[0]], bad.size)
        return 0.0
    g, w = got.astype(F64), want.astype(F64)
    exact = bound == 0
    bad = np.flatnonzero(exact & ~(((g == w) & (np.signbit(g) == np.signbit(w))) | (np.isnan(g) & np.isnan(w))))   # a bound of 0: the sign of a zero too
    assert bad.size == 0, "element %d: %r where %r must stand (%d differ)" % (bad[0], got[bad[0]], want[bad[0]], bad.size)
    if exact.all():
        return 0.0
    with np.errstate(invalid="ignore"):
        ratio = np.where(exact, 0.0, np.abs(g - w) / np.where(exact, 1.0, bound))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    worst = int(np.argmax(ratio))
    assert ratio[worst] <= 1.0, "element %d: %r, float64 %r, error %.3g = %.2f bounds" % (worst, got[worst], want[worst], abs(g[worst] - w[worst]), ratio[worst])
    return float(ratio[worst])


# ---------------------------------------------------------------- the composed log-mel front end (frames -> DFT -> power -> mel -> finish)
def slaney_filters(n_mels, n_bins=NFFT // 2 + 1, sr=16000.0):
    """Slaney mel scale (linear below 1 kHz at 200/3 Hz per mel, logarithmic above with 27 steps per factor 6.4), triangles between n_mels + 2 points
    equally spaced in mel over 0..sr/2, each normalised to unit area (2 / width in Hz)"""
    def to_mel(f):
        return f / (200.0 / 3.0) if f < 1000.0 else 15.0 + np.log(f / 1000.0) / (np.log(6.4) / 27.0)

    def to_hz(m):
        return m * (200.0 / 3.0) if m < 15.0 else 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0))
    pts = np.array([to_hz(m) for m in np.linspace(to_mel(0.0), to_mel(sr / 2), n_mels + 2)])
    freqs = np.arange(n_bins) * (sr / NFFT)
    w = np.zeros((n_mels, n_bins))
    for i in range(n_mels):
        up, down = (freqs - pts[i]) / (pts[i + 1] - pts[i]), (pts[i + 2] - freqs) / (pts[i + 2] - pts[i + 1])
        w[i] = np.maximum(0.0, np.minimum(up, down)) * 2.0 / (pts[i + 2] - pts[i])
    return w


def logmel_composed(pcm, n_total, T, n_mels):
    """pcm int16 [B][n] -> (log-mel [B][T][n_mels] in float64, bound): an rfft of the reflect-padded, Hann-windowed frames, the Slaney bank, the finish;
    the bound follows the float32 evaluation: the window table and the product (2 U), an NFFT-term chain against rounded cos / sin tables
    ((NFFT + 2) U sum |x w|, whatever the order of the sum), the power's two products and sum, a 201-term chain against the rounded filter table, tk_log10f
    (LOG10_ABS) on an argument known to its own error, the utterance maximum as an interval, the clamp, + 4, / 4"""
    pcm = np.asarray(pcm, np.int16)
    B, n = pcm.shape
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NFFT) / NFFT)
    bank = slaney_filters(n_mels)
    out, bound = np.zeros((B, T, n_mels)), np.zeros((B, T, n_mels))
    tiny = float(F32(1e-10))
    for b in range(B):
        x = np.zeros(n_total)
        x[:n] = pcm[b].astype(F64) / 32768.0
        pad = np.pad(x, NFFT // 2, mode="reflect")
        seg = np.stack([pad[t * HOP:t * HOP + NFFT] for t in range(T)]) * win[None, :]
        s1 = np.abs(seg).sum(axis=1, keepdims=True)
        spec = np.fft.rfft(seg, axis=1)
        d = (NFFT + 4) * U * s1 + 1e-15 * s1                               # re and im alike (the float64 FFT's own error is far below)
        p = spec.real ** 2 + spec.imag ** 2
        dp = 2 * (np.abs(spec.real) + np.abs(spec.imag)) * d + 2 * d * d + 3 * U * p
        m = p @ bank.T
        dm = dp @ bank.T + (NFFT // 2 + 3) * U * m
        v = np.log10(np.maximum(m, tiny))
        v_lo, v_hi = np.log10(np.maximum(m - dm, tiny)) - LOG10_ABS, np.log10(np.maximum(m + dm, tiny)) + LOG10_ABS
        fl, fl_lo, fl_hi = v.max() - 8.0, v_lo.max() - 8.0, v_hi.max() - 8.0
        c, c_lo, c_hi = np.maximum(v, fl), np.maximum(v_lo, fl_lo - 8.0 * U), np.maximum(v_hi, fl_hi + 8.0 * U)
        out[b] = (c + 4.0) * 0.25
        bound[b] = (np.maximum(c_hi - c, c - c_lo) + np.abs(c + 4.0) * U) * 0.25 * SLACK
    return out, bound
