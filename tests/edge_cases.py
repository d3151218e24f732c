"""The launches of tests/test_perception_edges_gpu.py, shared with tests/test_perception_edges_cpu.py: one tk_mi355x_edge_probe call each.

A case is a dict: op, name, the hook's geometry fields, the arrays a / b / c (inputs) and y / y2 (in/out, filled with a sentinel that must come back
wherever the kernel does not write: a few elements past the written region are always there), `kernel` (the launcher's answer) and `hand`: a list of
(array, indices, values) written by hand from the operation's definition, compared exactly.  reference_a(case) is the oracle's own host function on the
same arrays (bit for bit); tests/edge_ref.py is reference B.  Shapes are the smallest at which each kernel can still be wrong."""
import functools

import numpy as np

import edge_ref as R
import oracle_lib as O

F32 = np.float32
SENT = F32(-777.25)       # floats the kernels must not touch
HOSTILE = 12345           # pcm padding between rows: must never be read
GRID_CAP = 2048           # blocks of 256: tk_kernels_postprocess_depth_map / tk_kernels_depth_to_point_cloud (the hook reports it; the CPU test asserts it)
GROUPS = ("frames", "power", "logmel_finish", "vad_head", "preprocess", "depth_minmax", "depth_metric", "postprocess_depth", "depth_to_points", "box_attributes")
MIN_HAND = {"frames": 2000, "power": 20, "logmel_finish": 5000, "vad_head": 100, "preprocess": 60, "depth_minmax": 40, "depth_metric": 3000,
            "postprocess_depth": 8, "depth_to_points": 30, "box_attributes": 2000}
GEOMETRY = ("B", "n_samples", "pcm_stride", "n_total", "T", "rows", "nb", "per_b", "hidden", "in_w", "in_h", "in_stride", "bpp", "out_w", "out_h", "nhwc", "width",
            "height", "n", "mean", "std_dev", "scale", "shift", "min_depth", "max_depth", "fx", "fy", "cx", "cy")


def rng(*key):
    return np.random.default_rng([20260, *key])


def out_array(n, dtype=F32, extra=5):
    return np.full(n + extra, SENT if dtype == F32 else -777, dtype)


def case(op, name, y, a=None, b=None, c=None, y2=None, kernel=0, hand=(), **geometry):
    d = dict(op=op, name="%s %s" % (op, name), a=a, b=b, c=c, y=y, y2=y2, kernel=kernel, hand=list(hand))
    d.update(geometry)
    return d


# ------------------------------------------------------------------------------------------------ FRAMES
def frames_hand(pcm_row, ns, nt, T, window):
    """first and last frame and the zero region of one utterance, from the definition: tap n of frame t reads sample j = 160 t + n - 200 of the clip
    zero-padded to n_total, mirrored about sample 0 (j -> -j) and about sample n_total - 1 (j -> 2 (n_total - 1) - j), / 32768, times window[n]"""
    idx, val = [], []
    for t in sorted({0, T - 1}):
        for n in range(400):
            j = 160 * t + n - 200
            if j < 0:
                j = -j
            if j > nt - 1:
                j = 2 * (nt - 1) - j
            x = F32(pcm_row[j]) / F32(32768.0) if j < ns else F32(0)
            idx.append(t * 400 + n)
            val.append(F32(x) * window[n])
    for t in range(1, T - 1):                                               # frames wholly past the clip: zeros (times the window: +0 or -0 by the sample's sign)
        if 160 * t - 200 >= ns:
            idx.extend(range(t * 400, t * 400 + 400))
            val.extend([F32(0)] * 400)
    return np.array(idx), np.array(val, F32)


@functools.lru_cache(None)
def frames_cases():
    out = []
    ones, hann = np.ones(400, F32), R.hann()
    for nt, T in ((640, 4), (3200, 20)):
        for ns in (1, 199, 200, 201, nt - 1, nt):
            for B in (1, 3):
                stride = ns if B == 1 else ns + 7
                for kind in ("ramp", "extremes", "impulses", "noise"):
                    if kind != "ramp" and not (ns in (201, nt) or (ns == 1 and kind == "impulses")):
                        continue
                    pcm = np.full((B, stride), HOSTILE, np.int16)
                    g = rng(1, nt, ns, B)
                    for b in range(B):
                        if kind == "ramp":                                  # every output names the sample it read (and the row: + 10000 b)
                            pcm[b, :ns] = np.arange(ns) + 10000 * b
                        elif kind == "extremes":
                            pcm[b, :ns] = np.array([32767, -32768, -32767, 1, -1, 0], np.int16)[(np.arange(ns) + b) % 6]
                        elif kind == "impulses":
                            pcm[b, :ns] = 0
                            pcm[b, 0], pcm[b, ns - 1] = 32767 - b, -32768 + b
                        else:
                            pcm[b, :ns] = g.integers(-32768, 32768, ns)
                    for wname, w in (("ones", ones), ("hann", hann)):
                        if wname == "ones" and kind != "ramp":
                            continue
                        y = out_array(B * T * 400)
                        hand = []
                        for b in range(B):
                            i, v = frames_hand(pcm[b], ns, nt, T, w)
                            hand.append(("y", i + b * T * 400, v))
                        out.append(case("frames", "n_total %d T %d n_samples %d B %d %s window %s" % (nt, T, ns, B, kind, wname), y, a=pcm.reshape(-1), b=w,
                                        hand=hand, B=B, n_samples=ns, pcm_stride=stride, n_total=nt, T=T))
    return out


# ------------------------------------------------------------------------------------------------ POWER
@functools.lru_cache(None)
def power_cases():
    out = []
    for rows in (1, 3):
        for nb in (1, 201, 256, 257):
            g = rng(2, rows, nb)
            ri = g.standard_normal((rows, 2, nb)).astype(F32)
            ri[:, 0] *= F32(1e4) if nb % 2 else F32(1e-4)                 # re^2 >> im^2, or the reverse
            hand = []
            if nb >= 201:
                ri[0, 0, :4], ri[0, 1, :4] = [3.0, 0.0, 0.0, -0.0], [4.0, 5.0, 0.0, 2.0]       # 25, 25, 0, 4
                ri[0, 0, 4:8], ri[0, 1, 4:8] = [2.0 ** -70, 2.0 ** -75, 2.0 ** -74, 1e-20], [2.0 ** -70, 2.0 ** -75, 0.0, 2.0 ** -64]
                # 2^-140 + 2^-140 = 2^-139; 2^-150 + 2^-150: im^2 rounds to 0 (tie to even), then re^2 alone rounds to 0; 2^-148; 1e-40 + 2^-128 (subnormal sum)
                hand.append(("y", np.arange(7), np.array([25.0, 25.0, 0.0, 4.0, 2.0 ** -139, 0.0, 2.0 ** -148], F32)))
            if rows == 3:
                ri[1, 0], ri[2, 1] = 0.0, 0.0                               # a row with re = 0, one with im = 0
                hand.append(("y", nb + np.arange(nb), (ri[1, 1].astype(np.float64) ** 2).astype(F32)))
                hand.append(("y", 2 * nb + np.arange(nb), (ri[2, 0].astype(np.float64) ** 2).astype(F32)))
            out.append(case("power", "rows %d nb %d" % (rows, nb), out_array(rows * nb), a=ri.reshape(-1), hand=hand, rows=rows, nb=nb))
    return out


# ------------------------------------------------------------------------------------------------ LOGMEL_FINISH
@functools.lru_cache(None)
def logmel_cases():
    out = []
    for per in (1, 63, 1023, 1024, 1025, 2049, 160 * 80):
        for B in (1, 3):
            spots = sorted({0, per - 1} | {min(per - 1, 64 * w + 17) for w in range(16)} | ({1024 + 5, per - 3} if per > 1030 else set()))
            for kind in ["zero", "spike", "spike clamps"] + ["max at %d" % s for s in (spots if B == 1 else spots[:2])] + ["floor", "loud and quiet"]:
                if kind == "loud and quiet" and B == 1:
                    continue
                g = rng(3, per, B, len(kind), sum(map(ord, kind)))
                mel = (10.0 ** g.uniform(-6, -1, (B, per))).astype(F32)
                hand = []
                if kind == "zero":
                    mel[:] = 0.0
                    if B == 3:
                        mel[1] = 10.0 ** g.uniform(-3, 2, per)
                elif kind in ("spike", "spike clamps"):                     # one element 1e6 above the rest: they stay 6 decades below, unclamped;
                    low = -3.0 if kind == "spike" else -6.0                 # 1e9 (and more) above: everything else sits on max - 8
                    mel[:] = 10.0 ** low
                    for b in range(B):
                        mel[b, (per // 2 + b) % per] = 1e3 * 10.0 ** b
                        if per > 1:
                            rest = np.setdiff1d(np.arange(per), [(per // 2 + b) % per])
                            hand.append(("y~", b * per + rest, np.full(len(rest), (max(low, 3.0 + b - 8.0) + 4.0) / 4.0)))
                        hand.append(("y~", np.array([b * per + (per // 2 + b) % per]), np.array([(3.0 + b + 4.0) / 4.0])))
                elif kind.startswith("max at"):
                    s = int(kind.split()[-1])
                    mel[:, :] = (10.0 ** g.uniform(-12, -9.5, (B, per))).astype(F32)  # around and below the 1e-10 floor
                    mel[:, s] = 100.0
                    rest = np.setdiff1d(np.arange(per), [s])
                    for b in range(B):                                      # max = 2, floor -6: every other element is clamped there -> (-6 + 4) / 4
                        hand.append(("y~", b * per + rest, np.full(len(rest), -0.5)))
                        hand.append(("y~", np.array([b * per + s]), np.array([1.5])))
                elif kind == "floor":                                       # values just on either side of max - 8, and below 1e-10
                    mel[:] = 1.0
                    edge = np.array([1e-8 * (1 + 3e-6), 1e-8 * (1 - 3e-6), 1e-8, 0.99e-10, 1e-10, 1.01e-10, 1e-30, 0.0], F32)
                    mel[:, 1:] = edge[np.arange(per - 1) % len(edge)]
                else:                                                       # very different loudness per row: no maximum may leak into another utterance
                    for b in range(B):
                        mel[b] = (10.0 ** (g.uniform(-3, 0, per) + 4 * b - 6)).astype(F32)
                        mel[b, b % per] = 10.0 ** (4 * b - 6)
                if kind == "zero":
                    for b in range(B):
                        if not mel[b].any():
                            hand.append(("y~", b * per + np.arange(per), np.full(per, -1.5)))
                y = out_array(B * per)
                y[:B * per] = mel.reshape(-1)
                out.append(case("logmel_finish", "per_b %d B %d %s" % (per, B, kind), y, hand=hand, B=B, per_b=per))
    return out


# ------------------------------------------------------------------------------------------------ VAD_HEAD
@functools.lru_cache(None)
def vad_cases():
    out = []
    for n in (1, 63, 64, 65, 129):
        for hidden in (1, 63, 64, 65):
            g = rng(4, n, hidden)
            hid = g.standard_normal((n, hidden)).astype(F32)
            w2 = (g.standard_normal(hidden) * 0.5).astype(F32)
            b2 = np.array([-1.0], F32)
            hand = []
            hid[0] = -np.abs(hid[0]) - F32(0.5)                             # all negative: relu gives 0, the probability is sigmoid(b2)
            hand.append(("y~", np.array([0]), np.array([1.0 / (1.0 + np.e)])))
            if n > 2:
                hid[1] = -0.0                                               # -0.0 > 0 is false: relu(-0.0) is +0 or -0, the sum is b2 either way
                hand.append(("y~", np.array([1]), np.array([1.0 / (1.0 + np.e)])))
                hid[2], sgn = 100.0, np.sign(w2).astype(F32)                # saturation at both ends: sum = +/- 100 sum |w2|
                hid[2] = np.where(sgn > 0, 300.0, -1.0)
                top = 300.0 * float(np.abs(w2[w2 > 0]).astype(np.float64).sum()) - 1.0
                if top > 90.0:
                    hand.append(("y", np.array([2]), np.array([1.0], F32)))
            if n > 3:
                hid[3] = np.where(np.sign(w2) < 0, 300.0, -1.0)             # a large negative sum: tk_expf's argument is clamped to 88
                low = -300.0 * float(np.abs(w2[w2 < 0]).astype(np.float64).sum()) - 1.0
                if low < -90.0:
                    hand.append(("y~", np.array([3]), np.array([1.0 / (1.0 + np.exp(88.0))])))
            out.append(case("vad_head", "n %d hidden %d" % (n, hidden), out_array(n), a=hid.reshape(-1), b=w2, c=b2, hand=hand, rows=n, hidden=hidden))
        # b2 = 0 and a zero sum: exactly one half
        out.append(case("vad_head", "n %d hidden 3 zero sum" % n, out_array(n), a=np.tile(np.array([1.0, 2.0, -5.0], F32), n), b=np.array([2.0, -1.0, 9.0], F32),
                        c=np.array([0.0], F32), hand=[("y", np.arange(n), np.full(n, 0.5, F32))], rows=n, hidden=3))
    return out


# ------------------------------------------------------------------------------------------------ PREPROCESS
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
PLAIN = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
OTHER = ((0.1, 0.5, 0.9), (0.5, 2.0, 0.25))


@functools.lru_cache(None)
def preprocess_cases():
    out = []
    geoms = [  # in_w in_h out_w out_h bpp pad nhwc norm fill
        (2, 2, 7, 3, 3, 0, 0, IMAGENET, "rand"), (2, 2, 1, 1, 3, 0, 1, PLAIN, "rand"), (5, 3, 65, 5, 3, 0, 0, IMAGENET, "rand"), (5, 3, 65, 5, 4, 9, 1, OTHER, "rand"),
        (37, 23, 32, 32, 3, 0, 1, IMAGENET, "rand"), (37, 23, 32, 32, 4, 5, 0, OTHER, "rand"), (2001, 2, 2, 2, 3, 0, 0, PLAIN, "rand"), (2, 3001, 3, 3, 3, 1, 1, IMAGENET, "rand"),
        (23, 37, 64, 4, 3, 3, 0, PLAIN, "rand"), (37, 23, 4, 64, 4, 0, 1, IMAGENET, "rand"), (9, 7, 9, 7, 3, 0, 0, PLAIN, "zero"), (9, 7, 13, 5, 4, 2, 1, IMAGENET, "full"),
        (3, 3, 6, 6, 3, 0, 0, PLAIN, "rand")]
    for gi, (iw, ih, ow, oh, bpp, padb, nhwc, (mean, std), fill) in enumerate(geoms):
        stride = iw * bpp + padb
        g = rng(5, gi)
        src = g.integers(0, 256, ih * stride).astype(np.uint8)
        img = np.zeros((ih, iw, 3), np.uint8)
        rows = np.lib.stride_tricks.as_strided(src, (ih, stride), (stride, 1))
        if fill != "rand":
            rows[:, :iw * bpp] = 0 if fill == "zero" else 255
        if bpp == 4:
            rows[:, 3:iw * 4:4] = 77                                        # alpha is not 255 and must not be read
        rows[:, iw * bpp:] = 201                                           # row padding: hostile, never read
        img[:] = rows[:, :iw * bpp].reshape(ih, iw, bpp)[:, :, :3]
        src = src[:(ih - 1) * stride + (iw - 1) * bpp + 3].copy()          # the buffer ends at the last pixel's third byte
        for scale, sname in ((1.0 / 255.0, "1/255"), (0.0, "0"), (1.0 / 256.0, "1/256"), (1.0, "1")):
            mult = {"1/255": 1.0 / 255.0, "0": 1.0 / 255.0, "1/256": 1.0 / 256.0, "1": 1.0}[sname]
            hand, np_ = [], ow * oh
            m64, s64 = np.asarray(mean, F32).astype(np.float64), np.asarray(std, F32).astype(np.float64)

            def at(oy, ox, ch):
                return (oy * ow + ox) * 3 + ch if nhwc else ch * np_ + oy * ow + ox
            # output (0, 0) samples source pixel (0, 0) exactly, whatever the ratio
            hand.append(("y~", np.array([at(0, 0, ch) for ch in range(3)]), (img[0, 0].astype(np.float64) * mult - m64) / s64))
            if fill != "rand":                                              # a constant frame stays constant
                hand.append(("y~", np.arange(3 * np_), np.tile(((0.0 if fill == "zero" else 255.0) * mult - m64) / s64, np_) if nhwc else
                             np.repeat(((0.0 if fill == "zero" else 255.0) * mult - m64) / s64, np_)))
            if (iw, ih, ow, oh) == (3, 3, 6, 6):                            # ratio 1/3: output 3 sits on source pixel 1 within rounding, where the stretch is continuous
                hand.append(("y~", np.array([at(3, 3, ch) for ch in range(3)]), (img[1, 1].astype(np.float64) * mult - m64) / s64))
            y = out_array(3 * np_)
            out.append(case("preprocess", "%dx%d -> %dx%d bpp %d stride %d %s %s scale %s" % (iw, ih, ow, oh, bpp, stride, "nhwc" if nhwc else "chw", fill, sname), y, a=src,
                            kernel=0 if sname in ("1/255", "0") else 1, hand=hand, in_w=iw, in_h=ih, in_stride=stride, bpp=bpp, out_w=ow, out_h=oh, nhwc=nhwc,
                            mean=mean, std_dev=std, scale=float(F32(scale)) if sname != "1/255" else float(F32(1.0) / F32(255.0))))
    return out


# ------------------------------------------------------------------------------------------------ DEPTH_MINMAX, DEPTH_METRIC
def depth_maps(n):
    """(name, map, hand min, hand max, flat)"""
    maps = []
    spots = sorted({0, n - 1, min(n - 1, 1023), (n - 1) // 1024 * 1024 + (n - 1) % 1024 // 2})   # element 0, n - 1, thread 1023's share, the last partial stride
    for s in spots:
        for t in spots:
            if s == t and n > 1:
                continue
            x = rng(6, n, s, t).uniform(1.0, 2.0, n).astype(F32)
            x[s] = 0.5
            if t != s:
                x[t] = 3.0
            maps.append(("min at %d max at %d" % (s, t), x, F32(0.5), F32(3.0) if t != s else F32(0.5), n == 1))
    x = -rng(6, n, 77).uniform(1.0, 9.0, n).astype(F32)
    x[n // 2], x[n // 3] = -10.0, -0.25
    maps.append(("all negative", x, x.min(), x.max(), n == 1))
    if n >= 3:
        x = rng(6, n, 78).uniform(0.5, 2.0, n).astype(F32)
        x[0], x[n - 1], x[n // 2] = 0.0, -0.0, -0.0                         # the minimum occurs as +0.0 and as -0.0
        maps.append(("minimum is both zeros", x, F32(0.0), x.max(), False))
    maps.append(("flat", np.full(n, 7.25, F32), F32(7.25), F32(7.25), True))
    if n >= 2:
        below, at = np.nextafter(F32(1e-6), F32(0)), F32(1e-6)
        for name, top, flat in (("range just below 1e-6", below, True), ("range of exactly 1e-6f", at, False), ("range just above 1e-6", np.nextafter(at, F32(1)), False)):
            x = np.zeros(n, F32)
            x[n - 1] = top
            x[1:n - 1] = top / 2
            maps.append((name, x, F32(0), top, flat))
    return maps


@functools.lru_cache(None)
def depth_cases():
    mm_out, metric_out = [], []
    for n in (1, 63, 64, 65, 1023, 1024, 1025, 2049, 24 * 40):
        for name, x, lo, hi, flat in depth_maps(n):
            mm_out.append(case("depth_minmax", "n %d %s" % (n, name), out_array(2), a=x, hand=[("y", np.arange(2), np.array([lo, hi], F32))], n=n))
            for mn, mxd in ((0.1, 10.0), (5.0, 5.0)) if name in ("flat", "all negative") or name.startswith("min at 0 ") else ((0.1, 10.0),):
                hand = [("y2", np.arange(2), np.array([lo, hi], F32))]
                if flat:
                    hand.append(("y", np.arange(n), np.full(n, mxd, F32)))
                else:                                                       # the minimum maps to max_depth exactly, the maximum to min_depth within the span's and the difference's roundings
                    hand.append(("y", np.flatnonzero(x == lo), np.full(int((x == lo).sum()), mxd, F32)))
                    hand.append(("y~", np.flatnonzero(x == hi), np.full(int((x == hi).sum()), float(F32(mn)))))
                metric_out.append(case("depth_metric", "n %d %s depths %g..%g" % (n, name, mn, mxd), out_array(n), a=x, y2=out_array(2), hand=hand, n=n,
                                       min_depth=mn, max_depth=mxd))
    return mm_out, metric_out


# ------------------------------------------------------------------------------------------------ POSTPROCESS_DEPTH, DEPTH_TO_POINTS
SPECIAL_DEPTHS = np.array([2.5, 0.0, -0.0, -1.0, 2.0 ** -149, 1.0], F32)


@functools.lru_cache(None)
def map_cases():
    post, pts = [], []
    for w, h in ((1, 1), (1, 9), (7, 5), (40, 24), (641, 3), (1025, 1030)):
        n = w * h
        blocks = min((n + 255) // 256, GRID_CAP)
        g = rng(7, w, h)
        d = g.uniform(-2.0, 8.0, n).astype(F32)
        k = min(len(SPECIAL_DEPTHS), n)
        d[:k] = SPECIAL_DEPTHS[:k]
        if n > GRID_CAP * 256:                                              # the same specials in the second and in the partial third trip
            d[GRID_CAP * 256:GRID_CAP * 256 + k] = SPECIAL_DEPTHS
            d[n - k:] = SPECIAL_DEPTHS
        scale, shift = 2.0, -0.5
        hand = [("y", np.arange(k), SPECIAL_DEPTHS[:k] * F32(scale) + F32(shift))]
        if n > GRID_CAP * 256:
            hand.append(("y", np.arange(n - k, n), SPECIAL_DEPTHS * F32(scale) + F32(shift)))
        post.append(case("postprocess_depth", "%dx%d scale 2 shift -0.5" % (w, h), out_array(n), a=d, kernel=blocks, hand=hand, width=w, height=h, scale=scale, shift=shift))
        if n <= 1000:
            post.append(case("postprocess_depth", "%dx%d scale 0.1 shift 3" % (w, h), out_array(n), a=d, kernel=blocks, width=w, height=h, scale=0.1, shift=3.0))
        fx, fy, cx, cy = 2.0, 4.0, 0.5 * w - 0.25, 0.5 * h + 0.125             # fx != fy (powers of two: the hand values are exact), fractional centre
        hand = []
        for i in list(range(k)) + ([n - k + q for q in range(k)] if n > GRID_CAP * 256 else []):
            dv = d[i]
            u, v = i % w, i // w
            want = [(u - cx) * float(dv) / fx, (v - cy) * float(dv) / fy, float(dv)] if dv > 0 else [0.0, 0.0, 0.0]
            hand.append(("y~", 3 * i + np.arange(2), np.array(want[:2])))   # x, y inside their three roundings (a subnormal depth: half a unit of 2^-149)
            hand.append(("y", np.array([3 * i + 2]), np.array(want[2:], F32)))
        pts.append(case("depth_to_points", "%dx%d" % (w, h), out_array(3 * n), a=d, kernel=blocks, hand=hand, width=w, height=h, fx=fx, fy=fy, cx=cx, cy=cy))
        if n <= 1000:
            pts.append(case("depth_to_points", "%dx%d odd intrinsics" % (w, h), out_array(3 * n), a=d, kernel=blocks, width=w, height=h, fx=517.3, fy=-331.7, cx=w / 3.0,
                            cy=h / 7.0))
    return post, pts


# ------------------------------------------------------------------------------------------------ BOX_ATTRIBUTES
@functools.lru_cache(None)
def threshold_colours():
    """every RGB triple, in float64: those whose hue lies on a bin boundary, whose saturation is exactly 1/10, whose value is next to 0.1 or 0.9, or whose hue
    is negative before the +360 wrap and lands within a degree of 330 or 360 (one in 31 of those); and a few hundred ordinary ones"""
    v = np.arange(256, dtype=np.int64)
    r, g, b = np.meshgrid(v, v, v, indexing="ij")
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    delta = mx - mn
    # hue * delta / 60 in integers: (g - b), 2 delta + (b - r), 4 delta + (r - g); boundary k * 30 degrees <=> 2 * numerator == k * delta (k odd)
    num = np.where(r == mx, g - b, np.where(g == mx, 2 * delta + (b - r), 4 * delta + (r - g)))
    num = np.where(num < 0, num + 6 * delta, num)
    on_hue = np.zeros(r.shape, bool)
    for k in (1, 3, 5, 7, 9, 11):
        on_hue |= (delta > 0) & (2 * num == k * delta)
    on_sat = (mx > 0) & (10 * delta == mx)
    next_v = np.isin(mx, (25, 26, 229, 230)) & (10 * delta <= mx + 2)
    raw = np.where(r == mx, g - b, 1)
    wrapped = (raw < 0) & (delta > 0) & ((-raw * 60 <= delta) | ((-raw * 60 >= 29 * delta) & (-raw * 60 <= 31 * delta)))   # within a degree of 360 or of 330
    keep = on_hue | on_sat | next_v | (wrapped & ((r + 3 * g + 5 * b) % 31 == 0))
    cols = np.stack([r[keep], g[keep], b[keep]], axis=1).astype(np.uint8)
    crafted = len(cols)
    ordinary = rng(8).integers(0, 256, (400, 3)).astype(np.uint8)
    return np.concatenate([cols, ordinary]), crafted


def luma_pixel(l):
    """a gray pixel whose integer luminance is exactly l"""
    return np.array([l, l, l], np.uint8)


@functools.lru_cache(None)
def box_cases():
    out = []
    # 1. threshold colours: each colour a 2 x 2 region of its own, with a 1 x 1 or a 2 x 2 box
    cols, crafted = threshold_colours()
    per_row = 128
    nrows = -(-len(cols) // per_row)
    W, H = 2 * per_row, 2 * nrows
    frame = np.zeros((H, W, 3), np.uint8)
    rects = np.zeros((len(cols), 4), np.int32)
    for i, c in enumerate(cols):
        x, y = 2 * (i % per_row), 2 * (i // per_row)
        frame[y:y + 2, x:x + 2] = c
        rects[i] = (x, y, 1 + i % 2, 1 + i % 2)
    # the expectation of a one-colour box: that colour's bin, from the float64 definition where it is not ON a boundary; on a boundary the reference's own
    # float32 evaluation decides, and that is recorded from the compiled reference (tests/golden/edge_attributes.json)
    out.append(case("box_attributes", "threshold colours (%d crafted of %d)" % (crafted, len(cols)), out_array(2 * len(cols), np.int32), a=frame.reshape(-1), b=rects.reshape(-1),
                    hand=[("y", 2 * np.arange(len(cols)) + 1, np.zeros(len(cols), np.int32))], in_w=W, in_h=H, rows=len(cols)))
    # 2. ties, frame edges, boxes outside, thin boxes and the edge threshold: one 24 x 20 gray frame (128: bin 8, "gray")
    W, H = 24, 20
    frame = np.full((H, W, 3), 128, np.uint8)
    RED, GREEN, BLUE, WHITE = (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255)
    frame[0:2, 0:2] = [[RED, GREEN], [BLUE, WHITE]]                        # one pixel each of red (0), green (2), blue (4), white (7): the lowest index wins
    frame[0:2, 2:4] = [[GREEN, BLUE], [BLUE, GREEN]]                      # 2 green, 2 blue: green (2)
    # luminance 200 above and 100 (99) below rows 8 (12), columns 4..13: |d| = 100 is no edge, 101 is one
    frame[7, 4:14], frame[9, 4:14] = luma_pixel(200), luma_pixel(100)
    frame[11, 4:14], frame[13, 4:14] = luma_pixel(200), luma_pixel(99)
    frame[16, 0:3] = [RED, GREEN, GREEN]
    boxes = [((0, 0, 2, 2), 0, 0), ((2, 0, 2, 2), 2, 0),
             ((-1, -1, 2, 2), 0, 0),                                       # partly outside: only pixel (0, 0), red, is inside
             ((-5, -5, 3, 3), 0, 0), ((W, H, 4, 4), 0, 0),                 # wholly outside: every bin 0 -> bin 0; no edges
             ((0, 0, 0, 5), 0, 0), ((3, 3, -2, 4), 0, 0), ((3, 3, 4, -1), 0, 0), ((3, 3, -2, -2), 0, 0),   # empty: bin 0; 0 / 0, 0 / -8, 0 / 4 are not > 0.1
             ((5, 5, 1, 6), 8, 0),                                         # 1 pixel wide: no interior
             ((3, 7, 12, 3), 8, 0),                                        # 3 rows: interior row 8, 10 pixels of |d| = 100: no edge
             ((3, 11, 12, 3), 8, 1),                                       # interior row 12, 10 pixels of |d| = 101: 10 / 36
             ((3, 11, 12, 2), 8, 0),                                       # 2 rows tall: no interior
             ((3, 11, 10, 10), 8, 0),                                      # interior columns 4..11 of row 12: 8 / 100 (the box's last row, 20, is outside the frame)
             ((2, 11, 10, 10), 8, 0),                                      # interior columns 3..10: 7 / 100
             ((0, 0, W, H), 8, 0),                                         # the whole frame: row 12's 10 edges and (2, 1) under the white pixel, of 480
             ((4, -1, 6, 3), 8, 0), ((4, H - 2, 6, 3), 8, 0),              # interior row = frame row 0 / H - 1: the edge test skips it (no row above / below)
             ((-3, 16, 6, 1), 2, 0),                                       # columns -3..2 of row 16: red, green, green inside; the three outside count for nothing
             ((-80, 11, 94, 3), 8, 0)]                                     # row 12's edges at columns 4..12: 9 / 282 of the box, though 9 / 42 of its part inside the frame
    rects = np.array([b[0] for b in boxes], np.int32)
    want = np.array([b[1:] for b in boxes], np.int32).reshape(-1)
    out.append(case("box_attributes", "ties, frame edges, thin and empty boxes, edge threshold", out_array(2 * len(boxes), np.int32), a=frame.reshape(-1), b=rects.reshape(-1),
                    hand=[("y", np.arange(2 * len(boxes)), want)], in_w=W, in_h=H, rows=len(boxes)))
    # 3. the density threshold: a 12 x 12 frame of luminance 100, one 10 x 10 box at (1, 1): interior rows 2..9, columns 2..9.  A pixel of luminance 201 in the
    # box's top row (frame row 1) makes ONE strong edge, in row 2 below it (row 0 is no interior); one in the bottom row (10) makes one in row 9 (row 11 is outside
    # the box).  10 edges / 100: (double)(10.0f / 100.0f) = 0.100000001... > 0.1
    for k, closed in ((9, 0), (10, 1), (11, 1)):
        f = np.full((12, 12, 3), 100, np.uint8)
        f[1, 2:10] = 201
        f[10, 2:2 + k - 8] = 201
        out.append(case("box_attributes", "density %d / 100" % k, out_array(2, np.int32), a=f.reshape(-1), b=np.array([1, 1, 10, 10], np.int32),
                        hand=[("y", np.arange(2), np.array([8, closed], np.int32))], in_w=12, in_h=12, rows=1))
    return out


def box_case_list():
    return box_cases()


def every_case(groups=GROUPS):
    out = []
    for gname in groups:
        out.extend(group(gname))
    return out


def group(name):
    if name == "frames":
        return frames_cases()
    if name == "power":
        return power_cases()
    if name == "logmel_finish":
        return logmel_cases()
    if name == "vad_head":
        return vad_cases()
    if name == "preprocess":
        return preprocess_cases()
    if name in ("depth_minmax", "depth_metric"):
        return depth_cases()[0 if name == "depth_minmax" else 1]
    if name in ("postprocess_depth", "depth_to_points"):
        return map_cases()[0 if name == "postprocess_depth" else 1]
    if name == "box_attributes":
        return box_case_list()
    raise KeyError(name)


def probe(tk, c, device):
    """one launch of the hook -> {"y": ..., "y2": ...}, kernel"""
    geometry = {k: c[k] for k in GEOMETRY if k in c}
    y, y2, kernel = tk.edge_probe(getattr(tk, "EDGE_" + c["op"].upper()), c["y"], a=c["a"], b=c["b"], c=c["c"], y2=c["y2"], device=device, **geometry)
    return {"y": y, "y2": y2}, kernel


def reference_a(c):
    """the oracle's own host function on the case's arrays -> {"y": ..., "y2": ...}"""
    op = c["op"]
    if op == "frames":
        return {"y": O.frames(c["a"], c["B"], c["n_samples"], c["pcm_stride"], c["n_total"], c["T"], c["b"], c["y"])}
    if op == "power":
        return {"y": O.power(c["a"], c["rows"], c["nb"], c["y"])}
    if op == "logmel_finish":
        return {"y": O.logmel_finish(c["y"], c["B"], c["per_b"])}
    if op == "vad_head":
        return {"y": O.vad_head(c["a"], c["rows"], c["hidden"], c["b"], c["c"], c["y"])}
    if op == "preprocess":
        return {"y": O.preprocess_scaled(c["a"], c["in_w"], c["in_h"], c["in_stride"], c["bpp"], c["y"], c["out_w"], c["out_h"], c["mean"], c["std_dev"], c["nhwc"], c["scale"])}
    if op == "depth_minmax":
        y = c["y"].copy()
        y[:2] = O.depth_minmax(c["a"])
        return {"y": y}
    if op == "depth_metric":
        y, mm = O.depth_metric(c["a"], c["min_depth"], c["max_depth"], c["y"])
        y2 = c["y2"].copy()
        y2[:2] = mm
        return {"y": y, "y2": y2}
    if op == "postprocess_depth":
        return {"y": O.postprocess_depth(c["a"], c["scale"], c["shift"], c["y"])}
    if op == "depth_to_points":
        return {"y": O.depth_to_points(c["a"], c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], c["y"])}
    if op == "box_attributes":
        return {"y": O.box_attributes(c["a"], c["in_w"], c["in_h"], c["b"], c["y"])}
    raise KeyError(op)


def same_bits(got, want, zero_sign_free=False):
    """bit for bit, except that any NaN matches any NaN; zero_sign_free: +0 and -0 match too (the minimum of a map that holds both)"""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    if got.dtype != F32:
        return np.array_equal(got, want)
    nan = np.isnan(want)
    if zero_sign_free:
        return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], want[~nan])
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def check_hand(c, arrays, bounds=None):
    """the hand-written expectations of a case against the arrays a launch (or a reference) left; "y~": inside B's bound (the value is stated in float64),
    otherwise exact as values.  Returns how many elements were checked."""
    count = 0
    for name, idx, val in c["hand"]:
        soft = name.endswith("~")
        got = np.asarray(arrays[name.rstrip("~")]).reshape(-1)[idx]
        if soft:
            tol = bounds[name.rstrip("~")][idx]
            bad = np.flatnonzero(~(np.abs(got.astype(np.float64) - np.asarray(val, np.float64)) <= tol))
        else:
            bad = np.flatnonzero(~(got == np.asarray(val)))
        assert bad.size == 0, "%s: hand value at %s[%d]: got %r, expected %r" % (c["name"], name, idx[bad[0]], got[bad[0]], np.asarray(val)[bad[0]])
        count += len(idx)
    return count


def refusals():
    """(name, op, keyword arguments of tk.edge_probe) the hook must refuse before any device is touched"""
    f = np.zeros
    out = [
        ("power: out one short", "POWER", dict(y=f(5, F32), a=f(12, F32), rows=2, nb=3)),
        ("power: in one short", "POWER", dict(y=f(6, F32), a=f(11, F32), rows=2, nb=3)),
        ("power: no input", "POWER", dict(y=f(6, F32), a=None, rows=2, nb=3)),
        ("power: a stray array", "POWER", dict(y=f(6, F32), a=f(12, F32), b=f(1, F32), rows=2, nb=3)),
        ("frames: pcm one short", "FRAMES", dict(y=f(2 * 4 * 400, F32), a=f(209 + 199, np.int16), b=f(400, F32), B=2, n_samples=200, pcm_stride=209, n_total=640, T=4)),
        ("frames: stride below the row", "FRAMES", dict(y=f(4 * 400, F32), a=f(400, np.int16), b=f(400, F32), B=1, n_samples=200, pcm_stride=199, n_total=640, T=4)),
        ("frames: window one short", "FRAMES", dict(y=f(4 * 400, F32), a=f(400, np.int16), b=f(399, F32), B=1, n_samples=200, pcm_stride=200, n_total=640, T=4)),
        ("frames: out one short", "FRAMES", dict(y=f(4 * 400 - 1, F32), a=f(400, np.int16), b=f(400, F32), B=1, n_samples=200, pcm_stride=200, n_total=640, T=4)),
        ("frames: n_samples above n_total", "FRAMES", dict(y=f(4 * 400, F32), a=f(700, np.int16), b=f(400, F32), B=1, n_samples=641, pcm_stride=700, n_total=640, T=4)),
        ("frames: a second reflection on the right", "FRAMES", dict(y=f(9 * 400, F32), a=f(400, np.int16), b=f(400, F32), B=1, n_samples=200, pcm_stride=200, n_total=640, T=9)),
        ("frames: a second reflection on the left", "FRAMES", dict(y=f(400, F32), a=f(100, np.int16), b=f(400, F32), B=1, n_samples=100, pcm_stride=100, n_total=200, T=1)),
        ("logmel: one short", "LOGMEL_FINISH", dict(y=f(3 * 63 - 1, F32), B=3, per_b=63)),
        ("logmel: per_b 0", "LOGMEL_FINISH", dict(y=f(3, F32), B=3, per_b=0)),
        ("vad: hidden 0", "VAD_HEAD", dict(y=f(4, F32), a=f(4, F32), b=f(1, F32), c=f(1, F32), rows=4, hidden=0)),
        ("vad: hid one short", "VAD_HEAD", dict(y=f(4, F32), a=f(4 * 5 - 1, F32), b=f(5, F32), c=f(1, F32), rows=4, hidden=5)),
        ("vad: no b2", "VAD_HEAD", dict(y=f(4, F32), a=f(20, F32), b=f(5, F32), c=None, rows=4, hidden=5)),
        ("vad: prob one short", "VAD_HEAD", dict(y=f(3, F32), a=f(20, F32), b=f(5, F32), c=f(1, F32), rows=4, hidden=5)),
        ("depth_minmax: n 0", "DEPTH_MINMAX", dict(y=f(2, F32), a=f(1, F32), n=0)),
        ("depth_minmax: mm one short", "DEPTH_MINMAX", dict(y=f(1, F32), a=f(8, F32), n=8)),
        ("depth_metric: no mm", "DEPTH_METRIC", dict(y=f(8, F32), a=f(8, F32), n=8, min_depth=0.1, max_depth=10.0)),
        ("depth_metric: map one short", "DEPTH_METRIC", dict(y=f(8, F32), y2=f(2, F32), a=f(7, F32), n=8, min_depth=0.1, max_depth=10.0)),
        ("postprocess: out one short", "POSTPROCESS_DEPTH", dict(y=f(34, F32), a=f(35, F32), width=7, height=5, scale=1.0, shift=0.0)),
        ("postprocess: width 0", "POSTPROCESS_DEPTH", dict(y=f(35, F32), a=f(35, F32), width=0, height=5, scale=1.0, shift=0.0)),
        ("points: out one short", "DEPTH_TO_POINTS", dict(y=f(104, F32), a=f(35, F32), width=7, height=5, fx=1.0, fy=1.0, cx=0.0, cy=0.0)),
        ("points: fx 0", "DEPTH_TO_POINTS", dict(y=f(105, F32), a=f(35, F32), width=7, height=5, fx=0.0, fy=1.0, cx=0.0, cy=0.0)),
        ("box: frame one short", "BOX_ATTRIBUTES", dict(y=f(2, np.int32), a=f(4 * 4 * 3 - 1, np.uint8), b=np.array([0, 0, 2, 2], np.int32), in_w=4, in_h=4, rows=1)),
        ("box: rects one short", "BOX_ATTRIBUTES", dict(y=f(4, np.int32), a=f(48, np.uint8), b=f(7, np.int32), in_w=4, in_h=4, rows=2)),
        ("box: out one short", "BOX_ATTRIBUTES", dict(y=f(3, np.int32), a=f(48, np.uint8), b=f(8, np.int32), in_w=4, in_h=4, rows=2)),
        ("box: a box of 2^25 pixels", "BOX_ATTRIBUTES", dict(y=f(2, np.int32), a=f(48, np.uint8), b=np.array([0, 0, 1 << 13, 1 << 12], np.int32), in_w=4, in_h=4, rows=1)),
    ]
    pre = dict(in_w=5, in_h=3, in_stride=15, bpp=3, out_w=4, out_h=4, nhwc=0, mean=(0, 0, 0), std_dev=(1, 1, 1), scale=0.0)
    need = 2 * 15 + 4 * 3 + 3
    for name, change, n_src, n_out in (("src one short", {}, need - 1, 48), ("out one short", {}, need, 47), ("stride below the row", {"in_stride": 14}, need, 48),
                                       ("in_w 1", {"in_w": 1}, need, 48), ("in_h 1", {"in_h": 1}, need, 48), ("bpp 2", {"bpp": 2}, need, 48),
                                       ("out_w 0", {"out_w": 0}, need, 48), ("scale nan", {"scale": float("nan")}, need, 48)):
        kw = dict(pre)
        kw.update(change)
        out.append(("preprocess: " + name, "PREPROCESS", dict(y=f(n_out, F32), a=f(n_src, np.uint8), **kw)))
    return out


# ------------------------------------------------------------------------------------------------ the composed log-mel (Asr.transcribe_tokens)
@functools.lru_cache(None)
def composed_utterances(n_total=16000):
    """[(name, pcm [B][n])]: the utterances of one call share their length"""
    g = rng(9)
    t = np.arange(n_total)
    full = np.zeros((7, n_total), np.int16)
    names = ["silence", "impulse at sample 0", "impulse at the last sample", "full-scale 1 kHz tone", "DC at -32768", "white noise", "white noise, quiet"]
    full[1, 0] = 32767
    full[2, n_total - 1] = 32767
    full[3] = np.round(32767 * np.sin(2 * np.pi * 1000.0 * t / 16000.0)).astype(np.int16)
    full[4] = -32768
    full[5] = np.clip(g.normal(0, 6000, n_total), -32768, 32767).astype(np.int16)
    full[6] = np.clip(g.normal(0, 300, n_total), -32768, 32767).astype(np.int16)
    return [("n_total samples", names, full),
            ("100 samples", ["noise, 100 samples"], np.clip(g.normal(0, 6000, (1, 100)), -32768, 32767).astype(np.int16)),
            ("201 samples", ["noise, 201 samples"], np.clip(g.normal(0, 6000, (1, 201)), -32768, 32767).astype(np.int16))]


def check_composed(names, mel, want, bound):
    """mel [B][T][n_mels] against the float64 restatement; the hand expectations; returns (worst error / bound, share of elements whose bound is below 1e-3 per row)"""
    err = np.abs(mel.astype(np.float64) - want)
    ratio = err / bound
    worst = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    assert ratio[worst] <= 1.0, "%s frame %d mel %d: %r, float64 %r = %.2f bounds" % (names[worst[0]], worst[1], worst[2], mel[worst], want[worst], ratio[worst])
    for b, name in enumerate(names):
        if name == "silence":                                               # every power is 0: log10(1e-10) = -10 everywhere, the maximum included
            assert np.abs(mel[b].astype(np.float64) + 1.5).max() <= R.LOG10_ABS, name
        if name.startswith("impulse"):                                      # frames that do not see the impulse are silent: -10, or the clamp 8 below the maximum
            quiet = mel[b, 2:] if "sample 0" in name else mel[b, :-1]      # sample 0 lies in frames 0 and 1 (tap 200, window 1: the clamp is active); the last one in frame T - 1
            floor = max(-1.5, float(mel[b].max()) - 2.0)
            assert np.abs(quiet.astype(np.float64) - floor).max() <= 2.4e-7 + R.LOG10_ABS / 4, name
            assert ("sample 0" in name) == (floor > -1.5), name
        if name.startswith("full-scale"):                                   # 1 kHz is bin 25 of 201; the loudest mel filter of an interior frame is the one around it
            peak = int(np.argmax(mel[b, mel.shape[1] // 2]))
            centres = np.argmax(R.slaney_filters(mel.shape[2]), axis=1)
            assert abs(int(centres[peak]) - 25) <= 1, (name, peak)
    return float(ratio[worst]), (bound < 1e-3).mean(axis=(1, 2))


# ------------------------------------------------------------------------------------------------ recorded answers of the compiled reference
@functools.lru_cache(None)
def recorded():
    """tests/golden/edge_reference_answers.npz (tests/golden/make_edge_golden.py): the compiled reference's own answers on the box cases and on the
    tightly packed RGB8 pre-processor cases at scale 1/255, keyed by the case's position in its group, with the sha256 of the inputs"""
    import os
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edge_reference_answers.npz")))


def check_recorded(op, index, c, arrays):
    """what a launch (or reference A) left against the compiled reference's recorded answer; returns the number of elements compared (0: nothing recorded)"""
    import hashlib
    if op not in ("box_attributes", "preprocess"):
        return 0
    rec = recorded()
    key = ("box%d" if op == "box_attributes" else "pre%d") % index
    if key not in rec:
        return 0
    digest = hashlib.sha256(c["a"].tobytes()).hexdigest() + (hashlib.sha256(c["b"].tobytes()).hexdigest() if op == "box_attributes" else "")
    assert bytes(rec[key + "_sha"]).hex() == digest, "%s: the case's inputs are not the recorded ones: run tests/golden/make_edge_golden.py" % c["name"]
    if op == "box_attributes":
        want = rec[key].reshape(-1)
        got = np.asarray(arrays["y"])[:len(want)]
        have = want != 255
        bad = np.flatnonzero(have & (got != want))
        assert bad.size == 0, "%s: box %d %s: %d, the compiled reference %d" % (c["name"], bad[0] // 2, ("colour", "door")[bad[0] % 2], got[bad[0]], want[bad[0]])
        return int(have.sum())
    want = rec[key]                                                         # planar [3][out_h][out_w]
    n = want.size
    got = np.asarray(arrays["y"])[:n]
    got = got.reshape(c["out_h"], c["out_w"], 3).transpose(2, 0, 1) if c["nhwc"] else got.reshape(want.shape)
    assert same_bits(got, want), "%s: differs from the compiled reference by up to %g" % (c["name"], np.abs(got - want).max())
    return n
