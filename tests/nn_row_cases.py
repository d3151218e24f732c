"""The launches of tests/test_nn_rows_gpu.py, shared with tests/test_nn_rows_cpu.py: one tk_mi355x_nn_row_probe call each.

A launch: dict(name, op, geometry (the probe's integer fields and eps), a / b / c / idx / pos_idx inputs, y (and img) with the caller's initial content —
SENTINEL wherever the kernel must not write — a_offset / y_offset, kernel (the launcher's expected code), oracle_only (rows with infinities or NaN:
compared against the oracle alone, NaN positions included)).  GROUP_NAMES lists the groups, one GPU test each; group(name) builds a group's launches
when asked (nothing is generated at import).

reference_a(launch) runs the oracle on a copy of y / img and returns the whole arrays; with one of ORACLE_MUTATIONS it runs the oracle's mutant instead:
the two modelled kernel errors that only the BITS of reference A can show (float64 cannot tell them from the contract)."""
import functools
import itertools
import zlib

import numpy as np

import nn_row_ref as R
import oracle_lib as O

SENTINEL = np.float32(-777.25)
SOFTMAX_GENERIC, SOFTMAX_REG, SOFTMAX_WAVE = 0, 1, 2
IM2COL_ELEMENT, IM2COL_V4 = 0, 1


def launch(name, op, geometry, y, kernel=0, **kw):
    l = dict(name=name, op=op, geometry=geometry, y=np.ascontiguousarray(y, np.float32).reshape(-1), kernel=kernel, a=None, b=None, c=None, idx=None, pos_idx=None,
             img=None, a_offset=0, y_offset=0, oracle_only=False, plain=False)
    l.update(kw)
    return l


def rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ---------------------------------------------------------------- softmax_rows

def softmax_kernel(rows, cols, ld, offset):
    """the issue's statement of the launcher's choice: one wave per row for cols <= 2048 with 16-byte rows and at least 1024 of them, registers for
    cols <= 2048, else the three-pass kernel"""
    if cols <= 2048 and cols % 4 == 0 and ld % 4 == 0 and offset % 4 == 0 and rows >= 1024:
        return SOFTMAX_WAVE
    return SOFTMAX_REG if cols <= 2048 else SOFTMAX_GENERIC


def softmax_rows_content(r, rows, cols):
    """row r's pattern: random, one dominant value, all equal, spread +/-80 — cycling, so every launch holds each"""
    x = np.empty((rows, cols), np.float32)
    for i in range(rows):
        kind = i % 4
        if kind == 0:
            x[i] = r.normal(0, 3, cols)
        elif kind == 1:
            x[i] = r.normal(0, 1, cols)
            x[i, (i * 7) % cols] = 60.0
        elif kind == 2:
            x[i] = 1.5
        else:
            x[i] = r.uniform(-80, 80, cols)
    return x


def softmax_launch(rows, cols, ld, offset=0, special=False):
    r = rng("softmax", rows, cols, ld, offset)
    x = softmax_rows_content(r, rows, cols)
    if special:                                                             # a -inf entry, an all -inf row, a +inf entry
        x[0, cols // 2] = -np.inf
        x[1 % rows] = -np.inf
        x[2 % rows, cols - 1] = np.inf
    y = np.full((rows, ld), SENTINEL, np.float32)
    y[:, :cols] = x
    y = y.reshape(-1)[:(rows - 1) * ld + cols] if ld > cols and rows % 2 else y.reshape(-1)      # with and without the last row's pitch
    return launch("softmax %d x %d ld %d%s%s" % (rows, cols, ld, " +%d" % offset if offset else "", " inf" if special else ""), "softmax_rows",
                  dict(rows=rows, C=cols, ldy=ld), y, kernel=softmax_kernel(rows, cols, ld, offset), y_offset=offset, oracle_only=special)


SOFTMAX_COLS = (1, 3, 4, 63, 64, 65, 255, 256, 257, 1500, 2044, 2047, 2048, 2049, 2052, 4099)


def softmax_group(which):
    if which == "softmax_few_rows":
        few = []
        for i, cols in enumerate(SOFTMAX_COLS):
            for rows in (1, 5):
                few.append(softmax_launch(rows, cols, cols))
                few.append(softmax_launch(rows, cols, cols + (4 if (i + rows) % 2 else 3)))
        few.append(softmax_launch(5, 257, 260, special=True))
        few.append(softmax_launch(5, 4099, 4099, special=True))
        return few
    narrow = which == "softmax_1024_rows_narrow"
    many = []
    # rows around the wave kernel's threshold; cols on both sides of every condition it has (a multiple of 4 or not, 2048 / 2052), packed rows and
    # pitches of + 4 (still 16-byte rows) and + 3 (not), and a base one element off
    for rows, cols, ld, off in ((1023, 64, 64, 0), (1024, 64, 64, 0), (1027, 64, 68, 0), (1024, 64, 67, 0), (1024, 64, 64, 1), (1027, 4, 4, 0), (1024, 1, 1, 0),
                                (1024, 3, 4, 0), (1024, 63, 64, 0), (1024, 65, 68, 0), (1027, 255, 256, 0), (1024, 256, 256, 0), (1024, 257, 260, 0),
                                (1027, 1500, 1500, 0), (1024, 1500, 1504, 1), (1024, 2044, 2044, 0), (1027, 2047, 2048, 0), (1024, 2048, 2048, 0),
                                (1024, 2048, 2052, 0), (1027, 2048, 2051, 0), (1024, 2049, 2052, 0), (1024, 2052, 2052, 0), (1027, 4099, 4099, 0)):
        if (cols <= 257) == narrow:
            many.append(softmax_launch(rows, cols, ld, off))
    if not narrow:
        many.append(softmax_launch(1027, 1500, 1504, special=True))
    return many


# ---------------------------------------------------------------- layernorm

def layernorm_launch(rows, D, with_img, eps):
    r = rng("layernorm", rows, D)
    x = r.normal(0, 1, (rows, D)).astype(np.float32)
    x[0] = 2.5                                                              # a constant row: variance 0, y = b
    if rows > 1:
        x[1] = 1e4 + r.uniform(-1e-2, 1e-2, D)                              # mean 1e4, spread 1e-2: the variance is all cancellation
    if rows > 2:
        x[2] = 100.0 + r.uniform(-1, 1, D)                                  # mean 100, spread 1: still well conditioned in two passes
    w, b = r.normal(1, 0.3, D).astype(np.float32), r.normal(0, 0.5, D).astype(np.float32)
    img = np.full(-(-rows // 16) * 16 * D, SENTINEL, np.float32) if with_img else None
    return launch("layernorm %d x %d%s" % (rows, D, " img" if with_img else ""), "layernorm", dict(rows=rows, C=D, eps=eps), np.full(rows * D, SENTINEL, np.float32),
                  a=x, b=w, c=b, img=img)


def layernorm_groups(eps):
    out = []
    for D in (1, 16, 100, 255, 256, 257, 384, 1000):
        for rows in (1, 15, 16, 17, 33):
            out.append(layernorm_launch(rows, D, False, eps))
            if D % 16 == 0:
                out.append(layernorm_launch(rows, D, True, eps))
    return {"layernorm": out}


# ---------------------------------------------------------------- im2col, im2col1d

def pixels(r, n, C, ldx):
    x = np.full((n, ldx), SENTINEL, np.float32)
    x[:, :C] = r.normal(0, 1, (n, C))
    return x.reshape(-1)[:(n - 1) * ldx + C]


def im2col_groups():
    two_d, one_d = [], []
    for C, wider in itertools.product((3, 4, 8, 12), (0, 1, 4)):
        ldx = C + wider
        for k, stride, pad, (H, W), B in itertools.product((1, 3), (1, 2), (0, 1, 2), ((5, 7), (1, 1)), (1, 3)):
            if H + 2 * pad < k:
                continue
            Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
            for off in ((0, 1) if (B, stride) == (1, 1) else (0,)):       # an unaligned col base on a part of them
                v4 = C % 4 == 0 and ldx % 4 == 0 and off == 0
                two_d.append(launch("im2col C %d ldx %d k %d s %d p %d %dx%d B %d +%d" % (C, ldx, k, stride, pad, H, W, B, off), "im2col",
                                    dict(B=B, H=H, W=W, C=C, ldx=ldx, k=k, stride=stride, pad=pad), np.full(B * Ho * Wo * k * k * C + 5, SENTINEL, np.float32),
                                    a=pixels(rng("im2col", C, ldx, H, B), B * H * W, C, ldx), kernel=IM2COL_V4 if v4 else IM2COL_ELEMENT, y_offset=off))
        if C % 4 == 0 and wider == 0:                                       # the INPUT one element off 16 bytes: 16-byte channel groups, but no 16-byte loads
            two_d.append(launch("im2col C %d ldx %d k 3 s 1 p 1 5x7 B 1 x +1" % (C, ldx), "im2col", dict(B=1, H=5, W=7, C=C, ldx=ldx, k=3, stride=1, pad=1),
                                np.full(35 * 9 * C + 5, SENTINEL, np.float32), a=pixels(rng("im2col x off", C), 35, C, ldx), kernel=IM2COL_ELEMENT, a_offset=1))
        for k, stride, pad, T, B in itertools.product((1, 3), (1, 2), (0, 1, 2), (7, 1), (1, 3)):
            if T + 2 * pad < k or wider == 4:                               # one element-wise kernel: two pitches are enough
                continue
            To = (T + 2 * pad - k) // stride + 1
            one_d.append(launch("im2col1d C %d ldx %d k %d s %d p %d T %d B %d" % (C, ldx, k, stride, pad, T, B), "im2col1d",
                                dict(B=B, H=T, C=C, ldx=ldx, k=k, stride=stride, pad=pad), np.full(B * To * k * C + 5, SENTINEL, np.float32),
                                a=pixels(rng("im2col1d", C, ldx, T, B), B * T, C, ldx), y_offset=(C + T) % 2))
    return {"im2col": two_d, "im2col1d": one_d}


# ---------------------------------------------------------------- conv_stem

def conv_stem_groups():
    out = []
    r = rng("stem weights")
    w, bias = r.normal(0, 0.3, (16, 27)).astype(np.float32), r.normal(0, 0.5, 16).astype(np.float32)
    for (H, W), stride, pad, B, ldx, ldy, has_bias, act in itertools.product(((1, 1), (5, 7), (17, 16)), (1, 2), (0, 1), (1, 2), (3, 4), (16, 20), (False, True), (0, 1)):
        if H + 2 * pad < 3:
            continue
        Ho, Wo = (H + 2 * pad - 3) // stride + 1, (W + 2 * pad - 3) // stride + 1
        out.append(launch("conv_stem %dx%d s %d p %d B %d ldx %d ldy %d%s%s" % (H, W, stride, pad, B, ldx, ldy, " bias" if has_bias else "", " silu" if act else ""), "conv_stem",
                          dict(B=B, H=H, W=W, C=3, ldx=ldx, N=16, k=3, stride=stride, pad=pad, ldy=ldy, act=act), np.full(B * Ho * Wo * ldy, SENTINEL, np.float32),
                          a=pixels(rng("stem", H, B, ldx), B * H * W, 3, ldx), b=w, c=bias if has_bias else None))
    # "padding taps taking part as a = 0": an infinite weight on the top-left tap makes 0 * inf = NaN wherever that tap lies in the padding (the first
    # row and column of channel 5) — a kernel that SKIPS padding taps answers a finite value there.  Finite weights cannot tell the two apart.
    w_inf = w.copy()
    w_inf[5, 1] = np.inf
    for stride, has_bias in ((1, False), (2, True)):
        Ho, Wo = (5 + 2 - 3) // stride + 1, (7 + 2 - 3) // stride + 1
        out.append(launch("conv_stem 5x7 s %d p 1 inf weight on a padding tap%s" % (stride, " bias" if has_bias else ""), "conv_stem",
                          dict(B=2, H=5, W=7, C=3, ldx=3, N=16, k=3, stride=stride, pad=1, ldy=16, act=0), np.full(2 * Ho * Wo * 16, SENTINEL, np.float32),
                          a=pixels(rng("stem inf", stride), 2 * 35, 3, 3), b=w_inf, c=bias if has_bias else None, oracle_only=True))
    return {"conv_stem": out}


# ---------------------------------------------------------------- maxpool5, upsample2x, copy_cols, add_rows, embed_rows

def layout_groups():
    pool, up, copy = [], [], []
    for (H, W), C in itertools.product(((1, 1), (1, 9), (2, 3), (3, 2), (5, 5), (9, 2), (5, 9)), (1, 5)):
        B, ldx, ldy = 2, C + 2, C + 3
        r = rng("layout", H, W, C)
        x = pixels(r, B * H * W, C, ldx)
        xp = x.copy()
        xp[(np.arange(B * H * W) * ldx)[::3]] = -np.inf                      # -inf among the inputs: a window of nothing else answers -inf
        pool.append(launch("maxpool5 %dx%d C %d" % (H, W, C), "maxpool5", dict(B=B, H=H, W=W, C=C, ldx=ldx, ldy=ldy), np.full(B * H * W * ldy, SENTINEL, np.float32), a=xp))
        up.append(launch("upsample2x %dx%d C %d" % (H, W, C), "upsample2x", dict(B=B, H=H, W=W, C=C, ldx=ldx, ldy=ldy), np.full(B * 4 * H * W * ldy, SENTINEL, np.float32), a=x))
        copy.append(launch("copy_cols %d x %d" % (B * H * W, C), "copy_cols", dict(rows=B * H * W, C=C, ldx=ldx, ldy=ldy), np.full(B * H * W * ldy, SENTINEL, np.float32), a=x))
    xn = pixels(rng("nan"), 2 * 5 * 5, 5, 7)
    xn[7 * 12 + 2] = np.nan                                                  # tk_fmaxf keeps or drops a NaN by its place in the window: the oracle's order
    pool.append(launch("maxpool5 5x5 C 5 nan", "maxpool5", dict(B=2, H=5, W=5, C=5, ldx=7, ldy=8), np.full(2 * 25 * 8, SENTINEL, np.float32), a=xn, oracle_only=True))
    add = []
    for rows, n_add in ((7, 1), (7, 7), (7, 3), (300, 3)):
        r = rng("add", rows, n_add)
        add.append(launch("add_rows %d + %d" % (rows, n_add), "add_rows", dict(rows=rows, C=33, add_rows=n_add),
                          np.concatenate([r.normal(0, 1, rows * 33).astype(np.float32), np.full(4, SENTINEL, np.float32)]), a=r.normal(0, 1, (n_add, 33)).astype(np.float32)))
    embed = []
    for D in (1, 127, 129, 384):
        r = rng("embed", D)
        idx = np.array([0, 10, 10, 3, 10, 0, 9], np.int32)                   # repeated indices, the first and the last table row
        pos_idx = np.array([5, 0, 0, 5, 1, 2, 2], np.int32)
        embed.append(launch("embed_rows D %d" % D, "embed_rows", dict(rows=7, C=D, table_rows=11, pos_rows=6), np.full(7 * D + 3, SENTINEL, np.float32),
                            a=r.normal(0, 1, (11, D)).astype(np.float32), b=r.normal(0, 1, (6, D)).astype(np.float32), idx=idx, pos_idx=pos_idx))
    return {"maxpool5": pool, "upsample2x": up, "copy_cols": copy, "add_rows": add, "embed_rows": embed}


# ---------------------------------------------------------------- attend1

def attend1_launch(hd, nh, B, Tk, wide=False, img=False, special=None, patterns=(0, 1, 2, 3), q_offset=0):
    """score patterns cycle over (sequence, head): 0 random, 1 one dominant key at a chunk edge (64 keys per ring slot), 2 all equal, 3 spread +/-80.
    patterns = (0, 2) keeps the scores small: reference B's bound, which carries the score chain's error through the exponent, is then tight"""
    d = nh * hd
    r = rng("attend1", hd, nh, B, Tk, wide, special, patterns)
    qs, kvs = (d + 8, Tk * d + 4 * d) if wide else (d, Tk * d)
    if special == "gap":
        kvs = Tk * d + d
    q = np.full((B - 1) * qs + d, SENTINEL, np.float32)
    k = np.full((B - 1) * kvs + Tk * d + (d if special == "gap" else 0), 1e30 if special == "gap" else 0.0, np.float32)
    v = k.copy()
    scale = 1.0 / np.sqrt(hd)
    edges = [t for t in (0, 63, 64, 127, 128, 191, 192, Tk - 1) if t < Tk]
    for b in range(B):
        q[b * qs:b * qs + d] = r.normal(0, 1, d)
        K, V = r.normal(0, 1, (Tk, d)).astype(np.float32), r.normal(0, 1, (Tk, d)).astype(np.float32)
        for h in range(nh):
            qh = q[b * qs + h * hd:b * qs + (h + 1) * hd].astype(np.float64)
            unit = qh / (qh @ qh) / scale                                   # a key c * unit scores c
            kind = patterns[(b * nh + h) % len(patterns)]
            if kind == 1:
                K[edges[(b + h) % len(edges)], h * hd:(h + 1) * hd] = 30.0 * unit
            elif kind == 2:
                K[:, h * hd:(h + 1) * hd] = K[0, h * hd:(h + 1) * hd]
            elif kind == 3:
                K[:, h * hd:(h + 1) * hd] = r.uniform(-80, 80, (Tk, 1)) * unit
            if special == "underflow" and Tk > 1:                           # the last key 100 below the best: its probability is exactly 0 and 0 * 1e30 = 0
                K[:, h * hd:(h + 1) * hd] = r.uniform(-1, 1, (Tk, 1)) * unit
                K[Tk - 1, h * hd:(h + 1) * hd] = -100.0 * unit
        if special == "underflow":
            V[Tk - 1] = 1e30
        k[b * kvs:b * kvs + Tk * d], v[b * kvs:b * kvs + Tk * d] = K.reshape(-1), V.reshape(-1)
    image = np.full(-(-B // 16) * 16 * d, SENTINEL, np.float32) if img else None
    name = "attend1 hd %d nh %d B %d Tk %d%s%s%s%s%s" % (hd, nh, B, Tk, " wide" if wide else "", " img" if img else "", " " + special if special else "",
                                                       " plain" if patterns == (0, 2) else "", " q +%d" % q_offset if q_offset else "")
    return launch(name, "attend1", dict(B=B, H=Tk, C=d, N=nh, q_bstride=qs, kv_bstride=kvs), np.full(q.size, SENTINEL, np.float32), a=q, b=k, c=v, img=image,
                  a_offset=q_offset, plain=patterns == (0, 2))


def attend1_groups():
    out = []
    shapes = itertools.cycle([(16, 6, 3), (32, 2, 1), (48, 1, 17), (64, 6, 1), (64, 2, 3), (16, 1, 1), (32, 6, 17), (48, 2, 3)])
    for i, Tk in enumerate((1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257, 449, 1500)):
        hd, nh, B = next(shapes)
        out.append(attend1_launch(hd, nh, B, Tk, wide=bool(i % 2), img=i % 3 != 1))
        if Tk in (65, 193, 449):                                            # the ring's edges at the Whisper head size as well
            out.append(attend1_launch(64, 6, 3, Tk, wide=True, img=True))
    out.append(attend1_launch(64, 2, 17, 200, img=True))                    # 17 sequences: the second image block holds one row
    out.append(attend1_launch(64, 1, 1, 3008))                              # the largest Tk the launcher admits at hd = 64
    out.append(attend1_launch(64, 2, 3, 130, special="underflow"))
    out.append(attend1_launch(32, 2, 3, 65, special="gap"))
    out.append(attend1_launch(32, 2, 3, 65, q_offset=1))                    # q one element off 16 bytes: it is read one float at a time
    out.append(attend1_launch(64, 6, 3, 193, patterns=(0, 2)))              # small scores only: reference B's bound at its tightest
    out.append(attend1_launch(48, 2, 3, 449, wide=True, patterns=(0, 2)))
    return {"attend1": out}


GROUP_NAMES = ("softmax_few_rows", "softmax_1024_rows_narrow", "softmax_1024_rows_wide", "layernorm", "im2col", "im2col1d", "conv_stem", "maxpool5", "upsample2x",
               "copy_cols", "add_rows", "embed_rows", "attend1")
ORACLE_MUTATIONS = ("softmax_sum_order_reversed", "conv_stem_padding_tap_skipped")


@functools.lru_cache(maxsize=1)
def group(name):
    """the launches of one group, built when asked for (the softmax groups hold tens of megabytes: only the last one asked for is kept)"""
    if name.startswith("softmax"):
        return softmax_group(name)
    family = {"layernorm": lambda: layernorm_groups(O.layernorm_eps()), "im2col": im2col_groups, "im2col1d": im2col_groups, "conv_stem": conv_stem_groups,
              "attend1": attend1_groups}.get(name, layout_groups)
    return family()[name]


def every_launch(ops=None):
    """all launches, group after group (ops: only the groups that hold these ops)"""
    for name in GROUP_NAMES:
        if ops is None or any(name.startswith(o.split("_")[0]) for o in ops):
            for l in group(name):
                if ops is None or l["op"] in ops:
                    yield l


def reference_a(l, mutant=None):
    """the oracle on copies of the launch's in/out arrays -> (y, img), whole; None where the oracle has no such step (pure gathers: reference B is exact).
    mutant: one of ORACLE_MUTATIONS"""
    g, op = l["geometry"], l["op"]
    y = np.array(l["y"], np.float32)
    img = None
    if op == "softmax_rows":
        y = O.softmax_rows(y, g["rows"], g["C"], g["ldy"], reversed_sum=mutant == "softmax_sum_order_reversed")
    elif op == "layernorm":
        rows, D = g["rows"], g["C"]
        v = O.layernorm(np.asarray(l["a"]).reshape(rows, D), l["b"], l["c"])
        y[:rows * D] = v.reshape(-1)
        if l["img"] is not None:
            img = np.array(l["img"], np.float32)
            img[R.image_index(rows, D)] = v
    elif op == "im2col1d":
        col = O.im2col1d(l["a"], g["B"], g["H"], g["C"], g["ldx"], g["k"], g["stride"], g["pad"])
        y[:col.size] = col
    elif op in ("maxpool5", "upsample2x"):
        y = O.pool_or_upsample(op, l["a"], y, g["B"], g["H"], g["W"], g["C"], g["ldx"], g["ldy"])
    elif op == "add_rows":
        y[:g["rows"] * g["C"]] = O.add_rows(y[:g["rows"] * g["C"]], l["a"], g["rows"], g["C"], g["add_rows"])
    elif op == "embed_rows":
        y[:g["rows"] * g["C"]] = O.embed_rows(l["a"], l["b"], l["idx"], l["pos_idx"], g["C"])
    elif op == "conv_stem":                                                # the chain the stem must equal: the oracle's own im2col + orc_gemm with its epilogue
        y = O.conv_chain(l["a"], l["b"], l["c"], y, g["B"], g["H"], g["W"], 3, g["ldx"], 16, 3, g["stride"], g["pad"], g["ldy"], g["act"],
                         skip_padding_taps=mutant == "conv_stem_padding_tap_skipped")
    elif op == "attend1":
        y = O.attend1(l["a"], l["b"], l["c"], y, g["B"], g["H"], g["q_bstride"], g["kv_bstride"], g["C"], g["N"])
        if l["img"] is not None:
            img = np.array(l["img"], np.float32)
            img[R.image_index(g["B"], g["C"])] = np.lib.stride_tricks.as_strided(y, (g["B"], g["C"]), (g["q_bstride"] * 4, 4))
    else:
        return None, None
    return y, img


def probe(tk, l, device):
    """one launch of the list through the hook -> (y, img, kernel code)"""
    return tk.nn_row_probe(getattr(tk, "ROW_" + l["op"].upper()), l["y"], a=l["a"], b=l["b"], c=l["c"], idx=l["idx"], pos_idx=l["pos_idx"], img=l["img"],
                           a_offset=l["a_offset"], y_offset=l["y_offset"], device=device, **l["geometry"])


def refusals():
    """(name, op, keyword arguments) the hook must refuse (TK_ERROR_INVALID_ARGUMENT, nothing launched), with the kernel code it then reports"""
    z = np.zeros
    stem = dict(B=1, H=5, W=7, C=3, ldx=3, N=16, k=3, stride=1, pad=1, ldy=16, act=0)
    sw, sx, sy = z(16 * 27, np.float32), z(35 * 3, np.float32), z(35 * 16, np.float32)
    out = [("softmax rows 0", "softmax_rows", dict(y=z(8, np.float32), rows=0, C=8, ldy=8)),
           ("softmax ld below cols", "softmax_rows", dict(y=z(64, np.float32), rows=4, C=8, ldy=7)),
           ("softmax y too short", "softmax_rows", dict(y=z(31, np.float32), rows=4, C=8, ldy=8)),
           ("layernorm image with D % 16 != 0", "layernorm", dict(y=z(40, np.float32), a=z(40, np.float32), b=z(20, np.float32), c=z(20, np.float32), img=z(16 * 20, np.float32), rows=2, C=20, eps=1e-5)),
           ("layernorm image too short", "layernorm", dict(y=z(17 * 16, np.float32), a=z(17 * 16, np.float32), b=z(16, np.float32), c=z(16, np.float32), img=z(17 * 16, np.float32), rows=17, C=16, eps=1e-5)),
           ("layernorm rows 0", "layernorm", dict(y=z(16, np.float32), a=z(16, np.float32), b=z(16, np.float32), c=z(16, np.float32), rows=0, C=16, eps=1e-5)),
           ("conv_stem N 8", "conv_stem", dict(y=sy, a=sx, b=sw, **dict(stem, N=8, ldy=8))),
           ("conv_stem C 4", "conv_stem", dict(y=sy, a=z(35 * 4, np.float32), b=z(16 * 36, np.float32), **dict(stem, C=4, ldx=4))),
           ("conv_stem ldy 18", "conv_stem", dict(y=z(35 * 18, np.float32), a=sx, b=sw, **dict(stem, ldy=18))),
           ("conv_stem y off 16 bytes", "conv_stem", dict(y=sy, a=sx, b=sw, y_offset=1, **stem)),
           ("conv_stem stride 0", "conv_stem", dict(y=sy, a=sx, b=sw, **dict(stem, stride=0))),
           ("conv_stem x too short", "conv_stem", dict(y=sy, a=sx[:-1], b=sw, **stem)),
           ("im2col window wider than the input", "im2col", dict(y=z(64, np.float32), a=z(3, np.float32), B=1, H=1, W=1, C=3, ldx=3, k=3, stride=1, pad=0)),
           ("im2col col too short", "im2col", dict(y=z(35 * 27 - 1, np.float32), a=sx, B=1, H=5, W=7, C=3, ldx=3, k=3, stride=1, pad=1)),
           ("maxpool ldy below C", "maxpool5", dict(y=z(35 * 3, np.float32), a=sx, B=1, H=5, W=7, C=3, ldx=3, ldy=2)),
           ("embed_rows index beyond the table", "embed_rows", dict(y=z(8, np.float32), a=z(12, np.float32), b=z(8, np.float32), idx=np.array([0, 3], np.int32), pos_idx=np.array([0, 1], np.int32), rows=2, C=4, table_rows=3, pos_rows=2)),
           ("embed_rows negative position", "embed_rows", dict(y=z(8, np.float32), a=z(12, np.float32), b=z(8, np.float32), idx=np.array([0, 2], np.int32), pos_idx=np.array([0, -1], np.int32), rows=2, C=4, table_rows=3, pos_rows=2)),
           ("add_rows add_rows 0", "add_rows", dict(y=z(8, np.float32), a=z(4, np.float32), rows=2, C=4, add_rows=0))]
    def att(Tk=8, d=64, nh=1, B=2, qs=None, kvs=None, n_kv=None):
        qs, kvs = d if qs is None else qs, Tk * d if kvs is None else kvs
        n_kv = (B - 1) * kvs + Tk * d if n_kv is None else n_kv
        return dict(y=z((B - 1) * qs + d, np.float32), a=z((B - 1) * qs + d, np.float32), b=z(n_kv, np.float32), c=z(n_kv, np.float32), B=B, H=Tk, C=d, N=nh, q_bstride=qs, kv_bstride=kvs)
    out += [("attend1 hd 64 Tk 3009: more than 60 KiB of LDS", "attend1", att(Tk=3009, B=1)), ("attend1 hd 80", "attend1", att(d=80)), ("attend1 hd 8", "attend1", att(d=16, nh=2)),
            ("attend1 q_bstride 66", "attend1", att(qs=66)), ("attend1 kv_bstride no multiple of 4", "attend1", att(kvs=8 * 64 + 2)),
            ("attend1 d no multiple of nh", "attend1", att(d=64, nh=3)), ("attend1 k too short", "attend1", att(n_kv=2 * 8 * 64 - 1)),
            ("attend1 q rows overlap", "attend1", att(qs=32))]
    return out


def accepted():
    """validate-only calls the hook must accept: the launcher's LDS limit from below"""
    z = np.zeros
    return [("attend1 hd 64 Tk 3008", "attend1", dict(y=z(64, np.float32), a=z(64, np.float32), b=z(3008 * 64, np.float32), c=z(3008 * 64, np.float32), B=1, H=3008, C=64, N=1,
                                                      q_bstride=64, kv_bstride=3008 * 64))]
