"""The launches of tests/test_llm_step_gpu.py, shared with tests/test_llm_step_cpu.py: one tk_mi355x_llm_step_probe call each.

The shapes are the smallest at which each kernel can still go wrong, not a model's: every size at which a launcher or a kernel takes another path
(d_model / 4 no multiple of 256, above 1024 threads' worth, the second chunk pass from d_model 8448; d_ff with a partly filled second workgroup;
1, 2 .. 8 K-split slabs; every head geometry a model may have), rows on both sides of an M-tile's edge, and crafted rows:

- ties: +a and -a in one 256-block at element pairs that cross every shuffle distance of the image writer's merge, the chunk boundary and one pair
  inside a chunk, in both orders; which element becomes -127 and the sign of d are written by hand (TIE_EXPECT);
- an all-zero block between live ones, an all-zero row;
- sub-blocks of all +127 / all -127 (sums +-4064) and sub-block sums of -1, +1, -63, -127 for the (l, h) and (hh, ll) splits;
- for QUANT, whose input is exact: a block whose extreme is -127 (iscale exactly 1) holding 0.5, 1.5, 2.5, -0.5, -1.5, 126.5;
- K-split slabs built to cancel (B, -B, the value, ...): the order of the additions decides the result.
Every image, cache and table is pre-filled with a sentinel byte.  Rows with NaN or Inf, and blocks whose maximum is so small that -127 / max
overflows, are left out: the arithmetic there is undefined on both sides and no contract.  No case is a shape the hook ought to refuse."""
import functools

import numpy as np

M = 256
FILL = 0x5A             # every byte of the images before a launch: int8 90, f16 210.5 and a float near 1.5e16 — nothing a kernel writes here
TILE_FILL = 0x5A5A5A5A
ROUND_NONE, ROUND_F16, ROUND_BF16 = 0, 1, 2

# element pairs of a 256-block: lanes 0 and 31 (every shuffle distance at once), neighbouring chunks, chunks 1 and 2 (distance 1 after distance 2 ..),
# the two half-blocks, chunk 0 against chunk 31 off its first element, and two elements of one chunk
PAIRS = ((0, 255), (7, 8), (8, 16), (127, 128), (1, 248), (3, 5))
# (pair, sign of the FIRST element) -> (element that becomes -127, element that becomes +127, sign of d): the first element of largest magnitude is
# the extreme, iscale = -127 / it maps it to -127 and its mirror image to +127, and d = 1 / iscale has the sign opposite to the extreme's
TIE_EXPECT = {
    ((0, 255), +1): (0, 255, -1), ((0, 255), -1): (0, 255, +1),
    ((7, 8), +1): (7, 8, -1), ((7, 8), -1): (7, 8, +1),
    ((8, 16), +1): (8, 16, -1), ((8, 16), -1): (8, 16, +1),
    ((127, 128), +1): (127, 128, -1), ((127, 128), -1): (127, 128, +1),
    ((1, 248), +1): (1, 248, -1), ((1, 248), -1): (1, 248, +1),
    ((3, 5), +1): (3, 5, -1), ((3, 5), -1): (3, 5, +1),
}
# the exact block of QUANT: element -> (value, q); nearest with ties to even, 127 the cap
EXACT_BLOCK = {0: (-127.0, -127), 9: (0.5, 0), 10: (1.5, 2), 11: (2.5, 2), 40: (-0.5, 0), 41: (-1.5, -2), 200: (126.5, 126), 201: (127.0, 127), 202: (63.5, 64)}
KINDS = ["normal_1e-3", "normal_1", "normal_1e3"] + ["tie_%d_%d_%s" % (p[0], p[1], "pm"[s < 0]) for p in PAIRS for s in (+1, -1)] + \
        ["zero_block", "zero_row", "full_subblocks", "small_sums"]


def target_rows(K, nrows, seed, first=0, exact=False):
    """the values the image writer is to see, up to a positive factor per row: T [nrows][K] float32, crafted [nrows][K] bool (elements whose q reference B
    must decide), expect: list of (row, block, dict) hand-written results.  Row r is of kind KINDS[(first + r) % len] and no two rows are equal"""
    kinds = KINDS + (["exact_halves"] if exact else [])
    nb = K // 256
    T = np.zeros((nrows, K), np.float32)
    crafted = np.zeros((nrows, K), bool)
    expect = []
    for r in range(nrows):
        kind = kinds[(first + r) % len(kinds)]
        rng = np.random.default_rng([seed, r, K])
        base = rng.standard_normal(K).astype(np.float32)
        b = r % nb
        a = np.float32(3.0 + (r % 64) / 64.0 + r // 64)                   # above every |0.2 normal| of the row, different in every row
        lo = 256 * b
        if kind.startswith("normal"):
            T[r] = base * np.float32(float(kind.split("_")[1]))
            continue
        if kind == "zero_row":
            crafted[r] = True
            expect.append((r, None, dict(zero_row=True)))
            continue
        T[r] = np.clip(base * np.float32(0.2), -0.9 * a, 0.9 * a)
        if kind.startswith("tie"):
            _, i, j, s = kind.split("_")
            i, j, s = int(i), int(j), +1 if s == "p" else -1
            T[r, lo + i], T[r, lo + j] = s * a, -s * a
            crafted[r, [lo + i, lo + j]] = True
            m127, p127, dsign = TIE_EXPECT[((i, j), s)]
            expect.append((r, b, dict(q={m127: -127, p127: 127}, d_sign=dsign)))
        elif kind == "zero_block":
            zb = 1 + r % (nb - 2) if nb >= 3 else nb - 1                   # between two live blocks where the row has three
            T[r, 256 * zb:256 * zb + 256] = 0.0
            crafted[r, 256 * zb:256 * zb + 256] = True
            expect.append((r, zb, dict(zero_block=True)))
        elif kind == "full_subblocks":                                      # element 0 = -a is the extreme: iscale = 127 / a
            T[r, lo] = -a
            T[r, lo + 96:lo + 128] = a
            T[r, lo + 160:lo + 192] = -a
            crafted[r, lo] = True
            crafted[r, lo + 96:lo + 128] = crafted[r, lo + 160:lo + 192] = True
            expect.append((r, b, dict(q={0: -127, 96: 127, 127: 127, 160: -127, 191: -127}, sums={3: 4064, 5: -4064}, d_sign=+1)))
        elif kind == "small_sums":                                          # element 0 = +a is the extreme: q = -127 x / a, so x = -k a / 127 gives k
            unit = np.float64(a) / 127.0
            T[r, lo:lo + 256] = 0.0
            T[r, lo] = a
            T[r, lo + 32 + (r % 32)] = np.float32(unit)                     # q = -1, the sub-block's only live element
            T[r, lo + 64 + (r % 31)] = np.float32(-unit)                    # q = +1
            T[r, lo + 128 + 5] = np.float32(63 * unit)                      # q = -63
            T[r, lo + 224] = np.float32(-2 * unit)
            T[r, lo + 225] = np.float32(unit)                               # q = 2 - 1: an odd positive sum
            crafted[r, lo:lo + 256] = True
            expect.append((r, b, dict(q={0: -127, 32 + (r % 32): -1, 64 + (r % 31): 1, 133: -63}, sums={0: -127, 1: -1, 2: 1, 3: 0, 4: -63, 5: 0, 6: 0, 7: 1}, d_sign=-1)))
        elif kind == "exact_halves":
            T[r, lo:lo + 256] = 0.0
            sums = [0] * 8
            for e, (val, q) in EXACT_BLOCK.items():
                T[r, lo + e] = val
                sums[e // 32] += q
            crafted[r, lo:lo + 256] = True
            expect.append((r, b, dict(q={e: q for e, (_, q) in EXACT_BLOCK.items()}, sums=dict(enumerate(sums)), d_sign=+1, d=1.0)))
    return T, crafted, expect


def split_slabs(t, ks, seed, big=1e8):
    """ks float32 arrays [rows][cols] whose float32 sum in ascending order is t up to a few units in the last place, odd in t (a tie pair stays one) and
    exact where t is zero.  From three slabs on the first two are +-B with B far above the values: added in another order, or into x first, the
    value is lost"""
    t = np.asarray(t, np.float64)
    rng = np.random.default_rng([seed, ks, 77])
    rows = t.shape[0]
    if ks == 1:
        return [t.astype(np.float32)]
    out = []
    rest = t
    if ks >= 3:
        B = (big * (1.0 + rng.random((rows, 1)))).astype(np.float32) * np.ones(t.shape, np.float32)
        out += [B, -B]
    n_small = ks - len(out)
    for _ in range(n_small - 1):
        p = (rest * rng.uniform(-2.0, 2.0, (rows, 1))).astype(np.float32)
        out.append(p)
        rest = rest - p.astype(np.float64)
    out.append(rest.astype(np.float32))
    return out


def pack_slabs(slabs, n_total, seed):
    """partial [ks][M][n_total]: the slabs' rows and columns, seeded normal values everywhere else (rows past the pass's, columns past the slabs')"""
    ks = len(slabs)
    rows, cols = slabs[0].shape
    p = np.random.default_rng([seed, 5]).standard_normal((ks, M, n_total)).astype(np.float32) * np.float32(7.0)
    for s in range(ks):
        p[s, :rows, :cols] = slabs[s]
    return p.reshape(-1)


def image_case(name, op, K, nrows, **kw):
    c = dict(name=name, op=op, K=K, nrows=nrows, fill=FILL, x=None, partial=None, w=None, ks=1, n_total=0, eps=0.0, af_round=ROUND_NONE, want_af=False, crafted=None,
             expect=[], pv_part=None, l_part=None, n_head=0, head_dim=0)
    c.update(kw)
    return c


# ------------------------------------------------------------------------------------------ RMSNORM
def rmsnorm_case(D, nrows, ks, seed, n_total=None, eps=1e-5, af_round=ROUND_NONE, want_af=False, weights="signs", first=0):
    """x and the slabs are made so that x + slabs = T / w up to rounding: the norm then sees T times the row's scale.  weights "signs": +-1.5 with
    four zero entries in every block (columns 40 .. 43: no crafted element sits there), so ties and ratios survive the product; "normal": seeded
    normal weights, rows of the normal kinds only"""
    rng = np.random.default_rng([seed, D, 3])
    if weights == "signs":
        T, crafted, expect = target_rows(D, nrows, seed, first)
        w = np.where(rng.random(D) < 0.5, np.float32(-1.5), np.float32(1.5)).astype(np.float32)
        w[(np.arange(D) % 256 >= 40) & (np.arange(D) % 256 < 44)] = 0.0
        crafted[:, w == 0.0] = True                                         # q = 0 there whatever the row holds
        expect = [e for e in expect if not (e[2].get("q") and any(40 <= k < 44 for k in e[2]["q"]))]
    else:
        T = (np.random.default_rng([seed, D, 4]).standard_normal((nrows, D)) * np.array([1e-3, 1.0, 1e3])[np.arange(nrows) % 3][:, None]).astype(np.float32)
        crafted, expect = np.zeros((nrows, D), bool), []
        w = rng.standard_normal(D).astype(np.float32)
        w[::97] = 0.0
    X = np.where(w != 0.0, T.astype(np.float64) / np.where(w != 0.0, w, 1.0), T.astype(np.float64))
    xfull = np.random.default_rng([seed, D, 6]).standard_normal((M, D)).astype(np.float32)   # rows past nrows: must come back as they are
    partial = None
    nt = 0
    if ks is None:
        xfull[:nrows] = X.astype(np.float32)
        xfull[:nrows][:, 41::256] = np.float32(-0.0)                        # x + nothing must stay -0.0: the weight there is 0, q = 0 either way
    else:
        nt = n_total or D
        x0 = (X * rng.uniform(-1.5, 1.5, (nrows, 1))).astype(np.float32)
        xfull[:nrows] = x0
        partial = pack_slabs(split_slabs(X - x0.astype(np.float64), ks, seed), nt, seed)
    # values on rounding ties of f16 and bf16 in the rows (1 + 2^-11, 1 + 3 2^-11, 1 + 2^-8, 1 + 3 2^-8, and an f16 subnormal): where a row's scale is
    # a power of two they stay ties; everywhere they are values like any other
    if want_af and ks is None:
        for i, val in enumerate((1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 3 * 2.0 ** -25)):
            rows = np.flatnonzero(~crafted[:, 48 + i])
            xfull[rows, 48 + i] = np.float32(val)
    return image_case("rmsnorm_D%d_r%d_ks%s_%s%s" % (D, nrows, ks, weights, "_af%d" % af_round if want_af else ""), "rmsnorm", D, nrows, x=xfull.reshape(-1),
                      partial=partial, ks=ks or 1, n_total=nt, w=w, eps=eps, af_round=af_round, want_af=want_af, crafted=crafted, expect=expect)


@functools.lru_cache(maxsize=None)
def rmsnorm_cases():
    return [
        rmsnorm_case(256, 256, None, 11, af_round=ROUND_F16, want_af=True),
        rmsnorm_case(256, 33, 2, 12, af_round=ROUND_BF16, want_af=True, first=3),
        rmsnorm_case(256, 17, 1, 13, af_round=ROUND_NONE, want_af=True, first=9, n_total=512),
        rmsnorm_case(256, 1, 8, 14, first=4),
        rmsnorm_case(256, 2, 3, 15, first=15, eps=1e-6),
        rmsnorm_case(768, 16, 4, 16, n_total=1024),                         # 192 groups: the 256-thread workgroup, a quarter of it idle
        rmsnorm_case(768, 2, None, 17, first=17, eps=1e-6),
        rmsnorm_case(4096, 256, 7, 18),
        rmsnorm_case(4096, 17, None, 19, eps=1e-6, weights="normal"),
        rmsnorm_case(5120, 33, 2, 20, first=1),                             # 1280 groups: the workgroup clamped to 1024, two group passes
        rmsnorm_case(5120, 1, 5, 21, first=6),
        rmsnorm_case(8448, 3, 4, 22, first=3),                              # 1056 chunks: the second chunk pass and its reload of the weights
        rmsnorm_case(8448, 2, None, 23, first=16),
        rmsnorm_case(8448, 4, 6, 24, weights="normal"),
    ]


# ------------------------------------------------------------------------------------------ SWIGLU, QUANT, PV_JOIN
def swiglu_case(FF, nrows, ks, seed, first=0):
    """crafted rows: one gate per row, up = T / silu(gate), so silu(gate) * up is T and a tie pair stays one; then sweep rows: gates over [-90, 90] with
    +-0 among them against large seeded up values"""
    T, crafted, expect = target_rows(FF, nrows, seed, first)
    rng = np.random.default_rng([seed, FF, 8])
    g = np.repeat(rng.choice([1.5, -0.75, 4.0, 0.3, -2.5], nrows)[:, None], FF, axis=1)
    u = T.astype(np.float64) / (g / (1.0 + np.exp(-g)))
    sweep = [r for r in range(nrows) if r % 7 == 6 and not crafted[r].any()]
    for r in sweep:
        g[r] = np.linspace(-90.0, 90.0, FF) if r % 2 else rng.uniform(-12.0, 12.0, FF)
        g[r, 3], g[r, 4] = 0.0, -0.0
        u[r] = rng.standard_normal(FF) * 1e3
    slabs = split_slabs(np.concatenate([g, u], axis=1), ks, seed, big=1e10)
    return image_case("swiglu_FF%d_r%d_ks%d" % (FF, nrows, ks), "swiglu", FF, nrows, partial=pack_slabs(slabs, 2 * FF, seed), ks=ks, n_total=2 * FF, crafted=crafted,
                      expect=expect)


@functools.lru_cache(maxsize=None)
def swiglu_cases():
    return [swiglu_case(256, 256, 1, 31), swiglu_case(256, 17, 2, 32, first=2), swiglu_case(256, 1, 7, 33, first=5), swiglu_case(256, 33, 8, 34, first=8),
            swiglu_case(2304, 16, 1, 35, first=1), swiglu_case(2304, 2, 2, 36, first=13), swiglu_case(2304, 33, 7, 37), swiglu_case(2304, 17, 8, 38, first=11),
            swiglu_case(256, 2, 3, 39, first=18)]


def quant_case(FF, nrows, seed, first=0, af_round=ROUND_NONE, want_af=False):
    T, crafted, expect = target_rows(FF, nrows, seed, first, exact=True)
    if want_af:                                                             # exact input: values on the float types' rounding ties, in rows of the normal kinds
        ties = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 3 * 2.0 ** -25, 2.0 ** -25,
                         65519.99], np.float32)                               # the last: just below the f16 tie that rounds to infinity
        for r in range(nrows):
            if not crafted[r].any():
                T[r, 60:60 + len(ties)] = ties
    return image_case("quant_FF%d_r%d%s" % (FF, nrows, "_af%d" % af_round if want_af else ""), "quant", FF, nrows, x=T.reshape(-1), crafted=crafted, expect=expect,
                      af_round=af_round, want_af=want_af)


@functools.lru_cache(maxsize=None)
def quant_cases():
    return [quant_case(256, 1, 41, first=19), quant_case(256, 2, 42, first=3), quant_case(256, 16, 43), quant_case(256, 17, 44, first=4), quant_case(256, 33, 45),
            quant_case(256, 256, 46), quant_case(2304, 17, 47, first=7), quant_case(2304, 256, 48, first=2),
            quant_case(256, 33, 49, af_round=ROUND_F16, want_af=True), quant_case(256, 17, 50, af_round=ROUND_BF16, want_af=True, first=10),
            quant_case(512, 2, 51, af_round=ROUND_NONE, want_af=True)]


def pv_join_case(n_head, head_dim, nrows, seed, first=0):
    """the four classes' partial outputs are T times the class's share of the denominator, so the joined value is T; the shares are seeded, no powers of
    two, and the same for the heads of one 256-block (a tie pair may straddle two heads)"""
    K = n_head * head_dim
    T, crafted, expect = target_rows(K, nrows, seed, first)
    rng = np.random.default_rng([seed, K, 9])
    hpb = 256 // head_dim
    share = rng.uniform(0.3, 1.7, (nrows, n_head // hpb, 1, 4)).repeat(hpb, axis=2).reshape(nrows, n_head, 4).astype(np.float32)
    pv = (T.astype(np.float64).reshape(nrows, n_head, 1, head_dim) * share.astype(np.float64)[:, :, :, None]).astype(np.float32)
    return image_case("pv_join_h%d_d%d_r%d" % (n_head, head_dim, nrows), "pv_join", K, nrows, pv_part=pv.reshape(-1), l_part=share.reshape(-1), n_head=n_head,
                      head_dim=head_dim, crafted=crafted, expect=expect)


@functools.lru_cache(maxsize=None)
def pv_join_cases():
    return [pv_join_case(nh, hd, n, 60 + i, first=5 * i) for i, (nh, hd, n) in enumerate([(4, 64, 1), (4, 64, 8), (8, 64, 1), (8, 64, 8), (4, 128, 1), (4, 128, 8),
                                                                                          (8, 128, 1), (8, 128, 8)])]


def image_cases():
    return rmsnorm_cases() + swiglu_cases() + quant_cases() + pv_join_cases()


# ------------------------------------------------------------------------------------------ RESIDUAL_FOLD
def fold_case(D, n_total, ks, nrows, seed):
    rng = np.random.default_rng([seed, D])
    want = rng.standard_normal((nrows, D)) * np.array([1e-3, 1.0, 1e3])[np.arange(nrows) % 3][:, None]
    x = rng.standard_normal((M, D)).astype(np.float32)
    want[:, 5::64] = 0.0
    slabs = split_slabs(want - x[:nrows].astype(np.float64), ks, seed)
    return dict(name="fold_D%d_nt%d_ks%d_r%d" % (D, n_total, ks, nrows), op="fold", K=D, nrows=nrows, ks=ks, n_total=n_total, x=x.reshape(-1),
                partial=pack_slabs(slabs, n_total, seed))


@functools.lru_cache(maxsize=None)
def fold_cases():
    shapes = [(256, 256, 1), (256, 512, 17), (1280, 1280, 256), (1280, 1536, 1), (4096, 4096, 17), (4096, 4352, 1), (256, 256, 256), (1280, 1536, 17)]
    out = [fold_case(D, nt, ks, n, 70 + ks) for ks, (D, nt, n) in zip(range(1, 9), shapes)]
    return out + [fold_case(4096, 4352, 3, 256, 80), fold_case(256, 512, 8, 1, 81), fold_case(1280, 1280, 5, 17, 82)]


# ------------------------------------------------------------------------------------------ ROPE_APPEND
ROPE_ROWS = [(0, 0), (0, 1), (2, 7), (2, 0), (0, 7), (2, 1)]                # (sequence, position): several rows of each sequence, positions 0, 1 and 7 of 8
F16_TIES = (1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(2.0 + 2.0 ** -10), 2.0 ** -24 * 1.5, 2.0 ** -25, 1024.5, 2049.0, 65519.99)   # exact in float32, ties (or next to one) in f16


def rope_case(n_head, n_kv_head, head_dim, ks, layer, seed, pad=0):
    QD, KVD, half = n_head * head_dim, n_kv_head * head_dim, head_dim // 2
    n_layer, max_seq, max_ctx = 2, 3, 8
    nrows = len(ROPE_ROWS)
    rng = np.random.default_rng([seed, head_dim])
    want = rng.standard_normal((nrows, QD + 2 * KVD))
    want[:, QD + KVD:QD + KVD + len(F16_TIES)] = np.array(F16_TIES)[None, :] * np.where(np.arange(nrows) % 2, -1.0, 1.0)[:, None]   # V: no rotation, the sums are these values
    want[:, 7::50] = 0.0
    slabs = split_slabs(want.astype(np.float32), ks, seed, big=1e6)
    vt = slice(QD + KVD, QD + KVD + len(F16_TIES))                          # the ties exactly: B, -B, the value, zeros — every float32 sum is the value itself
    for s in range(ks):
        if s == (2 if ks >= 3 else 0):
            slabs[s][:, vt] = want[:, vt].astype(np.float32)
        elif ks < 3 or s >= 2:
            slabs[s][:, vt] = 0.0
    n_total = QD + 2 * KVD + pad
    cache = n_layer * max_seq * n_kv_head * max_ctx * head_dim
    seq, pos = np.array(ROPE_ROWS, np.int32).T
    return dict(name="rope_h%d_kv%d_d%d_ks%d_l%d" % (n_head, n_kv_head, head_dim, ks, layer), op="rope", nrows=nrows, ks=ks, n_total=n_total, n_head=n_head,
                n_kv_head=n_kv_head, head_dim=head_dim, n_layer=n_layer, max_seq=max_seq, max_ctx=max_ctx, layer=layer, seq=np.ascontiguousarray(seq),
                pos=np.ascontiguousarray(pos), partial=pack_slabs(slabs, n_total, seed),
                rope_cos=rng.uniform(-2.0, 2.0, max_ctx * half).astype(np.float32), rope_sin=rng.uniform(-2.0, 2.0, max_ctx * half).astype(np.float32),   # no unit circle
                qbuf=np.full(M * QD, np.float32(-7.5)), kcache=np.full(cache, 0x5A5A, np.uint16), vcache=np.full(cache, 0xA5A5, np.uint16))


@functools.lru_cache(maxsize=None)
def rope_cases():
    geo = [(4, 1, 64), (8, 2, 128), (4, 2, 128), (2, 2, 256), (4, 1, 192)]
    out = [rope_case(nh, nkv, hd, ks, i % 2, 90 + i, pad=64 * (i % 2)) for i, ((nh, nkv, hd), ks) in enumerate(zip(geo, (1, 3, 4, 8, 3)))]
    return out + [rope_case(4, 1, 64, 8, 1, 96), rope_case(8, 2, 128, 1, 0, 97, pad=256), rope_case(2, 2, 256, 2, 1, 98), rope_case(4, 1, 192, 4, 0, 99)]


# ------------------------------------------------------------------------------------------ ATT_TILES
def tiles_case(name, seq, expect=None):
    seq = np.asarray(seq, np.int32)
    return dict(name="tiles_" + name, op="tiles", nrows=len(seq), seq=seq, tiles=np.full(1 + M, TILE_FILL, np.int32), expect_tiles=expect)


def T_(first, rows):
    return first | (rows << 16)


@functools.lru_cache(maxsize=None)
def tiles_cases():
    rng = np.random.default_rng(5)
    return [
        tiles_case("one_row", [3], [T_(0, 1)]),
        tiles_case("15_of_one", [2] * 15, [T_(0, 15)]),
        tiles_case("16_of_one", [2] * 16, [T_(0, 16)]),
        tiles_case("17_of_one", [2] * 17, [T_(0, 16), T_(16, 1)]),
        tiles_case("256_of_one", [0] * 256, [T_(16 * i, 16) for i in range(16)]),
        tiles_case("runs_17_16_15_1", [4] * 17 + [1] * 16 + [9] * 15 + [0], [T_(0, 16), T_(16, 1), T_(17, 16), T_(33, 15), T_(48, 1)]),
        tiles_case("a_a_b_a", [5, 5, 7, 5], [T_(0, 2), T_(2, 1), T_(3, 1)]),
        tiles_case("a17_b_a17", [5] * 17 + [7] + [5] * 17, [T_(0, 16), T_(16, 1), T_(17, 1), T_(18, 16), T_(34, 1)]),
        tiles_case("256_ids", rng.permutation(256), [T_(i, 1) for i in range(256)]),
        tiles_case("seeded_runs", np.repeat(rng.integers(0, 4, 40), rng.integers(1, 20, 40))[:256]),
    ]


# ------------------------------------------------------------------------------------------ EMBED
def embed_types(tk):
    return [tk.TYPE_F32, tk.TYPE_F16, tk.TYPE_BF16, tk.TYPE_Q4_0, tk.TYPE_Q4_1, tk.TYPE_Q5_0, tk.TYPE_Q5_1, tk.TYPE_Q8_0, tk.TYPE_Q2_K, tk.TYPE_Q3_K, tk.TYPE_Q4_K,
            tk.TYPE_Q5_K, tk.TYPE_Q6_K, tk.TYPE_IQ4_NL, tk.TYPE_IQ4_XS, tk.TYPE_TQ1_0, tk.TYPE_TQ2_0]


EMBED_VOCAB = 64


def embed_tokens(nrows):
    """0, 63, repeats and a descending run, then seeded ids"""
    head = [0, 63, 63, 0, 7, 7, 7, 62, 61, 60, 59, 58, 1]
    rest = np.random.default_rng(nrows).integers(0, EMBED_VOCAB, max(0, nrows - len(head))).tolist()
    return np.array(([63] if nrows == 1 else head + rest)[:nrows], np.int32)


def embed_table(tk, ttype, D, seed=7):
    """(raw blocks of a 64-row table built with the project's own quantisers, bytes) for one token_embd type"""
    import bf16_ref
    w = (np.random.default_rng([seed, ttype, D]).standard_normal((EMBED_VOCAB, D)) * 0.05).astype(np.float32)
    if ttype in (tk.TYPE_F32, tk.TYPE_F16, tk.TYPE_BF16):
        return np.ascontiguousarray(bf16_ref.encode(ttype, w)).view(np.uint8).reshape(-1)
    return tk.quantize_blocks(ttype, w).reshape(-1)


def decode_table(tk, ttype, blocks, D):
    """[64][D] float32 through the NumPy decoder the type's own tests use"""
    import bf16_ref
    import iq4_ref
    import oracle_lib as O
    import q2k_ref
    import q3k_ref
    import q4_0_ref
    import q4_1_ref
    import q5k_ref
    import q8_0_ref
    import tq_ref
    b = np.asarray(blocks, np.uint8)
    if ttype == tk.TYPE_F32:
        return bf16_ref.decode(ttype, b.view(np.float32)).reshape(EMBED_VOCAB, D)
    if ttype in (tk.TYPE_F16, tk.TYPE_BF16):
        return bf16_ref.decode(ttype, b.view(np.uint16)).reshape(EMBED_VOCAB, D)
    if ttype in (tk.TYPE_Q4_0, tk.TYPE_Q5_0):
        v = q4_0_ref.dequant(ttype, b)
    elif ttype in (tk.TYPE_Q4_1, tk.TYPE_Q5_1):
        v = q4_1_ref.dequant(ttype, b)
    elif ttype == tk.TYPE_Q8_0:
        v = q8_0_ref.dequant(b)
    elif ttype == tk.TYPE_Q2_K:
        v = q2k_ref.dequant(b)
    elif ttype == tk.TYPE_Q3_K:
        v = q3k_ref.dequant(b)
    elif ttype == tk.TYPE_Q4_K:
        v = q5k_ref.dequant(q5k_ref.q4k_to_q5k(b))
    elif ttype == tk.TYPE_Q5_K:
        v = q5k_ref.dequant(b)
    elif ttype == tk.TYPE_Q6_K:
        v = O.dequant_rows(O.TYPE_Q6_K, b, EMBED_VOCAB, D)                  # no NumPy decoder of Q6_K in the suite: the oracle's
    elif ttype in (tk.TYPE_IQ4_NL, tk.TYPE_IQ4_XS):
        v = iq4_ref.dequant(ttype, b)
    else:
        v = tq_ref.dequant(ttype, b)
    return np.asarray(v, np.float32).reshape(EMBED_VOCAB, D)


def embed_cases(tk):
    out = []
    for i, ttype in enumerate(embed_types(tk)):
        for D in (256, 768):
            nrows = (1, 17, 256)[(i + D // 768) % 3]
            out.append(dict(name="embed_t%d_D%d_r%d" % (ttype, D, nrows), op="embed", type=ttype, K=D, vocab=EMBED_VOCAB, nrows=nrows, tok=embed_tokens(nrows),
                            x=np.full(nrows * D, np.float32(-7.5)), embd=embed_table(tk, ttype, D)))
    return out


# ------------------------------------------------------------------------------------------ the twins
TWIN_ROWS = 64          # weight rows of the twins' matrix: four 16-row tiles, the least a launch takes
Y_FILL = np.float32(-7.5)


def twin_matrix(ttype, rows, K, seed):
    """raw blocks of a seeded Q4_K (12) or Q6_K (14) matrix [rows][K], by the oracle's quantiser"""
    import oracle_lib as O
    return O.quantize_rows(ttype, (np.random.default_rng([seed, ttype, K]).standard_normal((rows, K)) * 0.05).astype(np.float32))


@functools.lru_cache(maxsize=None)
def fused_cases():
    """FUSED_NORM and FUSED_SWIGLU: nrows 1 and 2, K 512 and 1024, the mat-vec split 1 and 2 ways, the producer's slabs none (norm only), 1, 4, 8; the rows
    are the tie / zero-block / cancelling-slab rows of the stand-alone cases"""
    out = []
    i = 0
    for K in (512, 1024):
        for nrows in (1, 2):
            for ks in (1, 2):
                if K % (512 * ks):                                          # the fused form needs K % (512 ks) == 0: K = 512 runs with ks = 1 alone
                    continue
                for fks in (None, 1, 4, 8):
                    i += 1
                    ttype = (12, 14)[i % 2]
                    wb = twin_matrix(ttype, TWIN_ROWS, K, 200 + i)
                    y = np.full(ks * M * TWIN_ROWS, Y_FILL)
                    n = rmsnorm_case(K, nrows, fks, 300 + i, first=3 * i, n_total=K + 256 * (i % 2) if fks else None)
                    out.append(dict(n, name="fused_norm_K%d_r%d_ks%d_fks%s_t%d" % (K, nrows, ks, fks, ttype), twin="norm", gemv_ks=ks, fks=fks or 0, wtype=ttype, wblocks=wb,
                                    y=y, x_b=np.full(M * K, Y_FILL)))
                    if fks:
                        g = swiglu_case(K, nrows, fks, 400 + i, first=3 * i + 1)
                        out.append(dict(g, name="fused_swiglu_K%d_r%d_ks%d_fks%d_t%d" % (K, nrows, ks, fks, ttype), twin="swiglu", gemv_ks=ks, fks=fks, wtype=ttype,
                                        wblocks=wb, y=y))
    return out


@functools.lru_cache(maxsize=None)
def wide_cases():
    out = []
    for i, (nrows, ttype) in enumerate(((193, 12), (256, 14), (256, 12), (193, 14))):
        D = FF = 256
        x = target_rows(D, nrows, 500 + i, first=i)[0]
        out.append(dict(name="wide_swiglu_r%d_t%d" % (nrows, ttype), twin="wide", op="wide", K=D, wrows=FF, nrows=nrows, wtype=ttype, x=x.reshape(-1), fill=FILL,
                        wblocks=twin_matrix(ttype, 2 * FF, D, 600 + i)))
    return out


def twin_kwargs(tk, c):
    if c["twin"] == "wide":
        return tk.STEP_WIDE_SWIGLU, dict(K=c["K"], wrows=c["wrows"], nrows=c["nrows"], wtype=c["wtype"], x=c["x"], wblocks=c["wblocks"], image_fill=c["fill"])
    kw = dict(K=c["K"], nrows=c["nrows"], ks=c["gemv_ks"], fks=c["fks"], wtype=c["wtype"], wrows=TWIN_ROWS, wblocks=c["wblocks"], y_a=c["y"], y_b=c["y"])
    if c["twin"] == "norm":
        kw.update(x=c["x"], x_b=c["x_b"], w=c["w"], eps=c["eps"])
        if c["partial"] is not None:
            kw.update(partial=c["partial"], n_total=c["n_total"])
        return tk.STEP_FUSED_NORM, kw
    kw.update(partial=c["partial"])
    return tk.STEP_FUSED_SWIGLU, kw


# ------------------------------------------------------------------------------------------ the hook's arguments
def probe_kwargs(tk, c):
    """the keyword arguments of tk.llm_step_probe for a case"""
    op = c["op"]
    if op in ("rmsnorm", "swiglu", "quant", "pv_join"):
        kw = dict(K=c["K"], nrows=c["nrows"], af_round=c["af_round"], image_fill=c["fill"], want_af=c["want_af"])
        if op == "rmsnorm":
            kw.update(x=c["x"], w=c["w"], eps=c["eps"])
            if c["partial"] is not None:
                kw.update(partial=c["partial"], ks=c["ks"], n_total=c["n_total"])
        elif op == "swiglu":
            kw.update(partial=c["partial"], ks=c["ks"])
        elif op == "quant":
            kw.update(x=c["x"])
        else:
            kw.update(pv_part=c["pv_part"], l_part=c["l_part"], n_head=c["n_head"], head_dim=c["head_dim"])
        return {"rmsnorm": tk.STEP_RMSNORM, "swiglu": tk.STEP_SWIGLU, "quant": tk.STEP_QUANT, "pv_join": tk.STEP_PV_JOIN}[op], kw
    if op == "fold":
        return tk.STEP_RESIDUAL_FOLD, dict(K=c["K"], nrows=c["nrows"], ks=c["ks"], n_total=c["n_total"], x=c["x"], partial=c["partial"])
    if op == "rope":
        return tk.STEP_ROPE_APPEND, {k: c[k] for k in ("nrows", "ks", "n_total", "n_head", "n_kv_head", "head_dim", "n_layer", "max_seq", "max_ctx", "layer", "seq", "pos",
                                                       "partial", "rope_cos", "rope_sin", "qbuf", "kcache", "vcache")}
    if op == "tiles":
        return tk.STEP_ATT_TILES, dict(nrows=c["nrows"], seq=c["seq"], tiles=c["tiles"])
    return tk.STEP_EMBED, dict(K=c["K"], nrows=c["nrows"], type=c["type"], vocab=c["vocab"], tok=c["tok"], x=c["x"], embd=c["embd"])


def refusals(tk):
    """(refused, accepted): (name, op, keyword arguments) the hook must refuse with TK_ERROR_INVALID_ARGUMENT before anything is launched, and their
    accepted neighbours.  device = -1 answers both without a device"""
    q = quant_case(256, 2, 1)
    op_q, kw_q = probe_kwargs(tk, q)
    n = rmsnorm_case(256, 2, 2, 2)
    op_n, kw_n = probe_kwargs(tk, n)
    r = rope_case(4, 1, 64, 1, 0, 3)
    op_r, kw_r = probe_kwargs(tk, r)
    t = tiles_cases()[0]
    op_t, kw_t = probe_kwargs(tk, t)
    f = fold_case(256, 256, 2, 2, 4)
    op_f, kw_f = probe_kwargs(tk, f)
    e = dict(K=256, nrows=2, type=tk.TYPE_Q4_K, vocab=4, tok=np.array([0, 3], np.int32), x=np.zeros(512, np.float32), embd=np.zeros(4 * 144, np.uint8))
    big = 16384                                                             # a d_model whose norm row is past the 64 KiB every kernel has unasked
    wide = dict(K=big, nrows=1, x=np.zeros(M * big, np.float32), w=np.ones(big, np.float32), eps=1e-5, image_fill=0)
    too_wide = dict(K=40960, nrows=1, x=np.zeros(M * 40960, np.float32), w=np.ones(40960, np.float32), eps=1e-5, image_fill=0)

    def but(kw, **ch):
        o = dict(kw)
        o.update(ch)
        return o
    refused = [
        ("nrows 0", op_q, but(kw_q, nrows=0)), ("nrows 257", op_q, but(kw_q, nrows=257)), ("K 0", op_q, but(kw_q, K=0)), ("K 384", op_q, but(kw_q, K=384)),
        ("x too short", op_q, but(kw_q, x=q["x"][:-1])), ("x NULL", op_q, but(kw_q, x=None)), ("af_round 3", op_q, but(kw_q, af_round=3)),
        ("rounding without af", op_q, but(kw_q, af_round=1, want_af=False, af=None)), ("aq too short", op_q, but(kw_q, aq=np.zeros(M * 256 - 1, np.int8))),
        ("ks 0", op_n, but(kw_n, ks=0)), ("ks 9", op_n, but(kw_n, ks=9)), ("partial too short", op_n, but(kw_n, partial=n["partial"][:-1])),
        ("n_total below K", op_n, but(kw_n, n_total=252)), ("w NULL", op_n, but(kw_n, w=None)), ("w too short", op_n, but(kw_n, w=n["w"][:-1])),
        ("norm row above the LDS opt-in", tk.STEP_RMSNORM, too_wide),
        ("fold ks 9", op_f, but(kw_f, ks=9)), ("fold n_total % 4", op_f, but(kw_f, n_total=258)), ("fold x short", op_f, but(kw_f, x=f["x"][:-1])),
        ("grp 3", op_r, but(kw_r, n_head=3)), ("head_dim 96", op_r, but(kw_r, head_dim=96)), ("n_kv_head 0", op_r, but(kw_r, n_kv_head=0)),
        ("layer 2", op_r, but(kw_r, layer=2)), ("layer -1", op_r, but(kw_r, layer=-1)), ("seq 3", op_r, but(kw_r, seq=np.array([0, 0, 3, 2, 0, 2], np.int32))),
        ("pos 8", op_r, but(kw_r, pos=np.array([0, 1, 8, 0, 7, 1], np.int32))), ("pos -1", op_r, but(kw_r, pos=np.array([0, -1, 7, 0, 7, 1], np.int32))),
        ("cache short", op_r, but(kw_r, kcache=r["kcache"][:-1])), ("rope table short", op_r, but(kw_r, rope_sin=r["rope_sin"][:-1])),
        ("rope n_total small", op_r, but(kw_r, n_total=kw_r["n_total"] - 4)), ("seq short", op_r, but(kw_r, seq=r["seq"][:-1])),
        ("tiles short", op_t, but(kw_t, tiles=np.zeros(M, np.int32))), ("tiles no seq", op_t, but(kw_t, seq=None)),
        ("embed type 99", tk.STEP_EMBED, but(e, type=99)), ("embed type Q8_K", tk.STEP_EMBED, but(e, type=15)), ("embed tok 4", tk.STEP_EMBED, but(e, tok=np.array([0, 4], np.int32))),
        ("embed tok -1", tk.STEP_EMBED, but(e, tok=np.array([-1, 0], np.int32))), ("embed table short", tk.STEP_EMBED, but(e, embd=np.zeros(4 * 144 - 1, np.uint8))),
        ("pv_join head_dim 96", tk.STEP_PV_JOIN, dict(K=384, nrows=1, n_head=4, head_dim=96, pv_part=np.zeros(4 * 4 * 96, np.float32), l_part=np.ones(16, np.float32), image_fill=0)),
        ("pv_join K mismatch", tk.STEP_PV_JOIN, dict(K=512, nrows=1, n_head=4, head_dim=64, pv_part=np.zeros(4 * 4 * 64, np.float32), l_part=np.ones(16, np.float32), image_fill=0)),
        ("unknown op", 99, kw_q),
    ]
    fn, fs, wd = fused_cases()[0], [c for c in fused_cases() if c["twin"] == "swiglu"][0], wide_cases()[0]
    (op_fn, kw_fn), (op_fs, kw_fs), (op_wd, kw_wd) = twin_kwargs(tk, fn), twin_kwargs(tk, fs), twin_kwargs(tk, wd)
    k8 = 8192                                                               # 16 K + K / 16 + K of image and (K + 4) floats of row: 174 096 bytes, past the 160 KiB opt-in
    refused += [
        ("fused norm 3 rows", op_fn, but(kw_fn, nrows=3)), ("fused norm ks 3 of K 512", op_fn, but(kw_fn, ks=3)), ("fused norm wtype Q5_K", op_fn, but(kw_fn, wtype=13)),
        ("fused norm wrows 48", op_fn, but(kw_fn, wrows=48)), ("fused norm y short", op_fn, but(kw_fn, y_b=fn["y"][:-1])), ("fused norm no x_b", op_fn, but(kw_fn, x_b=None)),
        ("fused norm matrix short", op_fn, but(kw_fn, wblocks=fn["wblocks"][:-1])),
        ("fused norm image above the LDS opt-in", op_fn, dict(K=k8, nrows=1, ks=1, fks=0, wtype=12, wrows=64, wblocks=np.zeros(64 * 32 * 144, np.uint8),
                                                              y_a=np.zeros(M * 64, np.float32), y_b=np.zeros(M * 64, np.float32), x=np.zeros(M * k8, np.float32),
                                                              x_b=np.zeros(M * k8, np.float32), w=np.ones(k8, np.float32), eps=1e-5)),
        ("fused swiglu fks 0", op_fs, but(kw_fs, fks=0)), ("fused swiglu fks 9", op_fs, but(kw_fs, fks=9)), ("fused swiglu slabs short", op_fs, but(kw_fs, partial=fs["partial"][:-1])),
        ("wide 192 rows", op_wd, but(kw_wd, nrows=192, x=wd["x"][:192 * 256])), ("wide wrows 64", op_wd, but(kw_wd, wrows=64)), ("wide matrix short", op_wd, but(kw_wd, wblocks=wd["wblocks"][:-1])),
        ("wide with a float image", op_wd, but(kw_wd, af=np.zeros(M * 256, np.float32))),
    ]
    accepted = [("quant", op_q, kw_q), ("rmsnorm", op_n, kw_n), ("rope", op_r, kw_r), ("tiles", op_t, kw_t), ("fold", op_f, kw_f), ("embed", tk.STEP_EMBED, e),
                ("norm row of d_model 16384", tk.STEP_RMSNORM, wide), ("fused norm", op_fn, kw_fn), ("fused swiglu", op_fs, kw_fs), ("wide swiglu", op_wd, kw_wd)]
    return refused, accepted
