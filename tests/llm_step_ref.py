"""Reference B of tests/test_llm_step_gpu.py: the LLM stream's step kernels restated in NumPy, float64, from the comments of
csrc/llm/tk_llm_layout.h and above the kernels of csrc/llm/tk_llm_kernels.hip (not from quantize_chunk8 or the oracle's source).

Two parts.  The DECODERS turn the five raw images of a Q8 activation (aq, ad, abs as 64 h + l, abs16 as 2 hh + ll, af) back into [rows][K]
arrays, by reshaping; the ENCODER writes the same images from index arithmetic (tests/test_llm_step_cpu.py holds the two against each other).
The OPERATIONS give, per launch, everything the launch leaves behind.  Integer results (q, sub-block sums, the extreme element and its sign, tile
tables, cache placement) are decisions; on elements a case does not mark as crafted the reference abstains where its own float64 iscale * x lies
within MARGIN of a half-integer.  K-split slabs are added in float32, one rounded addition after the other in the documented order: an IEEE
addition is a decision too, and with slabs built to cancel the order IS the result.

mut: a tuple of mutation switches, each one a plausible kernel error; tests/test_llm_step_cpu.py shows every one changes some GPU case."""
import numpy as np

M = 256                 # tk_mi355x_llm_max_rows(): rows of a pass, 16 M-tiles of 16 slots
EPS = 2.0 ** -24        # one float32 rounding, relative
# iscale = -127 / max and iscale * x are two float32 roundings on top of the value's own error (norm or SwiGLU chain: about 1e-5 relative at the
# outside, see ad_rel_bound); times |iscale * x| <= 127 that is 1.3e-3 absolute around a half-integer.  About 0.3 % of normal values fall inside
MARGIN = 1.3e-3
# tk_divf is an IEEE division (half an ulp); tk_sqrtf documents 1 ulp; tk_siluf = x * (1 / (1 + tk_expf(-x))): tk_expf's 2^-22, one addition, one
# division, one product: 2^-22 + 3 x 2^-24 < 2^-21 of silu(x), and where tk_expf clamps its argument (|x| > 87) the result is below 1e-35 in
# magnitude on both sides.  tests/test_llm_step_cpu.py measures the three against float64 on every run
DIVF_REL_ERR = 2.0 ** -24
SQRTF_REL_ERR = 2.0 ** -23
SILUF_REL_ERR = 2.0 ** -21
SILUF_ABS_ERR = 1e-35

MUTATIONS = (
    "tie_last", "tie_high_lane", "sign_lost", "round_half_away", "bsum_trunc", "abs_images_swapped", "slot_tile_mix",   # the Q8 image writer
    "slabs_descending", "slab_into_x_first", "slab_pitch_nrows", "fold_writes_x_without_slabs",                         # the K-split slabs
    "norm_weight_chunk0", "mean_over_ngrp", "af_round_none",                                                            # the norm
    "rope_cos_sin_swapped", "rope_half_split", "rope_on_v", "cache_pos_major",                                          # q / k / v
    "tiles_len_off_by_one", "tiles_run_not_reset", "embed_block_of_next_row")


# ------------------------------------------------------------------------------------------ the images
def decode_aq(aq, K):
    """int8 [M-tile][K / 64][4 g][16 slot][2 sub-blocks][8] -> [M][K]: k = 64 j + 32 sub-block + 8 g + t"""
    a = np.asarray(aq, np.int8).reshape(M // 16, K // 64, 4, 16, 2, 8)
    return a.transpose(0, 3, 1, 4, 2, 5).reshape(M, K)


def decode_ad(ad, K):
    """float [M-tile][K / 256][16] -> [M][K / 256]"""
    return np.asarray(ad, np.float32).reshape(M // 16, K // 256, 16).transpose(0, 2, 1).reshape(M, K // 256)


def _split_images(img, K):
    a = np.asarray(img).reshape(M // 16, K // 256, 2, 16, 8)
    return [a[:, :, i].transpose(0, 2, 1, 3).reshape(M, K // 32) for i in (0, 1)]


def decode_abs(abs_, K):
    """int8 [M-tile][K / 256][2][16][8], image 0 = l, image 1 = h -> (sums = 64 h + l, l, h), each [M][K / 32]"""
    lo, hi = _split_images(np.asarray(abs_, np.int8), K)
    return 64 * hi.astype(np.int64) + lo.astype(np.int64), lo, hi


def decode_abs16(abs16, K):
    """f16 bits, the same shape: image 0 = hh, image 1 = ll -> (sums = 2 hh + ll, hh, ll) as float64"""
    hh, ll = _split_images(np.asarray(abs16, np.uint16).view(np.float16), K)
    return 2.0 * hh.astype(np.float64) + ll.astype(np.float64), hh, ll


def decode_af(af, K):
    """float [M-tile][K / 16][4 g][16 rows][4 t], k = 16 j + 4 t + g -> [M][K]"""
    a = np.asarray(af, np.float32).reshape(M // 16, K // 16, 4, 16, 4)
    return a.transpose(0, 3, 1, 4, 2).reshape(M, K)


def encode_image(K, nrows, fill, q, d, sums, af=None, mut=()):
    """the raw images a launch of nrows rows leaves in buffers that held the byte `fill` everywhere: q [nrows][K] ints, d [nrows][K / 256] float32,
    sums [nrows][K / 32] ints, af [nrows][K] float32 or None -> dict(aq, ad, abs, abs16, af).  Written from the offsets the layout comment gives"""
    out = dict(aq=np.full(M * K, fill, np.uint8).view(np.int8), ad=np.full(K * 4, fill, np.uint8).view(np.float32),
               abs=np.full(M // 16 * K, fill, np.uint8).view(np.int8), abs16=np.full(M // 16 * K * 2, fill, np.uint8).view(np.uint16),
               af=None if af is None else np.full(M * K * 4, fill, np.uint8).view(np.float32))
    r = np.arange(nrows)
    mt, sl = (r % 16, r // 16) if "slot_tile_mix" in mut else (r // 16, r % 16)
    k = np.arange(K)
    out["aq"][(mt[:, None] * (K * 16) + (k // 64 * 1024 + (k % 32 // 8 * 16) * 16 + k % 64 // 32 * 8 + k % 8)[None, :] + sl[:, None] * 16)] = np.asarray(q, np.int8)
    b = np.arange(K // 256)
    out["ad"][mt[:, None] * (K // 256 * 16) + b[None, :] * 16 + sl[:, None]] = np.asarray(d, np.float32)
    s = np.asarray(sums, np.int64)
    if "bsum_trunc" in mut:                                                 # C's / and %: toward zero
        h6, h1 = np.trunc(s / 64).astype(np.int64), np.trunc(s / 2).astype(np.int64)
    else:                                                                   # arithmetic shifts: toward minus infinity, so l and ll are never negative
        h6, h1 = s >> 6, s >> 1
    lo, ll = s - 64 * h6, s - 2 * h1
    j = np.arange(K // 32)
    at = mt[:, None] * K + (j // 8 * 256 + j % 8)[None, :] + sl[:, None] * 8
    i_first, i_second = (128, 0) if "abs_images_swapped" in mut else (0, 128)
    out["abs"][at + i_first] = lo.astype(np.int8)
    out["abs"][at + i_second] = h6.astype(np.int8)
    out["abs16"][at + i_first] = h1.astype(np.float16).view(np.uint16)
    out["abs16"][at + i_second] = ll.astype(np.float16).view(np.uint16)
    if af is not None:
        out["af"][mt[:, None] * (16 * K) + (k // 16 * 256 + k % 4 * 64 + k % 16 // 4)[None, :] + sl[:, None] * 4] = np.asarray(af, np.float32)
    return out


# ------------------------------------------------------------------------------------------ the Q8 image of a row
def q8_reference(v, crafted=None, mut=()):
    """v [rows][K] float64, the values a kernel quantises -> dict(q, d, sums, first (index of the extreme element per block), abstain [rows][K]).
    Per 256-block: the signed value of the FIRST element of largest magnitude, iscale = -127 / it, q = min(127, nearest(iscale x)) with ties to
    even, d = 1 / iscale; an all-zero block has d = 0 and q = 0"""
    v = np.asarray(v, np.float64)
    rows, K = v.shape
    blk = v.reshape(rows, K // 256, 256)
    a = np.abs(blk)
    amax = a.max(axis=2)
    first = a.argmax(axis=2)
    if "tie_last" in mut:
        first = 255 - a[:, :, ::-1].argmax(axis=2)
    if "tie_high_lane" in mut:                                              # the highest 8-element chunk that holds a maximum, its first maximum
        is_max = a == amax[:, :, None]
        chunk = 31 - is_max.reshape(rows, K // 256, 32, 8).any(axis=3)[:, :, ::-1].argmax(axis=2)
        inside = np.take_along_axis(is_max.reshape(rows, K // 256, 32, 8), chunk[:, :, None, None], axis=2)[:, :, 0]
        first = 8 * chunk + inside.argmax(axis=2)
    mval = np.take_along_axis(blk, first[:, :, None], axis=2)[:, :, 0]
    if "sign_lost" in mut:
        mval = amax
    live = amax > 0
    iscale = np.where(live, -127.0 / np.where(live, mval, 1.0), 0.0)
    t = iscale[:, :, None] * blk
    q = np.sign(t) * np.floor(np.abs(t) + 0.5) if "round_half_away" in mut else np.rint(t)
    q = np.minimum(q, 127).astype(np.int64)
    near_half = np.abs(np.abs(t - np.floor(t)) - 0.5) < MARGIN
    abstain = near_half.reshape(rows, K)
    if crafted is not None:
        abstain = abstain & ~np.asarray(crafted, bool)
    return dict(q=q.reshape(rows, K), d=np.where(live, 1.0 / np.where(live, iscale, 1.0), 0.0), sums=q.reshape(rows, K // 32, 32).sum(axis=2), first=first,
                abstain=abstain)


def round_reference(v, mode):
    """float64 -> the nearest f16 (1) / bf16 (2) value, ties to even, as float64; 0: as it is"""
    v = np.asarray(v, np.float64)
    if mode == 1:
        return v.astype(np.float16).astype(np.float64)
    if mode == 2:
        e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -126)))
        ulp = 2.0 ** (e - 7)
        return np.rint(v / ulp) * ulp
    return v


def round_bound(v, mode, rel):
    """|kernel af - float64 v| for a value known to `rel`: half a unit of the float type at v (f16 below 2^-14: half of 2^-24), plus the value's own error"""
    av = np.abs(np.asarray(v, np.float64))
    own = rel * av
    if mode == 1:
        return 1.01 * (own + np.maximum(av * 2.0 ** -11, 2.0 ** -25))
    if mode == 2:
        return 1.01 * (own + av * 2.0 ** -8) + 1e-45
    return 1.01 * own + 1e-45


# ------------------------------------------------------------------------------------------ K-split slabs
def slab_sum32(partial, ks, n_total, nrows, cols, mut=(), x=None):
    """float32 [nrows][cols]: slabs 0 .. ks - 1 of partial [ks][M][n_total] added one rounded addition after the other, ascending, starting from
    slab 0; with x [nrows][cols]: x + (that sum)"""
    p = np.asarray(partial, np.float32).reshape(-1)
    pitch = (nrows if "slab_pitch_nrows" in mut else M) * n_total
    r = np.arange(nrows)[:, None] * n_total + np.arange(cols)[None, :]
    slabs = [p[np.minimum(s * pitch + r, p.size - 1)] for s in range(ks)]
    if "slabs_descending" in mut:
        slabs = slabs[::-1]
    if x is not None and "slab_into_x_first" in mut:
        o = np.asarray(x, np.float32)
        for s in slabs:
            o = o + s
        return o
    o = slabs[0]
    for s in slabs[1:]:
        o = o + s
    return o if x is None else np.asarray(x, np.float32) + o


def fold_bound(x, partial, ks, n_total, nrows, cols):
    """(float64 value of x + sum of the slabs, bound of the float32 chain: ks rounded additions of partial results no larger than the sum of magnitudes)"""
    p = np.asarray(partial, np.float64).reshape(ks, M, n_total)[:, :nrows, :cols]
    x = np.asarray(x, np.float64)
    return x + p.sum(axis=0), 1.01 * EPS * ks * (np.abs(x) + np.abs(p).sum(axis=0)) + 1e-45


# ------------------------------------------------------------------------------------------ the operations
def norm_threads(D):
    """threads of a norm workgroup: one per 16-byte group of the row, rounded up to 256 .. 1024"""
    return min(1024, max(256, (D // 4 + 255) // 256 * 256))


def ref_rmsnorm(c, mut=()):
    D, nrows = c["K"], c["nrows"]
    x0 = np.asarray(c["x"], np.float32).reshape(M, D)
    x_out = x0.copy()
    if c["partial"] is not None:
        h = slab_sum32(c["partial"], c["ks"], c["n_total"], nrows, D, mut, x=x0[:nrows])
        x_out[:nrows] = h
    else:
        h = x0[:nrows]
        if "fold_writes_x_without_slabs" in mut:
            x_out[:nrows] = h + np.float32(0.0)                             # -0.0 comes back as +0.0
    h64 = h.astype(np.float64)
    mean = (h64 * h64).sum(axis=1) / (D // 4 if "mean_over_ngrp" in mut else D)
    scale = 1.0 / np.sqrt(mean + float(np.float32(c["eps"])))
    w = np.asarray(c["w"], np.float64)
    if "norm_weight_chunk0" in mut:                                          # a thread's second chunk keeps the weights of its first
        k = np.arange(D)
        w = w[k // 8 % norm_threads(D) * 8 + k % 8]
    v = h64 * scale[:, None] * w[None, :]
    out = q8_reference(v, c.get("crafted"), mut)
    out.update(v=v, x=x_out, rel=ad_rel_bound("rmsnorm", D))
    return out


def ref_swiglu(c, mut=()):
    FF, nrows = c["K"], c["nrows"]
    gu = slab_sum32(c["partial"], c["ks"], 2 * FF, nrows, 2 * FF, mut).astype(np.float64)
    g, u = gu[:, :FF], gu[:, FF:]
    with np.errstate(over="ignore"):
        v = g / (1.0 + np.exp(-g)) * u
    out = q8_reference(v, c.get("crafted"), mut)
    out.update(v=v, rel=ad_rel_bound("swiglu", FF), v_abs=SILUF_ABS_ERR * np.abs(u))
    return out


def ref_quant(c, mut=()):
    v = np.asarray(c["x"], np.float64).reshape(c["nrows"], c["K"])
    out = q8_reference(v, c.get("crafted"), mut)
    out.update(v=v, rel=ad_rel_bound("quant", c["K"]))
    return out


def ref_pv_join(c, mut=()):
    nrows, nh, hd = c["nrows"], c["n_head"], c["head_dim"]
    pv = np.asarray(c["pv_part"], np.float64).reshape(nrows, nh, 4, hd)
    lp = np.asarray(c["l_part"], np.float64).reshape(nrows, nh, 4)
    v = (pv.sum(axis=2) / lp.sum(axis=2)[:, :, None]).reshape(nrows, nh * hd)
    out = q8_reference(v, c.get("crafted"), mut)
    out.update(v=v, rel=ad_rel_bound("pv_join", c["K"]))
    return out


def ad_rel_bound(op, K):
    """relative error of the float32 value a kernel quantises against this module's float64 one, first order.  d = 1 / (-127 / max) adds two divisions
    (ad_bound).  rmsnorm: the sum of squares is 256 chains of K / 256 fmas, a 6-level butterfly and 3 joins of non-negative terms, each rounding
    once; the mean one division, + eps one addition; the square root halves that and adds tk_sqrtf's own error; 1 / it one division; (h * scale) * w two
    products.  swiglu: tk_siluf and one product (the slab sums are exact: they are added in float32 here too).  pv_join: three additions each of
    same-signed parts above and below, one division.  quant: the input itself"""
    if op == "rmsnorm":
        return 0.5 * ((K // 256 + 6 + 3) * EPS + 2 * EPS) + SQRTF_REL_ERR + DIVF_REL_ERR + 2 * EPS
    if op == "swiglu":
        return SILUF_REL_ERR + EPS
    if op == "pv_join":
        return 6 * EPS + DIVF_REL_ERR
    return 0.0


def ad_bound(d, rel):
    return 1.01 * np.abs(d) * (rel + 2 * DIVF_REL_ERR) + 1e-45


def ref_residual_fold(c, mut=()):
    D, nrows = c["K"], c["nrows"]
    x = np.asarray(c["x"], np.float32).reshape(M, D).copy()
    x[:nrows] = slab_sum32(c["partial"], c["ks"], c["n_total"], nrows, D, mut, x=x[:nrows])
    return dict(x=x)


def cache_index(c, layer, seq, kvh, pos, mut=()):
    """halves in front of the row of (layer, sequence, KV head, position): [n_layer][max_seq][n_kv_head][max_ctx][head_dim]"""
    if "cache_pos_major" in mut:
        return (((layer * c["max_seq"] + seq) * c["max_ctx"] + pos) * c["n_kv_head"] + kvh) * c["head_dim"]
    return (((layer * c["max_seq"] + seq) * c["n_kv_head"] + kvh) * c["max_ctx"] + pos) * c["head_dim"]


def ref_rope_append(c, mut=()):
    """-> dict(q [nrows][QD] float64 and its bound, k [nrows][KVD] float64 and its bound, v [nrows][KVD] float32 (exact), at [nrows][n_kv_head]: the
    cache offset of each row's halves)"""
    nrows, nh, nkv, hd = c["nrows"], c["n_head"], c["n_kv_head"], c["head_dim"]
    QD, KVD, half = nh * hd, nkv * hd, hd // 2
    s = slab_sum32(c["partial"], c["ks"], c["n_total"], nrows, QD + 2 * KVD, mut)
    cs = np.asarray(c["rope_cos"], np.float64).reshape(c["max_ctx"], half)[np.asarray(c["pos"])]
    sn = np.asarray(c["rope_sin"], np.float64).reshape(c["max_ctx"], half)[np.asarray(c["pos"])]
    if "rope_cos_sin_swapped" in mut:
        cs, sn = sn, cs

    def rope(z, heads):
        z = z.astype(np.float64).reshape(nrows, heads, hd)
        if "rope_half_split" in mut:
            a, b = z[:, :, :half], z[:, :, half:]
        else:
            a, b = z[:, :, 0::2], z[:, :, 1::2]
        o0, o1 = a * cs[:, None, :] - b * sn[:, None, :], a * sn[:, None, :] + b * cs[:, None, :]
        # fma(-b, sn, a * cs): the product a * cs is rounded, then the sum: EPS of each; the same for the other half
        e0 = 1.01 * EPS * (np.abs(a * cs[:, None, :]) + np.abs(o0)) + 1e-45
        e1 = 1.01 * EPS * (np.abs(b * cs[:, None, :]) + np.abs(o1)) + 1e-45
        out, err = np.empty_like(z), np.empty_like(z)
        if "rope_half_split" in mut:
            out[:, :, :half], out[:, :, half:], err[:, :, :half], err[:, :, half:] = o0, o1, e0, e1
        else:
            out[:, :, 0::2], out[:, :, 1::2], err[:, :, 0::2], err[:, :, 1::2] = o0, o1, e0, e1
        return out.reshape(nrows, heads * hd), err.reshape(nrows, heads * hd)

    q, q_err = rope(s[:, :QD], nh)
    k, k_err = rope(s[:, QD:QD + KVD], nkv)
    v = s[:, QD + KVD:]
    if "rope_on_v" in mut:
        v = rope(v, nkv)[0].astype(np.float32)
    at = np.array([[cache_index(c, c["layer"], int(c["seq"][r]), h, int(c["pos"][r]), mut) for h in range(nkv)] for r in range(nrows)], np.int64)
    return dict(q=q, q_err=q_err, k=k, k_err=k_err, v=v, at=at)


def f16_decide(v, err):
    """float64 values known to +-err -> (f16 bits of the nearest, abstain where the interval reaches a rounding tie, i.e. both ends round differently)"""
    lo, hi = (v - err).astype(np.float16), (v + err).astype(np.float16)
    return v.astype(np.float16).view(np.uint16), lo.view(np.uint16) != hi.view(np.uint16)


def expected_caches(c, r, k_bits, v_bits):
    """both caches as the launch leaves them: the caller's content, and the rows' halves at their places"""
    kc, vc = np.array(c["kcache"], np.uint16).reshape(-1), np.array(c["vcache"], np.uint16).reshape(-1)
    hd, nkv = c["head_dim"], c["n_kv_head"]
    for row in range(c["nrows"]):
        for h in range(nkv):
            a = r["at"][row, h]
            kc[a:a + hd] = k_bits[row, h * hd:(h + 1) * hd]
            vc[a:a + hd] = v_bits[row, h * hd:(h + 1) * hd]
    return kc, vc


def ref_att_tiles(c, mut=()):
    """tiles [1 + M] as the launch leaves it: [0] = number of tiles, then per tile first row | rows << 16: a tile is up to 16 consecutive rows of one
    run of equal sequence ids, a new one every 16 rows of the run; entries past the count keep the caller's content"""
    seq, nrows = [int(v) for v in c["seq"]], c["nrows"]
    tiles = np.array(c["tiles"], np.int32).copy()
    run0, first_of = [], {}
    for t in range(nrows):
        if t == 0 or seq[t] != seq[t - 1]:
            start = first_of.get(seq[t], t) if "tiles_run_not_reset" in mut else t
            first_of.setdefault(seq[t], t)
        run0.append(start)
    n = 0
    for t in range(nrows):
        if (t - run0[t]) % 16 == 0:
            ln = 1
            while ln < 16 and t + ln < nrows and seq[t + ln] == seq[t]:
                ln += 1
            if "tiles_len_off_by_one" in mut:
                ln -= 1
            n += 1
            tiles[n] = t | (ln << 16)
    tiles[0] = n
    return dict(tiles=tiles)


def ref_embed(c, table, mut=()):
    """table [vocab][K]: the type's own NumPy decoder's values (tests/llm_step_cases.py: decode_table) -> x [nrows][K]"""
    tok = np.asarray(c["tok"], np.int64)
    if "embed_block_of_next_row" in mut:
        tok = (tok + 1) % c["vocab"]
    return dict(x=np.asarray(table, np.float32)[tok])


REF = {"rmsnorm": ref_rmsnorm, "swiglu": ref_swiglu, "quant": ref_quant, "pv_join": ref_pv_join}


def ref_image_launch(c, mut=()):
    """an image op's launch, whole: the decoded results and the raw images (and x for the norm) as reference B expects them"""
    r = REF[c["op"]](c, mut)
    mode = c.get("af_round", 0)
    if c.get("want_af"):
        r["af"] = r["v"] if "af_round_none" in mut else round_reference(r["v"], mode)
    r["raw"] = encode_image(c["K"], c["nrows"], c["fill"], r["q"], r["d"].astype(np.float32), r["sums"], r["af"].astype(np.float32) if c.get("want_af") else None, mut)
    return r


# ------------------------------------------------------------------------------------------ reference A: the oracle, launch by launch
def oracle_image_launch(c):
    """what orc_rmsnorm / orc_swiglu / orc_divf / orc_slab_sum / orc_q8k_quantize / orc_round_through make of a case: dict(q, d, sums, v, x, af, raw)"""
    import oracle_lib as O
    op, nrows, K = c["op"], c["nrows"], c["K"]
    v = np.empty((nrows, K), np.float32)
    x_out = None
    if op == "rmsnorm":
        x_out = np.array(c["x"], np.float32).reshape(M, K)
        for r in range(nrows):
            if c["partial"] is not None:
                x_out[r] = x_out[r] + O.slab_sum(c["partial"][r * c["n_total"]:], c["ks"], M * c["n_total"], K)
            v[r] = O.rmsnorm(x_out[r], c["w"], c["eps"])
    elif op == "swiglu":
        for r in range(nrows):
            gu = O.slab_sum(c["partial"][r * 2 * K:], c["ks"], M * 2 * K, 2 * K)
            v[r] = O.swiglu(gu[:K], gu[K:])
    elif op == "quant":
        v[:] = np.asarray(c["x"], np.float32).reshape(nrows, K)
    else:
        nh, hd = c["n_head"], c["head_dim"]
        for r in range(nrows):
            for h in range(nh):
                a = O.slab_sum(c["pv_part"][(r * nh + h) * 4 * hd:], 4, hd, hd)
                ll = O.slab_sum(c["l_part"][(r * nh + h) * 4:], 4, 1, 1)
                v[r, h * hd:(h + 1) * hd] = O.divf(a, np.repeat(ll, hd))
    q, d, sums = np.empty((nrows, K), np.int8), np.empty((nrows, K // 256), np.float32), np.empty((nrows, K // 32), np.int32)
    for r in range(nrows):
        q[r], d[r], sums[r] = O.q8k_quantize(v[r])
    af = O.round_through(v, c["af_round"]) if c.get("want_af") else None
    return dict(q=q, d=d, sums=sums, v=v, x=x_out, af=af, raw=encode_image(K, nrows, c["fill"], q, d, sums, af))


def oracle_fold_launch(c):
    import oracle_lib as O
    x = np.array(c["x"], np.float32).reshape(M, c["K"])
    for r in range(c["nrows"]):
        x[r] = x[r] + O.slab_sum(c["partial"][r * c["n_total"]:], c["ks"], M * c["n_total"], c["K"])
    return dict(x=x)


def oracle_rope_launch(c):
    """-> dict(qbuf [M][QD] with the caller's content past nrows, kcache, vcache whole)"""
    import oracle_lib as O
    nrows, nh, nkv, hd = c["nrows"], c["n_head"], c["n_kv_head"], c["head_dim"]
    QD, KVD, half = nh * hd, nkv * hd, hd // 2
    qbuf = np.array(c["qbuf"], np.float32).reshape(M, QD)
    kb, vb = np.empty((nrows, KVD), np.uint16), np.empty((nrows, KVD), np.uint16)
    cos, sin = np.asarray(c["rope_cos"], np.float32).reshape(-1, half), np.asarray(c["rope_sin"], np.float32).reshape(-1, half)
    for r in range(nrows):
        s = O.slab_sum(c["partial"][r * c["n_total"]:], c["ks"], M * c["n_total"], QD + 2 * KVD)
        cs, sn = cos[c["pos"][r]], sin[c["pos"][r]]
        qbuf[r] = O.rope_pairs(s[:QD], np.tile(cs, nh), np.tile(sn, nh)).reshape(-1)
        kb[r] = O.f32_to_f16(O.rope_pairs(s[QD:QD + KVD], np.tile(cs, nkv), np.tile(sn, nkv)).reshape(-1))
        vb[r] = O.f32_to_f16(s[QD + KVD:])
    at = np.array([[cache_index(c, c["layer"], int(c["seq"][r]), h, int(c["pos"][r])) for h in range(nkv)] for r in range(nrows)], np.int64)
    kc, vc = expected_caches(c, dict(at=at), kb, vb)
    return dict(qbuf=qbuf, kcache=kc, vcache=vc)


# ------------------------------------------------------------------------------------------ the checks both test files make of a launch's results
def check_expectations(c, q, d, sums):
    """the hand-written results of the crafted rows: q [nrows][K], d [nrows][K / 256], sums [nrows][K / 32]"""
    n = 0
    for r, b, e in c["expect"]:
        if e.get("zero_row"):
            assert not q[r].any() and not d[r].any() and not sums[r].any(), (c["name"], r)
        elif e.get("zero_block"):
            assert not q[r, 256 * b:256 * b + 256].any() and d[r, b] == 0.0 and not sums[r, 8 * b:8 * b + 8].any(), (c["name"], r, b)
            assert all(d[r, o] != 0.0 for o in range(d.shape[1]) if o != b), (c["name"], r, "the live blocks")
        else:
            for k, want in e["q"].items():
                assert q[r, 256 * b + k] == want, (c["name"], r, b, k, int(q[r, 256 * b + k]), want)
            for j, want in e.get("sums", {}).items():
                assert sums[r, 8 * b + j] == want, (c["name"], r, b, j, int(sums[r, 8 * b + j]), want)
            assert np.sign(d[r, b]) == e["d_sign"], (c["name"], r, b, float(d[r, b]))
            if "d" in e:
                assert d[r, b] == e["d"]
        n += 1
    return n


def compare_with_b(c, b, q, d, sums, af, x, worst):
    """decoded results of a launch (the oracle's or a kernel's) against reference B; worst: op -> quantity -> (error / bound, case)"""
    nrows = c["nrows"]
    decided = ~b["abstain"]
    assert np.array_equal(np.asarray(q, np.int64)[decided], b["q"][decided]), (c["name"], np.argwhere(np.asarray(q, np.int64) != np.where(decided, b["q"], q))[:5])
    quiet = ~b["abstain"].reshape(nrows, -1, 32).any(axis=2)                # sub-blocks with no abstention: their sums are decided too
    assert np.array_equal(np.asarray(sums, np.int64)[quiet], b["sums"][quiet]), c["name"]
    frac = b["abstain"].mean()
    assert frac <= 0.01, (c["name"], frac)
    if c["crafted"] is not None:
        assert not (b["abstain"] & c["crafted"]).any()

    def note(what, err, bound):
        ratio = float((err / bound).max())
        assert ratio <= 1.0, (c["name"], what, ratio, np.argwhere(err > bound)[:5])
        if ratio > worst.setdefault(c["op"], {}).get(what, (-1.0, ""))[0]:
            worst[c["op"]][what] = (ratio, c["name"])
    note("ad", np.abs(np.asarray(d, np.float64) - b["d"]), ad_bound(b["d"], b["rel"]) + 127.0 ** -1 * b.get("v_abs", np.zeros(1)).max())
    if af is not None:
        own = b["rel"] * np.abs(b["v"]) + (b["v_abs"] if "v_abs" in b else 0.0)    # the value's own error: where it cannot move the rounding, af is decided
        sure = round_reference(b["v"] - own, c["af_round"]) == round_reference(b["v"] + own, c["af_round"])
        if c["af_round"] != 0:
            assert np.array_equal(np.asarray(af, np.float64)[sure], b["af"][sure]) and sure.mean() >= 0.99, (c["name"], "af", sure.mean())
        note("af", np.abs(np.asarray(af, np.float64) - b["v"]), round_bound(b["v"], c["af_round"], b["rel"]) + (b["v_abs"] if "v_abs" in b else 0.0))
    if x is not None:
        assert np.array_equal(np.asarray(x, np.float32).view(np.uint32), b["x"].view(np.uint32)), c["name"]
        if c["partial"] is not None:
            want, bound = fold_bound(np.asarray(c["x"]).reshape(M, -1)[:nrows], c["partial"], c["ks"], c["n_total"], nrows, c["K"])
            note("x", np.abs(np.asarray(x, np.float64)[:nrows] - want), bound)
    return frac


def print_worst(worst):
    for op in sorted(worst):
        print("%s: worst error / bound: %s" % (op, ", ".join("%s %.3f (%s)" % (k, v[0], v[1]) for k, v in sorted(worst[op].items()))))


def compare_rope(c, b, qbuf, kcache, vcache, worst):
    nrows, QD = c["nrows"], c["n_head"] * c["head_dim"]
    q = np.asarray(qbuf, np.float32).reshape(M, QD)
    assert np.array_equal(q[nrows:], np.asarray(c["qbuf"]).reshape(M, QD)[nrows:]), c["name"]
    ratio = float((np.abs(q[:nrows].astype(np.float64) - b["q"]) / b["q_err"]).max())
    assert ratio <= 1.0, (c["name"], "qbuf", ratio)
    if ratio > worst.setdefault("rope", {}).get("qbuf", (-1.0, ""))[0]:
        worst["rope"]["qbuf"] = (ratio, c["name"])
    k_bits, k_abstain = f16_decide(b["k"], b["k_err"])
    assert k_abstain.mean() <= 0.01, (c["name"], k_abstain.mean())
    v_bits = b["v"].astype(np.float16).view(np.uint16)
    got_k, got_v = np.asarray(kcache, np.uint16).reshape(-1), np.asarray(vcache, np.uint16).reshape(-1)
    kc, vc = expected_caches(c, b, np.where(k_abstain, 0, k_bits), v_bits)
    hd = c["head_dim"]
    for r in range(nrows):                                                  # where B abstains on a key half, take the launch's own
        for h in range(c["n_kv_head"]):
            a = b["at"][r, h]
            m = k_abstain[r, h * hd:(h + 1) * hd]
            kc[a:a + hd][m] = got_k[a:a + hd][m]
    assert np.array_equal(got_k, kc), (c["name"], "kcache", np.flatnonzero(got_k != kc)[:8])
    assert np.array_equal(got_v, vc), (c["name"], "vcache", np.flatnonzero(got_v != vc)[:8])
