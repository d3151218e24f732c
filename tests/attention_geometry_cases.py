"""The passes of tests/test_attention_geometry_gpu.py, shared with tests/test_attention_geometry_cpu.py: every head geometry TkLlmModel::init accepts,
at the pass widths, context lengths and session windows at which the attention launcher takes another kernel or instantiation.

Every model has one layer, d_model = d_ff = 256, 512 tokens and the automatic K-split plan: only the head geometry and the window vary, so the
W4A8 side stays trivial and the oracle cheap.  A CASE names one launch class — a (geometry, kind, width / shape / top position, environment) —
and the instantiation it claims to reach on a 256-CU device, written out by hand (PLAN columns below) from tk_attention_plan as it reads today;
the GPU test asks the launcher itself (tk_mi355x_attention_plan / _plan_at) and asserts the two agree.  A case is one or several PASSES (passes
narrower than the list of context lengths repeat with a shifted assignment until every length has been seen); a pass is compared with OracleLlm:
logits as uint32, ids, and every cache row the pass may or may not touch.

Nothing is generated at import: cases() lists light descriptors, passes(case) and kv_rows() make the arrays on demand, from the case's seed.

Plan tuples are (kernel, query heads per workgroup, positions per ring slot, slots); kernel 0 = k_attention<GQ, FUSED, HD, CH> (HD = head_dim when
it is 64 or 128, else 0: the run-time head_dim instantiation), 1 = k_attention_narrow, 2 = k_attention_prefill<head_dim>, 3 = the long-context trio
k_att_scores_long / k_att_pv_chain / k_att_pv_join.  None in a plan = not claimed (the narrow kernel's resident chunk follows the window)."""
import functools

import numpy as np

MODEL = dict(n_layer=1, d_model=256, d_ff=256, vocab=512)
RING, NARROW, PREFILL, LONG = 0, 1, 2, 3
K_SCALE, V_SCALE = 0.6, 1.0      # keys scaled so that the scores spread over several units: a softmax neither flat nor one-hot
POOL = 1031                      # positions in a geometry's K / V pool (a prime: sequences start at different offsets and never line up)
DECODE_SEQS = 257                # sequences of a decode session: 256 rows of a pass and one bystander behind the last of them

# name -> (n_head, n_kv_head, head_dim): the smallest geometries that reach every branch of tk_attention_plan on 256 CUs
GEOMETRIES = {
    "g4_d64": (32, 8, 64),       # 8 KV heads: 256 rows are 2048 workgroups (32-position slots); prefill<64>, long<64>
    "g2_d128": (16, 8, 128),     # a native group of 2: narrow with grp 2, <2, *, 128, 128 | 64 | 32>, prefill<128> and long<128> with grp 2
    "g1_d256": (8, 8, 256),      # group 1 exists only from head_dim 256: <1, *, 0, 64 | 32>
    "g2_d256": (8, 4, 256),      # <2, *, 0, 64>
    "g2_d256_6kv": (12, 6, 256), # the same group with 6 KV heads: from 171 rows more than 4 * 256 workgroups, <2, *, 0, 32>
    "g4_d256": (24, 6, 256),     # group 4 halved to gq = 2 at few rows, <4, *, 0, 64>, <4, *, 0, 32>
    "g4_d192": (8, 2, 192),      # 24 16-byte pieces per key row: not a power of two (att_swizzle_mask)
}

# fused decode passes: width -> plan, TK_MI355X_NO_NARROW_ATT=0 (narrow wherever it applies).  1, 2 and 16 rows, both sides of every
# threshold of the geometry (workgroups = n_head / gq * rows against 4 * 256; the halving of group 4 below 2 * 256 / n_kv_head rows; the narrow
# kernel's n_head / 2 * rows <= 256), 200 and 256 rows
DECODE_PLAN = {
    "g4_d64": {1: (RING, 4, 64, 2), 2: (RING, 4, 64, 2), 16: (RING, 4, 64, 2), 128: (RING, 4, 64, 2), 129: (RING, 4, 32, 2), 200: (RING, 4, 32, 2),
               256: (RING, 4, 32, 2)},
    "g2_d128": {1: (NARROW, 2, None, 1), 2: (NARROW, 2, None, 1), 16: (NARROW, 2, None, 1), 32: (NARROW, 2, None, 1), 33: (RING, 2, 64, 2),
                64: (RING, 2, 64, 2), 128: (RING, 2, 64, 2), 129: (RING, 2, 32, 2), 200: (RING, 2, 32, 2), 256: (RING, 2, 32, 2)},
    "g1_d256": {1: (RING, 1, 64, 2), 2: (RING, 1, 64, 2), 16: (RING, 1, 64, 2), 128: (RING, 1, 64, 2), 129: (RING, 1, 32, 2), 200: (RING, 1, 32, 2),
                256: (RING, 1, 32, 2)},
    "g2_d256": {1: (RING, 2, 64, 2), 2: (RING, 2, 64, 2), 16: (RING, 2, 64, 2), 200: (RING, 2, 64, 2), 256: (RING, 2, 64, 2)},
    "g2_d256_6kv": {1: (RING, 2, 64, 2), 2: (RING, 2, 64, 2), 16: (RING, 2, 64, 2), 170: (RING, 2, 64, 2), 171: (RING, 2, 32, 2), 200: (RING, 2, 32, 2),
                    256: (RING, 2, 32, 2)},
    "g4_d256": {1: (RING, 2, 64, 2), 2: (RING, 2, 64, 2), 16: (RING, 2, 64, 2), 85: (RING, 2, 64, 2), 86: (RING, 4, 64, 2), 170: (RING, 4, 64, 2),
                171: (RING, 4, 32, 2), 200: (RING, 4, 32, 2), 256: (RING, 4, 32, 2)},
    "g4_d192": {1: (RING, 4, 64, 2), 2: (RING, 4, 64, 2), 16: (RING, 4, 64, 2), 200: (RING, 4, 64, 2), 256: (RING, 4, 64, 2)},
}
# the same under TK_MI355X_NO_NARROW_ATT=1 where that changes the answer: k_attention<2, fused, 128, 128> (at most one workgroup per CU)
DECODE_PLAN_RING_ONLY = {"g2_d128": {1: (RING, 2, 128, 2), 2: (RING, 2, 128, 2), 16: (RING, 2, 128, 2), 32: (RING, 2, 128, 2)}}

# a window that is no multiple of 4: with a run-time head_dim q, the wave maxima and the row's own key lie BEHIND the [window][gq] score array,
# so their 16-byte reads start at window * gq * 4 bytes — 4 or 8 bytes off a 16-byte boundary here
ODD_WINDOW = 261
ODD_WIDTHS = (2, 200)

# cached positions of a decode row (= its position): the list of test_attention_wide_gpu.py, 191 .. 193 and 255 .. 257 (a third and a fourth
# 64-position slot begin), 129 (the first row of a second 128-position slot), and the window's last position
LENGTHS = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 190, 191, 192, 193, 255, 256, 257]
WINDOWS = {260: LENGTHS + [259], 520: LENGTHS + [383, 384, 385, 511], ODD_WINDOW: LENGTHS + [260]}
# passes of more than 8 rows in the wide window also reach its end (narrower ones would take the long-context form there: LONG_CASES has those)
WIDE_ONLY = {260: [], 520: [512, 513, 519], ODD_WINDOW: []}

# unfused passes (several new positions of a sequence in one pass, k_qkv_rope_append first): (sequences, new positions each) -> (gq, slot) of the
# k_attention<GQ, unfused, HD, CH> the plan names; below position 128 that is what runs, from there k_attention_prefill where it applies
UNFUSED_STARTS = [0, 31, 97, 159]
UNFUSED_PLAN = {
    "g4_d64": {(4, 8): (4, 64), (5, 12): (4, 64), (8, 32): (4, 32)},
    "g2_d128": {(4, 8): (2, 128), (5, 12): (2, 64), (8, 32): (2, 32)},
    "g1_d256": {(4, 8): (1, 64), (5, 12): (1, 64), (8, 32): (1, 32)},
    "g2_d256": {(4, 8): (2, 64), (5, 12): (2, 64), (8, 32): (2, 64)},
    "g2_d256_6kv": {(4, 8): (2, 64), (5, 12): (2, 64), (8, 32): (2, 32)},
    "g4_d256": {(4, 8): (2, 64), (10, 12): (4, 64), (8, 32): (4, 32)},
    "g4_d192": {(4, 8): (4, 64), (5, 12): (4, 64), (8, 32): (4, 64)},
}
PREFILL_GEOMETRIES = ("g4_d64", "g2_d128")     # head_dim 64 / 128 with the group a multiple of 256 / head_dim
PREFILL_FROM = 128                             # top position from which a multi-position pass is tiled

# the long-context form: (rows, top position) -> taken?  1 .. 4 rows from position 512, 5 .. 8 rows from 768; window 1024
LONG_GEOMETRIES = ("g4_d64", "g2_d128")
LONG_WINDOW = 1024
LONG_CASES = {(rows, top): top >= (768 if rows > 4 else 512) for rows in (1, 4, 5, 8) for top in (511, 512, 767, 768, 1000)}
LONG_DELTAS = [0, 1, 63, 64, 65, 200, 300, 511]  # row i of a long pass sits this far below the top position
LONG_ROWS_SEEN = 16
# what runs instead (TK_MI355X_NO_LONG_ATT=1, and below the thresholds)
LONG_FALLBACK = {"g4_d64": (RING, 4, 64, 2), "g2_d128": (NARROW, 2, None, 1)}
# where the long form does not apply the ring walks the whole context: 16 to 32 slots of 64 positions
DEEP_GEOMETRIES = {"g1_d256": (RING, 1, 64, 2), "g4_d256": (RING, 2, 64, 2)}
DEEP_CASES = [(1, 700), (1, 1000), (3, 1000)]


def hd_class(geometry):
    hd = GEOMETRIES[geometry][2]
    return hd if hd in (64, 128) else 0


def instantiation(geometry, plan, fused):
    """the name of what a plan runs, for messages and the coverage list"""
    kernel, gq, chunk, _ = plan
    hd = GEOMETRIES[geometry][2]
    if kernel == NARROW:
        return "k_attention_narrow(grp %d)" % (GEOMETRIES[geometry][0] // GEOMETRIES[geometry][1])
    if kernel == PREFILL:
        return "k_attention_prefill<%d>" % hd
    if kernel == LONG:
        return "k_att_scores_long<%d> + k_att_pv_chain<%d> + k_att_pv_join<%d>" % (hd, hd, hd)
    return "k_attention<%d, %s, %d, %d>" % (gq, "fused" if fused else "unfused", hd_class(geometry), chunk)


def _case(geometry, kind, name, window, plan, fused=True, env=None, twin=None, **kw):
    """twin: the case whose passes this one repeats under another environment (same seed, so the very same rows through another kernel)"""
    passes_of = twin or name
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate("%s/%s" % (geometry, passes_of)))
    return dict(geometry=geometry, kind=kind, name=name, window=window, plan=plan, fused=fused, env=env or {}, seed=seed, passes_of=passes_of, **kw)


@functools.lru_cache(maxsize=None)
def cases(geometry):
    """every case of one geometry, as descriptors; the group of a case is (geometry, kind)"""
    out = []
    for window in WINDOWS:
        for width, plan in DECODE_PLAN[geometry].items():
            if window == ODD_WINDOW and width not in ODD_WIDTHS:
                continue
            out.append(_case(geometry, "decode_w%d" % window, "w%d_rows%d" % (window, width), window, plan, width=width))
    for width, plan in DECODE_PLAN_RING_ONLY.get(geometry, {}).items():
        out.append(_case(geometry, "decode_ring_only", "w260_rows%d_ring" % width, 260, plan, width=width, twin="w260_rows%d" % width, env={"TK_MI355X_NO_NARROW_ATT": "1"}))
    for start in UNFUSED_STARTS:
        for shape, (gq, chunk) in UNFUSED_PLAN[geometry].items():
            tiled = geometry in PREFILL_GEOMETRIES and start + shape[1] - 1 >= PREFILL_FROM
            out.append(_case(geometry, "unfused", "from%d_%dx%d" % (start, shape[0], shape[1]), 260, (PREFILL if tiled else RING, gq, chunk, 2), fused=False,
                             shape=shape, start=start))
    for shape, (gq, chunk) in UNFUSED_PLAN[geometry].items():   # the one-workgroup-per-row form where the tiled one would run
        out.append(_case(geometry, "unfused_per_row", "from159_%dx%d_per_row" % shape, 260, (RING, gq, chunk, 2), fused=False, shape=shape, start=159, twin="from159_%dx%d" % shape,
                         env={"TK_MI355X_NO_PREFILL_ATT": "1"}))
    if geometry in LONG_GEOMETRIES:
        grp = GEOMETRIES[geometry][0] // GEOMETRIES[geometry][1]
        for (rows, top), taken in LONG_CASES.items():
            out.append(_case(geometry, "long", "rows%d_top%d" % (rows, top), LONG_WINDOW, (LONG, grp, 64, 1) if taken else LONG_FALLBACK[geometry], rows=rows, top=top))
            if taken:
                out.append(_case(geometry, "long_fused", "rows%d_top%d_fused" % (rows, top), LONG_WINDOW, LONG_FALLBACK[geometry], rows=rows, top=top, twin="rows%d_top%d" % (rows, top),
                                 env={"TK_MI355X_NO_LONG_ATT": "1"}))
    if geometry in DEEP_GEOMETRIES:
        for rows, top in DEEP_CASES:
            out.append(_case(geometry, "deep", "rows%d_top%d" % (rows, top), LONG_WINDOW, DEEP_GEOMETRIES[geometry], rows=rows, top=top))
    return out


def groups(geometry):
    """kind -> cases, in table order"""
    out = {}
    for c in cases(geometry):
        out.setdefault(c["kind"], []).append(c)
    return out


def max_seq(case):
    return DECODE_SEQS if case["kind"].startswith("decode") else 16


@functools.lru_cache(maxsize=None)
def kv_pool(geometry):
    """f16 bits of POOL seeded key and value rows [POOL][n_kv_head][head_dim]; a sequence's cached rows are a run of it (kv_rows)"""
    _, nkv, hd = GEOMETRIES[geometry]
    rng = np.random.default_rng([17, nkv, hd])
    k = (rng.standard_normal((POOL, nkv, hd), dtype=np.float32) * np.float32(K_SCALE)).astype(np.float16).view(np.uint16)
    v = (rng.standard_normal((POOL, nkv, hd), dtype=np.float32) * np.float32(V_SCALE)).astype(np.float16).view(np.uint16)
    k.setflags(write=False)
    v.setflags(write=False)
    return k, v


def kv_rows(geometry, offset, n):
    """rows offset .. offset + n - 1 (mod POOL) of the pool"""
    k, v = kv_pool(geometry)
    idx = (offset + np.arange(n)) % POOL
    return k[idx], v[idx]


def _preload(window, seq, cached, salt):
    """what a sequence holds before the pass: `cached` positions and two more (the appended row overwrites the first of them, the second must
    survive), as (first pool row, count)"""
    return (seq * 53 + salt * 7) % POOL, min(cached + 2, window)


def passes(case):
    """the passes of a case: dicts of seq, pos, tok (int32 arrays), preload {sequence: (pool offset, rows)} and bystander (a sequence outside the
    pass whose whole window is loaded and must not change), top = the highest position"""
    vocab = MODEL["vocab"]
    rng = np.random.default_rng(case["seed"])
    window = case["window"]
    out = []

    def add(seq, pos, pre_cached, bystander):
        seq, pos = np.asarray(seq, np.int32), np.asarray(pos, np.int32)
        tok = rng.integers(3, vocab, seq.size).astype(np.int32)
        salt = len(out)
        preload = {int(s): _preload(window, int(s), int(c), salt) for s, c in pre_cached.items()}
        out.append(dict(seq=seq, pos=pos, tok=tok, preload=preload, bystander=bystander, top=int(pos.max())))

    if case["kind"].startswith("decode"):
        w = case["width"]
        lengths = WINDOWS[window] + (WIDE_ONLY[window] if w > 8 else [])
        n = len(lengths)
        for j in range(1 if w >= n else -(-n // w)):
            pos = [lengths[(i + j * w + w) % n] for i in range(w)]
            add(np.arange(w), pos, dict(enumerate(pos)), w)
    elif case["kind"].startswith("unfused"):
        nseq, npos = case["shape"]
        start = case["start"]
        seq = np.repeat(np.arange(nseq), npos)
        pos = np.tile(np.arange(start, start + npos), nseq)
        # the runs' last position is the first row the pass must leave alone: preload through it
        add(seq, pos, {s: start + npos - 1 for s in range(nseq)}, nseq)
    else:  # long, long_fused, deep: one row per sequence, row 0 at the top and the others LONG_DELTAS below it.  The pass repeats over other
        # cache rows and tokens until the case has LONG_ROWS_SEEN rows: one row over 1000 positions seldom moves a q or a block scale of its Q8
        # image under a reordered sum, and a case must be able to show that (test_attention_geometry_cpu.py)
        rows, top = case["rows"], case["top"]
        for j in range(-(-LONG_ROWS_SEEN // rows)):
            pos = [top] + [top - LONG_DELTAS[(i + j) % len(LONG_DELTAS)] for i in range(1, rows)]
            add(np.arange(rows), pos, dict(enumerate(pos)), rows)
    return out


def sub_pass(case, p, limit=16):
    """rows of pass `p` that stand for it where only the oracle runs: the first `limit` rows of a decode pass (rows of different sequences do not
    see each other), every row of the first sequences of a multi-position pass up to `limit` rows at least"""
    n = p["seq"].size
    if n <= limit:
        keep = np.arange(n)
    elif case["fused"]:
        keep = np.arange(limit)
    else:
        keep = np.flatnonzero(p["seq"] <= p["seq"][limit - 1])
    seqs = {int(s) for s in p["seq"][keep]}
    return dict(p, seq=p["seq"][keep], pos=p["pos"][keep], tok=p["tok"][keep], preload={s: v for s, v in p["preload"].items() if s in seqs})


def swizzle_mask(head_dim):
    """att_swizzle_mask of tk_llm_kernels.hip: the largest power of two that divides the key row's head_dim / 8 pieces, less one"""
    ppr = head_dim // 8
    return (ppr & -ppr) - 1


def accepted_head_dims():
    """head_dim values some (n_head, n_kv_head) passes TkLlmModel::init with: multiples of 64 up to 256 whose group of 1, 2 or 4 heads fills 256s"""
    return [hd for hd in range(64, 257, 64) if any((grp * hd) % 256 == 0 for grp in (1, 2, 4))]
