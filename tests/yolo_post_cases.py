"""The launches of tests/test_yolo_post_gpu.py, shared with tests/test_yolo_post_cpu.py: one tk_mi355x_detector_post_probe call each.

A case: name, kind (0: three raw head maps, 1: a graph's decoded [4 + nc][anchors] output), B, nc, conf, iou, n_anchors and
  kind 0: in_w, in_h, ld (three pitches), heads (three float32 arrays [B][H_i W_i][ld_i])
  kind 1: out float32 [B][4 + nc][n_anchors]
random: frames reference B may abstain on (everything else is crafted: boxes on an integer grid, scores that are binary fractions);
expect: per frame, hand-derived dict(n_cand=, kept=[anchor ids], order_head=[first anchor ids]) — any subset."""
import functools

import numpy as np

import oracle_lib as O

CONF, IOU = 0.25, 0.5


def grid_box(i, size=2, pitch=4, per_row=64):
    """disjoint boxes on an integer grid"""
    x, y = pitch * (i % per_row), pitch * (i // per_row)
    return (x, y, x + size, y + size)


def frame_out(n, nc, items):
    """one kind-1 frame: items = [(anchor, (x1, y1, x2, y2), score, cls) or (..., score, cls, other classes given the same score)] ; the other
    anchors hold an empty box at the origin with every class at 0"""
    f = np.zeros((4 + nc, n), np.float32)
    for it in items:
        a, (x1, y1, x2, y2), score, cls = it[:4]
        f[0, a], f[1, a], f[2, a], f[3, a] = (x1 + x2) / 2.0, (y1 + y2) / 2.0, x2 - x1, y2 - y1
        f[4 + cls, a] = score
        for k in (it[4] if len(it) > 4 else ()):
            f[4 + k, a] = score
    return f


def k1(name, frames, nc, conf=CONF, iou=IOU, random=False, expect=None):
    out = np.stack(frames)
    return dict(name=name, kind=1, B=len(frames), nc=nc, conf=conf, iou=iou, n_anchors=out.shape[2], out=out, random=random, expect=expect or {})


def spread(n, count):
    """`count` anchors of n, spread over every 256-anchor tile, first and last anchor included"""
    if count == 0:
        return np.zeros(0, np.int64)
    return np.unique(np.round(np.linspace(0, n - 1, count)).astype(np.int64)) if count < n else np.arange(n)


def counts_case(n, count, nc=1):
    """`count` candidates among n anchors on disjoint boxes; scores are binary fractions that repeat every 1024 candidates and run against the
    anchor order, so ranks cross tiles and ties are broken by the anchor"""
    anchors = spread(n, count)
    assert len(anchors) == count
    items = [(int(a), grid_box(j), 0.5 + ((j * 37) % 1024) / 4096.0, 0) for j, a in enumerate(anchors)]
    key = sorted(range(count), key=lambda j: (-items[j][2], items[j][0]))
    order = [items[j][0] for j in key][:2048]
    return k1("k1_n%d_cand%d" % (n, count), [frame_out(n, nc, items)], nc, expect={0: dict(n_cand=min(count, 2048), kept=order[:500], order_head=order[:70])})


def disjoint_case(count):
    items = [(a, grid_box(a), 0.75, 0) for a in range(count)]                # all equal scores: anchor order
    return k1("k1_disjoint_%d" % count, [frame_out(count, 1, items)], 1, expect={0: dict(n_cand=min(count, 2048), kept=list(range(min(count, 500))))})


def suppressor_case():
    """2048 candidates with distinct scores falling with the anchor id (rank = anchor); rank 3 suppresses ranks 63, 64 (the first bit of mask word 1)
    and 2047 (the last bit of the last word); ranks 100 .. 2046 share rank 5's box, so the survivors are few and rank 2047 would show"""
    n = 2049
    items = []
    for a in range(2048):
        box = grid_box(a)
        if a in (63, 64, 2047):
            box = grid_box(3)
        elif 100 <= a < 2047:
            box = grid_box(5)
        items.append((a, box, 1.0 - (a + 1) / 4096.0, 0))
    kept = [a for a in range(100) if a not in (63, 64)]
    return k1("k1_suppressor_rank3", [frame_out(n, 1, items)], 1, expect={0: dict(n_cand=2048, kept=kept)})


def random_out(seed, n, nc, B):
    r = np.random.default_rng(seed)
    f = np.zeros((B, 4 + nc, n), np.float32)
    f[:, 0:2] = r.uniform(0, 96, (B, 2, n))
    f[:, 2:4] = r.uniform(4, 40, (B, 2, n))
    f[:, 4:] = r.uniform(0, 1, (B, nc, n)) ** 3                              # most anchors below conf
    return f


def heads_case(name, in_h, in_w, nc, B, ld, fill, conf=CONF, iou=IOU, random=False, expect=None):
    heads = []
    for i in range(3):
        H, W = in_h >> (3 + i), in_w >> (3 + i)
        h = np.full((B, H * W, ld[i]), 7.0, np.float32)                      # the pitch beyond 64 + nc: a large logit nobody may read
        fill(i, h[:, :, :64 + nc])
        heads.append(h)
    n = sum((in_h >> s) * (in_w >> s) for s in (3, 4, 5))
    return dict(name=name, kind=0, B=B, nc=nc, conf=conf, iou=iou, n_anchors=n, in_w=in_w, in_h=in_h, ld=list(ld), heads=heads, random=random, expect=expect or {})


def one_hot_fill(nc):
    """DFL logits one-hot at +50 / -50 elsewhere in bins (1, 2, 3, 4): boxes (a - 1, a - 2, a + 3, a + 4) * stride exactly; the last side of the
    second scale all equal (expectation 7.5); class logits 0 -> score 0.5 exactly, every class tied"""
    def fill(i, h):
        h[:, :, :64] = -50.0
        for side, bin_ in enumerate((1, 2, 3, 4)):
            h[:, :, 16 * side + bin_] = 50.0
        if i == 1:
            h[:, :, 48:64] = 3.0
        h[:, :, 64:] = 0.0
    return fill


def random_fill(seed, cls_mean):
    def fill(i, h):
        r = np.random.default_rng(seed + i)
        h[:, :, :64] = r.normal(0.0, 2.0, h[:, :, :64].shape)
        h[:, :, 64:] = r.normal(cls_mean, 1.5, h[:, :, 64:].shape)
    return fill


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # candidate counts around the tile (64 per wave, 256 per block) and the cap, n_anchors around the block and above the cap
    for n, count in ((1, 0), (1, 1), (255, 63), (256, 64), (257, 65), (257, 257), (2049, 2047), (2049, 2048), (2049, 2049), (3000, 3000)):
        out.append(counts_case(n, count))
    out.append(k1("k1_all_equal_2100", [frame_out(2100, 1, [(a, grid_box(a), 0.5, 0) for a in range(2100)])], 1,
                  expect={0: dict(n_cand=2048, kept=list(range(500)), order_head=list(range(70)))}))
    # score exactly conf (not a candidate: strict >), the next float above it (one), the next below (not)
    c = np.float32(0.3)
    out.append(k1("k1_conf_edge", [frame_out(4, 1, [(0, grid_box(0), c, 0), (1, grid_box(1), np.nextafter(c, np.float32(1)), 0),
                                                     (2, grid_box(2), np.nextafter(c, np.float32(0)), 0), (3, grid_box(3), 0.5, 0)])], 1, conf=float(c),
                  expect={0: dict(n_cand=2, kept=[3, 1])}))
    for count in (499, 500, 501, 1600):
        out.append(disjoint_case(count))
    # A > B > C in one class: A drops B (IoU 70 / 130), B would drop C (70 / 130) but is dead, A and C overlap 40 / 160; D = A's box in another
    # class stays; E ties over classes 1 and 3 (first wins) and equals F of class 1 (dropped) and G of class 3 (kept)
    A, Bb, Cc = (0, 0, 10, 10), (3, 0, 13, 10), (6, 0, 16, 10)
    E = (40, 40, 50, 50)
    chain = [(0, A, 0.875, 0), (1, Bb, 0.75, 0), (2, Cc, 0.625, 0), (3, A, 0.5, 2), (4, E, 0.4375, 1, (3,)), (5, E, 0.375, 1), (6, E, 0.3125, 3)]
    out.append(k1("k1_chain_classes", [frame_out(16, 4, chain)], 4, expect={0: dict(n_cand=7, kept=[0, 2, 3, 4, 6])}))
    # IoU exactly at the threshold: [0, 0, 2, 2] against [0, 0, 2, 1] is 2 / 4; '>' keeps both at 0.5 and drops the second just below it
    half = [(0, (0, 0, 2, 2), 0.75, 0), (1, (0, 0, 2, 1), 0.5, 0)]
    out.append(k1("k1_iou_exactly_half", [frame_out(2, 1, half)], 1, iou=0.5, expect={0: dict(n_cand=2, kept=[0, 1])}))
    out.append(k1("k1_iou_just_below_half", [frame_out(2, 1, half)], 1, iou=float(np.nextafter(np.float32(0.5), np.float32(0))), expect={0: dict(n_cand=2, kept=[0])}))
    # zero width, inverted, duplicated zero-area boxes inside a real one: no area, no overlap, nobody dropped
    deg = [(0, (0, 0, 20, 20), 0.875, 0), (1, (3, 3, 3, 7), 0.75, 0), (2, (9, 9, 5, 5), 0.625, 0), (3, (4, 4, 4, 4), 0.5, 0), (4, (4, 4, 4, 4), 0.5, 0),
           (5, (4, 4, 4, 4), 0.5, 0), (6, (9, 9, 5, 5), 0.375, 0)]
    out.append(k1("k1_degenerate_boxes", [frame_out(7, 1, deg)], 1, expect={0: dict(n_cand=7, kept=[0, 1, 2, 3, 4, 5, 6])}))
    out.append(suppressor_case())
    # one launch, three frames: all 2100 anchors candidates with class ties over 80 classes, none, 65
    full = frame_out(2100, 80, [(a, grid_box(a), 0.5 + ((a * 37) % 512) / 2048.0, a % 80, ((a % 80 + 7) % 80,)) for a in range(2100)])
    some = frame_out(2100, 80, [(int(a), grid_box(j), 0.5 + j / 256.0, 79) for j, a in enumerate(spread(2100, 65))])
    out.append(k1("k1_batch_2100_0_65", [full, np.zeros_like(full), some], 80,
                  expect={1: dict(n_cand=0, kept=[]), 2: dict(n_cand=65, kept=[int(a) for a in spread(2100, 65)[::-1]])}))
    for i in range(5):
        out.append(k1("k1_random_%d" % i, list(random_out(100 + i, 150, 4, 4)), 4, random=True))
    # raw head maps: 32 x 32 (21 anchors), 64 x 96 (126, not square), 320 x 320 (2100: the smallest grid above the cap)
    out.append(heads_case("k0_32_one_hot", 32, 32, 1, 1, (65, 65, 65), one_hot_fill(1)))
    out.append(heads_case("k0_64x96_one_hot_wide_pitch", 64, 96, 4, 2, (72, 69, 80), one_hot_fill(4)))
    out.append(heads_case("k0_64x96_random", 64, 96, 4, 3, (68, 68, 71), random_fill(7, 0.0), conf=0.5, random=True))
    out.append(heads_case("k0_320_all_equal", 320, 320, 80, 1, (144, 144, 144), lambda i, h: h.fill(0.0), expect={0: dict(n_cand=2048, order_head=list(range(70)))}))
    out.append(heads_case("k0_320_random", 320, 320, 4, 3, (68, 70, 68), random_fill(21, -4.0), conf=0.5, random=True))
    assert len({c["name"] for c in out}) == len(out)
    return out


def oracle_frames(case):
    """reference A: every frame of a case through the oracle"""
    out = []
    for f in range(case["B"]):
        if case["kind"] == 0:
            ld = case["ld"]
            if len(set(ld)) == 1:                                           # the three scales concatenated at their common pitch
                raw, pitch = np.concatenate([case["heads"][i][f] for i in range(3)]), ld[0]
            else:                                                           # different pitches: packed to 64 + nc (the oracle reads one pitch)
                pitch = 64 + case["nc"]
                raw = np.concatenate([case["heads"][i][f][:, :pitch] for i in range(3)])
            out.append(O.yolo_post_ranked(case["conf"], case["iou"], case["nc"], raw=raw, ld=pitch, H=case["in_h"], W=case["in_w"]))
        else:
            out.append(O.yolo_post_ranked(case["conf"], case["iou"], case["nc"], out=case["out"][f]))
    return out



def by_name():
    return {c["name"]: c for c in cases()}


def refusals():
    """(name, keyword arguments of tk.detector_post_probe) the hook must refuse without launching, and calls it must accept"""
    out1 = np.zeros((1, 5, 7), np.float32)
    h = [np.zeros((1, 16, 65), np.float32), np.zeros((1, 4, 65), np.float32), np.zeros((1, 1, 65), np.float32)]
    ok1 = dict(B=1, nc=1, n_anchors=7, conf=0.5, iou=0.5, out=out1)
    ok0 = dict(B=1, nc=1, n_anchors=21, conf=0.5, iou=0.5, heads=h, ld=(65, 65, 65), in_w=32, in_h=32)
    refused = [("B = 0", dict(ok1, B=0)), ("B = 257", dict(ok1, B=257)), ("nc = 0", dict(ok1, nc=0)), ("n_anchors = 0", dict(ok1, n_anchors=0)),
               ("out too short", dict(ok1, n_anchors=8)), ("nc beyond out", dict(ok1, nc=2)), ("cand too short", dict(ok1, sizes=dict(cand=6))),
               ("order too short", dict(ok1, sizes=dict(order=2047))), ("mask too short", dict(ok1, sizes=dict(mask=2048 * 32 - 1))),
               ("kept too short", dict(ok1, sizes=dict(kept=499))), ("n_kept missing", dict(ok1, sizes=dict(n_kept=0))),
               ("kind 0: pitch below 64 + nc", dict(ok0, ld=(65, 64, 65))), ("kind 0: anchors do not add up", dict(ok0, n_anchors=20)),
               ("kind 0: width no multiple of 32", dict(ok0, in_w=48)), ("kind 0: head too short", dict(ok0, nc=2, ld=(66, 66, 66))),
               ("kind 0: two frames in one frame's arrays", dict(ok0, B=2))]
    return refused, [("kind 1", ok1), ("kind 0", ok0), ("no host mask", dict(ok1, with_mask=False))]
