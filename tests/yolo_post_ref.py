"""Reference B of the detector post-processing: float64 NumPy written from the comments of csrc/common/tk_yolo_post.h and of the kernels in
csrc/vision/tk_vision_engine.hip (k_yolo_decode, k_yolo_decode_out, k_yolo_rank, k_yolo_mask, k_yolo_scan).  It never imports the oracle.

What it computes, per frame:
  decode   kind 0: per anchor four DFL expectations over 16 bins (softmax-weighted bin index), anchor centre (x + 0.5, y + 0.5) on the grid of its
           scale, xyxy = (centre -/+ distance) * stride (8, 16, 32); score = max_c sigmoid(logit_c), first class on ties.
           kind 1: xyxy = centre -/+ size / 2, score = max_c p_c, first class on ties.
  rank     candidates are the anchors with score > conf, ordered by (score descending, anchor ascending); at most 2048 enter NMS.
  NMS      a plain O(n^2) greedy loop: a candidate is dropped iff a box KEPT before it has the same class and IoU > iou; at most 500 results.

Every value carries a bound on the distance between it and the kernels' float32 value, built term by term in the running-error form of
tests/split_f16_ref.py: an operation whose exact result is a float32 number and whose inputs are exact adds nothing (IEEE operations are correctly
rounded), any other adds |result| * 2^-24; tk_expf adds its relative error 2^-22 and tk_divf is a correctly rounded division (both from
csrc/common/tk_exact_math.h, not from a measurement).  A frame ABSTAINS when one of its decisions — score against conf, two scores against each
other, an IoU against the threshold, an overlap against zero — is closer than the bounds of its operands can decide.  Boxes on an integer grid
with scores that are binary fractions have bounds of zero everywhere but the final division of the IoU, so crafted frames never abstain.

MUTATIONS: one plausible kernel error each; tests/test_yolo_post_cpu.py shows that every one changes the answer of at least one GPU case."""
import numpy as np

U = 2.0 ** -24                      # half an ulp, relative: one correctly rounded float32 operation
EXPF_REL = 2.0 ** -22               # tk_expf: "relative error <= 2^-22" (tk_exact_math.h)
SLACK = 1.001                       # second-order terms of the first-order propagation below
MAX_CAND, MAX_DET = 2048, 500
MUTATIONS = ("conf_ge", "iou_ge", "ties_desc", "cap_2047", "cap_2049", "det_499", "det_501", "class_blind", "dead_suppresses", "mask_word_dropped",
             "wh_swapped", "wrong_stride", "last_class_on_ties")


def _rnd(v, in_err):
    """the rounding term of one float32 operation with exact result v: nothing when the operands are exact and v is a float32 number"""
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        exact = (np.asarray(in_err) == 0) & (v.astype(np.float32).astype(np.float64) == v)
    return np.where(exact, 0.0, np.abs(v) * U)


def _argmax_classes(v, mut):
    """first (mutation: last) index of the row maximum of v [n][nc]; NaN never wins, an all-NaN / empty row answers class 0 with score -1"""
    w = np.where(np.isnan(v), -np.inf, v)
    first = np.argmax(w, axis=1)
    if "last_class_on_ties" in mut:
        first = v.shape[1] - 1 - np.argmax(w[:, ::-1], axis=1)
    best = w[np.arange(len(w)), first]
    none = ~(best > -1.0)                                                   # the kernels start from best = -1 and take s > best
    return np.where(none, 0, first), np.where(none, -1.0, best)


def decode_out(out, nc, mut=()):
    """kind 1, one frame: out [4 + nc][n] float32 -> dict of float64 arrays with bounds"""
    o = np.asarray(out, np.float32).astype(np.float64)
    cx, cy, w, h = o[0], o[1], o[2], o[3]
    box = np.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], axis=1)      # 0.5 * w is exact
    cls, score = _argmax_classes(o[4:4 + nc].T, mut)
    return dict(box=box, box_err=_rnd(box, 0.0) * SLACK, score=score, score_err=np.zeros(len(score)), tie_key=score.copy(), cls=cls, cls_open=np.zeros(len(score), bool))


def _dfl(l):
    """l [..., 16] float32 logits -> (expectation, bound), tk_yolo_dfl's order: m = max, p_i = tk_expf(l_i - m), s += p_i, e = fma(i, p_i, e), e / s"""
    l = np.asarray(l, np.float64)
    d = l - l.max(axis=-1, keepdims=True)
    d_err = _rnd(d, 0.0)
    zero = d < -87.0                                                        # tk_expf returns 0 below -87
    p = np.where(zero, 0.0, np.exp(np.where(zero, 0.0, d)))
    p_err = np.where(zero | (d == 0.0), 0.0, p * (EXPF_REL + d_err))        # tk_expf(0) is exactly 1
    s = np.zeros(l.shape[:-1]); s_err = np.zeros_like(s); e = np.zeros_like(s); e_err = np.zeros_like(s)
    for i in range(16):
        s = s + p[..., i]
        s_err = s_err + p_err[..., i]
        s_err = s_err + _rnd(s, s_err)
        e = e + i * p[..., i]
        e_err = e_err + i * p_err[..., i]
        e_err = e_err + _rnd(e, e_err)
    q = e / s
    q_err = e_err / s + q * s_err / s
    return q, (q_err + _rnd(q, q_err)) * SLACK


def decode_heads(heads, in_h, in_w, nc, mut=()):
    """kind 0, one frame: heads[i] [H_i W_i][>= 64 + nc] float32 -> dict as decode_out"""
    boxes, errs, logits = [], [], []
    strides = (16.0, 32.0, 8.0) if "wrong_stride" in mut else (8.0, 16.0, 32.0)
    for i, hm in enumerate(heads):
        H, W = in_h >> (3 + i), in_w >> (3 + i)
        hm = np.asarray(hm, np.float32)
        assert hm.shape[0] == H * W and np.all(np.abs(hm[:, :64 + nc]) <= 80.0)
        local = np.arange(H * W)
        ax, ay = (local % H + 0.5, local // H + 0.5) if "wh_swapped" in mut else (local % W + 0.5, local // W + 0.5)
        d, d_err = _dfl(hm[:, :64].reshape(-1, 4, 16))
        c = np.stack([ax - d[:, 0], ay - d[:, 1], ax + d[:, 2], ay + d[:, 3]], axis=1)
        c_err = d_err + _rnd(c, d_err)
        boxes.append(c * strides[i])                                        # a power of two: exact
        errs.append(c_err * strides[i] * SLACK)
        logits.append(hm[:, 64:64 + nc].astype(np.float64))
    x = np.concatenate(logits)
    sig = 1.0 / (1.0 + np.exp(-x))
    # e = tk_expf(-x) (2^-22, exactly 1 at x = 0), t = 1 + e, s = 1 / t: relative error of s <= 2^-22 e / (1 + e) + 2^-24 + 2^-24
    sig_err = np.where(x == 0.0, 0.0, sig * (EXPF_REL * (1.0 - sig) + 2 * U) * SLACK)
    cls, score = _argmax_classes(sig, mut)
    rows = np.arange(len(x))
    err = sig_err[rows, cls]
    # another class whose score is closer to the best than the bounds decide, from a different logit: its float32 score may tie or win
    rival = (np.abs(sig - score[:, None]) <= sig_err + err[:, None]) & (x != x[rows, cls][:, None])
    return dict(box=np.concatenate(boxes), box_err=np.concatenate(errs), score=score, score_err=err, tie_key=x[rows, cls], cls=cls, cls_open=rival.any(axis=1))


def _iou(dec, others, one):
    """IoU of boxes `others` (index array) against box `one` -> (iou, bound, undecided): tk_yolo_iou's operations one by one"""
    b, e = dec["box"], dec["box_err"]
    A, Ae, Bx, Be = b[others], e[others], b[one], e[one]
    iw = np.minimum(A[:, 2], Bx[2]) - np.maximum(A[:, 0], Bx[0])
    ih = np.minimum(A[:, 3], Bx[3]) - np.maximum(A[:, 1], Bx[1])
    iw_in, ih_in = np.maximum(Ae[:, 2], Be[2]) + np.maximum(Ae[:, 0], Be[0]), np.maximum(Ae[:, 3], Be[3]) + np.maximum(Ae[:, 1], Be[1])
    iw_err, ih_err = iw_in + _rnd(iw, iw_in), ih_in + _rnd(ih, ih_in)
    apart = ~((iw > 0) & (ih > 0))
    surely_apart = (iw <= -iw_err) | (ih <= -ih_err)                       # with exact operands (bound 0) "not above zero" is decided
    undecided = ~surely_apart & ((np.abs(iw) < iw_err) | (np.abs(ih) < ih_err))
    inter = iw * ih
    inter_err = iw_err * np.abs(ih) + ih_err * np.abs(iw)
    inter_err = inter_err + _rnd(inter, inter_err)

    def area(X, Xe):
        w, h = X[..., 2] - X[..., 0], X[..., 3] - X[..., 1]
        w_in, h_in = Xe[..., 2] + Xe[..., 0], Xe[..., 3] + Xe[..., 1]
        w_err, h_err = w_in + _rnd(w, w_in), h_in + _rnd(h, h_in)
        a = w * h
        a_err = w_err * np.abs(h) + h_err * np.abs(w)
        return a, a_err + _rnd(a, a_err)
    ua, ua_err = area(A, Ae)
    ub, ub_err = area(Bx, Be)
    t = ua + ub
    t_err = ua_err + ub_err
    t_err = t_err + _rnd(t, t_err)
    uni = t - inter
    uni_err = t_err + inter_err
    uni_err = uni_err + _rnd(uni, uni_err)
    undecided |= ~apart & (np.abs(uni) < uni_err)
    empty = apart | ~(uni > 0)
    safe = np.where(empty, 1.0, uni)
    q = np.where(empty, 0.0, inter / safe)
    q_err = np.where(empty, 0.0, inter_err / np.abs(safe) + np.abs(q) * uni_err / np.abs(safe))
    q_err = np.where(empty, 0.0, (q_err + _rnd(q, q_err)) * SLACK)
    return q, q_err, undecided


def post(dec, conf, iou, mut=(), want_pairs=False):
    """rank + NMS of one decoded frame -> dict(valid [n] bool, order, n_cand, kept (anchor ids), n_kept, abstain, why); with want_pairs also
    pairs [n_cand][n_cand] int8: 1 where rank i suppresses rank j > i (same class, IoU > iou), 0 where not, -1 where undecided"""
    conf, thr = float(np.float32(conf)), float(np.float32(iou))
    s, e = dec["score"], dec["score_err"]
    why = []
    valid = (s >= conf) if "conf_ge" in mut else (s > conf)
    if np.any((np.abs(s - conf) <= e) & (e > 0)):
        why.append("a score within its bound of conf")
    idx = np.flatnonzero(valid)
    if np.any(dec["cls_open"][idx]):
        why.append("two class scores of a candidate within their bounds")
    o = idx[np.lexsort((-idx if "ties_desc" in mut else idx, -s[idx]))]
    close = (np.abs(np.diff(s[o])) <= e[o][1:] + e[o][:-1]) & (dec["tie_key"][o][1:] != dec["tie_key"][o][:-1])
    if np.any(close):
        why.append("two neighbouring scores within their bounds")
    o = o[:2047 if "cap_2047" in mut else 2049 if "cap_2049" in mut else MAX_CAND]
    n = len(o)
    det_cap = 499 if "det_499" in mut else 501 if "det_501" in mut else MAX_DET
    cls = dec["cls"][o]
    pairs = np.zeros((n, n), np.int8) if want_pairs else None
    kept, before = [], []
    # boxes that cannot overlap even at the far ends of their bounds have IoU 0 whatever the rounding: only the others go through _iou
    lo, hi = dec["box"][o][:, :2] - dec["box_err"][o][:, :2], dec["box"][o][:, 2:] + dec["box_err"][o][:, 2:]
    for j in range(n):
        if len(kept) >= det_cap:
            break
        prev = np.asarray(before if "dead_suppresses" in mut else kept, np.int64)
        sup_any = False
        if len(prev):
            near = np.all(np.minimum(hi[prev], hi[j]) > np.maximum(lo[prev], lo[j]), axis=1)
            if "class_blind" not in mut:
                near &= cls[prev] == cls[j]
            prev = prev[near]
        if len(prev):
            q, q_err, und = _iou(dec, o[prev], o[j])
            und = und | ((q_err > 0) & (np.abs(q - thr) <= q_err))
            sup = (q >= thr) if "iou_ge" in mut else (q > thr)
            if "mask_word_dropped" in mut and j % 64 == 0:
                sup = sup & False
            sup_any = bool(np.any(sup & ~und))                              # one decided suppressor is enough; none but an open pair leaves the frame open
            if not sup_any and np.any(und):
                why.append("an IoU within its bound of the threshold")
        before.append(j)
        if not sup_any:
            kept.append(j)
    if want_pairs:
        for j in range(1, n):
            q, q_err, und = _iou(dec, o[:j], o[j])
            und = und | ((q_err > 0) & (np.abs(q - thr) <= q_err))
            same = cls[:j] == cls[j]
            pairs[:j, j] = np.where(same & und, -1, (same & (q > thr)).astype(np.int8))
    return dict(valid=valid, order=o, n_cand=n, kept=o[np.asarray(kept, np.int64)], n_kept=len(kept), abstain=bool(why), why=why, pairs=pairs)


def run_case(case, mut=(), want_pairs=False):
    """every frame of a case (tests/yolo_post_cases.py) -> list of (decoded, post) per frame"""
    frames = []
    for f in range(case["B"]):
        if case["kind"] == 0:
            heads = [case["heads"][i][f][:, :64 + case["nc"]] for i in range(3)]
            dec = decode_heads(heads, case["in_h"], case["in_w"], case["nc"], mut)
        else:
            dec = decode_out(case["out"][f], case["nc"], mut)
        frames.append((dec, post(dec, case["conf"], case["iou"], mut, want_pairs)))
    return frames


def compare_frame(got, dec, res):
    """what one frame of a launch left behind (got: cand records [n], order, n_cand, kept records, n_kept) against this reference.  Decoded boxes and
    scores of EVERY anchor must lie inside their bounds (exactly equal where the bound is zero); the discrete answers must be equal unless the frame
    abstains.  Returns (worst box error / bound, worst score error / bound) over the entries with a bound above zero."""
    cand = got["cand"]
    box = np.stack([cand[k].astype(np.float64) for k in ("x1", "y1", "x2", "y2")], axis=1)
    d = np.abs(box - dec["box"])
    assert np.all(d <= dec["box_err"]), ("a decoded box outside its bound", float(np.max(d - dec["box_err"])))
    ds = np.abs(cand["score"].astype(np.float64) - dec["score"])
    assert np.all(ds <= dec["score_err"]), ("a score outside its bound", float(np.max(ds - dec["score_err"])))
    assert np.array_equal(cand["anchor"], np.arange(len(cand)))
    ratio = [float(np.max(np.where(b > 0, e / np.where(b > 0, b, 1.0), 0.0), initial=0.0)) for e, b in ((d, dec["box_err"]), (ds, dec["score_err"]))]
    if not res["abstain"]:
        assert np.array_equal(cand["cls"] >= 0, res["valid"]), "the candidate set"
        assert np.array_equal(cand["cls"][res["valid"]], dec["cls"][res["valid"]]), "a candidate's class"
        assert got["n_cand"] == res["n_cand"] and np.array_equal(got["order"][:res["n_cand"]], res["order"]), "the ranked list"
        assert got["n_kept"] == res["n_kept"] and np.array_equal(got["kept"]["anchor"][:res["n_kept"]], res["kept"]), "the survivors"
    return tuple(ratio)
