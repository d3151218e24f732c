"""CPU: pins the float64 reference of tests/onnx_ops_ref.py and the bounds of the per-op executor tests — not the kernels.

1. The reference against torch in float64, on the cases of tests/onnx_ops_cases.py, for every op torch has.  Where torch's definition is
   not ONNX's the case is left out and the reason is stated next to it (torch_eval returns None).
2. The bounds' own sensitivity: every contraction case is broken in one way (one tap dropped, one index shifted by one, the k_h k_w
   divisor) and the bound of onnx_ops_ref.check must reject the broken result; its input conditions are asserted as well.
3. Resize: float32 and float64 pick the same pixel in every nearest case — each source coordinate is 1e-4 away from a rounding tie or
   an integer boundary, or it is a value both precisions compute exactly (the ties of scale 2 and 0.5, which pin round_prefer_floor
   against round_prefer_ceil)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import onnx_ops_cases as OC
import onnx_ops_ref as R

T64 = lambda a: torch.from_numpy(np.asarray(a, np.float32).astype(np.float64))
RUNNABLE = [c for c in OC.CASES if not c.refuse or c.either]


def _inputs(c):
    nd = c.spec[-1]
    vals = {**c.floats, **c.feeds}
    ints = {k: np.asarray(v[0]).reshape(v[1] if v[1] is not None else [-1]) for k, v in c.ints.items()}
    return nd, [None if not n else (T64(vals[n]) if n in vals else ints[n]) for n in nd["in"]], R._attrs(nd)


def _pad_hw(x, pads, value=0.0):
    return F.pad(x, (pads[1], pads[3], pads[0], pads[2]), value=value)


def torch_eval(c):
    """the case's outputs from torch (float64), or None when torch has no such op or defines it differently"""
    if len(c.spec) != 1:
        return None
    nd, ins, at = _inputs(c)
    op, x = nd["op"], ins[0]
    opt = lambda i: ins[i] if len(ins) > i else None
    if op == "Conv":
        w, b = ins[1], opt(2)
        if "auto_pad" in at and at["auto_pad"] != "VALID":
            return None  # torch's padding="same" takes stride 1 only; SAME_UPPER / SAME_LOWER are checked against hand-placed pads below
        if x.dim() == 3:
            pd = at.get("pads", [0, 0])
            return [F.conv1d(F.pad(x, (pd[0], pd[1])), w, b, stride=at.get("strides", [1]), dilation=at.get("dilations", [1]), groups=at.get("group", 1))]
        pd = at.get("pads", [0, 0, 0, 0]) if at.get("auto_pad") != "VALID" else [0, 0, 0, 0]
        if len(pd) != 4 or len(at.get("strides", [1, 1])) != 2 or len(at.get("dilations", [1, 1])) != 2:
            return None  # the wrong-length attributes: no defined result
        return [F.conv2d(_pad_hw(x, pd), w, b, stride=at.get("strides", [1, 1]), dilation=at.get("dilations", [1, 1]), groups=at.get("group", 1))]
    if op == "ConvTranspose":
        pd, st, opd = at.get("pads", [0, 0, 0, 0]), at.get("strides", [1, 1]), at.get("output_padding", [0, 0])
        if len(pd) != 4 or len(st) != 2:
            return None
        y = F.conv_transpose2d(x, ins[1], opt(2), stride=st, output_padding=opd)  # torch pads symmetrically only: crop ONNX's four pads by hand
        return [y[:, :, pd[0]:y.shape[2] - pd[2], pd[1]:y.shape[3] - pd[3]]]
    if op in ("MaxPool", "AveragePool"):
        k, st, pd = at["kernel_shape"], at.get("strides", [1, 1]), at.get("pads", [0, 0, 0, 0])
        if len(pd) != 4 or len(st) != 2:
            return None
        cm, sym = bool(at.get("ceil_mode", 0)), pd[0] == pd[2] and pd[1] == pd[3]
        if op == "MaxPool":
            if sym:
                return [F.max_pool2d(x, k, st, (pd[0], pd[1]), ceil_mode=cm)]
            return [F.max_pool2d(_pad_hw(x, pd, float("-inf")), k, st, 0, ceil_mode=cm)]
        if sym:  # the divisor of ceil_mode windows is torch's by definition (ONNX's operator tests follow it)
            return [F.avg_pool2d(x, k, st, (pd[0], pd[1]), ceil_mode=cm, count_include_pad=bool(at.get("count_include_pad", 0)))]
        if cm:
            return None  # torch cannot pad asymmetrically under ceil_mode (its clip of the last window needs the pad it was given)
        if at.get("count_include_pad", 0):
            return [F.avg_pool2d(_pad_hw(x, pd), k, st, 0)]
        s = F.avg_pool2d(_pad_hw(x, pd), k, st, 0, divisor_override=1)
        n = F.avg_pool2d(_pad_hw(torch.ones_like(x), pd), k, st, 0, divisor_override=1)
        return [s / n]
    if op == "GlobalAveragePool":
        return [F.adaptive_avg_pool2d(x, 1)]
    if op in ("Resize", "Upsample"):
        mode = at.get("mode", "nearest")
        ct = "asymmetric" if op == "Upsample" else at.get("coordinate_transformation_mode", "half_pixel")
        nm = "floor" if op == "Upsample" else at.get("nearest_mode", "round_prefer_floor")
        sizes = ins[3] if len(ins) > 3 and ins[3] is not None else None
        sc = at.get("scales") if "scales" in at else (ins[1] if len(ins) == 2 else opt(2))
        kw = dict(size=(int(sizes[2]), int(sizes[3]))) if sizes is not None else dict(scale_factor=(float(sc[2]), float(sc[3])), recompute_scale_factor=False)
        Ho, Wo, _, _ = R.resize_geometry(x.shape[2], x.shape[3], None if sizes is not None else np.asarray(sc), sizes)
        if mode == "nearest":
            if ct == "asymmetric" and nm == "floor":
                return [F.interpolate(x, mode="nearest", **kw)]
            if (ct == "half_pixel" or (ct == "pytorch_half_pixel" and min(Ho, Wo) > 1)) and nm == "round_prefer_ceil":
                return [F.interpolate(x, mode="nearest-exact", **kw)]  # floor((o + 0.5) / scale) = floor(c + 0.5)
            return None  # torch has no other nearest rounding: round_prefer_floor, ceil and align_corners nearest are ONNX's alone
        if ct == "align_corners":
            return [F.interpolate(x, mode="bilinear", align_corners=True, **kw)] if sizes is not None else None  # with align_corners torch ignores scale_factor
        if ct == "half_pixel" or (ct == "pytorch_half_pixel" and min(Ho, Wo) > 1):
            return [F.interpolate(x, mode="bilinear", align_corners=False, **kw)]
        return None  # asymmetric bilinear is ONNX's alone; so is pytorch_half_pixel to ONE pixel: ONNX reads pixel 0 there, torch the centre
    if op == "Pad":
        pads = at["pads"] if "pads" in at else [int(p) for p in ins[1]]
        r = x.dim()
        tp = [p for i in range(r - 1, -1, -1) for p in (pads[i], pads[r + i])]
        if at.get("mode", "constant") == "reflect":
            lead = [i for i in range(r) if pads[i] or pads[r + i]]
            if not lead or r - min(lead) > 3:
                return None  # torch reflects the last three axes at the most
            k = r - min(lead)
            xx = x.reshape((1,) * (k + 2 - r) + tuple(x.shape)) if r < k + 2 else x
            y = F.pad(xx, tp[:2 * k], mode="reflect")
            return [y.reshape([x.shape[i] + pads[i] + pads[r + i] for i in range(r)])]
        cval = float(ins[2].reshape(-1)[0]) if len(ins) > 2 and ins[2] is not None else at.get("value", 0.0)
        return [F.pad(x, tp, value=cval)]
    if op == "LayerNormalization":
        return [F.layer_norm(x, x.shape[-1:], ins[1], opt(2), at.get("epsilon", float(np.float32(1e-5))))]
    if op == "BatchNormalization":
        return [F.batch_norm(x, ins[3], ins[4], ins[1], ins[2], False, 0.0, at.get("epsilon", float(np.float32(1e-5))))]
    if op == "Softmax":
        if c.opset < 13 and x.dim() != 2:
            return None  # the 2-D coercion of the old opsets is ONNX's alone; checked against a hand-written flattening below
        return [torch.softmax(x, at.get("axis", -1 if c.opset >= 13 else 1))]
    if op == "LSTM":
        H, I_ = ins[2].shape[2], ins[1].shape[2]
        m = torch.nn.LSTM(I_, H, bias=True).double()
        perm = lambda t: torch.cat([t[0:H], t[2 * H:3 * H], t[3 * H:4 * H], t[H:2 * H]])  # ONNX rows i, o, f, c -> torch's i, f, g, o
        B = ins[3].reshape(-1) if opt(3) is not None else torch.zeros(8 * H, dtype=torch.float64)
        with torch.no_grad():
            m.weight_ih_l0.copy_(perm(ins[1][0])); m.weight_hh_l0.copy_(perm(ins[2][0]))
            m.bias_ih_l0.copy_(perm(B[:4 * H])); m.bias_hh_l0.copy_(perm(B[4 * H:]))
            h0 = opt(5) if opt(5) is not None else torch.zeros(1, 1, H, dtype=torch.float64)
            c0 = opt(6) if opt(6) is not None else torch.zeros(1, 1, H, dtype=torch.float64)
            y, (hn, cn) = m(x, (h0, c0))
        return [y[:, None], hn, cn]
    if op == "Erf":
        return [torch.erf(x)]
    if op == "Gelu":
        return [F.gelu(x, approximate=at.get("approximate", "none"))]
    if op == "Pow":
        return [torch.pow(x, ins[1])]
    if op == "MatMul":
        return [torch.matmul(x, ins[1])]
    if op == "Gemm":
        if len(ins) > 2 and ins[2] is not None:
            return [x @ (ins[1].T if at.get("transB", 0) else ins[1]) + ins[2]]
        return [x @ (ins[1].T if at.get("transB", 0) else ins[1])]
    if op in ("Sigmoid", "Tanh", "Exp", "Log", "Sqrt"):
        return [getattr(torch, op.lower())(x)]
    if op == "HardSigmoid" and not nd["attrs"]:
        return None  # torch's hardsigmoid is x / 6 + 0.5, ONNX's default alpha is 0.2
    if op == "HardSwish":
        return [F.hardswish(x)]
    if op in ("ReduceSum", "ReduceMean", "ReduceL2", "ReduceMax", "ReduceMin"):
        axes = at.get("axes") if "axes" in at else ([int(a) for a in ins[1]] if len(ins) > 1 and ins[1] is not None else [])
        if not axes:
            if at.get("noop_with_empty_axes", 0):
                return [x]
            axes = list(range(x.dim()))
        keep = bool(at.get("keepdims", 1))
        f = {"ReduceSum": torch.sum, "ReduceMean": torch.mean, "ReduceMax": torch.amax, "ReduceMin": torch.amin}.get(op)
        return [f(x, dim=axes, keepdim=keep) if f else torch.linalg.vector_norm(x, 2, dim=axes, keepdim=keep)]
    return None


def _close(ref, want, what):
    want = want.detach().numpy()
    assert ref.shape == tuple(want.shape), (what, ref.shape, want.shape)
    with np.errstate(all="ignore"):
        same = (ref.v == want) | (np.isnan(ref.v) & np.isnan(want))
        err = np.where(same, 0.0, np.abs(ref.v - want))
    scale = np.max(np.abs(want[np.isfinite(want)]), initial=0.0)
    assert np.all(err <= 1e-12 * max(scale, 1e-300)), (what, float(np.max(err)), scale)


@pytest.mark.parametrize("group", OC.GROUPS)
def test_reference_matches_torch_float64(group):
    """1e-12 of the tensor's scale: two float64 evaluations in different orders"""
    n = 0
    for c in OC.cases_of(group):
        if (c.refuse and not c.either) or c.group == "attr_len":  # refused inputs and malformed attributes have no defined result
            continue
        want = torch_eval(c)
        if want is None:
            continue
        refs = R.run(c.spec, c.feeds, c.floats, c.ints, c.opset)
        for o, w in zip(c.outputs, want):
            _close(refs[o], w, c.id + ":" + o)
        n += 1
    ops_without_torch = {"attr_len", "broadcast", "domain", "gather", "layout", "slice"}  # moves, selects and single operations: nothing to pin
    assert n > 0 or group in ops_without_torch, group


def test_reference_definitions_torch_lacks():
    """the ONNX-only definitions, against a second hand-written evaluation: SAME_UPPER / SAME_LOWER pads, opset-11 Softmax coercion"""
    for c in OC.cases_of("conv_dense"):
        ap = c.spec[0]["attrs"].get("auto_pad")
        if ap not in ("SAME_UPPER", "SAME_LOWER"):
            continue
        x, w, b = T64(c.feeds["x0"]), T64(c.floats["k1"]), T64(c.floats["k2"])
        st = c.spec[0]["attrs"]["strides"]
        pads = []
        for d in (2, 3):  # ONNX: output = ceil(in / stride); the odd cell goes to the end for SAME_UPPER, to the beginning for SAME_LOWER
            out = -(-x.shape[d] // st[d - 2])
            total = max(0, (out - 1) * st[d - 2] + w.shape[d] - x.shape[d])
            small, large = total // 2, total - total // 2
            pads.append((small, large) if ap == "SAME_UPPER" else (large, small))
        want = F.conv2d(F.pad(x, (pads[1][0], pads[1][1], pads[0][0], pads[0][1])), w, b, stride=st)
        _close(R.run(c.spec, c.feeds, c.floats, c.ints, c.opset)["y"], want, c.id)
    upper, lower = [R.run(c.spec, c.feeds, c.floats, c.ints)["y"].v for c in OC.cases_of("conv_dense") if c.name in ("same_upper", "same_lower")]
    assert upper.shape == lower.shape == (1, 4, 4, 5)
    for c in OC.cases_of("softmax"):
        if c.opset >= 13 or c.feeds["x0"].ndim != 3:
            continue
        x = T64(c.feeds["x0"])
        ax = c.spec[0]["attrs"].get("axis", 1)
        want = torch.softmax(x.reshape(int(np.prod(x.shape[:ax])), -1), 1).reshape(x.shape)
        ref = R.run(c.spec, c.feeds, c.floats, c.ints, c.opset)["y"]
        _close(ref, want, c.id)
        single = torch.softmax(x, ax).numpy()
        assert np.max(np.abs(single - ref.v)) > 1e-3, "the case must tell the coerced definition from a single-axis softmax"


CONTRACTIONS = [c for c in RUNNABLE if R.kind_of(c.spec[-1]) in R.CHAIN and c.group != "attr_len"]


def _broken_inputs(c):
    """one deliberate error per contraction case: a weight tap dropped (two-operand contractions), or one input element replaced by its
    neighbour (an index shifted by one) where the clamp of HardSigmoid / HardSwish does not hide it, or one summed element dropped"""
    nd = c.spec[-1]
    feeds, floats = {k: v.copy() for k, v in c.feeds.items()}, {k: v.copy() for k, v in c.floats.items()}
    if nd["op"] in ("MatMul", "Gemm", "Conv", "ConvTranspose"):
        name = nd["in"][1]
        t = floats[name] if name in floats else feeds[name]
        t.reshape(-1)[np.argmax(np.abs(t.reshape(-1)))] = 0.0
        return feeds, floats
    x = feeds[nd["in"][0]].reshape(-1)
    if nd["op"] in ("HardSigmoid", "HardSwish"):
        i = int(np.argmin(np.abs(x)))
        x[i] = x[i + 1] if i + 1 < x.size else x[i - 1]
    else:  # sums and means: drop the first tap of typical size (at least the median magnitude)
        x[int(np.argmax(np.abs(x) >= np.median(np.abs(x))))] = 0.0
    return feeds, floats


@pytest.mark.parametrize("case", CONTRACTIONS, ids=lambda c: c.id)
def test_bound_rejects_a_one_tap_error(case):
    c = case
    refs = R.run(c.spec, c.feeds, c.floats, c.ints, c.opset)
    feeds, floats = _broken_inputs(c)
    broken = R.run(c.spec, feeds, floats, c.ints, c.opset)
    for o in c.outputs:
        ref, kind = refs[o], R.kind_of(c.producer(o))
        if ref.info.get("exact"):
            continue
        n, S = ref.info["n"], ref.info["S"]
        # the input condition: gamma(n + 2) S stays under a quarter of the mean |term| = S / n (so n <= ~2000)
        assert R.gamma(n + 2) * n < 0.25, (c.id, n)
        ok, _ = R.check(kind, ref.v.astype(np.float32), ref)
        assert ok.all(), (c.id, "the float32 rounding of the reference itself must pass")
        ok, ratio = R.check(kind, broken[o].v.astype(np.float32), ref)
        assert not ok.all(), (c.id, "a one-tap error stays inside the bound: reshape the case", float(ratio.max()))


@pytest.mark.parametrize("case", [c for c in OC.cases_of("pool_avg")], ids=lambda c: c.id)
def test_bound_rejects_the_kh_kw_divisor(case):
    """every AveragePool case has a window that is not full; dividing it by k_h k_w must fall outside the bound whenever that differs from
    the definition (count_include_pad = 0 with pads, ceil_mode windows beyond the padded extent)"""
    c = case
    at = R._attrs(c.spec[0])
    x = c.feeds["x0"].astype(np.float64)
    args = (at["kernel_shape"], at.get("strides", [1, 1]), at.get("pads", [0, 0, 0, 0]), at.get("ceil_mode", 0), at.get("count_include_pad", 0))
    wrong, _ = R.pool2d(x, "avg", *args, divisor="khkw")
    ref = R.run(c.spec, c.feeds, c.floats, c.ints, c.opset)["y"]
    ok, _ = R.check("AveragePool", wrong.astype(np.float32), ref)
    differs = np.abs(wrong - ref.v) > 0
    pads_only_inside = at.get("count_include_pad", 0) and not (at.get("ceil_mode", 0) and c.name.startswith(("ceil_k2", "ceil_k3_s2_p0011")))
    assert differs.any() != bool(pads_only_inside), c.id
    assert np.array_equal(~ok, differs), c.id


RESIZE_NEAREST = [c for c in OC.CASES if c.spec[0]["op"] in ("Resize", "Upsample") and c.spec[0]["attrs"].get("mode", "nearest") == "nearest"]


@pytest.mark.parametrize("case", RESIZE_NEAREST, ids=lambda c: c.id)
def test_resize_coordinates_pick_one_pixel_in_both_precisions(case):
    c = case
    nd, ins, at = _inputs(c)
    up = nd["op"] == "Upsample"
    ct = "asymmetric" if up else at.get("coordinate_transformation_mode", "half_pixel")
    nm = "floor" if up else at.get("nearest_mode", "round_prefer_floor")
    sizes = ins[3] if len(ins) > 3 and ins[3] is not None else None
    sc = at.get("scales") if "scales" in at else (ins[1] if len(ins) == 2 else (ins[2] if len(ins) > 2 else None))
    H, W = c.feeds["x0"].shape[2:]
    Ho, Wo, sh, sw = R.resize_geometry(H, W, None if sizes is not None else np.asarray(sc), sizes)
    for in_, out, s in ((H, Ho, sh), (W, Wo, sw)):
        c64 = R.resize_coords(in_, out, s, ct)
        c32 = R.resize_coords(in_, out, np.float32(s), ct, dtype=np.float32)  # the executor's arithmetic: float32, one rounding per operation
        tie_at = 0.0 if nm in ("floor", "ceil") else 0.5
        dist = np.abs((c64 - tie_at) - np.round(c64 - tie_at))
        exact = c32.astype(np.float64) == c64
        assert np.all((dist >= 1e-4) | exact), (c.id, c64[(dist < 1e-4) & ~exact])
        assert np.array_equal(R.nearest_index(c64, in_, nm), R.nearest_index(c32.astype(np.float64), in_, nm)), c.id


def test_resize_ties_tell_the_two_round_modes_apart():
    """scale 2 and 0.5 put source coordinates exactly on .5: round_prefer_floor and round_prefer_ceil must read different pixels there"""
    by = {c.name: R.run(c.spec, c.feeds, c.floats, c.ints)["y"].v for c in OC.cases_of("resize_nearest")}
    for which in ("asymmetric_x2", "half_pixel_x0.5"):  # o / 2 and 2 o + 0.5
        assert not np.array_equal(by["round_prefer_floor_" + which], by["round_prefer_ceil_" + which]), which


def test_reference_stands_alone():
    """the reference imports nothing from oracle/ and does not read the float32 oracle's code"""
    import os
    for f in ("onnx_ops_ref.py", "onnx_ops_cases.py"):
        src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), f)).read()
        assert "oracle_lib" not in src and "depth_oracle" not in src and "import oracle" not in src and "from oracle" not in src, f
