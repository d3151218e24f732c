"""The per-op cases of the graph-executor tests: one small ONNX graph each, shared by tests/test_onnx_ops_cpu.py (the reference against
torch, the bounds' sensitivity) and tests/test_onnx_ops_gpu.py (the executor against the reference).

A case names its group (one GPU test function per group), its nodes, the float tensors fed at run time, float / integer initialisers, the
values read back, the opset, and — for inputs the executor must refuse — the words its error text must contain.  `either` marks the cases
where a correct result and a refusal are both acceptable, a silently different result is not."""
import zlib

import numpy as np

import onnx_util as OU

INT64_MAX = (1 << 63) - 1


class K:
    """a float initialiser (weights, Clip bounds, Resize scales: what the executor needs as constants)"""
    def __init__(self, a):
        self.a = np.asarray(a, np.float32)


class I:
    """an int64 initialiser"""
    def __init__(self, v, dims=None):
        self.v, self.dims = list(np.asarray(v, np.int64).reshape(-1)), dims


class Bm(I):
    """a bool initialiser"""


class Case:
    def __init__(self, group, name, spec, feeds, floats, ints, outputs, opset=17, refuse=None, either=False):
        self.group, self.name, self.spec, self.feeds, self.floats, self.ints = group, name, spec, feeds, floats, ints
        self.outputs, self.opset, self.refuse, self.either = outputs, opset, refuse, either

    @property
    def id(self):
        return self.group + "/" + self.name

    def model(self):
        inits = [OU.tensor(k, v) for k, v in self.floats.items()]
        inits += [(OU.bool_tensor if (k == "mask" or k.startswith("bool_")) else OU.int_tensor)(k, np.asarray(v[0]).reshape(-1), v[1]) for k, v in self.ints.items()]
        ins = [OU.value_info(k, 1, list(v.shape)) for k, v in self.feeds.items()]
        outs = [OU.value_info(k, 1, []) for k in self.outputs]
        return OU.model(OU.spec_nodes(self.spec), inits, ins, outs, opset=self.opset)

    def producer(self, name):
        return next(nd for nd in self.spec if name in nd["out"])


def nd(op, ins, outs, **attrs):
    return {"op": op, "in": list(ins), "out": list(outs) if isinstance(outs, (list, tuple)) else [outs], "attrs": attrs}


CASES = []


def rng_for(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def add(group, name, op, ins, /, n_out=1, opset=17, refuse=None, either=False, **attrs):
    """a single-node case: ins are float32 arrays (fed as x0, x1, ...), K / I / Bm initialisers, or None for an omitted optional input"""
    feeds, floats, ints, names = {}, {}, {}, []
    for i, a in enumerate(ins):
        if a is None:
            names.append("")
        elif isinstance(a, K):
            floats["k%d" % i] = a.a
            names.append("k%d" % i)
        elif isinstance(a, Bm):
            ints["bool_%d" % i] = (a.v, a.dims)
            names.append("bool_%d" % i)
        elif isinstance(a, I):
            ints["i%d" % i] = (a.v, a.dims)
            names.append("i%d" % i)
        else:
            feeds["x%d" % i] = np.asarray(a, np.float32)
            names.append("x%d" % i)
    while names and names[-1] == "":
        names.pop()
    outs = ["y"] if n_out == 1 else ["y%d" % i for i in range(n_out)]
    CASES.append(Case(group, name, [nd(op, names, outs, **attrs)], feeds, floats, ints, outs, opset, refuse, either))


def _build():
    def rn(name, *shape):
        return rng_for(name).standard_normal(shape).astype(np.float32)

    # ---------------------------------------------------------------- MatMul: [M, K] x [K, N] activations, b_kn = 1 (tk_launch_gemm)
    for M, K_, N, where in [(1, 1, 1, "k_gemm_f32, path 0 (K % 4 != 0)"),
                            (5, 7, 3, "k_gemm_f32, path 0"),
                            (65, 33, 66, "k_gemm_f32, path 0: tails of the 64 x 64 x 32 tile in M, N and K"),
                            (64, 32, 64, "k_gemm_f32, path 2: exactly one tile"),
                            (68, 36, 100, "k_gemm_f32, path 2: K % 4 == 0 and N % 4 == 0, tails"),
                            (257, 36, 100, "k_gemm_f32_big (M >= 256, N >= 96), path 2"),
                            (257, 35, 97, "k_gemm_f32_big, path 0"),
                            (255, 36, 100, "k_gemm_f32 just under the M threshold of the big kernel, path 2"),
                            (256, 36, 95, "k_gemm_f32 just under the N threshold of the big kernel (b_kn keeps it off the tall kernel), path 0")]:
        n = "%dx%dx%d" % (M, K_, N)
        add("matmul", n, "MatMul", [rn(n + "a", M, K_), rn(n + "b", K_, N)])
    add("matmul", "rank3_a", "MatMul", [rn("r3a", 2, 5, 7), rn("r3b", 7, 3)])  # A [2, 5, 7] flattens to M = 10: k_gemm_f32, path 0
    add("matmul", "batched_2x3", "MatMul", [rn("ba", 2, 3, 5, 7), rn("bb", 2, 3, 7, 4)])  # batch 6, sA = 35, sB = 28 (no multiples of 4): path 0
    add("matmul", "batched_bcast_b", "MatMul", [rn("bc", 2, 3, 5, 8), rn("bd", 1, 1, 8, 4)])  # B broadcast (sB = 0), sA = 40: path 2
    add("matmul", "batched_big", "MatMul", [rn("be", 2, 256, 8), rn("bf", 2, 8, 96)])  # k_gemm_f32_big with a batch, path 2

    # ---------------------------------------------------------------- Gemm
    for M, K_, N, where in [(3, 8, 5, "k_gemm_f32, path 1 ([N][K] weights, K % 4 == 0)"),
                            (3, 7, 5, "k_gemm_f32, path 0"),
                            (256, 32, 96, "k_gemm_f32_big, path 1"),
                            (513, 4, 1, "k_gemm_f32_tall NT = 1, path 1"), (513, 5, 1, "tall NT = 1, path 0"),
                            (513, 4, 33, "tall NT = 2, path 1"), (513, 5, 33, "tall NT = 2, path 0"),
                            (513, 4, 95, "tall NT = 3, path 1"), (513, 5, 95, "tall NT = 3, path 0"),
                            (511, 4, 33, "k_gemm_f32: one row under the tall kernel's M >= 512"),
                            (512, 4, 96, "k_gemm_f32_big: N = 96 leaves the tall kernel")]:
        for cshape in ([N], [1, N]):
            n = "tb_%dx%dx%d_c%d" % (M, K_, N, len(cshape))
            add("gemm", n, "Gemm", [rn(n + "a", M, K_), K(rn(n + "b", N, K_)), K(rn(n + "c", *cshape))], transB=1)
    add("gemm", "tn_5x7x3", "Gemm", [rn("g1a", 5, 7), K(rn("g1b", 7, 3)), K(rn("g1c", 3))])  # transB = 0: b_kn, path 0
    add("gemm", "tn_8x8x8", "Gemm", [rn("g2a", 8, 8), K(rn("g2b", 8, 8)), K(rn("g2c", 1, 8))], transB=0)  # path 2
    add("gemm", "no_c", "Gemm", [rn("g3a", 4, 6), K(rn("g3b", 5, 6))], transB=1)
    add("gemm", "c_column_m_eq_n", "Gemm", [rn("g4a", 5, 8), K(rn("g4b", 5, 8)), K(rn("g4c", 5, 1))], transB=1, refuse=["Gemm", "C"], either=True)
    add("gemm", "alpha", "Gemm", [rn("g5a", 3, 4), K(rn("g5b", 4, 2))], alpha=0.5, refuse=["Gemm", "alpha"])
    add("gemm", "beta", "Gemm", [rn("g6a", 3, 4), K(rn("g6b", 4, 2)), K(rn("g6c", 2))], beta=2.0, refuse=["Gemm", "beta"])
    add("gemm", "transA", "Gemm", [rn("g7a", 4, 3), K(rn("g7b", 4, 2))], transA=1, refuse=["Gemm", "transA"])

    # ---------------------------------------------------------------- dense Conv 2-D: im2col (K1 = roundup4(K + 1)) + the GEMM, [N][K] weights, path 1
    def conv(group, name, xs, ws, /, bias=True, **attrs):
        x, w = rn(name + "x", *xs), rn(name + "w", *ws) / np.float32(np.sqrt(np.prod(ws[1:])))
        add(group, name, "Conv", [x, K(w)] + ([K(rn(name + "b", ws[0]))] if bias else []), **attrs)
    conv("conv_dense", "c1_k1", (1, 1, 7, 9), (4, 1, 1, 1))                       # K = 1, K1 = 4
    conv("conv_dense", "c3_k3", (1, 3, 7, 9), (4, 3, 3, 3))                       # K = 27, K1 = 28
    conv("conv_dense", "c5_k1x3", (1, 5, 7, 9), (4, 5, 1, 3))
    conv("conv_dense", "batch2", (2, 3, 7, 9), (4, 3, 3, 3))
    conv("conv_dense", "strides_2_1", (1, 3, 7, 9), (4, 3, 3, 3), strides=[2, 1])
    conv("conv_dense", "pads_0123", (1, 3, 7, 9), (4, 3, 3, 3), pads=[0, 1, 2, 3])
    conv("conv_dense", "dilations_2_3", (1, 3, 7, 9), (4, 3, 3, 3), dilations=[2, 3])
    conv("conv_dense", "no_bias", (1, 3, 7, 9), (4, 3, 3, 3), bias=False)
    # stride 2 on even extents (8 x 10): the total pad is 1 per axis, SAME_UPPER puts it at the end, SAME_LOWER at the beginning
    conv("conv_dense", "same_upper", (1, 3, 8, 10), (4, 3, 3, 3), strides=[2, 2], auto_pad="SAME_UPPER")
    conv("conv_dense", "same_lower", (1, 3, 8, 10), (4, 3, 3, 3), strides=[2, 2], auto_pad="SAME_LOWER")
    conv("conv_dense", "same_upper_odd_in", (1, 3, 7, 9), (4, 3, 3, 3), strides=[2, 2], auto_pad="SAME_UPPER")  # even total pad
    conv("conv_dense", "valid", (1, 3, 7, 9), (4, 3, 3, 3), auto_pad="VALID")
    conv("conv_dense", "m256_big", (1, 3, 10, 10), (256, 3, 3, 3), pads=[1, 1, 1, 1])   # GEMM M = 256, N = 100: k_gemm_f32_big
    conv("conv_dense", "m256_small_n", (1, 3, 10, 10), (256, 3, 3, 3))                  # N = 64 < 96: k_gemm_f32
    conv("conv_dense", "m512_tall", (1, 1, 7, 9), (512, 1, 1, 1))                       # GEMM M = 512, N = 63: k_gemm_f32_tall NT = 2

    # ---------------------------------------------------------------- grouped Conv (k_oe_conv2d_direct), Conv 1-D (k_vg_conv1d)
    conv("conv_grouped", "groups2", (1, 4, 7, 9), (6, 2, 3, 3), group=2)
    conv("conv_grouped", "depthwise_x2", (1, 3, 7, 9), (6, 1, 3, 3), group=3)
    conv("conv_grouped", "dil2_n2_asym_pads", (2, 4, 7, 9), (6, 2, 3, 3), group=2, dilations=[2, 2], pads=[1, 0, 2, 3])
    conv("conv_grouped", "strides_no_bias", (1, 4, 7, 9), (4, 1, 3, 2), group=4, strides=[2, 3], bias=False)
    conv("conv1d", "base", (1, 3, 20), (4, 3, 3))
    conv("conv1d", "dilation2", (1, 3, 20), (4, 3, 3), dilations=[2])
    conv("conv1d", "stride3", (1, 3, 20), (4, 3, 3), strides=[3])
    conv("conv1d", "pads_2_0", (1, 3, 20), (4, 3, 3), pads=[2, 0])
    conv("conv1d", "no_bias", (1, 3, 20), (4, 3, 3), bias=False)
    conv("conv1d", "k1", (1, 3, 20), (4, 3, 1))
    conv("conv1d", "all", (1, 2, 131), (3, 2, 5), dilations=[2], strides=[3], pads=[2, 1])  # more than one 128-thread block

    # ---------------------------------------------------------------- ConvTranspose (k_sq_conv_transpose)
    def convt(name, xs, ws, bias=True, refuse=None, **attrs):
        x, w = rn(name + "x", *xs), rn(name + "w", *ws) / np.float32(np.sqrt(ws[0] * ws[2] * ws[3]))
        add("conv_transpose", name, "ConvTranspose", [x, K(w)] + ([K(rn(name + "b", ws[1]))] if bias else []), refuse=refuse, **attrs)
    convt("base", (1, 3, 4, 5), (3, 2, 3, 3))
    convt("strides_2_3", (1, 3, 4, 5), (3, 2, 3, 3), strides=[2, 3])
    convt("pads_0120", (1, 3, 4, 5), (3, 2, 3, 3), strides=[2, 3], pads=[0, 1, 2, 0])
    convt("output_padding_1_2", (1, 3, 4, 5), (3, 2, 3, 3), strides=[2, 3], output_padding=[1, 2])
    convt("batch2", (2, 3, 4, 5), (3, 2, 3, 3), strides=[2, 2])
    convt("no_bias", (1, 3, 4, 5), (3, 2, 3, 3), bias=False)
    convt("k1", (1, 3, 4, 5), (3, 2, 1, 1), strides=[2, 2])
    convt("output_shape_agrees", (1, 3, 4, 5), (3, 2, 3, 3), strides=[2, 2], output_shape=[9, 11])
    convt("output_shape_disagrees", (1, 3, 4, 5), (3, 2, 3, 3), strides=[2, 2], output_shape=[10, 12], refuse=["ConvTranspose", "output_shape"])

    # ---------------------------------------------------------------- pools (k_oe_pool, k_oe_gap)
    neg = -np.abs(rn("negx", 1, 2, 7, 7)) - np.float32(0.5)
    add("pool_max", "all_negative_pads", "MaxPool", [neg], kernel_shape=[3, 3], pads=[1, 1, 1, 1])          # a pad cell must never win
    add("pool_max", "all_negative_asym", "MaxPool", [neg], kernel_shape=[3, 2], pads=[0, 1, 2, 1], strides=[2, 1])
    add("pool_max", "ceil_k2_s2", "MaxPool", [rn("mp1", 1, 2, 7, 7)], kernel_shape=[2, 2], strides=[2, 2], ceil_mode=1)
    add("pool_max", "ceil_k3_s2_p1", "MaxPool", [rn("mp2", 1, 2, 7, 7)], kernel_shape=[3, 3], strides=[2, 2], pads=[1, 1, 1, 1], ceil_mode=1)
    add("pool_max", "floor_k2_s2", "MaxPool", [rn("mp3", 2, 2, 7, 7)], kernel_shape=[2, 2], strides=[2, 2])
    for cip in (0, 1):
        add("pool_avg", "pads_0121_cip%d" % cip, "AveragePool", [rn("ap1", 1, 2, 7, 7)], kernel_shape=[3, 3], pads=[0, 1, 2, 1], count_include_pad=cip)
        add("pool_avg", "ceil_k3_s2_p1_cip%d" % cip, "AveragePool", [rn("ap2", 1, 2, 7, 7)], kernel_shape=[3, 3], strides=[2, 2], pads=[1, 1, 1, 1],
            ceil_mode=1, count_include_pad=cip)
        # the last window of each axis reaches one cell past the (unpadded) extent: that cell is never counted
        add("pool_avg", "ceil_k2_s2_cip%d" % cip, "AveragePool", [rn("ap3", 1, 2, 7, 7)], kernel_shape=[2, 2], strides=[2, 2], ceil_mode=1, count_include_pad=cip)
        add("pool_avg", "ceil_k3_s2_p0011_cip%d" % cip, "AveragePool", [rn("ap4", 1, 2, 7, 7)], kernel_shape=[3, 3], strides=[2, 2], pads=[0, 0, 1, 1],
            ceil_mode=1, count_include_pad=cip)
    for shape in [(1, 3, 1, 1), (1, 3, 15, 17), (1, 3, 16, 16), (1, 3, 1, 257), (3, 1, 25, 40)]:  # H W = 1, 255, 256, 257, 1000
        add("gap", "hw%d" % (shape[2] * shape[3]), "GlobalAveragePool", [rn("gap%d" % shape[3], *shape)])

    # ---------------------------------------------------------------- Resize / Upsample (k_oe_resize) on a 5 x 7 input
    x57 = rn("x57", 1, 2, 5, 7)
    cts = ["half_pixel", "pytorch_half_pixel", "align_corners", "asymmetric"]
    for nm in ["round_prefer_floor", "floor", "ceil", "round_prefer_ceil"]:
        for ct in cts:
            for sc in (2.0, 1.5, 0.5):
                add("resize_nearest", "%s_%s_x%g" % (nm, ct, sc), "Resize", [x57, None, K([1, 1, sc, sc])], mode="nearest", nearest_mode=nm, coordinate_transformation_mode=ct)
    for mode in ("nearest", "linear"):
        for ct in cts:
            add("resize_sizes", "%s_%s_7x5" % (mode, ct), "Resize", [x57, None, None, I([1, 2, 7, 5])], mode=mode, coordinate_transformation_mode=ct)
            add("resize_sizes", "%s_%s_1x1" % (mode, ct), "Resize", [x57, None, None, I([1, 2, 1, 1])], mode=mode, coordinate_transformation_mode=ct)
    x88 = rn("x88", 1, 2, 8, 8)
    for ct in cts:
        for sc in (2.0, 1.6):
            add("resize_linear", "%s_x%g" % (ct, sc), "Resize", [x57, None, K([1, 1, sc, sc])], mode="linear", coordinate_transformation_mode=ct)
        add("resize_linear", "%s_8to3" % ct, "Resize", [x88, None, None, I([1, 2, 3, 3])], mode="linear", coordinate_transformation_mode=ct)
    add("upsample", "scales_input", "Upsample", [x57, K([1, 1, 2, 2])], opset=9, mode="nearest")
    add("upsample", "scales_attr", "Upsample", [x57], opset=7, mode="nearest", scales=[1.0, 1.0, 2.0, 3.0])
    add("upsample", "linear", "Upsample", [x57, K([1, 1, 2, 2])], opset=9, mode="linear")
    add("upsample", "resize_opset10", "Resize", [x57, K([1, 1, 2, 1.5])], opset=10, mode="nearest")
    add("upsample", "resize_opset10_linear", "Resize", [x57, K([1, 1, 1.6, 2])], opset=10, mode="linear")

    # ---------------------------------------------------------------- Pad (k_oe_pad4, k_vg_pad_last)
    xp = rn("xp", 1, 2, 5, 4)
    add("pad", "reflect_hw", "Pad", [xp, I([0, 0, 1, 3, 0, 0, 2, 0])], mode="reflect")            # W: pad 3 = dim - 1
    add("pad", "reflect_hw_attr", "Pad", [xp], opset=2, mode="reflect", pads=[0, 0, 4, 1, 0, 0, 0, 3])  # H: pad 4 = dim - 1
    add("pad", "const_attr", "Pad", [xp], opset=2, pads=[0, 1, 1, 0, 0, 0, 2, 3], value=2.5)
    add("pad", "const_input", "Pad", [xp, I([0, 1, 1, 0, 0, 0, 2, 3]), K(np.float32(2.5).reshape(()))])
    add("pad", "const_default_zero", "Pad", [xp, I([1, 0, 0, 2, 0, 0, 1, 0])])
    add("pad", "last_rank3_const", "Pad", [rn("xp3", 2, 3, 6), I([0, 0, 2, 0, 0, 3]), K(np.float32(2.5).reshape(()))])
    add("pad", "last_rank3_reflect", "Pad", [rn("xp3", 2, 3, 6), I([0, 0, 5, 0, 0, 2])], mode="reflect")
    add("pad", "last_rank2_const", "Pad", [rn("xp2", 3, 6), I([0, 1, 0, 4])])
    add("pad", "last_rank2_reflect", "Pad", [rn("xp2", 3, 6), I([0, 1, 0, 5])], mode="reflect")
    add("pad", "last_rank1", "Pad", [rn("xp1", 300), I([7, 9])], mode="reflect")
    add("pad", "reflect_too_wide_4d", "Pad", [xp, I([0, 0, 5, 0, 0, 0, 0, 0])], mode="reflect", refuse=["Pad", "pads"])
    add("pad", "reflect_too_wide_last", "Pad", [rn("xp2", 3, 6), I([0, 0, 0, 6])], mode="reflect", refuse=["Pad", "pads"])

    # ---------------------------------------------------------------- Softmax (tk_launch_softmax_rows: wave, reg, plain; k_oe_softmax_axis)
    for rows, cols, where in [(1025, 4, "wave kernel, row tail"), (1025, 12, "wave"), (1024, 8, "wave, the rows threshold"), (1023, 8, "reg: one row under it"),
                              (1025, 6, "reg: cols % 4 != 0"), (3, 1, "reg"), (3, 3, "reg"), (3, 255, "reg"), (3, 257, "reg"), (3, 2048, "reg, its widest row"),
                              (2, 2049, "plain")]:
        add("softmax", "%dx%d" % (rows, cols), "Softmax", [rn("sm%d_%d" % (rows, cols), rows, cols)])
    add("softmax", "inner_axis1", "Softmax", [rn("sma", 2, 5, 3)], axis=1)
    add("softmax", "inner_axis0", "Softmax", [rn("sma", 2, 5, 3)], axis=0)
    add("softmax", "inner_many_pairs", "Softmax", [rn("smb", 3, 16, 50)], axis=1)   # 150 (outer, inner) pairs: two blocks
    big = rn("smc", 4, 9)
    big[1, 4] += 90.0                                                                # without the max subtraction exp overflows
    add("softmax", "one_entry_90_above", "Softmax", [big])
    bigc = rn("smd", 2, 9, 3)
    bigc[1, 4, 2] += 90.0
    add("softmax", "one_entry_90_above_inner", "Softmax", [bigc], axis=1)
    eq = rn("sme", 3, 7)
    eq[1, :] = 1.25
    add("softmax", "equal_row", "Softmax", [eq])
    add("softmax", "opset11_rank3_axis1", "Softmax", [rn("smf", 2, 5, 3)], opset=11, axis=1, refuse=["Softmax", "opset"], either=True)
    add("softmax", "opset11_rank3_default_axis", "Softmax", [rn("smg", 2, 5, 3)], opset=11, refuse=["Softmax", "opset"], either=True)
    add("softmax", "opset11_rank2", "Softmax", [rn("smh", 4, 6)], opset=11, axis=1)

    # ---------------------------------------------------------------- reductions (k_vg_reduce_mean, k_sq_reduce) and norms
    x4 = rn("red4", 2, 3, 4, 5)
    for op in ("ReduceMean", "ReduceSum", "ReduceL2", "ReduceMax", "ReduceMin"):
        src = -np.abs(x4) - np.float32(0.25) if op == "ReduceMax" else x4           # all-negative data: a 0 seed would win
        o11 = 11                                                                     # axes as an attribute (ReduceSum up to opset 12, the others up to 17)
        add("reduce", op + "_attr_12_keep", op, [src], opset=o11, axes=[1, 2], keepdims=1)
        add("reduce", op + "_attr_12_drop", op, [src], opset=o11, axes=[1, 2], keepdims=0)
        add("reduce", op + "_input_0_drop", op, [src, I([0])], opset=18, keepdims=0)
        add("reduce", op + "_input_last_keep", op, [src, I([-1])], opset=18, keepdims=1)
        add("reduce", op + "_all_axes", op, [src], opset=18, keepdims=0)
        add("reduce", op + "_noop_empty_axes", op, [src, I([], [0])], opset=18, noop_with_empty_axes=1)
        add("reduce", op + "_empty_axes_all", op, [src, I([], [0])], opset=18, keepdims=1)
        add("reduce", op + "_non_adjacent", op, [src], opset=11, axes=[0, 2], refuse=[op, "axes"])
    for D in (1, 3, 256, 257, 1030):
        add("layernorm", "d%d" % D, "LayerNormalization", [rn("ln%d" % D, 3, D), K(rn("lns%d" % D, D)), K(rn("lnb%d" % D, D))])
    add("layernorm", "no_bias", "LayerNormalization", [rn("ln_nb", 2, 3, 20), K(rn("lns_nb", 20))])
    add("layernorm", "epsilon", "LayerNormalization", [rn("ln_e", 4, 33) * np.float32(0.01), K(rn("lns_e", 33)), K(rn("lnb_e", 33))], epsilon=1e-3)
    for shape in [(2, 3, 4, 5), (1, 3, 7)]:
        r = rng_for("bn%d" % len(shape))
        add("batchnorm", "rank%d" % len(shape), "BatchNormalization", [rn("bnx%d" % len(shape), *shape), K(r.standard_normal(3)), K(r.standard_normal(3)),
                                                                        K(r.standard_normal(3)), K(r.uniform(0.5, 1.5, 3))])
    add("batchnorm", "epsilon", "BatchNormalization", [rn("bnxe", 2, 3, 4, 5), K([1.5, -2, 0.5]), K([0.1, 0.2, -0.3]), K([0.5, -0.5, 0]), K([0.01, 0.02, 0.005])], epsilon=1e-2)

    # ---------------------------------------------------------------- elementwise: broadcasting, Pow, unary
    for op in ("Add", "Sub", "Mul", "Div"):
        add("broadcast", op + "_2141_315", op, [rn("b1", 2, 1, 4, 1), rn("b2", 3, 1, 5)])
        add("broadcast", op + "_scalar_rank4", op, [rn("b3", 1).reshape(()), rn("b4", 2, 3, 4, 5)])
        add("broadcast", op + "_rank4_scalar1", op, [rn("b4", 2, 3, 4, 5), rn("b5", 1)])
        add("broadcast", op + "_rank6", op, [rn("b6", 2, 1, 3, 1, 2, 3), rn("b7", 2, 1, 2, 1, 3)])
        add("broadcast", op + "_both", op, [rn("b8", 4, 1), rn("b9", 1, 5)])
    for op in ("Max", "Min"):
        add("broadcast", op + "_2141_315", op, [rn("b1", 2, 1, 4, 1), rn("b2", 3, 1, 5)])
    pos = rng_for("powpos").uniform(0.1, 10.0, (4, 33)).astype(np.float32)
    for z in (2.0, 1.0, 0.5, 0.0, 3.0, -1.0, -1.5, 7.3):
        add("pow", "positive_z%g" % z, "Pow", [pos, K(np.float32(z).reshape(()))])
    negb = -pos
    for z in (3.0, 4.0, -1.0, 2.0, 1.0):
        add("pow", "negative_z%g" % z, "Pow", [negb, K(np.float32(z).reshape(()))])
    add("pow", "zero_base_z3", "Pow", [np.zeros((2, 3), np.float32), K(np.float32(3.0).reshape(()))])
    add("pow", "ten_7.3", "Pow", [np.full((1,), 10.0, np.float32), K(np.float32(7.3).reshape(()))])
    add("pow", "tensor_exponent", "Pow", [np.array([[-2.0], [2.0], [0.5]], np.float32), np.array([3.0, 2.0, -2.0, 4.0, 1.0], np.float32)])

    add("unary", "Sigmoid_points", "Sigmoid", [np.array([0, 20, -20, 100, -100], np.float32)])
    add("unary", "Sigmoid_normal", "Sigmoid", [rn("u1", 300) * np.float32(3)])
    add("unary", "Tanh_points", "Tanh", [np.array([1e-4, -1e-4, 0.5, -0.5, 20, -20], np.float32)])
    add("unary", "Tanh_normal", "Tanh", [rn("u2", 300) * np.float32(3)])
    add("unary", "Exp_range", "Exp", [np.linspace(-87, 88, 701).astype(np.float32)])
    add("unary", "Log_range", "Log", [np.geomspace(1e-30, 1e30, 601).astype(np.float32)])
    add("unary", "Sqrt_range", "Sqrt", [np.geomspace(1e-30, 1e30, 601).astype(np.float32)])
    for op, at in [("Erf", {}), ("Gelu", {}), ("Gelu", {"approximate": "tanh"})]:
        add("unary", op + "_" + at.get("approximate", "exact"), op, [np.linspace(-6, 6, 481).astype(np.float32)], opset=20, **at)
    xu = rn("u3", 3, 50) * np.float32(4)
    add("unary", "HardSigmoid_default", "HardSigmoid", [xu])
    add("unary", "HardSigmoid_alpha_beta", "HardSigmoid", [xu], alpha=0.25, beta=0.4)
    add("unary", "HardSwish", "HardSwish", [xu])
    add("unary", "Clip_attr", "Clip", [xu], opset=6, min=-1.5, max=2.25)
    add("unary", "Clip_input", "Clip", [xu, K(np.float32(-1.5).reshape(())), K(np.float32(2.25).reshape(()))])
    add("unary", "Clip_min_only", "Clip", [xu, K(np.float32(-0.5).reshape(()))])
    add("unary", "Clip_max_only", "Clip", [xu, None, K(np.float32(0.75).reshape(()))])
    add("unary", "Clip_attr_max_only", "Clip", [xu], opset=6, max=0.75)
    add("unary", "Clip_unbounded", "Clip", [xu])
    add("unary", "LeakyRelu_default", "LeakyRelu", [xu])
    add("unary", "LeakyRelu_alpha", "LeakyRelu", [xu], alpha=0.2)
    for op in ("Relu", "Abs", "Neg"):
        add("unary", op, op, [xu])
    # IEEE results at the edges of the domains (what ONNX Runtime gives)
    add("domain", "Log", "Log", [np.array([0.0, -1.0, -np.inf, np.inf, 1e-40, 1.4e-45, 1.1754942e-38, 1.0], np.float32)])
    add("domain", "Sqrt", "Sqrt", [np.array([-1.0, -1e-40, np.inf, 0.0, 1e-40, 1.4e-45, 1.1754942e-38, 3.4e38], np.float32)])
    add("domain", "Exp", "Exp", [np.array([88.73, 89.0, 100.0, np.inf, -104.0, -110.0, -np.inf, 0.0], np.float32)])
    add("domain", "NaN_passes", "Exp", [np.array([np.nan, 1.0], np.float32)])

    # ---------------------------------------------------------------- layout / index
    xg = rn("xg", 4, 5, 3)
    add("gather", "negative_indices", "Gather", [xg, I([-1, 0, -4])])
    add("gather", "axis1_rank3", "Gather", [xg, I([4, 0, 2, 2])], axis=1)
    add("gather", "indices_2d", "Gather", [xg, I([0, 2, 1, 1, 4, 3], [2, 3])], axis=1)
    add("gather", "scalar_index", "Gather", [xg, I([2], [])], axis=1)                 # the rank drops
    add("gather", "last_axis", "Gather", [xg, I([2, -3])], axis=-1)
    add("gather", "out_of_range", "Gather", [xg, I([5])], axis=1, refuse=["Gather", "ind"])
    add("gather", "out_of_range_negative", "Gather", [xg, I([-6])], axis=1, refuse=["Gather", "ind"])
    add("layout", "Expand_higher_rank", "Expand", [rn("xe", 3, 1), I([2, 3, 4])])
    add("layout", "Expand_ones_keep", "Expand", [rn("xe2", 2, 3), I([1, 1])])
    wmask = [1, 0, 0, 1, 1, 0, 1, 0, 0, 0, 1, 1]
    add("layout", "Where_const_mask", "Where", [Bm(wmask, [3, 4]), rn("w1", 3, 4), rn("w2", 3, 4)])
    add("layout", "Where_mask_broadcast", "Where", [Bm([1, 0, 1, 1], [4]), rn("w3", 3, 4), rn("w4", 1)])
    xw = rn("w5", 4, 5)
    CASES.append(Case("layout", "Where_greater_mask", [nd("Greater", ["x0", "k"], ["m"]), nd("Where", ["m", "x1", "x2"], ["y"])],
                      {"x0": xw, "x1": rn("w6", 4, 5), "x2": rn("w7", 4, 5)}, {"k": np.float32(0.1).reshape(())}, {}, ["y"]))
    xs7 = rn("xs7", 2, 7, 3)
    add("layout", "Split_default_uneven", "Split", [xs7], n_out=2, opset=18, axis=1, num_outputs=2)
    add("layout", "Split_attr", "Split", [xs7], n_out=3, opset=11, axis=1, split=[1, 4, 2])
    add("layout", "Split_input", "Split", [xs7, I([5, 2])], n_out=2, opset=13, axis=1)
    add("layout", "Split_negative_axis", "Split", [xs7, I([2, 1])], n_out=2, opset=13, axis=-1)
    add("layout", "Concat_negative_axis", "Concat", [rn("c1", 2, 3, 2), rn("c2", 2, 3, 5)], axis=-1)
    add("layout", "Concat_rank6", "Concat", [rn("c3", 2, 1, 3, 2, 2, 3), rn("c4", 2, 1, 1, 2, 2, 3), rn("c5", 2, 1, 2, 2, 2, 3)], axis=2)
    add("layout", "Transpose_default", "Transpose", [rn("t1", 2, 3, 4)])
    add("layout", "Transpose_rank6", "Transpose", [rn("t2", 2, 3, 2, 4, 3, 2)], perm=[0, 2, 4, 1, 5, 3])
    xs = rn("xsl", 6, 7, 5)
    add("slice", "negative_start_end", "Slice", [xs, I([-5, -6]), I([-1, -2]), I([0, 1])])
    add("slice", "end_int64_max", "Slice", [xs, I([2]), I([INT64_MAX]), I([1])])
    add("slice", "beyond_bounds", "Slice", [xs, I([-100, 3]), I([100, 1000]), I([0, 2])])
    add("slice", "omitted_axes", "Slice", [xs, I([1, 2]), I([5, 6])])
    add("slice", "negative_axis", "Slice", [xs, I([1]), I([4]), I([-1])])
    add("slice", "attrs_opset1", "Slice", [xs], opset=1, starts=[1, 0], ends=[INT64_MAX, 3], axes=[0, 2])
    add("slice", "steps_2_3", "Slice", [xs, I([0, 1]), I([INT64_MAX, 7]), I([1, 0]), I([2, 3])])   # 7 / 2 and 5 / 3 leave remainders
    add("slice", "step_2_negative_bounds", "Slice", [xs, I([-6]), I([-1]), I([1]), I([2])])
    add("slice", "empty_result", "Slice", [xs, I([4]), I([2]), I([0])])
    add("slice", "negative_step", "Slice", [xs, I([5]), I([0]), I([0]), I([-1])], refuse=["Slice", "step"])
    add("layout", "Squeeze_no_axes", "Squeeze", [rn("q1", 1, 3, 1, 2)], opset=13)
    add("layout", "Squeeze_axes_input", "Squeeze", [rn("q1", 1, 3, 1, 2), I([-2])], opset=13)
    add("layout", "Unsqueeze_unsorted_negative", "Unsqueeze", [rn("q2", 3, 2), I([-1, 0, -3])], opset=13)
    add("layout", "Unsqueeze_attr", "Unsqueeze", [rn("q2", 3, 2)], opset=11, axes=[1])
    xf = rn("q3", 2, 3, 4)
    for ax in (0, 2, -1, 1):
        add("layout", "Flatten_axis%d" % ax, "Flatten", [xf], axis=ax)
    add("layout", "Reshape_0_and_minus1", "Reshape", [xf, I([0, -1, 2])])
    add("layout", "Reshape_minus1", "Reshape", [xf, I([-1])])
    add("layout", "Identity", "Identity", [xf])

    # ---------------------------------------------------------------- LSTM (k_vg_lstm: one workgroup of 4H threads)
    def lstm(name, T, I_, H, bias, init):
        r = rng_for("lstm" + name)
        g = lambda *s: (r.standard_normal(s) / np.sqrt(s[-1])).astype(np.float32)
        ins = [g(T, 1, I_) * np.float32(np.sqrt(I_)), K(g(1, 4 * H, I_)), K(g(1, 4 * H, H)), K(g(1, 8 * H)) if bias else None, None]
        ins += [g(1, 1, H), g(1, 1, H)] if init else []
        add("lstm", name, "LSTM", ins, n_out=3, hidden_size=H)
    for T in (1, 3):
        for bias in (False, True):
            for init in (False, True):
                lstm("t%d_b%d_s%d" % (T, bias, init), T, 5, 4, bias, init)
    lstm("h256_t1", 1, 5, 256, True, True)      # 1024 threads: the workgroup limit
    lstm("h256_t2", 2, 5, 256, True, False)

    # ---------------------------------------------------------------- attributes of the wrong length: refused (or applied per the spec), never ignored
    xa, wa = rn("al_x", 1, 3, 7, 9), rn("al_w", 4, 3, 3, 3)
    add("attr_len", "Conv_pads2", "Conv", [xa, K(wa)], pads=[1, 1], refuse=["Conv", "pads"], either=True)
    add("attr_len", "Conv_strides1", "Conv", [xa, K(wa)], strides=[2], refuse=["Conv", "strides"], either=True)
    add("attr_len", "Conv_dilations1", "Conv", [xa, K(wa)], dilations=[2], refuse=["Conv", "dilations"], either=True)
    add("attr_len", "MaxPool_pads2", "MaxPool", [xa], kernel_shape=[3, 3], pads=[1, 1], refuse=["MaxPool", "pads"], either=True)
    add("attr_len", "MaxPool_strides1", "MaxPool", [xa], kernel_shape=[3, 3], strides=[2], refuse=["MaxPool", "strides"], either=True)
    add("attr_len", "AveragePool_pads2", "AveragePool", [xa], kernel_shape=[3, 3], pads=[1, 1], refuse=["AveragePool", "pads"], either=True)
    wt = rn("al_wt", 3, 2, 3, 3)
    add("attr_len", "ConvTranspose_pads2", "ConvTranspose", [xa, K(wt)], pads=[1, 1], refuse=["ConvTranspose", "pads"], either=True)
    add("attr_len", "ConvTranspose_strides1", "ConvTranspose", [xa, K(wt)], strides=[2], refuse=["ConvTranspose", "strides"], either=True)
    add("attr_len", "Conv1d_pads1", "Conv", [rn("al_x1", 1, 3, 20), K(rn("al_w1", 4, 3, 3))], pads=[1], refuse=["Conv", "pads"], either=True)


_build()
GROUPS = sorted({c.group for c in CASES})


def cases_of(group):
    return [c for c in CASES if c.group == group]
