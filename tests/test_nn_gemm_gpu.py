"""Every perception GEMM kernel and the fused split-f16 attention, ONE launch at a time (tk_mi355x_gemm_probe, tk_mi355x_attention_h3_probe).

Exact kernels (k_gemm_f32, k_gemm_f32_tall, k_gemm_f32_big; every PATH, implicit im2col, batching, pitches, f16 B): bit for bit the oracle's
chain on the same operands; within the fp32 running-error bound of the float64 result (no oracle involved); C cells the launch does not own
keep their sentinel; the launcher reports the instantiation the case is there for.
Fast kernels (k_gemm_h3_tall, k_gemm_h3_big, k_attention_h3): within the bounds tests/split_f16_ref.py derives from the documented scheme —
the bounds tests/test_split_f16_cpu.py shows to be met by the scheme and missed by each of its mutations.  All elements, no sampling.
Each fast test prints its worst error / bound ratio (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

import nn_gemm_cases as NC
import oracle_lib as O
import split_f16_ref as R
from trackiellm_amd import GEMM_F32 as F32, GEMM_F32_TALL as TALL, GEMM_F32_BIG as BIG, GEMM_H3_TALL as H3_TALL, GEMM_H3_BIG as H3_BIG, gemm_code as code

pytestmark = pytest.mark.gpu


def run(gpu, built, **override):
    kw = dict(built["kw"])
    kw.update(override)
    c, kernel = gpu.gemm_probe(**kw)
    c = c.reshape(-1)
    assert np.array_equal(c[built["untouched"]].view(np.uint32), np.full(built["untouched"].size, NC.SENTINEL, np.float32).view(np.uint32)), \
        "a C cell outside the launch's M x N (per member) was written"
    assert built["untouched"].size > 0
    return c, kernel


def check_exact(gpu, want_code, **case):
    built = NC.build_gemm(seed=case.pop("seed", 3), **case)
    c, kernel = run(gpu, built)
    assert kernel == want_code, (kernel, want_code)
    for z, m in enumerate(built["members"]):
        got = c[m["cidx"]]
        want = O.gemm(m["A"], m["B"].T if case.get("b_kn") else m["B"], built["bias"], m["R"], bool(case.get("b_kn")), built["act"], built["alpha"])
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (z, len(bad), bad[:4].tolist(), [(float(got[i, j]), float(want[i, j])) for i, j in bad[:4]])
        acc, S, _, v64 = R.ref_gemm64(m["A"], m["B"], built["bias"], m["R"], built["act"], built["alpha"])
        bound = R.epilogue_bound(acc, R.chain_acc_bound(S, built["K"]), built["bias"], m["R"], built["act"], built["alpha"])
        over = np.argwhere(np.abs(got.astype(np.float64) - v64) > bound)
        assert over.size == 0, (z, len(over), over[:4].tolist())


# ---------------------------------------------------------------- exact kernels
@pytest.mark.parametrize("case,path", [
    (dict(M=65, N=67, K=30), 0),                                   # K % 4 != 0
    (dict(M=65, N=67, K=30, lda=31, ldb=33), 0),                   # odd pitches
    (dict(M=65, N=67, K=30, a_offset=1), 0),                       # bases off 16 bytes
    (dict(M=65, N=67, K=32, b_offset=1, bias=True), 0),
    (dict(M=65, N=67, K=32, lda=36, ldb=40, bias=True, act=1), 1),  # aligned pitches wider than K
    (dict(M=65, N=68, K=32, b_kn=True, bias=True), 2),
    (dict(M=65, N=67, K=32, b_kn=True, residual=True, ldr=70), 0),
    (dict(M=65, N=68, K=30, b_kn=True, ldb=71), 0),
])
def test_gemm_f32_paths(gpu, case, path):
    check_exact(gpu, code(F32, path=path), ldc=case["N"] + 3, **case)


def test_gemm_f32_f16_weights(gpu):
    check_exact(gpu, code(F32, path=0), M=33, N=67, K=132, b_f16=True, ldc=70, bias=True)
    check_exact(gpu, code(F32, path=0), M=33, N=68, K=130, b_f16=True, b_kn=True, ldc=70)


@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_gemm_f32_big_epilogue(gpu, act):
    check_exact(gpu, code(BIG, path=1), M=257, N=97, K=36, ldc=97 + 5, bias=True, residual=True, ldr=97 + 2, act=act)


def test_gemm_f32_big_paths(gpu):
    check_exact(gpu, code(BIG, path=0), M=257, N=97, K=34, ldc=100, bias=True)
    check_exact(gpu, code(BIG, path=0), M=257, N=97, K=36, ldc=100, a_offset=1, alpha=0.5)
    check_exact(gpu, code(BIG, path=2), M=257, N=100, K=36, b_kn=True, ldc=101)
    check_exact(gpu, code(BIG, path=0), M=257, N=97, K=36, b_kn=True, ldc=101)
    check_exact(gpu, code(BIG, path=0), M=257, N=97, K=36, b_f16=True, ldc=101)


@pytest.mark.parametrize("N", [31, 33, 64, 95])
def test_gemm_f32_tall(gpu, N):
    nt = (N + 31) // 32
    check_exact(gpu, code(TALL, path=1, nt=nt), M=513, N=N, K=144, ldc=N + 1, bias=True, act=1)
    check_exact(gpu, code(TALL, path=0, nt=nt), M=513, N=N, K=144, lda=145, ldc=N + 1, residual=True, ldr=N + 2)
    check_exact(gpu, code(TALL, path=0, nt=nt), M=513, N=N, K=142, ldc=N + 1)


def test_gemm_two_level_batch(gpu):
    """the Whisper attention launches: Q K^T (alpha = 1/8, [N][K] keys) and P V ([K][N] values, K = the context)"""
    check_exact(gpu, code(F32, path=1), M=50, N=50, K=64, batch=6, inner=3, alpha=0.125, ldc=53)
    check_exact(gpu, code(F32, path=0), M=50, N=64, K=50, batch=6, inner=3, b_kn=True, ldc=64 + 1)
    check_exact(gpu, code(F32, path=2), M=50, N=64, K=52, batch=6, inner=3, b_kn=True, ldc=64 + 1, residual=True)
    check_exact(gpu, code(F32, path=1), M=50, N=50, K=64, batch=4, ldc=53, bias=True)       # one level
    check_exact(gpu, code(BIG, path=1), M=257, N=97, K=36, batch=4, inner=2, ldc=99)


@pytest.mark.parametrize("conv,N,family,nt", [
    (dict(B=2, H=9, W=7, C=8, ldx=8, stride=1), 67, F32, 0),        # M = 126
    (dict(B=2, H=18, W=13, C=4, ldx=8, stride=2), 67, F32, 0),      # M = 126, stride 2, pixel pitch wider than the channels
    (dict(B=2, H=17, W=16, C=4, ldx=4, stride=1), 48, TALL, 2),     # M = 544
    (dict(B=2, H=33, W=32, C=8, ldx=12, stride=2), 48, TALL, 2),    # M = 544
    (dict(B=2, H=16, W=9, C=8, ldx=8, stride=1), 128, BIG, 0),      # M = 288
    (dict(B=2, H=32, W=17, C=4, ldx=4, stride=2), 128, BIG, 0),     # M = 288
])
def test_gemm_implicit_im2col(gpu, conv, N, family, nt):
    """against the explicit column matrix built in NumPy and run through the oracle's chain; K = 9 C: the taps straddle the 32-k slabs"""
    M, K = NC.conv_shape(**conv)
    check_exact(gpu, code(family, im=True, path=1, nt=nt), M=M, N=N, K=K, conv=conv, ldc=N + 3, bias=True, act=1, residual=True, ldr=N + 1)


# ---------------------------------------------------------------- fast kernels
FAST_CASES = NC.fast_gemm_cases()


def fast_ratio(gpu, built, c):
    worst = 0.0
    for m in built["members"]:
        acc, S, T, want = R.ref_gemm64(m["A"], m["B"], built["bias"], m["R"], built["act"], built["alpha"])
        bound = R.epilogue_bound(acc, R.gemm_acc_bound(S, T, built["K"]), built["bias"], m["R"], built["act"], built["alpha"])
        worst = max(worst, float((np.abs(c[m["cidx"]].astype(np.float64) - want) / bound).max()))
    return worst


@pytest.mark.parametrize("kind", NC.KINDS)
@pytest.mark.parametrize("name,case,expect", FAST_CASES, ids=[c[0] for c in FAST_CASES])
def test_fast_gemm_within_the_derived_bound(gpu, name, case, expect, kind):
    built = NC.build_gemm(kind=kind, seed=11, fast=True, **case)
    c, kernel = run(gpu, built)
    assert kernel == NC.code_of(expect)
    worst = fast_ratio(gpu, built, c)
    print(f"RATIO {'h3_tall' if expect[0] == H3_TALL else 'h3_big'} {name} {kind} {worst:.4f}")
    assert worst < 1, (name, kind, worst)


@pytest.mark.parametrize("case,want", [
    (dict(M=65, N=68, K=32, b_kn=True), code(F32, path=2)),                         # [K][N] weights
    (dict(M=257, N=100, K=36, b_kn=True), code(BIG, path=2)),
    (dict(M=65, N=67, K=30), code(F32, path=0)),                                     # no 16-byte groups
    (dict(M=129, N=97, K=36, a_offset=1), code(F32, path=0)),
    (dict(M=50, N=64, K=64, batch=6, inner=3, alpha=0.125), code(F32, path=1)),      # N < 96 with a batch
    (dict(M=513, N=64, K=64, batch=2), code(F32, path=1)),
])
def test_fast_flag_on_an_ineligible_descriptor_keeps_the_exact_chain(gpu, case, want):
    check_exact(gpu, want, fast=True, ldc=case["N"] + 3, **case)


@pytest.mark.parametrize("N,family", [(95, H3_TALL), (129, H3_BIG)])
def test_fast_row_does_not_depend_on_its_launch(gpu, N, family):
    """tk_launch_gemm's promise: a row computed alone (M = 1) has the bits it has among 300 rows"""
    built = NC.build_gemm(M=300, N=N, K=240, seed=13, fast=True, bias=True, act=1, ldc=N + 3)
    c, kernel = run(gpu, built)
    assert kernel // 1000 == family
    m = built["members"][0]
    for i in (0, 31, 127, 128, 255, 256, 299):
        alone = NC.build_gemm(M=1, N=N, K=240, seed=13, fast=True, bias=True, act=1, ldc=N + 3)
        kw = dict(alone["kw"], a=m["A"][i], b=built["kw"]["b"], bias=built["bias"])
        ci, ki = gpu.gemm_probe(**kw)
        assert ki // 1000 == family
        assert np.array_equal(ci.reshape(-1)[alone["members"][0]["cidx"]][0].view(np.uint32), c[m["cidx"]][i].view(np.uint32)), i


# ---------------------------------------------------------------- attention
class _SoftmaxParams(C.Structure):
    _fields_ = [("d_input_tensor", C.c_void_p), ("d_output_tensor", C.c_void_p), ("num_rows", C.c_uint32), ("num_cols", C.c_uint32)]


def softmax_rows(gpu, x):
    d = gpu.RocmDispatcher(0)
    buf = d.malloc(x.nbytes)
    d.upload(buf, x)
    p = _SoftmaxParams(d.ptr(buf), d.ptr(buf), x.shape[0], x.shape[1])
    assert gpu.lib().tk_kernels_softmax(C.byref(p), d.stream()) == 0
    got = d.download(buf, x.shape, np.float32)
    d.free(buf)
    d.close()
    return got


def three_launch_attention(gpu, a):
    """the exact form the fused kernel replaces: batched Q K^T (alpha = scale), row softmax, batched P V — all through the launchers"""
    B, nh, Tq, Tk, d = a["B"], a["nh"], a["Tq"], a["Tk"], a["d"]
    z = B * nh
    inner = nh if B > 1 else 0
    s0 = np.zeros((z * Tq, Tk), np.float32)
    s, k1 = gpu.gemm_probe(a["q"], a["k"], s0, Tq, Tk, 64, lda=d, ldb=d, ldc=Tk, alpha=NC.ATT_SCALE, batch=z, strides=(64, 64, Tq * Tk, 0), batch_inner=inner,
                           strides2=(a["q_bstride"], a["kv_bstride"], nh * Tq * Tk, 0) if inner else (0, 0, 0, 0))
    p = softmax_rows(gpu, s)
    out, k2 = gpu.gemm_probe(p, a["v"], a["out0"], Tq, 64, Tk, lda=Tk, ldb=d, ldc=d, b_kn=True, batch=z, strides=(Tq * Tk, 64, 64, 0), batch_inner=inner,
                             strides2=(nh * Tq * Tk, a["kv_bstride"], a["q_bstride"], 0) if inner else (0, 0, 0, 0))
    assert k1 // 1000 in (F32, BIG) and k2 // 1000 in (F32, BIG)
    return out.reshape(-1)


def check_attention(gpu, a, tag):
    sent = np.full(a["untouched"].size, NC.SENTINEL, np.float32).view(np.uint32)
    fused = gpu.attention_h3_probe(a["q"], a["k"], a["v"], a["out0"], a["B"], a["nh"], a["Tq"], a["Tk"], a["d"], NC.ATT_SCALE, a["q_bstride"], a["kv_bstride"]).reshape(-1)
    exact = three_launch_attention(gpu, a)
    assert np.array_equal(fused[a["untouched"]].view(np.uint32), sent) and np.array_equal(exact[a["untouched"]].view(np.uint32), sent)
    worst = 0.0
    for hd in a["heads"]:
        want, _, _ = R.ref_attention64(hd["q"], hd["k"], hd["v"], NC.ATT_SCALE)
        bf = R.attention_bound(hd["q"], hd["k"], hd["v"], NC.ATT_SCALE)
        be = R.attention_bound(hd["q"], hd["k"], hd["v"], NC.ATT_SCALE, exact=True)
        f, e = fused[hd["oidx"]].astype(np.float64), exact[hd["oidx"]].astype(np.float64)
        rf = np.abs(f - want) / bf
        if rf.max() > worst:
            worst, at = float(rf.max()), np.unravel_index(int(rf.argmax()), rf.shape)
            print(f"  worst so far {worst:.4f} at query {at[0]} (design {at[0] % 6}) dim {at[1]}: error {abs(f - want)[at]:.3e}, output {want[at]:.3e}, {tag}")
        assert rf.max() < 1, (tag, "fused against float64", float(rf.max()), np.argwhere(rf >= 1)[:4].tolist())
        assert (np.abs(e - want) <= be).all(), (tag, "three-launch form against float64", float((np.abs(e - want) / np.maximum(be, 1e-300)).max()))
        assert (np.abs(f - e) <= bf + be).all(), (tag, "fused against the three-launch form")
    return worst


@pytest.mark.parametrize("Tk", NC.ATT_TK)
@pytest.mark.parametrize("Tq", NC.ATT_TQ)
def test_attention_h3_within_the_derived_bound(gpu, Tq, Tk):
    worst = (0.0, None)
    for rows in NC.ATT_ROWS:
        for v_kind in NC.ATT_V_KINDS:
            a = NC.build_attention(1, 1, Tq, Tk, v_kind, seed=5, rows=rows)
            worst = max(worst, (check_attention(gpu, a, (Tq, Tk, rows, v_kind)), f"{rows}/{v_kind}"))
    print(f"RATIO attention_h3 {Tq}x{Tk} {worst[0]:.4f} ({worst[1]})")


def test_attention_h3_heads_sequences_and_strides(gpu):
    """two sequences of two heads, both strides wider than the dense ones: rows >= Tq and the floats between sequences keep their sentinel"""
    a = NC.build_attention(2, 2, 129, 65, "indicator", seed=8, q_gap=128 * 3 + 4, kv_gap=8)
    print(f"RATIO attention_h3 2x2x129x65 {check_attention(gpu, a, 'strided'):.4f}")


def test_attention_h3_at_the_encoder_length(gpu):
    a = NC.build_attention(2, 2, 200, 1500, "one_signed", seed=6, q_gap=64, kv_gap=128)
    print(f"RATIO attention_h3 2x2x200x1500 {check_attention(gpu, a, 'encoder'):.4f}")


def test_attention_probe_refuses_without_writing(gpu):
    fn = gpu.lib().tk_mi355x_attention_h3_probe
    fn.argtypes = [C.c_int] * 5 + [C.c_int64, C.c_int64, C.c_int, C.c_float] + [C.c_void_p] * 3 + [C.c_int64, C.c_int64, C.c_void_p]
    q = np.ones(2 * 4 * 128, np.float32)
    kv = np.ones(2 * 8 * 128, np.float32)
    out = np.full(q.size, NC.SENTINEL, np.float32)
    p = lambda x: x.ctypes.data

    def rc(B=2, nh=2, Tq=4, Tk=8, qb=4 * 128, kb=8 * 128, d=128, nq=q.size, nkv=kv.size):
        return fn(0, B, nh, Tq, Tk, qb, kb, d, 0.125, p(q), p(kv), p(kv), nq, nkv, p(out))

    assert rc(d=64) == 1001 and rc(nh=1) == 1001            # d != 64 nh
    assert rc(qb=4 * 128 + 2, B=1) == 1001 and rc(kb=8 * 128 + 1, B=1) == 1001   # strides that are no multiple of 4
    assert rc(Tq=5) == 1001 and rc(Tk=9) == 1001 and rc(nq=q.size - 1) == 1001 and rc(nkv=kv.size - 1) == 1001
    assert rc(qb=3 * 128) == 1001                           # overlapping sequences
    assert rc(Tq=0) == 1001 and rc(B=0) == 1001 and rc(qb=-4) == 1001
    assert (out == NC.SENTINEL).all()
    assert rc() == 0 and not (out == NC.SENTINEL).any()


def test_gemm_probe_refuses_on_the_device_too(gpu):
    built = NC.build_gemm(M=33, N=35, K=36, seed=2)
    with pytest.raises(gpu.TkError) as e:
        gpu.gemm_probe(**dict(built["kw"], a=built["kw"]["a"][:-1]))
    assert e.value.code == 1001
    with pytest.raises(gpu.TkError):
        gpu.gemm_probe(**dict(built["kw"], device=99))
    M, K = NC.conv_shape(**NC.CONV_TALL)
    conv = NC.build_gemm(M=M, N=48, K=K, conv=NC.CONV_TALL, seed=3)
    with pytest.raises(gpu.TkError) as e:
        gpu.gemm_probe(**dict(conv["kw"], a_offset=1))        # implicit im2col from a misaligned input: refused by the launcher, C unwritten
    assert e.value.code == 1001
