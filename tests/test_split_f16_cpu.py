"""CPU: the bounds of tests/split_f16_ref.py are (a) met by a faithful emulation of the split-f16 scheme at every shape and operand
construction tests/test_nn_gemm_gpu.py uses, and (b) missed, on at least half of the elements of some of those shapes, by every mutation
of the scheme — a dropped product (three in the GEMM / Q K^T contraction, three in P V), a wrong 1 / 2048, a mis-permuted V staging.
A bound that a wrong kernel would pass is not a test.  Also: the launcher's kernel choice (tk_gemm_kernel_of through the probe's
no-device mode) and the probe's argument checks, neither of which needs a GPU."""
import numpy as np
import pytest

import nn_gemm_cases as NC
import split_f16_ref as R

FAST_CASES = NC.fast_gemm_cases()


def _gemm_ratio(case, kind, **mutation):
    """worst |emulation - float64| / bound and the share of elements over the bound, over all batch members"""
    built = NC.build_gemm(kind=kind, seed=11, fast=True, **case)
    worst, over, count = 0.0, 0, 0
    for m in built["members"]:
        acc, S, T, want = R.ref_gemm64(m["A"], m["B"], built["bias"], m["R"], built["act"], built["alpha"])
        bound = R.epilogue_bound(acc, R.gemm_acc_bound(S, T, built["K"]), built["bias"], m["R"], built["act"], built["alpha"])
        got = R.emu_gemm(m["A"], m["B"], built["bias"], m["R"], built["act"], built["alpha"], **mutation)
        ratio = np.abs(got.astype(np.float64) - want) / bound
        worst, over, count = max(worst, float(ratio.max())), over + int((ratio > 1).sum()), count + ratio.size
    return worst, over / count


@pytest.mark.parametrize("kind", NC.KINDS)
@pytest.mark.parametrize("name,case,expect", FAST_CASES, ids=[c[0] for c in FAST_CASES])
def test_emulated_gemm_meets_the_bound(name, case, expect, kind):
    worst, share = _gemm_ratio(case, kind)
    assert share == 0 and worst < 1, (name, kind, worst)


@pytest.mark.parametrize("mutation", [dict(drop="hh"), dict(drop="hl"), dict(drop="lh"), dict(join_scale=1024.0)], ids=["no-hi.hi", "no-hi.lo", "no-lo.hi", "scale-1024"])
@pytest.mark.parametrize("name", ["tall-129x95x240", "tall-127x33x36", "big-129x129x240", "big-batch2"])
def test_mutated_gemm_misses_the_bound_everywhere(name, mutation):
    """with one-signed low halves every element of every shape notices — not just half of them at one shape"""
    case = dict((c[0], c[1]) for c in FAST_CASES)[name]
    worst, share = _gemm_ratio(case, "one_signed", **mutation)
    assert share == 1.0, (name, mutation, worst, share)


def test_emulation_ratio_stays_small_up_to_long_k():
    """tightness: the honest scheme uses a small part of its bound from K = 32 to K = 1536 (so a GPU ratio near 1 would be news)"""
    for K in (32, 240, 1536):
        worst, _ = _gemm_ratio(dict(M=33, N=40, K=K), "one_signed")
        assert worst < 0.25, (K, worst)


# ---- attention ----
ATT_SHAPES = [(Tq, Tk) for Tq in NC.ATT_TQ for Tk in NC.ATT_TK]


def _att_ratio(built, **mutation):
    worst, over, count = 0.0, 0, 0
    for hd in built["heads"]:
        want, _, _ = R.ref_attention64(hd["q"], hd["k"], hd["v"], NC.ATT_SCALE)
        bound = R.attention_bound(hd["q"], hd["k"], hd["v"], NC.ATT_SCALE)
        got = R.emu_attention(hd["q"], hd["k"], hd["v"], NC.ATT_SCALE, **mutation)
        ratio = np.abs(got.astype(np.float64) - want) / bound
        worst, over, count = max(worst, float(ratio.max())), over + int((ratio > 1).sum()), count + ratio.size
    return worst, over / count


@pytest.mark.parametrize("rows", NC.ATT_ROWS)
@pytest.mark.parametrize("v_kind", NC.ATT_V_KINDS)
@pytest.mark.parametrize("Tq,Tk", ATT_SHAPES)
def test_emulated_attention_meets_the_bound(Tq, Tk, v_kind, rows):
    worst, share = _att_ratio(NC.build_attention(1, 1, Tq, Tk, v_kind, seed=5, rows=rows))
    assert share == 0 and worst < 1, (Tq, Tk, v_kind, rows, worst)


@pytest.mark.parametrize("Tq,Tk", ATT_SHAPES)
def test_fp32_attention_meets_the_exact_forms_bound(Tq, Tk):
    """the bound the three-launch exact form is held to, on plain fp32 arithmetic — including rows whose far keys underflow"""
    for rows in NC.ATT_ROWS:
        for v_kind in NC.ATT_V_KINDS:
            for hd in NC.build_attention(1, 1, Tq, Tk, v_kind, seed=5, rows=rows)["heads"]:
                want, _, _ = R.ref_attention64(hd["q"], hd["k"], hd["v"], NC.ATT_SCALE)
                bound = R.attention_bound(hd["q"], hd["k"], hd["v"], NC.ATT_SCALE, exact=True)
                err = np.abs(R.fp32_attention(hd["q"], hd["k"], hd["v"], NC.ATT_SCALE).astype(np.float64) - want)
                assert (err <= bound).all(), (Tq, Tk, rows, v_kind, float((err / np.maximum(bound, 1e-300)).max()))


def test_emulated_attention_meets_the_bound_at_the_encoder_length():
    built = NC.build_attention(2, 2, 200, 1500, "one_signed", seed=6, q_gap=64, kv_gap=128)
    built["heads"] = built["heads"][1:3]  # two of the four (sequence, head) pairs: the emulation walks 47 blocks for each
    worst, share = _att_ratio(built)
    assert share == 0 and worst < 1, worst


def _worst_share(mutation, v_kinds):
    best = 0.0
    for Tq, Tk in ((129, 65), (127, 33), (129, 32)):
        for v_kind in v_kinds:
            for rows in NC.ATT_ROWS:
                _, share = _att_ratio(NC.build_attention(1, 1, Tq, Tk, v_kind, seed=5, rows=rows), **mutation)
                best = max(best, share)
    return best


@pytest.mark.parametrize("mutation", [dict(drop_qk="hh"), dict(drop_qk="hl"), dict(drop_qk="lh"), dict(drop_pv="hh"), dict(drop_pv="hl"), dict(drop_pv="lh"),
                                      dict(join_scale=1024.0), dict(v_perm=False)],
                         ids=["qk-no-hi.hi", "qk-no-hi.lo", "qk-no-lo.hi", "pv-no-hi.hi", "pv-no-hi.lo", "pv-no-lo.hi", "scale-1024", "v-permuted"])
def test_mutated_attention_misses_the_bound_on_half_the_elements(mutation):
    assert _worst_share(mutation, ("random", "one_signed", "ramp")) >= 0.5, mutation


def test_indicator_values_make_a_wrong_key_mapping_gross():
    """with v[j] = e_(j mod 64) or v[j] = j a wrong key-to-column mapping is an error of the size of the output, not of its rounding"""
    for v_kind in ("indicator", "ramp"):
        built = NC.build_attention(1, 1, 127, 33, v_kind, seed=5)
        hd = built["heads"][0]
        want, _, _ = R.ref_attention64(hd["q"], hd["k"], hd["v"], NC.ATT_SCALE)
        got = R.emu_attention(hd["q"], hd["k"], hd["v"], NC.ATT_SCALE, v_perm=False)
        assert np.abs(got - want).max() > 0.05 * np.abs(want).max()


# ---- the launcher's choice and the probe's argument checks: no device involved (device = -1) ----
def _plan(tk, **case):
    built = NC.build_gemm(seed=1, **case)
    return tk.gemm_probe(device=-1, **built["kw"])[1]


def test_launcher_choice_of_every_fast_case(tk):
    for name, case, expect in FAST_CASES:
        assert _plan(tk, fast=True, **case) == NC.code_of(expect), name


def test_launcher_choice_exact_kernels(tk):
    F32, TALL, BIG = tk.GEMM_F32, tk.GEMM_F32_TALL, tk.GEMM_F32_BIG
    code = tk.gemm_code
    assert _plan(tk, M=65, N=67, K=30) == code(F32, path=0)                       # K % 4 != 0
    assert _plan(tk, M=65, N=67, K=32) == code(F32, path=1)
    assert _plan(tk, M=65, N=67, K=32, lda=33) == code(F32, path=0)               # odd pitch
    assert _plan(tk, M=65, N=67, K=32, a_offset=1) == code(F32, path=0)           # misaligned base
    assert _plan(tk, M=65, N=67, K=32, b_offset=1) == code(F32, path=0)
    assert _plan(tk, M=65, N=68, K=32, b_kn=True) == code(F32, path=2)
    assert _plan(tk, M=65, N=67, K=32, b_kn=True) == code(F32, path=0)
    assert _plan(tk, M=65, N=67, K=32, b_f16=True) == code(F32, path=0)
    assert _plan(tk, M=257, N=97, K=36) == code(BIG, path=1)
    assert _plan(tk, M=255, N=97, K=36) == code(F32, path=1)                      # the threshold between the two tilings
    assert _plan(tk, M=256, N=96, K=36) == code(BIG, path=1)
    assert _plan(tk, M=256, N=95, K=36) == code(F32, path=1)
    assert _plan(tk, M=512, N=95, K=36) == code(TALL, path=1, nt=3)
    assert _plan(tk, M=511, N=95, K=36) == code(F32, path=1)
    assert _plan(tk, M=513, N=31, K=30) == code(TALL, path=0, nt=1)
    assert _plan(tk, M=513, N=33, K=144, b_kn=True) == code(F32, path=0)          # the tall kernel reads [N][K] only
    assert _plan(tk, M=513, N=64, K=144, batch=2) == code(F32, path=1)            # and has no batch
    # the fast path is taken by N and the batch layout, never by M; ineligible descriptors keep the exact chain
    for M in (1, 300, 600):
        assert _plan(tk, M=M, N=95, K=36, fast=True) == code(tk.GEMM_H3_TALL, path=1, nt=3)
        assert _plan(tk, M=M, N=96, K=36, fast=True) == code(tk.GEMM_H3_BIG, path=1)
    assert _plan(tk, M=65, N=68, K=32, b_kn=True, fast=True) == code(F32, path=2)
    assert _plan(tk, M=65, N=67, K=30, fast=True) == code(F32, path=0)
    assert _plan(tk, M=50, N=64, K=64, batch=6, inner=3, fast=True) == code(F32, path=1)


def test_probe_refuses_what_it_could_not_run_safely(tk):
    built = NC.build_gemm(M=33, N=35, K=36, bias=True, residual=True, seed=2)

    def rc(**change):
        kw = dict(built["kw"])
        kw.update(change)
        try:
            tk.gemm_probe(device=-1, **kw)
        except tk.TkError as e:
            return e.code
        return 0

    assert rc() == 0
    assert rc(a=built["kw"]["a"][:-1]) == 1001          # one float short of the last row of A
    assert rc(b=built["kw"]["b"][:-1]) == 1001
    assert rc(c=built["kw"]["c"][:33 * 35 - 1]) == 1001
    assert rc(residual=built["kw"]["residual"][:-1]) == 1001
    assert rc(bias=built["bias"][:-1]) == 1001
    assert rc(M=34) == 1001 and rc(K=37) == 1001 and rc(N=36) == 1001
    assert rc(lda=37) == 1001 and rc(ldb=37) == 1001 and rc(ldc=34) == 1001
    assert rc(M=0) == 1001 and rc(act=4) == 1001 and rc(batch=0) == 1001 and rc(batch=2, strides=(1, 0, 0, 0)) == 1001
    assert rc(batch=6, batch_inner=4) == 1001 and rc(a_offset=-1) == 1001 and rc(strides=(-4, 0, 0, 0), batch=2) == 1001
    # implicit im2col the launcher refuses: channels that are no multiple of 4, a misaligned input, f16 weights; and input arrays too small
    M, K = NC.conv_shape(**NC.CONV_TALL)
    conv = NC.build_gemm(M=M, N=48, K=K, conv=NC.CONV_TALL, seed=3)
    kw = conv["kw"]

    def rc_im(im_change=None, **change):
        k2 = dict(kw)
        k2.update(change)
        if im_change:
            k2["im"] = dict(kw["im"], **im_change)
        try:
            return 0 if tk.gemm_probe(device=-1, **k2)[1] >= 0 else -1
        except tk.TkError as e:
            return e.code

    assert rc_im() == 0
    assert rc_im(a_offset=1) == 1001
    # [K][N] weights: the implicit kernels read B as [N][K] only (N = 48, ldb = 48: every 16-byte condition holds, so nothing else refuses it)
    assert rc_im(b_kn=True, ldb=48, b=np.zeros(K * 48, np.float32)) == 1001
    assert rc_im(b_kn=True, ldb=48, b=np.zeros(K * 48, np.float32), fast=True) == 1001
    assert rc_im(dict(C=6), K=54) == 1001
    assert rc_im(dict(ldx=10)) == 1001
    assert rc_im(ldb=K + 1, b=np.zeros(48 * (K + 1), np.float32)) == 1001
    assert rc_im(a=kw["a"][:-5]) == 1001
    assert rc_im(dict(H=10)) == 1001                     # a taller image than the array holds
    assert rc_im(K=K + 4, b=np.zeros(48 * (K + 4), np.float32), ldb=K + 4) == 1001   # K is not whole taps
