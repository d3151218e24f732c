"""Operands and shapes of the perception launch tests, shared by tests/test_split_f16_cpu.py (the emulation against the bounds) and
tests/test_nn_gemm_gpu.py (the kernels against the same bounds): NumPy only, no device (the package is imported for its kernel codes).

build_gemm() lays one launch out in memory exactly as the descriptor addresses it — pitches, base offsets, [K][N] weights, f16 weights, the
two-level batch, a convolution input for implicit im2col — and hands back, per batch member, the LOGICAL operands (A [M][K], B [N][K],
residual [M][N]) and the flat indices of that member's C cells, so a reference never has to know the layout."""
import numpy as np

import split_f16_ref as R
from trackiellm_amd import GEMM_H3_BIG as H3_BIG, GEMM_H3_TALL as H3_TALL, gemm_code

SENTINEL = np.float32(-7777.25)
KINDS = ("random", "one_signed")


def _values(rng, kind, n, scale=1.0):
    return (R.one_signed_operands if kind == "one_signed" else R.random_operands)(rng, n, scale)


def im2col(x, kw, stride, pad):
    """x [B][H][W][C] -> (col [B Ho Wo][kw kw C] with k = (ky kw + kx) C + c, Ho, Wo)"""
    B, H, W, C = x.shape
    Ho, Wo = (H + 2 * pad - kw) // stride + 1, (W + 2 * pad - kw) // stride + 1
    xp = np.zeros((B, H + 2 * pad, W + 2 * pad, C), x.dtype)
    xp[:, pad:pad + H, pad:pad + W] = x
    col = np.empty((B, Ho, Wo, kw, kw, C), x.dtype)
    for ky in range(kw):
        for kx in range(kw):
            col[:, :, :, ky, kx] = xp[:, ky:ky + stride * Ho:stride, kx:kx + stride * Wo:stride]
    return col.reshape(B * Ho * Wo, kw * kw * C), Ho, Wo


def conv_shape(B, H, W, C, stride, ldx=None, kw=3, pad=1):
    Ho, Wo = (H + 2 * pad - kw) // stride + 1, (W + 2 * pad - kw) // stride + 1
    return B * Ho * Wo, kw * kw * C


def build_gemm(M, N, K, kind="random", seed=0, lda=None, ldb=None, ldc=None, ldr=None, b_kn=False, act=0, bias=False, residual=False, alpha=1.0,
               batch=1, inner=0, b_f16=False, conv=None, a_offset=0, b_offset=0, fast=False):
    """conv = dict(B, H, W, C, ldx, stride) (3 x 3, pad 1) replaces A by a convolution input; M and K must be conv_shape()'s.
    Returns dict(kw = gemm_probe keyword arguments incl. a, b, c; members = [dict(A, B, R, cidx)]; bias; untouched = flat indices of C that no
    member owns)."""
    rng = np.random.default_rng(seed)
    ldb = (N if b_kn else K) if ldb is None else ldb
    ldc = N if ldc is None else ldc
    ldr = N if ldr is None else ldr
    nzo, nzi = (batch // inner, inner) if inner else (1, batch)
    bshape = (K, ldb) if b_kn else (N, ldb)
    # member strides: the inner level packs members back to back, the outer level leaves a gap (a multiple of 4: the aligned paths stay eligible)
    if conv:
        assert batch == 1
        x = _values(rng, kind, (conv["B"], conv["H"], conv["W"], conv["ldx"]))
        colm, Ho, Wo = im2col(x[..., :conv["C"]], 3, conv["stride"], 1)
        assert colm.shape == (M, K)
        a_store = x.reshape(-1)
        sA = sA2 = 0
        im = dict(C=conv["C"], H=conv["H"], W=conv["W"], ldx=conv["ldx"], kw=3, stride=conv["stride"], pad=1, Ho=Ho, Wo=Wo)
        lda = 0
    else:
        lda = K if lda is None else lda
        sA, im = M * lda, None
        sA2 = nzi * sA + 8
        a_store = _values(rng, kind, (nzo - 1) * sA2 + (nzi - 1) * sA + (M - 1) * lda + K)
    sB = bshape[0] * ldb
    sB2 = nzi * sB + 4
    nb = (nzo - 1) * sB2 + (nzi - 1) * sB + (bshape[0] - 1) * ldb + (N if b_kn else K)
    b_vals = _values(rng, kind, nb, 1.0 / np.sqrt(K))
    if b_f16:
        b_store = b_vals.astype(np.float16).view(np.uint16)
        b_vals = b_store.view(np.float16).astype(np.float32)
    else:
        b_store = b_vals
    sC, sR = (M + 1) * ldc, M * ldr
    sC2, sR2 = nzi * sC + 5, nzi * sR + 3
    n_c = (nzo - 1) * sC2 + (nzi - 1) * sC + (M + 2) * ldc
    c0 = np.full(n_c, SENTINEL, np.float32)
    r_store = rng.standard_normal((nzo - 1) * sR2 + (nzi - 1) * sR + (M - 1) * ldr + N).astype(np.float32) if residual else None
    bias_v = rng.standard_normal(N).astype(np.float32) if bias else None
    rows, cols, ks = np.arange(M)[:, None], np.arange(N)[None, :], np.arange(K)[None, :]
    members = []
    owned = np.zeros(n_c, bool)
    for zo in range(nzo):
        for zi in range(nzi):
            A = colm if conv else a_store[zo * sA2 + zi * sA + rows * lda + ks]
            ob = zo * sB2 + zi * sB
            Bm = b_vals[ob + ks.T * ldb + cols].T if b_kn else b_vals[ob + np.arange(N)[:, None] * ldb + ks]
            Rm = r_store[zo * sR2 + zi * sR + rows * ldr + cols] if residual else None
            cidx = zo * sC2 + zi * sC + rows * ldc + cols
            owned[cidx] = True
            members.append(dict(A=np.ascontiguousarray(A), B=np.ascontiguousarray(Bm), R=Rm, cidx=cidx))
    one = batch == 1
    kw = dict(a=a_store, b=b_store, c=c0, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, bias=bias_v, residual=r_store, ldr=ldr if residual else 0, b_kn=b_kn,
              act=act, alpha=alpha, batch=batch, strides=(0, 0, 0, 0) if one else (sA, sB, sC, sR if residual else 0), batch_inner=inner,
              strides2=(sA2, sB2, sC2, sR2 if residual else 0) if inner else (0, 0, 0, 0), b_f16=b_f16, im=im, fast=fast, a_offset=a_offset, b_offset=b_offset)
    return dict(kw=kw, members=members, bias=bias_v, untouched=np.nonzero(~owned)[0], act=act, alpha=alpha, K=K)


# ---- the fast (split-f16) GEMM cases: (id, build_gemm keyword arguments, expected kernel as (family, im, path, nt)) ----
CONV_TALL = dict(B=2, H=9, W=7, C=8, ldx=12, stride=1)    # M = 126, K = 72
CONV_BIG = dict(B=2, H=16, W=9, C=4, ldx=4, stride=2)     # M = 80, K = 36


def fast_gemm_cases():
    cases = []
    for M in (1, 127, 129):
        for N in (31, 33, 95):
            for K in (36, 240):
                cases.append((f"tall-{M}x{N}x{K}", dict(M=M, N=N, K=K, ldc=N + 3, bias=True), (H3_TALL, False, 1, (N + 31) // 32)))
    M, K = conv_shape(**CONV_TALL)
    cases.append(("tall-im2col", dict(M=M, N=48, K=K, conv=CONV_TALL, bias=True, act=1), (H3_TALL, True, 1, 2)))
    for N in (96, 97, 129):
        for M in (1, 129):
            cases.append((f"big-{M}x{N}x240", dict(M=M, N=N, K=240, ldc=N + 3), (H3_BIG, False, 1, 0)))
    cases.append(("big-batch2", dict(M=50, N=100, K=64, batch=6, inner=3, alpha=0.125), (H3_BIG, False, 1, 0)))
    M, K = conv_shape(**CONV_BIG)
    cases.append(("big-im2col", dict(M=M, N=128, K=K, conv=CONV_BIG, bias=True), (H3_BIG, True, 1, 0)))
    for act in (1, 2, 3):
        cases.append((f"big-act{act}", dict(M=129, N=97, K=240, act=act, bias=True), (H3_BIG, False, 1, 0)))
    cases.append(("big-residual", dict(M=129, N=97, K=240, bias=True, residual=True, ldr=101), (H3_BIG, False, 1, 0)))
    return cases


def code_of(expect):
    return gemm_code(*expect)


# ---- attention ----
ATT_TQ, ATT_TK = (2, 127, 129), (1, 31, 32, 33, 65)
ATT_V_KINDS = ("random", "one_signed", "indicator", "ramp")
ATT_SCALE = 0.125
ATT_ROWS = ("designed", "random")


def build_attention(B, nh, Tq, Tk, v_kind="random", seed=0, q_gap=0, kv_gap=0, rows="designed"):
    """q / k / v / out storage for one launch plus per (sequence, head) logical views.  Query rows cycle through six designs by row index:
    0 flat (q = 0); 1 the maximum in the first key; 2 scores rising with the key index, so the running maximum moves in EVERY block and last
    in the final, partial one; 3 one key ahead of all others by more than 80; 4 scores in the hundreds; 5 random.  Designs 1 - 4 read one
    coordinate of the keys each (q = g e_a + 0.05 noise), and the keys' coordinates 0 - 3 are written to produce them.
    rows = "random" leaves every query and key random: the rows on which a rounding-sized defect of the score contraction shows best
    (a flat or a one-hot row hides it)."""
    rng = np.random.default_rng(seed)
    d = nh * 64
    qb, kb = Tq * d + q_gap, Tk * d + kv_gap
    q = rng.standard_normal(B * qb).astype(np.float32)  # the gap follows the last sequence too
    k = rng.standard_normal(B * kb).astype(np.float32)
    nv = k.size
    if v_kind == "one_signed":
        v = R.one_signed_operands(rng, nv)
    else:
        v = rng.standard_normal(nv).astype(np.float32)
    out0 = np.full(q.size + 0, SENTINEL, np.float32)
    g = np.float32(1.0 / ATT_SCALE)
    heads = []
    j = np.arange(Tk)
    for b in range(B):
        for h in range(nh):
            qi = b * qb + np.arange(Tq)[:, None] * d + h * 64 + np.arange(64)[None, :]
            ki = b * kb + j[:, None] * d + h * 64 + np.arange(64)[None, :]
            kk = k[ki]
            kk[:, 0] = rng.standard_normal(Tk) * 0.5; kk[0, 0] = 6.0                 # design 1: key 0 leads by ~6
            kk[:, 1] = 8.0 * (j + 1) / Tk + rng.standard_normal(Tk) * 0.01          # design 2: rising
            kk[:, 2] = rng.standard_normal(Tk); kk[Tk // 2, 2] = 95.0                # design 3: one key > 80 ahead
            kk[:, 3] = rng.uniform(-300, 300, Tk)                                    # design 4: hundreds
            if rows == "designed":
                k[ki] = kk.astype(np.float32)
            qq = q[qi]
            for i in range(Tq if rows == "designed" else 0):
                des = i % 6
                if des == 0:
                    qq[i] = 0
                elif des <= 4:
                    qq[i] = rng.standard_normal(64) * 0.05
                    qq[i, :4] = 0
                    qq[i, des - 1] = g
            q[qi] = qq
            if v_kind == "indicator":
                vv = np.zeros((Tk, 64), np.float32)
                vv[j, j % 64] = 1
                v[ki] = vv
            elif v_kind == "ramp":
                v[ki] = np.repeat(j.astype(np.float32)[:, None], 64, 1)
            heads.append(dict(q=q[qi], k=k[ki], v=v[ki], oidx=qi))
    owned = np.zeros(q.size, bool)
    for hd in heads:
        owned[hd["oidx"]] = True
    return dict(q=q, k=k, v=v, out0=out0, heads=heads, untouched=np.nonzero(~owned)[0], B=B, nh=nh, Tq=Tq, Tk=Tk, d=d, q_bstride=qb, kv_bstride=kb)
