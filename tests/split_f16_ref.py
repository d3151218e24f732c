"""References for the perception GEMM / attention launch tests (NumPy only, no GPU, no oracle).

Three things live here:
  1. float64 references: GEMM + epilogue (ref_gemm64) and softmax attention (ref_attention64);
  2. a NumPy EMULATION of the documented split-f16 scheme (csrc/nn/tk_nn_kernels.hip: k_gemm_h3_*, k_attention_h3) with switches that break
     it on purpose (drop one of the three products, a wrong 1/2048, a mis-permuted V staging);
  3. error BOUNDS derived from that scheme, below.  tests/test_split_f16_cpu.py shows on the CPU that the emulation meets every bound and
     that every mutation misses it; tests/test_nn_gemm_gpu.py holds the kernels to the same bounds.  No constant is fitted to a GPU result.

Notation: u = 2^-24 (fp32 unit roundoff, round to nearest), S = sum_k |a_k| |b_k| of the element, n16 = ceil(K / 16) MFMA steps.

The split.  hi = f16(x) has |x - hi| <= 2^-11 |x|; r = x - hi is exact in fp32 (it holds the <= 13 low bits of x) and so is 2048 r;
lo = f16(2048 r) has |lo / 2048 - r| <= 2^-11 |r| <= 2^-22 |x|.  So x = hi + lo / 2048 + dx with |dx| <= 2^-22 |x|.  Where 2048 r falls below
the f16 normal range (|x| < ~2^-13) lo is a subnormal with spacing 2^-24, and |dx| <= 2^-25 / 2048 = ETA = 2^-36 absolutely instead.

GEMM element, before the epilogue (gemm_acc_bound):
  truncation   a b - [ah bh + (ah bl + al bh) / 2048] = da b + a db + (al bl) / 2048^2 - (second order): each of the three <= 2^-22 |a||b|
               -> 3 2^-22 S, plus ETA sum_k (|a_k| + |b_k|) for subnormal low halves;
  hh chain     products of f16 values are exact in fp32; one MFMA adds 16 of them to the accumulator with one rounding of a partial sum
               that never exceeds S (1 + 2^-10): n16 u S;
  hx chain     two MFMAs per step on terms of size <= 2 S, then divided by 2048: 2 n16 (2 S) u / 2048 = n16 2^-9 u S  (<= 1 u S for K <= 8192);
  join         hh + hx / 2048: the division is exact, the sum one rounding: 1 u S;
  second order the (1 + 2^-10), (1 + 2^-11)^2 and (1 + u)^n - 1 factors dropped above: < 3 2^-22 2^-9 + ... < 1 u S.
  => |acc - sum_k a_k b_k| <= (3 2^-22 + (n16 + H3_C) u) S + ETA sum_k (|a_k| + |b_k|),  H3_C = 3  (hx, join, second order).
The exact kernels evaluate one fma chain per element: |acc - sum| <= K u S (chain_acc_bound), the usual running-error bound.

Epilogue (epilogue_bound), v = act(alpha acc + bias) + residual, each fp32 operation one rounding of its own result:
  alpha (skipped when 1): |alpha| E + u |alpha acc|;  bias: + u |v|;  activation: L E + A(v) with L = sup |act'| (SiLU 1.1, GELU 1.13,
  sigmoid 0.25) and A the evaluation error of the activation itself; residual: + u |result|.
  A(v), for both the exact-math sequences (exp <= 1 ulp, division <= 1 ulp) and the hardware forms of the fast kernels (v_exp_f32, v_rcp_f32:
  1 ulp = 2 u each, as documented):
    sigmoid = 1 / (1 + exp2(-v log2 e)):  the constant and the product each move the exponent by u |v| -> 2 |v| u relative; exp 2 u;
              1 + e: 1 u; reciprocal 2 u; so <= (2 |v| + 5) u sigmoid(v); (2 |v| + 8) u is used (three spare roundings for the exact form's
              negation / division sequence);
    SiLU    = v sigmoid(v): one more product: (2 |v| + 9) u |SiLU(v)|;
    GELU    = (v / 2) (1 + th), th = 1 - r, r = 2 / (exp(w) + 1), w = 2 inner, inner = 0.79788 (v + 0.044715 v^3): inner carries 5 roundings,
              the exponent 2 more (constant, product) -> exp(w) is off by (7 |w| + 2) u, e + 1: 1 u, reciprocal 2 u: r is off by
              (7 |w| + 5) u r, 1 - r and 1 + th one rounding each of values <= 2 (3 u with the first), the outer product 1 u:
              <= |v / 2| (r (7 |w| + 5) + 3) u + u |GELU(v)|.  (For v << 0 this is an ABSOLUTE error of some 1e-5: 1 + th cancels.)

Attention, one (sequence, head, query); s_j = scale q.k_j, P = softmax(s), out_d = sum_j P_j v_jd, Vbar_d = sum_j P_j |v_jd|,
nb = ceil(Tk / 32) blocks, Rg = max_j s_j - min_j s_j:
  scores       t = fl(scale q) (1 u), then a 64-long split contraction: E_j = gemm_acc_bound(n16 = 4) + u S_j with S_j = sum_d |t_d||k_jd|;
  weights      the kernel's weight of key j is exp(s^_j - m_b) prod_{b' > b} alpha_b'; a common factor cancels between numerator and
               denominator, so only RELATIVE errors of the weights count:  theta_j <= 1.01 E_j                 (score error, e^x - 1 <= 1.01 x)
                 + (3 |s_j - m_b| + 2) u <= (3 Rg + 2) u    (subtraction, rounded log2 e, product: 3 u of the exponent; v_exp_f32 2 u)
                 + (3 Rg + 2 nb) u                          (each rescale factor likewise; the maximum moves by Rg in all; alpha == 1 is exact)
               and |out^ - out| from the weights alone <= sum_j P_j theta_j |v_jd| + Vbar_d sum_j P_j theta_j;
  numerator    p and v split like GEMM operands: 3 2^-22 Vbar + ETA (sum_j |v_jd| + 1); two hh MFMAs and one rescale product per block:
               3 nb u Vbar; hx chain, join, the product with 1 / l, second order: 4 u Vbar;
  denominator  16 additions, one rescale product and one addition per block and lane half, all terms positive: (18 nb) u; the two halves
               1 u; v_rcp_f32 2 u: (18 nb + 3) u Vbar (as |out_d| <= Vbar_d).
The exact three-launch form (fp32 chains, two-pass softmax) has, by the same steps, theta_j <= 1.01 (64 + 1) u S_j + (Rg + 4) u, numerator
Tk u Vbar (one fma chain) and denominator (Tk + 3) u Vbar (any summation order of Tk positive terms, the division).
Underflow, both forms: a weight exp(s_j - m) near or below the fp32 normal range is lost or denormal — the exact path's tk_expf returns 0
below e^-87 (csrc/common/tk_exact_math.h), the hardware exp2 below 2^-126 — an ABSOLUTE error <= e^-87 of a weight, against a denominator >= 1:
e^-87 (sum_j |v_jd| + Tk Vbar_d) — the only error where Vbar_d is 0 or tiny.
"""
import numpy as np

U = 2.0 ** -24
ETA = 2.0 ** -36
H3_SCALE = 2048.0
H3_C = 3
ACT_LIP = {0: 1.0, 1: 1.1, 2: 1.13, 3: 0.25}
L2E = np.float32(1.4426950408889634)


def f32(x):
    return np.asarray(x, dtype=np.float32)


def f16r(x):
    """x rounded to f16 and widened again (float32 in, float32 out)"""
    return f32(x).astype(np.float16).astype(np.float32)


def split(x, scale=H3_SCALE):
    x = f32(x)
    hi = f16r(x)
    lo = f16r((x - hi) * np.float32(scale))
    return hi, lo


# ---------------------------------------------------------------- operands
def random_operands(rng, shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def one_signed_operands(rng, shape, scale=1.0):
    """positive f16 values times (1 + 2^-13): hi is the f16 value and every low half is +2^-13 of it, so every product has cross terms of ONE
    sign — a dropped cross product or a wrong 1 / 2048 is then an error of 2^-13 S on every element instead of a random walk"""
    h = np.abs(rng.standard_normal(shape) * scale).astype(np.float16).astype(np.float32) + np.float32(2.0 ** -6)
    h = f16r(h)
    return (h * np.float32(1.0 + 2.0 ** -13)).astype(np.float32)


# ---------------------------------------------------------------- float64 references
def act64(v, act):
    v = np.asarray(v, np.float64)
    if act == 1:
        return v / (1.0 + np.exp(-v))
    if act == 2:
        return 0.5 * v * (1.0 + np.tanh(0.797884560802865356 * (v + 0.044715 * v ** 3)))
    if act == 3:
        return 1.0 / (1.0 + np.exp(-v))
    return v


def ref_gemm64(A, Bnk, bias=None, residual=None, act=0, alpha=1.0):
    """float64: (pre-epilogue sums, S = sum |a||b|, T = sum (|a| + |b|), result); A [M][K], Bnk [N][K]"""
    A64, B64 = np.asarray(A, np.float64), np.asarray(Bnk, np.float64)
    acc = A64 @ B64.T
    S = np.abs(A64) @ np.abs(B64).T
    T = np.abs(A64).sum(1)[:, None] + np.abs(B64).sum(1)[None, :]
    v = acc * np.float64(np.float32(alpha))
    if bias is not None:
        v = v + np.asarray(bias, np.float64)[None, :]
    v = act64(v, act)
    if residual is not None:
        v = v + np.asarray(residual, np.float64)
    return acc, S, T, v


def ref_attention64(q, k, v, scale):
    """q [Tq][64], k / v [Tk][64] of one head -> (out [Tq][64], P [Tq][Tk], s [Tq][Tk]) in float64"""
    s = (np.asarray(q, np.float64) * np.float64(np.float32(scale))) @ np.asarray(k, np.float64).T
    e = np.exp(s - s.max(1, keepdims=True))
    P = e / e.sum(1, keepdims=True)
    return P @ np.asarray(v, np.float64), P, s


# ---------------------------------------------------------------- bounds
def gemm_acc_bound(S, T, K):
    n16 = -(-K // 16)
    assert K <= 8192
    return (3 * 2.0 ** -22 + (n16 + H3_C) * U) * S + ETA * T


def chain_acc_bound(S, K):
    return K * U * S


def act_eval_bound(v, act):
    v = np.asarray(v, np.float64)
    if act == 0:
        return np.zeros_like(v)
    if act == 3:
        return (2 * np.abs(v) + 8) * U * act64(v, 3)
    if act == 1:
        return (2 * np.abs(v) + 9) * U * np.abs(act64(v, 1))
    w = 2 * 0.797884560802865356 * (v + 0.044715 * v ** 3)
    r = 2.0 / (np.exp(np.minimum(w, 700.0)) + 1.0)
    return np.abs(0.5 * v) * (r * (7 * np.abs(w) + 5) + 3) * U + U * np.abs(act64(v, 2))


def epilogue_bound(acc, E, bias=None, residual=None, act=0, alpha=1.0):
    """bound of |kernel - float64| after the epilogue, given the float64 pre-epilogue sums `acc` and their bound E"""
    al = np.float64(np.float32(alpha))
    v = acc * al
    if np.float32(alpha) != np.float32(1.0):
        E = abs(al) * E + U * np.abs(v)
    if bias is not None:
        v = v + np.asarray(bias, np.float64)[None, :]
    E = E + U * np.abs(v)  # the kernels add the bias, +0 when there is none
    if act != 0:
        # the activation is evaluated at a point within E of v: its own evaluation error there, bounded at the worse end of that interval
        E = ACT_LIP[act] * E + np.maximum(act_eval_bound(v - E, act), act_eval_bound(v + E, act))
        v = act64(v, act)
    if residual is not None:
        v = v + np.asarray(residual, np.float64)
        E = E + U * np.abs(v)
    return E * (1 + 2.0 ** -10)  # the bound's own terms were evaluated at the float64 values, not at the kernel's


def attention_bound(q, k, v, scale, exact=False):
    """bound [Tq][64] of |kernel - float64| for one head (fused split-f16 kernel, or the exact three-launch form)"""
    out, P, s = ref_attention64(q, k, v, scale)
    Tk = k.shape[0]
    nb = -(-Tk // 32)
    t = np.abs(np.asarray(q, np.float64) * np.float64(np.float32(scale)))
    k64, v64 = np.abs(np.asarray(k, np.float64)), np.abs(np.asarray(v, np.float64))
    Sj = t @ k64.T
    Rg = (s.max(1) - s.min(1))[:, None]
    if exact:
        theta = 1.01 * (64 + 1) * U * Sj + (Rg + 4) * U
        num, den = Tk * U, (Tk + 3) * U
        eta = 0.0
    else:
        Ej = gemm_acc_bound(Sj, t.sum(1)[:, None] + k64.sum(1)[None, :], 64) + U * Sj
        theta = 1.01 * Ej + (6 * Rg + 2 * nb + 4) * U
        num, den = 3 * 2.0 ** -22 + (3 * nb + 4) * U, (18 * nb + 3) * U
        eta = ETA * (v64.sum(0)[None, :] + 1.0)
    Vbar = P @ v64
    PT = P * theta
    under = np.exp(-87.0) * (v64.sum(0)[None, :] + Tk * Vbar)
    return (PT @ v64 + Vbar * PT.sum(1, keepdims=True) + Vbar * (num + den) + eta + under) * (1 + 2.0 ** -10)


# ---------------------------------------------------------------- emulation of the scheme
def _mfma(acc, a, b):
    """one v_mfma_f32_32x32x16_f16 step as the scheme documents it: 16 exact products and the accumulator, one fp32 rounding;
    a [M][16], b [N][16] f16 values held in float32"""
    return (acc.astype(np.float64) + a.astype(np.float64) @ b.astype(np.float64).T).astype(np.float32)


def emu_contract(A, B, drop=None, join_scale=H3_SCALE):
    """sum_k A[m][k] B[n][k] by the split scheme: hi.hi into one fp32 accumulator, hi.lo and lo.hi into a second, joined once.
    drop in (None, 'hh', 'hl', 'lh') leaves one of the three products out; join_scale != 2048 is the wrong-scale mutation"""
    A, B = f32(A), f32(B)
    M, K = A.shape
    Kp = -(-K // 32) * 32
    Ap, Bp = np.zeros((M, Kp), np.float32), np.zeros((B.shape[0], Kp), np.float32)
    Ap[:, :K], Bp[:, :K] = A, B
    ah, al = split(Ap)
    bh, bl = split(Bp)
    hh = np.zeros((M, B.shape[0]), np.float32)
    hx = np.zeros_like(hh)
    for ks in range(0, Kp, 16):
        sl = slice(ks, ks + 16)
        if drop != "hh":
            hh = _mfma(hh, ah[:, sl], bh[:, sl])
        if drop != "hl":
            hx = _mfma(hx, ah[:, sl], bl[:, sl])
        if drop != "lh":
            hx = _mfma(hx, al[:, sl], bh[:, sl])
    return hh + hx * np.float32(1.0 / join_scale)


def emu_gemm(A, Bnk, bias=None, residual=None, act=0, alpha=1.0, drop=None, join_scale=H3_SCALE):
    """the fast GEMM: emu_contract, then the epilogue in fp32 steps (activations through float64, rounded once: the hardware's are ~1 ulp)"""
    v = emu_contract(A, Bnk, drop, join_scale)
    if np.float32(alpha) != np.float32(1.0):
        v = v * np.float32(alpha)
    v = v + (f32(bias)[None, :] if bias is not None else np.float32(0))
    if act != 0:
        v = act64(v, act).astype(np.float32)
    if residual is not None:
        v = v + f32(residual)
    return v


def _exp2(x):
    return np.exp2(x.astype(np.float64)).astype(np.float32)


# V^T staging of k_attention_h3: LDS column c = 16 s + 8 g + j of a 32-key block holds key 16 s + 4 g + (j % 4) + 8 (j / 4), the order in which
# the S^T accumulator hands the lane its 16 probabilities
_C = np.arange(32)
V_KEY_OF_COLUMN = 16 * (_C // 16) + 4 * ((_C % 16) // 8) + (_C % 4) + 8 * ((_C % 8) // 4)


def emu_attention(q, k, v, scale, drop_qk=None, drop_pv=None, join_scale=H3_SCALE, v_perm=True):
    """k_attention_h3 for one head: 32-key blocks, online maximum / sum / rescale, split operands on both contractions.
    v_perm False stages V with column c <- key c (the mis-permutation: probabilities then meet the wrong keys' values)"""
    q, k, v = f32(q), f32(k), f32(v)
    Tq, Tk = q.shape[0], k.shape[0]
    t = q * np.float32(scale)
    o_hh = np.zeros((Tq, 64), np.float32)
    o_hx = np.zeros_like(o_hh)
    m_run = np.full(Tq, -np.inf, np.float32)
    l_run = np.zeros((Tq, 2), np.float32)  # one partial sum per lane half g
    inv_s = np.float32(1.0 / join_scale)
    half = ((np.arange(32) % 8) // 4)  # g of key offset c: keys 4 g + (r % 4) + 8 (r / 4)
    for k0 in range(0, Tk, 32):
        nk = min(32, Tk - k0)
        kb, vb = np.zeros((32, 64), np.float32), np.zeros((32, 64), np.float32)
        kb[:nk], vb[:nk] = k[k0:k0 + nk], v[k0:k0 + nk]
        st = emu_contract(t, kb, drop_qk, join_scale)  # [Tq][32]; K = 64: 4 steps, as the kernel's
        st[:, nk:] = -np.inf
        m_new = np.maximum(m_run, st.max(1))
        alpha = _exp2((m_run - m_new) * L2E)
        m_run = m_new
        pr = _exp2((st - m_new[:, None]) * L2E)
        for g in range(2):
            psum = np.zeros(Tq, np.float32)
            for c in np.nonzero(half == g)[0]:
                psum = psum + pr[:, c]
            l_run[:, g] = l_run[:, g] * alpha + psum
        o_hh = o_hh * alpha[:, None]
        o_hx = o_hx * alpha[:, None]
        ph, pl = split(pr)
        vstaged = vb if v_perm else vb[V_KEY_OF_COLUMN]
        vh, vl = split(vstaged)
        for sp in range(2):
            sl = slice(16 * sp, 16 * sp + 16)
            if drop_pv != "hh":
                o_hh = _mfma(o_hh, ph[:, sl], vh[sl].T)
            if drop_pv != "hl":
                o_hx = _mfma(o_hx, pl[:, sl], vh[sl].T)
            if drop_pv != "lh":
                o_hx = _mfma(o_hx, ph[:, sl], vl[sl].T)
    l = l_run[:, 0] + l_run[:, 1]
    inv = (1.0 / l.astype(np.float64)).astype(np.float32)
    return (o_hh + o_hx * inv_s) * inv[:, None]


def fp32_attention(q, k, v, scale):
    """the three-launch form in plain fp32 steps (NumPy's summation order, not the kernels' chains: any order is inside the exact form's bound)"""
    q, k, v = f32(q), f32(k), f32(v)
    s = (q @ k.T) * np.float32(scale)
    e = np.exp(s - s.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True, dtype=np.float32)
    return p @ v
