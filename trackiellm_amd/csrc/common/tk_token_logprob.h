/*
 * tk_token_logprob.h — the log-probability of a sampled token and the most probable alternatives (host + device).
 *
 * What llama.cpp's server reports as `n_probs` and the hosted APIs as `logprobs` / `top_logprobs`, restated here once as lane / row functions in
 * plain C++ that k_token_logprobs (llm/tk_llm_kernels.hip) runs per thread and tk_token_logprob_row runs in a host loop.
 *
 * Distribution.  Softmax over the WHOLE vocabulary of the row's logits as the token pick sees them: after logit bias and repetition penalties
 * (stages 1 and 2 of the chain in include/tk/tk_mi355x_ext.h), BEFORE the grammar mask and without temperature, top-k, top-p or min-p — the
 * model's own distribution.  A token banned with a -inf bias has log-probability -inf; a token the grammar forbids keeps its model
 * log-probability and may appear among the alternatives.
 *
 * Order.  Tokens are ordered as the sampler orders them (common/tk_sample_device.h): descending tk_lp_key(logit) — the unsigned key whose order
 * is the float order with -0 below +0 —, ties to the lower id.  "First" below means first in that order.
 *
 * Arithmetic, every operation one correctly rounded fp32 operation, never contracted, the same on both sides:
 *   1. m = the logit of the first token: the maximum logit (+0 when the maximum is a zero of both signs).
 *   2. e_i = tk_expf(l_i - m).  A -inf logit gives exactly 0; the first token gives exp(0) = 1.
 *   3. S = the sum of the e_i in ONE fixed order that depends neither on the number of rows nor on the pass, the order k_pick_rows
 *      (nn/tk_nn_kernels.hip) uses for its log-probability:
 *        - each of TK_LOGPROB_LANES = 1024 lanes adds its terms i = t, t + 1024, ... ascending, starting from +0        (tk_lp_lane_sum);
 *        - inside each wave of 64 lanes a six-level xor butterfly, distances 32, 16, 8, 4, 2, 1: v_t <- v_t + v_(t ^ d)  (every lane of a wave
 *          ends with the same bits: fp32 addition commutes);
 *        - the sixteen wave sums joined in ascending wave order: S = ((w_0 + w_1) + w_2) + ... + w_15                    (tk_lp_join_waves).
 *      S >= 1 always, so tk_logf(S) >= 0 is finite.
 *   4. logprob_i = (l_i - m) - tk_logf(S): two subtractions                                                              (tk_lp_logprob).
 *
 * Alternatives.  The min(n_top, vocab) first tokens, in order, each with its log-probability.  Invariant (tests/test_token_logprob_cpu.py): the
 * list is the prefix of the candidate list sample_row builds for an unmasked row.  The order is total, so HOW the tokens are selected does not show:
 * the kernel finds the K-th largest key bit by bit over keys it holds in registers, the host loop below extracts by comparison, sample_row runs a
 * radix select — one exact decision.  The first entry
 * equals the greedy pick except on a row whose maximum is a zero of both signs: k_argmax compares floats (-0 == +0: the lower id wins), the key
 * order puts +0 above -0.
 *
 * Limits: n_top in [-1, TK_LOGPROB_MAX_TOP]; -1 = the row is off — its workgroup returns after reading its descriptor, nothing of the row is
 * read or written; 0 = the chosen id only.  Vocabularies up to 65536 tokens, the sampler's limit.  A row must hold a finite logit and neither a
 * NaN nor +inf (the probe checks; the model's rows do).
 */
#ifndef TK_TOKEN_LOGPROB_H
#define TK_TOKEN_LOGPROB_H

#include <stdint.h>

#include "tk_exact_math.h" /* TK_HD, tk_expf, tk_logf */

#define TK_LOGPROB_MAX_TOP 20
#define TK_LOGPROB_MAX_VOCAB 65536
#define TK_LOGPROB_LANES 1024 /* the workgroup of k_token_logprobs: sixteen waves of 64 */

/* one row's record: the layout of the public tk_mi355x_token_logprob_t.  n_top = the count actually filled; entries past it are not written */
struct TkTokenLogprob {
    float logprob;
    int32_t n_top;
    int32_t top_ids[TK_LOGPROB_MAX_TOP];
    float top_logprobs[TK_LOGPROB_MAX_TOP];
};

TK_HD float tk_lp_sub(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fsub_rn(a, b);
#else
    return a - b;
#endif
}
TK_HD float tk_lp_add(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(a, b);
#else
    return a + b;
#endif
}

/* the sampler's key (sample_key): unsigned order == float order, -0 < +0 */
TK_HD uint32_t tk_lp_key(float f) {
    const uint32_t u = tk_f32_bits(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
/* the logit of a key: exact, tk_lp_unkey(tk_lp_key(f)) has f's bits */
TK_HD float tk_lp_unkey(uint32_t k) { return tk_bits_f32((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
/* token (la, ia) stands before token (lb, ib) */
TK_HD bool tk_lp_before(float la, int32_t ia, float lb, int32_t ib) {
    const uint32_t ka = tk_lp_key(la), kb = tk_lp_key(lb);
    return ka > kb || (ka == kb && ia < ib);
}

/* step 2 */
TK_HD float tk_lp_term(float l, float m) { return tk_expf(tk_lp_sub(l, m)); }
/* step 3, lane t < TK_LOGPROB_LANES: its terms in ascending order from +0 (the kernel adds the same terms in the same order from its registers) */
TK_HD float tk_lp_lane_sum(const float* lg, int cols, float m, int t) {
    /* eight loads in flight at a time (k_argmax's form; an index past the row loads a clamped element that is skipped); the additions keep their order */
    constexpr int NU = 8;
    float s = 0.0f;
    for (int i0 = t; i0 < cols; i0 += TK_LOGPROB_LANES * NU) {
        float v[NU];
        for (int u = 0; u < NU; ++u) {
            const int i = i0 + TK_LOGPROB_LANES * u;
            v[u] = lg[i < cols ? i : cols - 1];
        }
        for (int u = 0; u < NU; ++u)
            if (i0 + TK_LOGPROB_LANES * u < cols) s = tk_lp_add(s, tk_lp_term(v[u], m));
    }
    return s;
}
/* step 3, the sixteen wave sums in ascending order */
TK_HD float tk_lp_join_waves(const float* w) {
    float S = w[0];
    for (int k = 1; k < TK_LOGPROB_LANES / 64; ++k) S = tk_lp_add(S, w[k]);
    return S;
}
/* step 4 */
TK_HD float tk_lp_logprob(float l, float m, float logS) { return tk_lp_sub(tk_lp_sub(l, m), logS); }

/* the limits of one row's request; the message names the first one broken */
static inline const char* tk_logprob_check(int32_t n_top, int64_t vocab) {
    if (n_top < -1 || n_top > TK_LOGPROB_MAX_TOP) return "n_top must be in [-1, 20]";
    if (n_top >= 0 && (vocab < 1 || vocab > TK_LOGPROB_MAX_VOCAB)) return "log-probabilities support vocabularies of at most 65536 tokens";
    return nullptr;
}
/* what a live row's logits must be before either side may run it (the probe's check) */
static inline const char* tk_logprob_check_row(const float* lg, int cols) {
    bool finite = false;
    for (int i = 0; i < cols; ++i) {
        const float v = lg[i];
        if (v != v) return "a NaN logit";
        if (v > 3.402823466e38f) return "a +inf logit";
        finite = finite || v >= -3.402823466e38f;
    }
    return finite ? nullptr : "no finite logit in the row";
}

/* one row on the host: the device kernel's lanes in a loop.  tok = the chosen id, in [0, cols); n_top in [-1, TK_LOGPROB_MAX_TOP] */
static inline void tk_token_logprob_row(const float* lg, int cols, int32_t tok, int32_t n_top, TkTokenLogprob* rec) {
    if (n_top < 0) return;
    int32_t first = 0;
    for (int32_t i = 1; i < cols; ++i)
        if (tk_lp_before(lg[i], i, lg[first], first)) first = i;
    const float m = lg[first];
    float v[TK_LOGPROB_LANES], nv[TK_LOGPROB_LANES], w[TK_LOGPROB_LANES / 64];
    for (int t = 0; t < TK_LOGPROB_LANES; ++t) v[t] = tk_lp_lane_sum(lg, cols, m, t);
    for (int d = 32; d >= 1; d >>= 1) {
        for (int t = 0; t < TK_LOGPROB_LANES; ++t) nv[t] = tk_lp_add(v[t], v[t ^ d]);
        for (int t = 0; t < TK_LOGPROB_LANES; ++t) v[t] = nv[t];
    }
    for (int k = 0; k < TK_LOGPROB_LANES / 64; ++k) w[k] = v[64 * k];
    const float logS = tk_logf(tk_lp_join_waves(w));
    rec->logprob = tk_lp_logprob(lg[tok], m, logS);
    const int32_t n = n_top < cols ? n_top : cols;
    rec->n_top = n;
    /* extraction: entry j is the first token that stands behind entry j - 1 */
    for (int32_t j = 0; j < n; ++j) {
        int32_t best = -1;
        for (int32_t i = 0; i < cols; ++i) {
            if (j > 0 && !tk_lp_before(lg[rec->top_ids[j - 1]], rec->top_ids[j - 1], lg[i], i)) continue;
            if (best < 0 || tk_lp_before(lg[i], i, lg[best], best)) best = i;
        }
        rec->top_ids[j] = best;
        rec->top_logprobs[j] = tk_lp_logprob(lg[best], m, logS);
    }
}

#endif
