/*
 * tk_logit_adjust.h — the two sampler stages that run in front of the token pick: logit bias and the repetition penalties (host + device).
 *
 * llama.cpp's llama_sampling_prepare, in every generation the reference's calls fit (src/ai_models/tk_runner_lifecycle.c:76-77 installs
 * llama_sampling_default_params(), tk_runner_streaming.c:60-61 samples with it), changes the logits before grammar and the chain see them:
 *   1. logit_bias:  logits[id] += bias                              for every (id, bias) entry
 *   2. llama_sample_repetition_penalties over the last penalty_last_n accepted tokens: for every DISTINCT token t among them, c = how often
 *      it occurs there,  l = logits[t];  l = l <= 0 ? l * repeat : l / repeat;  l = l - (float(c) * freq + present)
 * restated here once, as lane functions in plain C++ that k_logit_adjust (llm/tk_llm_kernels.hip) runs one per thread and
 * tk_logit_adjust_row runs in a host loop.  Every operation is one correctly rounded fp32 operation, never contracted, in this order on both
 * sides, so host and device rows agree bit for bit.  -inf and signed zeros follow from the formulas (-0.0 <= 0: it is multiplied).
 *
 * A token's logit is written by exactly one lane: the bias lane of its (unique) entry, then — after a barrier — the lane that holds its FIRST
 * occurrence in the window.  The result therefore depends neither on lane order nor on duplicates.
 *
 * Two llama.cpp behaviours are NOT restated:
 *   - its `prev` ring starts as penalty_last_n zeros, so token 0 is penalised until that many tokens have been accepted.  Here the window
 *     holds accepted tokens only.
 *   - penalty_last_n = -1 ("the context size") is refused: a window holds at most TK_ADJUST_MAX_RECENT ids.
 * The newline token is penalised like any other (penalize_nl = true, that generation's default).
 */
#ifndef TK_LOGIT_ADJUST_H
#define TK_LOGIT_ADJUST_H

#include <stdint.h>

#include "tk_exact_math.h" /* TK_HD */

#define TK_ADJUST_MAX_RECENT 256 /* ids of one row's window */
#define TK_ADJUST_MAX_BIAS 256   /* bias entries of one row */
#define TK_ADJUST_LANES 256      /* one lane per window id / bias entry: the workgroup of k_logit_adjust */

/* one row's adjustment; its window ids, bias ids and bias values sit in row-major tables of TK_ADJUST_MAX_RECENT / TK_ADJUST_MAX_BIAS entries per row */
struct TkAdjustRow {
    float repeat, freq, present; /* 1, 0, 0 = no penalty */
    int32_t n_recent, n_bias;
};

TK_HD float tk_adj_mul(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, b);
#else
    return a * b;
#endif
}
TK_HD float tk_adj_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}
TK_HD float tk_adj_add(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(a, b);
#else
    return a + b;
#endif
}
TK_HD float tk_adj_sub(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fsub_rn(a, b);
#else
    return a - b;
#endif
}

/* a neutral row is not adjusted at all: nothing reads or writes its logits */
TK_HD bool tk_adjust_neutral(const TkAdjustRow& d) {
    return d.n_bias == 0 && (d.n_recent == 0 || (d.repeat == 1.0f && d.freq == 0.0f && d.present == 0.0f));
}

/* step 1, lane j < n_bias */
TK_HD void tk_adjust_bias_lane(float* logits, const int32_t* bias_ids, const float* bias, int j) {
    const int32_t t = bias_ids[j];
    logits[t] = tk_adj_add(logits[t], bias[j]);
}

/* step 3, lane j < n_recent, after every bias lane is done.  `recent` is the row's window (LDS on the device) */
TK_HD void tk_adjust_penalty_lane(float* logits, const TkAdjustRow& d, const int32_t* recent, int j) {
    const int32_t t = recent[j];
    int c = 0;
    bool first = true;
    for (int k = 0; k < d.n_recent; ++k) {
        const bool same = recent[k] == t;
        c += same ? 1 : 0;
        first = first && !(same && k < j);
    }
    if (!first) return; /* an earlier lane holds this token */
    float l = logits[t];
    l = l <= 0.0f ? tk_adj_mul(l, d.repeat) : tk_adj_div(l, d.repeat);
    l = tk_adj_sub(l, tk_adj_add(tk_adj_mul((float)c, d.freq), d.present));
    logits[t] = l;
}

/* the limits a row must keep before either side may run it; the message names the first one broken */
static inline const char* tk_adjust_check(const TkAdjustRow& d, const int32_t* recent, const int32_t* bias_ids, const float* bias, int64_t vocab) {
    if (d.n_recent < 0 || d.n_recent > TK_ADJUST_MAX_RECENT) return "n_recent must be in [0, 256]";
    if (d.n_bias < 0 || d.n_bias > TK_ADJUST_MAX_BIAS) return "n_bias must be in [0, 256]";
    if (!(d.repeat > 0.0f) || d.repeat - d.repeat != 0.0f) return "repeat must be finite and > 0";
    if (d.freq - d.freq != 0.0f || d.present - d.present != 0.0f) return "freq and present must be finite";
    if ((d.n_recent > 0 && !recent) || (d.n_bias > 0 && (!bias_ids || !bias))) return "a null array with a non-zero count";
    for (int j = 0; j < d.n_recent; ++j)
        if (recent[j] < 0 || recent[j] >= vocab) return "a window id is outside the vocabulary";
    for (int j = 0; j < d.n_bias; ++j) {
        if (bias_ids[j] < 0 || bias_ids[j] >= vocab) return "a bias id is outside the vocabulary";
        if (bias[j] != bias[j] || bias[j] > 3.402823466e38f) return "a bias must be finite or -inf";
        for (int k = 0; k < j; ++k)
            if (bias_ids[k] == bias_ids[j]) return "bias ids must be unique within a row";
    }
    return nullptr;
}

/* what a caller hands over for one row: the descriptor's values and the caller's arrays (read before the call returns).  The layout of the public
 * tk_mi355x_logit_adjust_t */
struct TkLogitAdjust {
    float repeat = 1.0f, freq = 0.0f, present = 0.0f;
    int32_t n_recent = 0;
    const int32_t* recent = nullptr;
    int32_t n_bias = 0;
    const int32_t* bias_ids = nullptr;
    const float* bias = nullptr;
    TkAdjustRow row() const { return TkAdjustRow{repeat, freq, present, n_recent, n_bias}; }
    const char* check(int64_t vocab) const { return tk_adjust_check(row(), recent, bias_ids, bias, vocab); }
    /* call after check(): the counts are in range */
    bool neutral() const { return tk_adjust_neutral(row()); }
};

/* one row on the host: the device kernel's lanes in a loop (the barrier is the end of the first loop) */
static inline void tk_logit_adjust_row(float* logits, const TkAdjustRow& d, const int32_t* recent, const int32_t* bias_ids, const float* bias) {
    if (tk_adjust_neutral(d)) return;
    for (int j = 0; j < d.n_bias; ++j) tk_adjust_bias_lane(logits, bias_ids, bias, j);
    for (int j = 0; j < d.n_recent; ++j) tk_adjust_penalty_lane(logits, d, recent, j);
}

#endif
