/*
 * tk_lang_pick.h — Whisper's language detection over one row of decoder logits (host + device).
 *
 * whisper.cpp's whisper_lang_auto_detect, which the reference reaches through `language = "auto"` (src/audio/tk_asr_whisper.c:252,386): encode, decode
 * <|startoftranscript|> once, soft-max the logits of the language tokens, take the most probable one.  Restated here once, as a per-row function
 * over the n_lang consecutive logits l[0 .. n_lang) that start at token tok0 = sot + 1:
 *   1. decision       id = first index of the maximum under `>` (a NaN is never greater); no logit above -inf: id = 0.  m = l[id]
 *   2. probabilities  d_i = (l_i == m) ? 0 : l_i - m;  p_i = 0 where l_i is a NaN or -inf (tk_expf is not called), else tk_expf(d_i);
 *                     no logit above -inf: every p_i = 0 and every prob_i = 0
 *   3. sum            S = p_0 + p_1 + ... in fp32, i ascending, starting from +0
 *   4. result         prob_i = tk_divf(p_i, S)
 * Every step is one correctly rounded fp32 operation or one call of tk_exact_math.h after the other, never contracted, so tk_lang_pick_row (a host
 * loop) and k_lang_pick (nn/tk_nn_kernels.hip: one 64-lane wave per row, lanes take i = lane and lane + 64) agree bit for bit.
 *
 * whisper.cpp itself is absent: its own arithmetic (it sorts the candidates, and its accumulator type and tie order follow from that) is not
 * pinned.  The decision agrees with any soft-max arg max wherever the maximum is unique.
 */
#ifndef TK_LANG_PICK_H
#define TK_LANG_PICK_H

#include <stdint.h>

#include "tk_exact_math.h" /* TK_HD */

#define TK_LANG_MAX 128 /* language tokens of one row: two per lane of a wave */

#define TK_WH_SOT_MULTILINGUAL 50258 /* <|startoftranscript|> of a multilingual vocabulary (whisper.cpp's whisper_vocab); <|en|> follows it */

/* language tokens of a Whisper vocabulary: 99 at 51865 tokens, 100 (+ yue) at 51866; 0 = an English-only vocabulary, which has none */
static inline int tk_whisper_n_lang(int n_vocab) { return n_vocab >= 51865 ? n_vocab - 51865 + 99 : 0; }

/* is v above -inf?  false for -inf and for a NaN */
TK_HD bool tk_lang_live(float v) { return v > tk_bits_f32(0xff800000u); }

/* step 2 for one logit; any = some logit of the row is above -inf, m = the row's maximum */
TK_HD float tk_lang_weight(float l, float m, bool any) {
    if (!any || !tk_lang_live(l)) return 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
    const float d = l == m ? 0.0f : __fsub_rn(l, m);
#else
    const float d = l == m ? 0.0f : l - m;
#endif
    return tk_expf(d);
}

TK_HD float tk_lang_add(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(a, b);
#else
    return a + b;
#endif
}

/* step 4 */
TK_HD float tk_lang_prob(float p, float S, bool any) { return any ? tk_divf(p, S) : 0.0f; }

/* one row on the host: the kernel's lanes in a loop.  probs (optional): [n_lang].  Returns the language id; *prob_id = prob[id] */
static inline int32_t tk_lang_pick_row(const float* l, int n_lang, float* prob_id, float* probs) {
    float best = tk_bits_f32(0xff800000u);
    int32_t id = 0;
    bool any = false;
    for (int i = 0; i < n_lang; ++i)
        if (l[i] > best) { best = l[i]; id = i; any = true; }
    const float m = l[id];
    float S = 0.0f;
    for (int i = 0; i < n_lang; ++i) S = tk_lang_add(S, tk_lang_weight(l[i], m, any));
    for (int i = 0; probs && i < n_lang; ++i) probs[i] = tk_lang_prob(tk_lang_weight(l[i], m, any), S, any);
    if (prob_id) *prob_id = tk_lang_prob(tk_lang_weight(l[id], m, any), S, any);
    return id;
}

/* the limits of one launch (rows of `cols` logits, `ld` apart), checked before either side runs; the message names the first one broken */
static inline const char* tk_lang_pick_check(int64_t rows, int64_t cols, int64_t ld, int64_t tok0, int64_t n_lang) {
    if (rows < 1 || rows > 4096) return "rows must be in [1, 4096]";
    if (n_lang < 1 || n_lang > TK_LANG_MAX) return "n_lang must be in [1, 128]";
    if (cols < 1 || tok0 < 0 || tok0 + n_lang > cols) return "the language tokens must lie inside the row";
    if (ld < cols) return "ld must be at least cols";
    return nullptr;
}

#endif
