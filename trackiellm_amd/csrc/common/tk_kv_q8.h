/*
 * tk_kv_q8.h — the Q8_0 KV cache: what a cached key or value row becomes, and what attention reads back (host + device).
 *
 * llama.cpp hosts shrink the cache with --cache-type-k q8_0 --cache-type-v q8_0: a row is stored as ggml's Q8_0 blocks, 32 int8 values and one
 * f16 scale, 34 bytes where the f16 cache takes 64.  Here a Q8_0 row is a function of the row the f16 cache would hold: x[i] = the f16-rounded
 * key (after RoPE) or value, widened to fp32 — this project's choice (ggml quantises the fp32 value); it makes the Q8_0 cache a function of the
 * f16 cache.  Per block of 32, value for value ggml's quantize_row_q8_0_ref:
 *     amax = max |x|;  d = amax / 127;  id = d ? 1 / d : 0;  q[i] = roundf(x[i] * id);  stored scale = f16(d)
 * and the value of a cached element is f16_to_f32(scale) * (float)q — exact in fp32 (11 significant bits times 7).
 *
 * The cache layout is the project's own, not ggml's 34-byte struct: int8 values [layer][seq][kv head][max_ctx][head_dim] and f16 scales
 * [layer][seq][kv head][max_ctx][head_dim / 32], for K and for V.
 *
 * tk_kv_q8_attention_row is k_attention_far's arithmetic (llm/tk_llm_kernels.hip) of one (row, block of query heads) in a plain host loop, with
 * the element value above where the f16 kernels widen a cached f16: host and device outputs agree bit for bit.
 */
#ifndef TK_KV_Q8_H
#define TK_KV_Q8_H

#include <stdint.h>

#include "tk_exact_math.h"

#define TK_KV_F16 0
#define TK_KV_Q8_0 1
#define TK_KV_Q8_BLOCK 32

/* roundf for |v| < 2^23: halves away from zero.  The integer part and the remainder are both exact, so nothing is rounded before the comparison
 * (truncf(v + 0.5f) is not: 0.49999997f + 0.5f rounds up to 1) */
TK_HD float tk_kv_q8_roundf(float v) {
    const float t = (float)(int32_t)v; /* truncation toward zero */
    const float r = v - t;
    return r >= 0.5f ? t + 1.0f : r <= -0.5f ? t - 1.0f : t;
}

/* one block: x[32] fp32 (already f16-representable in the cache's use) -> q[32], the scale's f16 bits */
TK_HD uint16_t tk_kv_q8_block(const float* x, int8_t* q) {
    float amax = 0.0f;
    for (int i = 0; i < TK_KV_Q8_BLOCK; ++i) amax = tk_fmaxf(amax, tk_fabsf(x[i]));
    const float d = tk_divf(amax, 127.0f);
    const float id = d != 0.0f ? tk_divf(1.0f, d) : 0.0f;
    for (int i = 0; i < TK_KV_Q8_BLOCK; ++i) q[i] = (int8_t)(int32_t)tk_kv_q8_roundf(x[i] * id);
    return tk_f32_to_f16(d);
}

/* the value of a cached element */
TK_HD float tk_kv_q8_value(uint16_t scale, int8_t q) { return tk_f16_to_f32(scale) * (float)q; }

/* one f16 row of head_dim values (head_dim % 32 == 0) -> its int8 values and head_dim / 32 scales */
static inline void tk_kv_q8_row(const uint16_t* row, int head_dim, int8_t* q, uint16_t* d) {
    for (int b = 0; b < head_dim / TK_KV_Q8_BLOCK; ++b) {
        float x[TK_KV_Q8_BLOCK];
        for (int i = 0; i < TK_KV_Q8_BLOCK; ++i) x[i] = tk_f16_to_f32(row[b * TK_KV_Q8_BLOCK + i]);
        d[b] = tk_kv_q8_block(x, q + b * TK_KV_Q8_BLOCK);
    }
}

/* the attention of one (row, block of gq <= 4 query heads) over positions 0 .. T - 1 of one (sequence, KV head) run: kq / vq point at position 0
 * of the run's int8 values ([.][head_dim]), kd / vd at its scales ([.][head_dim / 32]); q [gq][head_dim]; out [gq][head_dim] = the quotient
 * k_attention_far hands to quantize_chunk8.  Order: a score is one fma chain over head_dim, ascending, times att_scale; the maximum; tk_expf;
 * PV and the denominator as four sums by position mod 4, each in ascending position order; ((p0 + p1) + p2) + p3; tk_divf.  (The kernel's dead
 * batch slots enter as fma(0, v, acc) and l + 0 with a finite v: they change no bit, so the loop leaves them out.)
 * scratch: T * gq floats */
static inline void tk_kv_q8_attention_row(const float* q, int gq, int head_dim, int T, const int8_t* kq, const uint16_t* kd, const int8_t* vq, const uint16_t* vd,
                                          float* scratch, float* out) {
    const int nb = head_dim / TK_KV_Q8_BLOCK;
    const float att_scale = tk_divf(1.0f, tk_sqrtf((float)head_dim));
    float m[4] = {0, 0, 0, 0};
    for (int h = 0; h < gq; ++h) {
        for (int t = 0; t < T; ++t) {
            float a = 0.0f;
            for (int i = 0; i < head_dim; ++i) a = tk_fmaf(q[h * head_dim + i], tk_kv_q8_value(kd[(size_t)t * nb + i / TK_KV_Q8_BLOCK], kq[(size_t)t * head_dim + i]), a);
            a = a * att_scale;
            scratch[(size_t)t * gq + h] = a;
            m[h] = t == 0 ? a : tk_fmaxf(m[h], a);
        }
        for (int t = 0; t < T; ++t) scratch[(size_t)t * gq + h] = tk_expf(scratch[(size_t)t * gq + h] - m[h]);
    }
    for (int h = 0; h < gq; ++h) {
        float l[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int t = 0; t < T; ++t) l[t & 3] = l[t & 3] + scratch[(size_t)t * gq + h];
        const float ll = ((l[0] + l[1]) + l[2]) + l[3];
        for (int i = 0; i < head_dim; ++i) {
            float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int t = 0; t < T; ++t)
                acc[t & 3] = tk_fmaf(scratch[(size_t)t * gq + h], tk_kv_q8_value(vd[(size_t)t * nb + i / TK_KV_Q8_BLOCK], vq[(size_t)t * head_dim + i]), acc[t & 3]);
            out[h * head_dim + i] = tk_divf(((acc[0] + acc[1]) + acc[2]) + acc[3], ll);
        }
    }
}

#endif
