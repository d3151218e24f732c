/*
 * tk_kv_shift.h — context shift: what becomes of a KV cache row that moves to a lower position (host + device).
 *
 * llama.cpp's hosts (main, server) answer a full context by keeping the first n_keep tokens, dropping half of the rest and moving the surviving
 * cache rows down (llama_kv_cache_seq_rm + llama_kv_cache_seq_add); its K-shift then re-rotates every moved key to its new position.  The cache
 * here is position-indexed and K is stored AFTER RoPE (k_qkv_rope_append, llm/tk_llm_kernels.hip), so a row that moves from position p to
 * p + delta (delta < 0, d = -delta) is a copy for V and a rotation by -d positions for K: for every adjacent pair (a, b) of the key row, widened
 * from f16 to fp32, with c = rope_cos[d][i], s = rope_sin[d][i] of the session's own tables,
 *     k'[2i]     = f16( fma( b, s, a * c) )
 *     k'[2i + 1] = f16( fma(-a, s, b * c) )
 * the product rounded to fp32 first, then the fma: k_qkv_rope_append's form with the sine negated.  The key is rounded to f16 a second time (it was
 * rounded once when it was appended); llama.cpp's K-shift on an f16 cache does the same.  A NaN stays a NaN; its payload is not specified.
 *
 * The functions below work on one 16-byte word of a row (8 f16 values = 4 pairs), which is what one lane of k_kv_shift_rows holds in registers
 * between its load and its store and what tk_kv_shift_run walks in a host loop: host and device rows agree bit for bit.
 */
#ifndef TK_KV_SHIFT_H
#define TK_KV_SHIFT_H

#include <stdint.h>
#include <string.h>

#include "tk_exact_math.h"

#define TK_KV_SHIFT_BLOCK_ROWS 128 /* rows one workgroup of k_kv_shift_rows holds in registers between a barrier and its stores */

/* one move: rows [p0, p1) of sequence seq become rows [p0 + delta, p1 + delta) */
struct TkKvShiftDesc {
    int32_t seq, p0, p1, delta;
};

/* the limits a move must keep before either side may run it */
TK_HD bool tk_kv_shift_ok(const TkKvShiftDesc& m, int max_seq, int max_ctx) {
    return m.seq >= 0 && m.seq < max_seq && m.p0 >= 0 && m.p0 < m.p1 && m.p1 <= max_ctx && m.delta < 0 && m.p0 + m.delta >= 0;
}

/* one pair of a key row */
TK_HD void tk_kv_shift_pair(uint16_t* k0, uint16_t* k1, float c, float s) {
    const float a = tk_f16_to_f32(*k0), b = tk_f16_to_f32(*k1);
    *k0 = tk_f32_to_f16(tk_fmaf(b, s, a * c));
    *k1 = tk_f32_to_f16(tk_fmaf(-a, s, b * c));
}

/* one 16-byte word of a key row: w[4] holds pairs 4j .. 4j + 3 of the row, c4 / s4 the table entries [d][4j .. 4j + 3] */
TK_HD void tk_kv_shift_word(uint32_t w[4], const float c4[4], const float s4[4]) {
    for (int j = 0; j < 4; ++j) {
        uint16_t lo = (uint16_t)(w[j] & 0xffffu), hi = (uint16_t)(w[j] >> 16);
        tk_kv_shift_pair(&lo, &hi, c4[j], s4[j]);
        w[j] = (uint32_t)lo | ((uint32_t)hi << 16);
    }
}

/* one (layer, KV head, K | V) run on the host: `run` points at position 0 of the run ([max_ctx][head_dim] f16).  Rows ascend, so a source row is
 * read before a destination row that lies on it is written (the destination lies below the source) */
static inline void tk_kv_shift_run(uint16_t* run, bool is_k, const TkKvShiftDesc& m, int head_dim, const float* rope_cos, const float* rope_sin) {
    const int d = -m.delta, half = head_dim / 2;
    for (int p = m.p0; p < m.p1; ++p) {
        const uint16_t* src = run + (size_t)p * head_dim;
        uint16_t* dst = run + (size_t)(p - d) * head_dim;
        for (int j = 0; j < head_dim / 8; ++j) {
            uint32_t w[4];
            memcpy(w, src + 8 * j, 16);
            if (is_k) tk_kv_shift_word(w, rope_cos + (size_t)d * half + 4 * j, rope_sin + (size_t)d * half + 4 * j);
            memcpy(dst + 8 * j, w, 16);
        }
    }
}

#endif
