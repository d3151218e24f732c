/*
 * tk_ggml_blocks.h — on-disk (GGUF) block formats of the ggml k-quants used by
 * Mistral-7B Q4_K_M, plus the deterministic quantisers this build uses to make
 * synthetic checkpoints and test GGUFs.
 *
 * The formats are the public ggml layouts (third-party: ggml-org/llama.cpp,
 * un-pinned and absent from /root/reference — SURVEY.md §0 F1, §8c).  The
 * reference only ever passes the file path to llama.cpp
 * (src/ai_models/tk_model_loader.c:245-251), so these structs are restated from
 * the published format description, not from reference code:
 *   Q4_K: 256 weights / 144 B: f16 d, f16 dmin, 12 B of packed 6-bit
 *         (scale, min) pairs for 8 sub-blocks of 32, 128 B of 4-bit quants.
 *         w = d*sc[j]*q - dmin*m[j]
 *   Q6_K: 256 weights / 210 B: 128 B low nibbles, 64 B high 2-bit pairs,
 *         16 int8 scales (groups of 16), f16 d.   w = d*sc[g]*(q-32)
 *   Q5_K: 256 weights / 176 B: Q4_K's d, dmin and 12 B of (scale, min) pairs,
 *         32 B of high bits (bit j of qh[l] = weight 32 j + l), 128 B of low
 *         nibbles laid out as Q4_K's.   w = d*sc[j]*q - dmin*m[j], q in 0..31
 *   Q3_K: 256 weights / 110 B: 32 B of high bits (bit 4 n + j of hmask[l] =
 *         weight 128 n + 32 j + l), 64 B of low 2-bit pairs, 12 B of packed
 *         6-bit scales (groups of 16), f16 d.   w = d*(sc[g]-32)*q, q in -4..3
 *   Q2_K: 256 weights / 84 B: 16 B of (scale, min) nibble pairs (groups of
 *         16: low nibble the scale, high nibble the min), 64 B of 2-bit quants
 *         (weight 128 n + 32 j + l = (qs[32 n + l] >> 2 j) & 3), f16 d, f16
 *         dmin.   w = d*sc[g]*q - dmin*m[g], q in 0..3
 *   Q8_0: 32 weights / 34 B: f16 d, 32 int8 quants.   w = d*q (exact in fp32), every int8 value legal, -128 included
 *   Q4_0: 32 weights / 18 B: f16 d, 16 B of nibbles (weight j = qs[j] & 15, weight j + 16 = qs[j] >> 4, j = 0..15).
 *         w = d*(q-8), q in 0..15 (exact in fp32): the Q8_0 block with the same d and q8 = q - 8
 *   Q5_0: 32 weights / 22 B: f16 d, 4 B of high bits (one little-endian u32: bit i = bit 4 of weight i), 16 B of nibbles laid out
 *         as Q4_0's.   w = d*(q-16), q in 0..31 (exact in fp32): the Q8_0 block with the same d and q8 = q - 16
 *   Q4_1: 32 weights / 20 B: f16 d, f16 m, 16 B of nibbles laid out as Q4_0's.   w = d*q + m, q in 0..15: d*q is exact in fp32, the add
 *         rounds once, so the decode is fmaf(d, q, m)
 *   Q5_1: 32 weights / 24 B: f16 d, f16 m, 4 B of high bits and 16 B of nibbles as Q5_0's.   w = d*q + m = fmaf(d, q, m), q in 0..31
 *   IQ4_NL: 32 weights / 18 B: the Q4_0 block's bytes, the nibble an index into the 16-entry code book tk_iq4_kv.
 *         w = d*kv[q] (exact in fp32): the Q8_0 block with the same d and q8 = kv[q]
 *   IQ4_XS: 256 weights / 136 B: f16 d, u16 scales_h (little endian), scales_l[4], 128 B of nibbles (sub-block j of 32 weights =
 *         qs[16 j .. 16 j + 15], ordered as an IQ4_NL block).  ls_j = ((scales_l[j / 2] >> 4 (j % 2)) & 15) | ((scales_h >> 2 j) & 3) << 4,
 *         s_j = ls_j - 32 in -32..31, w = (d*s_j)*kv[q], both products exact in fp32 (11 bits times 6, then 17 times 7)
 *   TQ2_0: 256 weights / 66 B: 64 B of 2-bit codes (weight 128 h + 32 l + m = (qs[32 h + m] >> 2 l) & 3), f16 d LAST.
 *         w = (c - 1)*d, c in 0..3: the quantiser writes 0..2, code 3 is a valid byte and decodes to +2 d
 *   TQ1_0: 256 weights / 54 B: 48 B qs and 4 B qh of base-3 digits (five trits a byte, four in qh), f16 d LAST.  Trit n of byte b is
 *         ((uint16_t)(uint8_t)(b * 3^n) * 3) >> 8, in 0..2 for every byte value; weights 0..159 = trit n of qs[m] at 32 n + m,
 *         160..239 = trit n of qs[32 + m] at 160 + 16 n + m, 240..255 = trit n of qh[j] at 240 + 4 n + j.   w = (t - 1)*d
 *         Both are the Q6_K block with the same d, all sixteen scales 1 and q6 = 32 + (t - 1)
 * Host + device code (the quantisers run inside the synthetic-weight kernel
 * and inside the oracle; they are bit-identical by construction).
 */
#ifndef TK_GGML_BLOCKS_H
#define TK_GGML_BLOCKS_H

#include <stddef.h>

#include "tk_exact_math.h"
#include "../llm/tk_llm_layout.h" /* TK_Q*K_TILE_BYTES feed the table's tile_bytes */

#define TK_QK_K 256

enum tk_ggml_type {
    TK_TYPE_F32 = 0,
    TK_TYPE_F16 = 1,
    TK_TYPE_Q4_0 = 2,
    TK_TYPE_Q4_1 = 3,
    TK_TYPE_Q5_0 = 6,
    TK_TYPE_Q5_1 = 7,
    TK_TYPE_Q8_0 = 8,
    TK_TYPE_Q2_K = 10,
    TK_TYPE_Q3_K = 11,
    TK_TYPE_Q4_K = 12,
    TK_TYPE_Q5_K = 13,
    TK_TYPE_Q6_K = 14,
    TK_TYPE_IQ4_NL = 20,
    TK_TYPE_IQ4_XS = 23,
    TK_TYPE_BF16 = 30,
    TK_TYPE_TQ1_0 = 34,
    TK_TYPE_TQ2_0 = 35,
};

typedef struct {
    uint16_t d;
    uint16_t dmin;
    uint8_t scales[12];
    uint8_t qs[128];
} tk_block_q4_K; /* 144 B */

typedef struct {
    uint16_t d;
    uint16_t dmin;
    uint8_t scales[12];
    uint8_t qh[32];
    uint8_t qs[128];
} tk_block_q5_K; /* 176 B */

typedef struct {
    uint8_t ql[128];
    uint8_t qh[64];
    int8_t scales[16];
    uint16_t d;
} tk_block_q6_K; /* 210 B */

typedef struct {
    uint8_t hmask[32];
    uint8_t qs[64];
    uint8_t scales[12];
    uint16_t d;
} tk_block_q3_K; /* 110 B */

typedef struct {
    uint8_t scales[16];
    uint8_t qs[64];
    uint16_t d;
    uint16_t dmin;
} tk_block_q2_K; /* 84 B */

typedef struct {
    uint16_t d;
    int8_t qs[32];
} tk_block_q8_0; /* 34 B, 32 weights */

typedef struct {
    uint16_t d;
    uint8_t qs[16];
} tk_block_q4_0; /* 18 B, 32 weights */

typedef struct {
    uint16_t d;
    uint8_t qh[4]; /* one little-endian u32 */
    uint8_t qs[16];
} tk_block_q5_0; /* 22 B, 32 weights */

typedef struct {
    uint16_t d;
    uint16_t m;
    uint8_t qs[16];
} tk_block_q4_1; /* 20 B, 32 weights */

typedef struct {
    uint16_t d;
    uint16_t m;
    uint8_t qh[4]; /* one little-endian u32 */
    uint8_t qs[16];
} tk_block_q5_1; /* 24 B, 32 weights */

typedef struct {
    uint16_t d;
    uint8_t qs[16];
} tk_block_iq4_nl; /* 18 B, 32 weights: the Q4_0 block's layout */

typedef struct {
    uint16_t d;
    uint16_t scales_h; /* little endian: bits 2 j, 2 j + 1 = the high two bits of sub-block j's 6-bit scale */
    uint8_t scales_l[4];
    uint8_t qs[128];
} tk_block_iq4_xs; /* 136 B, 256 weights */

typedef struct {
    uint8_t qs[64];
    uint16_t d;
} tk_block_tq2_0; /* 66 B, 256 weights; d is last */

typedef struct {
    uint8_t qs[48];
    uint8_t qh[4];
    uint16_t d;
} tk_block_tq1_0; /* 54 B, 256 weights; d is last */

/* the non-linear code book of IQ4_NL / IQ4_XS (ggml's published kvalues_iq4nl), indexed by the stored nibble */
/* -127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113 as the bytes of two constants: a shift and a sign extension on
 * host and device, no table in memory */
TK_HD constexpr int tk_iq4_kv(int q) {
    return (int)(int8_t)(uint8_t)((q < 8 ? 0xF6EADDCFBFAD9881ull : 0x7159453526190D01ull) >> (8 * (q & 7)));
}
static_assert(tk_iq4_kv(0) == -127 && tk_iq4_kv(1) == -104 && tk_iq4_kv(2) == -83 && tk_iq4_kv(3) == -65 && tk_iq4_kv(4) == -49 && tk_iq4_kv(5) == -35 &&
              tk_iq4_kv(6) == -22 && tk_iq4_kv(7) == -10 && tk_iq4_kv(8) == 1 && tk_iq4_kv(9) == 13 && tk_iq4_kv(10) == 25 && tk_iq4_kv(11) == 38 &&
              tk_iq4_kv(12) == 53 && tk_iq4_kv(13) == 69 && tk_iq4_kv(14) == 89 && tk_iq4_kv(15) == 113, "tk_iq4_kv: ggml's kvalues_iq4nl");

/* The tensor types, described once: what the loaders, the launchers and the W4A8 kernels ask about a type is a column of this table, and
 * a new type is one more row ("Adding a tensor type") */
struct tk_type_desc {
    const char* name;              /* null: no type of this build; it is sized like F32, as it always was, and refused by tk_type_known() */
    int block_elems, block_bytes;
    int tile_bytes;                /* the W4A8 weight tile of 16 rows x 256 k (tk_llm_layout.h); 0 = not a k-quant */
    int mask, kernel_index;        /* its bit in the kernels' TYPES argument; its column in k_gemv_fns / k_gemm_fns / k_gemm32_fns */
    bool shares_launch;            /* may ride in one launch beside another such type (the Q4_K | Q6_K kernels); tk_launch_gemv splits any other mix */
    bool token_embd, lora_merge;   /* k_embed decodes it; k_lora_merge re-quantises it */
    bool host_quantize;            /* tk_mi355x_quantize_blocks takes it (a pinned set: Q2_K, Q4_0, Q4_1, Q5_0, Q5_1, IQ4_NL, IQ4_XS, TQ1_0 and TQ2_0 have entry points of their own) */
};
TK_HD constexpr tk_type_desc tk_type_desc_of(int type) {
    switch (type) {
        /*                         name    elems bytes tile               mask idx shares embd   lora   host_q */
        case TK_TYPE_F32:  return {"F32",  1,    4,    0,                 0,   -1, false, true,  true,  false};
        case TK_TYPE_BF16: return {"BF16", 1,    2,    0,                 0,   -1, false, true,  true,  false};
        case TK_TYPE_F16:  return {"F16",  1,    2,    0,                 0,   -1, false, true,  true,  false};
        case TK_TYPE_Q4_0: return {"Q4_0", 32,   18,   TK_Q4_0_TILE_BYTES, 64, 7,  false, true,  false, false};
        case TK_TYPE_Q5_0: return {"Q5_0", 32,   22,   TK_Q5_0_TILE_BYTES, 128, 8, false, true,  false, false};
        case TK_TYPE_Q4_1: return {"Q4_1", 32,   20,   TK_Q4_1_TILE_BYTES, 1024, 11, false, true, false, false};
        case TK_TYPE_Q5_1: return {"Q5_1", 32,   24,   TK_Q5_1_TILE_BYTES, 2048, 12, false, true, false, false};
        case TK_TYPE_Q8_0: return {"Q8_0", 32,   34,   TK_Q8_0_TILE_BYTES, 32, 6,  false, true,  false, true};
        case TK_TYPE_Q2_K: return {"Q2_K", 256,  84,   TK_Q2K_TILE_BYTES, 16,  5,  false, true,  false, false};
        case TK_TYPE_Q3_K: return {"Q3_K", 256,  110,  TK_Q3K_TILE_BYTES, 8,   4,  false, true,  false, true};
        case TK_TYPE_Q4_K: return {"Q4_K", 256,  144,  TK_Q4K_TILE_BYTES, 1,   0,  true,  true,  true,  true};
        case TK_TYPE_Q5_K: return {"Q5_K", 256,  176,  TK_Q5K_TILE_BYTES, 4,   3,  false, true,  false, true};
        case TK_TYPE_Q6_K: return {"Q6_K", 256,  210,  TK_Q6K_TILE_BYTES, 2,   1,  true,  true,  true,  true};
        case TK_TYPE_IQ4_NL: return {"IQ4_NL", 32, 18, TK_IQ4_NL_TILE_BYTES, 256, 9, false, true, false, false};
        case TK_TYPE_IQ4_XS: return {"IQ4_XS", 256, 136, TK_IQ4_XS_TILE_BYTES, 512, 10, false, true, false, false};
        /* TQ1_0 is installed as the TQ2_0 tile (TkBlock<TK_TYPE_TQ1_0>::code is the decoded trit: the repack decodes the base-3 bytes once, at load): the same tile bytes, mask and
         * kernel column, so a TQ1_0 matrix runs the instantiations a TQ2_0 matrix runs and streams 66, not 54, bytes per 256 weights */
        case TK_TYPE_TQ2_0: return {"TQ2_0", 256, 66, TK_TQ2_0_TILE_BYTES, 4096, 13, false, true, false, false};
        case TK_TYPE_TQ1_0: return {"TQ1_0", 256, 54, TK_TQ2_0_TILE_BYTES, 4096, 13, false, true, false, false};
        default:           return {nullptr, 1,   4,    0,                 0,   -1, false, false, false, false};
    }
}
/* the lists the messages print: kept beside the table, edited with it */
#define TK_TYPE_NAMES "F32, F16, BF16, Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q2_K, Q3_K, Q4_K, Q5_K, Q6_K, IQ4_NL, IQ4_XS, TQ1_0, TQ2_0"
#define TK_TYPE_NAMES_OR "F32, F16, BF16, Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q2_K, Q3_K, Q4_K, Q5_K, Q6_K, IQ4_NL, IQ4_XS, TQ1_0 or TQ2_0"
#define TK_KQUANT_NAMES_OR "Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q2_K, Q3_K, Q4_K, Q5_K, Q6_K, IQ4_NL, IQ4_XS, TQ1_0 or TQ2_0"
#define TK_TOKEN_EMBD_NAMES_OR "Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q2_K, Q3_K, Q4_K, Q5_K, Q6_K, IQ4_NL, IQ4_XS, TQ1_0, TQ2_0, F16, BF16 or F32"
#define TK_LORA_MERGE_NAMES_OR "Q4_K, Q6_K, F16, BF16 or F32"
/* the float matrix types: tiles of the exact fp32 GEMM (nn/tk_gemm_tiled.h), 2 or 4 bytes a weight.  A model holds at most one of them among
 * its matrices: the sessions' operand image carries one rounding (tk_type_float_round) */
TK_HD constexpr bool tk_type_is_float(int type) { return type == TK_TYPE_F32 || type == TK_TYPE_F16 || type == TK_TYPE_BF16; }
TK_HD constexpr int tk_type_float_round(int type) { return type == TK_TYPE_F16 ? TK_ROUND_F16 : type == TK_TYPE_BF16 ? TK_ROUND_BF16 : TK_ROUND_NONE; }

TK_HD constexpr bool tk_type_known(int type) { return tk_type_desc_of(type).name != nullptr; }
TK_HD constexpr bool tk_type_is_kquant(int type) { return tk_type_desc_of(type).tile_bytes != 0; }
TK_HD constexpr size_t tk_type_block_bytes(int type) { return (size_t)tk_type_desc_of(type).block_bytes; }
TK_HD constexpr size_t tk_type_block_elems(int type) { return (size_t)tk_type_desc_of(type).block_elems; }

/* TYPES of a W4A8 launch = the masks of its segments' types or-ed together.  The launchers make fourteen values: the thirteen tile layouts
 * alone (TQ1_0 has TQ2_0's) and the one mix of the two shares_launch types, whose kernels pick the tile type per segment at run time. */
/* the tiled types (tile_bytes != 0), listed: their enum values are not one range (Q4_0 = 2, Q4_1 = 3, Q5_0 = 6, Q5_1 = 7, Q8_0 = 8, the k-quants 10 .. 14, IQ4_NL = 20, IQ4_XS = 23, TQ1_0 = 34, TQ2_0 = 35), and a
 * loop over [first, last] would lean on the types between having no row */
#define TK_TILED_TYPES 14
TK_HD constexpr int tk_tiled_type(int i) {
    constexpr int types[TK_TILED_TYPES] = {TK_TYPE_Q4_0, TK_TYPE_Q5_0, TK_TYPE_Q8_0, TK_TYPE_Q2_K, TK_TYPE_Q3_K, TK_TYPE_Q4_K, TK_TYPE_Q5_K, TK_TYPE_Q6_K,
                                             TK_TYPE_IQ4_NL, TK_TYPE_IQ4_XS, TK_TYPE_Q4_1, TK_TYPE_Q5_1, TK_TYPE_TQ2_0, TK_TYPE_TQ1_0};
    return types[i];
}

#define TK_TYPES_Q4K_Q6K (tk_type_desc_of(TK_TYPE_Q4_K).mask | tk_type_desc_of(TK_TYPE_Q6_K).mask)
#define TK_KERNEL_INDEX_Q4K_Q6K 2
#define TK_KERNEL_VARIANTS 14
TK_HD constexpr bool tk_types_has(int types, int type) { return (types & tk_type_desc_of(type).mask) != 0; }
TK_HD constexpr bool tk_types_is(int types, int type) { return types == tk_type_desc_of(type).mask; }
/* tile bytes of a single-type launch: a compile-time pitch (tile addresses become scalar base + immediate); 0 for the mix */
TK_HD constexpr size_t tk_types_tile_bytes(int types) {
    for (int i = 0; i < TK_TILED_TYPES; ++i)
        if (tk_types_is(types, tk_tiled_type(i))) return (size_t)tk_type_desc_of(tk_tiled_type(i)).tile_bytes;
    return 0;
}

/* every tiled type is listed once and nothing else has a tile; every tile layout's mask is one bit of its own, and the kernel indices of
 * the fourteen TYPES values are 0 .. 13, each once.  A type installed as another type's tile (TQ1_0 as TQ2_0's) carries that type's mask and has its tile
 * bytes, mask and index, and the other type is listed before it */
TK_HD constexpr bool tk_type_table_consistent() {
    int masks = 0, indices = 1 << TK_KERNEL_INDEX_Q4K_Q6K;
    int listed = 0;
    for (int t = 0; t < 64; ++t) listed += tk_type_is_kquant(t) ? 1 : 0;
    if (listed != TK_TILED_TYPES) return false;
    for (int i = 0; i < TK_TILED_TYPES; ++i) {
        const tk_type_desc d = tk_type_desc_of(tk_tiled_type(i));
        if (d.tile_bytes == 0) return false;
        if (tk_tiled_type(i) == TK_TYPE_TQ1_0) { /* the one row that repeats a mask: it must repeat the whole column of the type listed before it */
            const tk_type_desc as = tk_type_desc_of(TK_TYPE_TQ2_0);
            if (d.tile_bytes != as.tile_bytes || d.mask != as.mask || d.kernel_index != as.kernel_index || (masks & as.mask) == 0) return false;
            continue;
        }
        if (d.mask == 0 || (d.mask & (d.mask - 1)) != 0 || (masks & d.mask) != 0) return false;
        if (d.kernel_index < 0 || d.kernel_index >= TK_KERNEL_VARIANTS || ((indices >> d.kernel_index) & 1) != 0) return false;
        masks |= d.mask;
        indices |= 1 << d.kernel_index;
    }
    return indices == (1 << TK_KERNEL_VARIANTS) - 1;
}
static_assert(tk_type_table_consistent(), "tk_type_desc_of: tk_tiled_type must list the rows with a tile, masks must be distinct bits and kernel indices 0 .. 13, each once");

/* 6-bit (scale, min) pair j of a Q4_K block */
TK_HD void tk_q4k_get_scale_min(int j, const uint8_t* q, uint8_t* sc, uint8_t* m) {
    if (j < 4) {
        *sc = q[j] & 63;
        *m = q[j + 4] & 63;
    } else {
        *sc = (uint8_t)((q[j + 4] & 0x0F) | ((q[j - 4] >> 6) << 4));
        *m = (uint8_t)((q[j + 4] >> 4) | ((q[j] >> 6) << 4));
    }
}

TK_HD void tk_q4k_set_scale_min(int j, uint8_t* q, uint8_t sc, uint8_t m) {
    if (j < 4) {
        q[j] = (uint8_t)((q[j] & 0xC0) | sc);
        q[j + 4] = (uint8_t)((q[j + 4] & 0xC0) | m);
    } else {
        q[j + 4] = (uint8_t)((sc & 0x0F) | ((m & 0x0F) << 4));
        q[j - 4] = (uint8_t)((q[j - 4] & 0x3F) | ((sc >> 4) << 6));
        q[j] = (uint8_t)((q[j] & 0x3F) | ((m >> 4) << 6));
    }
}

/* weight i (0..255) of a Q4_K block as the integer triple the dot product uses */
TK_HD int tk_q4k_quant(const tk_block_q4_K* b, int i) {
    int c = i >> 6;          /* 64-weight chunk */
    int r = i & 63;
    uint8_t byte = b->qs[c * 32 + (r & 31)];
    return (r < 32) ? (byte & 0x0F) : (byte >> 4);
}

TK_HD float tk_q4k_dequant(const tk_block_q4_K* b, int i) {
    uint8_t sc, m;
    tk_q4k_get_scale_min(i >> 5, b->scales, &sc, &m);
    float d = tk_f16_to_f32(b->d), dmin = tk_f16_to_f32(b->dmin);
    return (d * (float)sc) * (float)tk_q4k_quant(b, i) - dmin * (float)m;
}

/* weight i (0..255) of a Q5_K block, q in [0,31]: the Q4_K nibble plus the high bit */
TK_HD int tk_q5k_quant(const tk_block_q5_K* b, int i) {
    int c = i >> 6;
    int r = i & 63;
    uint8_t byte = b->qs[c * 32 + (r & 31)];
    int lo = (r < 32) ? (byte & 0x0F) : (byte >> 4);
    return lo | (((b->qh[i & 31] >> (i >> 5)) & 1) << 4);
}

/* the expression of tk_q4k_dequant: a block with zero high bits dequantises to the Q4_K block's bits */
TK_HD float tk_q5k_dequant(const tk_block_q5_K* b, int i) {
    uint8_t sc, m;
    tk_q4k_get_scale_min(i >> 5, b->scales, &sc, &m);
    float d = tk_f16_to_f32(b->d), dmin = tk_f16_to_f32(b->dmin);
    return (d * (float)sc) * (float)tk_q5k_quant(b, i) - dmin * (float)m;
}

/* weight i (0..255) of a Q6_K block, q in [0,63] (the stored value, before -32) */
TK_HD int tk_q6k_quant(const tk_block_q6_K* b, int i) {
    int n = i >> 7;          /* 128-weight half */
    int r = i & 127;
    int l = r & 31;
    int quarter = r >> 5;    /* 0..3 */
    uint8_t qlb = b->ql[n * 64 + (quarter & 1) * 32 + l];
    int lo = (quarter < 2) ? (qlb & 0x0F) : (qlb >> 4);
    int hi = (b->qh[n * 32 + l] >> (2 * quarter)) & 3;
    return lo | (hi << 4);
}

TK_HD float tk_q6k_dequant(const tk_block_q6_K* b, int i) {
    float d = tk_f16_to_f32(b->d);
    return (d * (float)b->scales[i >> 4]) * (float)(tk_q6k_quant(b, i) - 32);
}

TK_HD void tk_q6k_set_quant(tk_block_q6_K* b, int i, int q) {
    int n = i >> 7, r = i & 127, l = r & 31, quarter = r >> 5;
    uint8_t* qlb = &b->ql[n * 64 + (quarter & 1) * 32 + l];
    if (quarter < 2) *qlb = (uint8_t)((*qlb & 0xF0) | (q & 0x0F));
    else *qlb = (uint8_t)((*qlb & 0x0F) | ((q & 0x0F) << 4));
    uint8_t* qhb = &b->qh[n * 32 + l];
    *qhb = (uint8_t)((*qhb & ~(3 << (2 * quarter))) | ((q >> 4) << (2 * quarter)));
}

/* weight i (0..255) of a Q3_K block, q in [-4,3]: the 2-bit pair plus 4 * the mask bit, minus 4 */
TK_HD int tk_q3k_quant(const tk_block_q3_K* b, int i) {
    int n = i >> 7, j = (i & 127) >> 5, l = i & 31;
    int lo = (b->qs[32 * n + l] >> (2 * j)) & 3;
    int hi = (b->hmask[l] >> (4 * n + j)) & 1;
    return lo + 4 * hi - 4;
}

/* scale of group g (0..15) of a Q3_K block: the stored 6 bits minus 32, in [-32,31] */
TK_HD int tk_q3k_scale(const tk_block_q3_K* b, int g) {
    int lo = g < 8 ? (b->scales[g] & 15) : (b->scales[g - 8] >> 4);
    int hi = (b->scales[8 + (g & 3)] >> (2 * (g >> 2))) & 3;
    return (lo | (hi << 4)) - 32;
}

TK_HD void tk_q3k_set_scale(tk_block_q3_K* b, int g, int s) {
    int v = s + 32;
    if (g < 8) b->scales[g] = (uint8_t)((b->scales[g] & 0xF0) | (v & 15));
    else b->scales[g - 8] = (uint8_t)((b->scales[g - 8] & 0x0F) | ((v & 15) << 4));
    uint8_t* h = &b->scales[8 + (g & 3)];
    *h = (uint8_t)((*h & ~(3 << (2 * (g >> 2)))) | ((v >> 4) << (2 * (g >> 2))));
}

/* the expression of tk_q6k_dequant: the Q6_K block with the same d, scales[g] = this scale and q6 = q + 32 dequantises to the same bits */
TK_HD float tk_q3k_dequant(const tk_block_q3_K* b, int i) {
    float d = tk_f16_to_f32(b->d);
    return (d * (float)tk_q3k_scale(b, i >> 4)) * (float)tk_q3k_quant(b, i);
}

TK_HD void tk_q3k_set_quant(tk_block_q3_K* b, int i, int q) {
    int n = i >> 7, j = (i & 127) >> 5, l = i & 31, u = q + 4;
    uint8_t* lo = &b->qs[32 * n + l];
    *lo = (uint8_t)((*lo & ~(3 << (2 * j))) | ((u & 3) << (2 * j)));
    uint8_t* hi = &b->hmask[l];
    *hi = (uint8_t)((*hi & ~(1 << (4 * n + j))) | ((u >> 2) << (4 * n + j)));
}

/* weight i (0..255) of a Q2_K block, q in [0,3] */
TK_HD int tk_q2k_quant(const tk_block_q2_K* b, int i) {
    int n = i >> 7, j = (i & 127) >> 5, l = i & 31;
    return (b->qs[32 * n + l] >> (2 * j)) & 3;
}

/* scale and min of group g (0..15) of a Q2_K block, both in [0,15] */
TK_HD int tk_q2k_scale(const tk_block_q2_K* b, int g) { return b->scales[g] & 15; }
TK_HD int tk_q2k_min(const tk_block_q2_K* b, int g) { return b->scales[g] >> 4; }

TK_HD void tk_q2k_set_scale(tk_block_q2_K* b, int g, int s) { b->scales[g] = (uint8_t)((b->scales[g] & 0xF0) | (s & 15)); }
TK_HD void tk_q2k_set_min(tk_block_q2_K* b, int g, int m) { b->scales[g] = (uint8_t)((b->scales[g] & 0x0F) | ((m & 15) << 4)); }

/* the expression of tk_q4k_dequant: the Q4_K block with the same d, dmin, (scale, min) and quants dequantises to the same bits */
TK_HD float tk_q2k_dequant(const tk_block_q2_K* b, int i) {
    float d = tk_f16_to_f32(b->d), dmin = tk_f16_to_f32(b->dmin);
    return (d * (float)tk_q2k_scale(b, i >> 4)) * (float)tk_q2k_quant(b, i) - dmin * (float)tk_q2k_min(b, i >> 4);
}

TK_HD void tk_q2k_set_quant(tk_block_q2_K* b, int i, int q) {
    int n = i >> 7, j = (i & 127) >> 5, l = i & 31;
    uint8_t* p = &b->qs[32 * n + l];
    *p = (uint8_t)((*p & ~(3 << (2 * j))) | ((q & 3) << (2 * j)));
}

/* weight i (0..31) of a Q8_0 block: d * q, exact in fp32 (11 significant bits times 8) */
TK_HD float tk_q8_0_dequant(const tk_block_q8_0* b, int i) { return tk_f16_to_f32(b->d) * (float)b->qs[i]; }

/* weight i (0..31) of a Q4_0 block, q in [0,15] (the stored value, before -8): weights 0..15 are the low nibbles, 16..31 the high ones */
TK_HD int tk_q4_0_quant(const tk_block_q4_0* b, int i) { return i < 16 ? (b->qs[i] & 15) : (b->qs[i - 16] >> 4); }
/* d * (q - 8), exact in fp32: the Q8_0 block with the same d and q8 = q - 8 dequantises to the same bits */
TK_HD float tk_q4_0_dequant(const tk_block_q4_0* b, int i) { return tk_f16_to_f32(b->d) * (float)(tk_q4_0_quant(b, i) - 8); }

/* weight i (0..31) of a Q5_0 block, q in [0,31] (before -16): the Q4_0 nibble plus bit i of the little-endian u32 qh */
TK_HD int tk_q5_0_quant(const tk_block_q5_0* b, int i) {
    const int lo = i < 16 ? (b->qs[i] & 15) : (b->qs[i - 16] >> 4);
    return lo | (((b->qh[i >> 3] >> (i & 7)) & 1) << 4);
}
TK_HD float tk_q5_0_dequant(const tk_block_q5_0* b, int i) { return tk_f16_to_f32(b->d) * (float)(tk_q5_0_quant(b, i) - 16); }

/* weight i (0..31) of a Q4_1 block, q in [0,15]: the Q4_0 nibble order.  w = d * q + m: the product is exact in fp32 (11 bits times 4), the
 * add rounds once, which is what one fma computes */
TK_HD int tk_q4_1_quant(const tk_block_q4_1* b, int i) { return i < 16 ? (b->qs[i] & 15) : (b->qs[i - 16] >> 4); }
TK_HD float tk_q4_1_dequant(const tk_block_q4_1* b, int i) { return tk_fmaf(tk_f16_to_f32(b->d), (float)tk_q4_1_quant(b, i), tk_f16_to_f32(b->m)); }

/* weight i (0..31) of a Q5_1 block, q in [0,31]: the Q5_0 nibble and high-bit order.  w = fmaf(d, q, m) (11 bits times 5) */
TK_HD int tk_q5_1_quant(const tk_block_q5_1* b, int i) {
    const int lo = i < 16 ? (b->qs[i] & 15) : (b->qs[i - 16] >> 4);
    return lo | (((b->qh[i >> 3] >> (i & 7)) & 1) << 4);
}
TK_HD float tk_q5_1_dequant(const tk_block_q5_1* b, int i) { return tk_fmaf(tk_f16_to_f32(b->d), (float)tk_q5_1_quant(b, i), tk_f16_to_f32(b->m)); }

/* stored nibble (the code-book index, 0..15) of weight i (0..31) of an IQ4_NL block or of one IQ4_XS sub-block, whose sixteen bytes qs
 * are laid out as Q4_0's */
TK_HD int tk_iq4_quant(const uint8_t* qs, int i) { return i < 16 ? (qs[i] & 15) : (qs[i - 16] >> 4); }
/* d * kv[q], exact in fp32: the Q8_0 block with the same d and q8 = kv[q] dequantises to the same bits */
TK_HD float tk_iq4nl_dequant(const tk_block_iq4_nl* b, int i) { return tk_f16_to_f32(b->d) * (float)tk_iq4_kv(tk_iq4_quant(b->qs, i)); }

/* scale of sub-block j (0..7) of an IQ4_XS block: the stored 6 bits minus 32, in [-32,31] */
TK_HD int tk_iq4xs_scale(const tk_block_iq4_xs* b, int j) {
    return (((b->scales_l[j >> 1] >> (4 * (j & 1))) & 15) | (((b->scales_h >> (2 * j)) & 3) << 4)) - 32;
}
TK_HD void tk_iq4xs_set_scale(tk_block_iq4_xs* b, int j, int s) {
    const int v = s + 32;
    uint8_t* l = &b->scales_l[j >> 1];
    *l = (uint8_t)((*l & ~(15 << (4 * (j & 1)))) | ((v & 15) << (4 * (j & 1))));
    b->scales_h = (uint16_t)((b->scales_h & ~(3 << (2 * j))) | ((v >> 4) << (2 * j)));
}
/* weight i (0..255): (d * s_j) * kv[q], one (exact) rounding per operation */
TK_HD float tk_iq4xs_dequant(const tk_block_iq4_xs* b, int i) {
    return (tk_f16_to_f32(b->d) * (float)tk_iq4xs_scale(b, i >> 5)) * (float)tk_iq4_kv(tk_iq4_quant(b->qs + 16 * (i >> 5), i & 31));
}

/* TQ2_0: code c in 0..3 of weight i (0..255); w = (c - 1) * d, exact in fp32.  Code 3 decodes to +2 d */
TK_HD int tk_tq2_0_quant(const tk_block_tq2_0* b, int i) { return (b->qs[32 * (i >> 7) + (i & 31)] >> (2 * ((i >> 5) & 3))) & 3; }
TK_HD float tk_tq2_0_dequant(const tk_block_tq2_0* b, int i) { return (float)(tk_tq2_0_quant(b, i) - 1) * tk_f16_to_f32(b->d); }

/* trit n (0..4) of a TQ1_0 byte: the byte times 3^n modulo 256, times 3, its ninth and tenth bit.  In 0..2 for every byte value */
TK_HD constexpr int tk_tq1_0_trit(uint8_t byte, int n) {
    return (int)(((uint16_t)(uint8_t)(byte * (uint8_t)(0x511B090301ull >> (8 * n))) * 3) >> 8); /* 3^n = 1, 3, 9, 27, 81 */
}
static_assert(tk_tq1_0_trit(255, 0) == 2 && tk_tq1_0_trit(255, 1) == 2 && tk_tq1_0_trit(255, 2) == 2 && tk_tq1_0_trit(255, 3) == 2 && tk_tq1_0_trit(255, 4) == 2 &&
              tk_tq1_0_trit(243, 0) == 2 && tk_tq1_0_trit(243, 1) == 2 && tk_tq1_0_trit(243, 2) == 1 && tk_tq1_0_trit(243, 3) == 1 && tk_tq1_0_trit(243, 4) == 2,
              "tk_tq1_0_trit: the non-canonical bytes 255 and 243");
/* TQ1_0: trit t in 0..2 of weight i (0..255): the three segments of the block */
TK_HD int tk_tq1_0_quant(const tk_block_tq1_0* b, int i) {
    if (i < 160) return tk_tq1_0_trit(b->qs[i & 31], i >> 5);
    if (i < 240) return tk_tq1_0_trit(b->qs[32 + ((i - 160) & 15)], (i - 160) >> 4);
    return tk_tq1_0_trit(b->qh[(i - 240) & 3], (i - 240) >> 2);
}
TK_HD float tk_tq1_0_dequant(const tk_block_tq1_0* b, int i) { return (float)(tk_tq1_0_quant(b, i) - 1) * tk_f16_to_f32(b->d); }

/*
 * Deterministic min/max quantisers ("the build's own Q4_K_M recipe").
 * Not llama.cpp's iterative search: one pass, IEEE ops only, so host and device
 * produce identical blocks.
 */
TK_HD void tk_quantize_q4_K(const float* x, tk_block_q4_K* out) {
    float scales[8], mins[8];
    float max_scale = 0.0f, max_min = 0.0f;
    for (int j = 0; j < 8; ++j) {
        float mn = x[32 * j], mx = x[32 * j];
        for (int i = 1; i < 32; ++i) {
            float v = x[32 * j + i];
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
        }
        if (mn > 0.0f) mn = 0.0f;
        scales[j] = tk_divf(mx - mn, 15.0f);
        if (scales[j] < 0.0f) scales[j] = 0.0f;
        mins[j] = -mn;
        max_scale = scales[j] > max_scale ? scales[j] : max_scale;
        max_min = mins[j] > max_min ? mins[j] : max_min;
    }
    float d = tk_divf(max_scale, 63.0f), dmin = tk_divf(max_min, 63.0f);
    out->d = tk_f32_to_f16(d);
    out->dmin = tk_f32_to_f16(dmin);
    float dq = tk_f16_to_f32(out->d), dminq = tk_f16_to_f32(out->dmin);
    for (int k = 0; k < 12; ++k) out->scales[k] = 0;
    for (int k = 0; k < 128; ++k) out->qs[k] = 0;
    for (int j = 0; j < 8; ++j) {
        int sc = dq > 0.0f ? (int)tk_rintf(tk_divf(scales[j], dq)) : 0;
        int m = dminq > 0.0f ? (int)tk_rintf(tk_divf(mins[j], dminq)) : 0;
        sc = sc > 63 ? 63 : sc;
        m = m > 63 ? 63 : m;
        tk_q4k_set_scale_min(j, out->scales, (uint8_t)sc, (uint8_t)m);
        float dl = dq * (float)sc, ml = dminq * (float)m;
        for (int i = 0; i < 32; ++i) {
            int q = 0;
            if (dl > 0.0f) {
                q = (int)tk_rintf(tk_divf(x[32 * j + i] + ml, dl));
                q = q < 0 ? 0 : (q > 15 ? 15 : q);
            }
            int idx = 32 * j + i;
            int c = idx >> 6, r = idx & 63;
            uint8_t* byte = &out->qs[c * 32 + (r & 31)];
            if (r < 32) *byte = (uint8_t)((*byte & 0xF0) | q);
            else *byte = (uint8_t)((*byte & 0x0F) | (q << 4));
        }
    }
}

/* tk_quantize_q4_K with 31 levels per sub-block */
TK_HD void tk_quantize_q5_K(const float* x, tk_block_q5_K* out) {
    float scales[8], mins[8];
    float max_scale = 0.0f, max_min = 0.0f;
    for (int j = 0; j < 8; ++j) {
        float mn = x[32 * j], mx = x[32 * j];
        for (int i = 1; i < 32; ++i) {
            float v = x[32 * j + i];
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
        }
        if (mn > 0.0f) mn = 0.0f;
        scales[j] = tk_divf(mx - mn, 31.0f);
        if (scales[j] < 0.0f) scales[j] = 0.0f;
        mins[j] = -mn;
        max_scale = scales[j] > max_scale ? scales[j] : max_scale;
        max_min = mins[j] > max_min ? mins[j] : max_min;
    }
    float d = tk_divf(max_scale, 63.0f), dmin = tk_divf(max_min, 63.0f);
    out->d = tk_f32_to_f16(d);
    out->dmin = tk_f32_to_f16(dmin);
    float dq = tk_f16_to_f32(out->d), dminq = tk_f16_to_f32(out->dmin);
    for (int k = 0; k < 12; ++k) out->scales[k] = 0;
    for (int k = 0; k < 32; ++k) out->qh[k] = 0;
    for (int k = 0; k < 128; ++k) out->qs[k] = 0;
    for (int j = 0; j < 8; ++j) {
        int sc = dq > 0.0f ? (int)tk_rintf(tk_divf(scales[j], dq)) : 0;
        int m = dminq > 0.0f ? (int)tk_rintf(tk_divf(mins[j], dminq)) : 0;
        sc = sc > 63 ? 63 : sc;
        m = m > 63 ? 63 : m;
        tk_q4k_set_scale_min(j, out->scales, (uint8_t)sc, (uint8_t)m);
        float dl = dq * (float)sc, ml = dminq * (float)m;
        for (int i = 0; i < 32; ++i) {
            int q = 0;
            if (dl > 0.0f) {
                q = (int)tk_rintf(tk_divf(x[32 * j + i] + ml, dl));
                q = q < 0 ? 0 : (q > 31 ? 31 : q);
            }
            int idx = 32 * j + i;
            int c = idx >> 6, r = idx & 63;
            uint8_t* byte = &out->qs[c * 32 + (r & 31)];
            if (r < 32) *byte = (uint8_t)((*byte & 0xF0) | (q & 15));
            else *byte = (uint8_t)((*byte & 0x0F) | ((q & 15) << 4));
            out->qh[i] = (uint8_t)(out->qh[i] | ((q >> 4) << j));
        }
    }
}

TK_HD void tk_quantize_q6_K(const float* x, tk_block_q6_K* out) {
    float gscale[16];
    float max_abs_scale = 0.0f;
    for (int g = 0; g < 16; ++g) {
        float amax = 0.0f;
        for (int i = 0; i < 16; ++i) {
            float a = tk_fabsf(x[16 * g + i]);
            amax = a > amax ? a : amax;
        }
        gscale[g] = tk_divf(amax, 31.0f);
        max_abs_scale = gscale[g] > max_abs_scale ? gscale[g] : max_abs_scale;
    }
    float d = tk_divf(max_abs_scale, 127.0f);
    out->d = tk_f32_to_f16(d);
    float dq = tk_f16_to_f32(out->d);
    for (int k = 0; k < 128; ++k) out->ql[k] = 0;
    for (int k = 0; k < 64; ++k) out->qh[k] = 0;
    for (int g = 0; g < 16; ++g) {
        int sc = dq > 0.0f ? (int)tk_rintf(tk_divf(gscale[g], dq)) : 0;
        sc = sc > 127 ? 127 : sc;
        out->scales[g] = (int8_t)sc;
        float dl = dq * (float)sc;
        for (int i = 0; i < 16; ++i) {
            int q = 32;
            if (dl > 0.0f) {
                q = (int)tk_rintf(tk_divf(x[16 * g + i], dl)) + 32;
                q = q < 0 ? 0 : (q > 63 ? 63 : q);
            }
            tk_q6k_set_quant(out, 16 * g + i, q);
        }
    }
}

/* Q3_K: eight levels -4..3 per group of 16 and a signed 6-bit group scale.  The sign of the group scale is chosen so that the
 * largest-magnitude weight of the group lands on -4 (the long side of the asymmetric range); d spreads the group scales over +-31 */
TK_HD void tk_quantize_q3_K(const float* x, tk_block_q3_K* out) {
    float gscale[16];
    float max_abs_scale = 0.0f;
    for (int g = 0; g < 16; ++g) {
        float amax = 0.0f, vmax = 0.0f;
        for (int i = 0; i < 16; ++i) {
            float a = tk_fabsf(x[16 * g + i]);
            if (a > amax) { amax = a; vmax = x[16 * g + i]; }
        }
        gscale[g] = tk_divf(-vmax, 4.0f);
        float as = tk_fabsf(gscale[g]);
        max_abs_scale = as > max_abs_scale ? as : max_abs_scale;
    }
    float d = tk_divf(max_abs_scale, 31.0f);
    out->d = tk_f32_to_f16(d);
    float dq = tk_f16_to_f32(out->d);
    for (int k = 0; k < 32; ++k) out->hmask[k] = 0;
    for (int k = 0; k < 64; ++k) out->qs[k] = 0;
    for (int k = 0; k < 12; ++k) out->scales[k] = 0;
    for (int g = 0; g < 16; ++g) {
        int sc = dq > 0.0f ? (int)tk_rintf(tk_divf(gscale[g], dq)) : 0;
        sc = sc < -32 ? -32 : (sc > 31 ? 31 : sc);
        tk_q3k_set_scale(out, g, sc);
        float dl = dq * (float)sc;
        for (int i = 0; i < 16; ++i) {
            int q = 0;
            if (dl != 0.0f) {
                q = (int)tk_rintf(tk_divf(x[16 * g + i], dl));
                q = q < -4 ? -4 : (q > 3 ? 3 : q);
            }
            tk_q3k_set_quant(out, 16 * g + i, q);
        }
    }
}

/* Q2_K: tk_quantize_q4_K with four levels per group of 16 and 4-bit fractions of d and dmin */
TK_HD void tk_quantize_q2_K(const float* x, tk_block_q2_K* out) {
    float scales[16], mins[16];
    float max_scale = 0.0f, max_min = 0.0f;
    for (int g = 0; g < 16; ++g) {
        float mn = x[16 * g], mx = x[16 * g];
        for (int i = 1; i < 16; ++i) {
            float v = x[16 * g + i];
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
        }
        if (mn > 0.0f) mn = 0.0f;
        scales[g] = tk_divf(mx - mn, 3.0f);
        if (scales[g] < 0.0f) scales[g] = 0.0f;
        mins[g] = -mn;
        max_scale = scales[g] > max_scale ? scales[g] : max_scale;
        max_min = mins[g] > max_min ? mins[g] : max_min;
    }
    float d = tk_divf(max_scale, 15.0f), dmin = tk_divf(max_min, 15.0f);
    out->d = tk_f32_to_f16(d);
    out->dmin = tk_f32_to_f16(dmin);
    float dq = tk_f16_to_f32(out->d), dminq = tk_f16_to_f32(out->dmin);
    for (int k = 0; k < 16; ++k) out->scales[k] = 0;
    for (int k = 0; k < 64; ++k) out->qs[k] = 0;
    for (int g = 0; g < 16; ++g) {
        int sc = dq > 0.0f ? (int)tk_rintf(tk_divf(scales[g], dq)) : 0;
        int m = dminq > 0.0f ? (int)tk_rintf(tk_divf(mins[g], dminq)) : 0;
        sc = sc > 15 ? 15 : sc;
        m = m > 15 ? 15 : m;
        tk_q2k_set_scale(out, g, sc);
        tk_q2k_set_min(out, g, m);
        float dl = dq * (float)sc, ml = dminq * (float)m;
        for (int i = 0; i < 16; ++i) {
            int q = 0;
            if (dl > 0.0f) {
                q = (int)tk_rintf(tk_divf(x[16 * g + i] + ml, dl));
                q = q < 0 ? 0 : (q > 3 ? 3 : q);
            }
            tk_q2k_set_quant(out, 16 * g + i, q);
        }
    }
}

/* Q8_0: ggml's published quantize_row_q8_0_ref, value for value: d = amax / 127, id = d ? 1 / d : 0, q = roundf(x * id) (half away
 * from zero), d stored as f16 */
TK_HD void tk_quantize_q8_0(const float* x, tk_block_q8_0* out) {
    float amax = 0.0f;
    for (int i = 0; i < 32; ++i) {
        float a = tk_fabsf(x[i]);
        amax = a > amax ? a : amax;
    }
    const float d = tk_divf(amax, 127.0f);
    const float id = d != 0.0f ? tk_divf(1.0f, d) : 0.0f;
    out->d = tk_f32_to_f16(d);
    for (int i = 0; i < 32; ++i) {
        const float v = x[i] * id, t = (float)(int)v; /* |v| <= 127 up to rounding: the truncation is exact */
        const float r = v - t;
        out->qs[i] = (int8_t)((int)t + (r >= 0.5f ? 1 : r <= -0.5f ? -1 : 0));
    }
}

/* Q4_0 / Q5_0: ggml's published quantize_row_q4_0_ref / quantize_row_q5_0_ref, value for value, all in binary32: max = the element of
 * largest magnitude with its sign (the first one on ties), d = max / -8 (-16), id = d ? 1 / d : 0 from the unrounded d, d stored as f16,
 * q = min(15 (31), (int8_t)(x * id + 8.5f (16.5f))): one multiply, one add, truncation.  x * id lies in [-8, 8] ([-16, 16]) up to
 * rounding, so the sum is in [0.49, 16.5] ([0.49, 32.5]) and the int8 conversion never wraps */
TK_HD void tk_quantize_q4_0(const float* x, tk_block_q4_0* out) {
    float amax = 0.0f, max = 0.0f;
    for (int i = 0; i < 32; ++i) {
        const float v = x[i];
        if (amax < tk_fabsf(v)) { amax = tk_fabsf(v); max = v; }
    }
    const float d = tk_divf(max, -8.0f);
    const float id = d != 0.0f ? tk_divf(1.0f, d) : 0.0f;
    out->d = tk_f32_to_f16(d);
    for (int j = 0; j < 16; ++j) {
        const float x0 = x[j] * id, x1 = x[16 + j] * id;
        int q0 = (int)(int8_t)(int)(x0 + 8.5f), q1 = (int)(int8_t)(int)(x1 + 8.5f);
        q0 = q0 > 15 ? 15 : q0;
        q1 = q1 > 15 ? 15 : q1;
        out->qs[j] = (uint8_t)((uint8_t)q0 | ((uint8_t)q1 << 4));
    }
}

TK_HD void tk_quantize_q5_0(const float* x, tk_block_q5_0* out) {
    float amax = 0.0f, max = 0.0f;
    for (int i = 0; i < 32; ++i) {
        const float v = x[i];
        if (amax < tk_fabsf(v)) { amax = tk_fabsf(v); max = v; }
    }
    const float d = tk_divf(max, -16.0f);
    const float id = d != 0.0f ? tk_divf(1.0f, d) : 0.0f;
    out->d = tk_f32_to_f16(d);
    uint32_t qh = 0;
    for (int j = 0; j < 16; ++j) {
        const float x0 = x[j] * id, x1 = x[16 + j] * id;
        int q0 = (int)(int8_t)(int)(x0 + 16.5f), q1 = (int)(int8_t)(int)(x1 + 16.5f);
        q0 = q0 > 31 ? 31 : q0;
        q1 = q1 > 31 ? 31 : q1;
        out->qs[j] = (uint8_t)((q0 & 15) | ((q1 & 15) << 4));
        qh |= (uint32_t)((q0 & 16) >> 4) << j;
        qh |= (uint32_t)((q1 & 16) >> 4) << (j + 16);
    }
    for (int k = 0; k < 4; ++k) out->qh[k] = (uint8_t)(qh >> (8 * k));
}

/* Q4_1 / Q5_1: ggml's published quantize_row_q4_1_ref / quantize_row_q5_1_ref, value for value, all in binary32: min and max the block's
 * smallest and largest element, d = (max - min) / 15 (31), id = d ? 1 / d : 0 from the unrounded d, d and m = min stored as f16,
 * q = min(15, (int8_t)((x - min) * id + 0.5f)) for Q4_1 and (uint8_t)((x - min) * id + 0.5f) for Q5_1, which takes no clamp:
 * (x - min) * id <= 31 (1 + a few 2^-24), so the sum stays below 32.  A constant block gives d = +0, q = 0, m = x */
TK_HD void tk_quantize_q4_1(const float* x, tk_block_q4_1* out) {
    float min = x[0], max = x[0];
    for (int i = 1; i < 32; ++i) {
        const float v = x[i];
        if (v < min) min = v;
        if (v > max) max = v;
    }
    const float d = tk_divf(max - min, 15.0f);
    const float id = d != 0.0f ? tk_divf(1.0f, d) : 0.0f;
    out->d = tk_f32_to_f16(d);
    out->m = tk_f32_to_f16(min);
    for (int j = 0; j < 16; ++j) {
        const float x0 = (x[j] - min) * id, x1 = (x[16 + j] - min) * id;
        int q0 = (int)(int8_t)(int)(x0 + 0.5f), q1 = (int)(int8_t)(int)(x1 + 0.5f);
        q0 = q0 > 15 ? 15 : q0;
        q1 = q1 > 15 ? 15 : q1;
        out->qs[j] = (uint8_t)((uint8_t)q0 | ((uint8_t)q1 << 4));
    }
}

TK_HD void tk_quantize_q5_1(const float* x, tk_block_q5_1* out) {
    float min = x[0], max = x[0];
    for (int i = 1; i < 32; ++i) {
        const float v = x[i];
        if (v < min) min = v;
        if (v > max) max = v;
    }
    const float d = tk_divf(max - min, 31.0f);
    const float id = d != 0.0f ? tk_divf(1.0f, d) : 0.0f;
    out->d = tk_f32_to_f16(d);
    out->m = tk_f32_to_f16(min);
    uint32_t qh = 0;
    for (int j = 0; j < 16; ++j) {
        const float x0 = (x[j] - min) * id, x1 = (x[16 + j] - min) * id;
        const int q0 = (int)(uint8_t)(int)(x0 + 0.5f), q1 = (int)(uint8_t)(int)(x1 + 0.5f);
        out->qs[j] = (uint8_t)((q0 & 15) | ((q1 & 15) << 4));
        qh |= (uint32_t)((q0 & 16) >> 4) << j;
        qh |= (uint32_t)((q1 & 16) >> 4) << (j + 16);
    }
    for (int k = 0; k < 4; ++k) out->qh[k] = (uint8_t)(qh >> (8 * k));
}

/* IQ4_NL / IQ4_XS: the build's own one-pass quantisers (IEEE operations only, so host and device make identical blocks), as Q3_K's and
 * Q2_K's are; ggml's IQ4 quantiser is an iterative search and is not restated.  The code-book index of a scaled value v = x * id is the
 * number of midpoints (kv[k] + kv[k + 1]) / 2 below it: the nearest code-book value, ties to the lower index */
/* the loops of these quantisers stay rolled in device code: unrolled and inlined, the 8 x 32 x 15 compares of one IQ4_XS block took the
 * device compiler a quarter of an hour.  The operations and their order are the same either way, so host and device blocks stay identical */
#if defined(__HIP_DEVICE_COMPILE__)
#define TK_ROLLED _Pragma("unroll 1")
#else
#define TK_ROLLED
#endif
TK_HD int tk_iq4_index(float v) {
    int q = 0;
    TK_ROLLED
    for (int k = 0; k < 15; ++k) q += v > (float)(tk_iq4_kv(k) + tk_iq4_kv(k + 1)) * 0.5f ? 1 : 0;
    return q;
}
/* the element of largest magnitude with its sign, the first one on ties */
TK_HD float tk_iq4_signed_max(const float* x) {
    float amax = 0.0f, max = 0.0f;
    TK_ROLLED
    for (int i = 0; i < 32; ++i) {
        const float v = x[i];
        if (amax < tk_fabsf(v)) { amax = tk_fabsf(v); max = v; }
    }
    return max;
}
TK_HD void tk_iq4_pack(const float* x, float id, uint8_t* qs) {
    TK_ROLLED
    for (int j = 0; j < 16; ++j) qs[j] = (uint8_t)(tk_iq4_index(x[j] * id) | (tk_iq4_index(x[16 + j] * id) << 4));
}

/* d = max / -127 (the extreme lands on kv[0] = -127), id = d ? 1 / d : 0 from the unrounded d, d stored as f16 */
TK_HD void tk_quantize_iq4_nl(const float* x, tk_block_iq4_nl* out) {
    const float d = tk_divf(tk_iq4_signed_max(x), -127.0f);
    const float id = d != 0.0f ? tk_divf(1.0f, d) : 0.0f;
    out->d = tk_f32_to_f16(d);
    tk_iq4_pack(x, id, out->qs);
}

/* per sub-block the real scale r_j = max_j / -127; d = max |r_j| / 31 stored as f16, s_j = clamp(rint(r_j / dq), -32, 31) with dq the
 * stored d (0 when dq == 0), and the indices against dl = dq * s_j */
TK_HD void tk_quantize_iq4_xs(const float* x, tk_block_iq4_xs* out) {
    float r[8];
    float max_abs = 0.0f;
    TK_ROLLED
    for (int j = 0; j < 8; ++j) {
        r[j] = tk_divf(tk_iq4_signed_max(x + 32 * j), -127.0f);
        const float a = tk_fabsf(r[j]);
        max_abs = a > max_abs ? a : max_abs;
    }
    out->d = tk_f32_to_f16(tk_divf(max_abs, 31.0f));
    const float dq = tk_f16_to_f32(out->d);
    out->scales_h = 0;
    for (int k = 0; k < 4; ++k) out->scales_l[k] = 0;
    TK_ROLLED
    for (int j = 0; j < 8; ++j) {
        int s = dq != 0.0f ? (int)tk_rintf(tk_divf(r[j], dq)) : 0;
        s = s < -32 ? -32 : (s > 31 ? 31 : s);
        tk_iq4xs_set_scale(out, j, s);
        const float dl = dq * (float)s;
        const float idl = dl != 0.0f ? tk_divf(1.0f, dl) : 0.0f;
        tk_iq4_pack(x + 32 * j, idl, out->qs + 16 * j);
    }
}

/* TQ2_0 / TQ1_0: ggml's published quantize_row_tq2_0_ref / quantize_row_tq1_0_ref, value for value, all in binary32: amax = max |x| over
 * the 256 values, d = amax stored as f16, id = amax ? 1 / amax : 0 from the f32 amax, xi = lroundf(x * id) + 1 in 0..2 (halves away from
 * zero; |x * id| <= 1 up to rounding and is clamped to that, so the truncation below is exact and xi stays in 0..2).  The loops stay rolled in device code, as IQ4's do */
TK_HD float tk_tq_amax(const float* x) {
    float amax = 0.0f;
    TK_ROLLED
    for (int i = 0; i < 256; ++i) {
        const float a = tk_fabsf(x[i]);
        amax = a > amax ? a : amax;
    }
    return amax;
}
TK_HD int tk_tq_xi(float x, float id) {
    float v = x * id;
    /* an amax below 2^-128 makes id infinite and v +-inf or NaN (0 * inf), where lroundf is unspecified and the truncation below undefined:
     * such a v is taken as -1 (NaN) or +-1, so host and device make the same bytes.  d is then +0 and every weight decodes to 0 anyway */
    if (!(v >= -1.0f)) v = -1.0f;
    if (!(v <= 1.0f)) v = 1.0f;
    const float t = (float)(int)v, r = v - t;
    return (int)t + (r >= 0.5f ? 1 : r <= -0.5f ? -1 : 0) + 1;
}
TK_HD void tk_quantize_tq2_0(const float* x, tk_block_tq2_0* out) {
    const float amax = tk_tq_amax(x);
    const float id = amax != 0.0f ? tk_divf(1.0f, amax) : 0.0f;
    out->d = tk_f32_to_f16(amax);
    TK_ROLLED
    for (int j = 0; j < 64; ++j) { /* byte 32 h + m holds weights 128 h + 32 l + m, l = 0..3 */
        const float* p = x + 128 * (j >> 5) + (j & 31);
        int q = 0;
        TK_ROLLED
        for (int l = 0; l < 4; ++l) q |= tk_tq_xi(p[32 * l], id) << (2 * l);
        out->qs[j] = (uint8_t)q;
    }
}
/* one base-3 byte: NT trits taken at x[0], x[stride], ..., the first the most significant, padded to five digits, then
 * (q * 256 + 242) / 243: the smallest byte whose decode gives the digits back */
TK_HD uint8_t tk_tq1_0_byte(const float* x, int stride, int nt, float id) {
    int q = 0;
    TK_ROLLED
    for (int n = 0; n < nt; ++n) q = q * 3 + tk_tq_xi(x[stride * n], id);
    if (nt == 4) q *= 3;
    return (uint8_t)((q * 256 + 242) / 243);
}
TK_HD void tk_quantize_tq1_0(const float* x, tk_block_tq1_0* out) {
    const float amax = tk_tq_amax(x);
    const float id = amax != 0.0f ? tk_divf(1.0f, amax) : 0.0f;
    out->d = tk_f32_to_f16(amax);
    TK_ROLLED
    for (int m = 0; m < 32; ++m) out->qs[m] = tk_tq1_0_byte(x + m, 32, 5, id);
    TK_ROLLED
    for (int m = 0; m < 16; ++m) out->qs[32 + m] = tk_tq1_0_byte(x + 160 + m, 16, 5, id);
    TK_ROLLED
    for (int j = 0; j < 4; ++j) out->qh[j] = tk_tq1_0_byte(x + 240 + j, 4, 4, id);
}

/* The GGUF side of a type, described once: TkBlock<T> for every row of tk_type_desc_of.  What k_synth_blocks, k_embed, k_lora_merge, the
 * repack (tk_repack_lane) and the host quantiser entries do per type is a member of this trait, reached from a run-time type through
 * tk_type_dispatch, the one per-type list:
 *   block, per_run, elems   the block struct, its count in a 256-k run and its weights.  The float types are "blocks" of one element
 *   dequant(b, i)           weight i (0 .. elems - 1) of block b
 *   quantize(x, out)        elems floats -> one block
 *   code(run, k)            the tiled types: the integer the W4A8 tile stores for weight k (0 .. 255) of a run (tk_llm_layout.h).  Q6_K's is
 *                           q ^ 32 (the 6-bit two's complement of q - 32), Q3_K's q + 4, Q8_0's the raw byte, TQ1_0's the decoded trit; an
 *                           IQ4_NL block has the Q4_0 block's bytes, and so its codes */
#if defined(__HIPCC__)
#define TK_HD_MEMBER static TK_HD
#else
#define TK_HD_MEMBER TK_HD /* static inline already */
#endif
template <int T> struct TkBlock;
#define TK_BLOCK(T, BLOCK, PER_RUN, DEQUANT, QUANTIZE, CODE)                                   \
    template <> struct TkBlock<T> {                                                            \
        typedef BLOCK block;                                                                   \
        static constexpr int type = T, per_run = PER_RUN, elems = TK_QK_K / (PER_RUN);         \
        TK_HD_MEMBER float dequant(const block* b, int i) { return DEQUANT; }                  \
        TK_HD_MEMBER void quantize(const float* x, block* out) { QUANTIZE; }                   \
        TK_HD_MEMBER int code(const block* run, int k) { return CODE; }                        \
    }
TK_BLOCK(TK_TYPE_F32, float, 256, b[i], *out = *x, 0);
TK_BLOCK(TK_TYPE_F16, uint16_t, 256, tk_f16_to_f32(b[i]), *out = tk_f32_to_f16(*x), 0);
TK_BLOCK(TK_TYPE_BF16, uint16_t, 256, tk_bf16_to_f32(b[i]), *out = tk_f32_to_bf16(*x), 0);
TK_BLOCK(TK_TYPE_Q4_0, tk_block_q4_0, 8, tk_q4_0_dequant(b, i), tk_quantize_q4_0(x, out), tk_q4_0_quant(run + (k >> 5), k & 31));
TK_BLOCK(TK_TYPE_Q4_1, tk_block_q4_1, 8, tk_q4_1_dequant(b, i), tk_quantize_q4_1(x, out), tk_q4_1_quant(run + (k >> 5), k & 31));
TK_BLOCK(TK_TYPE_Q5_0, tk_block_q5_0, 8, tk_q5_0_dequant(b, i), tk_quantize_q5_0(x, out), tk_q5_0_quant(run + (k >> 5), k & 31));
TK_BLOCK(TK_TYPE_Q5_1, tk_block_q5_1, 8, tk_q5_1_dequant(b, i), tk_quantize_q5_1(x, out), tk_q5_1_quant(run + (k >> 5), k & 31));
TK_BLOCK(TK_TYPE_Q8_0, tk_block_q8_0, 8, tk_q8_0_dequant(b, i), tk_quantize_q8_0(x, out), (uint8_t)run[k >> 5].qs[k & 31]);
TK_BLOCK(TK_TYPE_Q2_K, tk_block_q2_K, 1, tk_q2k_dequant(b, i), tk_quantize_q2_K(x, out), tk_q2k_quant(run, k));
TK_BLOCK(TK_TYPE_Q3_K, tk_block_q3_K, 1, tk_q3k_dequant(b, i), tk_quantize_q3_K(x, out), tk_q3k_quant(run, k) + 4);
TK_BLOCK(TK_TYPE_Q4_K, tk_block_q4_K, 1, tk_q4k_dequant(b, i), tk_quantize_q4_K(x, out), tk_q4k_quant(run, k));
TK_BLOCK(TK_TYPE_Q5_K, tk_block_q5_K, 1, tk_q5k_dequant(b, i), tk_quantize_q5_K(x, out), tk_q5k_quant(run, k));
TK_BLOCK(TK_TYPE_Q6_K, tk_block_q6_K, 1, tk_q6k_dequant(b, i), tk_quantize_q6_K(x, out), tk_q6k_quant(run, k) ^ 32);
TK_BLOCK(TK_TYPE_IQ4_NL, tk_block_iq4_nl, 8, tk_iq4nl_dequant(b, i), tk_quantize_iq4_nl(x, out), tk_iq4_quant(run[k >> 5].qs, k & 31));
TK_BLOCK(TK_TYPE_IQ4_XS, tk_block_iq4_xs, 1, tk_iq4xs_dequant(b, i), tk_quantize_iq4_xs(x, out), tk_iq4_quant(run->qs + 16 * (k >> 5), k & 31));
TK_BLOCK(TK_TYPE_TQ1_0, tk_block_tq1_0, 1, tk_tq1_0_dequant(b, i), tk_quantize_tq1_0(x, out), tk_tq1_0_quant(run, k));
TK_BLOCK(TK_TYPE_TQ2_0, tk_block_tq2_0, 1, tk_tq2_0_dequant(b, i), tk_quantize_tq2_0(x, out), tk_tq2_0_quant(run, k));
#undef TK_BLOCK

/* run-time type -> trait: f(TkBlock<type>{}) for a type of this build (true), nothing for any other value (false) */
template <typename F> TK_HD constexpr bool tk_type_dispatch(int type, F&& f) {
    switch (type) {
#define TK_CASE(T) case T: f(TkBlock<T>{}); return true
        TK_CASE(TK_TYPE_F32); TK_CASE(TK_TYPE_F16); TK_CASE(TK_TYPE_BF16);
        TK_CASE(TK_TYPE_Q4_0); TK_CASE(TK_TYPE_Q4_1); TK_CASE(TK_TYPE_Q5_0); TK_CASE(TK_TYPE_Q5_1); TK_CASE(TK_TYPE_Q8_0);
        TK_CASE(TK_TYPE_Q2_K); TK_CASE(TK_TYPE_Q3_K); TK_CASE(TK_TYPE_Q4_K); TK_CASE(TK_TYPE_Q5_K); TK_CASE(TK_TYPE_Q6_K);
        TK_CASE(TK_TYPE_IQ4_NL); TK_CASE(TK_TYPE_IQ4_XS); TK_CASE(TK_TYPE_TQ1_0); TK_CASE(TK_TYPE_TQ2_0);
#undef TK_CASE
        default: return false;
    }
}
/* a case for every row of tk_type_desc_of and for nothing else, and each trait agrees with its row: the block's size and its weights */
TK_HD constexpr bool tk_type_dispatch_complete() {
    for (int t = 0; t < 64; ++t) {
        bool agrees = false;
        const bool has = tk_type_dispatch(t, [&](auto b) {
            typedef decltype(b) B;
            agrees = B::type == t && (int)sizeof(typename B::block) == tk_type_desc_of(t).block_bytes && B::elems == tk_type_desc_of(t).block_elems &&
                     B::elems * B::per_run == TK_QK_K; /* a 256-k run is whole blocks */
        });
        if (has != tk_type_known(t) || (has && !agrees)) return false;
    }
    return true;
}
static_assert(tk_type_dispatch_complete(), "tk_type_dispatch: one case per row of tk_type_desc_of, whose block_bytes and block_elems are the trait's");

/* tile_bytes = 16 rows x the tile's bytes for one row's 256-k run (tk_llm_layout.h); the block sizes are held to the trait above */
#define TK_TYPE_ROW_CHECK(T, tile_per_run) \
    static_assert(tk_type_desc_of(T).tile_bytes == TK_TILE_ROWS * (tile_per_run), #T ": tile_bytes is not 16 x the tile's bytes per row and run (tk_llm_layout.h)")
TK_TYPE_ROW_CHECK(TK_TYPE_Q8_0, 8 * 34); /* a tile column is one 256-k run: eight blocks per row */
TK_TYPE_ROW_CHECK(TK_TYPE_Q4_0, 8 * 18);
TK_TYPE_ROW_CHECK(TK_TYPE_Q5_0, 8 * 22);
TK_TYPE_ROW_CHECK(TK_TYPE_Q4_1, 8 * 20);
TK_TYPE_ROW_CHECK(TK_TYPE_Q5_1, 8 * 24);
TK_TYPE_ROW_CHECK(TK_TYPE_Q2_K, 84);
TK_TYPE_ROW_CHECK(TK_TYPE_Q3_K, 114); /* the tile holds the sixteen group scales as int8: 4 B more than the block's packed 6-bit ones */
TK_TYPE_ROW_CHECK(TK_TYPE_Q4_K, 144);
TK_TYPE_ROW_CHECK(TK_TYPE_Q5_K, 176);
TK_TYPE_ROW_CHECK(TK_TYPE_Q6_K, 210);
TK_TYPE_ROW_CHECK(TK_TYPE_IQ4_NL, 8 * 18);
TK_TYPE_ROW_CHECK(TK_TYPE_IQ4_XS, 144); /* the tile holds the eight sub-block scales as int8 in a 16-byte row tail: 8 B more than the block */
static_assert(sizeof(tk_block_iq4_nl) == sizeof(tk_block_q4_0) && TK_IQ4_NL_TILE_BYTES == TK_Q4_0_TILE_BYTES, "IQ4_NL rides on the Q4_0 repack, fragment and load");
TK_TYPE_ROW_CHECK(TK_TYPE_TQ2_0, 66);
TK_TYPE_ROW_CHECK(TK_TYPE_TQ1_0, 66); /* the tile is TQ2_0's: 2-bit codes, 12 B more than the block's base-3 bytes */
static_assert(offsetof(tk_block_tq2_0, d) == 64 && offsetof(tk_block_tq1_0, qh) == 48 && offsetof(tk_block_tq1_0, d) == 52, "TQ1_0 / TQ2_0: d is the block's last field");
#undef TK_TYPE_ROW_CHECK

/* ---- seeded synthetic tensors (splitmix64, seed stated per item) ---- */

TK_HD uint64_t tk_splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

/* counter-based: element `index` of stream (seed, tensor_id). Irwin-Hall(4) ~ N(0,1) */
TK_HD float tk_synth_normal(uint64_t seed, uint64_t tensor_id, uint64_t index) {
    uint64_t h = tk_splitmix64(tk_splitmix64(seed ^ (tensor_id * 0xD6E8FEB86659FD93ull)) + index);
    int32_t s = (int32_t)(h & 0xffff) + (int32_t)((h >> 16) & 0xffff) +
                (int32_t)((h >> 32) & 0xffff) + (int32_t)((h >> 48) & 0xffff);
    /* sum of 4 U[0,65535]: mean 131070, std 65536/sqrt(3) */
    return (float)(s - 131070) * 2.64289216e-5f; /* sqrt(3)/65536 */
}

TK_HD uint32_t tk_synth_u32(uint64_t seed, uint64_t tensor_id, uint64_t index) {
    uint64_t h = tk_splitmix64(tk_splitmix64(seed ^ (tensor_id * 0xD6E8FEB86659FD93ull)) + index);
    return (uint32_t)(h >> 32);
}

#endif /* TK_GGML_BLOCKS_H */
