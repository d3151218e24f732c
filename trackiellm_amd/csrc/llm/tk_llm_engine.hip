/*
 * tk_llm_engine.hip — host side of the LLM stream: weight residency, KV cache, pass
 * scheduling and hipGraph capture.  See tk_llm_engine.h for the reference call sites replaced.
 */
#include "tk_llm_engine.h"

#include <chrono>
#include "tk_lora.h"

#include <math.h>
#include <algorithm>
#include <mutex>
#include <new>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../common/tk_ggml_blocks.h"
#include "tk/tk_mi355x_ext.h"
#include "../nn/tk_gemm_tiled.h"
#include "../nn/tk_nn_kernels.h"

#define HIPQ(expr)                                                                              \
    do {                                                                                        \
        hipError_t e__ = (expr);                                                                \
        if (e__ != hipSuccess) {                                                                \
            char b__[256];                                                                      \
            snprintf(b__, sizeof b__, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            error = b__;                                                                        \
            return false;                                                                       \
        }                                                                                       \
    } while (0)

/* ------------------------------------------------------------------ model ------------------ */

static int use_more_bits(int i, int n) { return i < n / 8 || i >= 7 * n / 8 || (i - n / 8) % 3 == 2; }

/* ftype 15 Q4_K_M / 17 Q5_K_M: the base type, Q6_K for v / down of use_more_bits layers; 16 Q5_K_S: all Q5_K; 14 Q4_K_S: Q4_K, Q5_K for v of
 * layers < 4 and down of layers < n_layer / 8; 11 Q3_K_S: all Q3_K; 12 Q3_K_M: Q3_K, v Q5_K for layers < 2 else Q4_K, o Q4_K, down Q5_K
 * for layers < n_layer / 16 else Q4_K; 10 Q2_K: Q2_K, v Q4_K when n_head / n_kv_head >= 4 else Q3_K, o and down Q3_K; 21 Q2_K_S: Q2_K,
 * v Q4_K when n_head / n_kv_head >= 4, down Q4_K for layers < n_layer / 8.  output is Q6_K in all eight.  7 Q8_0: every matrix, token_embd
 * and output Q8_0.  2 Q4_0 / 8 Q5_0 / 25 IQ4_NL / 30 IQ4_XS: every layer matrix and token_embd in the base type, output Q6_K.
 * 36 TQ1_0 / 37 TQ2_0 (llama.cpp's recipe for the ternary types): every layer matrix in the base type, token_embd Q4_K, output Q6_K.
 * ftype < 0 (fill_synthetic_type): the same recipe with the tensor type -ftype as the base type */
int TkLlmModel::recipe_type(const TkLlmHParams& hp, int layer, int which, int ftype) {
    if (ftype == 7) return (layer < 0 ? which == TK_T_OUT_NORM : which == TK_L_ATTN_NORM || which == TK_L_FFN_NORM) ? TK_TYPE_F32 : TK_TYPE_Q8_0;
    if (ftype == 36 || ftype == 37) {
        if (layer < 0) return which == TK_T_OUTPUT ? TK_TYPE_Q6_K : (which == TK_T_TOKEN_EMBD ? TK_TYPE_Q4_K : TK_TYPE_F32);
        return which == TK_L_ATTN_NORM || which == TK_L_FFN_NORM ? TK_TYPE_F32 : ftype == 36 ? TK_TYPE_TQ1_0 : TK_TYPE_TQ2_0;
    }
    if (ftype < 0 || ftype == 2 || ftype == 8 || ftype == 25 || ftype == 30) {
        const int base = ftype < 0 ? -ftype : ftype == 2 ? TK_TYPE_Q4_0 : ftype == 8 ? TK_TYPE_Q5_0 : ftype == 25 ? TK_TYPE_IQ4_NL : TK_TYPE_IQ4_XS;
        if (layer < 0) return which == TK_T_OUTPUT ? TK_TYPE_Q6_K : (which == TK_T_TOKEN_EMBD ? base : TK_TYPE_F32);
        return which == TK_L_ATTN_NORM || which == TK_L_FFN_NORM ? TK_TYPE_F32 : base;
    }
    const int base = ftype == 10 || ftype == 21 ? TK_TYPE_Q2_K : ftype == 11 || ftype == 12 ? TK_TYPE_Q3_K : ftype == 16 || ftype == 17 ? TK_TYPE_Q5_K : TK_TYPE_Q4_K;
    if (layer < 0) return which == TK_T_OUTPUT ? TK_TYPE_Q6_K : (which == TK_T_TOKEN_EMBD ? base : TK_TYPE_F32);
    if (which == TK_L_ATTN_NORM || which == TK_L_FFN_NORM) return TK_TYPE_F32;
    if (ftype == 11) return base;
    if (ftype == 10 || ftype == 21) {
        const bool gqa4 = hp.n_kv_head > 0 && hp.n_head / hp.n_kv_head >= 4;
        if (which == TK_L_V) return gqa4 ? TK_TYPE_Q4_K : ftype == 10 ? TK_TYPE_Q3_K : base;
        if (ftype == 10) return which == TK_L_O || which == TK_L_DOWN ? TK_TYPE_Q3_K : base;
        return which == TK_L_DOWN && layer < hp.n_layer / 8 ? TK_TYPE_Q4_K : base;
    }
    if (ftype == 12) {
        if (which == TK_L_V) return layer < 2 ? TK_TYPE_Q5_K : TK_TYPE_Q4_K;
        if (which == TK_L_O) return TK_TYPE_Q4_K;
        if (which == TK_L_DOWN) return layer < hp.n_layer / 16 ? TK_TYPE_Q5_K : TK_TYPE_Q4_K;
        return base;
    }
    if (ftype == 14) return (which == TK_L_V && layer < 4) || (which == TK_L_DOWN && layer < hp.n_layer / 8) ? TK_TYPE_Q5_K : TK_TYPE_Q4_K;
    if (ftype != 16 && (which == TK_L_V || which == TK_L_DOWN) && use_more_bits(layer, hp.n_layer)) return TK_TYPE_Q6_K;
    return base;
}

void TkLlmModel::shape(int layer, int which, int64_t* rows, int64_t* cols) const {
    const int64_t d = hp.d_model, kv = (int64_t)hp.n_kv_head * hp.head_dim, qd = (int64_t)hp.n_head * hp.head_dim;
    if (layer < 0) {
        if (which == TK_T_OUT_NORM) { *rows = 1; *cols = d; }
        else { *rows = hp.vocab; *cols = d; }
        return;
    }
    switch (which) {
        case TK_L_ATTN_NORM: case TK_L_FFN_NORM: *rows = 1; *cols = d; break;
        case TK_L_Q: *rows = qd; *cols = d; break;
        case TK_L_K: case TK_L_V: *rows = kv; *cols = d; break;
        case TK_L_O: *rows = d; *cols = qd; break;
        case TK_L_GATE: case TK_L_UP: *rows = hp.d_ff; *cols = d; break;
        default: *rows = d; *cols = hp.d_ff; break;
    }
}

TkDevTensor* TkLlmModel::slot(int layer, int which) {
    if (layer < 0) return which == TK_T_TOKEN_EMBD ? &token_embd : which == TK_T_OUT_NORM ? &out_norm : which == TK_T_OUTPUT ? &output : nullptr;
    if (layer >= (int)layers.size() || which < 0 || which >= TK_L_COUNT) return nullptr;
    TkLlmLayer& L = layers[layer];
    TkDevTensor* t[TK_L_COUNT] = {&L.attn_norm, &L.q, &L.k, &L.v, &L.o, &L.ffn_norm, &L.gate, &L.up, &L.down};
    return t[which];
}

/* the head geometry the step and attention kernels take; nullptr or why not (TkLlmModel::init, tk_llm_step_probe) */
static const char* head_geometry_error(int n_head, int n_kv_head, int head_dim) {
    const int grp = n_kv_head > 0 ? n_head / n_kv_head : 0;
    if (n_head <= 0 || head_dim <= 0 || ((int64_t)n_head * head_dim) % 256) return "d_model, d_ff and n_head*head_dim must be multiples of 256";
    if (n_kv_head <= 0 || n_head % n_kv_head || (grp != 1 && grp != 2 && grp != 4)) return "n_head / n_kv_head must be 1, 2 or 4";
    if ((grp * head_dim) % 256 || head_dim % 64) return "head_dim must be a multiple of 64 and (n_head/n_kv_head)*head_dim a multiple of 256";
    /* k_attention's value phase gives a lane the dims (2 lane, 2 lane + 1) of two blocks of 128: 256 dims of a head and no more */
    if (head_dim > 256) return "head_dim must be at most 256: the attention kernels form 256 output dims per head";
    return nullptr;
}

bool TkLlmModel::init(const TkLlmHParams& h, int dev) {
    hp = h;
    device = dev;
    const int64_t qd = (int64_t)h.n_head * h.head_dim, kvd = (int64_t)h.n_kv_head * h.head_dim;
    auto bad = [&](const char* why) { error = std::string("unsupported model geometry: ") + why; return false; };
    if (h.n_layer <= 0 || h.d_model <= 0 || h.d_ff <= 0 || h.d_model % 256 || h.d_ff % 256) return bad("d_model, d_ff and n_head*head_dim must be multiples of 256");
    if (const char* why = head_geometry_error(h.n_head, h.n_kv_head, h.head_dim)) return bad(why);
    /* the norm keeps a whole row of the residual stream in LDS: (d_model + 4) floats of the 160 KiB a kernel can be opted into */
    if (h.d_model > tk_llm_max_d_model()) return bad("d_model above 40704: the RMS norm keeps one row of d_model floats in 160 KiB of LDS");
    if (qd % 64 || kvd % 64 || h.d_ff % 64 || h.vocab % 64 || h.d_model % 64) return bad("row counts must be multiples of 64");
    if (h.ks_out != 1) return bad("ks_out must be 1");
    const int ksv[4] = {h.ks_qkv, h.ks_o, h.ks_gateup, h.ks_down};
    const int64_t kk[4] = {h.d_model, qd, h.d_model, h.d_ff};
    for (int i = 0; i < 4; ++i)
        if (ksv[i] <= 0 || ksv[i] > 8 || (kk[i] / 256) % ksv[i]) return bad("K-split must be in [1, 8] and divide K/256");
    HIPQ(hipSetDevice(device));
    layers.assign(h.n_layer, TkLlmLayer());
    return true;
}

TkLlmModel::~TkLlmModel() {
    (void)hipSetDevice(device);
    auto fr = [](TkDevTensor& t) { if (t.data) (void)hipFree(t.data); t.data = nullptr; };
    fr(token_embd); fr(out_norm); fr(output);
    for (auto& L : layers) { fr(L.attn_norm); fr(L.ffn_norm); fr(L.q); fr(L.k); fr(L.v); fr(L.o); fr(L.gate); fr(L.up); fr(L.down); }
}

/* dev_blocks: tensor in GGUF layout already in device memory */
bool TkLlmModel::install(TkDevTensor* t, int type, int64_t rows, int64_t cols, void* dev_blocks, hipStream_t s, int layer, int which) {
    const bool is_matrix = rows > 1 && t != &token_embd;
    if (is_matrix && tk_type_is_float(type)) { /* one float type per model: the sessions' operand image carries one rounding */
        const int have = float_type(nullptr, t); /* the tensor being replaced does not count */
        if (have >= 0 && have != type) {
            error = std::string("a model's matrices hold at most one float type: this one is ") + tk_type_desc_of(type).name + ", another is " + tk_type_desc_of(have).name;
            return false;
        }
    }
    if (t->data) { (void)hipFree(t->data); t->data = nullptr; }
    t->type = type; t->rows = rows; t->cols = cols;
    if (const TkLoraTensor* lt = (lora && is_matrix) ? lora->find(layer, which) : nullptr) {
        /* the reference's llama_model_apply_lora_from_file (tk_model_loader.c:259-270): W += (alpha / r) B A on the blocks as the file holds them */
        if (lt->n_out != rows || lt->k_in != cols) { error = "LoRA adapter does not fit this model (factor shapes against the base matrix)"; return false; }
        float *dA = nullptr, *dB = nullptr;
        HIPQ(hipMalloc((void**)&dA, lt->A.size() * 4));
        if (hipMalloc((void**)&dB, lt->B.size() * 4) != hipSuccess) { (void)hipFree(dA); error = "out of device memory (LoRA factors)"; return false; }
        bool ok = hipMemcpyAsync(dA, lt->A.data(), lt->A.size() * 4, hipMemcpyHostToDevice, s) == hipSuccess &&
                  hipMemcpyAsync(dB, lt->B.data(), lt->B.size() * 4, hipMemcpyHostToDevice, s) == hipSuccess;
        const bool taken = ok && tk_launch_lora_merge(type, dev_blocks, rows, cols, dA, dB, lt->r, lora->scale_of(*lt), s);
        const bool done = hipStreamSynchronize(s) == hipSuccess; /* the factors' host copies and dA / dB live until here */
        (void)hipFree(dA);
        (void)hipFree(dB);
        if (ok && !taken) {
            const tk_type_desc d = tk_type_desc_of(type);
            error = "LoRA merge needs a " TK_LORA_MERGE_NAMES_OR " matrix";
            if (d.tile_bytes != 0 && !d.lora_merge) error += std::string(": merging into a ") + d.name + " matrix is not built";
            else error += " with columns % 256 == 0";
            return false;
        }
        if (!ok || !done) { error = "LoRA merge failed on the device"; return false; }
        lora_merged++;
    }
    if (tk_type_is_float(type)) {
        /* float checkpoints: matrices become the tiled GEMM's weight tiles (csrc/nn/tk_gemm_tiled.h: 2 bytes a value for F16 / BF16, 4 for F32), the
         * embedding and the norm rows stay row-major */
        const int wb = type == TK_TYPE_F32 ? 4 : 2;
        /* a matrix is tiled 16 rows x 32 k.  A row-major tensor has no such need; an F16 token_embd has all the same been held to columns % 32
         * since F16 loads, and that refusal stays as it is (BF16 / F32 embeddings and the norm rows are not held to it) */
        if ((is_matrix && (rows % 16 || cols % 32)) || (type == TK_TYPE_F16 && cols % 32)) {
            error = std::string(type == TK_TYPE_F16 ? "f16" : tk_type_desc_of(type).name) + " matrices need rows % 16 == 0 and columns % 32 == 0";
            return false;
        }
        t->bytes = (size_t)rows * cols * wb;
        HIPQ(hipMalloc((void**)&t->data, t->bytes));
        if (is_matrix) {
            tk_launch_tile_weights(dev_blocks, wb, rows, cols, t->data, s);
            HIPQ(hipGetLastError());
        } else {
            HIPQ(hipMemcpyAsync(t->data, dev_blocks, t->bytes, hipMemcpyDeviceToDevice, s));
        }
        return true;
    }
    const tk_type_desc d = tk_type_desc_of(type);
    if (d.tile_bytes == 0) {
        error = "unsupported tensor type (want " TK_TYPE_NAMES_OR ")";
        return false;
    }
    /* a matrix is held as tiles (a Q3_K tile is larger than its sixteen blocks: tk_llm_layout.h), anything else as the file's blocks */
    if (cols % 256) { error = std::string("a ") + d.name + " tensor needs columns % 256 == 0 (the W4A8 tile and the Q8_K activation run are 256 k wide)"; return false; }
    t->bytes = is_matrix ? (size_t)(rows / TK_TILE_ROWS) * (cols / 256) * d.tile_bytes : (size_t)rows * cols / d.block_elems * d.block_bytes;
    HIPQ(hipMalloc((void**)&t->data, t->bytes));
    if (!is_matrix) { /* token_embd stays in GGUF layout: one row is gathered per token */
        if (!d.token_embd) { error = "token_embd must be " TK_TOKEN_EMBD_NAMES_OR; return false; }
        HIPQ(hipMemcpyAsync(t->data, dev_blocks, t->bytes, hipMemcpyDeviceToDevice, s));
        return true;
    }
    tk_launch_repack(type, dev_blocks, rows, cols, t->data, s);
    HIPQ(hipGetLastError());
    return true;
}

bool TkLlmModel::set_tensor(int layer, int which, int type, const void* host_blocks, size_t nbytes) {
    HIPQ(hipSetDevice(device));
    TkDevTensor* t = slot(layer, which);
    if (!t) { error = "no such tensor"; return false; }
    int64_t rows, cols;
    shape(layer, which, &rows, &cols);
    size_t expect = (size_t)rows * cols / tk_type_block_elems(type) * tk_type_block_bytes(type);
    if (expect != nbytes) { error = "tensor byte size does not match the model geometry"; return false; }
    void* tmp = nullptr;
    HIPQ(hipMalloc(&tmp, nbytes));
    HIPQ(hipMemcpy(tmp, host_blocks, nbytes, hipMemcpyHostToDevice));
    bool ok = install(t, type, rows, cols, tmp, nullptr, layer, which);
    (void)hipDeviceSynchronize();
    (void)hipFree(tmp);
    return ok;
}

int TkLlmModel::float_type(int* other, const TkDevTensor* except) const {
    int found = -1;
    if (other) *other = -1;
    auto see = [&](const TkDevTensor& t) {
        if (&t == except || !t.data || !tk_type_is_float(t.type)) return;
        if (found < 0) found = t.type;
        else if (t.type != found && other) *other = t.type;
    };
    see(output);
    for (const auto& L : layers) { see(L.q); see(L.k); see(L.v); see(L.o); see(L.gate); see(L.up); see(L.down); }
    return found;
}

bool TkLlmModel::fill_synthetic(uint64_t seed, bool f16, int ftype) { return fill_synthetic_as(seed, f16 ? (int)TK_TYPE_F16 : -1, ftype); }

bool TkLlmModel::fill_synthetic_float(uint64_t seed, int type) {
    if (type != TK_TYPE_BF16 && type != TK_TYPE_F32) { error = "fill_synthetic_float: type must be BF16 or F32"; return false; }
    return fill_synthetic_as(seed, type, 15);
}

bool TkLlmModel::fill_synthetic_as(uint64_t seed, int float_type, int ftype) {
    HIPQ(hipSetDevice(device));
    auto type_of = [&](int l, int w) {
        const int t = recipe_type(hp, l, w, ftype);
        return (float_type >= 0 && t != TK_TYPE_F32) ? float_type : t; /* float checkpoint: every matrix and the embedding in the float type, norms f32 */
    };
    /* a fill replaces every tensor: what an earlier fill or set_tensor left goes first, so that a handle may be refilled in another float type
     * (install() would refuse the first matrix of the new type beside the old ones) */
    for (int l = -1; l < hp.n_layer; ++l)
        for (int w = 0; w < (l < 0 ? 3 : (int)TK_L_COUNT); ++w) {
            TkDevTensor* t = slot(l, w);
            if (t->data) { (void)hipFree(t->data); t->data = nullptr; }
        }
    /* scratch big enough for the largest tensor in GGUF layout */
    size_t maxb = 0;
    for (int l = -1; l < hp.n_layer; ++l)
        for (int w = 0; w < (l < 0 ? 3 : (int)TK_L_COUNT); ++w) {
            int64_t r, c;
            shape(l, w, &r, &c);
            int type = type_of(l, w);
            size_t b = (size_t)r * c / tk_type_block_elems(type) * tk_type_block_bytes(type);
            maxb = b > maxb ? b : maxb;
        }
    void* tmp = nullptr;
    HIPQ(hipMalloc(&tmp, maxb));
    bool ok = true;
    for (int l = -1; l < hp.n_layer && ok; ++l)
        for (int w = 0; w < (l < 0 ? 3 : (int)TK_L_COUNT) && ok; ++w) {
            int64_t r, c;
            shape(l, w, &r, &c);
            int type = type_of(l, w);
            uint64_t tid = l < 0 ? (uint64_t)w : (uint64_t)(16 + l * 16 + w);
            if (r == 1) tk_launch_synth_f32(seed, tid, r * c, (float*)tmp, nullptr); /* the norm rows, F32 in every recipe */
            else if (type == TK_TYPE_BF16 || type == TK_TYPE_F32) tk_launch_synth_float(type, seed, tid, r * c, 0.02f, tmp, nullptr);
            else if (type == TK_TYPE_F16) tk_launch_synth_f16(seed, tid, r * c, 0.02f, (uint16_t*)tmp, nullptr);
            else tk_launch_synth_blocks(type, seed, tid, r * c / 256, 0.02f, tmp, nullptr);
            ok = install(slot(l, w), type, r, c, tmp, nullptr, l, w);
            if (ok && hipStreamSynchronize(nullptr) != hipSuccess) { error = "synthetic weight generation failed"; ok = false; }
        }
    (void)hipFree(tmp);
    return ok;
}

bool TkLlmModel::fill_synthetic_type(uint64_t seed, int type) {
    if (!tk_type_is_kquant(type)) { error = "fill_synthetic_type: not a tiled tensor type"; return false; }
    return fill_synthetic(seed, false, -type);
}

bool TkLlmModel::ready() const {
    if (!token_embd.data || !out_norm.data || !output.data) return false;
    for (const auto& L : layers) {
        if (!L.attn_norm.data || !L.ffn_norm.data || !L.q.data || !L.k.data || !L.v.data || !L.o.data || !L.gate.data || !L.up.data || !L.down.data)
            return false;
        /* the tensors of one fused launch (q|k|v, gate|up) are all tiled quantised types or all float */
        const bool f_qkv = tk_type_is_float(L.q.type), f_gu = tk_type_is_float(L.gate.type);
        if (tk_type_is_float(L.k.type) != f_qkv || tk_type_is_float(L.v.type) != f_qkv || tk_type_is_float(L.up.type) != f_gu) return false;
    }
    int other = -1;
    (void)float_type(&other);
    return other < 0; /* at most one float type among the matrices */
}

/* ------------------------------------------------------------------ session ---------------- */

/* float_type: the model's float kind (TkLlmModel::float_type), -1 = none: no operand image */
static bool alloc_act(TkActQ8* a, int K, int float_type, std::string& error) {
    a->aq_ts = TK_AQ_BYTES(K); a->ad_ts = TK_AD_FLOATS(K); a->abs_ts = TK_ABS_BYTES(K);
    a->af = nullptr; a->af_ts = (uint32_t)((size_t)K * TK_ROW_SLOTS);
    a->af_round = float_type >= 0 ? tk_type_float_round(float_type) : (int)TK_ROUND_NONE;
    if (float_type >= 0 && hipMalloc((void**)&a->af, (size_t)TK_MAX_ROWS * K * 4) != hipSuccess) { error = "out of device memory (float activation buffers)"; return false; }
    if (a->af) (void)hipMemset(a->af, 0, (size_t)TK_MAX_ROWS * K * 4);
    if (hipMalloc((void**)&a->aq, TK_MAX_TILES * a->aq_ts) != hipSuccess || hipMalloc((void**)&a->ad, TK_MAX_TILES * a->ad_ts * 4) != hipSuccess ||
        hipMalloc((void**)&a->abs, TK_MAX_TILES * a->abs_ts) != hipSuccess || hipMalloc((void**)&a->abs16, TK_MAX_TILES * a->abs_ts * 2) != hipSuccess) {
        error = "out of device memory (activation buffers)";
        return false;
    }
    (void)hipMemset(a->aq, 0, TK_MAX_TILES * a->aq_ts);
    (void)hipMemset(a->ad, 0, TK_MAX_TILES * a->ad_ts * 4);
    (void)hipMemset(a->abs, 0, TK_MAX_TILES * a->abs_ts);
    (void)hipMemset(a->abs16, 0, TK_MAX_TILES * a->abs_ts * 2);
    return true;
}
static void free_act(TkActQ8* a) {
    if (a->aq) (void)hipFree(a->aq);
    if (a->ad) (void)hipFree(a->ad);
    if (a->abs) (void)hipFree(a->abs);
    if (a->abs16) (void)hipFree(a->abs16);
    if (a->af) (void)hipFree(a->af);
    *a = TkActQ8{};
}

bool TkLlmSession::refuse_q8(const char* what) {
    if (kv_type != TK_KV_Q8_0) return false;
    error = std::string(what) + ": not built for a Q8_0 KV cache";
    return true;
}

size_t TkLlmSession::kv_bytes() const {
    if (!model) return 0;
    const TkLlmHParams& h = model->hp;
    const size_t kv = (size_t)h.n_layer * max_seq * max_ctx * h.n_kv_head * h.head_dim;
    return kv_type == TK_KV_Q8_0 ? 2 * (kv + kv / TK_KV_Q8_BLOCK * 2) : 2 * kv * 2;
}

bool TkLlmSession::init(TkLlmModel* m, int mseq, int mctx) {
    model = m;
    max_seq = mseq;
    max_ctx = mctx;
    if (kv_type != TK_KV_F16 && kv_type != TK_KV_Q8_0) { error = "kv_type must be 0 (F16) or 1 (Q8_0), asked for " + std::to_string(kv_type); return false; }
    if (m && !m->ready()) {
        int other = -1;
        const int ft = m->float_type(&other);
        if (other >= 0) { error = std::string("a model's matrices hold at most one float type: this model has ") + tk_type_desc_of(ft).name + " and " + tk_type_desc_of(other).name; return false; }
    }
    if (!m || !m->ready()) { error = "model has missing tensors"; return false; }
    if (mseq <= 0 || mctx <= 0) { error = "max_seq and max_ctx must be positive"; return false; }
    const TkLlmHParams& h = m->hp;
    /* a window beyond tk_attention_resident_limit takes k_attention_far, whose LDS does not depend on it (tk_attention_plan) */
    if (mctx > TK_MAX_CONTEXT) {
        error = "max_ctx too large: a session's context window is at most " + std::to_string(TK_MAX_CONTEXT) + " positions (RoPE is unscaled), asked for " + std::to_string(mctx);
        return false;
    }
    HIPQ(hipSetDevice(m->device));
    HIPQ(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    tk_attention_note_session(m->device, +1);
    counted_ = true;
    const int QD = h.n_head * h.head_dim, KVD = h.n_kv_head * h.head_dim, half = h.head_dim / 2;
    size_t kv = (size_t)h.n_layer * mseq * mctx * KVD;
    /* the one allocation that grows with sequences x window: a failure names what was asked for (16 sequences of 32 768 positions of a 7B model
     * are 69 GB) */
    if (kv_type == TK_KV_Q8_0) {
        /* head_dim % 64 == 0 (TkLlmModel::init): rows are whole blocks, value rows whole 16-byte words, scale rows whole 4-byte words */
        const size_t sc = kv / TK_KV_Q8_BLOCK * 2;
        if (hipMalloc((void**)&kvq.kq, kv) != hipSuccess || hipMalloc((void**)&kvq.vq, kv) != hipSuccess || hipMalloc((void**)&kvq.kd, sc) != hipSuccess ||
            hipMalloc((void**)&kvq.vd, sc) != hipSuccess) {
            (void)hipGetLastError();
            error = "Q8_0 KV cache: could not allocate 2 x " + std::to_string(kv) + " bytes of int8 values and 2 x " + std::to_string(sc) + " bytes of f16 scales on the device (" +
                    std::to_string(h.n_layer) + " layers x " + std::to_string(mseq) + " sequences x " + std::to_string(mctx) + " positions x " + std::to_string(KVD) +
                    " elements, keys and values)";
            return false;
        }
        HIPQ(hipMemset(kvq.kq, 0, kv));
        HIPQ(hipMemset(kvq.vq, 0, kv));
        HIPQ(hipMemset(kvq.kd, 0, sc));
        HIPQ(hipMemset(kvq.vd, 0, sc));
    } else {
        if (hipMalloc((void**)&kcache, kv * 2) != hipSuccess || hipMalloc((void**)&vcache, kv * 2) != hipSuccess) {
            (void)hipGetLastError();
            error = "KV cache: could not allocate 2 x " + std::to_string(kv * 2) + " bytes on the device (" + std::to_string(h.n_layer) + " layers x " + std::to_string(mseq) +
                    " sequences x " + std::to_string(mctx) + " positions x " + std::to_string(KVD) + " f16, keys and values)";
            return false;
        }
        HIPQ(hipMemset(kcache, 0, kv * 2));
        HIPQ(hipMemset(vcache, 0, kv * 2));
    }
    HIPQ(hipMalloc((void**)&x, (size_t)TK_MAX_ROWS * h.d_model * 4));
    HIPQ(hipMalloc((void**)&qbuf, (size_t)TK_MAX_ROWS * QD * 4));
    size_t pmax = (size_t)h.ks_qkv * (QD + 2 * KVD);
    pmax = std::max(pmax, (size_t)h.ks_o * h.d_model);
    pmax = std::max(pmax, (size_t)h.ks_gateup * 2 * h.d_ff);
    pmax = std::max(pmax, (size_t)h.ks_down * h.d_model);
    HIPQ(hipMalloc((void**)&partial, pmax * TK_MAX_ROWS * 4));
    /* twins for passes whose mat-vec launches run their producer themselves (enqueue_range): such a launch reads one (x, slab) pair while
     * its workgroups write the other */
    HIPQ(hipMalloc((void**)&x2, (size_t)TK_MAX_ROWS * h.d_model * 4));
    HIPQ(hipMalloc((void**)&partial2, pmax * TK_MAX_ROWS * 4));
    HIPQ(hipMalloc((void**)&logits, (size_t)TK_MAX_ROWS * h.vocab * 4));
    const int ft = m->float_type();
    if (!alloc_act(&act_d, h.d_model, ft, error) || !alloc_act(&act_qd, QD, ft, error) || !alloc_act(&act_ff, h.d_ff, ft, error)) return false;
    HIPQ(hipMalloc((void**)&d_seq, TK_MAX_ROWS * 4));
    HIPQ(hipMalloc((void**)&d_pos, TK_MAX_ROWS * 4));
    HIPQ(hipMalloc((void**)&d_tok, TK_MAX_ROWS * 4));
    HIPQ(hipMalloc((void**)&d_nsteps, TK_MAX_ROWS * 4));
    HIPQ(hipMemset(d_nsteps, 0, TK_MAX_ROWS * 4));
    hist_cap = mctx;
    HIPQ(hipMalloc((void**)&d_hist, (size_t)hist_cap * TK_MAX_ROWS * 4));
    HIPQ(hipMalloc((void**)&d_tiles, (size_t)(1 + TK_MAX_ROWS) * 4));
    HIPQ(hipMemset(d_tiles, 0, (size_t)(1 + TK_MAX_ROWS) * 4));
    if (kv_type == TK_KV_F16 && mctx > TK_LONG_ATT_MIN_POS && tk_attention_long_applies(1, h.n_head, h.n_kv_head, h.head_dim))
        HIPQ(hipMalloc((void**)&d_scores, tk_attention_long_scratch_floats(h.n_head, h.head_dim, mctx) * sizeof(float)));
    HIPQ(hipMalloc((void**)&d_mask, (size_t)TK_MAX_ROWS * (((size_t)h.vocab + 31) / 32) * 4));
    HIPQ(hipMalloc((void**)&d_mask_row, TK_MAX_ROWS * 4));
    HIPQ(hipMemset(d_mask_row, 0xFF, TK_MAX_ROWS * 4));
    mask_rows_dirty = false;
    HIPQ(hipMalloc((void**)&d_samp, TK_MAX_ROWS * sizeof(TkSampleRow)));
    HIPQ(hipMemset(d_samp, 0, TK_MAX_ROWS * sizeof(TkSampleRow))); /* temp 0: every row samples greedily */
    samp_dirty = false;
    HIPQ(hipMalloc((void**)&d_kvcopy, TK_MAX_ROWS * sizeof(TkKvCopyDesc)));
    HIPQ(hipMemset(d_kvcopy, 0, TK_MAX_ROWS * sizeof(TkKvCopyDesc)));
    HIPQ(hipHostMalloc((void**)&h_kvcopy, TK_MAX_ROWS * sizeof(TkKvCopyDesc), hipHostMallocDefault));
    HIPQ(hipMalloc((void**)&d_adj, TK_MAX_ROWS * sizeof(TkAdjustRow)));
    HIPQ(hipMemset(d_adj, 0, TK_MAX_ROWS * sizeof(TkAdjustRow))); /* no window, no bias: every row is neutral */
    HIPQ(hipMalloc((void**)&d_adj_ids, (size_t)TK_MAX_ROWS * TK_ADJUST_MAX_RECENT * 4));
    HIPQ(hipMalloc((void**)&d_adj_bias_ids, (size_t)TK_MAX_ROWS * TK_ADJUST_MAX_BIAS * 4));
    HIPQ(hipMalloc((void**)&d_adj_bias, (size_t)TK_MAX_ROWS * TK_ADJUST_MAX_BIAS * 4));
    HIPQ(hipHostMalloc((void**)&h_adj, TK_MAX_ROWS * (sizeof(TkAdjustRow) + (size_t)TK_ADJUST_MAX_RECENT * 4 + (size_t)TK_ADJUST_MAX_BIAS * 8), hipHostMallocDefault));
    adj_dirty = false;
    HIPQ(hipMalloc((void**)&d_lp_ntop, TK_MAX_ROWS * 4));
    HIPQ(hipMemset(d_lp_ntop, 0xFF, TK_MAX_ROWS * 4)); /* -1: no row asks */
    HIPQ(hipMalloc((void**)&d_lp_rec, TK_MAX_ROWS * sizeof(TkTokenLogprob)));
    HIPQ(hipMemset(d_lp_rec, 0, TK_MAX_ROWS * sizeof(TkTokenLogprob)));
    HIPQ(hipHostMalloc((void**)&h_lp_rec, TK_MAX_ROWS * sizeof(TkTokenLogprob), hipHostMallocDefault));
    lp_dirty = false;
    /* RoPE table, double precision on the host (same formula as the oracle) */
    std::vector<float> cs((size_t)mctx * half), sn((size_t)mctx * half);
    for (int p = 0; p < mctx; ++p)
        for (int i = 0; i < half; ++i) {
            double theta = pow((double)h.rope_theta, -2.0 * i / (double)h.head_dim);
            double a = (double)p * theta;
            cs[(size_t)p * half + i] = (float)cos(a);
            sn[(size_t)p * half + i] = (float)sin(a);
        }
    HIPQ(hipMalloc((void**)&rope_cos, cs.size() * 4));
    HIPQ(hipMalloc((void**)&rope_sin, sn.size() * 4));
    HIPQ(hipMemcpy(rope_cos, cs.data(), cs.size() * 4, hipMemcpyHostToDevice));
    HIPQ(hipMemcpy(rope_sin, sn.data(), sn.size() * 4, hipMemcpyHostToDevice));
    /* kernels that want more than the default 64 KiB of dynamic LDS: a per-device opt-in */
    if (const char* e = tk_llm_prepare_device(m->device)) { error = std::string("LDS opt-in failed: ") + e; return false; }
    if (ft >= 0 && !tk_gemm_tiled_prepare_device()) { error = "LDS opt-in of the tiled GEMM failed"; return false; }
    /* the prefix cache's copy kernel runs between passes, outside any capture: launched once here, with nothing to copy, so that its code object
     * is loaded before the first pass is recorded into a graph */
    if (kv_copy_applies() && !enqueue_kv_copy(nullptr, 0)) return false;
    /* so does the context shift's kernel: once with an empty move */
    if (kv_type == TK_KV_F16 && kv_copy_applies() &&
        !tk_launch_kv_shift_rows(TkKvShiftDesc{0, 0, 0, 0}, kcache, vcache, rope_cos, rope_sin, h.n_layer, h.n_kv_head, h.head_dim, max_seq, max_ctx, stream)) {
        error = "kv_shift: launch failed";
        return false;
    }
    /* and the Q8_0 cache's append and attention kernels: one row of sequence 0 at position 0, whose q | k | v slab is zero (the row quantises to the
     * zeros the cache already holds) */
    if (kv_type == TK_KV_Q8_0) {
        HIPQ(hipMemsetAsync(partial, 0, pmax * TK_MAX_ROWS * 4, stream));
        HIPQ(hipMemsetAsync(d_seq, 0, 4, stream));
        HIPQ(hipMemsetAsync(d_pos, 0, 4, stream));
        tk_launch_qkv_rope_append_q8(partial, 1, QD + 2 * KVD, h.n_head, h.n_kv_head, h.head_dim, rope_cos, rope_sin, d_seq, d_pos, 1, qbuf, kvq, 0, max_seq, max_ctx, stream);
        if (!tk_launch_attention_q8(qbuf, kvq, d_seq, d_pos, 1, h.n_head, h.n_kv_head, h.head_dim, 0, max_seq, max_ctx, act_qd, nullptr, stream)) {
            error = "Q8_0 KV cache: the attention kernel does not take this head geometry";
            return false;
        }
        HIPQ(hipGetLastError());
    }
    HIPQ(hipDeviceSynchronize());
    return true;
}

TkLlmSession::~TkLlmSession() {
    if (model && counted_) tk_attention_note_session(model->device, -1);
    if (model) (void)hipSetDevice(model->device);
    if (stream) (void)hipStreamSynchronize(stream);
    for (auto& v : graphs) for (auto& g : v) if (g) (void)hipGraphExecDestroy(g);
    void* ptrs[] = {kcache, vcache, kvq.kq, kvq.vq, kvq.kd, kvq.vd, x, x2, qbuf, partial, partial2, logits, rope_cos, rope_sin, d_seq, d_pos, d_tok, d_nsteps, d_hist, d_mask, d_mask_row, d_samp, d_tab, d_tiles, d_scores};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    if (d_kvcopy) (void)hipFree(d_kvcopy);
    if (h_kvcopy) (void)hipHostFree(h_kvcopy);
    void* adj[] = {d_adj, d_adj_ids, d_adj_bias_ids, d_adj_bias};
    for (void* p : adj) if (p) (void)hipFree(p);
    if (h_adj) (void)hipHostFree(h_adj);
    if (d_lp_ntop) (void)hipFree(d_lp_ntop);
    if (d_lp_rec) (void)hipFree(d_lp_rec);
    if (h_lp_rec) (void)hipHostFree(h_lp_rec);
    void* gm[] = {d_gm_arena, d_gm_offsets, d_gm_pieces, d_gm_states, d_mask_undecided};
    for (void* p : gm) if (p) (void)hipFree(p);
    for (uint32_t* p : gm_words) if (p) (void)hipFree(p);
    if (h_gm_states) (void)hipHostFree(h_gm_states);
    if (h_mask_undecided) (void)hipHostFree(h_mask_undecided);
    free_act(&act_d); free_act(&act_qd); free_act(&act_ff);
    if (stream) (void)hipStreamDestroy(stream);
}

/* ---- grammar masks on the device: the runners' side (the header comment has the contract) ---- */

bool TkLlmSession::install_vocab_image(const uint32_t* offsets, const uint8_t* pieces, int32_t eos) {
    std::lock_guard<std::mutex> lk(gm_mu);
    if (d_gm_offsets) return true;
    const size_t vocab = (size_t)model->hp.vocab, nbytes = offsets[vocab];
    if (hipSetDevice(model->device) != hipSuccess) return false;
    bool ok = hipMalloc((void**)&d_gm_pieces, nbytes ? nbytes : 1) == hipSuccess && hipMalloc((void**)&d_gm_arena, TK_GRAMMAR_ARENA_SLOTS * sizeof(TkGrammarImage)) == hipSuccess &&
              hipMalloc((void**)&d_gm_states, TK_MAX_ROWS * sizeof(TkGrammarStateImage)) == hipSuccess &&
              hipHostMalloc((void**)&h_gm_states, TK_MAX_ROWS * sizeof(TkGrammarStateImage), hipHostMallocDefault) == hipSuccess &&
              hipMalloc((void**)&d_mask_undecided, TK_MAX_ROWS * 4) == hipSuccess && hipHostMalloc((void**)&h_mask_undecided, TK_MAX_ROWS * 4, hipHostMallocDefault) == hipSuccess &&
              hipMemcpy(d_gm_pieces, pieces, nbytes, hipMemcpyHostToDevice) == hipSuccess;
    uint32_t* off = nullptr;
    ok = ok && hipMalloc((void**)&off, (vocab + 1) * 4) == hipSuccess && hipMemcpy(off, offsets, (vocab + 1) * 4, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) { if (off) (void)hipFree(off); (void)hipGetLastError(); return false; } /* what was allocated is freed with the session */
    gm_eos = eos;
    d_gm_offsets = off; /* last: forward() takes it as "installed" */
    return true;
}

int TkLlmSession::grammar_slot(const uint32_t* words, size_t n_words, int32_t n_rules, int32_t n_elems, int32_t n_sets, int32_t root) {
    std::lock_guard<std::mutex> lk(gm_mu);
    if (!d_gm_offsets || n_words == 0 || n_words != (size_t)n_rules + 1 + (size_t)n_elems + (size_t)n_sets * 8) return -1;
    int free_slot = -1;
    for (int i = 0; i < TK_GRAMMAR_ARENA_SLOTS; ++i) {
        if (gm_keys[i].empty()) { if (free_slot < 0) free_slot = i; continue; }
        if (gm_keys[i].size() == n_words && memcmp(gm_keys[i].data(), words, n_words * 4) == 0) return i;
    }
    if (free_slot < 0 || hipSetDevice(model->device) != hipSuccess) return -1;
    uint32_t* d = nullptr;
    TkGrammarImage img;
    if (hipMalloc((void**)&d, n_words * 4) != hipSuccess) { (void)hipGetLastError(); return -1; }
    img.rule_off = d; img.elems = d + n_rules + 1; img.sets = img.elems + n_elems;
    img.n_rules = n_rules; img.n_elems = n_elems; img.n_sets = n_sets; img.root = root;
    /* no pass reads this entry yet: a state that names it is attached after this returns */
    if (hipMemcpy(d, words, n_words * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_gm_arena + free_slot, &img, sizeof img, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        (void)hipGetLastError();
        return -1;
    }
    gm_words[free_slot] = d;
    gm_keys[free_slot].assign(words, words + n_words);
    return free_slot;
}

bool TkLlmSession::attach_grammar_state(const uint32_t* mask_ptr, const TkGrammarStateImage& image) {
    std::lock_guard<std::mutex> lk(gm_mu);
    if (!mask_ptr || !d_gm_offsets || image.grammar < 0 || image.grammar >= TK_GRAMMAR_ARENA_SLOTS || gm_keys[image.grammar].empty()) return false;
    GrammarRow& g = gm_rows[mask_ptr];
    g.image = image;
    g.ran = false;
    g.undecided = 0;
    return true;
}

void TkLlmSession::detach_grammar_state(const uint32_t* mask_ptr, bool* ran, int32_t* undecided) {
    std::lock_guard<std::mutex> lk(gm_mu);
    auto it = gm_rows.find(mask_ptr);
    *ran = it != gm_rows.end() && it->second.ran;
    *undecided = it != gm_rows.end() ? it->second.undecided : 0;
    if (it != gm_rows.end()) gm_rows.erase(it);
}

bool TkLlmSession::reset() {
    HIPQ(hipSetDevice(model->device));
    HIPQ(hipMemsetAsync(d_nsteps, 0, TK_MAX_ROWS * 4, stream));
    HIPQ(hipStreamSynchronize(stream));
    return true;
}

bool TkLlmSession::kv_write(int layer, int seq, int pos0, int n_pos, const uint16_t* k, const uint16_t* v) {
    const TkLlmHParams& h = model->hp;
    if (layer < 0 || layer >= h.n_layer || seq < 0 || seq >= max_seq || pos0 < 0 || n_pos <= 0 || pos0 + n_pos > max_ctx || !k || !v) { error = "kv_write: (layer, sequence, positions) outside the cache"; return false; }
    HIPQ(hipSetDevice(model->device));
    if (kv_type == TK_KV_Q8_0) { /* the rows quantised here by the one definition the append kernel runs, laid out [kv head][position] as the cache has them */
        const int nb = h.head_dim / TK_KV_Q8_BLOCK;
        const size_t rows = (size_t)h.n_kv_head * n_pos;
        std::vector<int8_t> q[2] = {std::vector<int8_t>(rows * h.head_dim), std::vector<int8_t>(rows * h.head_dim)};
        std::vector<uint16_t> d[2] = {std::vector<uint16_t>(rows * nb), std::vector<uint16_t>(rows * nb)};
        for (int kvh = 0; kvh < h.n_kv_head; ++kvh)
            for (int p = 0; p < n_pos; ++p) {
                const size_t src = ((size_t)p * h.n_kv_head + kvh) * h.head_dim, row = (size_t)kvh * n_pos + p;
                tk_kv_q8_row(k + src, h.head_dim, q[0].data() + row * h.head_dim, d[0].data() + row * nb);
                tk_kv_q8_row(v + src, h.head_dim, q[1].data() + row * h.head_dim, d[1].data() + row * nb);
            }
        for (int kvh = 0; kvh < h.n_kv_head; ++kvh) {
            const size_t dst = (((size_t)layer * max_seq + seq) * h.n_kv_head + kvh) * max_ctx + pos0, src = (size_t)kvh * n_pos;
            HIPQ(hipMemcpyAsync(kvq.kq + dst * h.head_dim, q[0].data() + src * h.head_dim, (size_t)n_pos * h.head_dim, hipMemcpyHostToDevice, stream));
            HIPQ(hipMemcpyAsync(kvq.vq + dst * h.head_dim, q[1].data() + src * h.head_dim, (size_t)n_pos * h.head_dim, hipMemcpyHostToDevice, stream));
            HIPQ(hipMemcpyAsync(kvq.kd + dst * nb, d[0].data() + src * nb, (size_t)n_pos * nb * 2, hipMemcpyHostToDevice, stream));
            HIPQ(hipMemcpyAsync(kvq.vd + dst * nb, d[1].data() + src * nb, (size_t)n_pos * nb * 2, hipMemcpyHostToDevice, stream));
        }
        HIPQ(hipStreamSynchronize(stream)); /* the staging vectors die with this scope */
        return true;
    }
    const size_t hd = (size_t)h.head_dim * 2; /* bytes of one cache row */
    for (int kvh = 0; kvh < h.n_kv_head; ++kvh) { /* host pitch = one position of all heads; device run of one head = consecutive positions */
        const size_t dst = ((((size_t)layer * max_seq + seq) * h.n_kv_head + kvh) * max_ctx + pos0) * h.head_dim;
        HIPQ(hipMemcpy2DAsync(kcache + dst, hd, k + (size_t)kvh * h.head_dim, hd * h.n_kv_head, hd, (size_t)n_pos, hipMemcpyHostToDevice, stream));
        HIPQ(hipMemcpy2DAsync(vcache + dst, hd, v + (size_t)kvh * h.head_dim, hd * h.n_kv_head, hd, (size_t)n_pos, hipMemcpyHostToDevice, stream));
    }
    HIPQ(hipStreamSynchronize(stream));
    return true;
}

bool TkLlmSession::kv_read(int layer, int seq, int pos0, int n_pos, uint16_t* k, uint16_t* v) {
    const TkLlmHParams& h = model->hp;
    if (kv_type == TK_KV_Q8_0) { error = "kv_read: the rows of a Q8_0 KV cache are not f16 numbers (kv_read_q8 returns them)"; return false; }
    if (layer < 0 || layer >= h.n_layer || seq < 0 || seq >= max_seq || pos0 < 0 || n_pos <= 0 || pos0 + n_pos > max_ctx || !k || !v) { error = "kv_read: (layer, sequence, positions) outside the cache"; return false; }
    HIPQ(hipSetDevice(model->device));
    const size_t hd = (size_t)h.head_dim * 2;
    for (int kvh = 0; kvh < h.n_kv_head; ++kvh) {
        const size_t src = ((((size_t)layer * max_seq + seq) * h.n_kv_head + kvh) * max_ctx + pos0) * h.head_dim;
        HIPQ(hipMemcpy2DAsync(k + (size_t)kvh * h.head_dim, hd * h.n_kv_head, kcache + src, hd, hd, (size_t)n_pos, hipMemcpyDeviceToHost, stream));
        HIPQ(hipMemcpy2DAsync(v + (size_t)kvh * h.head_dim, hd * h.n_kv_head, vcache + src, hd, hd, (size_t)n_pos, hipMemcpyDeviceToHost, stream));
    }
    HIPQ(hipStreamSynchronize(stream));
    return true;
}

bool TkLlmSession::kv_read_q8(int layer, int seq, int pos0, int n_pos, int8_t* kq, uint16_t* kd, int8_t* vq, uint16_t* vd) {
    const TkLlmHParams& h = model->hp;
    if (kv_type != TK_KV_Q8_0) { error = "kv_read_q8: the session's KV cache is f16 (kv_read returns its rows)"; return false; }
    if (layer < 0 || layer >= h.n_layer || seq < 0 || seq >= max_seq || pos0 < 0 || n_pos <= 0 || pos0 + n_pos > max_ctx || !kq || !kd || !vq || !vd) {
        error = "kv_read_q8: (layer, sequence, positions) outside the cache";
        return false;
    }
    HIPQ(hipSetDevice(model->device));
    const size_t hd = (size_t)h.head_dim, sb = (size_t)h.head_dim / TK_KV_Q8_BLOCK * 2; /* bytes of one row's values and scales */
    for (int kvh = 0; kvh < h.n_kv_head; ++kvh) {
        const size_t src = (((size_t)layer * max_seq + seq) * h.n_kv_head + kvh) * max_ctx + pos0;
        HIPQ(hipMemcpy2DAsync(kq + (size_t)kvh * hd, hd * h.n_kv_head, kvq.kq + src * hd, hd, hd, (size_t)n_pos, hipMemcpyDeviceToHost, stream));
        HIPQ(hipMemcpy2DAsync(vq + (size_t)kvh * hd, hd * h.n_kv_head, kvq.vq + src * hd, hd, hd, (size_t)n_pos, hipMemcpyDeviceToHost, stream));
        HIPQ(hipMemcpy2DAsync((uint8_t*)kd + (size_t)kvh * sb, sb * h.n_kv_head, (const uint8_t*)kvq.kd + src * sb, sb, sb, (size_t)n_pos, hipMemcpyDeviceToHost, stream));
        HIPQ(hipMemcpy2DAsync((uint8_t*)vd + (size_t)kvh * sb, sb * h.n_kv_head, (const uint8_t*)kvq.vd + src * sb, sb, sb, (size_t)n_pos, hipMemcpyDeviceToHost, stream));
    }
    HIPQ(hipStreamSynchronize(stream));
    return true;
}

bool TkLlmSession::enqueue_kv_copy(const TkKvCopyDesc* descs, int n) {
    const TkLlmHParams& h = model->hp;
    if (!kv_copy_applies()) { error = "kv_copy: head_dim must be a multiple of 8"; return false; }
    if (n < 0 || n > TK_MAX_ROWS || (n > 0 && !descs)) { error = "kv_copy: between 0 and TK_MAX_ROWS descriptors"; return false; }
    int max_n = 0;
    for (int i = 0; i < n; ++i) {
        const TkKvCopyDesc& d = descs[i];
        if (d.src_seq < 0 || d.src_seq >= max_seq || d.dst_seq < 0 || d.dst_seq >= max_seq || d.src_seq == d.dst_seq || d.p0 < 0 || d.n <= 0 || d.n > max_ctx - d.p0) {
            error = "kv_copy: (source, destination, positions) outside the cache, or source = destination";
            return false;
        }
        max_n = std::max(max_n, d.n);
    }
    HIPQ(hipSetDevice(model->device));
    if (n > 0) { /* h_kvcopy is free again: whoever enqueued the previous copy has waited for the stream since (forward() and kv_copy() end with a sync) */
        memcpy(h_kvcopy, descs, (size_t)n * sizeof(TkKvCopyDesc));
        HIPQ(hipMemcpyAsync(d_kvcopy, h_kvcopy, (size_t)n * sizeof(TkKvCopyDesc), hipMemcpyHostToDevice, stream));
    }
    const bool launched = kv_type == TK_KV_Q8_0 ? tk_launch_kv_copy_rows_q8(d_kvcopy, n, max_n, kvq, h.n_layer, h.n_kv_head, h.head_dim, max_seq, max_ctx, stream)
                                                : tk_launch_kv_copy_rows(d_kvcopy, n, max_n, kcache, vcache, h.n_layer, h.n_kv_head, h.head_dim, max_seq, max_ctx, stream);
    if (!launched) { error = "kv_copy: launch failed"; return false; }
    return true;
}

bool TkLlmSession::kv_copy(int src_seq, int dst_seq, int pos0, int n_pos) {
    const TkKvCopyDesc d{src_seq, dst_seq, pos0, n_pos};
    if (!enqueue_kv_copy(&d, 1)) return false;
    HIPQ(hipStreamSynchronize(stream));
    return true;
}

bool TkLlmSession::kv_shift(int seq, int p0, int p1, int delta, bool* bad_args) {
    const TkLlmHParams& h = model->hp;
    const TkKvShiftDesc m{seq, p0, p1, delta};
    if (bad_args) *bad_args = true;
    if (refuse_q8("kv_shift")) return false;
    if (!kv_copy_applies()) { error = "kv_shift: head_dim must be a multiple of 8"; return false; }
    if (!tk_kv_shift_ok(m, max_seq, max_ctx)) { error = "kv_shift: needs a sequence of the session, 0 <= p0 < p1 <= max_ctx, delta < 0 and p0 + delta >= 0"; return false; }
    if (bad_args) *bad_args = false;
    HIPQ(hipSetDevice(model->device));
    if (!tk_launch_kv_shift_rows(m, kcache, vcache, rope_cos, rope_sin, h.n_layer, h.n_kv_head, h.head_dim, max_seq, max_ctx, stream)) { error = "kv_shift: launch failed"; return false; }
    HIPQ(hipStreamSynchronize(stream));
    return true;
}

bool TkLlmSession::time_kv_shift(int seq, int p0, int p1, int delta, int iters, float* avg_ms, double* bytes) {
    const TkLlmHParams& h = model->hp;
    const TkKvShiftDesc m{seq, p0, p1, delta};
    if (refuse_q8("time_kv_shift")) return false;
    if (!kv_copy_applies() || !tk_kv_shift_ok(m, max_seq, max_ctx) || iters < 1) { error = "time_kv_shift: a move kv_shift refuses, or no iterations"; return false; }
    HIPQ(hipSetDevice(model->device));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIPQ(hipEventCreate(&e0));
    HIPQ(hipEventCreate(&e1));
    bool ok = true;
    for (int i = 0; i <= iters && ok; ++i) { /* launch 0 is the warm-up */
        if (i == 1) ok = hipEventRecord(e0, stream) == hipSuccess;
        ok = ok && tk_launch_kv_shift_rows(m, kcache, vcache, rope_cos, rope_sin, h.n_layer, h.n_kv_head, h.head_dim, max_seq, max_ctx, stream);
    }
    float ms = 0.0f;
    ok = ok && hipEventRecord(e1, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (!ok) { error = "time_kv_shift: device error"; return false; }
    *avg_ms = ms / (float)iters;
    *bytes = 2.0 * 2.0 * (double)h.n_layer * h.n_kv_head * (double)(p1 - p0) * h.head_dim * 2.0; /* read + written, K and V, f16 */
    return true;
}

static void set_act(TkGemvArgs& a, const TkActQ8& q) {
    a.aq = q.aq; a.ad = q.ad; a.abs = q.abs; a.abs16 = q.abs16; a.aq_ts = q.aq_ts; a.ad_ts = q.ad_ts; a.abs_ts = q.abs_ts;
}

static TkGemvSeg seg_of(const TkDevTensor& t) { return TkGemvSeg{t.data, t.type, (int)(t.rows / TK_TILE_ROWS)}; }

bool tk_llm_gemv_probe(int device, int type, const void* blocks, int64_t rows, int64_t K, int ks, int nrows, const float* x, float* y,
                       std::string& error) {
    if (!tk_type_is_kquant(type)) {
        error = "gemv probe: type must be " TK_KQUANT_NAMES_OR;
        return false;
    }
    if (rows < 64 || rows % 64 || rows > (1 << 20) || ks < 1 || ks > 8 || K < 256 || K % (256 * (int64_t)ks) || K > 65536 || nrows < 1 ||
        nrows > TK_MAX_ROWS) {
        error = "gemv probe: needs rows % 64 == 0, ks in [1, 8], K % (256 ks) == 0, nrows in [1, 256]";
        return false;
    }
    HIPQ(hipSetDevice(device));
    if (const char* e = tk_llm_prepare_device(device)) { error = e; return false; }
    const size_t nblk = (size_t)rows * (size_t)(K / 256); /* 256-k runs = tile columns; a run is 256 / block_elems blocks of the file */
    const size_t bb = 256 / tk_type_block_elems(type) * tk_type_block_bytes(type);
    const size_t tb = (size_t)tk_type_desc_of(type).tile_bytes;
    const size_t nout = (size_t)ks * TK_MAX_ROWS * (size_t)rows;
    void* db = nullptr;
    uint8_t* tiles = nullptr;
    float *dx = nullptr, *out = nullptr;
    TkActQ8 act{};
    std::vector<float> part;
    try { part.resize(nout); } catch (const std::bad_alloc&) { error = "gemv probe: out of host memory"; return false; } /* nothing may be thrown across the C ABI */
    bool ok = hipMalloc(&db, nblk * bb) == hipSuccess && hipMalloc((void**)&tiles, nblk / TK_TILE_ROWS * tb) == hipSuccess &&
              hipMalloc((void**)&dx, (size_t)nrows * K * 4) == hipSuccess && hipMalloc((void**)&out, nout * 4) == hipSuccess;
    if (!ok) error = "gemv probe: out of device memory";
    ok = ok && alloc_act(&act, (int)K, -1, error);
    if (ok) {
        hipStream_t s = nullptr;
        ok = hipMemcpy(db, blocks, nblk * bb, hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(dx, x, (size_t)nrows * K * 4, hipMemcpyHostToDevice) == hipSuccess && hipMemset(out, 0, nout * 4) == hipSuccess;
        if (ok) {
            tk_launch_repack(type, db, rows, K, tiles, s);
            tk_launch_quant_q8(dx, (int)K, nrows, act, s);
            TkGemvArgs a{};
            a.seg[0] = TkGemvSeg{tiles, type, (int)(rows / TK_TILE_ROWS)};
            a.nseg = 1; a.K = (int)K; a.ks = ks; a.n_total = (int)rows; a.nrows = nrows;
            set_act(a, act);
            a.out = out;
            tk_launch_gemv(a, s);
            ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
                 hipMemcpy(part.data(), out, nout * 4, hipMemcpyDeviceToHost) == hipSuccess;
        }
        if (!ok) error = "gemv probe: device error";
    }
    if (ok)
        for (int r = 0; r < nrows; ++r)
            for (int64_t n = 0; n < rows; ++n) { /* sum_partials' order */
                float o = part[(size_t)r * rows + n];
                for (int sl = 1; sl < ks; ++sl) o = o + part[((size_t)sl * TK_MAX_ROWS + r) * rows + n];
                y[(size_t)r * rows + n] = o;
            }
    free_act(&act);
    if (db) (void)hipFree(db);
    if (tiles) (void)hipFree(tiles);
    if (dx) (void)hipFree(dx);
    if (out) (void)hipFree(out);
    return ok;
}

/* ---- tk_mi355x_llm_step_probe: one step launcher on host arrays ---- */
namespace {
struct StepNeed { /* what an op reads and writes, in elements; 0 = unused */
    int64_t x = 0, partial = 0, w = 0, embd = 0, rows = 0, rope = 0, qbuf = 0, cache = 0, pv = 0, l = 0, tiles = 0, wblocks = 0, y = 0, xb = 0;
    int64_t image_k = 0; /* columns of the returned image(s); 0 = none */
    bool image = false, x_out = false, image_b = false;
};
}

static bool step_probe_check(const tk_mi355x_llm_step_probe_t& p, StepNeed& n, std::string& error) {
    auto bad = [&](const char* why) { error = std::string("step probe: ") + why; return false; };
    const int64_t M = TK_MAX_ROWS;
    if (p.nrows < 1 || p.nrows > TK_MAX_ROWS) return bad("nrows outside [1, 256]");
    const bool has_k = p.op != TK_MI355X_STEP_ROPE_APPEND && p.op != TK_MI355X_STEP_ATT_TILES;
    if (has_k && (p.K < 256 || p.K % 256 || p.K > 65536)) return bad("K must be a multiple of 256 in [256, 65536]");
    const bool has_slabs = p.op == TK_MI355X_STEP_RESIDUAL_FOLD || p.op == TK_MI355X_STEP_SWIGLU || p.op == TK_MI355X_STEP_ROPE_APPEND ||
                           (p.op == TK_MI355X_STEP_RMSNORM && p.partial);
    if (has_slabs && (p.ks < 1 || p.ks > 8)) return bad("ks outside [1, 8]");
    if (has_slabs && p.op != TK_MI355X_STEP_SWIGLU && (p.n_total < 4 || p.n_total % 4 || p.n_total > 65536)) return bad("n_total must be a multiple of 4 up to 65536");
    switch (p.op) {
    case TK_MI355X_STEP_EMBED: {
        if (!tk_type_desc_of(p.type).token_embd) return bad("type is no token_embd type");
        const int64_t be = tk_type_block_elems(p.type);
        if (p.K % be || p.vocab < 1 || p.vocab > (1 << 20)) return bad("K must hold whole blocks of the type and vocab lie in [1, 2^20]");
        n.embd = (int64_t)p.vocab * (p.K / be) * tk_type_block_bytes(p.type);
        n.rows = p.nrows; n.x = (int64_t)p.nrows * p.K; n.x_out = true;
        if (!p.tok || p.n_rows < n.rows) return bad("tok missing or too short");
        for (int r = 0; r < p.nrows; ++r)
            if (p.tok[r] < 0 || p.tok[r] >= p.vocab) return bad("a token outside the table");
        break;
    }
    case TK_MI355X_STEP_RMSNORM:
        if (tk_rmsnorm_lds_bytes(p.K) > tk_rmsnorm_lds_bytes(tk_llm_max_d_model())) return bad("K above 40704: the norm's row does not fit the 160 KiB of LDS the kernel is opted into");
        if (p.partial && p.n_total < p.K) return bad("n_total below K");
        n.x = M * p.K; n.x_out = true; n.w = p.K; n.image = true;
        n.partial = p.partial ? (int64_t)p.ks * M * p.n_total : 0;
        if (!(p.eps >= 0.0f) || !(p.eps < 1.0f)) return bad("eps outside [0, 1)");
        break;
    case TK_MI355X_STEP_RESIDUAL_FOLD:
        if (p.n_total < p.K) return bad("n_total below K");
        n.x = M * p.K; n.x_out = true; n.partial = (int64_t)p.ks * M * p.n_total;
        break;
    case TK_MI355X_STEP_SWIGLU:
        n.partial = (int64_t)p.ks * M * 2 * p.K; n.image = true;
        break;
    case TK_MI355X_STEP_QUANT:
        n.x = (int64_t)p.nrows * p.K; n.image = true;
        break;
    case TK_MI355X_STEP_ROPE_APPEND: {
        if (const char* why = head_geometry_error(p.n_head, p.n_kv_head, p.head_dim)) return bad(why);
        const int64_t qd = (int64_t)p.n_head * p.head_dim, kvd = (int64_t)p.n_kv_head * p.head_dim;
        if (qd + 2 * kvd > p.n_total) return bad("n_total below (n_head + 2 n_kv_head) head_dim");
        if (p.n_layer < 1 || p.max_seq < 1 || p.max_ctx < 1 || p.layer < 0 || p.layer >= p.n_layer) return bad("layer outside [0, n_layer), or an empty cache");
        n.cache = (int64_t)p.n_layer * p.max_seq * kvd * p.max_ctx;
        if (n.cache > (1LL << 28)) return bad("cache above 2^28 halves");
        n.partial = (int64_t)p.ks * M * p.n_total; n.rope = (int64_t)p.max_ctx * (p.head_dim / 2); n.qbuf = M * qd; n.rows = p.nrows;
        if (!p.seq || !p.pos || p.n_rows < n.rows) return bad("seq / pos missing or too short");
        for (int r = 0; r < p.nrows; ++r)
            if (p.seq[r] < 0 || p.seq[r] >= p.max_seq || p.pos[r] < 0 || p.pos[r] >= p.max_ctx) return bad("a (sequence, position) outside the cache");
        break;
    }
    case TK_MI355X_STEP_PV_JOIN:
        if ((p.head_dim != 64 && p.head_dim != 128) || p.n_head < 1 || p.n_head % (256 / p.head_dim) || (int64_t)p.n_head * p.head_dim != p.K)
            return bad("head_dim must be 64 or 128, n_head a multiple of 256 / head_dim, K = n_head head_dim");
        n.pv = (int64_t)p.nrows * p.n_head * 4 * p.head_dim; n.l = (int64_t)p.nrows * p.n_head * 4; n.image = true;
        break;
    case TK_MI355X_STEP_ATT_TILES:
        n.rows = p.nrows; n.tiles = 1 + M;
        if (!p.seq || p.n_rows < n.rows) return bad("seq missing or too short");
        break;
    case TK_MI355X_STEP_FUSED_NORM:
    case TK_MI355X_STEP_FUSED_SWIGLU: {
        const bool norm = p.op == TK_MI355X_STEP_FUSED_NORM;
        if (p.wtype != TK_TYPE_Q4_K && p.wtype != TK_TYPE_Q6_K) return bad("wtype must be Q4_K or Q6_K");
        if (p.wrows < 64 || p.wrows % 64 || p.wrows > 4096) return bad("wrows must be a multiple of 64 up to 4096");
        if (p.ks < 1 || p.ks > 8 || p.K % (256 * p.ks)) return bad("ks outside [1, 8] or K % (256 ks) != 0");
        const int fks = norm && !p.partial ? 0 : p.fks;
        if ((norm ? fks < 0 : fks < 1) || fks > 8) return bad("fks outside [1, 8]");
        if (!tk_gemv_fuses_producer(p.nrows, p.K, p.ks, fks)) return bad("no fused launch at this shape: nrows <= 2, K % (512 ks) == 0 and the image inside the LDS opt-in");
        if (norm) {
            if (fks && (p.n_total < p.K || p.n_total % 4 || p.n_total > 65536)) return bad("n_total must be a multiple of 4 in [K, 65536]");
            if (!(p.eps >= 0.0f) || !(p.eps < 1.0f)) return bad("eps outside [0, 1)");
            n.x = M * p.K; n.x_out = true; n.xb = M * p.K; n.w = p.K; n.partial = (int64_t)fks * M * p.n_total;
        } else n.partial = (int64_t)fks * M * 2 * p.K;
        n.wblocks = (int64_t)p.wrows * (p.K / 256) * (int64_t)tk_type_block_bytes(p.wtype);
        n.y = (int64_t)p.ks * M * p.wrows;
        break;
    }
    case TK_MI355X_STEP_WIDE_SWIGLU:
        if (p.wrows < 256 || p.wrows % 256 || p.wrows > 4096 || p.K > 4096) return bad("wrows must be a multiple of 256 up to 4096, K at most 4096");
        if (!tk_gemv_fuses_swiglu(p.nrows, 1, p.wtype, p.wtype) || (p.wtype != TK_TYPE_Q4_K && p.wtype != TK_TYPE_Q6_K)) return bad("no wide SwiGLU launch at this shape: nrows >= 193, wtype Q4_K or Q6_K");
        n.x = (int64_t)p.nrows * p.K; n.wblocks = 2 * (int64_t)p.wrows * (p.K / 256) * (int64_t)tk_type_block_bytes(p.wtype);
        n.image = n.image_b = true; n.image_k = p.wrows;
        break;
    default: return bad("unknown op");
    }
    if (n.image && !n.image_k) n.image_k = p.K;
    if (p.af_round < 0 || p.af_round > 2) return bad("af_round outside [0, 2]");
    if (n.image && p.af_round != 0 && !p.af) return bad("a float rounding needs the af image");
    auto need = [&](const void* a, int64_t have, int64_t want) { return want == 0 || (a && have >= want); };
    const int64_t K = n.image_k;
    if (!need(p.wblocks, p.n_wblocks, n.wblocks) || !need(p.y_a, p.n_y, n.y) || !need(p.y_b, p.n_y, n.y) || !need(p.x_b, p.n_xb, n.xb))
        return bad("a NULL array of the twins, or a count too small for the geometry");
    if (n.image_b && (!p.aq_b || !p.ad_b || !p.abs_b || !p.abs16_b || p.af)) return bad("the second image is NULL (or af given: the wide form has no float image)");
    if (!need(p.x, p.n_x, n.x) || !need(p.partial, p.n_partial, n.partial) || !need(p.w, p.n_w, n.w) || !need(p.embd, p.n_embd, n.embd) ||
        !need(p.rope_cos, p.n_rope, n.rope) || !need(p.rope_sin, p.n_rope, n.rope) || !need(p.qbuf, p.n_qbuf, n.qbuf) || !need(p.kcache, p.n_cache, n.cache) ||
        !need(p.vcache, p.n_cache, n.cache) || !need(p.pv_part, p.n_pv, n.pv) || !need(p.l_part, p.n_l, n.l) || !need(p.tiles, p.n_tiles, n.tiles))
        return bad("a NULL array, or a count too small for the geometry");
    if (n.image && (!need(p.aq, p.n_aq, M * K) || !need(p.ad, p.n_ad, K) || !need(p.abs, p.n_abs, TK_MAX_TILES * K) || !need(p.abs16, p.n_abs16, TK_MAX_TILES * K) ||
                    (p.af && p.n_af < M * K)))
        return bad("an image array is NULL or too small");
    return true;
}

bool tk_llm_step_probe(int device, tk_mi355x_llm_step_probe_s* pp, std::string& error) {
    tk_mi355x_llm_step_probe_t& p = *pp;
    StepNeed n;
    if (!step_probe_check(p, n, error)) return false;
    if (device < 0) return true;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) { error = "step probe: device ordinal out of range"; return false; }
    HIPQ(hipSetDevice(device));
    if (const char* e = tk_llm_prepare_device(device)) { error = e; return false; }
    std::vector<void*> owned;
    bool ok = true;
    auto up = [&](const void* src, int64_t elems, size_t esz) -> void* { /* a device copy of a host array; nullptr for an absent one */
        if (!ok || !src || elems <= 0) return nullptr;
        void* d = nullptr;
        if (hipMalloc(&d, (size_t)elems * esz) != hipSuccess) { ok = false; error = "step probe: out of device memory"; return nullptr; }
        owned.push_back(d);
        if (hipMemcpy(d, src, (size_t)elems * esz, hipMemcpyHostToDevice) != hipSuccess) { ok = false; error = "step probe: device error (upload)"; }
        return d;
    };
    const int64_t M = TK_MAX_ROWS, K = n.image_k ? n.image_k : p.K;
    float* dx = (float*)up(p.x, n.x, 4);
    const float* dpart = (const float*)up(p.partial, n.partial, 4);
    const float* dw = (const float*)up(p.w, n.w, 4);
    const void* dembd = up(p.embd, n.embd, 1);
    const int32_t* dtok = (const int32_t*)up(p.tok, p.op == TK_MI355X_STEP_EMBED ? n.rows : 0, 4);
    const int32_t* dseq = (const int32_t*)up(p.seq, p.op != TK_MI355X_STEP_EMBED ? n.rows : 0, 4);
    const int32_t* dpos = (const int32_t*)up(p.pos, p.op == TK_MI355X_STEP_ROPE_APPEND ? n.rows : 0, 4);
    const float* dcos = (const float*)up(p.rope_cos, n.rope, 4);
    const float* dsin = (const float*)up(p.rope_sin, n.rope, 4);
    float* dq = (float*)up(p.qbuf, n.qbuf, 4);
    uint16_t* dk = (uint16_t*)up(p.kcache, n.cache, 2);
    uint16_t* dv = (uint16_t*)up(p.vcache, n.cache, 2);
    const float* dpv = (const float*)up(p.pv_part, n.pv, 4);
    const float* dl = (const float*)up(p.l_part, n.l, 4);
    int32_t* dtiles = (int32_t*)up(p.tiles, n.tiles, 4);
    TkActQ8 act{};
    if (n.image) { /* alloc_act's strides over the caller's bytes: the image arrives as it was given, sentinels included */
        act.aq_ts = TK_AQ_BYTES(K); act.ad_ts = TK_AD_FLOATS(K); act.abs_ts = TK_ABS_BYTES(K);
        act.af_ts = (uint32_t)((size_t)K * TK_ROW_SLOTS); act.af_round = p.af_round;
        act.aq = (int8_t*)up(p.aq, M * K, 1);
        act.ad = (float*)up(p.ad, K, 4);
        act.abs = (int8_t*)up(p.abs, TK_MAX_TILES * K, 1);
        act.abs16 = (uint16_t*)up(p.abs16, TK_MAX_TILES * K, 2);
        act.af = (float*)up(p.af, M * K, 4);
    }
    const bool twin = p.op >= TK_MI355X_STEP_FUSED_NORM;
    auto make_act = [&](TkActQ8& a, int64_t k, const void* aq, const void* ad, const void* ab, const void* ab16) { /* an image over the caller's bytes, or (null) zeroed */
        a.aq_ts = TK_AQ_BYTES(k); a.ad_ts = TK_AD_FLOATS(k); a.abs_ts = TK_ABS_BYTES(k); a.af = nullptr; a.af_ts = (uint32_t)((size_t)k * TK_ROW_SLOTS); a.af_round = TK_ROUND_NONE;
        std::vector<uint8_t> zero;
        if (!aq) { try { zero.assign((size_t)M * k, 0); } catch (const std::bad_alloc&) { ok = false; error = "step probe: out of host memory"; return; } }
        a.aq = (int8_t*)up(aq ? aq : zero.data(), M * k, 1);
        a.ad = (float*)up(ad ? ad : zero.data(), k, 4);
        a.abs = (int8_t*)up(ab ? ab : zero.data(), TK_MAX_TILES * k, 1);
        a.abs16 = (uint16_t*)up(ab16 ? ab16 : zero.data(), TK_MAX_TILES * k, 2);
    };
    const void* dwb = up(p.wblocks, n.wblocks, 1);
    float *dya = (float*)up(p.y_a, n.y, 4), *dyb = (float*)up(p.y_b, n.y, 4), *dxb = (float*)up(p.x_b, n.xb, 4);
    TkActQ8 act_b{}, act_in{};
    if (n.image_b) make_act(act_b, K, p.aq_b, p.ad_b, p.abs_b, p.abs16_b);
    if (ok && twin) {
        hipStream_t s = nullptr;
        const int nseg = p.op == TK_MI355X_STEP_WIDE_SWIGLU ? 2 : 1;
        const size_t tb = (size_t)tk_type_desc_of(p.wtype).tile_bytes, nblk = (size_t)p.K / 256;
        void* dt = nullptr;
        if (hipMalloc(&dt, (size_t)nseg * p.wrows / TK_TILE_ROWS * nblk * tb) != hipSuccess) { ok = false; error = "step probe: out of device memory"; }
        else owned.push_back(dt);
        if (ok) {
            tk_launch_repack(p.wtype, dwb, (int64_t)nseg * p.wrows, p.K, (uint8_t*)dt, s);
            TkGemvArgs g{};
            g.seg[0] = TkGemvSeg{(const uint8_t*)dt, p.wtype, p.wrows / TK_TILE_ROWS};
            g.seg[1] = TkGemvSeg{(const uint8_t*)dt + (size_t)p.wrows / TK_TILE_ROWS * nblk * tb, p.wtype, p.wrows / TK_TILE_ROWS};
            g.nseg = nseg; g.K = p.K; g.nrows = p.nrows;
            if (p.op == TK_MI355X_STEP_WIDE_SWIGLU) {
                make_act(act_in, p.K, nullptr, nullptr, nullptr, nullptr);
                float* h = nullptr; /* form a's h [nrows][FF], then form b's gate | up slab [M][2 FF] */
                if (ok && hipMalloc((void**)&h, (size_t)M * 2 * p.wrows * 4) != hipSuccess) { ok = false; error = "step probe: out of device memory"; }
                if (ok) {
                    owned.push_back(h);
                    tk_launch_quant_q8(dx, p.K, p.nrows, act_in, s);
                    set_act(g, act_in);
                    g.ks = 1; g.out = h;
                    TkGemvArgs a = g;
                    a.swiglu = 1; a.n_total = p.wrows;
                    tk_launch_gemv(a, s);
                    tk_launch_quant_q8(h, p.wrows, p.nrows, act, s);
                    g.n_total = 2 * p.wrows; /* the launch order keeps h's two uses apart: one stream */
                    tk_launch_gemv(g, s);
                    tk_launch_swiglu_q8(h, 1, p.wrows, p.nrows, act_b, s);
                }
            } else {
                const bool norm = p.op == TK_MI355X_STEP_FUSED_NORM;
                const int fks = norm && !p.partial ? 0 : p.fks;
                make_act(act_in, p.K, nullptr, nullptr, nullptr, nullptr);
                if (ok) {
                    g.ks = p.ks; g.n_total = p.wrows;
                    TkGemvArgs b = g; /* form b first: it reads the caller's x, which form a's norm updates in place */
                    b.out = dyb; b.fuse = norm ? 1 : 2; b.fx_in = dx; b.fx_out = dxb; b.fslab = dpart; b.fks = fks; b.fn_total = norm ? p.n_total : 2 * p.K; b.fw = dw; b.feps = p.eps;
                    tk_launch_gemv(b, s);
                    if (norm) tk_launch_rmsnorm_q8(dx, dpart, fks, p.n_total, dw, p.eps, p.K, p.nrows, act_in, s);
                    else tk_launch_swiglu_q8(dpart, fks, p.K, p.nrows, act_in, s);
                    set_act(g, act_in);
                    g.out = dya;
                    tk_launch_gemv(g, s);
                }
            }
        }
        ok = ok && hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
        auto down = [&](void* dst, const void* src, int64_t elems, size_t esz) {
            if (ok && dst && src && elems > 0) ok = hipMemcpy(dst, src, (size_t)elems * esz, hipMemcpyDeviceToHost) == hipSuccess;
        };
        if (n.x_out) down(p.x, dx, n.x, 4);
        down(p.x_b, dxb, n.xb, 4);
        down(p.y_a, dya, n.y, 4);
        down(p.y_b, dyb, n.y, 4);
        if (n.image) {
            down(p.aq, act.aq, M * K, 1); down(p.ad, act.ad, K, 4); down(p.abs, act.abs, TK_MAX_TILES * K, 1); down(p.abs16, act.abs16, TK_MAX_TILES * K, 2);
            down(p.aq_b, act_b.aq, M * K, 1); down(p.ad_b, act_b.ad, K, 4); down(p.abs_b, act_b.abs, TK_MAX_TILES * K, 1); down(p.abs16_b, act_b.abs16, TK_MAX_TILES * K, 2);
        }
        if (!ok && error.empty()) error = "step probe: device error";
    } else if (ok) {
        hipStream_t s = nullptr;
        switch (p.op) {
        case TK_MI355X_STEP_EMBED: tk_launch_embed(dembd, p.type, p.K, dtok, p.nrows, dx, s); break;
        case TK_MI355X_STEP_RMSNORM: tk_launch_rmsnorm_q8(dx, dpart, p.ks, p.n_total, dw, p.eps, p.K, p.nrows, act, s); break;
        case TK_MI355X_STEP_RESIDUAL_FOLD: tk_launch_residual_fold(dx, dpart, p.ks, p.n_total, p.K, p.nrows, s); break;
        case TK_MI355X_STEP_SWIGLU: tk_launch_swiglu_q8(dpart, p.ks, p.K, p.nrows, act, s); break;
        case TK_MI355X_STEP_QUANT: tk_launch_quant_q8(dx, p.K, p.nrows, act, s); break;
        case TK_MI355X_STEP_ROPE_APPEND:
            tk_launch_qkv_rope_append(dpart, p.ks, p.n_total, p.n_head, p.n_kv_head, p.head_dim, dcos, dsin, dseq, dpos, p.nrows, dq, dk, dv, p.layer, p.max_seq, p.max_ctx, s);
            break;
        case TK_MI355X_STEP_PV_JOIN: tk_launch_att_pv_join(dpv, dl, p.nrows, p.n_head, p.head_dim, act, s); break;
        default: tk_launch_att_tiles(dseq, p.nrows, dtiles, s); break;
        }
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
        auto down = [&](void* dst, const void* src, int64_t elems, size_t esz) {
            if (ok && dst && src && elems > 0) ok = hipMemcpy(dst, src, (size_t)elems * esz, hipMemcpyDeviceToHost) == hipSuccess;
        };
        if (n.x_out) down(p.x, dx, n.x, 4);
        down(p.qbuf, dq, n.qbuf, 4);
        down(p.kcache, dk, n.cache, 2);
        down(p.vcache, dv, n.cache, 2);
        down(p.tiles, dtiles, n.tiles, 4);
        if (n.image) {
            down(p.aq, act.aq, M * K, 1);
            down(p.ad, act.ad, K, 4);
            down(p.abs, act.abs, TK_MAX_TILES * K, 1);
            down(p.abs16, act.abs16, TK_MAX_TILES * K, 2);
            down(p.af, act.af, M * K, 4);
        }
        if (!ok && error.empty()) error = "step probe: device error";
    }
    for (void* d : owned) (void)hipFree(d);
    return ok;
}

bool tk_llm_kv_q8_probe(int device, const tk_mi355x_kv_q8_probe_s* pp, std::string& error) {
    const tk_mi355x_kv_q8_probe_s& p = *pp;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) { error = "kv_q8 probe: no such HIP device"; return false; }
    HIPQ(hipSetDevice(device));
    if (const char* e = tk_llm_prepare_device(device)) { error = std::string("LDS opt-in failed: ") + e; return false; }
    const int hd = p.head_dim;
    const size_t elems = (size_t)p.n_layer * p.max_seq * p.n_kv_head * p.max_ctx * hd, scales = elems / TK_KV_Q8_BLOCK;
    const int n_head = p.mode == 0 ? p.n_kv_head : p.n_head; /* mode 0: one zero query head per KV head */
    const int QD = n_head * hd, KVD = p.n_kv_head * hd, n_total = QD + 2 * KVD;
    std::vector<void*> owned;
    bool ok = true;
    auto dev = [&](const void* host, size_t bytes) -> void* { /* a device array, a copy of `host` or zeros */
        void* d = nullptr;
        if (!ok || hipMalloc(&d, bytes ? bytes : 1) != hipSuccess) { ok = false; return nullptr; }
        owned.push_back(d);
        ok = (host ? hipMemcpy(d, host, bytes, hipMemcpyHostToDevice) : hipMemset(d, 0, bytes)) == hipSuccess;
        return d;
    };
    TkKvQ8 c{(int8_t*)dev(p.kq, elems), (uint16_t*)dev(p.kd, scales * 2), (int8_t*)dev(p.vq, elems), (uint16_t*)dev(p.vd, scales * 2)};
    int32_t* d_seq = (int32_t*)dev(p.seq, (size_t)p.nrows * 4);
    int32_t* d_pos = (int32_t*)dev(p.pos, (size_t)p.nrows * 4);
    TkActQ8 act{};
    if (p.mode == 0) {
        /* the production append launch on a slab that holds the rows: ks = 1, q columns zero, k | v columns the f16 values widened; RoPE by an identity
         * table (cos 1, sin 0) gives fma(-b, 0, a * 1) = a (a zero may change its sign, which the quantiser does not see), f16 rounding gives it back */
        std::vector<float> slab((size_t)p.nrows * n_total, 0.0f), cs((size_t)p.max_ctx * (hd / 2), 1.0f);
        for (int r = 0; r < p.nrows; ++r)
            for (int i = 0; i < KVD; ++i) {
                slab[(size_t)r * n_total + QD + i] = tk_f16_to_f32(p.k16[(size_t)r * KVD + i]);
                slab[(size_t)r * n_total + QD + KVD + i] = tk_f16_to_f32(p.v16[(size_t)r * KVD + i]);
            }
        float* d_slab = (float*)dev(slab.data(), slab.size() * 4);
        float* d_cos = (float*)dev(cs.data(), cs.size() * 4);
        float* d_sin = (float*)dev(nullptr, cs.size() * 4);
        float* d_q = (float*)dev(nullptr, (size_t)p.nrows * QD * 4);
        if (ok) {
            tk_launch_qkv_rope_append_q8(d_slab, 1, n_total, n_head, p.n_kv_head, hd, d_cos, d_sin, d_seq, d_pos, p.nrows, d_q, c, p.layer, p.max_seq, p.max_ctx, nullptr);
            ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy(p.kq, c.kq, elems, hipMemcpyDeviceToHost) == hipSuccess &&
                 hipMemcpy(p.vq, c.vq, elems, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(p.kd, c.kd, scales * 2, hipMemcpyDeviceToHost) == hipSuccess &&
                 hipMemcpy(p.vd, c.vd, scales * 2, hipMemcpyDeviceToHost) == hipSuccess;
        }
    } else {
        float* d_q = (float*)dev(p.q, (size_t)p.nrows * QD * 4);
        float* d_o = (float*)dev(p.out, (size_t)p.nrows * QD * 4);
        ok = ok && alloc_act(&act, QD, -1, error);
        if (ok) {
            ok = tk_launch_attention_q8(d_q, c, d_seq, d_pos, p.nrows, n_head, p.n_kv_head, hd, p.layer, p.max_seq, p.max_ctx, act, d_o, nullptr) &&
                 hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy(p.out, d_o, (size_t)p.nrows * QD * 4, hipMemcpyDeviceToHost) == hipSuccess;
        }
        free_act(&act);
    }
    for (void* d : owned) (void)hipFree(d);
    if (!ok) { (void)hipGetLastError(); if (error.empty()) error = "kv_q8 probe: device error"; }
    return ok;
}

bool tk_llm_repack_probe(int device, int type, const void* blocks, int64_t rows, int64_t K, void* tiles, std::string& error) {
    if (!tk_type_is_kquant(type)) {
        error = "repack probe: type must be " TK_KQUANT_NAMES_OR;
        return false;
    }
    if (rows < 16 || rows % 16 || rows > (1 << 20) || K < 256 || K % 256 || K > 65536 || rows * K > (1LL << 26)) {
        error = "repack probe: needs rows % 16 == 0, K % 256 == 0, K <= 65536 and rows x K <= 2^26";
        return false;
    }
    if (device < 0) {
        tk_repack_host(type, blocks, rows, K, (uint8_t*)tiles);
        return true;
    }
    const size_t nrun = (size_t)rows * (size_t)(K / 256);
    const size_t nb = nrun * (256 / tk_type_block_elems(type) * tk_type_block_bytes(type));
    const size_t nt = nrun / TK_TILE_ROWS * (size_t)tk_type_desc_of(type).tile_bytes;
    HIPQ(hipSetDevice(device));
    void* db = nullptr;
    uint8_t* dt = nullptr;
    bool ok = hipMalloc(&db, nb) == hipSuccess && hipMalloc((void**)&dt, nt) == hipSuccess;
    if (!ok) error = "repack probe: out of device memory";
    if (ok) {
        ok = hipMemcpy(db, blocks, nb, hipMemcpyHostToDevice) == hipSuccess;
        if (ok) {
            tk_launch_repack(type, db, rows, K, dt, nullptr);
            ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy(tiles, dt, nt, hipMemcpyDeviceToHost) == hipSuccess;
        }
        if (!ok) error = "repack probe: device error";
    }
    if (db) (void)hipFree(db);
    if (dt) (void)hipFree(dt);
    return ok;
}

bool tk_llm_matmul_float_probe(int device, int type, const void* w, int64_t rows, int64_t K, int ks, int nseg, const int32_t* seg_rows, int nrows,
                               const float* x, float* y, std::string& error) {
    if (type != TK_TYPE_F16 && type != TK_TYPE_BF16 && type != TK_TYPE_F32) { error = "float matmul probe: type must be F16, BF16 or F32"; return false; }
    int64_t sum = 0;
    bool segs_ok = nseg >= 1 && nseg <= 3;
    for (int i = 0; segs_ok && i < nseg; ++i) { segs_ok = seg_rows[i] >= 16 && seg_rows[i] % 16 == 0; sum += seg_rows[i]; }
    /* a test entry: rows x K up to 2^26 values (a 256 MiB F32 matrix; Mistral's largest is 14336 x 4096 = 2^25.8), so the host's slab copy
     * (ks x 256 x rows floats) stays below 512 MiB */
    if (!segs_ok || sum != rows || rows > 65536 || ks < 1 || ks > 8 || K < 256 || K % (256 * (int64_t)ks) || K > 65536 || rows * K > (1 << 26) || nrows < 1 ||
        nrows > TK_MAX_ROWS) {
        error = "float matmul probe: needs 1 .. 3 segments of rows % 16 == 0 that add up to rows <= 65536, ks in [1, 8], K % (256 ks) == 0, rows x K <= 2^26, nrows in [1, 256]";
        return false;
    }
    HIPQ(hipSetDevice(device));
    if (const char* e = tk_llm_prepare_device(device)) { error = e; return false; }
    if (!tk_gemm_tiled_prepare_device()) { error = "LDS opt-in of the tiled GEMM failed"; return false; }
    const int wb = type == TK_TYPE_F32 ? 4 : 2;
    const size_t wbytes = (size_t)rows * (size_t)K * wb, nout = (size_t)ks * TK_MAX_ROWS * (size_t)rows;
    uint8_t *dw = nullptr, *tiles = nullptr;
    float *dx = nullptr, *out = nullptr;
    TkActQ8 act{};
    std::vector<float> part;
    try { part.resize(nout); } catch (const std::bad_alloc&) { error = "float matmul probe: out of host memory"; return false; } /* nothing may be thrown across the C ABI */
    bool ok = hipMalloc((void**)&dw, wbytes) == hipSuccess && hipMalloc((void**)&tiles, wbytes) == hipSuccess &&
              hipMalloc((void**)&dx, (size_t)nrows * K * 4) == hipSuccess && hipMalloc((void**)&out, nout * 4) == hipSuccess;
    if (!ok) error = "float matmul probe: out of device memory";
    ok = ok && alloc_act(&act, (int)K, type, error);
    if (ok) {
        hipStream_t s = nullptr;
        ok = hipMemcpy(dw, w, wbytes, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dx, x, (size_t)nrows * K * 4, hipMemcpyHostToDevice) == hipSuccess &&
             hipMemset(out, 0, nout * 4) == hipSuccess;
        if (ok) {
            TkTiledGemm f{};
            size_t at = 0;
            for (int i = 0; i < nseg; ++i) { /* every segment a matrix of its own, tiled as install() tiles it */
                tk_launch_tile_weights(dw + at, wb, seg_rows[i], K, tiles + at, s);
                f.tiles[i] = tiles + at; f.row_tiles[i] = seg_rows[i] / TK_TILE_ROWS;
                at += (size_t)seg_rows[i] * (size_t)K * wb;
            }
            tk_launch_quant_q8(dx, (int)K, nrows, act, s);
            f.nseg = nseg; f.wbytes = wb; f.bf16 = type == TK_TYPE_BF16 ? 1 : 0; f.K = (int)K; f.ks = ks; f.ldc = (int)rows; f.n_valid = (int)rows; f.nrows = nrows;
            f.slab_rows = TK_MAX_ROWS; f.a_img = act.af; f.a_ts = act.af_ts; f.out = out;
            ok = tk_launch_gemm_tiled(f, s);
            if (!ok) error = "float matmul probe: the tiled GEMM refused the launch";
            else {
                ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
                     hipMemcpy(part.data(), out, nout * 4, hipMemcpyDeviceToHost) == hipSuccess;
                if (!ok) error = "float matmul probe: device error";
            }
        } else error = "float matmul probe: device error";
    }
    if (ok)
        for (int r = 0; r < nrows; ++r)
            for (int64_t n = 0; n < rows; ++n) { /* sum_partials' order */
                float o = part[(size_t)r * rows + n];
                for (int sl = 1; sl < ks; ++sl) o = o + part[((size_t)sl * TK_MAX_ROWS + r) * rows + n];
                y[(size_t)r * rows + n] = o;
            }
    free_act(&act);
    if (dw) (void)hipFree(dw);
    if (tiles) (void)hipFree(tiles);
    if (dx) (void)hipFree(dx);
    if (out) (void)hipFree(out);
    return ok;
}

void TkLlmSession::enqueue_pass(int nrows, const TkPassForm& f) { enqueue_range(nrows, 0, model->hp.n_layer, true, false, f); }

/* layers [l0, l1) of one pass.  embed: the residual stream starts from the token embeddings (first pipeline stage), otherwise x
 * already holds it.  fold_out: finish the last layer's residual update so x is the complete stream (it leaves this GPU).
 * f: the form of the pass (tk_pass_form.h); f.head: final norm + lm_head + arg max (last stage). */
/* one matmul group of a pass: the K-quant tensors of a launch go to the W4A8 kernels (K-split partial slabs, canonical plan `ks`); a float
 * group (F16 / BF16 / F32) goes through the exact fp32 GEMM on the activations rounded through that type (per slab one chain over its k).  Returns
 * the number of partial slabs the consumers must add. */
int TkLlmSession::enqueue_matmul(const TkDevTensor* const* t, int nseg, int K, int ks, int n_total, const TkActQ8& act, float* out, int nrows) {
    hipStream_t s = stream;
    if (tk_type_is_float(t[0]->type)) {
        TkTiledGemm f{};
        for (int i = 0; i < nseg; ++i) { f.tiles[i] = t[i]->data; f.row_tiles[i] = (int)(t[i]->rows / TK_TILE_ROWS); }
        f.nseg = nseg; f.wbytes = t[0]->type == TK_TYPE_F32 ? 4 : 2; f.bf16 = t[0]->type == TK_TYPE_BF16 ? 1 : 0; f.K = K; f.ks = ks; f.ldc = n_total; f.n_valid = n_total; f.nrows = nrows; f.slab_rows = TK_MAX_ROWS;
        f.a_img = act.af; f.a_ts = act.af_ts; f.out = out;
        /* shapes were validated when the model was installed (K a multiple of 256 ks); a refusal here would leave the slab unwritten, so it is
         * recorded and fails the pass (forward / decode / capture_pass check launch_error) instead of producing garbage silently */
        if (!tk_launch_gemm_tiled(f, s) && launch_error.empty()) launch_error = "tiled GEMM launch refused (shape outside what the float path supports)";
        return ks;
    }
    TkGemvArgs a{};
    for (int i = 0; i < nseg; ++i) a.seg[i] = seg_of(*t[i]);
    a.nseg = nseg; a.K = K; a.ks = ks; a.n_total = n_total; a.nrows = nrows;
    set_act(a, act); a.out = out;
    tk_launch_gemv(a, s);
    return ks;
}

static bool producer_fusion_enabled() {
    /* TK_MI355X_NO_FUSE=1: the norm / SwiGLU kernels stay launches of their own at every row count (A/B timing, bisecting) */
    const char* nf = getenv("TK_MI355X_NO_FUSE");
    return !(nf && nf[0] == '1');
}

/* rope/append and attention of one layer on the q|k|v slabs in `qkv_slab`, as the form says */
void TkLlmSession::enqueue_attention(const TkPassForm& f, const float* qkv_slab, int ks_qkv, int l, int nrows) {
    const TkLlmHParams& h = model->hp;
    const int n_qkv = (h.n_head + 2 * h.n_kv_head) * h.head_dim;
    hipStream_t s = stream;
    if (kv_type == TK_KV_Q8_0) { /* one form: rope apart, then kernel 6 (enqueue_range has refused every other description) */
        tk_launch_qkv_rope_append_q8(qkv_slab, ks_qkv, n_qkv, h.n_head, h.n_kv_head, h.head_dim, rope_cos, rope_sin, d_seq, d_pos, nrows, qbuf, kvq, l, max_seq, max_ctx, s);
        if (!tk_launch_attention_q8(qbuf, kvq, d_seq, d_pos, nrows, h.n_head, h.n_kv_head, h.head_dim, l, max_seq, max_ctx, act_qd, nullptr, s) && launch_error.empty())
            launch_error = "Q8_0 KV cache: the attention kernel does not take this pass";
        return;
    }
    if (!f.rope_in_attention)
        tk_launch_qkv_rope_append(qkv_slab, ks_qkv, n_qkv, h.n_head, h.n_kv_head, h.head_dim, rope_cos, rope_sin, d_seq, d_pos, nrows, qbuf, kcache, vcache, l, max_seq, max_ctx, s);
    if (f.attn == TK_ATT_LONG || f.attn == TK_ATT_RUN)
        tk_launch_attention_long(qkv_slab, ks_qkv, n_qkv, rope_cos, rope_sin, kcache, vcache, d_seq, d_pos, nrows, h.n_head, h.n_kv_head, h.head_dim, l, max_seq, max_ctx, d_scores, act_qd, s, f.attn == TK_ATT_RUN);
    else if (f.attn == TK_ATT_TILED)
        tk_launch_attention_prefill(qbuf, kcache, vcache, d_seq, d_pos, d_tiles, nrows, h.n_head, h.n_kv_head, h.head_dim, l, max_seq, max_ctx, act_qd, s);
    else
        tk_launch_attention(qbuf, qkv_slab, ks_qkv, n_qkv, rope_cos, rope_sin, kcache, vcache, d_seq, d_pos, nrows, h.n_head, h.n_kv_head, h.head_dim, l, max_seq, max_ctx, act_qd, f.rope_in_attention, s);
}

void TkLlmSession::enqueue_range(int nrows, int l0, int l1, bool embed, bool fold_out, const TkPassForm& f) {
    const TkLlmHParams& h = model->hp;
    const int D = h.d_model, QD = h.n_head * h.head_dim, KVD = h.n_kv_head * h.head_dim, FF = h.d_ff;
    hipStream_t s = stream;
    if (embed) tk_launch_embed(model->token_embd.data, model->token_embd.type, D, d_tok, nrows, x, s);
    /* One or two rows (the reference's own use: one runner, one token per step): a launch boundary (~1.5 us) plus a norm or SwiGLU kernel
     * that is one load latency long (5 - 6 us) costs more than that kernel's work repeated by every workgroup of the mat-vec launch that
     * consumes it — so q|k|v, gate|up and the logits matrix form their normalised int8 input themselves (TkGemvArgs::fuse = 1), the down
     * projection its SwiGLU input (fuse = 2): 8 launches per layer become 5.  Same arithmetic, value for value.  Such a launch reads
     * (x, slabs) of one buffer pair while workgroup 0 writes the updated stream into the other and all write their slabs there:
     *   q|k|v: x, partial -> x2, partial2;  attention reads partial2;  o -> partial;  gate|up: x2, partial -> x, partial2;
     *   down: partial2 -> partial — at every layer boundary x and `partial` hold what the unfused path leaves there. */
    bool kq = !tk_type_is_float(model->output.type);
    for (int l = l0; l < l1 && kq; ++l) {
        const TkLlmLayer& L = model->layers[l];
        kq = !tk_type_is_float(L.q.type) && !tk_type_is_float(L.k.type) && !tk_type_is_float(L.v.type) && !tk_type_is_float(L.o.type) &&
             !tk_type_is_float(L.gate.type) && !tk_type_is_float(L.up.type) && !tk_type_is_float(L.down.type);
    }
    const bool fuse = kq && producer_fusion_enabled() && tk_gemv_fuses_producer(nrows, D, h.ks_qkv, h.ks_down) &&
                      tk_gemv_fuses_producer(nrows, D, h.ks_gateup, h.ks_o) && tk_gemv_fuses_producer(nrows, FF, h.ks_down, h.ks_gateup) &&
                      tk_gemv_fuses_producer(nrows, D, 1, h.ks_down);
    auto fused_gemv = [&](const TkDevTensor* const* t, int nseg, int K, int ks, int n_total, float* out, int mode, const float* xin, float* xout,
                          const float* slab, int slab_ks, int slab_pitch, const float* w) {
        TkGemvArgs a{};
        for (int i = 0; i < nseg; ++i) a.seg[i] = seg_of(*t[i]);
        a.nseg = nseg; a.K = K; a.ks = ks; a.n_total = n_total; a.nrows = nrows; a.out = out;
        a.fuse = mode; a.fx_in = xin; a.fx_out = xout; a.fslab = slab; a.fks = slab_ks; a.fn_total = slab_pitch; a.fw = w; a.feps = h.rms_eps;
        tk_launch_gemv(a, s);
        return ks;
    };
    /* a form is only ever built by tk_pass_form.h's resolvers; one that names a launch its other fields rule out would read what nobody wrote */
    const bool scored = f.attn == TK_ATT_LONG || f.attn == TK_ATT_RUN;
    if ((f.rope_in_attention ? f.attn == TK_ATT_TILED || f.attn == TK_ATT_RUN : f.attn == TK_ATT_LONG) || (scored && !d_scores) ||
        (kv_type == TK_KV_Q8_0 && (f.rope_in_attention || f.attn != TK_ATT_ROW))) {
        if (launch_error.empty()) launch_error = "a pass was described in a form that does not exist";
        return;
    }
    /* k_attention_prefill's row -> tile table: built once per pass from the sequence ids on the device */
    if (f.attn == TK_ATT_TILED && l1 > l0) tk_launch_att_tiles(d_seq, nrows, d_tiles, s);
    int ks_res = 1; /* slabs of the pending residual update (the previous layer's down projection) */
    for (int l = l0; l < l1; ++l) {
        const TkLlmLayer& L = model->layers[l];
        const TkDevTensor* qkv[3] = {&L.q, &L.k, &L.v};
        const TkDevTensor* ot[1] = {&L.o};
        const TkDevTensor* gu[2] = {&L.gate, &L.up};
        const TkDevTensor* dn[1] = {&L.down};
        if (fuse) {
            const int ks_qkv = fused_gemv(qkv, 3, D, h.ks_qkv, QD + 2 * KVD, partial2, 1, x, x2, l == l0 ? nullptr : partial, ks_res, D, (const float*)L.attn_norm.data);
            enqueue_attention(f, partial2, ks_qkv, l, nrows);
            const int ks_o = enqueue_matmul(ot, 1, QD, h.ks_o, D, act_qd, partial, nrows);
            const int ks_gu = fused_gemv(gu, 2, D, h.ks_gateup, 2 * FF, partial2, 1, x2, x, partial, ks_o, D, (const float*)L.ffn_norm.data);
            ks_res = fused_gemv(dn, 1, FF, h.ks_down, D, partial, 2, nullptr, nullptr, partial2, ks_gu, 2 * FF, nullptr);
            continue;
        }
        tk_launch_rmsnorm_q8(x, l == l0 ? nullptr : partial, ks_res, D, (const float*)L.attn_norm.data, h.rms_eps, D, nrows, act_d, s);
        const int ks_qkv = enqueue_matmul(qkv, 3, D, h.ks_qkv, QD + 2 * KVD, act_d, partial, nrows);
        enqueue_attention(f, partial, ks_qkv, l, nrows);
        const int ks_o = enqueue_matmul(ot, 1, QD, h.ks_o, D, act_qd, partial, nrows);
        tk_launch_rmsnorm_q8(x, partial, ks_o, D, (const float*)L.ffn_norm.data, h.rms_eps, D, nrows, act_d, s);
        if (tk_gemv_fuses_swiglu(nrows, h.ks_gateup, L.gate.type, L.up.type)) { /* wide pass: SwiGLU in the launch's epilogue, `partial` holds h [rows][FF] */
            TkGemvArgs a{};
            a.seg[0] = seg_of(L.gate); a.seg[1] = seg_of(L.up);
            a.nseg = 2; a.K = D; a.ks = 1; a.n_total = FF; a.nrows = nrows; a.swiglu = 1;
            set_act(a, act_d); a.out = partial;
            tk_launch_gemv(a, s);
            tk_launch_quant_q8(partial, FF, nrows, act_ff, s);
        } else {
            const int ks_gu = enqueue_matmul(gu, 2, D, h.ks_gateup, 2 * FF, act_d, partial, nrows);
            tk_launch_swiglu_q8(partial, ks_gu, FF, nrows, act_ff, s);
        }
        ks_res = enqueue_matmul(dn, 1, FF, h.ks_down, D, act_ff, partial, nrows);
    }
    last_ks_res = ks_res;
    if (!f.head) { /* prompt rows whose logits nobody reads (K/V are already appended), or a pipeline stage that hands x on */
        if (fold_out && l1 > l0) tk_launch_residual_fold(x, partial, ks_res, D, D, nrows, s);
        return;
    }
    const TkDevTensor* lm[1] = {&model->output};
    if (fuse) (void)fused_gemv(lm, 1, D, 1, h.vocab, logits, 1, x, x2, l1 > l0 ? partial : nullptr, ks_res, D, (const float*)model->out_norm.data);
    else {
        tk_launch_rmsnorm_q8(x, l1 > l0 ? partial : nullptr, ks_res, D, (const float*)model->out_norm.data, h.rms_eps, D, nrows, act_d, s);
        (void)enqueue_matmul(lm, 1, D, 1, h.vocab, act_d, logits, nrows);
    }
    /* llama.cpp's order: bias, penalties, grammar, chain — masks and sampling see the adjusted logits */
    if (f.adjust) tk_launch_logit_adjust(logits, h.vocab, nrows, d_adj, d_adj_ids, d_adj_bias_ids, d_adj_bias, s);
    tk_launch_argmax(logits, h.vocab, nrows, d_mask, d_mask_row, d_samp, d_tok, d_pos, d_nsteps, d_hist, TK_MAX_ROWS, s);
    /* the rows that ask: the log-probability of the id just picked, on the logits the pick read (adjusted, unmasked) */
    if (f.logprobs) tk_launch_token_logprobs(logits, h.vocab, h.vocab, nrows, d_lp_ntop, d_tok, d_lp_rec, s);
}

static bool graphs_enabled() {
    /* TK_MI355X_NO_GRAPH=1: eager launches, for profilers that cannot follow hipGraphLaunch (see DESIGN.md "Profiling") */
    const char* ng = getenv("TK_MI355X_NO_GRAPH");
    return !(ng && ng[0] == '1');
}

/* two events that are released on every path */
struct EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t create() { const hipError_t e = hipEventCreate(&e0); return e != hipSuccess ? e : hipEventCreate(&e1); }
    ~EventPair() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};

/* one capture at a time per process; relaxed mode: other host threads (detector / ASR / VAD streams) keep calling allocation and copy
 * APIs while this stream records */
static std::mutex g_capture_mu;

bool TkLlmSession::capture(hipGraphExec_t* slot, const char* what, const std::function<void()>& enqueue) {
    if (*slot) return true;
    const auto t_cap = std::chrono::steady_clock::now();
    struct Tally { TkLlmSession* s; std::chrono::steady_clock::time_point t0; ~Tally() { s->n_captures++; s->capture_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); } } tally{this, t_cap};
    std::lock_guard<std::mutex> lk(g_capture_mu);
    hipGraph_t g = nullptr;
    HIPQ(hipStreamBeginCapture(stream, hipStreamCaptureModeRelaxed));
    launch_error.clear();
    enqueue();
    /* from here on the stream must leave capture mode and the graph must be freed whatever fails */
    const hipError_t e_end = hipStreamEndCapture(stream, &g);
    hipError_t e_inst = hipSuccess;
    if (e_end == hipSuccess && launch_error.empty()) e_inst = hipGraphInstantiate(slot, g, nullptr, nullptr, 0);
    if (g) (void)hipGraphDestroy(g);
    if (e_end != hipSuccess || e_inst != hipSuccess || !launch_error.empty()) {
        if (*slot && e_inst != hipSuccess) { (void)hipGraphExecDestroy(*slot); }
        *slot = nullptr;
        (void)hipGetLastError();
        error = !launch_error.empty() ? launch_error
                : std::string("graph capture of ") + what + " failed: " + hipGetErrorString(e_end != hipSuccess ? e_end : e_inst);
        return false;
    }
    return true;
}

hipGraphExec_t TkLlmSession::capture_pass(const TkPassForm& f, int nrows) {
    hipGraphExec_t* slot = &graphs[tk_pass_form_key(f)][nrows];
    if (*slot) return *slot; /* the replay path: an index, nothing built */
    return capture(slot, "a pass", [&] { enqueue_pass(nrows, f); }) ? *slot : nullptr;
}

bool TkLlmSession::launch_pass(const TkPassForm& f, int nrows, bool use_graph) {
    last_pass_key = tk_pass_form_key(f);
    if (use_graph) {
        const hipGraphExec_t g = capture_pass(f, nrows);
        if (!g) return false;
        HIPQ(hipGraphLaunch(g, stream));
        return true;
    }
    launch_error.clear();
    enqueue_pass(nrows, f);
    if (!launch_error.empty()) { error = launch_error; (void)hipStreamSynchronize(stream); return false; }
    return true;
}

TkPassCaps TkLlmSession::pass_caps(int nrows) const {
    const TkLlmHParams& h = model->hp;
    if (kv_type == TK_KV_Q8_0) return TkPassCaps{false, false, false}; /* one attention, the per-row one */
    return TkPassCaps{d_scores != nullptr, tk_attention_prefill_applies(h.n_head, h.n_kv_head, h.head_dim), tk_attention_long_applies(nrows, h.n_head, h.n_kv_head, h.head_dim)};
}

bool TkLlmSession::check_pass_rows(int nrows, const int32_t* seq, const int32_t* pos, const int32_t* tok, int* top, bool* distinct) {
    if (nrows <= 0 || nrows > TK_MAX_ROWS) { error = "nrows must be in [1,256]"; return false; }
    *top = 0;
    for (int r = 0; r < nrows; ++r) {
        if (seq[r] < 0 || seq[r] >= max_seq || pos[r] < 0 || pos[r] >= max_ctx || (tok && (tok[r] < 0 || tok[r] >= model->hp.vocab))) {
            error = "row out of range (sequence id, position or token id)";
            return false;
        }
        *top = pos[r] > *top ? pos[r] : *top;
    }
    if (!distinct) return true;
    *distinct = true; /* every sequence at most once in the pass -> rope/append can be fused into attention */
    for (int a = 0; a < nrows && *distinct; ++a)
        for (int b = a + 1; b < nrows; ++b)
            if (seq[a] == seq[b]) { *distinct = false; break; }
    return true;
}

bool TkLlmSession::upload_rows(int nrows, const int32_t* seq, const int32_t* pos, const int32_t* tok) {
    HIPQ(hipMemcpyAsync(d_seq, seq, nrows * 4, hipMemcpyHostToDevice, stream));
    HIPQ(hipMemcpyAsync(d_pos, pos, nrows * 4, hipMemcpyHostToDevice, stream));
    if (tok) HIPQ(hipMemcpyAsync(d_tok, tok, nrows * 4, hipMemcpyHostToDevice, stream));
    HIPQ(hipMemsetAsync(d_nsteps, 0, TK_MAX_ROWS * 4, stream));
    return true;
}

bool TkLlmSession::clear_row_tables(unsigned which) {
    if ((which & TK_ROWS_MASKS) && mask_rows_dirty) { HIPQ(hipMemsetAsync(d_mask_row, 0xFF, TK_MAX_ROWS * 4, stream)); mask_rows_dirty = false; }
    if ((which & TK_ROWS_SAMPLING) && samp_dirty) { HIPQ(hipMemsetAsync(d_samp, 0, TK_MAX_ROWS * sizeof(TkSampleRow), stream)); samp_dirty = false; }
    if ((which & TK_ROWS_ADJUST) && adj_dirty) { HIPQ(hipMemsetAsync(d_adj, 0, TK_MAX_ROWS * sizeof(TkAdjustRow), stream)); adj_dirty = false; }
    if ((which & TK_ROWS_LOGPROBS) && lp_dirty) { HIPQ(hipMemsetAsync(d_lp_ntop, 0xFF, TK_MAX_ROWS * 4, stream)); lp_dirty = false; }
    return true;
}

bool TkLlmSession::forward(int nrows, const int32_t* seq, const int32_t* pos, const int32_t* tok, float* logits_host, int32_t* argmax_host,
                           bool lm_head, const uint32_t* const* row_masks, const TkSampleRow* row_samp, const TkLogitAdjust* row_adjust,
                           const int32_t* row_ntop, TkTokenLogprob* records_host) {
    int top = 0, ngm = 0;
    const uint32_t* gm_ptr[TK_MAX_ROWS]; /* the host mask pointers of the rows whose masks the device builds */
    bool distinct = true, any_adj = false, any_lp = false;
    if (!check_pass_rows(nrows, seq, pos, tok, &top, &distinct)) return false;
    for (int r = 0; r < nrows && lm_head && row_ntop; ++r) {
        if (const char* why = tk_logprob_check(row_ntop[r], model->hp.vocab)) { error = "log-probabilities of row " + std::to_string(r) + ": " + why; return false; }
        any_lp = any_lp || row_ntop[r] >= 0;
    }
    if (any_lp && !records_host) { error = "log-probabilities asked for without records to fill"; return false; }
    for (int r = 0; r < nrows && lm_head && row_adjust; ++r) {
        if (const char* why = row_adjust[r].check(model->hp.vocab)) { error = "logit adjustment of row " + std::to_string(r) + ": " + why; return false; }
        any_adj = any_adj || !row_adjust[r].neutral();
    }
    HIPQ(hipSetDevice(model->device));
    if (!upload_rows(nrows, seq, pos, tok)) return false;
    if (lm_head) { /* per-row sampling masks: the masks of the constrained rows, compacted, + the row -> mask table the arg max kernel reads */
        int32_t rowtab[TK_MAX_ROWS];
        int nmask = 0;
        const size_t words = ((size_t)model->hp.vocab + 31) / 32;
        for (int r = 0; r < TK_MAX_ROWS; ++r) rowtab[r] = -1;
        for (int r = 0; r < nrows; ++r) {
            if (row_masks && row_masks[r]) {
                /* a row with a grammar state attached (attach_grammar_state) gets its bits from k_grammar_mask below, not from the host */
                bool on_device = false;
                {
                    std::lock_guard<std::mutex> lk(gm_mu);
                    auto it = gm_rows.find(row_masks[r]);
                    if (it != gm_rows.end()) { /* only a session with the vocabulary image installed has entries */
                        h_gm_states[ngm] = it->second.image;
                        h_gm_states[ngm].mask_row = nmask;
                        gm_ptr[ngm++] = row_masks[r];
                        on_device = true;
                    }
                }
                if (!on_device) HIPQ(hipMemcpyAsync(d_mask + (size_t)nmask * words, row_masks[r], words * 4, hipMemcpyHostToDevice, stream));
                rowtab[r] = nmask++;
            }
        }
        if (ngm > 0) { /* ONE launch for every such row of the pass, on the stream in front of the pass's graph (pinned staging: free again when forward() has waited) */
            HIPQ(hipMemcpyAsync(d_gm_states, h_gm_states, (size_t)ngm * sizeof(TkGrammarStateImage), hipMemcpyHostToDevice, stream));
            HIPQ(hipMemsetAsync(d_mask_undecided, 0, (size_t)ngm * 4, stream));
            tk_launch_grammar_mask(d_gm_arena, d_gm_states, ngm, d_gm_offsets, d_gm_pieces, model->hp.vocab, gm_eos, d_mask, d_mask_undecided, stream);
        }
        if (nmask > 0 || mask_rows_dirty) {
            HIPQ(hipMemcpyAsync(d_mask_row, rowtab, TK_MAX_ROWS * 4, hipMemcpyHostToDevice, stream)); /* whole table (a wider pass may have left entries); pageable source: staged before the call returns */
            mask_rows_dirty = nmask > 0;
        }
        /* per-row sampling state (temp <= 0: greedy): data of the pass like the masks, so sampled and greedy rows share passes and graphs */
        bool any_samp = false;
        for (int r = 0; r < nrows && row_samp; ++r) any_samp = any_samp || row_samp[r].temp > 0.0f;
        if (any_samp) {
            if (model->hp.vocab > 65536) { error = "stochastic sampling supports vocabularies of at most 65536 tokens"; return false; }
            TkSampleRow tab[TK_MAX_ROWS] = {};
            for (int r = 0; r < nrows; ++r) tab[r] = row_samp[r];
            HIPQ(hipMemcpyAsync(d_samp, tab, sizeof tab, hipMemcpyHostToDevice, stream));
            samp_dirty = true;
        }
        /* logit adjustment: the tables of the pass's rows through the pinned block (free: the last forward() waited for the stream); a neutral row
         * gets the all-zero descriptor its workgroup returns on */
        if (any_adj) {
            TkAdjustRow* hd = (TkAdjustRow*)h_adj;
            int32_t* hids = (int32_t*)(hd + TK_MAX_ROWS);
            int32_t* hbids = hids + (size_t)TK_MAX_ROWS * TK_ADJUST_MAX_RECENT;
            float* hbias = (float*)(hbids + (size_t)TK_MAX_ROWS * TK_ADJUST_MAX_BIAS);
            memset(hd, 0, TK_MAX_ROWS * sizeof(TkAdjustRow));
            for (int r = 0; r < nrows; ++r) {
                const TkLogitAdjust& a = row_adjust[r];
                if (a.neutral()) continue;
                hd[r] = a.row();
                if (a.n_recent > 0) memcpy(hids + (size_t)r * TK_ADJUST_MAX_RECENT, a.recent, (size_t)a.n_recent * 4);
                if (a.n_bias > 0) {
                    memcpy(hbids + (size_t)r * TK_ADJUST_MAX_BIAS, a.bias_ids, (size_t)a.n_bias * 4);
                    memcpy(hbias + (size_t)r * TK_ADJUST_MAX_BIAS, a.bias, (size_t)a.n_bias * 4);
                }
            }
            HIPQ(hipMemcpyAsync(d_adj, hd, TK_MAX_ROWS * sizeof(TkAdjustRow), hipMemcpyHostToDevice, stream));
            HIPQ(hipMemcpyAsync(d_adj_ids, hids, (size_t)nrows * TK_ADJUST_MAX_RECENT * 4, hipMemcpyHostToDevice, stream));
            HIPQ(hipMemcpyAsync(d_adj_bias_ids, hbids, (size_t)nrows * TK_ADJUST_MAX_BIAS * 4, hipMemcpyHostToDevice, stream));
            HIPQ(hipMemcpyAsync(d_adj_bias, hbias, (size_t)nrows * TK_ADJUST_MAX_BIAS * 4, hipMemcpyHostToDevice, stream));
            adj_dirty = true;
        }
        /* log-probabilities: the per-row n_top table, uploaded only when a row asks (pageable source: staged before the call returns) */
        if (any_lp) {
            int32_t ntab[TK_MAX_ROWS];
            for (int r = 0; r < TK_MAX_ROWS; ++r) ntab[r] = r < nrows ? row_ntop[r] : -1;
            HIPQ(hipMemcpyAsync(d_lp_ntop, ntab, TK_MAX_ROWS * 4, hipMemcpyHostToDevice, stream));
            lp_dirty = true;
        }
        /* the tables no row of this pass filled go back to neutral (masks: the upload above is the whole table) */
        if (!clear_row_tables((any_samp ? 0 : TK_ROWS_SAMPLING) | (any_adj ? 0 : TK_ROWS_ADJUST) | (any_lp ? 0 : TK_ROWS_LOGPROBS))) return false;
    }
    /* masked, sampled and greedy rows ride the same graphs (their tables are data); without the head the pass ropes apart whatever its rows, so
     * that it is the form of a prompt chunk */
    /* with the head, rows that are runs of consecutive positions — a verify pass with tables — take the attention a verify pass of them takes */
    bool runs = lm_head && !distinct && nrows <= TK_LONG_ATT_MAX_ROWS;
    for (int r = 1; r < nrows && runs; ++r) {
        if (seq[r] == seq[r - 1]) { runs = pos[r] == pos[r - 1] + 1; continue; }
        for (int b = 0; b + 1 < r && runs; ++b) runs = seq[b] != seq[r];
    }
    const bool once = distinct && kv_type == TK_KV_F16; /* a Q8_0 session always ropes apart */
    const TkPassForm form = lm_head ? tk_pass_form_rows(once, runs, nrows, top, pass_caps(nrows), any_adj, any_lp) : tk_pass_form(false, false, nrows, top, pass_caps(nrows));
    if (!launch_pass(form, nrows, graphs_enabled())) return false;
    HIPQ(hipGetLastError());
    if (!lm_head) { HIPQ(hipStreamSynchronize(stream)); return true; }
    if (logits_host) HIPQ(hipMemcpyAsync(logits_host, logits, (size_t)nrows * model->hp.vocab * 4, hipMemcpyDeviceToHost, stream));
    if (argmax_host) HIPQ(hipMemcpyAsync(argmax_host, d_tok, nrows * 4, hipMemcpyDeviceToHost, stream));
    if (any_lp) HIPQ(hipMemcpyAsync(h_lp_rec, d_lp_rec, (size_t)nrows * sizeof(TkTokenLogprob), hipMemcpyDeviceToHost, stream));
    if (ngm > 0) HIPQ(hipMemcpyAsync(h_mask_undecided, d_mask_undecided, (size_t)ngm * 4, hipMemcpyDeviceToHost, stream));
    HIPQ(hipStreamSynchronize(stream));
    if (ngm > 0) { /* the undecided counts came back with the ids: into the registry, where the rows' owners read them */
        std::lock_guard<std::mutex> lk(gm_mu);
        for (int i = 0; i < ngm; ++i) {
            auto it = gm_rows.find(gm_ptr[i]);
            if (it != gm_rows.end()) { it->second.ran = true; it->second.undecided = h_mask_undecided[i]; }
        }
    }
    /* the records of the rows that asked, as far as they were filled: everything else of records_host stays as the caller left it */
    for (int r = 0; r < nrows && any_lp; ++r) {
        if (row_ntop[r] < 0) continue;
        const TkTokenLogprob& g = h_lp_rec[r];
        TkTokenLogprob& o = records_host[r];
        o.logprob = g.logprob;
        o.n_top = g.n_top < 0 ? 0 : g.n_top > TK_LOGPROB_MAX_TOP ? TK_LOGPROB_MAX_TOP : g.n_top;
        for (int j = 0; j < o.n_top; ++j) { o.top_ids[j] = g.top_ids[j]; o.top_logprobs[j] = g.top_logprobs[j]; }
    }
    return true;
}

bool TkLlmSession::forward_verify(int nrows, const int32_t* seq, const int32_t* pos, const int32_t* tok, int form, float* logits_host, int32_t* picks_host,
                                  bool* bad_args) {
    const TkLlmHParams& h = model->hp;
    if (bad_args) *bad_args = true;
    if (!seq || !pos || !tok) { error = "verify pass: missing row arrays"; return false; }
    int top = 0;
    if (!check_pass_rows(nrows, seq, pos, tok, &top, nullptr)) return false;
    for (int r = 1; r < nrows; ++r) {
        if (seq[r] == seq[r - 1] && pos[r] != pos[r - 1] + 1) { error = "verify pass: the rows of a sequence stand at consecutive ascending positions"; return false; }
        for (int b = 0; b + 1 < r; ++b)
            if (seq[b] == seq[r] && seq[r - 1] != seq[r]) { error = "verify pass: the rows of a sequence are contiguous in the pass"; return false; }
    }
    const TkPassCaps caps = pass_caps(nrows);
    if (form == -1) form = tk_verify_form(nrows, top, caps);
    if (const char* why = tk_verify_form_error(form, caps)) { error = why; return false; }
    if (bad_args) *bad_args = false;
    HIPQ(hipSetDevice(model->device));
    if (!upload_rows(nrows, seq, pos, tok) || !clear_row_tables(TK_ROWS_MASKS | TK_ROWS_SAMPLING | TK_ROWS_ADJUST | TK_ROWS_LOGPROBS)) return false;
    if (!launch_pass(tk_pass_form_verify(form), nrows, graphs_enabled())) return false;
    HIPQ(hipGetLastError());
    if (logits_host) HIPQ(hipMemcpyAsync(logits_host, logits, (size_t)nrows * h.vocab * 4, hipMemcpyDeviceToHost, stream));
    if (picks_host) HIPQ(hipMemcpyAsync(picks_host, d_tok, nrows * 4, hipMemcpyDeviceToHost, stream));
    HIPQ(hipStreamSynchronize(stream));
    return true;
}

bool TkLlmSession::forward_stage(int nrows, const int32_t* seq, const int32_t* pos, const int32_t* tok, const float* x_in, float* x_out, bool x_on_host,
                                 int l0, int l1, bool head, int32_t* argmax_host) {
    const TkLlmHParams& h = model->hp;
    if (l0 < 0 || l1 < l0 || l1 > h.n_layer) { error = "bad layer range"; return false; }
    if ((tok == nullptr) == (x_in == nullptr)) { error = "a stage starts from tokens (first stage) or from a residual stream, not both"; return false; }
    if (head && l1 != h.n_layer) { error = "the head belongs to the stage that ends at the last layer"; return false; }
    if (!head && !x_out) { error = "a stage without the head must hand its residual stream on"; return false; }
    if (refuse_q8("forward_stage")) return false;
    int top = 0;
    bool distinct = true;
    if (!check_pass_rows(nrows, seq, pos, tok, &top, &distinct)) return false;
    HIPQ(hipSetDevice(model->device));
    if (!upload_rows(nrows, seq, pos, tok) || !clear_row_tables(TK_ROWS_MASKS | TK_ROWS_ADJUST | TK_ROWS_LOGPROBS)) return false;
    const size_t xb = (size_t)nrows * h.d_model * 4;
    if (x_in) HIPQ(hipMemcpyAsync(x, x_in, xb, x_on_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, stream));
    launch_error.clear();
    enqueue_range(nrows, l0, l1, tok != nullptr, !head, tk_pass_form(head, distinct, nrows, top, pass_caps(nrows)));
    if (!launch_error.empty()) { error = launch_error; (void)hipStreamSynchronize(stream); return false; }
    HIPQ(hipGetLastError());
    if (!head) HIPQ(hipMemcpyAsync(x_out, x, xb, x_on_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, stream));
    else if (argmax_host) HIPQ(hipMemcpyAsync(argmax_host, d_tok, nrows * 4, hipMemcpyDeviceToHost, stream));
    HIPQ(hipStreamSynchronize(stream));
    return true;
}

__global__ void k_stage_rows(const int32_t* __restrict__ tab, int n, int stride, int32_t* seq, int32_t* pos, int32_t* tok) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { seq[i] = tab[i]; pos[i] = tab[stride + i]; tok[i] = tab[2 * stride + i]; }
}

/* Prompt rows that nobody samples from (all but the last token of every prompt): the whole schedule — (sequence, position, token) of
 * every row of every pass — is uploaded once, each pass is one tiny staging launch + one replay of a captured pass (no lm_head,
 * rope/append as its own kernel so a pass may hold several positions of one sequence), and the host synchronises once, in the final
 * sampling pass.  Same kernels, same order, same arithmetic as forward(): bit-identical results. */
bool TkLlmSession::prefill(int nseq, int n_prompt, const int32_t* tokens, int32_t* first_tokens_host) {
    if (nseq <= 0 || nseq > TK_MAX_ROWS || nseq > max_seq) { error = "nseq must be in [1, min(256, max_seq)]"; return false; }
    if (n_prompt <= 0 || n_prompt >= max_ctx) { error = "prompt does not fit the context"; return false; }
    for (int64_t i = 0; i < (int64_t)nseq * n_prompt; ++i)
        if (tokens[i] < 0 || tokens[i] >= model->hp.vocab) { error = "row out of range (sequence id, position or token id)"; return false; }
    HIPQ(hipSetDevice(model->device));
    /* all but the last prompt token: up to 256 rows per pass, positions ascending inside a sequence so causality holds inside a pass */
    const int64_t total = (int64_t)nseq * (n_prompt - 1);
    if (total > 0) {
        std::vector<int32_t> tab((size_t)3 * total);
        int64_t k = 0;
        for (int s = 0; s < nseq; ++s)
            for (int p = 0; p + 1 < n_prompt; ++p, ++k) {
                tab[k] = s; tab[total + k] = p; tab[2 * total + k] = tokens[(size_t)s * n_prompt + p];
            }
        if ((int64_t)tab_cap < 3 * total) {
            if (d_tab) (void)hipFree(d_tab);
            d_tab = nullptr;
            HIPQ(hipMalloc((void**)&d_tab, (size_t)3 * total * 4));
            tab_cap = (size_t)3 * total;
        }
        HIPQ(hipMemcpyAsync(d_tab, tab.data(), (size_t)3 * total * 4, hipMemcpyHostToDevice, stream));
        HIPQ(hipStreamSynchronize(stream)); /* `tab` is pageable host memory that dies with this scope */
        const bool use_graph = graphs_enabled();
        for (int64_t off = 0; off < total; off += TK_MAX_ROWS) {
            const int n = (int)std::min<int64_t>(TK_MAX_ROWS, total - off);
            const int top = *std::max_element(tab.data() + total + off, tab.data() + total + off + n);
            hipLaunchKernelGGL(k_stage_rows, dim3((n + 255) / 256), dim3(256), 0, stream, d_tab + off, n, (int)total, d_seq, d_pos, d_tok);
            if (!launch_pass(tk_pass_form(false, false, n, top, pass_caps(n)), n, use_graph)) return false;
        }
        HIPQ(hipGetLastError());
    }
    /* last prompt token of every sequence: row r == sequence r, sampled -> decode() continues from here */
    std::vector<int32_t> sq(nseq), ps(nseq), tk(nseq);
    for (int s = 0; s < nseq; ++s) { sq[s] = s; ps[s] = n_prompt - 1; tk[s] = tokens[(size_t)s * n_prompt + n_prompt - 1]; }
    return forward(nseq, sq.data(), ps.data(), tk.data(), nullptr, first_tokens_host, true);
}

bool TkLlmSession::decode(int nrows, int n_steps, int32_t* out_tokens_host) {
    if (nrows <= 0 || nrows > TK_MAX_ROWS) { error = "nrows must be in [1,256]"; return false; }
    if (n_steps <= 0 || n_steps > hist_cap) { error = "n_steps exceeds the session context"; return false; }
    HIPQ(hipSetDevice(model->device));
    /* positions must stay inside the cache for the whole loop */
    int32_t hpos[TK_MAX_ROWS];
    HIPQ(hipMemcpyAsync(hpos, d_pos, nrows * 4, hipMemcpyDeviceToHost, stream));
    HIPQ(hipStreamSynchronize(stream));
    for (int r = 0; r < nrows; ++r)
        if (hpos[r] + n_steps > max_ctx) { error = "decode would run past max_ctx"; return false; }
    const bool use_graph = graphs_enabled();
    int top0 = 0;
    for (int r = 0; r < nrows; ++r) top0 = hpos[r] > top0 ? hpos[r] : top0;
    HIPQ(hipMemsetAsync(d_nsteps, 0, TK_MAX_ROWS * 4, stream));
    /* the loop samples unconstrained, unadjusted and reports no log-probabilities: its steps are plain forms */
    if (!clear_row_tables(TK_ROWS_MASKS | TK_ROWS_ADJUST | TK_ROWS_LOGPROBS)) return false;
    const TkPassCaps caps = pass_caps(nrows);
    EventPair ev;
    HIPQ(ev.create());
    HIPQ(hipEventRecord(ev.e0, stream));
    for (int i = 0; i < n_steps; ++i) /* positions advance on the device; the host knows where the loop stands */
        if (!launch_pass(tk_pass_form(true, kv_type == TK_KV_F16, nrows, top0 + i, caps), nrows, use_graph)) { (void)hipStreamSynchronize(stream); return false; }
    HIPQ(hipGetLastError());
    HIPQ(hipEventRecord(ev.e1, stream));
    if (out_tokens_host) HIPQ(hipMemcpyAsync(out_tokens_host, d_hist, (size_t)n_steps * TK_MAX_ROWS * 4, hipMemcpyDeviceToHost, stream));
    HIPQ(hipStreamSynchronize(stream));
    float ms = 0.0f;
    HIPQ(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    last_step_ms = ms / n_steps;
    return true;
}

bool TkLlmSession::time_launches(int iters, const std::function<void()>& warm, const std::function<void(int)>& launch, float* avg_ms) {
    EventPair ev;
    struct Exec { hipGraphExec_t g = nullptr; ~Exec() { if (g) (void)hipGraphExecDestroy(g); } } ge;
    HIPQ(ev.create());
    warm();
    /* launched the way decode() launches them: as nodes of a hipGraph (unless TK_MI355X_NO_GRAPH=1, see decode()) */
    const bool use_graph = graphs_enabled();
    if (use_graph) {
        if (!capture(&ge.g, "a timing loop", [&] { for (int i = 0; i < iters; ++i) launch(i); })) return false;
        HIPQ(hipGraphLaunch(ge.g, stream)); /* warm */
    }
    HIPQ(hipEventRecord(ev.e0, stream));
    if (use_graph) HIPQ(hipGraphLaunch(ge.g, stream));
    else for (int i = 0; i < iters; ++i) launch(i);
    HIPQ(hipEventRecord(ev.e1, stream));
    HIPQ(hipStreamSynchronize(stream));
    float ms = 0.0f;
    HIPQ(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    *avg_ms = ms / iters;
    return true;
}

bool TkLlmSession::time_gemv(int layer, int which, int nrows, int iters, float* avg_ms, double* algo_bytes) {
    const TkLlmHParams& h = model->hp;
    if (layer < 0 || layer >= h.n_layer || nrows < 1 || nrows > TK_MAX_ROWS) { error = "bad layer / nrows"; return false; }
    HIPQ(hipSetDevice(model->device));
    auto args_for = [&](int l, double* bytes) {
        const TkLlmLayer& L = model->layers[l];
        TkGemvArgs a{};
        a.nrows = nrows;
        if (which == 0) { /* gate+up */
            a.seg[0] = seg_of(L.gate); a.seg[1] = seg_of(L.up); a.nseg = 2; a.K = h.d_model; a.ks = h.ks_gateup; a.n_total = 2 * h.d_ff;
            if (tk_gemv_fuses_swiglu(nrows, h.ks_gateup, L.gate.type, L.up.type)) { a.swiglu = 1; a.n_total = h.d_ff; } /* the launch a wide pass makes */
            set_act(a, act_d); a.out = partial;
            *bytes = (double)L.gate.bytes + (double)L.up.bytes;
        } else if (which == 1) { /* down */
            a.seg[0] = seg_of(L.down); a.nseg = 1; a.K = h.d_ff; a.ks = h.ks_down; a.n_total = h.d_model;
            set_act(a, act_ff); a.out = partial;
            *bytes = (double)L.down.bytes;
        } else if (which == 4) { /* o */
            a.seg[0] = seg_of(L.o); a.nseg = 1; a.K = h.n_head * h.head_dim; a.ks = h.ks_o; a.n_total = h.d_model;
            set_act(a, act_qd); a.out = partial;
            *bytes = (double)L.o.bytes;
        } else if (which == 2) { /* qkv */
            a.seg[0] = seg_of(L.q); a.seg[1] = seg_of(L.k); a.seg[2] = seg_of(L.v); a.nseg = 3; a.K = h.d_model; a.ks = h.ks_qkv;
            a.n_total = (h.n_head + 2 * h.n_kv_head) * h.head_dim;
            set_act(a, act_d); a.out = partial;
            *bytes = (double)L.q.bytes + (double)L.k.bytes + (double)L.v.bytes;
        } else { /* lm head */
            a.seg[0] = seg_of(model->output); a.nseg = 1; a.K = h.d_model; a.ks = 1; a.n_total = h.vocab;
            set_act(a, act_d); a.out = logits;
            *bytes = (double)model->output.bytes;
        }
        /* algorithmic bytes of one launch: the weight tiles once, the int8 activation images (+ block scales and sub-block sums) once,
         * the fp32 K-split partial outputs once */
        *bytes += (double)nrows * ((double)a.K + (double)a.K / 256.0 * (4.0 + 16.0)) + (double)a.ks * nrows * (double)a.n_total * 4.0;
        return a;
    };
    /* every layer whose tensors have the same types as `layer`: cycling through them keeps each launch on
     * cold HBM lines (32 layers x 66 MB >> the 256 MiB Infinity Cache), as in a real decode step */
    std::vector<TkGemvArgs> set;
    double bytes = 0.0;
    const char* hot = getenv("TK_MI355X_TIME_HOT"); /* =1: the SAME layer's launch back to back (weights resident in L2 / Infinity Cache): the bound a prefetch could reach */
    for (int l = 0; l < h.n_layer; ++l) {
        if ((which == 3 || (hot && hot[0] == '1')) && l != layer) continue;
        if (model->layers[l].v.type != model->layers[layer].v.type || model->layers[l].down.type != model->layers[layer].down.type) continue;
        double b;
        set.push_back(args_for(l, &b));
        bytes = b;
    }
    *algo_bytes = bytes;
    return time_launches(iters, [&] { for (size_t i = 0; i < set.size(); ++i) tk_launch_gemv(set[i], stream); },
                         [&](int i) { tk_launch_gemv(set[(size_t)i % set.size()], stream); }, avg_ms);
}

/* stand-alone timing of the decode attention launch (k_attention, fused rope/append form) at `nrows` rows whose sequences all sit at
 * position ctx - 1: `iters` launches cycling through the layers (each layer's cache region is its own HBM range), launched as hipGraph
 * nodes like decode().  kv_bytes = the K and V rows one launch must read once: nrows * ctx * n_kv_head * head_dim * 2 B * 2. */
bool TkLlmSession::time_kv_copy(int n_pos, int n_dst, int iters, float* kernel_ms, float* memcpy_ms, double* bytes) {
    const TkLlmHParams& h = model->hp;
    if (n_pos < 1 || n_pos > max_ctx || n_dst < 1 || n_dst >= max_seq || n_dst > TK_MAX_ROWS || iters < 1) { error = "bad n_pos / n_dst / iters"; return false; }
    if (refuse_q8("time_kv_copy")) return false;
    HIPQ(hipSetDevice(model->device));
    std::vector<TkKvCopyDesc> ds((size_t)n_dst);
    for (int d = 0; d < n_dst; ++d) ds[(size_t)d] = TkKvCopyDesc{0, d + 1, 0, n_pos};
    const size_t width = (size_t)n_pos * h.head_dim * 2, pitch = (size_t)max_ctx * h.head_dim * 2; /* one KV head's run; the next head's starts a pitch on */
    auto memcpy_form = [&]() -> bool {
        for (int d = 0; d < n_dst; ++d)
            for (int l = 0; l < h.n_layer; ++l) {
                const size_t so = (((size_t)l * max_seq + 0) * h.n_kv_head) * max_ctx * h.head_dim, dof = (((size_t)l * max_seq + d + 1) * h.n_kv_head) * max_ctx * h.head_dim;
                HIPQ(hipMemcpy2DAsync(kcache + dof, pitch, kcache + so, pitch, width, (size_t)h.n_kv_head, hipMemcpyDeviceToDevice, stream));
                HIPQ(hipMemcpy2DAsync(vcache + dof, pitch, vcache + so, pitch, width, (size_t)h.n_kv_head, hipMemcpyDeviceToDevice, stream));
            }
        return true;
    };
    hipEvent_t e0, e1, e2;
    HIPQ(hipEventCreate(&e0));
    HIPQ(hipEventCreate(&e1));
    HIPQ(hipEventCreate(&e2));
    double k_sum = 0.0, m_sum = 0.0;
    for (int i = -1; i < iters; ++i) { /* round -1 is the warm-up */
        HIPQ(hipEventRecord(e0, stream));
        if (!enqueue_kv_copy(ds.data(), n_dst)) return false;
        HIPQ(hipEventRecord(e1, stream));
        if (!memcpy_form()) return false;
        HIPQ(hipEventRecord(e2, stream));
        HIPQ(hipStreamSynchronize(stream));
        float k = 0.0f, m = 0.0f;
        HIPQ(hipEventElapsedTime(&k, e0, e1));
        HIPQ(hipEventElapsedTime(&m, e1, e2));
        if (i >= 0) { k_sum += k; m_sum += m; }
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipEventDestroy(e2);
    *kernel_ms = (float)(k_sum / iters);
    *memcpy_ms = (float)(m_sum / iters);
    *bytes = 2.0 * (double)n_dst * n_pos * h.n_layer * h.n_kv_head * h.head_dim * 2.0 * 2.0; /* read + write, K + V, f16 */
    return true;
}

bool TkLlmSession::time_attention(int nrows, int ctx, int iters, float* avg_ms, double* kv_bytes) {
    const TkLlmHParams& h = model->hp;
    if (nrows < 1 || nrows > TK_MAX_ROWS || nrows > max_seq || ctx < 1 || ctx > max_ctx || iters < 1) { error = "bad nrows / ctx / iters"; return false; }
    HIPQ(hipSetDevice(model->device));
    std::vector<int32_t> sq(nrows), ps(nrows, ctx - 1);
    for (int r = 0; r < nrows; ++r) sq[r] = r;
    HIPQ(hipMemcpyAsync(d_seq, sq.data(), nrows * 4, hipMemcpyHostToDevice, stream));
    HIPQ(hipMemcpyAsync(d_pos, ps.data(), nrows * 4, hipMemcpyHostToDevice, stream));
    HIPQ(hipStreamSynchronize(stream));
    const int QD = h.n_head * h.head_dim, KVD = h.n_kv_head * h.head_dim;
    /* TK_MI355X_TIME_UNFUSED=1: time the two-launch form instead (k_qkv_rope_append + k_attention<.., not fused>): what a decode pass would
     * cost without the fused prologue */
    const char* uf = getenv("TK_MI355X_TIME_UNFUSED");
    const char* lf = getenv("TK_MI355X_TIME_LONG"); /* =1: the three-launch long-context form (tk_launch_attention_long) where it applies */
    const bool longf = lf && lf[0] == '1' && d_scores && tk_attention_long_applies(nrows, h.n_head, h.n_kv_head, h.head_dim);
    const bool unfused = (uf && uf[0] == '1') || longf;
    auto launch = [&](int l) {
        if (kv_type == TK_KV_Q8_0) { /* the Q8_0 session's decode launch set: append + kernel 6 */
            tk_launch_qkv_rope_append_q8(partial, h.ks_qkv, QD + 2 * KVD, h.n_head, h.n_kv_head, h.head_dim, rope_cos, rope_sin, d_seq, d_pos, nrows, qbuf, kvq, l % h.n_layer,
                                         max_seq, max_ctx, stream);
            (void)tk_launch_attention_q8(qbuf, kvq, d_seq, d_pos, nrows, h.n_head, h.n_kv_head, h.head_dim, l % h.n_layer, max_seq, max_ctx, act_qd, nullptr, stream);
            return;
        }
        if (longf) {
            tk_launch_attention_long(partial, h.ks_qkv, QD + 2 * KVD, rope_cos, rope_sin, kcache, vcache, d_seq, d_pos, nrows, h.n_head, h.n_kv_head, h.head_dim, l % h.n_layer,
                                     max_seq, max_ctx, d_scores, act_qd, stream);
            return;
        }
        if (unfused)
            tk_launch_qkv_rope_append(partial, h.ks_qkv, QD + 2 * KVD, h.n_head, h.n_kv_head, h.head_dim, rope_cos, rope_sin, d_seq, d_pos, nrows, qbuf, kcache,
                                      vcache, l % h.n_layer, max_seq, max_ctx, stream);
        tk_launch_attention(qbuf, partial, h.ks_qkv, QD + 2 * KVD, rope_cos, rope_sin, kcache, vcache, d_seq, d_pos, nrows, h.n_head, h.n_kv_head,
                            h.head_dim, l % h.n_layer, max_seq, max_ctx, act_qd, !unfused, stream);
    };
    *kv_bytes = (double)nrows * ctx * KVD * 2.0 * 2.0;
    if (kv_type == TK_KV_Q8_0) *kv_bytes = (double)nrows * ctx * KVD * (34.0 / 32.0) * 3.0; /* keys twice, values once, 34 bytes per 32 elements */
    return time_launches(iters, [&] { launch(0); }, launch, avg_ms);
}
