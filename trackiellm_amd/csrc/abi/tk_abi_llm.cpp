/*
 * tk_abi_llm.cpp — tk_model_loader_* / tk_llm_runner_* (reference surface) and the
 * tk_mi355x_llm_* extension entry points on top of the HIP engine.
 *
 * Behaviour mirrored from the reference:
 *   loader: find-or-load by path, handle is an opaque pointer (src/ai_models/tk_model_loader.c:918-1083,
 *           tk_model_loader_private.h:43-51)
 *   runner: prepare = tokenise(add_bos) -> clear KV -> prefill whole prompt (tk_runner_streaming.c:20-34);
 *           next_token = sample -> EOS? NULL -> decode one token -> piece valid until next call (:57-85);
 *           add_tool_response formats "[TOOL_RESULT] name: \"%s\", output: %s [/TOOL_RESULT]" and decodes it
 *           at n_past (tk_runner_helpers.c:78-126); reset_context clears the KV state (:128-138).
 * There is no CPU fallback: every entry fails with a GPU error when no gfx950 device is usable.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../llm/tk_gguf.h"
#include "../llm/tk_grammar.h"
#include "../llm/tk_llm_batcher.h"
#include "../llm/tk_llm_engine.h"
#include "../llm/tk_lookup.h"
#include "../llm/tk_lookup_scope.h"
#include "../llm/tk_lora.h"
#include "../llm/tk_prefix_match.h"
#include "../llm/tk_llm_pipe.h"
#include "../llm/tk_tokenizer.h"
#include "../common/tk_ggml_blocks.h"
#include "tk/tk_mi355x_ext.h"
#include "tk/tk_model_runner.h"

struct tk_mi355x_llm_model_s {
    TkLlmModel model;
    TkTokenizer tok;
    int context_length = 4096;
    std::string path;
    std::unique_ptr<TkLoraAdapter> lora; /* the adapter merged into this model's matrices at load (tk_lora.h); part of the registry key */
    int refcount = 1;
    /* continuous batching behind tk_llm_runner_*: the runners created on this model share decode sessions (declared after `model`:
     * destroyed before it) */
    std::mutex batch_mu;
    std::vector<std::unique_ptr<TkLlmBatcher>> batchers;
    int runner_slots = 0; /* sequences per shared session; 0 = $TK_MI355X_RUNNER_SLOTS or 16 */
    int kv_cache_type = TK_KV_F16; /* tk_mi355x_llm_model_set_kv_cache_type: the cache type of the runners' shared sessions */
    bool prefix_cache = false; /* tk_mi355x_llm_model_set_prefix_cache: handed to every scheduler of the model, present and future */
};

struct tk_mi355x_llm_session_s {
    TkLlmSession session;
};

static tk_error_code_t fail(tk_error_code_t code, const std::string& why) {
    tk_error_set_detail("%s", why.c_str());
    return code;
}

static TkLlmHParams to_hp(const tk_mi355x_llm_hparams_t& h) {
    TkLlmHParams o{};
    o.n_layer = h.n_layer; o.d_model = h.d_model; o.n_head = h.n_head; o.n_kv_head = h.n_kv_head; o.head_dim = h.head_dim;
    o.d_ff = h.d_ff; o.vocab = h.vocab; o.rms_eps = h.rms_eps; o.rope_theta = h.rope_theta;
    o.ks_qkv = h.ks_qkv; o.ks_o = h.ks_o; o.ks_gateup = h.ks_gateup; o.ks_down = h.ks_down; o.ks_out = h.ks_out;
    return o;
}

/* K-split plan: at least one 64-row workgroup per CU (256) where the matrix allows it */
static void default_plan(tk_mi355x_llm_hparams_t* h) {
    auto pick = [](int64_t rows, int64_t K) {
        if (rows < 64 || K < 256) return 1; /* geometry the model rejects later (TkLlmModel::init): no plan to make */
        int nb = (int)(K / 256);
        int want = (int)((256 + rows / 64 - 1) / (rows / 64));
        int ks = 1;
        /* prefer K-ranges of a multiple of 4 blocks: the GEMV keeps 4 weight tiles in flight per wave */
        for (int c = 1; c <= nb && c <= 8; ++c) /* at most 8 K-ranges: the consumers keep every partial slab of a row in flight at once */
            if (nb % c == 0 && ((nb / c) % 4 == 0 || nb < 4 * want)) { ks = c; if (c >= want) break; }
        if (K / ks > 4096) { /* LDS image of the K-range must fit: 16 B per k */
            for (int c = ks; c <= nb; ++c) if (nb % c == 0 && K / c <= 4096) { ks = c; break; }
        }
        return ks;
    };
    const int64_t qd = (int64_t)h->n_head * h->head_dim, kvd = (int64_t)h->n_kv_head * h->head_dim;
    h->ks_qkv = pick(qd + 2 * kvd, h->d_model);
    h->ks_o = pick(h->d_model, qd);
    h->ks_gateup = pick(2 * (int64_t)h->d_ff, h->d_model);
    h->ks_down = pick(h->d_model, h->d_ff);
    h->ks_out = 1;
}

/* the host quantiser entries' one loop: x [n_blocks][the type's weights per block] -> n_blocks blocks (n_blocks counts the type's own blocks: 32 weights
 * for Q8_0, 256 for the k-quants) */
template <int T> static tk_error_code_t quantize_blocks_of(const float* x, int64_t n_blocks, void* out) {
    typedef TkBlock<T> B;
    if (!x || !out || n_blocks < 0) return TK_ERROR_INVALID_ARGUMENT;
    for (int64_t b = 0; b < n_blocks; ++b) B::quantize(x + B::elems * b, (typename B::block*)out + b);
    return TK_SUCCESS;
}

extern "C" {

tk_error_code_t tk_mi355x_llm_model_create(tk_mi355x_llm_model_t** out, const tk_mi355x_llm_hparams_t* hp, int device) {
    if (!out || !hp) return TK_ERROR_INVALID_ARGUMENT;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(TK_ERROR_GPU_DEVICE_NOT_FOUND, "no HIP device visible (the MI355X path has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(TK_ERROR_INVALID_ARGUMENT, "device ordinal out of range");
    tk_mi355x_llm_hparams_t h = *hp;
    if (h.ks_qkv <= 0 || h.ks_o <= 0 || h.ks_gateup <= 0 || h.ks_down <= 0) default_plan(&h);
    std::unique_ptr<tk_mi355x_llm_model_s> m(new tk_mi355x_llm_model_s());
    if (!m->model.init(to_hp(h), device)) return fail(TK_ERROR_MODEL_LOAD_FAILED, m->model.error);
    m->tok.init_bytes(h.vocab);
    *out = m.release();
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_model_fill_synthetic(tk_mi355x_llm_model_t* m, uint64_t seed) {
    if (!m) return TK_ERROR_INVALID_ARGUMENT;
    if (!m->model.fill_synthetic(seed)) return fail(TK_ERROR_GPU_ROCM_ERROR, m->model.error);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_gemv_probe(int device, int type, const void* blocks, int64_t rows, int64_t K, int ks, int nrows, const float* x,
                                         float* y) {
    if (!blocks || !x || !y) return TK_ERROR_INVALID_ARGUMENT;
    std::string err;
    if (!tk_llm_gemv_probe(device, type, blocks, rows, K, ks, nrows, x, y, err)) return fail(TK_ERROR_INVALID_ARGUMENT, err);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_step_probe(int device, tk_mi355x_llm_step_probe_t* p) {
    if (!p) return TK_ERROR_INVALID_ARGUMENT;
    std::string err;
    if (!tk_llm_step_probe(device, p, err)) return fail(err.find("device error") != std::string::npos || err.find("memory") != std::string::npos ? TK_ERROR_GPU_ROCM_ERROR : TK_ERROR_INVALID_ARGUMENT, err);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_repack_probe(int device, int type, const void* blocks, int64_t rows, int64_t K, void* tiles) {
    if (!blocks || !tiles) return TK_ERROR_INVALID_ARGUMENT;
    std::string err;
    if (!tk_llm_repack_probe(device, type, blocks, rows, K, tiles, err))
        return fail(err.find("device") != std::string::npos ? TK_ERROR_GPU_ROCM_ERROR : TK_ERROR_INVALID_ARGUMENT, err);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_quantize_blocks(int type, const float* x, int64_t n_blocks, void* out) {
    if (!tk_type_desc_of(type).host_quantize) return TK_ERROR_INVALID_ARGUMENT; /* a pinned set: every other type has an entry of its own below */
    tk_error_code_t rc = TK_ERROR_INVALID_ARGUMENT;
    tk_type_dispatch(type, [&](auto trait) { rc = quantize_blocks_of<decltype(trait)::type>(x, n_blocks, out); });
    return rc;
}

tk_error_code_t tk_mi355x_quantize_blocks_q2k(const float* x, int64_t n_blocks, void* out) { return quantize_blocks_of<TK_TYPE_Q2_K>(x, n_blocks, out); }
tk_error_code_t tk_mi355x_quantize_blocks_q4_0(const float* x, int64_t n_blocks, void* out) { return quantize_blocks_of<TK_TYPE_Q4_0>(x, n_blocks, out); }
tk_error_code_t tk_mi355x_quantize_blocks_q5_0(const float* x, int64_t n_blocks, void* out) { return quantize_blocks_of<TK_TYPE_Q5_0>(x, n_blocks, out); }
tk_error_code_t tk_mi355x_quantize_blocks_q4_1(const float* x, int64_t n_blocks, void* out) { return quantize_blocks_of<TK_TYPE_Q4_1>(x, n_blocks, out); }
tk_error_code_t tk_mi355x_quantize_blocks_q5_1(const float* x, int64_t n_blocks, void* out) { return quantize_blocks_of<TK_TYPE_Q5_1>(x, n_blocks, out); }
tk_error_code_t tk_mi355x_quantize_blocks_iq4_nl(const float* x, int64_t n_blocks, void* out) { return quantize_blocks_of<TK_TYPE_IQ4_NL>(x, n_blocks, out); }
tk_error_code_t tk_mi355x_quantize_blocks_iq4_xs(const float* x, int64_t n_blocks, void* out) { return quantize_blocks_of<TK_TYPE_IQ4_XS>(x, n_blocks, out); }
tk_error_code_t tk_mi355x_quantize_blocks_tq1_0(const float* x, int64_t n_blocks, void* out) { return quantize_blocks_of<TK_TYPE_TQ1_0>(x, n_blocks, out); }
tk_error_code_t tk_mi355x_quantize_blocks_tq2_0(const float* x, int64_t n_blocks, void* out) { return quantize_blocks_of<TK_TYPE_TQ2_0>(x, n_blocks, out); }

tk_error_code_t tk_mi355x_llm_model_fill_synthetic_ftype(tk_mi355x_llm_model_t* m, uint64_t seed, int ftype) {
    if (!m || !(ftype == 2 || ftype == 8 || ftype == 7 || ftype == 10 || ftype == 11 || ftype == 12 || (ftype >= 14 && ftype <= 17) || ftype == 21 || ftype == 25 || ftype == 30 || ftype == 36 || ftype == 37)) return TK_ERROR_INVALID_ARGUMENT;
    if (!m->model.fill_synthetic(seed, false, ftype)) return fail(TK_ERROR_GPU_ROCM_ERROR, m->model.error);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_model_fill_synthetic_type(tk_mi355x_llm_model_t* m, uint64_t seed, int ggml_type) {
    if (!m || !(ggml_type == TK_TYPE_Q4_1 || ggml_type == TK_TYPE_Q5_1)) return TK_ERROR_INVALID_ARGUMENT;
    if (!m->model.fill_synthetic_type(seed, ggml_type)) return fail(TK_ERROR_GPU_ROCM_ERROR, m->model.error);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_model_fill_synthetic_f16(tk_mi355x_llm_model_t* m, uint64_t seed) {
    if (!m) return TK_ERROR_INVALID_ARGUMENT;
    if (!m->model.fill_synthetic(seed, true)) return fail(TK_ERROR_GPU_ROCM_ERROR, m->model.error);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_model_fill_synthetic_float(tk_mi355x_llm_model_t* m, uint64_t seed, int ggml_type) {
    if (!m || !(ggml_type == TK_TYPE_BF16 || ggml_type == TK_TYPE_F32)) return TK_ERROR_INVALID_ARGUMENT;
    if (!m->model.fill_synthetic_float(seed, ggml_type)) return fail(TK_ERROR_GPU_ROCM_ERROR, m->model.error);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_convert_bf16(const float* x, int64_t n, uint16_t* out) {
    if (!x || !out || n < 0) return TK_ERROR_INVALID_ARGUMENT;
    for (int64_t i = 0; i < n; ++i) out[i] = tk_f32_to_bf16(x[i]);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_matmul_float_probe(int device, int type, const void* w, int64_t rows, int64_t K, int ks, int nseg, const int32_t seg_rows[3],
                                                 int nrows, const float* x, float* y) {
    if (!w || !seg_rows || !x || !y || !(type == TK_TYPE_F16 || type == TK_TYPE_BF16 || type == TK_TYPE_F32)) return TK_ERROR_INVALID_ARGUMENT;
    std::string err;
    if (!tk_llm_matmul_float_probe(device, type, w, rows, K, ks, nseg, seg_rows, nrows, x, y, err))
        return fail(err.find("needs") != std::string::npos ? TK_ERROR_INVALID_ARGUMENT : TK_ERROR_GPU_ROCM_ERROR, err);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_model_set_lora(tk_mi355x_llm_model_t* m, const char* adapter_path) {
    if (!m) return TK_ERROR_INVALID_ARGUMENT;
    if (!adapter_path || !*adapter_path) { m->model.lora = nullptr; m->lora.reset(); return TK_SUCCESS; }
    std::unique_ptr<TkLoraAdapter> ad(new TkLoraAdapter());
    if (!ad->load(adapter_path)) return fail(TK_ERROR_MODEL_LOAD_FAILED, "LoRA adapter: " + ad->error);
    const TkLlmHParams& hp = m->model.hp;
    for (const auto& t : ad->tensors) {
        int64_t rows = 0, cols = 0;
        if (t.layer >= hp.n_layer) return fail(TK_ERROR_MODEL_LOAD_FAILED, "LoRA adapter names a layer this model does not have");
        m->model.shape(t.layer, t.which, &rows, &cols);
        if (rows != t.n_out || cols != t.k_in) return fail(TK_ERROR_MODEL_LOAD_FAILED, "LoRA adapter does not fit this model (factor shapes against the base matrix)");
    }
    m->lora = std::move(ad);
    m->model.lora = m->lora.get();
    return TK_SUCCESS;
}

int tk_mi355x_llm_model_lora_merged(const tk_mi355x_llm_model_t* m) { return m ? m->model.lora_merged : 0; }

tk_error_code_t tk_mi355x_lora_probe(const char* path, int32_t* rank, float* alpha, int32_t* n_tensors) {
    if (!path) return TK_ERROR_INVALID_ARGUMENT;
    TkLoraAdapter ad;
    if (!ad.load(path)) return fail(TK_ERROR_FILE_CORRUPT, "LoRA adapter: " + ad.error);
    if (rank) *rank = ad.r;
    if (alpha) *alpha = ad.alpha;
    if (n_tensors) *n_tensors = (int32_t)ad.tensors.size();
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_model_set_tensor(tk_mi355x_llm_model_t* m, int layer, int which, int type, const void* data, size_t nbytes) {
    if (!m || !data) return TK_ERROR_INVALID_ARGUMENT;
    if (!m->model.set_tensor(layer, which, type, data, nbytes)) return fail(TK_ERROR_INVALID_INPUT_TENSOR, m->model.error);
    return TK_SUCCESS;
}

void tk_mi355x_llm_model_get_hparams(const tk_mi355x_llm_model_t* m, tk_mi355x_llm_hparams_t* out) {
    if (!m || !out) return;
    const TkLlmHParams& h = m->model.hp;
    *out = tk_mi355x_llm_hparams_t{h.n_layer, h.d_model, h.n_head, h.n_kv_head, h.head_dim, h.d_ff, h.vocab, h.rms_eps, h.rope_theta,
                                   h.ks_qkv, h.ks_o, h.ks_gateup, h.ks_down, h.ks_out};
}

/* the bytes a decode step streams: the matrices as they are installed.  A TQ1_0 matrix counts the TQ2_0 tile it is installed as, 66 bytes
 * per 256 weights where its file holds 54: the price of running the 2-bit kernels (a shift and a mask per four weights) in place of a
 * base-3 decode of several VALU operations per weight inside the W4A8 loops, which nobody has built or measured */
uint64_t tk_mi355x_llm_model_weight_bytes(const tk_mi355x_llm_model_t* m) {
    if (!m) return 0;
    uint64_t b = m->model.output.bytes;
    for (const auto& L : m->model.layers) b += L.q.bytes + L.k.bytes + L.v.bytes + L.o.bytes + L.gate.bytes + L.up.bytes + L.down.bytes;
    return b;
}

/* Weights are immutable and 4.3 GB: a model file resident on a device is shared by every loader of the process (the reference caches
 * per loader, src/ai_models/tk_model_loader.c:918-1083; K cortex handles — each with its own loader, tk_cortex_main.c:779-925 — would
 * otherwise hold K copies and could not share decode passes).  force_reload loads a private copy.
 * Lifetime: refcount = the creator / the loaders that hold the handle + every live tk_llm_runner_t created on it (a runner keeps raw
 * pointers into the model's shared decode sessions, so the model must outlive it whatever order the host destroys things in). */
static std::mutex g_models_mu;
static std::vector<tk_mi355x_llm_model_t*> g_models;

static void release_model(tk_mi355x_llm_model_t* m) { /* g_models_mu held */
    if (--m->refcount > 0) return;
    for (size_t i = 0; i < g_models.size(); ++i)
        if (g_models[i] == m) { g_models.erase(g_models.begin() + i); break; }
    delete m;
}

void tk_mi355x_llm_model_destroy(tk_mi355x_llm_model_t** m) {
    if (!m || !*m) return;
    {
        std::lock_guard<std::mutex> gl(g_models_mu);
        release_model(*m); /* freed once the last runner created on it is gone too */
    }
    *m = nullptr;
}

/* GGUF metadata only (no GPU): lets the loader report geometry errors before touching the device */
tk_error_code_t tk_mi355x_gguf_probe(const char* path, tk_mi355x_llm_hparams_t* out, int32_t* n_vocab_tokens) {
    if (!path || !out) return TK_ERROR_INVALID_ARGUMENT;
    TkGgufFile f;
    if (!f.open(path)) return fail(access(path, 0) == 0 ? TK_ERROR_FILE_CORRUPT : TK_ERROR_FILE_NOT_FOUND, f.error);
    auto it = f.str.find("general.architecture");
    std::string arch = it == f.str.end() ? "llama" : it->second;
    tk_mi355x_llm_hparams_t h{};
    h.n_layer = (int)f.get(arch + ".block_count", 0);
    h.d_model = (int)f.get(arch + ".embedding_length", 0);
    h.d_ff = (int)f.get(arch + ".feed_forward_length", 0);
    h.n_head = (int)f.get(arch + ".attention.head_count", 0);
    h.n_kv_head = (int)f.get(arch + ".attention.head_count_kv", h.n_head);
    h.head_dim = (int)f.get(arch + ".rope.dimension_count", h.n_head ? h.d_model / h.n_head : 0);
    h.rms_eps = (float)f.get(arch + ".attention.layer_norm_rms_epsilon", 1e-5);
    h.rope_theta = (float)f.get(arch + ".rope.freq_base", 10000.0);
    const TkGgufTensor* te = f.find("token_embd.weight");
    h.vocab = te && te->dims.size() == 2 ? (int)te->dims[1] : (int)f.tokens.size();
    if (h.n_layer <= 0 || h.d_model <= 0 || h.n_head <= 0 || h.vocab <= 0 || h.d_ff <= 0 || h.n_kv_head <= 0 || h.head_dim <= 0)
        return fail(TK_ERROR_MODEL_LOAD_FAILED, "GGUF lacks llama hyper-parameters");
    default_plan(&h);
    *out = h;
    if (n_vocab_tokens) *n_vocab_tokens = (int32_t)f.tokens.size();
    return TK_SUCCESS;
}

/* tokenises with the vocabulary stored in a GGUF file (CPU only; byte tokens when the file has no vocabulary) */
int tk_mi355x_gguf_tokenize(const char* path, const char* text, int add_bos, int32_t* ids, int cap) {
    if (!path || !text || !ids || cap <= 0) return -1;
    TkGgufFile f;
    if (!f.open(path)) { tk_error_set_detail("%s", f.error.c_str()); return -1; }
    TkTokenizer t;
    if (!f.tokens.empty()) t.init_spm(f.tokens, f.scores, f.token_type, (int)f.get("tokenizer.ggml.bos_token_id", 1), (int)f.get("tokenizer.ggml.eos_token_id", 2));
    else t.init_bytes(1 << 30);
    std::vector<int32_t> v = t.encode(text, add_bos != 0);
    for (size_t i = 0; i < v.size() && (int)i < cap; ++i) ids[i] = v[i];
    return (int)v.size();
}

tk_error_code_t tk_mi355x_llm_model_load_gguf(tk_mi355x_llm_model_t** out, const char* path, int device) {
    return tk_mi355x_llm_model_load_gguf_lora(out, path, nullptr, device);
}

tk_error_code_t tk_mi355x_llm_model_load_gguf_lora(tk_mi355x_llm_model_t** out, const char* path, const char* lora_path, int device) {
    if (!out || !path) return TK_ERROR_INVALID_ARGUMENT;
    tk_mi355x_llm_hparams_t h{};
    tk_error_code_t rc = tk_mi355x_gguf_probe(path, &h, nullptr);
    if (rc != TK_SUCCESS) return rc;
    TkGgufFile f;
    if (!f.open(path)) return fail(TK_ERROR_FILE_CORRUPT, f.error);
    tk_mi355x_llm_model_t* m = nullptr;
    rc = tk_mi355x_llm_model_create(&m, &h, device);
    if (rc != TK_SUCCESS) return rc;
    if (lora_path && *lora_path) {
        rc = tk_mi355x_llm_model_set_lora(m, lora_path);
        if (rc != TK_SUCCESS) { delete m; return rc; } /* private to this call, like the failure path below */
    }
    auto put = [&](int layer, int which, const std::string& name, const char* alt) -> bool {
        const TkGgufTensor* t = f.find(name);
        if (!t && alt) t = f.find(alt);
        if (!t) { tk_error_set_detail("GGUF tensor missing: %s", name.c_str()); return false; }
        if (!t->data) { tk_error_set_detail("GGUF tensor %s has unsupported type %u (supported: " TK_TYPE_NAMES ")", name.c_str(), t->type); return false; }
        if (!m->model.set_tensor(layer, which, (int)t->type, t->data, t->nbytes)) { tk_error_set_detail("%s: %s", name.c_str(), m->model.error.c_str()); return false; }
        return true;
    };
    bool ok = put(-1, TK_T_TOKEN_EMBD, "token_embd.weight", nullptr) && put(-1, TK_T_OUT_NORM, "output_norm.weight", nullptr) &&
              put(-1, TK_T_OUTPUT, "output.weight", "token_embd.weight");
    static const char* names[TK_L_COUNT] = {"attn_norm", "attn_q", "attn_k", "attn_v", "attn_output", "ffn_norm", "ffn_gate", "ffn_up", "ffn_down"};
    for (int l = 0; l < h.n_layer && ok; ++l)
        for (int w = 0; w < TK_L_COUNT && ok; ++w) {
            char nm[96];
            snprintf(nm, sizeof nm, "blk.%d.%s.weight", l, names[w]);
            ok = put(l, w, nm, nullptr);
        }
    /* `m` is private to this call (never registered, no runner holds it): freed directly.  NOT tk_mi355x_llm_model_destroy — that takes
     * g_models_mu, which tk_model_loader_load_model holds across this call (a GGUF with a missing tensor hung the loader) */
    if (!ok) { delete m; return TK_ERROR_MODEL_LOAD_FAILED; }
    if (m->lora) { m->model.lora = nullptr; m->lora->drop_factors(); } /* every matrix is installed: nothing reads the factors any more */
    if (!f.tokens.empty()) m->tok.init_spm(f.tokens, f.scores, f.token_type, (int)f.get("tokenizer.ggml.bos_token_id", 1), (int)f.get("tokenizer.ggml.eos_token_id", 2));
    auto it = f.str.find("general.architecture");
    m->context_length = (int)f.get((it == f.str.end() ? std::string("llama") : it->second) + ".context_length", 4096);
    m->path = path;
    *out = m;
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_session_create(tk_mi355x_llm_session_t** out, tk_mi355x_llm_model_t* m, int max_seq, int max_ctx) {
    if (!out || !m) return TK_ERROR_INVALID_ARGUMENT;
    std::unique_ptr<tk_mi355x_llm_session_s> s(new tk_mi355x_llm_session_s());
    if (!s->session.init(&m->model, max_seq, max_ctx)) return fail(TK_ERROR_GPU_MEMORY, s->session.error);
    *out = s.release();
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_session_create_kv(tk_mi355x_llm_session_t** out, tk_mi355x_llm_model_t* m, int max_seq, int max_ctx, int kv_type) {
    if (!out || !m) return TK_ERROR_INVALID_ARGUMENT;
    if (kv_type != TK_KV_F16 && kv_type != TK_KV_Q8_0) return fail(TK_ERROR_INVALID_ARGUMENT, "kv_type must be 0 (F16) or 1 (Q8_0)");
    std::unique_ptr<tk_mi355x_llm_session_s> s(new tk_mi355x_llm_session_s());
    if (!s->session.init(&m->model, max_seq, max_ctx, kv_type)) return fail(TK_ERROR_GPU_MEMORY, s->session.error);
    *out = s.release();
    return TK_SUCCESS;
}

int tk_mi355x_llm_session_kv_type(const tk_mi355x_llm_session_t* s) { return s ? s->session.kv_type : -1; }
uint64_t tk_mi355x_llm_session_kv_bytes(const tk_mi355x_llm_session_t* s) { return s ? (uint64_t)s->session.kv_bytes() : 0; }

tk_error_code_t tk_mi355x_llm_session_kv_read_q8(tk_mi355x_llm_session_t* s, int layer, int seq, int pos0, int n_pos, int8_t* kq, uint16_t* kd, int8_t* vq, uint16_t* vd) {
    if (!s || !kq || !kd || !vq || !vd) return TK_ERROR_INVALID_ARGUMENT;
    if (!s->session.kv_read_q8(layer, seq, pos0, n_pos, kq, kd, vq, vd)) return fail(TK_ERROR_INVALID_ARGUMENT, s->session.error);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_model_set_kv_cache_type(void* model_handle, int kv_type) {
    if (!model_handle) return TK_ERROR_INVALID_ARGUMENT;
    if (kv_type != TK_KV_F16 && kv_type != TK_KV_Q8_0) return fail(TK_ERROR_INVALID_ARGUMENT, "kv_type must be 0 (F16) or 1 (Q8_0)");
    tk_mi355x_llm_model_t* m = (tk_mi355x_llm_model_t*)model_handle;
    std::lock_guard<std::mutex> lk(m->batch_mu);
    if (!m->batchers.empty()) return fail(TK_ERROR_INVALID_ARGUMENT, "the KV cache type is set before the first tk_llm_runner_create on the model: its sessions exist already");
    m->kv_cache_type = kv_type;
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_model_set_kv_cache_type_by_name(void* model_handle, const char* name) {
    if (!model_handle || !name) return TK_ERROR_INVALID_ARGUMENT;
    if (strcmp(name, "f16") == 0) return tk_mi355x_llm_model_set_kv_cache_type(model_handle, TK_KV_F16);
    if (strcmp(name, "q8_0") == 0) return tk_mi355x_llm_model_set_kv_cache_type(model_handle, TK_KV_Q8_0);
    return fail(TK_ERROR_INVALID_ARGUMENT, std::string("KV cache type \"") + name + "\" is not built: f16 or q8_0");
}

tk_error_code_t tk_mi355x_attention_plan_kv(int device, int nrows, int n_head, int n_kv_head, int head_dim, int max_ctx, int fused, int kv_type, int32_t out[4]) {
    if (kv_type == TK_KV_F16) return tk_mi355x_attention_plan(device, nrows, n_head, n_kv_head, head_dim, max_ctx, fused, out);
    if (kv_type != TK_KV_Q8_0 || !out || nrows < 1 || nrows > TK_MAX_ROWS || n_head < 1 || n_kv_head < 1 || n_head % n_kv_head || head_dim < 1 || max_ctx < 1)
        return TK_ERROR_INVALID_ARGUMENT;
    if (device >= 0 && hipSetDevice(device) != hipSuccess) return fail(TK_ERROR_GPU_DEVICE_NOT_FOUND, "no such HIP device");
    const TkAttentionPlan pl = tk_attention_plan_q8(nrows, n_head, n_kv_head, head_dim);
    out[0] = pl.kernel; out[1] = pl.gq; out[2] = pl.chunk; out[3] = pl.slots;
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_kv_q8_probe(int device, const tk_mi355x_kv_q8_probe_t* p) {
    const int32_t cap = 1 << 16;
    if (!p || (p->mode != 0 && p->mode != 1) || !p->seq || !p->pos || !p->kq || !p->vq || !p->kd || !p->vd) return TK_ERROR_INVALID_ARGUMENT;
    if (p->n_layer < 1 || p->n_layer > cap || p->max_seq < 1 || p->max_seq > cap || p->n_kv_head < 1 || p->n_kv_head > cap || p->max_ctx < 1 || p->max_ctx > cap ||
        p->head_dim < 32 || p->head_dim > 256 || p->head_dim % 32 != 0 || p->layer < 0 || p->layer >= p->n_layer || p->nrows < 1 || p->nrows > TK_MAX_ROWS)
        return TK_ERROR_INVALID_ARGUMENT;
    const int64_t elems = (int64_t)p->n_layer * p->max_seq * p->n_kv_head * p->max_ctx * p->head_dim;
    if (elems > ((int64_t)1 << 31) || p->n_values < elems || p->n_scales < elems / TK_KV_Q8_BLOCK) return TK_ERROR_INVALID_ARGUMENT;
    for (int r = 0; r < p->nrows; ++r)
        if (p->seq[r] < 0 || p->seq[r] >= p->max_seq || p->pos[r] < 0 || p->pos[r] >= p->max_ctx) return TK_ERROR_INVALID_ARGUMENT;
    const int hd = p->head_dim, nb = hd / TK_KV_Q8_BLOCK;
    if (p->mode == 0) {
        if (!p->k16 || !p->v16 || p->n_rows_elems < (int64_t)p->nrows * p->n_kv_head * hd) return TK_ERROR_INVALID_ARGUMENT;
        for (int a = 0; a < p->nrows; ++a) /* two rows on one cache row: the launch would write it in no particular order */
            for (int b = a + 1; b < p->nrows; ++b)
                if (p->seq[a] == p->seq[b] && p->pos[a] == p->pos[b]) return TK_ERROR_INVALID_ARGUMENT;
    } else {
        if (!p->q || !p->out || p->n_head < 1 || p->n_head % p->n_kv_head) return TK_ERROR_INVALID_ARGUMENT;
        const int grp = p->n_head / p->n_kv_head;
        if ((grp != 1 && grp != 2 && grp != 4) || p->n_rows_elems < (int64_t)p->nrows * p->n_head * hd) return TK_ERROR_INVALID_ARGUMENT;
        /* the production launch takes a model's geometries only (TkLlmModel::init): whole 256-blocks of its Q8 activation image */
        if (device >= 0 && (hd % 64 != 0 || (grp * hd) % 256 != 0)) return TK_ERROR_INVALID_ARGUMENT;
    }
    if (device >= 0) {
        std::string err;
        if (!tk_llm_kv_q8_probe(device, p, err)) return fail(TK_ERROR_GPU_ROCM_ERROR, err);
        return TK_SUCCESS;
    }
    auto row_of = [&](int r, int kvh) { return (((size_t)p->layer * p->max_seq + p->seq[r]) * p->n_kv_head + kvh) * p->max_ctx; };
    if (p->mode == 0) {
        for (int r = 0; r < p->nrows; ++r)
            for (int kvh = 0; kvh < p->n_kv_head; ++kvh) {
                const size_t row = row_of(r, kvh) + p->pos[r], src = ((size_t)r * p->n_kv_head + kvh) * hd;
                tk_kv_q8_row(p->k16 + src, hd, p->kq + row * hd, p->kd + row * nb);
                tk_kv_q8_row(p->v16 + src, hd, p->vq + row * hd, p->vd + row * nb);
            }
        return TK_SUCCESS;
    }
    const int grp = p->n_head / p->n_kv_head;
    std::vector<float> scratch((size_t)p->max_ctx * grp);
    for (int r = 0; r < p->nrows; ++r)
        for (int kvh = 0; kvh < p->n_kv_head; ++kvh) {
            const size_t run = row_of(r, kvh), qo = ((size_t)r * p->n_head + (size_t)kvh * grp) * hd;
            tk_kv_q8_attention_row(p->q + qo, grp, hd, p->pos[r] + 1, p->kq + run * hd, p->kd + run * nb, p->vq + run * hd, p->vd + run * nb, scratch.data(), p->out + qo);
        }
    return TK_SUCCESS;
}

void tk_mi355x_llm_session_destroy(tk_mi355x_llm_session_t** s) {
    if (!s || !*s) return;
    delete *s;
    *s = nullptr;
}

tk_error_code_t tk_mi355x_llm_forward(tk_mi355x_llm_session_t* s, int nrows, const int32_t* seq, const int32_t* pos, const int32_t* tok,
                                      float* logits, int32_t* argmax) {
    if (!s || !seq || !pos || !tok) return TK_ERROR_INVALID_ARGUMENT;
    if (!s->session.forward(nrows, seq, pos, tok, logits, argmax, true)) return fail(TK_ERROR_INFERENCE_FAILED, s->session.error);
    return TK_SUCCESS;
}

/* a sampling pass with optional per-row sampling states and logit adjustments: both checked per row before anything runs */
static tk_error_code_t forward_rows(tk_mi355x_llm_session_t* s, int nrows, const int32_t* seq, const int32_t* pos, const int32_t* tok,
                                    const tk_mi355x_sampling_t* sampling, const tk_mi355x_logit_adjust_t* adjust, float* logits, int32_t* ids,
                                    const int32_t* n_top = nullptr, tk_mi355x_token_logprob_t* records = nullptr, const uint32_t* const* masks = nullptr) {
    static_assert(sizeof(tk_mi355x_token_logprob_t) == sizeof(TkTokenLogprob) && offsetof(tk_mi355x_token_logprob_t, top_ids) == offsetof(TkTokenLogprob, top_ids) &&
                      offsetof(tk_mi355x_token_logprob_t, top_logprobs) == offsetof(TkTokenLogprob, top_logprobs),
                  "the public log-probability record is the library's TkTokenLogprob");
    static_assert(sizeof(tk_mi355x_logit_adjust_t) == sizeof(TkLogitAdjust), "the public logit adjustment is the library's TkLogitAdjust (tk_rocm_hal.hip checks the fields)");
    if (!s || !seq || !pos || !tok || nrows < 1 || nrows > TK_MAX_ROWS) return TK_ERROR_INVALID_ARGUMENT;
    const TkLogitAdjust* adj = (const TkLogitAdjust*)adjust;
    for (int r = 0; r < nrows && adj; ++r)
        if (const char* why = adj[r].check(s->session.model->hp.vocab)) return fail(TK_ERROR_INVALID_ARGUMENT, "logit adjustment of row " + std::to_string(r) + ": " + why);
    for (int r = 0; r < nrows && n_top; ++r)
        if (const char* why = tk_logprob_check(n_top[r], s->session.model->hp.vocab)) return fail(TK_ERROR_INVALID_ARGUMENT, "log-probabilities of row " + std::to_string(r) + ": " + why);
    TkSampleRow rows[TK_MAX_ROWS] = {};
    for (int r = 0; r < nrows && sampling; ++r) {
        const tk_mi355x_sampling_t& p = sampling[r];
        /* the checks tk_mi355x_llm_runner_set_sampling makes, per row */
        if (!(p.temperature >= 0.0f) || p.top_k < 0 || p.top_k > TK_SAMPLE_MAX_K || !(p.top_p > 0.0f) || p.top_p > 1.0f || !(p.min_p >= 0.0f) || p.min_p > 1.0f)
            return fail(TK_ERROR_INVALID_ARGUMENT, "sampling parameters of row " + std::to_string(r) + " are out of range (temperature >= 0, 0 <= top_k <= 64, 0 < top_p <= 1, 0 <= min_p <= 1)");
        rows[r].temp = p.temperature; rows[r].top_p = p.top_p; rows[r].min_p = p.min_p; rows[r].top_k = p.top_k; rows[r].seed = p.seed; rows[r].counter = p.counter;
    }
    if (!s->session.forward(nrows, seq, pos, tok, logits, ids, true, masks, sampling ? rows : nullptr, adj, n_top, (TkTokenLogprob*)records))
        return fail(TK_ERROR_INFERENCE_FAILED, s->session.error);
    return TK_SUCCESS;
}

/* the head pass with all four per-row tables; the rows themselves are checked here too, so that a refusal is an argument error with nothing enqueued */
tk_error_code_t tk_mi355x_llm_forward_rows(tk_mi355x_llm_session_t* s, int nrows, const int32_t* seq, const int32_t* pos, const int32_t* tok,
                                           const uint32_t* const* masks, const tk_mi355x_sampling_t* sampling, const tk_mi355x_logit_adjust_t* adjust,
                                           const int32_t* n_top, float* logits, int32_t* picks, tk_mi355x_token_logprob_t* records) {
    if (!s || !seq || !pos || !tok || nrows < 1 || nrows > TK_MAX_ROWS) return TK_ERROR_INVALID_ARGUMENT;
    const TkLlmSession& ses = s->session;
    bool any_lp = false, any_drawn = false;
    for (int r = 0; r < nrows; ++r) {
        if (seq[r] < 0 || seq[r] >= ses.max_seq || pos[r] < 0 || pos[r] >= ses.max_ctx || tok[r] < 0 || tok[r] >= ses.model->hp.vocab)
            return fail(TK_ERROR_INVALID_ARGUMENT, "row " + std::to_string(r) + " is out of range (sequence id, position or token id)");
        any_lp = any_lp || (n_top && n_top[r] >= 0);
        any_drawn = any_drawn || (sampling && sampling[r].temperature > 0.0f);
    }
    if (any_lp && !records) return fail(TK_ERROR_INVALID_ARGUMENT, "log-probabilities asked for without records to fill");
    if (any_drawn && ses.model->hp.vocab > 65536) return fail(TK_ERROR_INVALID_ARGUMENT, "stochastic sampling supports vocabularies of at most 65536 tokens");
    return forward_rows(s, nrows, seq, pos, tok, sampling, adjust, logits, picks, n_top, records, masks);
}

tk_error_code_t tk_mi355x_llm_session_last_pass_key(tk_mi355x_llm_session_t* s, int* key) {
    if (!s || !key) return TK_ERROR_INVALID_ARGUMENT;
    *key = s->session.last_pass_key;
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_forward_logprobs(tk_mi355x_llm_session_t* s, int nrows, const int32_t* seq, const int32_t* pos, const int32_t* tok,
                                               const tk_mi355x_sampling_t* sampling, const tk_mi355x_logit_adjust_t* adjust, const int32_t* n_top,
                                               float* logits, int32_t* ids, tk_mi355x_token_logprob_t* records) {
    if (!n_top || !records) return TK_ERROR_INVALID_ARGUMENT;
    return forward_rows(s, nrows, seq, pos, tok, sampling, adjust, logits, ids, n_top, records);
}

tk_error_code_t tk_mi355x_llm_forward_sampled(tk_mi355x_llm_session_t* s, int nrows, const int32_t* seq, const int32_t* pos, const int32_t* tok,
                                              const tk_mi355x_sampling_t* sampling, float* logits, int32_t* ids) {
    if (!sampling) return TK_ERROR_INVALID_ARGUMENT;
    return forward_rows(s, nrows, seq, pos, tok, sampling, nullptr, logits, ids);
}

tk_error_code_t tk_mi355x_llm_forward_adjusted(tk_mi355x_llm_session_t* s, int nrows, const int32_t* seq, const int32_t* pos, const int32_t* tok,
                                               const tk_mi355x_sampling_t* sampling, const tk_mi355x_logit_adjust_t* adjust, float* logits, int32_t* ids) {
    if (!adjust) return TK_ERROR_INVALID_ARGUMENT;
    return forward_rows(s, nrows, seq, pos, tok, sampling, adjust, logits, ids);
}

tk_error_code_t tk_mi355x_llm_session_kv_write(tk_mi355x_llm_session_t* s, int layer, int seq, int pos0, int n_pos, const uint16_t* k, const uint16_t* v) {
    if (!s || !k || !v) return TK_ERROR_INVALID_ARGUMENT;
    if (!s->session.kv_write(layer, seq, pos0, n_pos, k, v)) return fail(TK_ERROR_INVALID_ARGUMENT, s->session.error);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_session_kv_read(tk_mi355x_llm_session_t* s, int layer, int seq, int pos0, int n_pos, uint16_t* k, uint16_t* v) {
    if (!s || !k || !v) return TK_ERROR_INVALID_ARGUMENT;
    if (!s->session.kv_read(layer, seq, pos0, n_pos, k, v)) return fail(TK_ERROR_INVALID_ARGUMENT, s->session.error);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_session_kv_copy(tk_mi355x_llm_session_t* s, int src_seq, int dst_seq, int pos0, int n_pos) {
    if (!s) return TK_ERROR_INVALID_ARGUMENT;
    if (!s->session.kv_copy_applies()) return fail(TK_ERROR_NOT_IMPLEMENTED, "kv_copy needs head_dim to be a multiple of 8");
    if (src_seq < 0 || src_seq >= s->session.max_seq || dst_seq < 0 || dst_seq >= s->session.max_seq || src_seq == dst_seq || pos0 < 0 || n_pos <= 0 ||
        n_pos > s->session.max_ctx - pos0)
        return fail(TK_ERROR_INVALID_ARGUMENT, "kv_copy: (source, destination, positions) outside the cache, or source = destination");
    if (!s->session.kv_copy(src_seq, dst_seq, pos0, n_pos)) return fail(TK_ERROR_GPU_ROCM_ERROR, s->session.error);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_session_kv_shift(tk_mi355x_llm_session_t* s, int seq, int p0, int p1, int delta) {
    if (!s) return TK_ERROR_INVALID_ARGUMENT;
    if (!s->session.kv_copy_applies()) return fail(TK_ERROR_NOT_IMPLEMENTED, "kv_shift needs head_dim to be a multiple of 8");
    if (s->session.kv_type == TK_KV_Q8_0) return fail(TK_ERROR_NOT_IMPLEMENTED, "kv_shift: re-rotating quantised keys is not built for a Q8_0 KV cache");
    bool bad_args = false;
    if (!s->session.kv_shift(seq, p0, p1, delta, &bad_args)) return fail(bad_args ? TK_ERROR_INVALID_ARGUMENT : TK_ERROR_GPU_ROCM_ERROR, s->session.error);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_time_kv_shift(tk_mi355x_llm_session_t* s, int seq, int p0, int p1, int delta, int iters, float* avg_ms, double* bytes) {
    if (!s || !avg_ms || !bytes) return TK_ERROR_INVALID_ARGUMENT;
    if (s->session.kv_type == TK_KV_Q8_0) return fail(TK_ERROR_NOT_IMPLEMENTED, "time_kv_shift: not built for a Q8_0 KV cache");
    if (!s->session.time_kv_shift(seq, p0, p1, delta, iters, avg_ms, bytes)) return fail(TK_ERROR_GPU_ROCM_ERROR, s->session.error);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_prefill(tk_mi355x_llm_session_t* s, int nseq, int n_prompt, const int32_t* tokens, int32_t* first_tokens) {
    if (!s || !tokens) return TK_ERROR_INVALID_ARGUMENT;
    if (!s->session.prefill(nseq, n_prompt, tokens, first_tokens)) return fail(TK_ERROR_INFERENCE_FAILED, s->session.error);
    return TK_SUCCESS;
}

int tk_mi355x_llm_max_rows(void) { return TK_MAX_ROWS; }

tk_error_code_t tk_mi355x_llm_forward_stage(tk_mi355x_llm_session_t* s, int nrows, const int32_t* seq, const int32_t* pos, const int32_t* tok,
                                            const float* x_in, float* x_out, int x_on_host, int layer0, int layer1, int head, int32_t* argmax) {
    if (!s || !seq || !pos) return TK_ERROR_INVALID_ARGUMENT;
    if (s->session.kv_type == TK_KV_Q8_0) return fail(TK_ERROR_NOT_IMPLEMENTED, "forward_stage: pipeline stages are not built for a Q8_0 KV cache");
    if (!s->session.forward_stage(nrows, seq, pos, tok, x_in, x_out, x_on_host != 0, layer0, layer1, head != 0, argmax))
        return fail(TK_ERROR_INFERENCE_FAILED, s->session.error);
    return TK_SUCCESS;
}

/* ---- layer-sharded pipeline with the hand-off inside the library (csrc/llm/tk_llm_pipe.h) ---- */
struct tk_mi355x_pipe_s { TkLlmPipe pipe; };
static_assert(sizeof(tk_mi355x_pipe_handle_t) == sizeof(TkPipeHandle), "public and internal pipe handles must have one layout");

tk_error_code_t tk_mi355x_pipe_create(tk_mi355x_pipe_t** out, tk_mi355x_llm_session_t* s, int stage, int n_stages, int layer0, int layer1, int payload_f16,
                                      tk_mi355x_pipe_handle_t* my_handle) {
    if (!out || !s) return TK_ERROR_INVALID_ARGUMENT;
    if (s->session.kv_type == TK_KV_Q8_0) return fail(TK_ERROR_NOT_IMPLEMENTED, "the layer-sharded pipeline is not built for a Q8_0 KV cache");
    std::unique_ptr<tk_mi355x_pipe_s> p(new tk_mi355x_pipe_s());
    if (!p->pipe.init(&s->session, stage, n_stages, layer0, layer1, payload_f16 != 0, (TkPipeHandle*)my_handle)) return fail(TK_ERROR_INVALID_ARGUMENT, p->pipe.error);
    *out = p.release();
    return TK_SUCCESS;
}

void tk_mi355x_pipe_destroy(tk_mi355x_pipe_t** p) {
    if (!p || !*p) return;
    delete *p;
    *p = nullptr;
}

tk_error_code_t tk_mi355x_pipe_connect(tk_mi355x_pipe_t* p, const tk_mi355x_pipe_handle_t* next, const tk_mi355x_pipe_handle_t* prev) {
    if (!p) return TK_ERROR_INVALID_ARGUMENT;
    if (!p->pipe.connect((const TkPipeHandle*)next, (const TkPipeHandle*)prev)) return fail(TK_ERROR_GPU_ROCM_ERROR, p->pipe.error);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_pipe_connect_local(tk_mi355x_pipe_t* p, tk_mi355x_pipe_t* next, tk_mi355x_pipe_t* prev) {
    if (!p) return TK_ERROR_INVALID_ARGUMENT;
    if (!p->pipe.connect_local(next ? &next->pipe : nullptr, prev ? &prev->pipe : nullptr)) return fail(TK_ERROR_GPU_ROCM_ERROR, p->pipe.error);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_pipe_rccl_unique_id(uint8_t out[128]) {
    if (!out) return TK_ERROR_INVALID_ARGUMENT;
    std::string err;
    if (!tk_pipe_rccl_unique_id(out, &err)) return fail(TK_ERROR_GPU_ROCM_ERROR, err);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_pipe_connect_rccl(tk_mi355x_pipe_t* p, const uint8_t unique_id[128]) {
    if (!p || !unique_id) return TK_ERROR_INVALID_ARGUMENT;
    if (!p->pipe.connect_rccl(unique_id)) return fail(TK_ERROR_GPU_DEVICE_NOT_FOUND, p->pipe.error);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_pipe_pass(tk_mi355x_pipe_t* p, int nrows, const int32_t* seq, const int32_t* pos, const int32_t* tok, int head) {
    if (!p || !seq || !pos) return TK_ERROR_INVALID_ARGUMENT;
    if (!p->pipe.pass(nrows, seq, pos, tok, head != 0)) return fail(TK_ERROR_INFERENCE_FAILED, p->pipe.error);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_pipe_decode(tk_mi355x_pipe_t* p, int nrows, int n_steps) {
    if (!p) return TK_ERROR_INVALID_ARGUMENT;
    if (!p->pipe.decode(nrows, n_steps)) return fail(TK_ERROR_INFERENCE_FAILED, p->pipe.error);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_pipe_sync(tk_mi355x_pipe_t* p, int32_t* out_tokens, int n_steps) {
    if (!p) return TK_ERROR_INVALID_ARGUMENT;
    if (!p->pipe.sync(out_tokens, n_steps)) return fail(TK_ERROR_TIMEOUT, p->pipe.error);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_decode(tk_mi355x_llm_session_t* s, int nrows, int n_steps, int32_t* out_tokens, float* ms_per_step) {
    if (!s) return TK_ERROR_INVALID_ARGUMENT;
    if (!s->session.decode(nrows, n_steps, out_tokens)) return fail(TK_ERROR_INFERENCE_FAILED, s->session.error);
    if (ms_per_step) *ms_per_step = s->session.last_step_ms;
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_time_gemv(tk_mi355x_llm_session_t* s, int layer, int which, int nrows, int iters, float* avg_ms,
                                        double* algorithmic_bytes) {
    if (!s || !avg_ms || !algorithmic_bytes || iters <= 0) return TK_ERROR_INVALID_ARGUMENT;
    if (!s->session.time_gemv(layer, which, nrows, iters, avg_ms, algorithmic_bytes)) return fail(TK_ERROR_GPU_ROCM_ERROR, s->session.error);
    return TK_SUCCESS;
}

int tk_mi355x_device_cu_count(int device) {
    int n = 0;
    return hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess ? n : -1;
}

tk_error_code_t tk_mi355x_attention_plan(int device, int nrows, int n_head, int n_kv_head, int head_dim, int max_ctx, int fused, int32_t out[4]) {
    if (!out || nrows < 1 || nrows > TK_MAX_ROWS || n_head < 1 || n_kv_head < 1 || n_head % n_kv_head || head_dim < 1 || max_ctx < 1) return TK_ERROR_INVALID_ARGUMENT;
    /* device < 0: none is selected — the answer is for the thread's current device, and for a 256-CU one on a host that has none */
    if (device >= 0 && hipSetDevice(device) != hipSuccess) return fail(TK_ERROR_GPU_DEVICE_NOT_FOUND, "no such HIP device");
    const TkAttentionPlan pl = tk_attention_plan(nrows, n_head, n_kv_head, head_dim, max_ctx, fused != 0);
    out[0] = pl.kernel; out[1] = pl.gq; out[2] = pl.chunk; out[3] = pl.slots;
    return TK_SUCCESS;
}

/* what a session of this geometry and window would know when it describes a pass of nrows rows (TkLlmSession::pass_caps) */
static TkPassCaps plan_caps(int nrows, int n_head, int n_kv_head, int head_dim, int max_ctx) {
    return TkPassCaps{max_ctx > TK_LONG_ATT_MIN_POS, tk_attention_prefill_applies(n_head, n_kv_head, head_dim), tk_attention_long_applies(nrows, n_head, n_kv_head, head_dim)};
}
/* the launcher's plan in out[] with the session's per-pass choice (tk_pass_form.h) on top; far: the per-row form of this window is
 * k_attention_far (kernel 5), which is what a pass runs where the choice says 0 */
static void plan_set_kernel(int32_t out[4], int kernel, int n_head, int n_kv_head, bool far) {
    if (kernel == 3 || kernel == 4) { out[1] = n_head / n_kv_head; out[2] = 64; out[3] = 1; }
    out[0] = kernel == 0 && far ? 5 : kernel;
}
static bool plan_is_far(int nrows, int n_head, int n_kv_head, int head_dim, int max_ctx) { return tk_attention_plan(nrows, n_head, n_kv_head, head_dim, max_ctx, true).far; }

int tk_mi355x_attention_resident_limit(int n_head, int n_kv_head, int head_dim) { return tk_attention_resident_limit(n_head, n_kv_head, head_dim); }

tk_error_code_t tk_mi355x_attention_plan_at(int device, int nrows, int n_head, int n_kv_head, int head_dim, int max_ctx, int fused, int top_position, int32_t out[4]) {
    const tk_error_code_t rc = tk_mi355x_attention_plan(device, nrows, n_head, n_kv_head, head_dim, max_ctx, fused, out);
    if (rc != TK_SUCCESS) return rc;
    if (top_position < 0 || top_position >= max_ctx) return TK_ERROR_INVALID_ARGUMENT;
    plan_set_kernel(out, tk_plan_kernel_at(out[0], fused != 0, nrows, top_position, plan_caps(nrows, n_head, n_kv_head, head_dim, max_ctx)), n_head, n_kv_head,
                    plan_is_far(nrows, n_head, n_kv_head, head_dim, max_ctx));
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_attention_plan_verify(int device, int nrows, int n_head, int n_kv_head, int head_dim, int max_ctx, int top_position, int32_t out[4]) {
    const tk_error_code_t rc = tk_mi355x_attention_plan(device, nrows, n_head, n_kv_head, head_dim, max_ctx, 0, out);
    if (rc != TK_SUCCESS) return rc;
    if (top_position < 0 || top_position >= max_ctx) return TK_ERROR_INVALID_ARGUMENT;
    plan_set_kernel(out, tk_plan_kernel_verify(out[0], nrows, top_position, plan_caps(nrows, n_head, n_kv_head, head_dim, max_ctx)), n_head, n_kv_head,
                    plan_is_far(nrows, n_head, n_kv_head, head_dim, max_ctx));
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_session_graph_captures(tk_mi355x_llm_session_t* s, uint64_t* n) {
    if (!s || !n) return TK_ERROR_INVALID_ARGUMENT;
    *n = s->session.n_captures;
    return TK_SUCCESS;
}

int tk_mi355x_lookup_draft(const int32_t* ctx, int n_ctx, const int32_t* pred, int n_pred, int ngram_min, int ngram_max, int n_draft, int32_t* out) {
    return tk_lookup_draft(ctx, n_ctx, pred, n_pred, ngram_min, ngram_max, n_draft, out);
}

int tk_mi355x_lookup_accept(const int32_t* toks, const int32_t* picks, int n, int32_t eos, int32_t* out_ids) { return tk_lookup_accept(toks, picks, n, eos, out_ids); }

tk_error_code_t tk_mi355x_llm_forward_verify(tk_mi355x_llm_session_t* s, int nrows, const int32_t* seq, const int32_t* pos, const int32_t* tok, int form,
                                             float* logits, int32_t* picks) {
    if (!s || !seq || !pos || !tok) return TK_ERROR_INVALID_ARGUMENT;
    bool bad_args = false;
    if (!s->session.forward_verify(nrows, seq, pos, tok, form, logits, picks, &bad_args))
        return fail(bad_args ? TK_ERROR_INVALID_ARGUMENT : TK_ERROR_INFERENCE_FAILED, s->session.error);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_time_attention(tk_mi355x_llm_session_t* s, int nrows, int ctx, int iters, float* avg_ms, double* kv_bytes) {
    if (!s || !avg_ms || !kv_bytes) return TK_ERROR_INVALID_ARGUMENT;
    if (!s->session.time_attention(nrows, ctx, iters, avg_ms, kv_bytes)) return fail(TK_ERROR_GPU_ROCM_ERROR, s->session.error);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_time_kv_copy(tk_mi355x_llm_session_t* s, int n_pos, int n_dst, int iters, float* kernel_ms, float* memcpy_ms, double* bytes) {
    if (!s || !kernel_ms || !memcpy_ms || !bytes) return TK_ERROR_INVALID_ARGUMENT;
    if (s->session.kv_type == TK_KV_Q8_0) return fail(TK_ERROR_NOT_IMPLEMENTED, "time_kv_copy: not built for a Q8_0 KV cache");
    if (!s->session.time_kv_copy(n_pos, n_dst, iters, kernel_ms, memcpy_ms, bytes)) return fail(TK_ERROR_GPU_ROCM_ERROR, s->session.error);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_model_set_runner_slots(void* model_handle, int slots) {
    if (!model_handle || slots < 1 || slots > TK_MAX_ROWS) return TK_ERROR_INVALID_ARGUMENT;
    tk_mi355x_llm_model_t* m = (tk_mi355x_llm_model_t*)model_handle;
    std::lock_guard<std::mutex> lk(m->batch_mu);
    m->runner_slots = slots;
    return TK_SUCCESS;
}

void tk_mi355x_llm_model_batch_stats(void* model_handle, uint64_t* passes, uint64_t* rows, int32_t* max_rows_in_a_pass) {
    uint64_t p = 0, r = 0;
    int mx = 0;
    if (model_handle) {
        tk_mi355x_llm_model_t* m = (tk_mi355x_llm_model_t*)model_handle;
        std::lock_guard<std::mutex> lk(m->batch_mu);
        for (auto& b : m->batchers) {
            uint64_t bp, br;
            int bm;
            b->stats(&bp, &br, &bm);
            p += bp; r += br; mx = bm > mx ? bm : mx;
        }
    }
    if (passes) *passes = p;
    if (rows) *rows = r;
    if (max_rows_in_a_pass) *max_rows_in_a_pass = mx;
}

tk_error_code_t tk_mi355x_llm_model_set_prefix_cache(void* model_handle, int on) {
    if (!model_handle || (on != 0 && on != 1)) return TK_ERROR_INVALID_ARGUMENT;
    tk_mi355x_llm_model_t* m = (tk_mi355x_llm_model_t*)model_handle;
    if (on && m->model.hp.head_dim % 8 != 0) return fail(TK_ERROR_NOT_IMPLEMENTED, "the prefix cache copies rows in 16-byte words: head_dim must be a multiple of 8");
    std::lock_guard<std::mutex> lk(m->batch_mu);
    m->prefix_cache = on != 0;
    for (auto& b : m->batchers) (void)b->set_prefix_cache(on != 0);
    return TK_SUCCESS;
}

void tk_mi355x_llm_model_prefix_cache_stats(void* model_handle, uint64_t* prompt_rows, uint64_t* kept, uint64_t* copied, uint64_t* copy_launches) {
    uint64_t t[4] = {0, 0, 0, 0};
    if (model_handle) {
        tk_mi355x_llm_model_t* m = (tk_mi355x_llm_model_t*)model_handle;
        std::lock_guard<std::mutex> lk(m->batch_mu);
        for (auto& b : m->batchers) {
            uint64_t v[4] = {0, 0, 0, 0};
            b->prefix_stats(&v[0], &v[1], &v[2], &v[3]);
            for (int i = 0; i < 4; ++i) t[i] += v[i];
        }
    }
    if (prompt_rows) *prompt_rows = t[0];
    if (kept) *kept = t[1];
    if (copied) *copied = t[2];
    if (copy_launches) *copy_launches = t[3];
}

int tk_mi355x_prefix_match(const int32_t* toks, int n, const int32_t* records, const int32_t* record_len, int n_slots, int stride, int self_slot, int cursor,
                           int32_t out[3]) {
    if (!toks || n < 1 || !records || !record_len || n_slots < 1 || n_slots > TK_MAX_ROWS || stride < 0 || self_slot < -1 || self_slot >= n_slots || cursor < -1 || !out) return -1;
    const int32_t* recs[TK_MAX_ROWS];
    int lens[TK_MAX_ROWS];
    for (int s = 0; s < n_slots; ++s) {
        if (record_len[s] < 0 || record_len[s] > stride) return -1;
        recs[s] = records + (size_t)s * stride;
        lens[s] = record_len[s];
    }
    out[0] = self_slot >= 0 ? tk_prefix_common(toks, n, recs[self_slot], lens[self_slot]) : 0;
    if (cursor < 0) cursor = out[0];
    int match = cursor;
    out[1] = tk_prefix_best_donor(toks, n, recs, lens, n_slots, self_slot, cursor, nullptr, &match);
    out[2] = match;
    return 0;
}

uint64_t tk_mi355x_llm_model_run_ahead_wasted(void* model_handle) {
    uint64_t w = 0;
    if (model_handle) {
        tk_mi355x_llm_model_t* m = (tk_mi355x_llm_model_t*)model_handle;
        std::lock_guard<std::mutex> lk(m->batch_mu);
        for (auto& b : m->batchers) {
            uint64_t bw = 0;
            b->stats(nullptr, nullptr, nullptr, &bw);
            w += bw;
        }
    }
    return w;
}

/* grammar engine entry points (no GPU involved): used by the CPU tests and by hosts that want the tool-call text */
tk_error_code_t tk_mi355x_grammar_check(const char* gbnf, const char* text, int32_t* n_accepted, int32_t* complete) {
    if (!text || !n_accepted || !complete) return TK_ERROR_INVALID_ARGUMENT;
    TkGrammar g;
    std::string err;
    if (!g.parse(gbnf ? gbnf : TK_DEFAULT_TOOL_CALL_GBNF, &err)) return fail(TK_ERROR_CONFIG_PARSE_FAILED, "GBNF: " + err);
    TkGrammarState st;
    st.init(&g);
    int32_t n = 0;
    for (const char* c = text; *c; ++c, ++n)
        if (!st.accept((uint8_t)*c)) break;
    *n_accepted = n;
    *complete = st.complete() ? 1 : 0;
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_grammar_next_bytes(const char* gbnf, const char* prefix, uint8_t allowed[256], int32_t* complete) {
    if (!prefix || !allowed || !complete) return TK_ERROR_INVALID_ARGUMENT;
    TkGrammar g;
    std::string err;
    if (!g.parse(gbnf ? gbnf : TK_DEFAULT_TOOL_CALL_GBNF, &err)) return fail(TK_ERROR_CONFIG_PARSE_FAILED, "GBNF: " + err);
    TkGrammarState st;
    st.init(&g);
    if (!st.accept(std::string(prefix))) return fail(TK_ERROR_INVALID_ARGUMENT, "prefix is not in the grammar");
    for (int b = 0; b < 256; ++b) {
        TkGrammarState t = st;
        allowed[b] = t.accept((uint8_t)b) ? 1 : 0;
    }
    *complete = st.complete() ? 1 : 0;
    return TK_SUCCESS;
}

/* k_grammar_mask alone on host arrays (include/tk/tk_mi355x_ext.h): everything is validated, and every state exported, before a device is touched */
tk_error_code_t tk_mi355x_grammar_mask_probe(int device, const char* gbnf, int32_t n_rows, const char* const* prefixes, const uint8_t* pieces, const uint32_t* offsets,
                                             int32_t vocab, int32_t eos, uint32_t* bits, int32_t* undecided) {
    if (!prefixes || !pieces || !offsets || !bits || !undecided || n_rows < 1 || n_rows > TK_MAX_ROWS || vocab < 1 || vocab > (1 << 20) || eos < -1 || eos >= vocab)
        return TK_ERROR_INVALID_ARGUMENT;
    if (offsets[0] != 0) return fail(TK_ERROR_INVALID_ARGUMENT, "grammar mask: offsets start at 0");
    for (int32_t t = 0; t < vocab; ++t)
        if (offsets[t + 1] < offsets[t] || offsets[t + 1] > (1u << 26)) return fail(TK_ERROR_INVALID_ARGUMENT, "grammar mask: offsets ascend and stay below 2^26");
    TkGrammar g;
    std::string err;
    if (!g.parse(gbnf ? gbnf : TK_DEFAULT_TOOL_CALL_GBNF, &err)) return fail(TK_ERROR_CONFIG_PARSE_FAILED, "GBNF: " + err);
    TkGrammarImage gi;
    if (!g.flatten(&gi)) return fail(TK_ERROR_INVALID_ARGUMENT, "grammar mask: the grammar has too many elements for an image");
    std::vector<TkGrammarStateImage> states;
    std::vector<int32_t> live;
    for (int32_t r = 0; r < n_rows; ++r) {
        if (!prefixes[r]) continue; /* the row is off: its bits and its count stay as the caller left them */
        TkGrammarState st;
        st.init(&g);
        TkGrammarStateImage img;
        if (!st.accept(std::string(prefixes[r]))) return fail(TK_ERROR_INVALID_ARGUMENT, "grammar mask: prefix " + std::to_string(r) + " is not in the grammar");
        if (!st.export_image(&img)) return fail(TK_ERROR_INVALID_ARGUMENT, "grammar mask: the state after prefix " + std::to_string(r) + " does not fit the image's caps");
        img.mask_row = r;
        img.grammar = 0;
        states.push_back(img);
        live.push_back(r);
    }
    const size_t words = ((size_t)vocab + 31) / 32;
    if (states.empty()) return TK_SUCCESS;
    if (device < 0) {
        for (size_t i = 0; i < states.size(); ++i) undecided[live[i]] = tk_grammar_mask_row(gi, states[i], offsets, pieces, vocab, eos, bits + (size_t)live[i] * words);
        return TK_SUCCESS;
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return TK_ERROR_GPU_DEVICE_NOT_FOUND;
    if (device >= n || hipSetDevice(device) != hipSuccess) return TK_ERROR_INVALID_ARGUMENT;
    const std::vector<uint32_t>& gw = g.flat_words();
    std::vector<int32_t> und(states.size(), 0);
    const uint8_t none = 0;
    struct Buf { const void* host; size_t bytes; void* dev; };
    enum { WORDS, STATES, OFFSETS, PIECES, BITS, UND, ARENA };
    Buf b[] = {{gw.data(), gw.size() * 4, nullptr}, {states.data(), states.size() * sizeof(TkGrammarStateImage), nullptr}, {offsets, ((size_t)vocab + 1) * 4, nullptr},
               {offsets[vocab] ? pieces : &none, offsets[vocab] ? (size_t)offsets[vocab] : 1, nullptr}, {bits, (size_t)n_rows * words * 4, nullptr}, {und.data(), und.size() * 4, nullptr},
               {nullptr, sizeof(TkGrammarImage), nullptr}};
    bool ok = true;
    for (Buf& q : b) ok = ok && hipMalloc(&q.dev, q.bytes) == hipSuccess && (!q.host || hipMemcpy(q.dev, q.host, q.bytes, hipMemcpyHostToDevice) == hipSuccess);
    TkGrammarImage di;
    TkGrammar::image_over((const uint32_t*)b[WORDS].dev, gi.n_rules, gi.n_elems, gi.n_sets, gi.root, &di);
    ok = ok && hipMemcpy(b[ARENA].dev, &di, sizeof di, hipMemcpyHostToDevice) == hipSuccess;
    tk_error_code_t rc = ok ? TK_SUCCESS : TK_ERROR_GPU_ROCM_ERROR;
    if (ok) {
        tk_launch_grammar_mask((const TkGrammarImage*)b[ARENA].dev, (const TkGrammarStateImage*)b[STATES].dev, (int)states.size(), (const uint32_t*)b[OFFSETS].dev,
                               (const uint8_t*)b[PIECES].dev, vocab, eos, (uint32_t*)b[BITS].dev, (int32_t*)b[UND].dev, nullptr);
        if (hipGetLastError() != hipSuccess) rc = TK_ERROR_GPU_KERNEL_LAUNCH;
        else if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(bits, b[BITS].dev, b[BITS].bytes, hipMemcpyDeviceToHost) != hipSuccess ||
                 hipMemcpy(und.data(), b[UND].dev, b[UND].bytes, hipMemcpyDeviceToHost) != hipSuccess)
            rc = TK_ERROR_GPU_ROCM_ERROR;
        else
            for (size_t i = 0; i < states.size(); ++i) undecided[live[i]] = und[i];
    }
    for (Buf& q : b) if (q.dev) (void)hipFree(q.dev);
    return rc;
}

/* the launch and the host call it replaces, timed side by side (tools/time_grammar_mask.py): the tool-call grammar (gbnf NULL) after `prefix`, n_rows
 * equal rows over the given vocabulary.  device_ms: the state upload plus the launch, `iters` times between two events after one untimed round, the
 * average of one; host_ms: TkGrammarState::mask over a trie of the same pieces, the average of min(iters, 20) calls for ONE row */
tk_error_code_t tk_mi355x_time_grammar_mask(int device, const char* gbnf, const char* prefix, int32_t n_rows, const uint8_t* pieces, const uint32_t* offsets, int32_t vocab,
                                            int32_t eos, int32_t iters, float* device_ms, float* host_ms) {
    if (!prefix || !pieces || !offsets || !device_ms || !host_ms || n_rows < 1 || n_rows > TK_MAX_ROWS || vocab < 1 || vocab > (1 << 20) || eos < -1 || eos >= vocab || iters < 1 ||
        iters > 100000 || offsets[0] != 0)
        return TK_ERROR_INVALID_ARGUMENT;
    for (int32_t t = 0; t < vocab; ++t)
        if (offsets[t + 1] < offsets[t] || offsets[t + 1] > (1u << 26)) return TK_ERROR_INVALID_ARGUMENT;
    TkGrammar g;
    std::string err;
    if (!g.parse(gbnf ? gbnf : TK_DEFAULT_TOOL_CALL_GBNF, &err)) return fail(TK_ERROR_CONFIG_PARSE_FAILED, "GBNF: " + err);
    TkGrammarImage gi;
    TkGrammarState st;
    st.init(&g);
    TkGrammarStateImage img;
    if (!g.flatten(&gi) || !st.accept(std::string(prefix)) || !st.export_image(&img)) return fail(TK_ERROR_INVALID_ARGUMENT, "grammar mask timing: no image for this grammar and prefix");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return TK_ERROR_GPU_DEVICE_NOT_FOUND;
    if (device < 0 || device >= n || hipSetDevice(device) != hipSuccess) return TK_ERROR_INVALID_ARGUMENT;
    {   /* the host call */
        std::vector<std::string> pcs((size_t)vocab);
        for (int32_t t = 0; t < vocab; ++t) if (t != eos) pcs[(size_t)t].assign((const char*)pieces + offsets[t], offsets[t + 1] - offsets[t]);
        TkTokenTrie trie;
        trie.build(pcs);
        std::vector<uint32_t> hb;
        st.mask(trie, eos, &hb);
        const int reps = iters < 20 ? iters : 20;
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < reps; ++i) st.mask(trie, eos, &hb);
        *host_ms = (float)(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / reps);
    }
    const size_t words = ((size_t)vocab + 31) / 32;
    const std::vector<uint32_t>& gw = g.flat_words();
    void *d_words = nullptr, *d_states = nullptr, *d_off = nullptr, *d_pieces = nullptr, *d_bits = nullptr, *d_und = nullptr, *d_arena = nullptr;
    TkGrammarStateImage* h_states = nullptr;
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool ok = hipMalloc(&d_words, gw.size() * 4) == hipSuccess && hipMalloc(&d_states, (size_t)n_rows * sizeof img) == hipSuccess && hipMalloc(&d_off, ((size_t)vocab + 1) * 4) == hipSuccess &&
              hipMalloc(&d_pieces, (size_t)offsets[vocab] + 1) == hipSuccess && hipMalloc(&d_bits, (size_t)n_rows * words * 4) == hipSuccess && hipMalloc(&d_und, (size_t)n_rows * 4) == hipSuccess &&
              hipMalloc(&d_arena, sizeof(TkGrammarImage)) == hipSuccess && hipHostMalloc((void**)&h_states, (size_t)n_rows * sizeof img, hipHostMallocDefault) == hipSuccess &&
              hipMemcpy(d_words, gw.data(), gw.size() * 4, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d_off, offsets, ((size_t)vocab + 1) * 4, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d_pieces, pieces, offsets[vocab], hipMemcpyHostToDevice) == hipSuccess && hipStreamCreate(&s) == hipSuccess && hipEventCreate(&e0) == hipSuccess &&
              hipEventCreate(&e1) == hipSuccess;
    TkGrammarImage di;
    TkGrammar::image_over((const uint32_t*)d_words, gi.n_rules, gi.n_elems, gi.n_sets, gi.root, &di);
    ok = ok && hipMemcpy(d_arena, &di, sizeof di, hipMemcpyHostToDevice) == hipSuccess;
    tk_error_code_t rc = ok ? TK_SUCCESS : TK_ERROR_GPU_ROCM_ERROR;
    if (ok) {
        img.grammar = 0;
        for (int r = 0; r < n_rows; ++r) { h_states[r] = img; h_states[r].mask_row = r; }
        auto round = [&] { /* what TkLlmSession::forward enqueues for its device rows */
            (void)hipMemcpyAsync(d_states, h_states, (size_t)n_rows * sizeof img, hipMemcpyHostToDevice, s);
            (void)hipMemsetAsync(d_und, 0, (size_t)n_rows * 4, s);
            tk_launch_grammar_mask((const TkGrammarImage*)d_arena, (const TkGrammarStateImage*)d_states, n_rows, (const uint32_t*)d_off, (const uint8_t*)d_pieces, vocab, eos,
                                   (uint32_t*)d_bits, (int32_t*)d_und, s);
        };
        round();
        (void)hipEventRecord(e0, s);
        for (int i = 0; i < iters; ++i) round();
        (void)hipEventRecord(e1, s);
        float ms = 0.0f;
        if (hipGetLastError() != hipSuccess) rc = TK_ERROR_GPU_KERNEL_LAUNCH;
        else if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) rc = TK_ERROR_GPU_ROCM_ERROR;
        else *device_ms = ms / (float)iters;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (s) (void)hipStreamDestroy(s);
    if (h_states) (void)hipHostFree(h_states);
    void* ptrs[] = {d_words, d_states, d_off, d_pieces, d_bits, d_und, d_arena};
    for (void* q : ptrs) if (q) (void)hipFree(q);
    return rc;
}

/* ------------------------------------------------------------------ reference surface ------ */

struct tk_model_loader_s {
    std::mutex mu;
    std::vector<tk_mi355x_llm_model_t*> held; /* one entry per successful load_model: the references this loader owns */
    uint32_t max_models = 4;
};

static size_t distinct_held(const tk_model_loader_s* l) {
    size_t n = 0;
    for (size_t i = 0; i < l->held.size(); ++i) {
        bool seen = false;
        for (size_t j = 0; j < i; ++j) seen = seen || l->held[j] == l->held[i];
        n += seen ? 0 : 1;
    }
    return n;
}

tk_error_code_t tk_model_loader_create(tk_model_loader_t** out_loader, const tk_model_loader_config_t* config) {
    if (!out_loader || !config) return TK_ERROR_INVALID_ARGUMENT;
    tk_model_loader_s* l = new tk_model_loader_s();
    l->max_models = config->max_models ? config->max_models : 4;
    *out_loader = l;
    return TK_SUCCESS;
}

void tk_model_loader_destroy(tk_model_loader_t** loader) {
    if (!loader || !*loader) return;
    {
        std::lock_guard<std::mutex> gl(g_models_mu);
        for (auto* m : (*loader)->held) release_model(m);
    }
    delete *loader;
    *loader = nullptr;
}

static bool parse_synthetic(const std::string& p, std::string* name, uint64_t* seed) {
    const std::string pre = "synthetic://";
    if (p.compare(0, pre.size(), pre) != 0) return false;
    std::string rest = p.substr(pre.size());
    *seed = 4;
    size_t q = rest.find('?');
    *name = rest.substr(0, q);
    if (q != std::string::npos) {
        size_t s = rest.find("seed=", q);
        if (s != std::string::npos) *seed = strtoull(rest.c_str() + s + 5, nullptr, 10);
    }
    return true;
}

tk_error_code_t tk_model_loader_load_model(tk_model_loader_t* loader, const tk_model_load_params_t* params, void** out_model_handle) {
    if (!loader || !params || !out_model_handle || !params->model_path || !params->model_path->path_str) return TK_ERROR_INVALID_ARGUMENT;
    if (params->model_type == TK_MODEL_FORMAT_ONNX) return fail(TK_ERROR_NOT_IMPLEMENTED, "ONNX graphs are not interpreted: the detector/ASR/VAD streams have dedicated entry points");
    std::lock_guard<std::mutex> lk(loader->mu);
    std::lock_guard<std::mutex> gl(g_models_mu); /* also serialises loads: two threads asking for the same file get one copy */
    const std::string lora = params->lora_adapter ? params->lora_adapter : "";
    /* the registry's key: a model with an adapter merged in (tk_model_loader.c:259-270) is another model than the file alone */
    const std::string path = std::string(params->model_path->path_str) + (lora.empty() ? "" : "\n+lora=" + lora);
    const std::string file = params->model_path->path_str;
    const int device = tk_mi355x_get_default_device();
    if (!params->force_reload)
        for (auto* m : g_models)
            if (m->path == path && m->model.device == device) {
                bool mine = false;
                for (auto* h : loader->held) mine = mine || h == m;
                if (!mine && distinct_held(loader) >= loader->max_models) return fail(TK_ERROR_OUT_OF_MEMORY, "model cache full (max_models)");
                m->refcount++;
                loader->held.push_back(m);
                *out_model_handle = m;
                return TK_SUCCESS;
            }
    if (distinct_held(loader) >= loader->max_models) return fail(TK_ERROR_OUT_OF_MEMORY, "model cache full (max_models)");
    tk_mi355x_llm_model_t* m = nullptr;
    std::string name;
    uint64_t seed;
    tk_error_code_t rc;
    if (parse_synthetic(file, &name, &seed)) {
        tk_mi355x_llm_hparams_t h{};
        /* the float recipes of fill_synthetic_float, parsed before -f16 (which "-bf16" also ends in): synthetic://mistral-7b-bf16, synthetic://tiny-f32 */
        int flt = -1;
        if (name.size() > 5 && name.compare(name.size() - 5, 5, "-bf16") == 0) { flt = TK_TYPE_BF16; name.resize(name.size() - 5); }
        else if (name.size() > 4 && name.compare(name.size() - 4, 4, "-f32") == 0) { flt = TK_TYPE_F32; name.resize(name.size() - 4); }
        const bool f16 = flt < 0 && name.size() > 4 && name.compare(name.size() - 4, 4, "-f16") == 0; /* the fp16 checkpoint recipe (BASELINE configs[4]) */
        if (f16) name.resize(name.size() - 4);
        int ftype = 0; /* the Q8_0, Q4_0, Q5_0, IQ4_NL, IQ4_XS and Q2_K recipes of fill_synthetic_ftype: synthetic://mistral-7b-q80, synthetic://mistral-7b-q40, synthetic://tiny-q50, synthetic://mistral-7b-iq4nl, synthetic://tiny-iq4xs, synthetic://mistral-7b-q2k, synthetic://tiny-q2ks */
        int gtype = 0; /* the recipes of fill_synthetic_type, by tensor type: synthetic://mistral-7b-q41, synthetic://tiny-q51 */
        if (name.size() > 4 && name.compare(name.size() - 4, 4, "-q80") == 0) { ftype = 7; name.resize(name.size() - 4); }
        else if (name.size() > 4 && name.compare(name.size() - 4, 4, "-q40") == 0) { ftype = 2; name.resize(name.size() - 4); }
        else if (name.size() > 4 && name.compare(name.size() - 4, 4, "-q50") == 0) { ftype = 8; name.resize(name.size() - 4); }
        else if (name.size() > 4 && name.compare(name.size() - 4, 4, "-q41") == 0) { gtype = TK_TYPE_Q4_1; name.resize(name.size() - 4); }
        else if (name.size() > 4 && name.compare(name.size() - 4, 4, "-q51") == 0) { gtype = TK_TYPE_Q5_1; name.resize(name.size() - 4); }
        else if (name.size() > 6 && name.compare(name.size() - 6, 6, "-iq4nl") == 0) { ftype = 25; name.resize(name.size() - 6); }
        else if (name.size() > 6 && name.compare(name.size() - 6, 6, "-iq4xs") == 0) { ftype = 30; name.resize(name.size() - 6); }
        else if (name.size() > 5 && name.compare(name.size() - 5, 5, "-tq10") == 0) { ftype = 36; name.resize(name.size() - 5); } /* the ternary recipes: synthetic://mistral-7b-tq10, synthetic://tiny-tq20 */
        else if (name.size() > 5 && name.compare(name.size() - 5, 5, "-tq20") == 0) { ftype = 37; name.resize(name.size() - 5); }
        else if (name.size() > 5 && name.compare(name.size() - 5, 5, "-q2ks") == 0) { ftype = 21; name.resize(name.size() - 5); }
        else if (name.size() > 4 && name.compare(name.size() - 4, 4, "-q2k") == 0) { ftype = 10; name.resize(name.size() - 4); }
        if (name == "mistral-7b") h = tk_mi355x_llm_hparams_t{32, 4096, 32, 8, 128, 14336, 32000, 1e-5f, 10000.0f, 0, 0, 0, 0, 1};
        else if (name == "tiny") h = tk_mi355x_llm_hparams_t{2, 256, 8, 2, 64, 512, 512, 1e-5f, 10000.0f, 0, 0, 0, 0, 1};
        else return fail(TK_ERROR_FILE_NOT_FOUND, "unknown synthetic model: " + name);
        rc = tk_mi355x_llm_model_create(&m, &h, device);
        if (rc == TK_SUCCESS && !lora.empty()) rc = tk_mi355x_llm_model_set_lora(m, lora.c_str());
        if (rc == TK_SUCCESS)
            rc = flt >= 0 ? tk_mi355x_llm_model_fill_synthetic_float(m, seed, flt)
                     : f16 ? tk_mi355x_llm_model_fill_synthetic_f16(m, seed)
                     : gtype ? tk_mi355x_llm_model_fill_synthetic_type(m, seed, gtype)
                     : ftype ? tk_mi355x_llm_model_fill_synthetic_ftype(m, seed, ftype) : tk_mi355x_llm_model_fill_synthetic(m, seed);
        if (rc != TK_SUCCESS) { if (m) release_model(m); return rc; } /* g_models_mu is held here */
        if (m->lora) { m->model.lora = nullptr; m->lora->drop_factors(); }
        m->path = path;
    } else {
        rc = tk_mi355x_llm_model_load_gguf_lora(&m, file.c_str(), lora.c_str(), device);
        if (rc != TK_SUCCESS) return rc;
        m->path = path;
    }
    if (!params->force_reload) g_models.push_back(m); /* a force-reloaded copy stays private to its handle */
    loader->held.push_back(m);
    *out_model_handle = m;
    return TK_SUCCESS;
}

tk_error_code_t tk_model_loader_unload_model(tk_model_loader_t* loader, void** model_handle) {
    if (!loader || !model_handle || !*model_handle) return TK_ERROR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lk(loader->mu);
    std::lock_guard<std::mutex> gl(g_models_mu);
    for (size_t i = 0; i < loader->held.size(); ++i)
        if (loader->held[i] == *model_handle) {
            loader->held.erase(loader->held.begin() + i);
            release_model((tk_mi355x_llm_model_t*)*model_handle);
            *model_handle = nullptr;
            return TK_SUCCESS;
        }
    return fail(TK_ERROR_INVALID_ARGUMENT, "handle was not produced by this loader");
}

struct tk_llm_runner_s {
    tk_mi355x_llm_model_t* model = nullptr;
    TkLlmBatcher* batcher = nullptr; /* shared with the other runners of the model */
    int slot = -1;                   /* this runner's sequence in the shared KV cache */
    int n_ctx = 0;
    int n_past = 0;
    int32_t pending = -1; /* token sampled from the last logits, not yet decoded */
    TkLlmBatcher::PrefixRows last_prompt; /* what became of the rows of the last prepare_generation (tk_mi355x_llm_runner_last_prompt_rows) */
    /* sampling: greedy unless tk_mi355x_llm_runner_set_sampling gave a temperature; the generator is keyed by (config.random_seed, number of
     * tokens this runner has sampled since its creation), so a runner's ids do not depend on which other runners share its passes */
    TkSampleRow samp{};
    const TkSampleRow* next_samp() { return samp.temp > 0.0f ? &samp : nullptr; }
    /* logit bias and repetition penalties (tk_mi355x_ext.h "sampling"), off by default.  accepted: the ids generate_next_token has taken from
     * `pending` since the last prepare_generation (llama_sampling_accept), the most recent TK_ADJUST_MAX_RECENT of them, oldest first */
    std::vector<int32_t> accepted;
    int32_t pen_last_n = 0;
    float pen_repeat = 1.0f, pen_freq = 0.0f, pen_present = 0.0f;
    std::vector<int32_t> bias_ids;
    std::vector<float> bias;
    TkLogitAdjust adj;
    void accept(int32_t id) {
        if (accepted.size() == TK_ADJUST_MAX_RECENT) accepted.erase(accepted.begin());
        accepted.push_back(id);
    }
    /* the adjustment of the next sampled row, or nullptr when the runner has neither penalties nor a bias list (it then submits what it always did) */
    const TkLogitAdjust* next_adjust() {
        if (pen_last_n == 0 && bias_ids.empty()) return nullptr;
        const size_t n = std::min(accepted.size(), (size_t)pen_last_n);
        adj = TkLogitAdjust{};
        adj.repeat = pen_repeat; adj.freq = pen_freq; adj.present = pen_present;
        adj.n_recent = (int32_t)n; adj.recent = accepted.data() + (accepted.size() - n);
        adj.n_bias = (int32_t)bias_ids.size(); adj.bias_ids = bias_ids.data(); adj.bias = bias.data();
        return &adj;
    }
    /* log-probabilities (tk_mi355x_llm_runner_set_logprobs, csrc/common/tk_token_logprob.h), off by default.  last_lp: the record of the id in `pending`,
     * valid once something has been sampled since the feature was switched on */
    int32_t lp_ntop = -1;
    TkTokenLogprob last_lp{};
    bool lp_valid = false;
    /* context shift (tk_mi355x_llm_runner_set_context_shift), off by default: llama.cpp's answer to a full context */
    bool shift_on = false;
    int32_t shift_keep = 0;      /* n_keep; -1 = prompt_tokens, resolved when a shift happens */
    int32_t prompt_tokens = 0;   /* token count of the last prepare_generation */
    int32_t n_shifts = 0;        /* since the last prepare_generation */
    int64_t n_discarded = 0;
    /* lookup decoding (tk_mi355x_llm_runner_set_lookup, csrc/llm/tk_lookup.h), off by default.  ctx_ids: the ids of the context — one per cache row
     * below n_past, then the ids sampled but not handed out yet (`pending`, then `queued`); a context shift drops the ids whose rows it drops.
     * queued: the ids a verify pass accepted behind `pending`, handed out one per generate_next_token; while it is not empty `pending` and all of
     * them but the last have been fed already (n_past counts their rows), and no pass is submitted */
    int32_t lookup_draft = 0, lookup_min = 1, lookup_max = 1;
    std::vector<int32_t> prediction;
    std::vector<int32_t> ctx_ids;
    std::vector<int32_t> queued;
    uint64_t lookup_passes = 0, lookup_drafted = 0, lookup_accepted = 0; /* since the last prepare_generation */
    /* the scope (tk_mi355x_llm_runner_set_lookup_scope, csrc/llm/tk_lookup_scope.h), 0 by default: lookup does nothing while the runner samples
     * stochastically, under a grammar mask, with penalties or a bias, or with log-probabilities on, unless the scope has the bit of every such
     * condition that holds; an inactive runner submits what it always did */
    uint32_t lookup_scope = 0;
    bool adjusted() const { return pen_last_n != 0 || !bias_ids.empty(); }
    bool lookup_active() const { return lookup_draft > 0 && tk_lookup_scope_allows(lookup_scope, samp.temp > 0.0f, grammar_on, adjusted(), lp_ntop >= 0); }
    /* what a verify pass with tables left with the queued ids: their records (one per queued id when the pass asked for them, else empty), and whether
     * the pass drew them from the stochastic chain — samp.counter then counts them already */
    std::vector<TkTokenLogprob> queued_lp;
    bool queued_drawn = false;
    /* host time since the last prepare_generation (tk_mi355x_llm_runner_lookup_host_ms): cutting the drafts under the grammar and building the
     * per-row masks of the verify requests, and the verify requests themselves (submit_verify: queueing, the pass, the wake-up) */
    double lookup_masks_ms = 0.0, lookup_requests_ms = 0.0;
    /* the queued ids are forgotten (a new prompt, a reset): the sampling counter goes back to the number of tokens the runner has sampled and kept,
     * and their records go with them */
    void forget_queued() {
        if (queued_drawn) samp.counter -= (uint32_t)queued.size();
        queued.clear();
        queued_lp.clear();
        queued_drawn = false;
    }
    /* the owner abandons the ids it was handed but has not given out (a tool response): back to the state of a runner that holds `pending`
     * alone — the rows fed ahead are stale rows beyond n_past, overwritten before anything attends to them */
    void drop_queued() {
        n_past -= (int)queued.size();
        forget_queued();
        if ((int)ctx_ids.size() > n_past) ctx_ids.resize((size_t)n_past);
    }
    bool is_processing = false;
    std::string piece;
    std::string system_prompt;
    /* tool-call grammar (reference: tk_runner_lifecycle.c:59 loads it at create, tk_runner_streaming.c:44-48 arms it per generation) */
    TkGrammar grammar;
    bool has_grammar = false;
    bool grammar_on = false;
    TkGrammarState gstate;
    TkTokenTrie trie;
    bool trie_built = false;
    std::vector<uint32_t> mask;
    std::string tool_call_text; /* what the grammar has accepted so far: the tool call the host reads after the sentinel */
    std::string tool_grammar_text; /* what was loaded at create: tk_mi355x_llm_runner_set_grammar(NULL) goes back to it */
    /* masks built on the device (tk_mi355x_llm_runner_set_device_mask, csrc/common/tk_grammar_walk.h), off by default.  gslot: the grammar's image in
     * the session's arena, -2 = not asked for yet, -1 = none (no image, or the arena is full: host masks).  attached: the mask pointers of the
     * request being submitted that stand for a state on the device.  The three counters run since the last prepare_generation */
    bool device_mask = false;
    bool vocab_sent = false;
    int gslot = -2;
    std::vector<const uint32_t*> attached;
    uint64_t mask_device_rows = 0, mask_host_rows = 0, mask_redone = 0;
    bool device_ready() {
        if (gslot != -2) return gslot >= 0;
        gslot = -1;
        TkGrammarImage gi;
        if (!grammar.flatten(&gi)) return false;
        TkLlmSession* ses = batcher->session();
        if (!vocab_sent) { /* the vocabulary image: the pieces the trie indexes, back to back */
            const int vocab = model->model.hp.vocab;
            std::vector<uint32_t> off((size_t)vocab + 1, 0u);
            std::string bytes;
            for (int i = 0; i < vocab; ++i) {
                if (i != model->tok.eos) bytes += model->tok.piece(i);
                off[(size_t)i + 1] = (uint32_t)bytes.size();
            }
            if (!ses->install_vocab_image(off.data(), (const uint8_t*)bytes.data(), model->tok.eos)) return false;
            vocab_sent = true;
        }
        const std::vector<uint32_t>& w = grammar.flat_words();
        gslot = ses->grammar_slot(w.data(), w.size(), gi.n_rules, gi.n_elems, gi.n_sets, gi.root);
        return gslot >= 0;
    }
    /* the mask of one sampled row whose grammar state is `s`: the pointer the scheduler is given.  With the device mask on the state is attached to
     * that pointer and the bits are built by the pass itself (the words behind the pointer are not read); a state without an image, and every row
     * when host_only, takes TkGrammarState::mask */
    const uint32_t* row_mask(const TkGrammarState& s, std::vector<uint32_t>* bits, bool host_only) {
        if (device_mask && !host_only && device_ready()) {
            TkGrammarStateImage img;
            if (s.export_image(&img)) {
                img.grammar = gslot;
                bits->resize(((size_t)model->model.hp.vocab + 31) / 32);
                if (batcher->session()->attach_grammar_state(bits->data(), img)) {
                    attached.push_back(bits->data());
                    mask_device_rows++;
                    return bits->data();
                }
            }
        }
        if (!trie_built) {
            std::vector<std::string> pieces((size_t)model->model.hp.vocab);
            for (int i = 0; i < (int)pieces.size(); ++i) pieces[i] = (i == model->tok.eos) ? std::string() : model->tok.piece(i);
            trie.build(pieces);
            trie_built = true;
        }
        s.mask(trie, model->tok.eos, bits);
        mask_host_rows++;
        return bits->data();
    }
    /* after the request: the attached states are forgotten.  true (ok: the request succeeded): a row's mask was not built, or the walk left one of
     * its tokens undecided — the row may have picked from too small a set, and the request is submitted again with host masks */
    bool finish_masks(bool ok) {
        bool redo = false;
        for (const uint32_t* p : attached) {
            bool ran = false;
            int32_t undecided = 0;
            batcher->session()->detach_grammar_state(p, &ran, &undecided);
            redo = redo || !ran || undecided > 0;
        }
        attached.clear();
        return ok && redo;
    }
    /* allowed-token bits for the next sample, or nullptr when sampling is unconstrained */
    const uint32_t* next_mask(bool host_only = false) { return grammar_on ? row_mask(gstate, &mask, host_only) : nullptr; }
};

/* the reference reads the grammar from a cwd-relative path; fall back to the built-in text of the same language */
static std::string load_tool_grammar_text() {
    const char* env = getenv("TK_TOOL_GRAMMAR");
    const char* paths[2] = {env, "src/ai_models/grammars/tool_call.gbnf"};
    for (const char* path : paths) {
        if (!path) continue;
        FILE* f = fopen(path, "rb");
        if (!f) continue;
        std::string text;
        char buf[4096];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
        fclose(f);
        return text;
    }
    return TK_DEFAULT_TOOL_CALL_GBNF;
}

tk_error_code_t tk_mi355x_llm_runner_last_prompt_rows(tk_llm_runner_t* runner, int32_t* prompt_rows, int32_t* kept, int32_t* copied) {
    if (!runner) return TK_ERROR_INVALID_ARGUMENT;
    if (prompt_rows) *prompt_rows = runner->last_prompt.prompt_rows;
    if (kept) *kept = runner->last_prompt.kept;
    if (copied) *copied = runner->last_prompt.copied;
    return TK_SUCCESS;
}

const char* tk_mi355x_llm_runner_tool_call_text(tk_llm_runner_t* runner) { return runner ? runner->tool_call_text.c_str() : NULL; }

tk_error_code_t tk_mi355x_llm_runner_set_sampling(tk_llm_runner_t* runner, float temperature, int32_t top_k, float top_p, float min_p) {
    if (!runner || !(temperature >= 0.0f) || top_k < 0 || !(top_p > 0.0f) || top_p > 1.0f || !(min_p >= 0.0f) || min_p > 1.0f) return TK_ERROR_INVALID_ARGUMENT;
    /* the device sampler draws from at most TK_SAMPLE_MAX_K = 64 candidates: llama.cpp's default top_k (40) fits; a larger top_k is refused rather than
     * clamped silently, and top_k = 0 ("the whole vocabulary" in llama.cpp) means the 64 largest here (include/tk/tk_mi355x_ext.h) */
    if (top_k > TK_SAMPLE_MAX_K) return fail(TK_ERROR_INVALID_ARGUMENT, "top_k above 64: the sampler keeps at most 64 candidates");
    if (temperature > 0.0f && runner->model->model.hp.vocab > 65536) return fail(TK_ERROR_NOT_IMPLEMENTED, "stochastic sampling supports vocabularies of at most 65536 tokens");
    runner->samp.temp = temperature; runner->samp.top_k = top_k; runner->samp.top_p = top_p; runner->samp.min_p = min_p;
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_runner_set_penalties(tk_llm_runner_t* runner, int32_t last_n, float repeat, float freq, float present) {
    if (!runner) return TK_ERROR_INVALID_ARGUMENT;
    if (last_n < 0 || last_n > TK_ADJUST_MAX_RECENT) return fail(TK_ERROR_INVALID_ARGUMENT, "penalties: last_n must be in [0, 256] (-1, the context size, is not supported)");
    const TkAdjustRow d{repeat, freq, present, 0, 0}; /* the values; the window is the runner's own */
    if (const char* why = tk_adjust_check(d, nullptr, nullptr, nullptr, runner->model->model.hp.vocab)) return fail(TK_ERROR_INVALID_ARGUMENT, std::string("penalties: ") + why);
    runner->pen_last_n = last_n; runner->pen_repeat = repeat; runner->pen_freq = freq; runner->pen_present = present;
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_runner_set_logit_bias(tk_llm_runner_t* runner, int32_t n, const int32_t* ids, const float* bias) {
    if (!runner) return TK_ERROR_INVALID_ARGUMENT;
    const TkAdjustRow d{1.0f, 0.0f, 0.0f, 0, n};
    if (const char* why = tk_adjust_check(d, nullptr, ids, bias, runner->model->model.hp.vocab)) return fail(TK_ERROR_INVALID_ARGUMENT, std::string("logit bias: ") + why);
    runner->bias_ids.assign(ids, ids + n);
    runner->bias.assign(bias, bias + n);
    return TK_SUCCESS;
}

int32_t tk_mi355x_llm_runner_recent_tokens(tk_llm_runner_t* runner, int32_t* out, int32_t cap) {
    if (!runner) return -1;
    for (int32_t i = 0; out && i < cap && i < (int32_t)runner->accepted.size(); ++i) out[i] = runner->accepted[(size_t)i];
    return (int32_t)runner->accepted.size();
}

tk_error_code_t tk_mi355x_llm_runner_set_logprobs(tk_llm_runner_t* runner, int32_t n_top) {
    if (!runner) return TK_ERROR_INVALID_ARGUMENT;
    if (const char* why = tk_logprob_check(n_top, runner->model->model.hp.vocab)) return fail(TK_ERROR_INVALID_ARGUMENT, std::string("log-probabilities: ") + why);
    if ((n_top < 0) != (runner->lp_ntop < 0)) runner->lp_valid = false; /* switched on or off: the next sampled token brings the first record */
    runner->lp_ntop = n_top;
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_runner_last_logprobs(tk_llm_runner_t* runner, tk_mi355x_token_logprob_t* out) {
    if (!runner || !out) return TK_ERROR_INVALID_ARGUMENT;
    if (runner->lp_ntop < 0) return fail(TK_ERROR_INVALID_STATE, "log-probabilities are off for this runner");
    if (!runner->lp_valid) return fail(TK_ERROR_INVALID_STATE, "no token has been sampled since log-probabilities were switched on");
    const TkTokenLogprob& g = runner->last_lp;
    out->logprob = g.logprob;
    out->n_top = g.n_top;
    for (int j = 0; j < g.n_top; ++j) { out->top_ids[j] = g.top_ids[j]; out->top_logprobs[j] = g.top_logprobs[j]; }
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_runner_set_lookup(tk_llm_runner_t* runner, int32_t n_draft, int32_t ngram_min, int32_t ngram_max) {
    if (!runner) return TK_ERROR_INVALID_ARGUMENT;
    if (n_draft < 0 || n_draft > TK_LOOKUP_MAX_DRAFT) return fail(TK_ERROR_INVALID_ARGUMENT, "lookup: n_draft must be in [0, 15]");
    if (ngram_min < 1 || ngram_min > ngram_max || ngram_max > TK_LOOKUP_MAX_NGRAM) return fail(TK_ERROR_INVALID_ARGUMENT, "lookup: 1 <= ngram_min <= ngram_max <= 8");
    runner->lookup_draft = n_draft; runner->lookup_min = ngram_min; runner->lookup_max = ngram_max;
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_runner_set_lookup_scope(tk_llm_runner_t* runner, uint32_t flags) {
    if (!runner) return TK_ERROR_INVALID_ARGUMENT;
    if (flags & ~TK_LOOKUP_SCOPE_ALL) return fail(TK_ERROR_INVALID_ARGUMENT, "lookup scope: unknown flag bits");
    static_assert(TK_MI355X_LOOKUP_SAMPLED == TK_LOOKUP_SCOPE_SAMPLED && TK_MI355X_LOOKUP_GRAMMAR == TK_LOOKUP_SCOPE_GRAMMAR &&
                      TK_MI355X_LOOKUP_ADJUSTED == TK_LOOKUP_SCOPE_ADJUSTED && TK_MI355X_LOOKUP_LOGPROBS == TK_LOOKUP_SCOPE_LOGPROBS,
                  "the public scope flags are tk_lookup_scope.h's");
    runner->lookup_scope = flags;
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_runner_set_device_mask(tk_llm_runner_t* runner, int on) {
    if (!runner || (on != 0 && on != 1)) return TK_ERROR_INVALID_ARGUMENT;
    runner->device_mask = on != 0;
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_runner_mask_stats(tk_llm_runner_t* runner, uint64_t* device_rows, uint64_t* host_rows, uint64_t* redone_requests) {
    if (!runner) return TK_ERROR_INVALID_ARGUMENT;
    if (device_rows) *device_rows = runner->mask_device_rows;
    if (host_rows) *host_rows = runner->mask_host_rows;
    if (redone_requests) *redone_requests = runner->mask_redone;
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_runner_set_grammar(tk_llm_runner_t* runner, const char* gbnf) {
    if (!runner) return TK_ERROR_INVALID_ARGUMENT;
    if (runner->is_processing) return fail(TK_ERROR_INVALID_STATE, "set_grammar: a generation is in progress");
    TkGrammar g;
    std::string err;
    const bool parsed = g.parse(gbnf ? std::string(gbnf) : runner->tool_grammar_text, &err);
    if (gbnf && !parsed) return fail(TK_ERROR_INVALID_ARGUMENT, "GBNF: " + err); /* the runner's grammar is unchanged */
    /* NULL: the state tk_llm_runner_create left, a tool grammar that was rejected there included */
    runner->grammar = std::move(g); /* the same object: the grammar state keeps pointing at it */
    runner->has_grammar = parsed;
    runner->grammar_on = false; /* armed by the next prepare_generation(use_tool_grammar = true) */
    runner->gslot = -2;
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_runner_lookup_host_ms(tk_llm_runner_t* runner, double* masks_ms, double* requests_ms) {
    if (!runner) return TK_ERROR_INVALID_ARGUMENT;
    if (masks_ms) *masks_ms = runner->lookup_masks_ms;
    if (requests_ms) *requests_ms = runner->lookup_requests_ms;
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_runner_get_lookup_scope(tk_llm_runner_t* runner, uint32_t* flags) {
    if (!runner || !flags) return TK_ERROR_INVALID_ARGUMENT;
    *flags = runner->lookup_scope;
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_runner_set_prediction(tk_llm_runner_t* runner, const int32_t* ids, int32_t n) {
    if (!runner || n < 0 || (n > 0 && !ids)) return TK_ERROR_INVALID_ARGUMENT;
    if (n > TK_LOOKUP_MAX_PRED) return fail(TK_ERROR_INVALID_ARGUMENT, "prediction: at most 4096 ids");
    for (int32_t i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= runner->model->model.hp.vocab) return fail(TK_ERROR_INVALID_ARGUMENT, "prediction: id " + std::to_string(i) + " is outside the vocabulary");
    runner->prediction.assign(ids, ids + n);
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_runner_lookup_stats(tk_llm_runner_t* runner, uint64_t* verify_passes, uint64_t* drafted, uint64_t* accepted) {
    if (!runner) return TK_ERROR_INVALID_ARGUMENT;
    if (verify_passes) *verify_passes = runner->lookup_passes;
    if (drafted) *drafted = runner->lookup_drafted;
    if (accepted) *accepted = runner->lookup_accepted;
    return TK_SUCCESS;
}

tk_error_code_t tk_llm_runner_create(tk_llm_runner_t** out_runner, void* model_handle, const tk_llm_config_t* config) {
    if (!out_runner || !model_handle || !config) return TK_ERROR_INVALID_ARGUMENT;
    std::unique_ptr<tk_llm_runner_s> r(new tk_llm_runner_s());
    r->model = (tk_mi355x_llm_model_t*)model_handle;
    r->n_ctx = config->context_size ? (int)config->context_size : 4096;
    if (config->system_prompt) r->system_prompt = config->system_prompt;
    r->samp.seed = config->random_seed;
    {   /* a sequence slot in a shared session of this context size; a new session when every slot is taken */
        std::lock_guard<std::mutex> lk(r->model->batch_mu);
        for (auto& b : r->model->batchers)
            if (b->n_ctx() == r->n_ctx && (r->slot = b->acquire_slot()) >= 0) /* every session of a model has its one cache type: the setter refuses once one exists */ { r->batcher = b.get(); break; }
        if (!r->batcher) {
            int slots = r->model->runner_slots;
            if (slots <= 0) { const char* e = getenv("TK_MI355X_RUNNER_SLOTS"); slots = e ? atoi(e) : 0; }
            if (slots <= 0) slots = 16;
            std::unique_ptr<TkLlmBatcher> b(new TkLlmBatcher());
            std::string err;
            if (!b->init(&r->model->model, slots, r->n_ctx, r->model->tok.eos, &err, r->model->kv_cache_type)) return fail(TK_ERROR_GPU_MEMORY, err);
            if (r->model->prefix_cache) (void)b->set_prefix_cache(true);
            r->slot = b->acquire_slot();
            r->batcher = b.get();
            r->model->batchers.push_back(std::move(b));
        }
    }
    std::string gerr;
    r->tool_grammar_text = load_tool_grammar_text();
    r->has_grammar = r->grammar.parse(r->tool_grammar_text, &gerr);
    if (!r->has_grammar) tk_error_set_detail("tool-call grammar rejected (%s): tool grammar disabled", gerr.c_str()); /* the reference logs and goes on */
    {
        std::lock_guard<std::mutex> gl(g_models_mu);
        r->model->refcount++; /* released in tk_llm_runner_destroy: unloading the model under a live runner cannot free its sessions */
    }
    *out_runner = r.release();
    return TK_SUCCESS;
}

void tk_llm_runner_destroy(tk_llm_runner_t** runner) {
    if (!runner || !*runner) return;
    if ((*runner)->batcher) (*runner)->batcher->release_slot((*runner)->slot); /* the shared session lives as long as the model */
    {
        std::lock_guard<std::mutex> gl(g_models_mu);
        release_model((*runner)->model);
    }
    delete *runner;
    *runner = nullptr;
}

tk_error_code_t tk_mi355x_llm_runner_set_context_shift(tk_llm_runner_t* runner, int on, int32_t n_keep) {
    if (!runner || (on != 0 && on != 1)) return TK_ERROR_INVALID_ARGUMENT;
    if (n_keep < -1) return fail(TK_ERROR_INVALID_ARGUMENT, "context shift: n_keep must be >= 0, or -1 for the last prompt's token count");
    if (on && runner->model->model.hp.head_dim % 8 != 0) return fail(TK_ERROR_NOT_IMPLEMENTED, "context shift moves rows in 16-byte words: head_dim must be a multiple of 8");
    if (on && runner->model->kv_cache_type == TK_KV_Q8_0) return fail(TK_ERROR_NOT_IMPLEMENTED, "context shift re-rotates keys: not built for a Q8_0 KV cache");
    runner->shift_on = on != 0;
    runner->shift_keep = n_keep;
    return TK_SUCCESS;
}

tk_error_code_t tk_mi355x_llm_runner_context_shifts(tk_llm_runner_t* runner, int32_t* shifts, int64_t* discarded) {
    if (!runner) return TK_ERROR_INVALID_ARGUMENT;
    if (shifts) *shifts = runner->n_shifts;
    if (discarded) *discarded = runner->n_discarded;
    return TK_SUCCESS;
}

/* llama.cpp's context shift (examples/main): n_left = n_past - n_keep, n_discard = n_left / 2, rows [n_keep + n_discard, n_past) move down by
 * n_discard, n_past -= n_discard.  Applied once, when `need` more rows do not fit (n_past + need >= n_ctx) but fit after the shift; false (nothing
 * changed, *failed false) when the policy is off, nothing can be dropped or the rows still would not fit; false with *failed when the move failed */
static bool context_shift(tk_llm_runner_s* r, int need, bool* failed) {
    *failed = false;
    if (!r->shift_on) return false;
    const int n_keep = r->shift_keep < 0 ? r->prompt_tokens : r->shift_keep;
    const int n_discard = (r->n_past - n_keep) / 2;
    if (n_discard <= 0 || r->n_past - n_discard + need >= r->n_ctx) return false;
    std::string err;
    if (!r->batcher->shift(r->slot, n_keep, n_discard, r->n_past, &err)) {
        tk_error_set_detail("%s", err.c_str());
        *failed = true;
        return false;
    }
    /* the context's ids lose what the cache lost */
    if ((int)r->ctx_ids.size() >= n_keep + n_discard) r->ctx_ids.erase(r->ctx_ids.begin() + n_keep, r->ctx_ids.begin() + n_keep + n_discard);
    r->n_past -= n_discard;
    r->n_shifts++;
    r->n_discarded += n_discard;
    return true;
}

/* feed `toks` at positions n_past.. ; the last one is sampled.  The rows join whatever passes the model's scheduler is forming. */
static tk_error_code_t feed(tk_llm_runner_s* r, const std::vector<int32_t>& toks, bool whole_context = false) {
    if (toks.empty()) return TK_SUCCESS;
    r->drop_queued(); /* ids handed to the runner but not to its caller (lookup decoding): the tokens go where they go with lookup off */
    if (r->n_past + (int)toks.size() >= r->n_ctx) {
        bool failed = false;
        /* a prompt (whole_context) that is longer than the context is refused whatever the policy: there is nothing behind it to drop */
        if (whole_context || !context_shift(r, (int)toks.size(), &failed))
            return failed ? TK_ERROR_INFERENCE_FAILED : fail(TK_ERROR_INFERENCE_FAILED, "prompt exceeds the context window");
    }
    int32_t am = -1;
    std::string err;
    /* whole_context (prepare_generation): the tokens start at position 0, so the scheduler may keep or copy rows the cache already holds for them */
    bool ok = r->batcher->submit(r->slot, r->n_past, toks.data(), (int)toks.size(), r->next_mask(), &am, &err, r->next_samp(), whole_context ? &r->last_prompt : nullptr,
                                 r->next_adjust(), r->lookup_active(), r->lp_ntop, r->lp_ntop >= 0 ? &r->last_lp : nullptr);
    if (r->finish_masks(ok)) { /* an undecided token: the sampled row again, at its position, under a host mask; nothing of the runner has advanced */
        r->mask_redone++;
        ok = r->batcher->submit(r->slot, r->n_past + (int)toks.size() - 1, &toks.back(), 1, r->next_mask(true), &am, &err, r->next_samp(), nullptr, r->next_adjust(),
                                r->lookup_active(), r->lp_ntop, r->lp_ntop >= 0 ? &r->last_lp : nullptr);
    }
    if (!ok) return fail(TK_ERROR_INFERENCE_FAILED, err);
    r->lp_valid = r->lp_ntop >= 0;
    if (r->samp.temp > 0.0f) r->samp.counter++;
    r->n_past += (int)toks.size();
    r->pending = am;
    r->ctx_ids.insert(r->ctx_ids.end(), toks.begin(), toks.end());
    r->ctx_ids.push_back(am);
    return TK_SUCCESS;
}

tk_error_code_t tk_llm_runner_prepare_generation(tk_llm_runner_t* runner, const char* prompt, bool use_tool_grammar) {
    if (!runner || !prompt) return TK_ERROR_INVALID_ARGUMENT;
    /* greedy sampling constrained by the tool-call grammar: the arg max runs over the tokens the grammar allows (mask applied on
     * the device), the reference's llama_sampling_set_grammar(sctx, grammar or NULL) (tk_runner_streaming.c:44-48) */
    runner->grammar_on = use_tool_grammar && runner->has_grammar;
    if (runner->grammar_on) runner->gstate.init(&runner->grammar);
    runner->tool_call_text.clear();
    std::vector<int32_t> toks = runner->model->tok.encode(prompt, true);
    runner->n_past = 0; /* llama_kv_cache_clear: positions restart, stale cache rows are never attended */
    runner->pending = -1;
    runner->accepted.clear(); /* llama_sampling_reset (tk_runner_streaming.c:42): the only call that empties the window */
    runner->last_prompt = TkLlmBatcher::PrefixRows{(int32_t)toks.size(), 0, 0};
    runner->prompt_tokens = (int32_t)toks.size();
    runner->n_shifts = 0;
    runner->n_discarded = 0;
    runner->forget_queued();
    runner->ctx_ids.clear();
    runner->lookup_passes = runner->lookup_drafted = runner->lookup_accepted = 0;
    runner->lookup_masks_ms = runner->lookup_requests_ms = 0.0;
    runner->mask_device_rows = runner->mask_host_rows = runner->mask_redone = 0;
    tk_error_code_t rc = feed(runner, toks, true);
    if (rc != TK_SUCCESS) return rc;
    runner->is_processing = true;
    return TK_SUCCESS;
}

const char* tk_llm_runner_generate_next_token(tk_llm_runner_t* runner) {
    if (!runner || !runner->is_processing) return NULL;
    const int32_t id = runner->pending;
    if (id >= 0) runner->accept(id); /* llama_sampling_accept (tk_runner_streaming.c:61) comes before the EOS test: that id is in the window too */
    if (id < 0 || id == runner->model->tok.eos) { runner->is_processing = false; return NULL; }
    /* the per-id logic is the same for an id that a verify pass queued: the window above, the grammar here */
    if (runner->grammar_on) {
        /* llama_sampling_accept: advance the grammar by the sampled token; then the reference's "grammar rule completed" test
         * (tk_runner_streaming.c:69-75): the token is NOT decoded, generation pauses, the sentinel address is returned */
        const std::string pc = runner->model->tok.piece(id);
        if (!runner->gstate.accept(pc)) { /* cannot happen with the mask applied */
            tk_error_set_detail("sampled token %d is outside the grammar", id);
            runner->is_processing = false;
            return NULL;
        }
        runner->tool_call_text += pc;
        if (runner->gstate.complete()) {
            runner->is_processing = false;
            runner->grammar_on = false; /* the tool response and what follows it are free text */
            return (const char*)1;
        }
    }
    if (!runner->queued.empty()) { /* lookup decoding: this id's row is in the cache already, and the id behind it has been sampled */
        runner->pending = runner->queued.front();
        runner->queued.erase(runner->queued.begin());
        /* its record came with it when the verify pass asked for records; an id sampled before log-probabilities were switched on has none */
        runner->lp_valid = runner->lp_ntop >= 0 && !runner->queued_lp.empty();
        if (!runner->queued_lp.empty()) {
            runner->last_lp = runner->queued_lp.front();
            runner->queued_lp.erase(runner->queued_lp.begin());
        }
        runner->piece = runner->model->tok.piece(id);
        return runner->piece.c_str();
    }
    if (runner->n_past + 1 >= runner->n_ctx) {
        bool failed = false;
        if (!context_shift(runner, 1, &failed)) { runner->is_processing = false; return NULL; }
    }
    int32_t t = id, am = -1;
    std::string err;
    const bool lookup = runner->lookup_active();
    if (lookup) {
        /* the pending id and what the draft rule guesses behind it in ONE pass; the drafts are clipped so that every fed position q has q + 1 < n_ctx:
         * the generation ends, or shifts, at exactly the token it does with lookup off */
        int32_t fed[1 + TK_LOOKUP_MAX_DRAFT], ids[1 + TK_LOOKUP_MAX_DRAFT];
        fed[0] = id;
        int nd = tk_lookup_draft(runner->ctx_ids.data(), (int)runner->ctx_ids.size(), runner->prediction.data(), (int)runner->prediction.size(), runner->lookup_min,
                                 runner->lookup_max, runner->lookup_draft, fed + 1);
        nd = std::max(0, std::min(nd, runner->n_ctx - runner->n_past - 2));
        /* the tables of the rows (csrc/llm/tk_lookup_scope.h): row i gets what a one-row pass behind pending, d0 .. d(i-1) would have had.  The
         * grammar states are copies — the runner's own advances only when an id is handed out — and cut the drafts */
        std::vector<TkGrammarState> gstates;
        const auto t_masks = std::chrono::steady_clock::now();
        auto ms_since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
        if (runner->grammar_on && nd > 0) {
            const auto& tok = runner->model->tok;
            nd = tk_lookup_grammar_cut(
                runner->gstate, fed + 1, nd,
                [&](TkGrammarState* s, int32_t d) { const std::string pc = d == tok.eos ? std::string() : tok.piece(d); return !pc.empty() && s->accept(pc); },
                [](const TkGrammarState& s) { return s.complete(); }, &gstates);
        }
        if (nd > 0) {
            const int n = 1 + nd;
            int n_ids = 0;
            const bool drawn = runner->samp.temp > 0.0f, masked = runner->grammar_on, adjusted = runner->adjusted(), records = runner->lp_ntop >= 0;
            std::vector<std::vector<uint32_t>> mask_bits(masked ? (size_t)n : 0);
            const uint32_t* mask_ptr[1 + TK_LOOKUP_MAX_DRAFT] = {};
            std::vector<int32_t> windows(adjusted ? (size_t)n * (size_t)std::max(runner->pen_last_n, 1) : 0);
            TkLogitAdjust adj[1 + TK_LOOKUP_MAX_DRAFT];
            for (int i = 0; i < n && adjusted; ++i) {
                int32_t* w = windows.data() + (size_t)i * (size_t)std::max(runner->pen_last_n, 1);
                adj[i] = TkLogitAdjust{};
                adj[i].repeat = runner->pen_repeat; adj[i].freq = runner->pen_freq; adj[i].present = runner->pen_present;
                adj[i].n_recent = tk_lookup_row_window(runner->accepted.data(), (int)runner->accepted.size(), fed + 1, i, runner->pen_last_n, w);
                adj[i].recent = w;
                adj[i].n_bias = (int32_t)runner->bias_ids.size(); adj[i].bias_ids = runner->bias_ids.data(); adj[i].bias = runner->bias.data();
            }
            TkTokenLogprob recs[1 + TK_LOOKUP_MAX_DRAFT];
            bool ok = false;
            for (int attempt = 0; attempt < 2; ++attempt) {
                /* row 0's state is the runner's own (it has accepted the pending id), row i's the copy behind draft i - 1.  A second attempt
                 * follows a request in which a mask row held an undecided token: the WHOLE request again, at the same positions and with the same
                 * sampling counter, under host masks — nothing of the runner has advanced */
                const auto t_attempt = attempt ? std::chrono::steady_clock::now() : t_masks;
                for (int i = 0; i < n && masked; ++i)
                    mask_ptr[i] = runner->row_mask(i == 0 ? runner->gstate : gstates[(size_t)i], i == 0 ? &runner->mask : &mask_bits[(size_t)i], attempt > 0);
                if (masked) runner->lookup_masks_ms += ms_since(t_attempt);
                const auto t_request = std::chrono::steady_clock::now();
                ok = runner->batcher->submit_verify(runner->slot, runner->n_past, fed, n, ids, &n_ids, &err, masked ? mask_ptr : nullptr, runner->next_samp(),
                                                    adjusted ? adj : nullptr, runner->lp_ntop, records ? recs : nullptr, masked || adjusted || records ? n : 0) &&
                     n_ids >= 1;
                runner->lookup_requests_ms += ms_since(t_request);
                if (!runner->finish_masks(ok)) break;
                runner->mask_redone++;
                ok = false;
            }
            if (!ok) {
                tk_error_set_detail("%s", err.c_str());
                runner->is_processing = false;
                return NULL;
            }
            /* the chain has drawn the ids that were kept: the counter is the one n_ids one-row passes would have left */
            if (drawn) runner->samp.counter += (uint32_t)n_ids;
            runner->queued_drawn = drawn;
            runner->queued_lp.clear();
            if (records) {
                runner->last_lp = recs[0];
                runner->queued_lp.assign(recs + 1, recs + n_ids);
            }
            runner->lp_valid = records;
            runner->lookup_passes++;
            runner->lookup_drafted += (uint64_t)nd;
            runner->lookup_accepted += (uint64_t)(n_ids - 1);
            runner->n_past += n_ids; /* rows 0 .. m of the pass are valid cache rows */
            runner->pending = ids[0];
            runner->queued.assign(ids + 1, ids + n_ids);
            runner->ctx_ids.insert(runner->ctx_ids.end(), ids, ids + n_ids);
            runner->piece = runner->model->tok.piece(id);
            return runner->piece.c_str();
        }
    }
    bool ok = runner->batcher->submit(runner->slot, runner->n_past, &t, 1, runner->next_mask(), &am, &err, runner->next_samp(), nullptr, runner->next_adjust(), lookup,
                                      runner->lp_ntop, runner->lp_ntop >= 0 ? &runner->last_lp : nullptr);
    if (runner->finish_masks(ok)) { /* an undecided token: the row again under a host mask; nothing of the runner has advanced */
        runner->mask_redone++;
        ok = runner->batcher->submit(runner->slot, runner->n_past, &t, 1, runner->next_mask(true), &am, &err, runner->next_samp(), nullptr, runner->next_adjust(), lookup,
                                     runner->lp_ntop, runner->lp_ntop >= 0 ? &runner->last_lp : nullptr);
    }
    if (!ok) {
        tk_error_set_detail("%s", err.c_str());
        runner->is_processing = false;
        return NULL;
    }
    runner->lp_valid = runner->lp_ntop >= 0;
    if (runner->samp.temp > 0.0f) runner->samp.counter++;
    runner->n_past++;
    runner->pending = am;
    runner->ctx_ids.push_back(am);
    runner->piece = runner->model->tok.piece(id);
    return runner->piece.c_str();
}

tk_error_code_t tk_llm_runner_add_tool_response(tk_llm_runner_t* runner, const char* tool_name, const char* tool_output) {
    if (!runner || !tool_name || !tool_output) return TK_ERROR_INVALID_ARGUMENT;
    std::string text = std::string("[TOOL_RESULT] name: \"") + tool_name + "\", output: " + tool_output + " [/TOOL_RESULT]";
    std::vector<int32_t> toks = runner->model->tok.encode(text, false);
    tk_error_code_t rc = feed(runner, toks);
    if (rc != TK_SUCCESS) return rc;
    runner->is_processing = true;
    return TK_SUCCESS;
}

tk_error_code_t tk_llm_runner_reset_context(tk_llm_runner_t* runner) {
    if (!runner) return TK_ERROR_INVALID_ARGUMENT;
    runner->n_past = 0;
    runner->pending = -1;
    runner->forget_queued();
    runner->ctx_ids.clear();
    runner->is_processing = false;
    return TK_SUCCESS;
}

void tk_llm_result_destroy(tk_llm_result_t** result) {
    if (!result || !*result) return;
    tk_llm_result_t* r = *result;
    if (r->type == TK_LLM_RESULT_TYPE_TEXT_RESPONSE) free(r->data.text_response);
    else if (r->type == TK_LLM_RESULT_TYPE_TOOL_CALL) { free(r->data.tool_call.name); free(r->data.tool_call.arguments_json); }
    free(r);
    *result = NULL;
}

} /* extern "C" */
