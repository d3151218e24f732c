/*
 * tk_mi355x_ext.h — extensions of the drop-in library that have no reference counterpart.
 *
 * The reference runs ONE sequence per runner on one thread (src/cortex/tk_cortex_main.c:957-994).
 * SURVEY.md §0 F9 shows the headline target needs >= 6 cortex cycles decoded concurrently so the
 * 4.3 GB weight stream is shared; these entry points expose that batched path (and the pieces the
 * parity tests drive directly) with plain pointers and sizes only.
 */
#ifndef TK_MI355X_EXT_H
#define TK_MI355X_EXT_H

#include "tk_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int32_t n_layer, d_model, n_head, n_kv_head, head_dim, d_ff, vocab;
    float rms_eps, rope_theta;
    int32_t ks_qkv, ks_o, ks_gateup, ks_down, ks_out; /* K-split plan (canonical summation order) */
} tk_mi355x_llm_hparams_t;

typedef struct tk_mi355x_llm_model_s tk_mi355x_llm_model_t;
typedef struct tk_mi355x_llm_session_s tk_mi355x_llm_session_t;

TK_API const char* tk_mi355x_version(void);
TK_API int tk_mi355x_device_count(void);
/* HIP device used by the reference entry points whose config carries no device id (tk_vad_silero_create,
 * tk_asr_whisper_create, tk_preprocessor_*, tk_model_loader_load_model); default 0.  One process per GPU sets its rank's device. */
TK_API void tk_mi355x_set_default_device(int device);
TK_API int tk_mi355x_get_default_device(void);

/* models ----------------------------------------------------------------------------------- */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_model_create(tk_mi355x_llm_model_t** out, const tk_mi355x_llm_hparams_t* hp, int device);
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_model_fill_synthetic(tk_mi355x_llm_model_t* m, uint64_t seed);
/* the fp16 checkpoint recipe (BASELINE configs[4]): every matrix and the token embedding IEEE f16 (GGUF type 1), norms f32.  f16 matrices run
 * on the exact fp32 MFMA GEMM over f16-rounded activations (one k-ordered chain per output, no K-split): results stay bit-identical to
 * the oracle.  Loader name: synthetic://mistral-7b-f16, synthetic://tiny-f16; GGUF files with F16 tensors load the same way. */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_model_fill_synthetic_f16(tk_mi355x_llm_model_t* m, uint64_t seed);
/* the same recipe in the other two float types: ggml_type 30 (BF16: every matrix and the token embedding bfloat16, the seeded values stored through
 * tk_mi355x_convert_bf16's rounding) or 0 (F32: stored unconverted); norms f32.  Any other value: TK_ERROR_INVALID_ARGUMENT.  The matrices run on the
 * same exact fp32 MFMA GEMM: a BF16 weight is its bits << 16 and the activations are rounded to bf16 (ggml's vec_dot_type for BF16), an F32 weight
 * is used as stored against unrounded activations; per K-split slab one fmaf chain over k ascending from +0, the slabs added in ascending order.
 * Loader names: synthetic://mistral-7b-bf16, synthetic://tiny-bf16, synthetic://mistral-7b-f32, synthetic://tiny-f32; GGUF files with BF16 / F32
 * matrices (convert_hf_to_gguf.py --outtype bf16 | f32) load the same way.  Among a model's matrices (layer matrices and output) at most ONE of F16 /
 * BF16 / F32 may occur, beside any mix of quantised types: a second float type fails the load (set_tensor, load_gguf, session_create) with a message
 * naming both.  token_embd is free of that rule. */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_model_fill_synthetic_float(tk_mi355x_llm_model_t* m, uint64_t seed, int ggml_type);
/* no GPU: the build's float -> bfloat16 rounding (ggml_compute_fp32_to_bf16: nearest even on the bits, subnormals kept, 0x7f7f8000 -> +inf, a NaN
 * becomes (bits >> 16) | 64), the one function host and kernels share; x [n] -> out [n] */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_convert_bf16(const float* x, int64_t n, uint16_t* out);
/* test / measurement entry: one production float matmul.  w [rows][K]: row-major values of `type` (1 F16, 30 BF16: uint16 bits; 0 F32), rows = the sum
 * of nseg (1 .. 3) segments of seg_rows[i] rows (each % 16 == 0), every segment tiled as a matrix of its own, as a model's q | k | v are; x [nrows][K]
 * (nrows <= 256; K % (256 ks) == 0, ks <= 8, rows <= 65536, rows x K <= 2^26) goes through the production operand-image producer with the type's rounding; ONE production launch with the
 * segments side by side and K split ks ways; the ks slabs added in ascending order into y [nrows][rows].  Other types: TK_ERROR_INVALID_ARGUMENT
 * (tk_mi355x_llm_gemv_probe keeps its own set) */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_matmul_float_probe(int device, int type, const void* w, int64_t rows, int64_t K, int ks, int nseg,
                                                                     const int32_t seg_rows[3], int nrows, const float* x, float* y);
/* the seeded weights of fill_synthetic under llama.cpp's k-quant mix `ftype`: 10 Q2_K (every matrix and token_embd Q2_K; attn_v Q4_K when
 * n_head / n_kv_head >= 4, else Q3_K; attn_output and ffn_down Q3_K), 21 Q2_K_S (Q2_K; attn_v Q4_K when n_head / n_kv_head >= 4; ffn_down Q4_K
 * for layers < n_layer / 8) — this build's definition of the two, files load by each tensor's own type regardless —, 11 Q3_K_S (every matrix and token_embd Q3_K), 12 Q3_K_M (Q3_K;
 * attn_v Q5_K for layers < 2 else Q4_K, attn_output Q4_K, ffn_down Q5_K for layers < n_layer / 16 else Q4_K), 14 Q4_K_S (Q4_K; Q5_K for
 * attn_v of layers < 4 and ffn_down of layers < n_layer / 8), 15 Q4_K_M (= fill_synthetic), 16 Q5_K_S (every matrix and token_embd Q5_K),
 * 17 Q5_K_M (Q4_K_M with Q5_K in place of Q4_K); output is Q6_K in all eight; 7 Q8_0 (every matrix, token_embd and output Q8_0); 2 Q4_0, 8 Q5_0, 25 IQ4_NL and 30 IQ4_XS (every layer matrix and token_embd in the base type, output Q6_K); 36 TQ1_0 and 37 TQ2_0 (llama.cpp's recipe for the ternary types: every layer matrix in the base type, token_embd Q4_K, output Q6_K).  Other values: TK_ERROR_INVALID_ARGUMENT — among them 13 Q3_K_L
 * (Q3_K with Q5_K attn_v, attn_output and ffn_down), which has no synthetic recipe; Q3_K_L FILES load all the same, since loading goes by
 * each tensor's own type and any mix of Q4_0 / Q4_1 / Q5_0 / Q5_1 / Q8_0 / Q2_K / Q3_K / Q4_K / Q5_K / Q6_K / IQ4_NL / IQ4_XS / TQ1_0 / TQ2_0 tensors beside one of F16 / BF16 / F32 is accepted
 * (file type 18, all Q6_K with a Q6_K token_embd, among them; it has no synthetic recipe either).
 * Loader names of the Q2_K recipes: synthetic://mistral-7b-q2k, synthetic://mistral-7b-q2ks, synthetic://tiny-q2k, synthetic://tiny-q2ks; of
 * the Q8_0 recipe: synthetic://mistral-7b-q80, synthetic://tiny-q80; of the Q4_0 / Q5_0 recipes: synthetic://mistral-7b-q40, synthetic://tiny-q40,
 * synthetic://mistral-7b-q50, synthetic://tiny-q50; of the IQ4_NL / IQ4_XS recipes: synthetic://mistral-7b-iq4nl, synthetic://tiny-iq4nl,
 * synthetic://mistral-7b-iq4xs, synthetic://tiny-iq4xs; of the ternary recipes: synthetic://mistral-7b-tq10, synthetic://tiny-tq10,
 * synthetic://mistral-7b-tq20, synthetic://tiny-tq20.  File types 3 (Q4_1) and 9 (Q5_1) have no recipe here: tk_mi355x_llm_model_fill_synthetic_type */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_model_fill_synthetic_ftype(tk_mi355x_llm_model_t* m, uint64_t seed, int ftype);
/* seeded weights by TENSOR type: every layer matrix and token_embd of GGML type `ggml_type`, output Q6_K, norms F32.  Takes 3 (Q4_1) and
 * 7 (Q5_1), the types whose file types fill_synthetic_ftype refuses; any other value: TK_ERROR_INVALID_ARGUMENT.
 * Loader names: synthetic://mistral-7b-q41, synthetic://tiny-q41, synthetic://mistral-7b-q51, synthetic://tiny-q51 */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_model_fill_synthetic_type(tk_mi355x_llm_model_t* m, uint64_t seed, int ggml_type);
/* test / measurement entry: one production mat-vec of `rows` x K raw GGUF blocks of `type` (2 Q4_0, 3 Q4_1, 6 Q5_0, 7 Q5_1, 8 Q8_0, 10 Q2_K, 11 Q3_K, 12 Q4_K, 13 Q5_K, 14 Q6_K, 20 IQ4_NL, 23 IQ4_XS, 34 TQ1_0, 35 TQ2_0; rows % 64 == 0,
 * K % (256 ks) == 0, ks <= 8) against x [nrows][K] (nrows <= 256): the blocks are repacked, x is quantised by the production Q8_K kernel,
 * the production launcher runs at width nrows with K split ks ways, and the ks partial sums are added in ascending order into y [nrows][rows] */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_gemv_probe(int device, int type, const void* blocks, int64_t rows, int64_t K, int ks, int nrows,
                                                             const float* x, float* y);
/* test entry: the repack alone.  `rows` x K raw GGUF blocks of `type` (the types of tk_mi355x_llm_gemv_probe; rows % 16 == 0, K % 256 == 0,
 * K <= 65536, rows x K <= 2^26) -> tiles [rows / 16][K / 256][the type's tile bytes], the resident layout the W4A8 kernels read (an IQ4_NL
 * matrix gives the Q4_0 tiles of the same bytes, a TQ1_0 matrix TQ2_0 tiles).  device >= 0: the load-time repack kernel on that device;
 * device < 0: the same per-lane function in a host loop, no GPU touched.  The arguments are checked before any device is: a null pointer, another type
 * or another shape is TK_ERROR_INVALID_ARGUMENT */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_repack_probe(int device, int type, const void* blocks, int64_t rows, int64_t K, void* tiles);
/* no GPU: the build's own one-pass block quantisers (csrc/common/tk_ggml_blocks.h) on the host.  x [n_blocks][256] floats -> n_blocks GGUF
 * blocks of `type` (11 Q3_K, 12 Q4_K, 13 Q5_K, 14 Q6_K) in out; the same code the synthetic-weight kernel runs on the device.  Type 8
 * (Q8_0): n_blocks counts 32-weight blocks, x [n_blocks][32] -> n_blocks 34-byte blocks, ggml's quantize_row_q8_0_ref value for value */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_quantize_blocks(int type, const float* x, int64_t n_blocks, void* out);
/* ggml's quantize_row_q4_0_ref / quantize_row_q5_0_ref value for value (GGML types 2 and 6): x [n_blocks][32] floats -> n_blocks 18- / 22-byte
 * blocks.  Entries of their own for the reason given below for Q2_K: types 2 and 6 stay TK_ERROR_INVALID_ARGUMENT in tk_mi355x_quantize_blocks */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_quantize_blocks_q4_0(const float* x, int64_t n_blocks, void* out);
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_quantize_blocks_q5_0(const float* x, int64_t n_blocks, void* out);
/* ggml's quantize_row_q4_1_ref / quantize_row_q5_1_ref value for value (GGML types 3 and 7): x [n_blocks][32] floats -> n_blocks 20- / 24-byte
 * blocks (f16 d, f16 m = the block's minimum, then Q4_0's / Q5_0's quant bytes; w = d q + m).  Types 3 and 7 stay TK_ERROR_INVALID_ARGUMENT in
 * tk_mi355x_quantize_blocks */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_quantize_blocks_q4_1(const float* x, int64_t n_blocks, void* out);
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_quantize_blocks_q5_1(const float* x, int64_t n_blocks, void* out);
/* IQ4_NL / IQ4_XS (GGML types 20 and 23): x [n_blocks][32] / [n_blocks][256] floats -> n_blocks 18- / 136-byte blocks, by this build's own
 * one-pass quantisers (the nearest code-book value against a scale that puts the block's signed extreme on -127; ggml's iterative search
 * is not restated).  Entries of their own for the same reason: types 20 and 23 stay TK_ERROR_INVALID_ARGUMENT in tk_mi355x_quantize_blocks */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_quantize_blocks_iq4_nl(const float* x, int64_t n_blocks, void* out);
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_quantize_blocks_iq4_xs(const float* x, int64_t n_blocks, void* out);
/* TQ1_0 / TQ2_0 (GGML types 34 and 35, the ternary types): x [n_blocks][256] floats -> n_blocks 54- / 66-byte blocks, ggml's
 * quantize_row_tq1_0_ref / quantize_row_tq2_0_ref value for value (d = max |x| stored as f16, trits lroundf(x / max |x|) + 1, five to a
 * base-3 byte or four to a 2-bit byte).  Types 34 and 35 stay TK_ERROR_INVALID_ARGUMENT in tk_mi355x_quantize_blocks */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_quantize_blocks_tq1_0(const float* x, int64_t n_blocks, void* out);
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_quantize_blocks_tq2_0(const float* x, int64_t n_blocks, void* out);
/* the same for Q2_K (GGML type 10): x [n_blocks][256] floats -> n_blocks 84-byte blocks.  An entry of its own because the set of types
 * tk_mi355x_quantize_blocks takes is fixed — callers rely on type 10 being TK_ERROR_INVALID_ARGUMENT there */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_quantize_blocks_q2k(const float* x, int64_t n_blocks, void* out);
/* tensor in GGUF block layout; layer = -1 for {0 token_embd, 1 output_norm, 2 output}, else
 * {0 attn_norm,1 q,2 k,3 v,4 o,5 ffn_norm,6 gate,7 up,8 down}; type = ggml type id (0 F32, 1 F16, 2 Q4_0, 3 Q4_1, 6 Q5_0, 7 Q5_1, 8 Q8_0, 10 Q2_K, 11 Q3_K, 12 Q4_K, 13 Q5_K, 14 Q6_K, 20 IQ4_NL, 23 IQ4_XS, 30 BF16, 34 TQ1_0, 35 TQ2_0).
 * token_embd takes every one of them; a matrix of F32 / F16 / BF16 needs rows % 16 == 0 and columns % 32 == 0, and a model's matrices hold at most
 * one of the three (tk_mi355x_llm_model_fill_synthetic_float); a Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, IQ4_NL, IQ4_XS, TQ1_0, TQ2_0 or k-quant tensor needs columns % 256 == 0.
 * A TQ1_0 matrix is installed as TQ2_0 tiles (its base-3 bytes decoded once, here): it runs the TQ2_0 kernels and holds 66, not 54, bytes per 256 weights */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_model_set_tensor(tk_mi355x_llm_model_t* m, int layer, int which, int type, const void* data,
                                                                   size_t nbytes);
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_model_load_gguf(tk_mi355x_llm_model_t** out, const char* path, int device);
/* LoRA adapters.  The reference applies one right after the model is loaded, in place and once: llama_model_apply_lora_from_file
 * (src/ai_models/tk_model_loader.c:259-270) — W' = W + (alpha / r) B A, a quantised W dequantised, added to and quantised back to its own type.
 * Here the same merge runs on the GPU while a matrix is installed, so an adapted model decodes at the un-adapted model's speed.
 * tk_model_load_params_t.lora_adapter is the reference's way in; these are the pieces:
 *   load_gguf_lora: load_gguf with an adapter (NULL / "" = none);
 *   set_lora: the adapter to merge into every matrix installed FROM NOW ON (set_tensor, fill_synthetic); NULL / "" = none.  Fails with
 *     TK_ERROR_MODEL_LOAD_FAILED (the reference's code) on an unreadable file or factor shapes that do not fit the model;
 *   lora_merged: matrices the adapter has changed so far;
 *   lora_probe: rank, alpha and tensor-pair count of an adapter file ("ggla" v1 — what llama_model_apply_lora_from_file read — or a GGUF
 *     adapter, general.type = "adapter"); no GPU involved. */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_model_load_gguf_lora(tk_mi355x_llm_model_t** out, const char* path, const char* lora_path, int device);
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_model_set_lora(tk_mi355x_llm_model_t* m, const char* adapter_path);
TK_API int tk_mi355x_llm_model_lora_merged(const tk_mi355x_llm_model_t* m);
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_lora_probe(const char* path, int32_t* rank, float* alpha, int32_t* n_tensors);
/* parses GGUF metadata only (runs without a GPU); n_vocab_tokens optional */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_gguf_probe(const char* path, tk_mi355x_llm_hparams_t* out, int32_t* n_vocab_tokens);
/* token ids of `text` under the vocabulary of a GGUF file (CPU only); returns the count (may exceed cap) or -1 */
TK_API int tk_mi355x_gguf_tokenize(const char* path, const char* text, int add_bos, int32_t* ids, int cap);
TK_API void tk_mi355x_llm_model_get_hparams(const tk_mi355x_llm_model_t* m, tk_mi355x_llm_hparams_t* out);
/* bytes of the matrices as installed = what a decode step streams (a TQ1_0 matrix counts its TQ2_0 tiles: 66 bytes per 256 weights, not the file's 54) */
TK_API uint64_t tk_mi355x_llm_model_weight_bytes(const tk_mi355x_llm_model_t* m);
TK_API void tk_mi355x_llm_model_destroy(tk_mi355x_llm_model_t** m);

/* continuous batching behind tk_llm_runner_* (csrc/llm/tk_llm_batcher.h): the runners created on one model handle (what
 * tk_model_loader_load_model returns) share decode sessions of `slots` sequences; their prepare_generation / generate_next_token rows
 * are coalesced into passes by one scheduler thread per session.  Set before the first tk_llm_runner_create on the model (default:
 * $TK_MI355X_RUNNER_SLOTS, else 16; at most tk_mi355x_llm_max_rows()).  KV memory = slots x context_size x 128 KiB for Mistral-7B. */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_model_set_runner_slots(void* model_handle, int slots);
/* Passes of one or two rows (one runner stepping alone) run their RMS-norm and SwiGLU producers inside the mat-vec launches that consume
 * them (five launches per layer instead of eight; same values); $TK_MI355X_NO_FUSE=1, read when a pass is recorded, keeps them as launches of
 * their own.  $TK_MI355X_NO_GRAPH=1 launches every pass eagerly instead of replaying hipGraphs (profilers).
 * Passes that hold several positions of a sequence (prompt chunks) and reach position 128 run their attention with 16 rows of a sequence per
 * workgroup on the fp32 matrix pipe (k_attention_prefill; same values as the per-row kernel): $TK_MI355X_NO_PREFILL_ATT=1 keeps the per-row
 * kernel everywhere.  $TK_MI355X_TIME_HOT=1 makes the stand-alone mat-vec timing (tk_mi355x_llm_time_gemv) repeat ONE layer's launch — weights
 * resident in the caches — instead of cycling through the layers.  $TK_MI355X_ASR_POLICY=1: include/tk/tk_audio.h. */
/* what the schedulers of a model have done so far: passes run, rows processed, the widest pass */
TK_API void tk_mi355x_llm_model_batch_stats(void* model_handle, uint64_t* passes, uint64_t* rows, int32_t* max_rows_in_a_pass);
/* run-ahead rows (csrc/llm/tk_llm_batcher.h) that no owner came back for: the scheduler feeds a sequence's sampled id one position ahead
 * of its owner's next tk_llm_runner_generate_next_token; a runner that stops or changes course costs one such row.  `rows` above counts
 * only rows an owner asked for. */
TK_API uint64_t tk_mi355x_llm_model_run_ahead_wasted(void* model_handle);
/* ---- prompt prefix cache (csrc/llm/tk_llm_batcher.h; opt-in; include/tk/ABI_NOTES.md).  A cache row at position p depends only on tokens 0 .. p
 * and its bits do not depend on the pass that computes it, so a row already in the shared KV cache for the same leading tokens is the row a
 * recomputation would write. ---- */
/* on = 0 (default): prepare_generation recomputes every row, as the reference does.  on = 1: rows whose tokens equal what the runner's slot
 * already holds are kept, rows another slot of the model holds are copied.  May be changed at any time; takes effect for the next prompt.
 * Tokens are the same either way.  TK_ERROR_NOT_IMPLEMENTED on a model whose head_dim is not a multiple of 8. */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_model_set_prefix_cache(void* model_handle, int on);
/* totals over the model's schedulers since load: prompt rows asked for by prepare_generation, of them kept in place, of them copied from
 * another slot, copy launches.  tk_mi355x_llm_model_batch_stats' `rows` keeps its meaning (rows COMPUTED for an owner): with the cache on it
 * falls by kept + copied. */
TK_API void tk_mi355x_llm_model_prefix_cache_stats(void* model_handle, uint64_t* prompt_rows, uint64_t* kept, uint64_t* copied,
                                                   uint64_t* copy_launches);
/* the same three row counts for this runner's last prepare_generation */
struct tk_llm_runner_s;
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_runner_last_prompt_rows(struct tk_llm_runner_s* runner, int32_t* prompt_rows, int32_t* kept,
                                                                          int32_t* copied);
/* the cache's matching rules on hand-written records, no device involved (tests): records[s * stride ..] holds the record_len[s] token ids whose
 * rows slot s holds.  out[0] = rows of toks[0 .. n) that self_slot's own record covers (at most n - 1; 0 when self_slot = -1); out[1] = the slot
 * that rows [cursor, out[2]) would be copied from (cursor = -1: out[0]), -1 = none: the longest match of at least 16 positions beyond the
 * cursor, the lowest slot among equals.  Returns 0, or -1 on bad arguments. */
TK_API int tk_mi355x_prefix_match(const int32_t* toks, int n, const int32_t* records, const int32_t* record_len, int n_slots, int stride, int self_slot,
                                  int cursor, int32_t out[3]);

/* sessions --------------------------------------------------------------------------------- */
/* max_seq sequences of max_ctx positions each, 1 <= max_ctx <= 32768 (RoPE is unscaled; a wider window is refused with a message that says so).
 * The KV cache is 2 x n_layer x max_seq x max_ctx x n_kv_head x head_dim f16 in one allocation each; a failure to allocate names the bytes. */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_session_create(tk_mi355x_llm_session_t** out, tk_mi355x_llm_model_t* m, int max_seq,
                                                                 int max_ctx);
/* ---- Q8_0 KV cache (csrc/common/tk_kv_q8.h; opt-in; include/tk/ABI_NOTES.md): llama.cpp's --cache-type-k q8_0 --cache-type-v q8_0.  A key or value
 * row is stored as ggml's Q8_0 blocks (32 int8 and one f16 scale) of the row the f16 cache would hold: 17/32 of the cache's bytes. ---- */
#define TK_MI355X_KV_F16 0
#define TK_MI355X_KV_Q8_0 1
/* tk_mi355x_llm_session_create with the cache type; kv_type 0 is that call.  Any other value than 0 or 1: TK_ERROR_INVALID_ARGUMENT.  A Q8_0
 * session runs every pass as k_qkv_rope_append's Q8_0 form + kernel 6 (tk_mi355x_attention_plan_kv); kv_write quantises the f16 rows it is given;
 * kv_copy works; kv_read is refused with TK_ERROR_INVALID_ARGUMENT (kv_read_q8 returns the raw rows); kv_shift, forward_stage, the pipeline and the
 * kv_copy / kv_shift timing entries are refused with TK_ERROR_NOT_IMPLEMENTED and a message that says "Q8_0 KV cache"; forward_verify takes form 0
 * (-1 resolves to it; 2 and 4 are refused by their messages) */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_session_create_kv(tk_mi355x_llm_session_t** out, tk_mi355x_llm_model_t* m, int max_seq, int max_ctx,
                                                                    int kv_type);
TK_API int tk_mi355x_llm_session_kv_type(const tk_mi355x_llm_session_t* s);       /* 0 or 1; -1 for NULL */
TK_API uint64_t tk_mi355x_llm_session_kv_bytes(const tk_mi355x_llm_session_t* s); /* bytes of the cache arrays, keys and values */
/* the raw rows of a Q8_0 session: positions [pos0, pos0 + n_pos) of one (layer, sequence), int8 values [position][kv head][head_dim] and f16 scale
 * bits [position][kv head][head_dim / 32].  TK_ERROR_INVALID_ARGUMENT on an F16 session.  Synchronous. */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_session_kv_read_q8(tk_mi355x_llm_session_t* s, int layer, int seq, int pos0, int n_pos, int8_t* kq,
                                                                     uint16_t* kd, int8_t* vq, uint16_t* vd);
/* the cache type of the sessions the runners of a model handle share (what tk_model_loader_load_model returns); set before the first
 * tk_llm_runner_create on the handle, like tk_mi355x_llm_model_set_runner_slots: afterwards TK_ERROR_INVALID_ARGUMENT with a message.  Default F16.
 * Runners of a Q8_0 model work as before — sampling, grammars, penalties, log-probabilities, prefix cache, lookup decoding —, except that
 * tk_mi355x_llm_runner_set_context_shift(on = 1) returns TK_ERROR_NOT_IMPLEMENTED.  _by_name takes llama.cpp's names "f16" and "q8_0"; any other
 * name is refused by name */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_model_set_kv_cache_type(void* model_handle, int kv_type);
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_model_set_kv_cache_type_by_name(void* model_handle, const char* name);
/* tk_mi355x_attention_plan with the cache type: kv_type 1 = {6, query heads per workgroup, positions per ring slot, 2} — kernel 6 = k_attention_far over
 * a Q8_0 cache, at every window and pass; kv_type 0 = tk_mi355x_attention_plan's answer */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_attention_plan_kv(int device, int nrows, int n_head, int n_kv_head, int head_dim, int max_ctx, int fused, int kv_type,
                                                                int32_t out[4]);
/* The Q8_0 cache's quantiser and attention on host arrays (tests), tk_mi355x_kv_shift_probe's contract.  The cache arrays are in the cache layout for
 * the geometry given: kq / vq [n_layer][max_seq][n_kv_head][max_ctx][head_dim] int8, kd / vd [...][max_ctx][head_dim / 32] f16 bits; seq / pos [nrows]
 * name each row's sequence and position; `layer` the layer.
 *   mode 0 (quantise): k16 / v16 [nrows][n_kv_head][head_dim] f16 bits become the cache rows (seq[r], pos[r]); the cache arrays are IN/OUT, every
 *     other row keeps its bits.  device >= 0: ONE launch of the production append kernel (zero query columns, an identity RoPE table).
 *   mode 1 (attention): q [nrows][n_head][head_dim] fp32 over positions 0 .. pos[r] of sequence seq[r]; out [nrows][n_head][head_dim] = the quotients
 *     the kernel hands to its Q8 activation quantiser.  device >= 0: ONE launch of kernel 6; needs a head geometry a model may have.
 * device < 0: the host loops of csrc/common/tk_kv_q8.h, no GPU touched.  Everything is validated before a device is touched: a NULL array, head_dim not a
 * multiple of 32 (or above 256), n_head no multiple of n_kv_head or a group above 4, a row outside the cache, nrows outside [1, tk_mi355x_llm_max_rows()],
 * an array shorter than the geometry needs (n_values = elements of kq and of vq, n_scales of kd and of vd, n_rows_elems of k16 / v16 or of q / out)
 * or more than 2^31 cache elements are TK_ERROR_INVALID_ARGUMENT with nothing written */
typedef struct tk_mi355x_kv_q8_probe_s {
    int32_t mode, n_layer, max_seq, n_kv_head, max_ctx, head_dim, layer, nrows, n_head;
    const int32_t *seq, *pos;
    int8_t *kq, *vq;
    uint16_t *kd, *vd;
    int64_t n_values, n_scales;
    const uint16_t *k16, *v16; /* mode 0 */
    const float* q;            /* mode 1 */
    float* out;                /* mode 1 */
    int64_t n_rows_elems;
} tk_mi355x_kv_q8_probe_t;
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_kv_q8_probe(int device, const tk_mi355x_kv_q8_probe_t* p);
TK_API void tk_mi355x_llm_session_destroy(tk_mi355x_llm_session_t** s);
/* rows one pass can hold (16-row MFMA M-tiles x 8): the row capacity of forward(), the column count of decode()'s out_tokens */
TK_API int tk_mi355x_llm_max_rows(void);
/* one pass over nrows <= tk_mi355x_llm_max_rows() (sequence, position, token) rows; logits [nrows][vocab] and argmax [nrows] optional */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_forward(tk_mi355x_llm_session_t* s, int nrows, const int32_t* seq, const int32_t* pos,
                                                          const int32_t* tok, float* logits, int32_t* argmax);
/* one pipeline stage of a pass (the LLM layer-sharded over GPUs): layers [layer0, layer1) of this rank's model.  The
 * first stage starts from tok (x_in NULL), later stages from the residual stream x_in [nrows][d_model] fp32; every stage but the last
 * writes the stream to x_out; the last (head != 0, layer1 == n_layer) samples into argmax[nrows].  x_on_host != 0: x_in / x_out are
 * host pointers (gloo), else device pointers on this session's GPU (RCCL send / recv buffers).  Synchronous.  Bit-identical to
 * tk_mi355x_llm_forward whatever the split. */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_forward_stage(tk_mi355x_llm_session_t* s, int nrows, const int32_t* seq, const int32_t* pos,
                                                                const int32_t* tok, const float* x_in, float* x_out, int x_on_host, int layer0,
                                                                int layer1, int head, int32_t* argmax);
/* ---- sampling.  The reference installs llama.cpp's default sampler (llama_sampling_default_params(), src/ai_models/tk_runner_lifecycle.c:76-77;
 * llama_sampling_sample, tk_runner_streaming.c:60-61; seed = tk_llm_config_t.random_seed, tk_runner_lifecycle.c:49): top-k 40, top-p 0.95,
 * min-p 0.05, temperature 0.8, one draw.  Here the default of a runner is GREEDY (the parity definition, and what the bench
 * runs); tk_mi355x_llm_runner_set_sampling switches a runner to that chain, on the device, with a counter-based generator keyed by
 * (random_seed, tokens sampled so far by this runner): the same seed gives the same ids whatever else shares the runner's passes, and the
 * oracle restates the arithmetic (orc_sample_row) so tests compare ids for fixed seeds.  temperature 0 = back to greedy.  top_k 0 = 64 (the
 * most candidates kept); top_p 1 and min_p 0 switch those filters off.  llama.cpp itself is absent (parity unpinned vs its generator).
 *
 * The whole chain, in llama.cpp's order (llama_sampling_prepare, then grammar, then the sampler), every stage on the device:
 *   1. logit bias:  logit[id] += bias                                                     (tk_mi355x_llm_runner_set_logit_bias; bias -inf bans a token)
 *   2. repetition penalties over the window = the last last_n ids the runner has accepted: for every distinct token t in it, c occurrences,
 *      l = logit[t];  l = l <= 0 ? l * repeat : l / repeat;  l = l - (float(c) * freq + present)   (tk_mi355x_llm_runner_set_penalties)
 *   3. the tool-call grammar's token mask   4. greedy arg max, or top-k, top-p, min-p, temperature and one draw.
 * Stages 1 and 2 are OFF by default (llama.cpp: penalty_last_n 64, penalty_repeat 1.10 or 1.00 depending on its generation, freq = present = 0;
 * the reference pins no generation).  Each is one correctly rounded fp32 operation after the other, the same on host and device
 * (csrc/common/tk_logit_adjust.h), so adjusted logits are reproducible bit for bit.  They apply to greedy rows too.
 * The window: an id enters it when tk_llm_runner_generate_next_token takes it (llama_sampling_accept, the id that turns out to be EOS included);
 * it empties in tk_llm_runner_prepare_generation, the only call in which the reference resets its sampler; add_tool_response and reset_context
 * leave it alone.  The first token after a prompt is sampled over an empty window: only the bias applies.
 * Not restated from llama.cpp: its `prev` ring starts as last_n zeros, so it penalises token 0 until last_n tokens have been accepted — here the
 * window holds accepted ids only; and last_n = -1 ("the context size") is refused (a window holds at most 256 ids).  The newline token is
 * penalised like any other (penalize_nl = true).
 * Run-ahead: a runner whose next row is adjusted, or whose penalties are on, does not run ahead (csrc/llm/tk_llm_batcher.h) — its next window
 * depends on the id it accepts — and pays one host round trip per token, like a runner under a grammar mask or a temperature.  A runner
 * with neither bias nor penalties (or with repeat 1, freq 0, present 0) runs exactly the passes it ran before. ---- */
typedef struct {
    float temperature, top_p, min_p;
    int32_t top_k;
    uint64_t seed;
    uint32_t counter; /* draws made so far with this seed */
    uint32_t reserved;
} tk_mi355x_sampling_t;
struct tk_llm_runner_s;
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_runner_set_sampling(struct tk_llm_runner_s* runner, float temperature, int32_t top_k, float top_p, float min_p);
/* tk_mi355x_llm_forward with a sampling state per row (temperature <= 0: that row takes the arg max); ids [nrows] */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_forward_sampled(tk_mi355x_llm_session_t* s, int nrows, const int32_t* seq, const int32_t* pos,
                                                                  const int32_t* tok, const tk_mi355x_sampling_t* sampling, float* logits, int32_t* ids);
/* one row's logit adjustment.  Limits (checked wherever one is taken): 0 <= n_recent <= 256, 0 <= n_bias <= 256, repeat finite and > 0, freq and
 * present finite, every bias finite or -inf, every id in [0, vocab), bias ids unique, no NULL array with a non-zero count.  A row with n_bias == 0
 * and (n_recent == 0 or repeat == 1, freq == 0, present == 0) is NEUTRAL: it is not adjusted at all */
typedef struct {
    float repeat, freq, present; /* 1, 0, 0 = off */
    int32_t n_recent;
    const int32_t* recent;
    int32_t n_bias;
    const int32_t* bias_ids;
    const float* bias;
} tk_mi355x_logit_adjust_t;
/* the runner's repetition penalties: last_n in [0, 256] (0 = off); takes effect from the next sampled token */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_runner_set_penalties(struct tk_llm_runner_s* runner, int32_t last_n, float repeat, float freq, float present);
/* replaces the runner's bias list (copied); n = 0 clears it; takes effect from the next sampled token */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_runner_set_logit_bias(struct tk_llm_runner_s* runner, int32_t n, const int32_t* ids, const float* bias);
/* the ids the runner has accepted since the last prepare_generation, oldest first — the most recent 256 of them, whatever last_n is; the
 * penalties read the last last_n.  Writes at most cap ids and returns the count held (may exceed cap); -1: no runner */
TK_API int32_t tk_mi355x_llm_runner_recent_tokens(struct tk_llm_runner_s* runner, int32_t* out, int32_t cap);
/* tk_mi355x_llm_forward_sampled with an adjustment per row: adjust [nrows] (neutral rows are plain rows); sampling may be NULL (every row
 * greedy).  Masks and sampling see the adjusted logits, and `logits` receives the ADJUSTED rows.  A pass with no non-neutral row is the pass
 * tk_mi355x_llm_forward_sampled runs.  tk_mi355x_llm_decode after it is unadjusted */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_forward_adjusted(tk_mi355x_llm_session_t* s, int nrows, const int32_t* seq, const int32_t* pos,
                                                                   const int32_t* tok, const tk_mi355x_sampling_t* sampling,
                                                                   const tk_mi355x_logit_adjust_t* adjust, float* logits, int32_t* ids);
/* ---- log-probabilities (csrc/common/tk_token_logprob.h; opt-in; include/tk/ABI_NOTES.md): llama.cpp's server `n_probs`, the hosted APIs' `logprobs` /
 * `top_logprobs` — how sure the model was of the id it produced, and what it would have said instead.  One device kernel behind the token pick, on
 * the logits the pick read, for the rows that ask; a runner, session or pass that does not ask runs exactly the launches and graphs it ran before.
 *   Distribution: softmax over the WHOLE vocabulary of the row's logits after stages 1 and 2 of the chain above (logit bias, repetition penalties) and
 *   BEFORE stage 3 and 4: no grammar mask, no temperature, no top-k / top-p / min-p — the model's own distribution.  A token banned with a -inf bias has
 *   log-probability -inf; a token the grammar forbids keeps its model log-probability and may appear among the alternatives.
 *   Arithmetic (the same bits on host and device): m = the maximum logit; S = the sum of tk_expf(l_i - m) in one fixed order — 1024 lanes each adding
 *   their terms i = t, t + 1024, ... ascending from +0, a six-level xor butterfly inside each wave of 64, the sixteen wave sums in ascending order —;
 *   logprob_i = (l_i - m) - tk_logf(S).  The order depends neither on the pass width nor on the pass: a row's record is the same in any pass.
 *   Alternatives: the min(n_top, vocab) most probable tokens in the sampler's order — descending logit (+0 above -0), ties to the lower id —: the prefix of
 *   the candidate list the stochastic chain draws from on an unmasked row.  The first one is the greedy pick, except on a row whose maximum is a zero
 *   of both signs (the arg max compares floats and takes the lower id).
 *   Limits: n_top -1 = off, 0 = the produced id only, 1 .. 20 = that many alternatives; vocabularies of at most 65536 tokens.
 * Out of scope: the prompt's tokens ("echo"), the rows of tk_mi355x_llm_forward_verify, the pipeline (tk_mi355x_pipe_*) path. ---- */
#define TK_MI355X_LOGPROB_MAX_TOP 20
/* one produced token's record.  n_top = the count of alternatives actually filled (min(asked, vocab)); entries past it are not written */
typedef struct {
    float logprob; /* of the produced id */
    int32_t n_top;
    int32_t top_ids[TK_MI355X_LOGPROB_MAX_TOP];
    float top_logprobs[TK_MI355X_LOGPROB_MAX_TOP];
} tk_mi355x_token_logprob_t;
/* the runner's setting: -1 off (the default), 0 .. 20 on.  Anything else: TK_ERROR_INVALID_ARGUMENT, the previous setting kept.  Takes effect from the
 * next sampled token.  A runner with log-probabilities on keeps running ahead (csrc/llm/tk_llm_batcher.h: the record rides with the id); lookup
 * decoding does nothing while they are on unless its scope has TK_MI355X_LOOKUP_LOGPROBS.  Prefix cache, context shift and grammar are unaffected; the token stream is the one the runner emits with
 * the setting off */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_runner_set_logprobs(struct tk_llm_runner_s* runner, int32_t n_top);
/* the record of the id the last prepare_generation / generate_next_token (or add_tool_response) sampled — the id the NEXT generate_next_token hands out
 * as a piece, or finds to be EOS or the end of a tool call.  TK_ERROR_INVALID_STATE, `out` untouched: the setting is off, or nothing has been sampled
 * since it was switched on */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_runner_last_logprobs(struct tk_llm_runner_s* runner, tk_mi355x_token_logprob_t* out);
/* tk_mi355x_llm_forward_adjusted plus the records: n_top [nrows] per row, records [nrows]; sampling and adjust may be NULL.  Records of rows with
 * n_top = -1 come back as the caller left them, and so do the entries of a record past its filled count.  A pass with every n_top = -1 is the pass
 * tk_mi355x_llm_forward_adjusted runs.  An n_top outside [-1, 20], or a vocabulary above 65536 with a row that asks: TK_ERROR_INVALID_ARGUMENT, nothing
 * enqueued */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_forward_logprobs(tk_mi355x_llm_session_t* s, int nrows, const int32_t* seq, const int32_t* pos,
                                                                   const int32_t* tok, const tk_mi355x_sampling_t* sampling,
                                                                   const tk_mi355x_logit_adjust_t* adjust, const int32_t* n_top, float* logits, int32_t* ids,
                                                                   tk_mi355x_token_logprob_t* records);
/* the kernel alone on host arrays (tests), tk_mi355x_logit_adjust_probe's contract: logits = `rows` rows of `cols` floats `ld` apart (n_logits floats in
 * all), ids [rows] the chosen id of every row, n_top [rows], records [rows] IN/OUT.  device >= 0: ONE production launch (k_token_logprobs) on that
 * device, the records read back whole — what the kernel did not write is what the caller put there.  device < 0: the same row function in a host loop,
 * no GPU touched.  Everything is validated before anything is launched; TK_ERROR_INVALID_ARGUMENT with nothing written: rows outside
 * [1, tk_mi355x_llm_max_rows()], cols outside [1, 65536], ld < cols, logits too short (n_logits < (rows - 1) * ld + cols), an id outside [0, cols), an
 * n_top outside [-1, 20], a live row (n_top >= 0) that holds a NaN or +inf logit or no finite logit at all */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_token_logprobs_probe(int device, int32_t rows, int32_t cols, int32_t ld, const float* logits, int64_t n_logits,
                                                                   const int32_t* ids, const int32_t* n_top, tk_mi355x_token_logprob_t* records);
/* stand-alone timing of that launch (tools/time_token_logprobs.py): rows x cols generated logits, every row with the same n_top (0 .. 20); `iters`
 * launches after a warm-up, device events around them; average ms of one */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_time_token_logprobs(int device, int32_t rows, int32_t cols, int32_t n_top, int32_t iters, float* avg_ms);
/* KV cache import / export: positions [pos0, pos0 + n_pos) of one (layer, sequence) as IEEE f16 bits, host arrays laid out
 * [position][kv head][head_dim] (what llama.cpp's llama_state_seq_* moves for one sequence; the reference clears the cache per prompt,
 * src/ai_models/tk_runner_streaming.c:31, so it has no counterpart there).  Restores a saved prompt prefix; the parity tests use it to put
 * the attention launch at any context length in one decode step.  Synchronous. */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_session_kv_write(tk_mi355x_llm_session_t* s, int layer, int seq, int pos0, int n_pos,
                                                                   const uint16_t* k, const uint16_t* v);
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_session_kv_read(tk_mi355x_llm_session_t* s, int layer, int seq, int pos0, int n_pos,
                                                                  uint16_t* k, uint16_t* v);
/* rows [pos0, pos0 + n_pos) of sequence src_seq copied onto the same rows of dst_seq (src_seq != dst_seq) in every layer, on the device: one
 * launch of the prefix cache's copy kernel.  Synchronous. */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_session_kv_copy(tk_mi355x_llm_session_t* s, int src_seq, int dst_seq, int pos0, int n_pos);
/* stand-alone timing of that copy (tools/time_kv_copy.py): rows [0, n_pos) of sequence 0 onto sequences 1 .. n_dst as ONE kernel launch and as the
 * form it replaces, a hipMemcpy2DAsync per (destination, layer, K | V), alternating on the session's stream, device events around each; average ms
 * of `iters` rounds after a warm-up; bytes = read + written by one round of either form */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_time_kv_copy(tk_mi355x_llm_session_t* s, int n_pos, int n_dst, int iters, float* kernel_ms,
                                                               float* memcpy_ms, double* bytes);
/* ---- context shift (csrc/common/tk_kv_shift.h; opt-in; include/tk/ABI_NOTES.md): what llama.cpp's hosts do when a context fills — keep the first
 * n_keep tokens, drop half of the rest, move the surviving cache rows down and re-rotate their keys to the new positions. ---- */
/* rows [p0, p1) of sequence seq become rows [p0 + delta, p1 + delta) in every layer, KV head and both caches: values are copied bit for bit, every key
 * pair (a, b) becomes f16(fma(b, s, a c)), f16(fma(-a, s, b c)) with c, s = the session's RoPE table at row -delta (a second f16 rounding of the key,
 * as llama.cpp's K-shift on an f16 cache).  One launch, synchronous.  Valid: 0 <= p0 < p1 <= max_ctx, delta < 0, p0 + delta >= 0, seq a sequence of the
 * session; anything else is TK_ERROR_INVALID_ARGUMENT and nothing is launched.  Source and destination may overlap.  Rows outside the destination
 * range keep their bits — the stale tail [p1 + delta, p1) included — and so does every other sequence.  TK_ERROR_NOT_IMPLEMENTED: head_dim % 8 != 0 */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_session_kv_shift(tk_mi355x_llm_session_t* s, int seq, int p0, int p1, int delta);
/* stand-alone timing of that launch (tools/time_kv_shift.py): `iters` launches after a warm-up, device events around them; average ms of one, bytes
 * read + written by one */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_time_kv_shift(tk_mi355x_llm_session_t* s, int seq, int p0, int p1, int delta, int iters, float* avg_ms,
                                                                double* bytes);
/* the same move on host arrays (tests), tk_mi355x_logit_adjust_probe's contract: kcache / vcache are IN/OUT, in the cache layout
 * [n_layer][max_seq][n_kv_head][max_ctx][head_dim] f16 bits for the geometry given; rope_cos / rope_sin are [max_ctx][head_dim / 2] as the caller
 * gives them.  device >= 0: ONE production launch on that device, the arrays read back whole.  device < 0: the same per-row function in a host loop,
 * no GPU touched.  Everything is validated before any device is touched: a NULL array, head_dim not a multiple of 8 (or above 256), a move the
 * session entry refuses, or more than 2^31 cache elements are TK_ERROR_INVALID_ARGUMENT with the arrays untouched */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_kv_shift_probe(int device, int32_t n_layer, int32_t max_seq, int32_t n_kv_head, int32_t max_ctx, int32_t head_dim,
                                                             uint16_t* kcache, uint16_t* vcache, const float* rope_cos, const float* rope_sin, int32_t seq,
                                                             int32_t p0, int32_t p1, int32_t delta);
/* the runner's policy, OFF by default (off: generate_next_token ends at the end of the context and a tool response that does not fit fails, as the
 * reference does).  on = 1: when generate_next_token would stop because n_past + 1 >= n_ctx, or add_tool_response's tokens would not fit, the runner
 * applies llama.cpp's rule ONCE — n_left = n_past - n_keep, n_discard = n_left / 2, rows [n_keep + n_discard, n_past) move by -n_discard,
 * n_past -= n_discard — and goes on.  n_keep >= 0, or -1 = the token count of the last prepare_generation (llama.cpp's --keep -1), resolved when the
 * shift happens.  If n_discard == 0, or a tool response still does not fit after one shift, the call ends exactly as with the policy off and
 * nothing has moved.  prepare_generation with a prompt longer than the context fails as before.  The penalty window, the grammar state, the
 * sampling counter and tool_call_text are untouched by a shift.  Takes effect from the next call.  n_keep < -1: TK_ERROR_INVALID_ARGUMENT.
 * Two failures a host may want to tell apart.  A device error in the move itself: generate_next_token returns NULL, as at the end of a generation,
 * with the error detail set (tk_error_get_detail; it is empty after a normal end) and context_shifts unchanged; add_tool_response returns
 * TK_ERROR_INFERENCE_FAILED with that detail.  A shift that succeeded followed by a pass that failed: the rows HAVE moved, n_past is the reduced
 * one and context_shifts counts the shift — the runner's state is that of a shifted context whose next token was not computed. */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_runner_set_context_shift(struct tk_llm_runner_s* runner, int on, int32_t n_keep);
/* shifts made, and rows dropped by them in total, since the last prepare_generation */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_runner_context_shifts(struct tk_llm_runner_s* runner, int32_t* shifts, int64_t* discarded);
/* ---- lookup decoding (csrc/llm/tk_lookup.h; opt-in; include/tk/ABI_NOTES.md): llama.cpp's lookup / n-gram speculation and the hosted APIs'
 * "predicted outputs" for a GREEDY runner.  The runner drafts the ids that follow its pending one from a prediction its host gave it, then from its
 * own context, feeds the pending id and the drafts as consecutive positions of one pass and keeps the drafts the model's own arg max confirms: one
 * stream of the weights yields several tokens, and the tokens are exactly the ones the runner emits with lookup off. ---- */
/* the draft rule alone (no GPU).  ctx [n_ctx]: the prompt and every id sampled so far, the pending one last; pred [n_pred]: the prediction (may be
 * empty).  For n = ngram_max down to ngram_min (n <= n_ctx), s = the last n ids of ctx: first the prediction — the smallest j with
 * pred[j .. j + n) == s and j + n < n_pred, drafts pred[j + n ..) — then the context — the largest j with j + n <= n_ctx - 1 and ctx[j .. j + n) == s,
 * drafts ctx[j + n ..) — at most n_draft ids, cut at the end of the source; the first hit wins.  Returns the draft count (out: room for n_draft),
 * 0 when nothing matches; -1: n_draft outside [0, 15], not 1 <= ngram_min <= ngram_max <= 8, a negative count or a missing array */
TK_API int tk_mi355x_lookup_draft(const int32_t* ctx, int n_ctx, const int32_t* pred, int n_pred, int ngram_min, int ngram_max, int n_draft, int32_t* out);
/* the accept rule alone (no GPU).  toks [n]: what a verify pass fed (toks[0] the pending id, the drafts behind it); picks [n]: the arg max of every
 * row.  m = the number of leading drafts the picks confirm (picks[i] == toks[i + 1] for all i < m), cut so that picks[m] is the first pick equal to
 * eos.  out_ids (room for n) = picks[0 .. m]; returns m + 1; -1: n < 1 or a missing array */
TK_API int tk_mi355x_lookup_accept(const int32_t* toks, const int32_t* picks, int n, int32_t eos, int32_t* out_ids);
/* the verify pass on a session: nrows <= tk_mi355x_llm_max_rows() greedy, unmasked, unadjusted rows; the rows of each sequence stand at consecutive
 * ascending positions and are contiguous in the pass; the head runs on ALL rows: picks [nrows] = the arg max of every row, logits [nrows][vocab]
 * optional.  form: the attention of the pass — 0 k_attention per row, 2 k_attention_prefill's tiles, 4 the run form of the long-context attention
 * (k_qkv_rope_append, then k_att_scores_long's run variant, k_att_pv_chain, k_att_pv_join; at most 8 rows, head_dim 64 or 128, a session whose
 * max_ctx exceeds 512), -1 the session's choice (tk_mi355x_attention_plan_verify).  The three forms are bit-identical.  Rows that break the rule
 * above or a form that does not apply: TK_ERROR_INVALID_ARGUMENT, nothing enqueued */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_forward_verify(tk_mi355x_llm_session_t* s, int nrows, const int32_t* seq, const int32_t* pos,
                                                                 const int32_t* tok, int form, float* logits, int32_t* picks);
/* n_draft = 0 (off, the default) .. 15 drafts per pass; 1 <= ngram_min <= ngram_max <= 8.  Anything else: TK_ERROR_INVALID_ARGUMENT, the previous
 * setting kept.  Lookup does nothing — the runner submits exactly what it does with lookup off — while the runner has a temperature, a grammar mask,
 * penalties, a logit bias, or log-probabilities on, unless tk_mi355x_llm_runner_set_lookup_scope covers every such condition.  Takes effect from the
 * next pass */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_runner_set_lookup(struct tk_llm_runner_s* runner, int32_t n_draft, int32_t ngram_min, int32_t ngram_max);
/* the host's prediction of the reply (copied): at most 4096 ids, each inside the vocabulary; n = 0 clears it.  It survives prepare_generation.
 * Anything else: TK_ERROR_INVALID_ARGUMENT, the previous prediction kept */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_runner_set_prediction(struct tk_llm_runner_s* runner, const int32_t* ids, int32_t n);
/* since the last prepare_generation: passes that carried at least one draft, drafts fed, drafts accepted */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_runner_lookup_stats(struct tk_llm_runner_s* runner, uint64_t* verify_passes, uint64_t* drafted,
                                                                      uint64_t* accepted);
/* the scope of lookup decoding (csrc/llm/tk_lookup_scope.h; opt-in): under which of the four conditions above a runner with lookup on still drafts.
 * The default, 0, is the behaviour described at tk_mi355x_llm_runner_set_lookup.  A runner drafts while it has a temperature, a grammar mask, penalties
 * or a bias, or log-probabilities on iff the bit of EVERY condition that currently holds is set; one missing bit makes it inactive.  Row i of its verify
 * pass then samples under the tables a one-row pass at that position would have had — the chain with counter c + i, the mask of a copy of the grammar
 * state after the pending id and drafts 0 .. i - 1 (the drafts are cut in front of the first one the state refuses and of the first one that would
 * complete the grammar), the penalty window after them, the runner's n_top — so the ids, the records (tk_mi355x_llm_runner_last_logprobs is valid for
 * every id), the tool-call text, the counter and the token at which the runner ends or shifts are those of the runner with lookup off.  Unknown bits:
 * TK_ERROR_INVALID_ARGUMENT, the previous scope kept.  Takes effect from the next pass */
#define TK_MI355X_LOOKUP_SAMPLED 1u
#define TK_MI355X_LOOKUP_GRAMMAR 2u
#define TK_MI355X_LOOKUP_ADJUSTED 4u
#define TK_MI355X_LOOKUP_LOGPROBS 8u
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_runner_set_lookup_scope(struct tk_llm_runner_s* runner, uint32_t flags);
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_runner_get_lookup_scope(struct tk_llm_runner_s* runner, uint32_t* flags);
/* diagnostic (tools/time_lookup.py): host milliseconds since the last prepare_generation spent cutting the drafts under the grammar and building
 * the per-row masks of the runner's verify requests, and spent in the verify requests themselves (queueing, the pass, the wake-up) */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_runner_lookup_host_ms(struct tk_llm_runner_s* runner, double* masks_ms, double* requests_ms);
/* one sampling pass with all four optional per-row tables: masks [nrows] pointers, NULL = that row is unmasked, else (vocab + 31) / 32 words whose bit t
 * says token t may be picked; sampling, adjust, n_top / records as tk_mi355x_llm_forward_logprobs takes them; each table may be NULL.  The rows may be
 * several positions of one sequence: when the rows of each sequence stand at consecutive ascending positions and are contiguous in the pass, and some
 * sequence appears more than once, the pass takes the attention tk_mi355x_llm_forward_verify(form -1) takes for them — the run form of the long-context
 * attention where tk_mi355x_attention_plan_verify names kernel 4 — and every form gives the same bits.  This is the verify pass of a runner whose
 * lookup scope is not 0.  A row outside the session, an adjustment or n_top outside its limits, sampling parameters out of range, a row that asks for a
 * record without `records`: TK_ERROR_INVALID_ARGUMENT, nothing enqueued */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_forward_rows(tk_mi355x_llm_session_t* s, int nrows, const int32_t* seq, const int32_t* pos,
                                                               const int32_t* tok, const uint32_t* const* masks, const tk_mi355x_sampling_t* sampling,
                                                               const tk_mi355x_logit_adjust_t* adjust, const int32_t* n_top, float* logits, int32_t* picks,
                                                               tk_mi355x_token_logprob_t* records);
/* diagnostic: the form key (csrc/llm/tk_pass_form.h, tk_pass_form_key) of the last pass the session ran through tk_mi355x_llm_forward* /
 * _forward_verify, -1 before the first.  With the head the key is 5 + 4 * attention + 2 * adjusted + with records; attention 4 is the run form */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_session_last_pass_key(tk_mi355x_llm_session_t* session, int* key);
/* equal-length prompts for sequences 0..nseq-1; first_tokens[nseq] optional */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_prefill(tk_mi355x_llm_session_t* s, int nseq, int n_prompt, const int32_t* tokens,
                                                          int32_t* first_tokens);
/* greedy decode of n_steps tokens for rows 0..nrows-1, hipGraph replay; out_tokens[n_steps][tk_mi355x_llm_max_rows()] */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_decode(tk_mi355x_llm_session_t* s, int nrows, int n_steps, int32_t* out_tokens,
                                                         float* ms_per_step);
/* ---- the LLM layer-sharded over GPUs, stage hand-off inside the library (BASELINE configs[4]; what is sharded is the reference's
 * llama_decode call, src/ai_models/tk_runner_streaming.c:34,77).  Stage `stage` of `n_stages` runs layers [layer0, layer1) of every pass on its
 * session's GPU; the [rows, d_model] residual stream is stored by the producer's last kernel straight into the consumer's device mailbox (mapped
 * with hipIpc across processes — one process per GPU — or by pointer inside one process: peer memory over xGMI), the last stage samples and
 * returns the ids to stage 0 the same way.  No host synchronisation, host copy or collective per pass; a stage's decode step is one captured
 * hipGraph.  payload_f16 = 0: the stream crosses as exact fp32 (tokens and logits bit-identical to one GPU); 1: IEEE f16, half the bytes, the
 * stream rounded once per boundary.  Every device-side wait is bounded (20 s; $TK_MI355X_PIPE_TIMEOUT_S seconds when set at create time):
 * after a timeout every later wait of the stage returns at once, tk_mi355x_pipe_sync returns TK_ERROR_TIMEOUT and the pipe stays failed —
 * pass / decode / sync keep failing until it is destroyed and re-created (its sequence numbers no longer agree with its neighbours').
 * The mailbox is fine-grained device memory (peer writes while kernels poll; $TK_MI355X_PIPE_COARSE=1: plain hipMalloc, one-device A/B only).
 * Any number of generations may run on one set of pipes: a pass with host-given tokens first discards the ids the previous generation left in
 * the id mailbox; a decode() needs a sampling pass (head != 0) before it.
 * All stages must enqueue the same passes in the same order.  csrc/llm/tk_llm_pipe.h has the protocol and the coherence argument. ---- */
typedef struct tk_mi355x_pipe_s tk_mi355x_pipe_t;
typedef struct { uint8_t ipc[64]; uint64_t bytes; int32_t device; int32_t pid; } tk_mi355x_pipe_handle_t; /* plain bytes: move them between processes any way */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_pipe_create(tk_mi355x_pipe_t** out, tk_mi355x_llm_session_t* s, int stage, int n_stages, int layer0, int layer1,
                                                          int payload_f16, tk_mi355x_pipe_handle_t* my_handle);
TK_API void tk_mi355x_pipe_destroy(tk_mi355x_pipe_t** p);
/* the mailboxes of stage (stage + 1) % n and (stage - 1 + n) % n, from the processes that own them */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_pipe_connect(tk_mi355x_pipe_t* p, const tk_mi355x_pipe_handle_t* next, const tk_mi355x_pipe_handle_t* prev);
/* the same for stages created in this process (several GPUs driven by one process, or the tests' two stages on one GPU) */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_pipe_connect_local(tk_mi355x_pipe_t* p, tk_mi355x_pipe_t* next, tk_mi355x_pipe_t* prev);
/* The collective form of the same hand-off (ncclSend / ncclRecv; north_star: "RCCL over xGMI only for the LLM shard"): the stages
 * form one RCCL communicator — tk_mi355x_pipe_rccl_unique_id in ONE process (128 plain bytes, moved to the others any way), then
 * tk_mi355x_pipe_connect_rccl in every stage's process INSTEAD of tk_mi355x_pipe_connect — and every boundary is an ncclSend of the exact fp32
 * stream on the producer's stream matched by an ncclRecv on the consumer's; ids return to stage 0 the same way.  One GPU per stage: with fewer
 * than two visible devices, or two stages on one device, the call FAILS (TK_ERROR_GPU_DEVICE_NOT_FOUND) — it never falls back to the
 * mailboxes.  Decode steps are launched eagerly.  pass / decode / sync are used as with the mailbox transport and give the same tokens. */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_pipe_rccl_unique_id(uint8_t out[128]);
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_pipe_connect_rccl(tk_mi355x_pipe_t* p, const uint8_t unique_id[128]);
/* enqueue one pass (returns at once).  tok: stage 0 only; NULL = feed the ids the last stage sampled for these rows.  head != 0: the last stage
 * samples and returns the ids to stage 0; every stage's device-side positions then stand one past the rows' (a decode loop may follow). */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_pipe_pass(tk_mi355x_pipe_t* p, int nrows, const int32_t* seq, const int32_t* pos, const int32_t* tok, int head);
/* enqueue n_steps greedy decode steps for the rows of the last sampling pass: n_steps replays of this stage's captured pass */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_pipe_decode(tk_mi355x_pipe_t* p, int nrows, int n_steps);
/* wait for everything enqueued.  out_tokens [n_steps][tk_mi355x_llm_max_rows()] (optional): on the last stage the ids sampled at each decode step,
 * on stage 0 the ids fed at each step (the first one = the token the prompt's sampling pass produced) */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_pipe_sync(tk_mi355x_pipe_t* p, int32_t* out_tokens, int n_steps);

/* HIP-event timing of one GEMV launch on the session stream: which = 0 gate+up, 1 down, 2 qkv, 3 lm_head, 4 o */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_time_gemv(tk_mi355x_llm_session_t* s, int layer, int which, int nrows, int iters, float* avg_ms,
                                                            double* algorithmic_bytes);

/* HIP-event timing of the decode attention launch (k_attention) at nrows rows whose sequences hold ctx cached positions; kv_bytes =
 * the K / V bytes one launch must read once */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_time_attention(tk_mi355x_llm_session_t* s, int nrows, int ctx, int iters, float* avg_ms,
                                                                 double* kv_bytes);

/* which attention launch a pass of `nrows` rows takes on `device` (the choice depends on its CU count): out = {kernel, query heads per
 * workgroup, positions per ring slot / resident chunk, ring slots}; kernel 0 = k_attention (ring of chunks), 1 = k_attention_narrow (<= one
 * workgroup per CU, the context resident in LDS), 2 = k_attention_prefill (fused == 0 only: 16 rows of a sequence per workgroup on the fp32
 * matrix pipe, taken by passes that reach position 128 or beyond; the other three numbers describe the k_attention form that shorter contexts
 * take and that TK_MI355X_NO_PREFILL_ATT=1 puts back everywhere — the two forms are bit-identical).  fused != 0: a decode
 * pass (every sequence once), else a pass that holds several positions of a sequence (prompt chunks).  The parity
 * tests assert the instantiation they exercise from this answer (csrc/llm/tk_llm_kernels.hip: tk_attention_plan).
 * kernel 5 = k_attention_far: what stands in for kernels 0 and 1 in a session whose max_ctx is beyond tk_mi355x_attention_resident_limit (or beyond
 * $TK_MI355X_ATT_RESIDENT_MAX=<positions>, for tests and A/B timing): the same (row, block of query heads) workgroups and ring, no score row
 * in LDS — keys streamed twice, values once; a fused pass gets a k_qkv_rope_append launch in front.  Bit-identical to the others.
 * device < 0 selects none: the answer is for the thread's current device, and for a 256-CU one on a host without a GPU. */
TK_API int tk_mi355x_device_cu_count(int device); /* compute units of a HIP device (256 on an MI355X), -1 when there is no such device */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_attention_plan(int device, int nrows, int n_head, int n_kv_head, int head_dim, int max_ctx, int fused, int32_t out[4]);
/* host only, no device: the largest max_ctx at which a session of this head geometry still keeps its score rows in LDS (kernels 0 and 1) — 8192
 * for 32 / 8 / 128, 9216 for 32 / 8 / 64; 0 for a geometry that is none.  Sessions above it run kernel 5 in their place. */
TK_API int tk_mi355x_attention_resident_limit(int n_head, int n_kv_head, int head_dim);
/* the same for a pass whose highest position is `top_position` (a session picks per pass from the positions it is handed): kernel 3 = the
 * long-context decode form (fused != 0; 1 .. 4 rows from position 512, 5 .. 8 rows from 768: k_att_scores_long +
 * k_att_pv_chain + k_att_pv_join — scores over (row, KV head, 64-position block) workgroups, one PV chain per (row, head, class) wave — instead
 * of one latency chain per pair of heads; $TK_MI355X_NO_LONG_ATT=1 keeps the fused kernels), kernel 2 only from position 128 on.  All forms
 * are bit-identical. */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_attention_plan_at(int device, int nrows, int n_head, int n_kv_head, int head_dim, int max_ctx, int fused,
                                                                int top_position, int32_t out[4]);
/* the same for a verify pass (tk_mi355x_llm_forward_verify, form -1) of nrows rows whose highest position is top_position: kernel 4 = the run form of
 * the long-context attention where it is chosen (profiles/lookup_decoding.txt), else kernel 2 from position 128, else kernel 0; the other three
 * numbers as tk_mi355x_attention_plan(fused = 0) gives them */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_attention_plan_verify(int device, int nrows, int n_head, int n_kv_head, int head_dim, int max_ctx,
                                                                    int top_position, int32_t out[4]);
/* read-only: how many passes (and timing loops) the session has recorded into a hipGraph so far.  A session records one graph per (form of a pass,
 * row count) at first use and replays it from then on; $TK_MI355X_NO_GRAPH=1 records none */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_session_graph_captures(tk_mi355x_llm_session_t* session, uint64_t* n);

/* ---- tool-call grammar (GBNF) — the sampling constraint of tk_llm_runner_prepare_generation(..., use_tool_grammar = true)
 * (reference: src/ai_models/grammars/tool_call.gbnf via llama.cpp's grammar sampler, tk_runner_lifecycle.c:59,
 * tk_runner_streaming.c:44-48,69-75).  gbnf == NULL selects the built-in tool-call grammar.  No GPU involved. ---- */
/* how many leading bytes of `text` the grammar accepts, and whether the grammar is complete after them */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_grammar_check(const char* gbnf, const char* text, int32_t* n_accepted, int32_t* complete);
/* allowed[b] = 1 when byte b may follow `prefix` (which must itself be accepted) */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_grammar_next_bytes(const char* gbnf, const char* prefix, uint8_t allowed[256], int32_t* complete);
/* ---- grammar masks built on the device; a grammar per runner (csrc/common/tk_grammar_walk.h) ---- */
/* The allowed-token mask of a grammar state, built by k_grammar_mask inside the runner's pass instead of by the host's trie walk: off (0, the default) or
 * on (1).  Off: the runner submits exactly what it always did.  On: every masked row of the runner — the sampled row of a prompt or a token, and each row
 * of a scoped lookup verify request — carries its grammar state; the bits are exact (bit for bit the host's).  A state that does not fit the image's
 * caps, a grammar without an image, and a runner whose session holds 8 other grammars already, take the host mask, row by row.  A token whose walk
 * exceeds a cap is written as forbidden and counted: the runner then discards that request's result and submits it once more with host masks, so the
 * ids it emits are the ids of the setting off in every case */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_runner_set_device_mask(struct tk_llm_runner_s* runner, int on);
/* since the last prepare_generation: mask rows built on the device, built on the host, and requests submitted again because of an undecided token */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_runner_mask_stats(struct tk_llm_runner_s* runner, uint64_t* device_rows, uint64_t* host_rows, uint64_t* redone_requests);
/* The runner's grammar becomes `gbnf` (llama.cpp server's `grammar` field); NULL restores the tool-call grammar loaded at create.  It is armed by
 * prepare_generation(use_tool_grammar = true) as before; the completion sentinel and tool_call_text behave as before.  A text that does not parse:
 * TK_ERROR_INVALID_ARGUMENT, the parser's message in the error detail, the grammar unchanged.  While a generation is in progress:
 * TK_ERROR_INVALID_STATE.  Works with the device mask on and off */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_runner_set_grammar(struct tk_llm_runner_s* runner, const char* gbnf);
/* k_grammar_mask alone on host arrays (tests), tk_mi355x_token_logprobs_probe's contract.  n_rows mask rows; row r is the state after the grammar
 * accepted prefixes[r], or is off when prefixes[r] is NULL (its bits and its count stay as given).  The vocabulary: offsets [vocab + 1] ascending from 0
 * into `pieces`; an empty piece is never allowed; eos (-1: none) is allowed iff the state is complete, whatever its piece.  bits [n_rows][(vocab + 31) /
 * 32] IN/OUT; undecided [n_rows] receives, for every live row, the number of tokens whose walk exceeded a cap (written 0).  device >= 0: ONE production
 * launch over the live rows, bits read back whole.  device < 0: the same walk in a host loop, no GPU touched.  Everything is validated before a device is
 * touched; TK_ERROR_INVALID_ARGUMENT with nothing written: n_rows outside [1, tk_mi355x_llm_max_rows()], vocab outside [1, 2^20], eos outside
 * [-1, vocab), offsets that do not start at 0, descend or pass 2^26, a prefix the grammar does not accept, a state or grammar without an image;
 * TK_ERROR_CONFIG_PARSE_FAILED: the grammar does not parse */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_grammar_mask_probe(int device, const char* gbnf, int32_t n_rows, const char* const* prefixes, const uint8_t* pieces,
                                                                 const uint32_t* offsets, int32_t vocab, int32_t eos, uint32_t* bits, int32_t* undecided);
/* timing (tools/time_grammar_mask.py): n_rows equal states after `prefix`; device_ms = state upload + launch, the average of `iters` rounds between two
 * events; host_ms = the trie walk it replaces for ONE row, in the same process */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_time_grammar_mask(int device, const char* gbnf, const char* prefix, int32_t n_rows, const uint8_t* pieces,
                                                                const uint32_t* offsets, int32_t vocab, int32_t eos, int32_t iters, float* device_ms, float* host_ms);
/* text accepted by the grammar in the current generation: the tool call to read after tk_llm_runner_generate_next_token
 * returned the sentinel (const char*)1; valid until the next prepare_generation */
struct tk_llm_runner_s;
TK_API const char* tk_mi355x_llm_runner_tool_call_text(struct tk_llm_runner_s* runner);

/* test hook for the two exact fp32 GEMMs: C[M][N] = act(A[M][K] W[N][K]^T + bias) + residual on host buffers, once through the LDS-staged
 * kernel (k_gemm_f32 / k_gemm_f32_big) into c_staged and once through the tiled kernel (csrc/nn/tk_gemm_tiled.h: weights as f32 tiles, or
 * as f16 tiles with f16-rounded activations when f16 != 0) into c_tiled.  K must be a multiple of 128.  bias / residual may be NULL;
 * act: 0 none, 1 SiLU, 2 GELU, 3 sigmoid. */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_gemm_pair(int device, int M, int N, int K, const float* a, const float* w, const float* bias,
                                                        const float* residual, int act, int f16, float* c_staged, float* c_tiled);

/* test hook for the perception GEMM launcher (csrc/nn/tk_nn_kernels: tk_launch_gemm): ONE launch described by plain numbers and host arrays,
 * so that every kernel and instantiation the launcher can take — the element-wise fallbacks, [K][N] weights, the two-level batch, implicit
 * im2col, pitches wider than the extent, f16 B, the opt-in split-f16 contraction — is reachable at shapes no network sends.
 * The fields mirror the launcher's descriptor (csrc/common/tk_gemm_desc.h) one to one.  a / b / bias / residual / c are host arrays of
 * n_a / n_b / n_bias / n_residual / n_c ELEMENTS (b: uint16 f16 bits when b_f16 != 0, float otherwise; bias and residual may be NULL with
 * count 0); each is copied into a device allocation of exactly that size, A and B a_offset / b_offset elements into theirs (the only way to
 * a base that is not 16-byte aligned).  c is IN/OUT: its content is uploaded before the launch and the whole array read back after it, so
 * columns n >= N inside the pitch, rows >= M and the gaps between batch members come back as the caller left them.
 * Every address the descriptor can reach is checked against those counts first: anything outside, a negative extent, pitch or stride, a C
 * pitch below N or an unknown act is TK_ERROR_INVALID_ARGUMENT and nothing is launched; so is a descriptor the launcher itself refuses
 * (kernel = -1: an implicit-im2col form with [K][N] weights (b_kn != 0: its kernels read B as [N][K] only), f16 weights, or without 16-byte
 * groups — channels, pixel pitch, K or ldb no multiple of 4, a base off 16 bytes, K not whole rows of taps).
 * kernel (out) is the launcher's own answer, tk_gemm_kernel_of: family * 1000 + IM * 100 + PATH * 10 + NT with family 0 k_gemm_f32,
 * 1 k_gemm_f32_tall, 2 k_gemm_f32_big, 3 k_gemm_h3_tall, 4 k_gemm_h3_big; IM 1 = implicit im2col; PATH the operand loaders' instantiation
 * (0 element-wise fallbacks, 1 [N][K] and 2 [K][N] 16-byte groups); NT the 32-column accumulators per wave of the tall kernels (0 elsewhere).
 * device < 0: validate and report `kernel` only — no device is touched (the answer then assumes 16-byte aligned allocations, which is what
 * the device allocator returns). */
typedef struct {
    int32_t M, N, K, lda, ldb, ldc, ldr, b_kn, act;
    float alpha;
    int32_t batch, batch_inner;
    int64_t sA, sB, sC, sR, sA2, sB2, sC2, sR2;
    int32_t b_f16;
    int32_t im_C, im_H, im_W, im_ldx, im_kw, im_stride, im_pad, im_Ho, im_Wo;
    int32_t fast;
    int32_t a_offset, b_offset;
    int32_t kernel; /* out */
    const float* a; const void* b; const float* bias; const float* residual; float* c;
    int64_t n_a, n_b, n_bias, n_residual, n_c;
} tk_mi355x_gemm_probe_t;
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_gemm_probe(int device, tk_mi355x_gemm_probe_t* p);

/* test hook for the fused split-f16 attention (csrc/nn/tk_nn_kernels: tk_launch_attention_h3): ONE launch over host arrays.  q and out
 * [B] sequences q_bstride floats apart, each [Tq] rows of pitch d; k and v [B] x [Tk] rows of pitch d, kv_bstride apart; head h reads and writes
 * columns [64 h, 64 h + 64).  n_q counts q's and out's floats, n_kv k's and v's.  out is IN/OUT like the GEMM probe's c: rows >= Tq and the
 * floats between sequences keep the caller's content.  Arrays too small for the geometry, or a geometry the launcher refuses (d != 64 nh, a
 * stride that is not a multiple of 4), are TK_ERROR_INVALID_ARGUMENT: nothing is launched and out is not written. */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_attention_h3_probe(int device, int B, int nh, int Tq, int Tk, int64_t q_bstride, int64_t kv_bstride, int d, float scale,
                                                                 const float* q, const float* k, const float* v, int64_t n_q, int64_t n_kv, float* out);

/* test hook for the five token-selection kernels: ONE launch of tk_launch_argmax (kind 0: k_argmax — greedy, greedy under per-row masks,
 * stochastic through the canonical sampler), tk_launch_argmax_rows (1), tk_launch_pick_rows (2) or tk_launch_pick_rows_filtered (3) on host
 * arrays, so that crafted logit rows (ties, -inf, signed zeros, any vocabulary size) reach each kernel alone.
 * logits: [rows] rows of `cols` floats, `ld` floats apart (n_logits floats in all; kind 0 reads packed rows: ld == cols).
 * kind 0: masks (optional) = n_masks bit masks of (cols + 31) / 32 words each (bit i & 31 of word i >> 5 = token i allowed), allow_row (optional)
 *   [rows] = the row's mask index or -1; samp (optional, IN/OUT) [rows]: temperature > 0 samples the row and adds one to its counter;
 *   tok / pos / nsteps (optional, IN/OUT) [rows]; hist (optional, IN/OUT) n_hist ints, row r's token goes to hist[nsteps[r] * hist_stride + r]
 *   (hist needs nsteps).
 * kinds 1-3: tok [rows] is required; temperature / seed / counter0 are the pick's generator (row r draws with counter0 + r; kind 1 ignores
 *   them), logprob (optional, IN/OUT) [rows] asks for the log-probabilities (kind 1: must be NULL).
 * kind 3: suppress [cols] (non-zero = never sampled), state (IN/OUT) [rows][8] as tk_launch_pick_rows_filtered documents it, beg / eot / tid0.
 * Every IN/OUT array is uploaded before the launch and read back whole after it: what the kernel must not touch comes back as the caller
 * left it.  Checked before anything is launched (TK_ERROR_INVALID_ARGUMENT): rows outside [1, tk_mi355x_llm_max_rows()] (kind 0) or
 * [1, 4096]; cols < 1; ld < cols (kind 0: ld != cols); logits too short; a mask index outside [-1, n_masks); cols > 65536 with any sampled
 * row or with kind 3 (the sampler's ids have 16 bits, the filter's LDS mask 2048 words); a temperature that is negative or not finite; hist
 * too small for nsteps (or nsteps negative, hist_stride < rows); kind 3: beg / eot / tid0 outside the vocabulary, a live row with no allowed
 * token or a NaN logit (the kernel would read logits[0x7fffffff]), counters in state outside [0, 2^24].
 * device < 0: validate only — no device is touched. */
enum { TK_MI355X_PICK_ARGMAX = 0, TK_MI355X_PICK_ARGMAX_ROWS = 1, TK_MI355X_PICK_ROWS = 2, TK_MI355X_PICK_ROWS_FILTERED = 3 };
typedef struct {
    int32_t kind, rows, cols, ld;
    const float* logits;
    int64_t n_logits;
    const uint32_t* masks;
    const int32_t* allow_row;
    int32_t n_masks, hist_stride;
    tk_mi355x_sampling_t* samp;
    int32_t *tok, *pos, *nsteps, *hist;
    int64_t n_hist;
    float temperature;
    uint32_t counter0;
    uint64_t seed;
    float* logprob;
    const uint8_t* suppress;
    int32_t* state;
    int32_t beg, eot, tid0, reserved;
} tk_mi355x_token_pick_probe_t;
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_token_pick_probe(int device, tk_mi355x_token_pick_probe_t* p);

/* test hook for the logit adjustment, the contract of tk_mi355x_token_pick_probe: ONE launch of k_logit_adjust (tk_launch_logit_adjust) on logits
 * [rows][cols] (IN/OUT, packed, n_logits floats in all, read back whole), adjust [rows].  Everything is validated before anything is launched
 * (TK_ERROR_INVALID_ARGUMENT, logits untouched): rows outside [1, tk_mi355x_llm_max_rows()], cols outside [1, 2^24], n_logits < rows * cols, and
 * every limit of tk_mi355x_logit_adjust_t for every row.  device < 0: the same per-row function in a host loop, no GPU touched */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_logit_adjust_probe(int device, int32_t rows, int32_t cols, float* logits, int64_t n_logits,
                                                                 const tk_mi355x_logit_adjust_t* adjust);

/* test hook for Whisper's language detection (csrc/common/tk_lang_pick.h), the contract of tk_mi355x_token_pick_probe: ONE launch of k_lang_pick
 * (tk_launch_lang_pick) on logits [rows] rows `ld` floats apart (n_logits floats in all), language tokens tok0 .. tok0 + n_lang - 1.  auto_row [rows]:
 * != 0 = the row stores its language token tok0 + id into slot[row]; slot [rows] IN/OUT (read back whole: other rows come back as they went in);
 * ids [rows] OUT; probs [rows][n_lang] OUT.  Everything is validated before anything is launched (TK_ERROR_INVALID_ARGUMENT, nothing written): a
 * NULL array, rows outside [1, 4096], n_lang outside [1, 128], tok0 < 0 or tok0 + n_lang > cols, ld < cols, n_logits < (rows - 1) ld + cols, a
 * +inf logit in a language slice.  device < 0: the same per-row function in a host loop, no GPU touched */
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_lang_pick_probe(int device, int32_t rows, int32_t cols, int32_t ld, const float* logits, int64_t n_logits, int32_t tok0,
                                                              int32_t n_lang, const int32_t* auto_row, int32_t* slot, int32_t* ids, float* probs);

/* test hook for the LLM stream's step kernels (csrc/llm/tk_llm_kernels.hip), the contract of tk_mi355x_token_pick_probe: ONE launch of one production
 * launcher on host arrays.  M = tk_mi355x_llm_max_rows().  Every array is given with its count in ELEMENTS; IN/OUT arrays are uploaded before the
 * launch and read back whole after it, so every byte the kernel must not touch comes back as the caller left it.
 *   op             launcher                      arrays
 *   EMBED          tk_launch_embed               embd = vocab rows of K weights as GGUF blocks of `type` (n_embd BYTES), tok [nrows] in [0, vocab),
 *                                                x [nrows][K] IN/OUT
 *   RMSNORM        tk_launch_rmsnorm_q8          x [M][K] IN/OUT, partial [ks][M][n_total] or NULL (ks, n_total then unused), w [K], eps, af_round -> image
 *   RESIDUAL_FOLD  tk_launch_residual_fold       x [M][K] IN/OUT, partial [ks][M][n_total], n_total >= K
 *   SWIGLU         tk_launch_swiglu_q8           partial [ks][M][2 K] (gate | up) -> image; K = d_ff
 *   QUANT          tk_launch_quant_q8            x [nrows][K] (read only), af_round -> image
 *   ROPE_APPEND    tk_launch_qkv_rope_append     partial [ks][M][n_total], n_total >= (n_head + 2 n_kv_head) head_dim, rope_cos / rope_sin
 *                                                [max_ctx][head_dim / 2] (n_rope each) as the caller gives them, seq / pos [nrows], layer -> qbuf
 *                                                [M][n_head head_dim] IN/OUT, kcache / vcache [n_layer][max_seq][n_kv_head][max_ctx][head_dim] f16 bits
 *                                                IN/OUT (n_cache each)
 *   PV_JOIN        tk_launch_att_pv_join         pv_part [nrows][n_head][4][head_dim], l_part [nrows][n_head][4] -> image; K = n_head head_dim
 *   ATT_TILES      tk_launch_att_tiles           seq [nrows] -> tiles [1 + M] IN/OUT
 * The image (RMSNORM, SWIGLU, QUANT, PV_JOIN) comes back RAW, in the layout csrc/llm/tk_llm_layout.h documents, all M rows' worth, IN/OUT: aq
 * [M / 16][K 16] int8, ad [M / 16][K / 256][16] floats, abs [M / 16][K / 256][2][16][8] int8, abs16 the same shape in f16 bits, and af
 * [M / 16][K / 16][4][16][4] floats when af_round is 1 (F16) or 2 (BF16) or af is given (af_round 0: unrounded); af NULL: no float image.
 * Everything is validated before anything is launched; a refusal is TK_ERROR_INVALID_ARGUMENT with nothing written: a NULL array the op needs, a
 * count too small for its geometry, nrows outside [1, M], ks outside [1, 8], K < 256 or no multiple of 256 (EMBED: of `type`'s block too), K or
 * n_total above 65536, n_total % 4, a (n_head, n_kv_head, head_dim) that a model refuses (PV_JOIN: head_dim 64 or 128 with n_head a multiple of
 * 256 / head_dim), seq / pos / layer / tok outside their arrays, a `type` that is no token_embd type, af_round outside [0, 2], and a launch whose
 * dynamic LDS exceeds what its kernel is opted into (RMSNORM: K > 40704).  device < 0: validate only, no device is touched.
 * The twins run one operation in its two production forms on the same inputs, in one call, and return both results.  wblocks: raw GGUF blocks of
 * wtype (Q4_K or Q6_K), wrows x K weights (n_wblocks BYTES); y_a / y_b [ks][M][wrows] IN/OUT: the mat-vec's K-split slabs of form a / form b.
 *   FUSED_NORM     a: tk_launch_rmsnorm_q8 (x [M][K] IN/OUT, partial [fks][M][n_total] or NULL, w, eps) then a plain tk_launch_gemv;
 *                  b: tk_launch_gemv with fuse = 1 on the caller's x, its updated rows into x_b [M][K] IN/OUT
 *   FUSED_SWIGLU   a: tk_launch_swiglu_q8 (partial [fks][M][2 K]) then a plain tk_launch_gemv; b: tk_launch_gemv with fuse = 2
 *                  both: nrows <= 2, wrows a multiple of 64, and what tk_gemv_fuses_producer asks (K % (512 ks) == 0, the image inside the LDS opt-in)
 *   WIDE_SWIGLU    x [nrows][K] quantised by tk_launch_quant_q8; wblocks = gate [wrows][K] then up [wrows][K]; a: tk_launch_gemv with swiglu = 1 then
 *                  tk_launch_quant_q8 -> the image (aq, ad, abs, abs16 of wrows columns); b: the plain gate | up launch then tk_launch_swiglu_q8 -> the
 *                  image aq_b, ad_b, abs_b, abs16_b (the counts of the first); nrows >= 193 (where a pass takes form a), wrows a multiple of 256 */
enum {
    TK_MI355X_STEP_EMBED = 0, TK_MI355X_STEP_RMSNORM = 1, TK_MI355X_STEP_RESIDUAL_FOLD = 2, TK_MI355X_STEP_SWIGLU = 3, TK_MI355X_STEP_QUANT = 4,
    TK_MI355X_STEP_ROPE_APPEND = 5, TK_MI355X_STEP_PV_JOIN = 6, TK_MI355X_STEP_ATT_TILES = 7,
    TK_MI355X_STEP_FUSED_NORM = 8, TK_MI355X_STEP_FUSED_SWIGLU = 9, TK_MI355X_STEP_WIDE_SWIGLU = 10
};
typedef struct tk_mi355x_llm_step_probe_s {
    int32_t op, nrows, K, ks, n_total, af_round, type, vocab;
    int32_t n_head, n_kv_head, head_dim, n_layer, max_seq, max_ctx, layer;
    float eps;
    float* x;
    const float *partial, *w;
    const void* embd;
    const int32_t *tok, *seq, *pos;
    const float *rope_cos, *rope_sin;
    float* qbuf;
    uint16_t *kcache, *vcache;
    const float *pv_part, *l_part;
    int32_t* tiles;
    int8_t* aq;
    float* ad;
    int8_t* abs;
    uint16_t* abs16;
    float* af;
    int64_t n_x, n_partial, n_w, n_embd, n_rows /* tok, seq, pos */, n_rope, n_qbuf, n_cache, n_pv, n_l, n_tiles, n_aq, n_ad, n_abs, n_abs16, n_af;
    /* the twins */
    const void* wblocks;
    float *y_a, *y_b, *x_b;
    int8_t* aq_b;
    float* ad_b;
    int8_t* abs_b;
    uint16_t* abs16_b;
    int64_t n_wblocks, n_y, n_xb;
    int32_t wtype, wrows, fks, reserved;
} tk_mi355x_llm_step_probe_t;
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_llm_step_probe(int device, tk_mi355x_llm_step_probe_t* p);

/* test hook for the perception streams' row and layout kernels (csrc/nn/tk_nn_kernels): ONE launch of one launcher on host arrays, so that
 * shapes no network sends (pitches wider than the extent, odd sizes around the kernels' 256 / 2048 thresholds, unaligned bases, rows that are
 * no multiple of 16) reach each kernel alone.  The contract is the GEMM probe's: a / b / c / idx / pos_idx are inputs of n_a / n_b / n_c /
 * n_idx / n_idx ELEMENTS; y (n_y floats) and img (n_img floats, optional) are IN/OUT: uploaded before the launch, read back whole after it, so
 * every float the kernel must not touch comes back as the caller left it.  a is placed a_offset floats and y y_offset floats into their
 * device allocations (0..64): the only way to a base that is not 16-byte aligned.  Every address the launch can reach is computed from the
 * geometry and checked against the counts first; anything outside, an extent < 1, a pitch below the extent, a stride < 1, a negative pad, a
 * window wider than the padded input, or anything the launcher itself refuses is TK_ERROR_INVALID_ARGUMENT with nothing launched.
 *   op                 geometry                                   arrays
 *   CONV_STEM          B H W C ldx | N k stride pad ldy act       a = x [B H W][ldx], b = w [N][k k C], c = bias [N] or NULL, y [B Ho Wo][ldy]
 *   IM2COL             B H W C ldx | k (square) stride pad        a = x, y = col [B Ho Wo][k k C] packed
 *   IM2COL1D           B H(=T) C ldx | k stride pad               a = x [B T][ldx], y = col [B To][k C] packed
 *   MAXPOOL5           B H W C ldx ldy                            a = x, y [B H W][ldy]
 *   UPSAMPLE2X         B H W C ldx ldy                            a = x, y [B 2H 2W][ldy]
 *   COPY_COLS          rows C ldx ldy                             a = x [rows][ldx], y [rows][ldy]
 *   LAYERNORM          rows C(=D) eps                             a = x [rows][D], b = w [D], c = bias [D], y [rows][D], img (optional)
 *                                                                 [ceil(rows / 16) 16][D]: the tiled GEMM's operand image, D % 16 == 0 only
 *   SOFTMAX_ROWS       rows C(=cols) ldy(=ld)                     y [rows][ld], in place (a unused)
 *   ADD_ROWS           rows C(=D) add_rows                        y = x [rows][D] in place, a = add [add_rows][D]
 *   EMBED_ROWS         rows C(=D) table_rows pos_rows             a = table [table_rows][D], b = pos [pos_rows][D], idx / pos_idx [rows], y [rows][D];
 *                                                                 every index is checked against table_rows / pos_rows
 *   ATTEND1            B H(=Tk) C(=d) N(=nh) q_bstride kv_bstride a = q [B] rows q_bstride apart, b = k and c = v [B] x [Tk][d], kv_bstride apart, y = out
 *                                                                 like q, img (optional) [ceil(B / 16) 16][d]; with B > 1 q_bstride >= d
 * kernel (out) is the launcher's own choice: ATTEND1 0, or -1 when the launcher refuses (d / nh no multiple of 16 or above 256, more than 60 KiB
 * of LDS: d / nh = 64 admits Tk = 3008 and refuses 3009, 80 is refused; a batch stride that is no multiple of 4); SOFTMAX_ROWS 0 the three-pass kernel, 1 one block per row out of registers, 2 one wave per row;
 * IM2COL 0 element-wise, 1 16-byte groups; CONV_STEM 0, or -1 when the launcher refuses (N != 16, C != 3, k != 3, ldy % 4, y off 16 bytes);
 * every other op 0.  device < 0: validate and report `kernel` only, no device is touched (bases then as the device allocator aligns them). */
enum {
    TK_MI355X_ROW_CONV_STEM = 0, TK_MI355X_ROW_IM2COL = 1, TK_MI355X_ROW_IM2COL1D = 2, TK_MI355X_ROW_MAXPOOL5 = 3, TK_MI355X_ROW_UPSAMPLE2X = 4,
    TK_MI355X_ROW_COPY_COLS = 5, TK_MI355X_ROW_LAYERNORM = 6, TK_MI355X_ROW_SOFTMAX_ROWS = 7, TK_MI355X_ROW_ADD_ROWS = 8, TK_MI355X_ROW_EMBED_ROWS = 9,
    TK_MI355X_ROW_ATTEND1 = 10
};
typedef struct {
    int32_t op;
    int32_t B, H, W, C, ldx, ldy;   /* images */
    int32_t rows;                   /* row ops */
    int32_t N, k, stride, pad, act; /* conv_stem / im2col / im2col1d; act: 0 none, 1 SiLU */
    int32_t add_rows, table_rows, pos_rows;
    float eps;
    int32_t a_offset, y_offset;
    int32_t kernel;                 /* out */
    const float *a, *b, *c;
    const int32_t *idx, *pos_idx;
    float *y, *img;
    int64_t n_a, n_b, n_c, n_idx, n_y, n_img;
    int64_t q_bstride, kv_bstride;  /* attend1 */
} tk_mi355x_nn_row_probe_t;
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_nn_row_probe(int device, tk_mi355x_nn_row_probe_t* p);

/* test hook for the kernels at the two ends of the perception streams — sensor bytes to the networks' first tensor, the networks' last tensor to
 * what the cortex reads: ONE launch of one production launcher on host arrays (DEPTH_METRIC: the min / max launch and then the metric launch,
 * as the depth engine issues them).  The contract is tk_mi355x_nn_row_probe's: a / b / c are inputs of n_a / n_b / n_c ELEMENTS of the type
 * the table names; y (n_y elements) and y2 (n_y2) are IN/OUT: uploaded before the launch, read back whole after it, so every element the kernel
 * must not touch comes back as the caller left it.  Every address the launch can reach is computed from the geometry and checked against the
 * counts first; anything outside, an extent < 1, a pitch below the row, an array the op does not use that is not NULL with a count of 0, or
 * anything the launcher itself refuses is TK_ERROR_INVALID_ARGUMENT with nothing launched.
 *   op                 geometry                                   arrays
 *   FRAMES             B n_samples pcm_stride n_total T           a = pcm int16 [B] rows pcm_stride apart (n_samples read of each), b = window [400],
 *                                                                 y [B][T][400]; 1 <= n_samples <= n_total, pcm_stride >= n_samples, n_total > 200 and
 *                                                                 160 (T - 1) + 199 <= 2 (n_total - 1): one reflection at either end stays inside
 *   POWER              rows nb                                    a = ri [rows][2 nb] (re | im), y [rows][nb]
 *   LOGMEL_FINISH      B per_b                                    y = mel [B][per_b], in place
 *   VAD_HEAD           rows(=n) hidden                            a = hid [n][hidden], b = w2 [hidden], c = b2 [1], y = prob [n]
 *   PREPROCESS         in_w in_h in_stride bpp out_w out_h nhwc   a = frame uint8, rows in_stride BYTES apart (the last row may end at its last pixel's third
 *                      mean std_dev scale                         byte), y [3][out_h][out_w] or, nhwc = 1, [out_h][out_w][3]; in_w, in_h >= 2, bpp 3 or 4,
 *                                                                 in_stride >= in_w bpp.  scale == 1/255 or 0 selects k_preprocess, any other finite value
 *                                                                 k_preprocess_scaled, exactly as tk_kernels_preprocess_image chooses
 *   DEPTH_MINMAX       n                                          a = x [n], y = {min, max}
 *   DEPTH_METRIC       n min_depth max_depth                      a = x [n], y = metric [n], y2 = {min, max} as the first launch left them
 *   POSTPROCESS_DEPTH  width height scale shift                   a = raw [height][width], y [height][width] (tk_kernels_postprocess_depth_map)
 *   DEPTH_TO_POINTS    width height fx fy cx cy                   a = depth [height][width], y [height][width][3] (tk_kernels_depth_to_point_cloud);
 *                                                                 fx or fy == 0 is the launcher's refusal
 *   BOX_ATTRIBUTES     in_w in_h (the frame) rows(=boxes)         a = frame uint8 [in_h][in_w][3] packed, b = rects int32 [boxes][4] = {x, y, w, h},
 *                                                                 y int32 [boxes][2] = {colour bin, door closed}; the hook (not the kernel) asks |x|, |y| <= 2^30,
 *                                                                 |w|, |h| <= 2^20 and an area of at most 2^24 pixels, so that no launch runs long
 * kernel (out): PREPROCESS 0 k_preprocess, 1 k_preprocess_scaled; POSTPROCESS_DEPTH and DEPTH_TO_POINTS the number of 256-thread blocks of the
 * launch (capped by the launcher: a map of more elements takes further trips of the grid-stride loop); -1 a refusal; every other op 0.
 * device < 0: validate and report `kernel` only, no device is touched. */
enum {
    TK_MI355X_EDGE_FRAMES = 0, TK_MI355X_EDGE_POWER = 1, TK_MI355X_EDGE_LOGMEL_FINISH = 2, TK_MI355X_EDGE_VAD_HEAD = 3, TK_MI355X_EDGE_PREPROCESS = 4,
    TK_MI355X_EDGE_DEPTH_MINMAX = 5, TK_MI355X_EDGE_DEPTH_METRIC = 6, TK_MI355X_EDGE_POSTPROCESS_DEPTH = 7, TK_MI355X_EDGE_DEPTH_TO_POINTS = 8,
    TK_MI355X_EDGE_BOX_ATTRIBUTES = 9
};
typedef struct {
    int32_t op;
    int32_t B, n_samples, pcm_stride, n_total, T;           /* FRAMES; B also LOGMEL_FINISH */
    int32_t rows, nb, per_b, hidden;
    int32_t in_w, in_h, in_stride, bpp, out_w, out_h, nhwc; /* PREPROCESS; in_w, in_h also BOX_ATTRIBUTES */
    int32_t width, height;                                  /* POSTPROCESS_DEPTH, DEPTH_TO_POINTS */
    int32_t kernel;                                         /* out */
    int64_t n;                                              /* DEPTH_MINMAX, DEPTH_METRIC */
    float mean[3], std_dev[3], scale, shift;
    float min_depth, max_depth, fx, fy, cx, cy;
    const void *a, *b, *c;
    void *y, *y2;
    int64_t n_a, n_b, n_c, n_y, n_y2;
} tk_mi355x_edge_probe_t;
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_edge_probe(int device, tk_mi355x_edge_probe_t* p);

/* test hook for the detector's post-processing kernels (csrc/vision/tk_vision_engine.hip), ONE decode + rank + mask + scan sequence on host arrays:
 * kind 0: three raw head maps head[i] = [B][H_i W_i][ld[i]] floats (n_head[i] in all) with ld[i] >= 64 + nc and H_i = in_h / s, W_i = in_w / s
 *         for s = 8, 16, 32 (in_w, in_h multiples of 32; n_anchors must be the three grids' total): k_yolo_decode, then tk_launch_yolo_post;
 * kind 1: out = [B][4 + nc][n_anchors] decoded boxes and class probabilities (n_out floats), any n_anchors >= 1: k_yolo_decode_out per frame,
 *         then the same post launches.
 * IN/OUT, each uploaded before the launches and read back whole after them, so stale content of an earlier call can be planted and whatever the
 * kernels must not touch comes back as it was: cand [B][n_anchors] records, order [B][2048] anchor ids by (score desc, anchor asc), n_cand [B],
 * mask [B][2048][32] 64-bit words (optional: NULL leaves the device matrix filled with 0xFF bytes), kept [B][500] records, n_kept [B].  The
 * counts must be exactly those sizes.  A record is tk_mi355x_box_t (cls = -1 in cand: not a candidate).
 * TK_ERROR_INVALID_ARGUMENT with nothing launched: B outside [1, 256], nc outside [1, 4096], n_anchors outside [1, 2^20], a pitch below
 * 64 + nc, an array too small for its geometry or of the wrong count.  device < 0: validate only. */
typedef struct { float x1, y1, x2, y2, score; int32_t cls, anchor; } tk_mi355x_box_t;
typedef struct {
    int32_t kind, B, nc, n_anchors;
    int32_t in_w, in_h;
    int32_t ld[3];
    int32_t reserved;
    float conf, iou;
    const float* head[3];
    int64_t n_head[3];
    const float* out;
    int64_t n_out;
    tk_mi355x_box_t* cand;
    int32_t* order;
    int32_t* n_cand;
    uint64_t* mask;
    tk_mi355x_box_t* kept;
    int32_t* n_kept;
    int64_t cand_count, order_count, n_cand_count, mask_count, kept_count, n_kept_count;
} tk_mi355x_detector_post_probe_t;
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_detector_post_probe(int device, tk_mi355x_detector_post_probe_t* p);

/* test hook for the node-by-node ONNX executor (csrc/nn/tk_onnx_exec): loads `path`, binds the n_feeds float tensors (name, data on the
 * host, rank and dims), runs the graph once and keeps host copies of the n_outputs named float values WITH THE SHAPES THE EXECUTOR
 * PRODUCED.  A refusal (unsupported op / attribute, bad shapes) comes back as an error code with the executor's text as the error
 * detail.  Integer tensors enter a graph only as initialisers; an integer-valued output is an error.  The result is read with the
 * accessors below (i = index into output_names) and released with tk_mi355x_onnx_result_free. */
typedef struct tk_mi355x_onnx_result_s tk_mi355x_onnx_result_t;
TK_API TK_NODISCARD tk_error_code_t tk_mi355x_onnx_run(int device, const char* path, int32_t n_feeds, const char* const* feed_names,
                                                       const float* const* feed_data, const int32_t* feed_ranks, const int64_t* const* feed_dims,
                                                       int32_t n_outputs, const char* const* output_names, tk_mi355x_onnx_result_t** out_result);
TK_API int32_t tk_mi355x_onnx_result_rank(const tk_mi355x_onnx_result_t* r, int32_t i);
TK_API const int64_t* tk_mi355x_onnx_result_dims(const tk_mi355x_onnx_result_t* r, int32_t i);
TK_API const float* tk_mi355x_onnx_result_data(const tk_mi355x_onnx_result_t* r, int32_t i);
TK_API void tk_mi355x_onnx_result_free(tk_mi355x_onnx_result_t** r);

#ifdef __cplusplus
}
#endif
#endif
