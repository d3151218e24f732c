/*
 * tk_llm_kernels.h — launch wrappers of the hand-written gfx950 kernels of the LLM stream.
 * Every wrapper only enqueues on `stream` (no allocation, no sync) so a whole decode step
 * can be captured in a hipGraph.
 */
#ifndef TK_LLM_KERNELS_H
#define TK_LLM_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tk_llm_layout.h"

struct TkGemvSeg {
    const uint8_t* tiles; /* device tiles [row_tile][K/256][tile bytes] */
    int type;             /* a k-quant of tk_type_desc_of (common/tk_ggml_blocks.h) */
    int row_tiles;        /* rows / 16; must be a multiple of 4 */
};

struct TkGemvArgs {
    TkGemvSeg seg[3];
    int nseg;
    int K;        /* reduction length, multiple of 256*ks */
    int ks;       /* K-split count: partial sums land in out[ks][16][n_total] */
    int n_total;  /* row pitch of `out`: the sum of rows over all segments of the matrix */
    int col0;     /* column of `out` where segment 0 starts (non-zero when a launch carries only some of the matrix's segments) */
    int nrows;    /* live rows (<= TK_MAX_ROWS); rows 16.. use the second M-tile */
    int swiglu;   /* 1 (only where tk_gemv_fuses_swiglu() says so): seg[0] = gate, seg[1] = up, out = h[nrows][n_total = d_ff] = silu(gate) * up */
    size_t aq_ts, ad_ts, abs_ts; /* M-tile strides of aq (bytes), ad (floats), abs (ints) */
    const int8_t* aq;
    const float* ad;
    const int8_t* abs; /* sub-block sums as (l, h) int8 images: [K/256][2][16][8] */
    const uint16_t* abs16; /* the same sums as two f16 images (sum = 2 hh + ll): [K/256][2][16][8] halves, M-tile stride abs_ts halves */
    float* out;
    /* fuse != 0 (only where tk_gemv_fuses_producer() says so: passes of one or two rows, where a launch boundary costs more than the
     * producer's work repeated in every workgroup): the launch builds its int8 activation image in LDS itself and aq / ad / abs are unused.
     *   1: residual update + RMS norm + Q8 — k_rmsnorm_q8's arithmetic: row = fx_in + (the fks slabs of fslab, ascending; pitch
     *      fn_total; fslab null: none), written once to fx_out (a buffer OTHER than fx_in: other workgroups still read it), norm
     *      weights fw, epsilon feps; K = d_model
     *   2: SwiGLU + Q8 — k_swiglu_q8's arithmetic on the fks slabs of the gate | up projection in fslab ([.][2 K] per row); K = d_ff */
    int fuse;
    const float* fx_in;
    float* fx_out;
    const float* fslab;
    int fks, fn_total;
    const float* fw;
    float feps;
};

struct TkActQ8 { /* quantised-activation buffers for one K */
    int8_t* aq;
    float* ad;
    int8_t* abs; /* (l, h) images of the sub-block sums, 256 B per 256-block */
    uint16_t* abs16; /* (hh, ll) f16 images of the same sums, 512 B per 256-block: the batched kernel's one-MFMA min term */
    size_t aq_ts, ad_ts, abs_ts; /* M-tile strides */
    /* float-weight matrices (F16 / BF16 / F32 checkpoints) consume the activations as f32 values rounded through the weight type — what a CPU
     * engine's matmul does to its f32 input (ggml's vec_dot_type: F16 for F16, BF16 for BF16, none for F32); null when the model has no such
     * matrix */
    float* af;    /* the tiled GEMM's operand image (csrc/nn/tk_gemm_tiled.h): [M-tile][K / 16][4 g][16 rows][4 t] floats, k = 16 j + 4 t + g */
    uint32_t af_ts;   /* floats between M-tiles = 16 K */
    int32_t af_round; /* TkRound (common/tk_exact_math.h): the image's rounding; one per model.  (The two share the eight bytes af_ts had alone) */
};


/* weights */
void tk_launch_synth_blocks(int type, uint64_t seed, uint64_t tensor_id, int64_t nblocks, float scale, void* out, hipStream_t s);
void tk_launch_synth_f32(uint64_t seed, uint64_t tensor_id, int64_t n, float* out, hipStream_t s);
/* W += scale (B A) on a matrix in GGUF layout (a lora_merge type of tk_type_desc_of), quantised back to its own type; A [r][K], B [rows][r] on the device.
 * false: arguments the kernel does not take (type, K % 256, more than 2^31 blocks) */
/* F16 / BF16 / F32 (one value per "block"): the sum is stored through tk_f32_to_f16 / tk_f32_to_bf16 / as it is */
bool tk_launch_lora_merge(int type, void* blocks, int64_t rows, int64_t K, const float* A, const float* B, int r, float scale, hipStream_t s);
void tk_launch_repack(int type, const void* blocks, int64_t rows, int64_t K, uint8_t* tiles, hipStream_t s);
void tk_repack_host(int type, const void* blocks, int64_t rows, int64_t K, uint8_t* tiles); /* the same tiles without a device */

/* step kernels */
void tk_launch_embed(const void* embd, int type /* a token_embd type of tk_type_desc_of */, int D, const int32_t* tok, int nrows, float* x, hipStream_t s);
void tk_launch_synth_f16(uint64_t seed, uint64_t tensor_id, int64_t n, float scale, uint16_t* out, hipStream_t s);
/* scale * tk_synth_normal stored as `type`: TK_TYPE_BF16 through tk_f32_to_bf16 (uint16 out), TK_TYPE_F32 unconverted (float out) */
void tk_launch_synth_float(int type, uint64_t seed, uint64_t tensor_id, int64_t n, float scale, void* out, hipStream_t s);
void tk_launch_rmsnorm_q8(float* x, const float* partial, int ks, int n_total_partial, const float* w, float eps, int D, int nrows,
                          TkActQ8 out, hipStream_t s);
size_t tk_rmsnorm_lds_bytes(int D); /* dynamic LDS of one k_rmsnorm_q8 workgroup */
int tk_llm_max_d_model();           /* the widest d_model whose norm fits the LDS opt-in (a multiple of 256) */
void tk_launch_residual_fold(float* x, const float* partial, int ks, int n_total, int D, int nrows, hipStream_t s);
void tk_launch_gemv(const TkGemvArgs& a, hipStream_t s);
void tk_launch_qkv_rope_append(const float* partial, int ks, int n_total, int n_head, int n_kv_head, int head_dim, const float* rope_cos,
                               const float* rope_sin, const int32_t* seq, const int32_t* pos, int nrows, float* qbuf, uint16_t* kcache,
                               uint16_t* vcache, int layer, int max_seq, int max_ctx, hipStream_t s);
void tk_launch_attention(const float* qbuf, const float* partial, int ks, int n_total, const float* rope_cos, const float* rope_sin,
                         uint16_t* kcache, uint16_t* vcache, const int32_t* seq, const int32_t* pos, int nrows, int n_head, int n_kv_head,
                         int head_dim, int layer, int max_seq, int max_ctx, TkActQ8 out, bool fused, hipStream_t s);
void tk_launch_swiglu_q8(const float* partial, int ks, int FF, int nrows, TkActQ8 out, hipStream_t s);
/* wide passes: the gate | up launch forms h = silu(gate) * up in its epilogue (half the slab bytes written and read back); then only the quantisation is left */
/* rows up to which the norm / SwiGLU producer of a mat-vec launch runs inside it (TkGemvArgs::fuse) */
#define TK_GEMV_FUSE_MAX_ROWS 2
size_t tk_gemv_fused_lds_bytes(int K, int ks, int fuse /* 1 or 2 */); /* dynamic LDS of a mat-vec launch that carries its producer */
bool tk_gemv_fuses_producer(int nrows, int K, int ks, int fks);
bool tk_gemv_fuses_swiglu(int nrows, int ks, int type_gate, int type_up);
void tk_launch_quant_q8(const float* hbuf, int FF, int nrows, TkActQ8 out, hipStream_t s);
#include "../common/tk_sample.h"
/* allow_base / allow_row (both optional): per-row allowed-token bit masks, allow_row[r] = mask index or -1; samp (optional): [nrows] */
void tk_launch_argmax(const float* logits, int vocab, int nrows, const uint32_t* allow_base, const int32_t* allow_row, TkSampleRow* samp, int32_t* tok,
                      int32_t* pos, int32_t* nsteps, int32_t* hist, int hist_stride, hipStream_t s);
#include "../common/tk_logit_adjust.h"
/* logit bias + repetition penalties on logits [nrows][vocab], in place, before tk_launch_argmax: desc [nrows]; ids [nrows][TK_ADJUST_MAX_RECENT] the
 * rows' windows; bias_ids / bias [nrows][TK_ADJUST_MAX_BIAS].  The caller has checked every row with tk_adjust_check: the kernel trusts the ids */
void tk_launch_logit_adjust(float* logits, int vocab, int nrows, const TkAdjustRow* desc, const int32_t* ids, const int32_t* bias_ids, const float* bias, hipStream_t s);
#include "../common/tk_token_logprob.h"
/* log-probability of the picked token and the n_top[r] most probable alternatives of every row with n_top[r] >= 0 (common/tk_token_logprob.h), after
 * tk_launch_argmax on the logits it read: logits [nrows] rows of `vocab` floats `ld` apart; tok [nrows] the picked ids; rec [nrows].  The caller has
 * checked n_top with tk_logprob_check (vocab <= 65536) and tok[r] is a token of the row */
void tk_launch_token_logprobs(const float* logits, int vocab, int ld, int nrows, const int32_t* n_top, const int32_t* tok, TkTokenLogprob* rec, hipStream_t s);
#include "../common/tk_grammar_walk.h"
/* grammar token masks on the device (common/tk_grammar_walk.h): ONE launch for n_rows states.  states [n_rows], each naming its grammar image in
 * grammars[] (device pointers inside) and its row of `mask` ([.][(vocab + 31) / 32] words, every word of such a row written whole); offsets [vocab + 1]
 * and pieces: the vocabulary image; eos (< 0: none) is allowed iff the state is complete; undecided [n_rows], zeroed by the caller, counts the tokens
 * of each state whose walk exceeded a cap (written 0).  The caller vouches for the images: the kernel trusts positions and offsets */
void tk_launch_grammar_mask(const TkGrammarImage* grammars, const TkGrammarStateImage* states, int n_rows, const uint32_t* offsets, const uint8_t* pieces, int vocab,
                            int eos, uint32_t* mask, int32_t* undecided, hipStream_t s);

/* the attention launch a pass takes: kernel 0 = k_attention<gq, fused, head_dim, chunk> (chunk = positions per ring slot, slots = ring depth 2), kernel 1 =
 * k_attention_narrow (gq 2, chunk = positions resident per chunk, the whole context when it fits), kernel 5 = k_attention_far<gq, head_dim, chunk>
 * (the per-row form of a window beyond tk_attention_resident_limit: no score row in LDS; a fused pass gets k_qkv_rope_append in front).
 * far: the window takes the far form wherever a pass takes the per-row one (kernel 2 names the tiled form the session prefers from
 * TK_TILED_ATT_FROM_POS; below it the pass runs kernel 5 when `far`, else 0) */
struct TkAttentionPlan { int kernel, gq, chunk, slots; size_t lds_bytes; bool far; };
/* the widest context window a session may have: RoPE is unscaled, and the 32 k checkpoints this library loads need none up to here */
#define TK_MAX_CONTEXT 32768
/* host only: the largest window whose score rows — one per query head of a KV group — fit a k_attention workgroup's LDS beside a 64-position
 * ring (what TkLlmSession::init refused beyond, before the far form); sessions above it, or above TK_MI355X_ATT_RESIDENT_MAX=<positions>
 * (read where the plan is made; tests and A/B timing), take k_attention_far instead of k_attention and k_attention_narrow */
int tk_attention_resident_limit(int n_head, int n_kv_head, int head_dim);
size_t tk_attention_far_lds_bytes(int gq, int head_dim, int chunk);
/* a decode session on `device` came (+1) or went (-1): with more than one alive the plan prefers forms that share a CU with other streams' launches */
void tk_attention_note_session(int device, int delta);
TkAttentionPlan tk_attention_plan(int nrows, int n_head, int n_kv_head, int head_dim, int max_ctx, bool fused);

/* multi-position passes (prompt chunks): 16 rows of a sequence per workgroup on the fp32 matrix pipe, bit-identical to k_attention's non-fused
 * form.  tiles: 1 + TK_MAX_ROWS ints built by tk_launch_att_tiles from the pass's sequence ids (once per pass); the cache must already hold
 * the pass's own K / V rows (tk_launch_qkv_rope_append) */
bool tk_attention_prefill_applies(int n_head, int n_kv_head, int head_dim);
void tk_launch_att_tiles(const int32_t* seq, int nrows, int32_t* tiles, hipStream_t s);
void tk_launch_attention_prefill(const float* qbuf, const uint16_t* kcache, const uint16_t* vcache, const int32_t* seq, const int32_t* pos,
                                 const int32_t* tiles, int nrows, int n_head, int n_kv_head, int head_dim, int layer, int max_seq, int max_ctx, TkActQ8 out,
                                 hipStream_t s);
/* decode passes of few rows over long contexts: scores spread over (row, KV head, 64-position block) workgroups, then one sequential PV chain per
 * (row, head, class) wave — bit-identical to the fused kernels.  scores: tk_attention_long_scratch_floats() floats; `partial` holds the
 * q | k | v projection's K-split slabs (the launch finishes q / k / v itself and appends this pass's rows to the cache) */
/* by measurement, end to end (profiles/r05_attention_long_ctx.txt): 1 .. 4 rows from position 512, 5 .. 8 rows from 768 (the isolated launch
 * already wins from ~384 at one row; a whole step does not before ~500); at 16 rows the fused kernels' 256 workgroups already cover the chip */
#define TK_LONG_ATT_MAX_ROWS 8
#define TK_LONG_ATT_MIN_POS 512
static inline int tk_long_att_min_pos(int nrows) { return nrows > 4 ? 768 : TK_LONG_ATT_MIN_POS; }
bool tk_attention_long_applies(int nrows, int n_head, int n_kv_head, int head_dim);
size_t tk_attention_long_scratch_floats(int n_head, int head_dim, int max_ctx); /* floats of the `scores` scratch buffer */
void tk_launch_attention_long(const float* partial, int ks, int n_total, const float* rope_cos, const float* rope_sin, uint16_t* kcache, uint16_t* vcache,
                              const int32_t* seq, const int32_t* pos, int nrows, int n_head, int n_kv_head, int head_dim, int layer, int max_seq, int max_ctx,
                              float* scores, TkActQ8 out, hipStream_t s, bool run = false);
/* run = the verify pass of lookup decoding (TkLlmSession::forward_verify): several consecutive positions of a sequence in one pass of at most
 * TK_LONG_ATT_MAX_ROWS rows.  tk_launch_qkv_rope_append has already put the pass's rows into the cache; the scores launch finishes only the queries,
 * stores nothing to the caches and reads key rows <= p from them.  Bit-identical to k_attention's per-row form and to k_attention_prefill.
 * tk_verify_run_min_pos: the top position from which the session prefers the run form to k_attention_prefill for a pass of `nrows` rows.  By
 * measurement on full 7B (profiles/lookup_decoding.txt): at 2, 5 and 8 rows the run form wins every round at every context timed, 256 .. 4 000
 * (2.6 against 3.3 ms per pass at 256, 3.5 against 13.9 ms at 4 000); 256 is the lowest context that was timed, so the choice starts there */
static inline int tk_verify_run_min_pos(int nrows) { (void)nrows; return 256; }
/* prompt prefix cache (tk_llm_batcher.h): rows [p0, p0 + n) of sequence src_seq copied onto the same rows of dst_seq in every layer, KV head and
 * both caches, all `ndesc` <= TK_MAX_ROWS descriptors (a device array) in one launch.  src_seq != dst_seq; no two descriptors of a launch share a
 * destination, and no destination of a launch is another descriptor's source.  max_n = the largest n among them (sizes the grid together with the
 * device's CU count).  ndesc = 0 launches one idle workgroup.  false: arguments the kernel does not take (head_dim % 8 != 0) or a failed launch */
struct TkKvCopyDesc { int32_t src_seq, dst_seq, p0, n; };
bool tk_launch_kv_copy_rows(const TkKvCopyDesc* desc, int ndesc, int max_n, uint16_t* kcache, uint16_t* vcache, int n_layer, int n_kv_head, int head_dim, int max_seq,
                            int max_ctx, hipStream_t s);
#include "../common/tk_kv_q8.h"
/* The Q8_0 KV cache (common/tk_kv_q8.h): int8 values [layer][seq][kv_head][max_ctx][head_dim] and f16 scales [layer][seq][kv_head][max_ctx][head_dim / 32],
 * for K and for V.  head_dim % 64 == 0 (every geometry TkLlmModel::init accepts), so value rows are whole 16-byte words and scale rows 4-byte ones */
struct TkKvQ8 { int8_t* kq; uint16_t* kd; int8_t* vq; uint16_t* vd; };
/* k_qkv_rope_append's Q8_0 form: the same K-split sums, RoPE and f16 rounding, then the block quantiser; q goes to qbuf unchanged */
void tk_launch_qkv_rope_append_q8(const float* partial, int ks, int n_total, int n_head, int n_kv_head, int head_dim, const float* rope_cos, const float* rope_sin,
                                  const int32_t* seq, const int32_t* pos, int nrows, float* qbuf, TkKvQ8 cache, int layer, int max_seq, int max_ctx, hipStream_t s);
/* kernel 6 of the attention plan: k_attention_far over a Q8_0 cache (the rows appended by tk_launch_qkv_rope_append_q8 before), every pass of a
 * Q8_0 session.  o32 (optional, the probe's): the quotients [nrows][n_head * head_dim] before quantize_chunk8 as well.  false: a geometry the
 * kernel does not take (nothing is launched) */
TkAttentionPlan tk_attention_plan_q8(int nrows, int n_head, int n_kv_head, int head_dim);
bool tk_launch_attention_q8(const float* qbuf, TkKvQ8 cache, const int32_t* seq, const int32_t* pos, int nrows, int n_head, int n_kv_head, int head_dim, int layer,
                            int max_seq, int max_ctx, TkActQ8 out, float* o32, hipStream_t s);
/* tk_launch_kv_copy_rows on a Q8_0 cache: values and scales of both caches, bit for bit, in one launch */
bool tk_launch_kv_copy_rows_q8(const TkKvCopyDesc* desc, int ndesc, int max_n, TkKvQ8 cache, int n_layer, int n_kv_head, int head_dim, int max_seq, int max_ctx,
                               hipStream_t s);
#include "../common/tk_kv_shift.h"
/* context shift (common/tk_kv_shift.h): rows [p0, p1) of sequence m.seq moved to [p0 + delta, p1 + delta), delta < 0, in every layer, KV head and both
 * caches in one launch; V copied, K re-rotated by delta positions with rows -delta of rope_cos / rope_sin ([max_ctx][head_dim / 2]).  Source and
 * destination may overlap.  A move with p1 <= p0 launches one idle workgroup.  false: a move or geometry the kernel does not take (nothing is
 * launched) or a failed launch */
bool tk_launch_kv_shift_rows(const TkKvShiftDesc& m, uint16_t* kcache, uint16_t* vcache, const float* rope_cos, const float* rope_sin, int n_layer, int n_kv_head,
                             int head_dim, int max_seq, int max_ctx, hipStream_t s);
/* the long-context form's last launch alone: the four classes of every head joined, divided, quantised (head_dim 64 or 128, n_head a multiple of 256 / head_dim) */
void tk_launch_att_pv_join(const float* pv_part, const float* l_part, int nrows, int n_head, int head_dim, TkActQ8 out, hipStream_t s);
size_t tk_gemv_lds_bytes(int K, int ks, int mtiles);
/* dynamic LDS of one k_attention workgroup; must stay below 160 KiB (the session checks it against its max_ctx) */
size_t tk_attention_lds_bytes(int gq, int head_dim, int max_ctx, int chunk /* positions per ring slot: 32, 64 or 128 */);
/* opts every kernel of this file into 160 KiB of dynamic LDS on `device` (which must be the calling thread's current device); idempotent,
 * thread-safe; returns nullptr or an error string.  Sessions call it at creation: launches never change function attributes. */
const char* tk_llm_prepare_device(int device);

#endif
