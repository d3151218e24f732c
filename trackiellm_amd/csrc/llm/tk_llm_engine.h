/*
 * tk_llm_engine.h — device-resident Mistral-class model + batched decode session.
 *
 * Replaces what the reference obtains from llama.cpp:
 *   model  <-> llama_load_model_from_file            (src/ai_models/tk_model_loader.c:245-251)
 *   session<-> llama_new_context_with_model + KV     (src/ai_models/tk_runner_lifecycle.c:47-51)
 *   forward<-> llama_decode(batch)                   (src/ai_models/tk_runner_streaming.c:34,77)
 * One model is shared by any number of sessions; a session owns a KV cache for `max_seq`
 * sequences and runs up to 16 (sequence, position) rows per pass so that B concurrent
 * cortex cycles read the 4.3 GB of weights once per step.
 */
#ifndef TK_LLM_ENGINE_H
#define TK_LLM_ENGINE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "tk_llm_kernels.h"
#include "tk_pass_form.h"

struct TkLlmHParams {
    int32_t n_layer, d_model, n_head, n_kv_head, head_dim, d_ff, vocab;
    float rms_eps, rope_theta;
    /* K-split plan: part of the canonical summation order shared with the oracle */
    int32_t ks_qkv, ks_o, ks_gateup, ks_down, ks_out;
};

struct TkDevTensor {
    uint8_t* data = nullptr; /* tiles (matrices) or raw f32 / GGUF blocks */
    int type = 0;
    int64_t rows = 0, cols = 0;
    size_t bytes = 0;
};

struct TkLlmLayer {
    TkDevTensor attn_norm, ffn_norm, q, k, v, o, gate, up, down;
};

enum TkLlmTensorId { TK_T_TOKEN_EMBD = 0, TK_T_OUT_NORM = 1, TK_T_OUTPUT = 2 };
enum TkLlmLayerTensorId { TK_L_ATTN_NORM = 0, TK_L_Q, TK_L_K, TK_L_V, TK_L_O, TK_L_FFN_NORM, TK_L_GATE, TK_L_UP, TK_L_DOWN, TK_L_COUNT };

class TkLlmModel {
public:
    TkLlmHParams hp{};
    int device = 0;
    TkDevTensor token_embd, out_norm, output;
    std::vector<TkLlmLayer> layers;
    std::string error;
    size_t weight_bytes = 0; /* bytes a decode step streams (matrices only) */

    ~TkLlmModel();
    /* returns false and sets `error` on failure */
    bool init(const TkLlmHParams& hp, int device);
    /* f16: the fp16 checkpoint recipe (every matrix and the embedding IEEE f16, norms f32) instead of Q4_K_M */
    /* ftype (k-quant checkpoints): llama.cpp's file type 10 Q2_K, 21 Q2_K_S, 11 Q3_K_S, 12 Q3_K_M, 14 Q4_K_S, 15 Q4_K_M, 16 Q5_K_S, 17 Q5_K_M; 7 Q8_0, 2 Q4_0, 8 Q5_0, 25 IQ4_NL, 30 IQ4_XS, 36 TQ1_0, 37 TQ2_0 (recipe_type) */
    bool fill_synthetic(uint64_t seed, bool f16 = false, int ftype = 15);
    /* by tensor type, for the types no file type of fill_synthetic names (Q4_1, Q5_1): every layer matrix and token_embd `type`, output Q6_K, norms F32 */
    bool fill_synthetic_type(uint64_t seed, int type);
    /* by float tensor type (30 BF16 or 0 F32; F16 is fill_synthetic's f16): every matrix and token_embd of that type, the values 0.02 * tk_synth_normal
     * stored through tk_f32_to_bf16 / unconverted; norms F32 */
    bool fill_synthetic_float(uint64_t seed, int type);
    /* the model's float kind: the one float type (F16 / BF16 / F32) among its matrices — layer matrices and output; token_embd is free —, or -1
     * when every matrix is a tiled quantised type.  Sessions of a float model also keep their activations as f32 values rounded through that type
     * (TkActQ8::af).  Two float types among the matrices: install refuses the second, ready() is false; *other (optional) = that second type.
     * except (optional): a tensor left out of the count */
    int float_type(int* other = nullptr, const TkDevTensor* except = nullptr) const;
    /* a LoRA adapter to merge into every matrix it names WHILE that matrix is installed (set before set_tensor / fill_synthetic; tk_lora.h);
     * not owned, only read during those calls */
    const struct TkLoraAdapter* lora = nullptr;
    int lora_merged = 0; /* matrices the adapter changed */
    /* `host_blocks` is the tensor in GGUF layout (F32 for norms) */
    bool set_tensor(int layer, int which, int type, const void* host_blocks, size_t nbytes);
    bool ready() const;
    static int recipe_type(const TkLlmHParams& hp, int layer, int which, int ftype = 15);
    void shape(int layer, int which, int64_t* rows, int64_t* cols) const;

private:
    TkDevTensor* slot(int layer, int which);
    bool install(TkDevTensor* t, int type, int64_t rows, int64_t cols, void* dev_blocks, hipStream_t s, int layer, int which);
    bool fill_synthetic_as(uint64_t seed, int float_type, int ftype);
};

class TkLlmPipe;

class TkLlmSession {
public:
    TkLlmModel* model = nullptr;
    int max_seq = 0, max_ctx = 0;
    std::string error;
    hipStream_t stream = nullptr;

    ~TkLlmSession();
    /* kv_type: TK_KV_F16, or TK_KV_Q8_0 (common/tk_kv_q8.h) — the cache holds ggml Q8_0 blocks of the rows the f16 cache would hold, 17/32 of its
     * bytes.  A Q8_0 session describes every pass as "rope apart + per-row attention" (its TkPassCaps are all false, rope_in_attention is never
     * set): tk_launch_qkv_rope_append_q8, then kernel 6 (k_attention_far over the Q8_0 cache).  kv_read, kv_shift, forward_stage and the kv_copy /
     * kv_shift timing entries are refused on it.  The type is a member that init reads, so that init keeps its three arguments (the scheduler's
     * CPU harness defines it); the four-argument form sets the member first */
    int kv_type = TK_KV_F16;
    bool init(TkLlmModel* m, int max_seq, int max_ctx);
    bool init(TkLlmModel* m, int max_seq, int max_ctx, int kv_type_) { kv_type = kv_type_; return init(m, max_seq, max_ctx); }
    size_t kv_bytes() const; /* bytes of the cache arrays, keys and values */
    /* one pass over nrows <= TK_MAX_ROWS rows (16-row M-tiles); host arrays.  row_masks (optional): row_masks[r] = nullptr or the
     * (vocab + 31) / 32 words whose bit t says token t may be sampled for row r: grammar-constrained greedy sampling, per row, so
     * constrained and unconstrained rows share passes (and the captured graphs).  row_samp (optional): [nrows] sampling state, temp > 0
     * = the reference's default stochastic chain for that row (tk_llm_kernels.h), else greedy.  row_adjust (optional): [nrows] logit bias and
     * repetition penalties per row (common/tk_logit_adjust.h), applied to the row's logits before masks and sampling see them; every row is checked
     * before anything is enqueued.  A pass with at least one non-neutral row uploads the tables and is a form of its own (TkPassForm::adjust: the
     * k_logit_adjust launch); any other pass replays the graphs it always did and uploads nothing.  logits_host of an adjusted row are the ADJUSTED
     * logits.  row_ntop (optional): [nrows] per row -1 = off, 0 .. TK_LOGPROB_MAX_TOP = the log-probability of the row's picked id and that many
     * alternatives (common/tk_token_logprob.h) into records_host[r]; checked before anything is enqueued.  A pass with a row that asks uploads the
     * table, is a form of its own (TkPassForm::logprobs: the k_token_logprobs launch behind the pick) and copies
     * the pass's records back; a record is written as far as it was filled, a row that is off leaves records_host[r] alone; any other pass runs
     * what it always did.  A pass with the head in which some sequence stands at several positions and whose rows keep forward_verify's layout
     * rule takes the attention forward_verify would choose for them (tk_pass_form_rows: the run form of the long attention from
     * tk_verify_run_min_pos on), whatever tables its rows carry: the verify pass of a runner that samples, is masked, adjusted or asks for records */
    bool forward(int nrows, const int32_t* seq, const int32_t* pos, const int32_t* tok, float* logits_host, int32_t* argmax_host,
                 bool lm_head = true, const uint32_t* const* row_masks = nullptr, const TkSampleRow* row_samp = nullptr,
                 const TkLogitAdjust* row_adjust = nullptr, const int32_t* row_ntop = nullptr, TkTokenLogprob* records_host = nullptr);
    /* the verify pass of lookup decoding (tk_lookup.h): up to TK_MAX_ROWS greedy, unmasked, unadjusted rows; the rows of each sequence stand at
     * consecutive ascending positions and are contiguous in the pass; the head runs on ALL rows (picks_host[r] = arg max of row r, logits_host
     * optional).  form: the attention of the pass — 0 k_attention per row, 2 k_attention_prefill's 16-row tiles, 4 the run form of the long-context
     * attention (tk_llm_kernels.h; at most TK_LONG_ATT_MAX_ROWS rows, head_dim 64 or 128, a session whose window can reach TK_LONG_ATT_MIN_POS), all
     * three bit-identical; -1 = the session's choice (tk_verify_form).  A form that does not apply is refused before anything is enqueued
     * (*bad_args, optional, tells that from a device error).  Forms 0 and 2 are the forms of a sampling pass that holds several positions of a
     * sequence and share its graphs; the run form is chosen through this entry only. */
    bool forward_verify(int nrows, const int32_t* seq, const int32_t* pos, const int32_t* tok, int form, float* logits_host, int32_t* picks_host,
                        bool* bad_args = nullptr);
    /* one pipeline stage of a pass: layers [l0, l1) on this GPU.  The first stage starts from `tok` (x_in == nullptr), later stages
     * from the residual stream x_in [nrows][d_model] fp32; every stage but the last writes the stream to x_out; the last one
     * (head == true, l1 == n_layer) samples.  x_on_host: x_in / x_out are host pointers (gloo transport), otherwise device
     * pointers (RCCL transport).  Bit-identical to forward() whatever the split. */
    bool forward_stage(int nrows, const int32_t* seq, const int32_t* pos, const int32_t* tok, const float* x_in, float* x_out, bool x_on_host,
                       int l0, int l1, bool head, int32_t* argmax_host);
    /* prompts of equal length for sequences 0..nseq-1 (tokens[nseq][n_prompt]); leaves row r = sequence r
     * holding the first sampled token so decode() can follow; first_tokens_host[nseq] optional */
    bool prefill(int nseq, int n_prompt, const int32_t* tokens, int32_t* first_tokens_host);
    /* greedy decode loop, on-device feedback, hipGraph replay.  Starts from the rows' current
     * (tok, pos) state left by the previous forward()/decode(); out_tokens[n_steps][nrows].  The loop is unadjusted: its passes are plain
     * forms, and it clears the adjustment descriptors and the log-probability table a previous forward() left as it clears the masks. */
    bool decode(int nrows, int n_steps, int32_t* out_tokens_host);
    bool reset();
    /* KV cache import / export: rows [pos0, pos0 + n_pos) of one (layer, sequence) as f16 bits, host arrays in [position][kv head][dim]
     * order (the cache itself is [layer][sequence][kv head][position][dim]).  Restores a saved prompt prefix without re-running it; the
     * parity tests use it to put an attention launch at any context length in one decode step. */
    bool kv_write(int layer, int seq, int pos0, int n_pos, const uint16_t* k, const uint16_t* v);
    bool kv_read(int layer, int seq, int pos0, int n_pos, uint16_t* k, uint16_t* v);
    /* Q8_0 sessions.  kv_write quantises the f16 rows it is given on the host (tk_kv_q8_row) and uploads; kv_read is refused (the cache's values
     * are not f16 numbers); kv_read_q8 returns the raw rows: int8 values [position][kv head][dim] and scale bits [position][kv head][dim / 32] */
    bool kv_read_q8(int layer, int seq, int pos0, int n_pos, int8_t* kq, uint16_t* kd, int8_t* vq, uint16_t* vd);
    /* rows [pos0, pos0 + n_pos) of sequence src_seq copied onto the same rows of dst_seq (src_seq != dst_seq) in every layer: one launch of
     * k_kv_copy_rows, synchronous.  A cache row at position p depends only on tokens 0 .. p, so a sequence that is to hold the same leading
     * tokens as another can take its rows instead of recomputing them (the prompt prefix cache, tk_llm_batcher.h). */
    bool kv_copy(int src_seq, int dst_seq, int pos0, int n_pos);
    /* the scheduler's form: up to TK_MAX_ROWS copies in one launch on `stream`, not waited for — a forward() that follows on the stream sees the
     * copied rows, and a source row that forward() overwrites is read first.  Descriptors are checked like kv_copy's arguments; no two share a
     * destination and no destination is another one's source (the caller's rule: the kernel copies them in no particular order). */
    bool enqueue_kv_copy(const TkKvCopyDesc* descs, int n);
    /* context shift (common/tk_kv_shift.h): rows [p0, p1) of sequence seq become rows [p0 + delta, p1 + delta), delta < 0, in every layer: values copied,
     * keys re-rotated to their new positions; one launch of k_kv_shift_rows on `stream`, synchronous.  Needs 0 <= p0 < p1 <= max_ctx and
     * p0 + delta >= 0; source and destination may overlap.  Rows outside the destination range keep their bits, the stale tail [p1 + delta, p1)
     * included.  *bad_args (optional) tells a refused argument from a device error */
    bool kv_shift(int seq, int p0, int p1, int delta, bool* bad_args = nullptr);
    /* stand-alone timing of that launch (tools/time_kv_shift.py): the move `iters` times after one untimed launch, device events around them; average
     * ms of one launch, bytes = read + written by one (the two table rows aside) */
    bool time_kv_shift(int seq, int p0, int p1, int delta, int iters, float* avg_ms, double* bytes);
    bool kv_copy_applies() const { return model && model->hp.head_dim % 8 == 0; } /* 16-byte accesses need rows of whole 16-byte words */
    /* per-launch timing of the last decode(): average ms of one step measured with HIP events */
    float last_step_ms = 0.0f;
    /* stand-alone timing of the dominant GEMV (gate/up of layer 0) for bench.py's roofline leg */
    bool time_gemv(int layer, int which, int nrows, int iters, float* avg_ms, double* algo_bytes);
    /* stand-alone timing of the decode attention launch at nrows rows x ctx cached positions, for bench.py's second roofline object */
    bool time_attention(int nrows, int ctx, int iters, float* avg_ms, double* kv_bytes);
    /* stand-alone timing of the prefix cache's copy: rows [0, n_pos) of sequence 0 onto sequences 1 .. n_dst, as ONE k_kv_copy_rows launch and as the
     * form it replaces — a hipMemcpy2DAsync per (destination, layer, K | V) on the same stream — alternating, `iters` times after one untimed round
     * of each, device events around each form; bytes = read + written by one round of either */
    bool time_kv_copy(int n_pos, int n_dst, int iters, float* kernel_ms, float* memcpy_ms, double* bytes);
    /* Grammar masks built on the device (common/tk_grammar_walk.h, k_grammar_mask).  All four are thread-safe and called by the runners
     * (abi/tk_abi_llm.cpp), never by the scheduler: the scheduler hands forward() the host mask pointers it always did, and forward() looks each one up.
     *   install_vocab_image   once per session, at first use: offsets [vocab + 1] and the bytes of the pieces (an empty piece is never allowed)
     *   grammar_slot          the image of a grammar in the session's arena, keyed by its words: the slot of an equal image when there is one, else a
     *                         new one (a slot stays taken while the session lives); -1 = the arena's TK_GRAMMAR_ARENA_SLOTS are taken (such a
     *                         runner keeps building its masks on the host)
     *   attach_grammar_state  the masked row whose host mask pointer is `mask_ptr` gets its mask from `image` (image.grammar = a slot): forward()
     *                         uploads the state images of such rows, runs ONE k_grammar_mask launch for all of them into the compacted rows of d_mask, in
     *                         front of the pass where the host masks are copied, and copies nothing from mask_ptr.  After the pass it reads the
     *                         undecided counts back with the ids
     *   detach_grammar_state  forgets the pointer; *ran = a pass built the mask, *undecided = tokens of it that the walk could not decide (written as
     *                         forbidden: the row may have picked from too small a set) */
    enum { TK_GRAMMAR_ARENA_SLOTS = 8 };
    bool install_vocab_image(const uint32_t* offsets, const uint8_t* pieces, int32_t eos);
    int grammar_slot(const uint32_t* words, size_t n_words, int32_t n_rules, int32_t n_elems, int32_t n_sets, int32_t root);
    bool attach_grammar_state(const uint32_t* mask_ptr, const TkGrammarStateImage& image);
    void detach_grammar_state(const uint32_t* mask_ptr, bool* ran, int32_t* undecided);

private:
    struct GrammarRow { TkGrammarStateImage image; bool ran = false; int32_t undecided = 0; };
    std::mutex gm_mu;                                   /* guards the registry, the arena's keys and the installation */
    std::map<const uint32_t*, GrammarRow> gm_rows;      /* attached states by host mask pointer */
    std::vector<uint32_t> gm_keys[TK_GRAMMAR_ARENA_SLOTS];
    uint32_t* gm_words[TK_GRAMMAR_ARENA_SLOTS] = {};    /* device copies of the grammars' words */
    TkGrammarImage* d_gm_arena = nullptr;               /* [TK_GRAMMAR_ARENA_SLOTS] images with device pointers */
    uint32_t* d_gm_offsets = nullptr;                   /* the vocabulary image */
    uint8_t* d_gm_pieces = nullptr;
    int32_t gm_eos = -1;
    TkGrammarStateImage *d_gm_states = nullptr, *h_gm_states = nullptr; /* [TK_MAX_ROWS] state images of a pass: device array, pinned staging */
    int32_t *d_mask_undecided = nullptr, *h_mask_undecided = nullptr;   /* [TK_MAX_ROWS] per launch row */
    friend class TkLlmPipe; /* tk_llm_pipe.h: a pipeline stage enqueues layer ranges of this session between its hand-off kernels */
    int last_ks_res = 1;    /* slabs of the residual update the last enqueue_range left pending in `partial` */
    /* A pass is described once, as a TkPassForm (tk_pass_form.h; DESIGN.md "The forms of a pass"), by the entry that runs it; these launch what
     * the form says and hold no state of their own about it */
    TkPassCaps pass_caps(int nrows) const;
    void enqueue_pass(int nrows, const TkPassForm& f);
    void enqueue_range(int nrows, int l0, int l1, bool embed, bool fold_out, const TkPassForm& f);
    void enqueue_attention(const TkPassForm& f, const float* qkv_slab, int ks_qkv, int layer, int nrows);
    int enqueue_matmul(const TkDevTensor* const* t, int nseg, int K, int ks, int n_total, const TkActQ8& act, float* out, int nrows);
    /* the pass on the stream: a replay of its graph, recorded at first use (one per (form, row count)) — a host that asks for one token at a time,
     * the reference's runner API, pays one graph launch, not ~260 kernel launches, per token —, or eager launches (TK_MI355X_NO_GRAPH=1) */
    bool launch_pass(const TkPassForm& f, int nrows, bool use_graph);
    hipGraphExec_t capture_pass(const TkPassForm& f, int nrows); /* nullptr: failed, `error` says why */
    hipGraphExec_t graphs[TK_PASS_FORM_KEYS][TK_MAX_ROWS + 1] = {}; /* [tk_pass_form_key][row count] */
    /* THE capture path of the process: `enqueue` recorded from `stream` into *slot (untouched when it holds a graph already), one capture at a time
     * per process.  The stream always leaves capture mode and the graph is always freed; a launcher's refusal (launch_error) or a HIP error
     * leaves *slot null and `error` set ("graph capture of <what> failed: ...").  Counts into n_captures / capture_ms */
    bool capture(hipGraphExec_t* slot, const char* what, const std::function<void()>& enqueue);
    /* the timing entries' loop: warm(), then launch(0 .. iters - 1) recorded into one graph, replayed once untimed and once between two events
     * (TK_MI355X_NO_GRAPH=1: the launches themselves between the events); *avg_ms = one launch */
    bool time_launches(int iters, const std::function<void()>& warm, const std::function<void(int)>& launch, float* avg_ms);
    /* Row plumbing of the host-described entries.  check_pass_rows: 1 <= nrows <= TK_MAX_ROWS and every (sequence, position, token) inside the session
     * (tok may be null: a later pipeline stage); *top = the highest position, *distinct (optional) = no sequence twice.  upload_rows: the rows'
     * tables to the device (d_tok only when given) and the decode history's step counts cleared.  clear_row_tables: the per-row tables an earlier
     * forward() may have left and this pass does not want, each only when it is dirty.  Who clears what:
     *   forward() with the head      uploads or clears all four itself, table by table, as its rows ask
     *   forward() without the head   nothing: no launch of the pass reads a table
     *   forward_verify()             masks, sampling, adjust, logprobs: greedy, unmasked, unadjusted rows, whatever an earlier pass left
     *   forward_stage()              masks, adjust, logprobs; d_samp stays (a stale stochastic row would sample: see DESIGN.md)
     *   decode()                     masks, adjust, logprobs; d_samp stays ON PURPOSE: the loop continues the rows' sampling state
     *   TkLlmPipe::pass / ::decode   masks only: a pipe's session is fed by the pipe alone, which never sets the other three */
    enum { TK_ROWS_MASKS = 1, TK_ROWS_SAMPLING = 2, TK_ROWS_ADJUST = 4, TK_ROWS_LOGPROBS = 8 };
    bool check_pass_rows(int nrows, const int32_t* seq, const int32_t* pos, const int32_t* tok, int* top, bool* distinct);
    bool upload_rows(int nrows, const int32_t* seq, const int32_t* pos, const int32_t* tok);
    bool clear_row_tables(unsigned which);
    uint16_t *kcache = nullptr, *vcache = nullptr;
    TkKvQ8 kvq{}; /* the Q8_0 cache (kcache / vcache stay null) */
    bool refuse_q8(const char* what); /* true (and `error` set) on a Q8_0 session */
    float *x = nullptr, *x2 = nullptr, *qbuf = nullptr, *partial = nullptr, *partial2 = nullptr, *logits = nullptr, *rope_cos = nullptr, *rope_sin = nullptr;
    TkActQ8 act_d{}, act_qd{}, act_ff{};
    int32_t *d_seq = nullptr, *d_pos = nullptr, *d_tok = nullptr, *d_nsteps = nullptr, *d_hist = nullptr;
    uint32_t* d_mask = nullptr;     /* [TK_MAX_ROWS][(vocab + 31) / 32] allowed-token bits of the masked rows of the current pass */
    int32_t* d_mask_row = nullptr;  /* [TK_MAX_ROWS] index into d_mask, -1 = the row samples unconstrained */
    bool mask_rows_dirty = true;    /* d_mask_row holds something other than all -1 */
    TkSampleRow* d_samp = nullptr;  /* [TK_MAX_ROWS] sampling state of the rows of the current pass (temp 0 = greedy); decode() continues from it */
    bool samp_dirty = false;        /* d_samp holds a stochastic row */
    TkKvCopyDesc *d_kvcopy = nullptr, *h_kvcopy = nullptr; /* [TK_MAX_ROWS] descriptors of one k_kv_copy_rows launch: device array, pinned staging */
    /* logit adjustment of the rows of the current pass, at fixed addresses (the graphs hold them): [TK_MAX_ROWS] descriptors, the rows'
     * windows [TK_MAX_ROWS][TK_ADJUST_MAX_RECENT], bias ids and values [TK_MAX_ROWS][TK_ADJUST_MAX_BIAS]; h_adj: one pinned staging block of
     * the four in that order (free again when forward() has waited for the stream) */
    TkAdjustRow* d_adj = nullptr;
    int32_t *d_adj_ids = nullptr, *d_adj_bias_ids = nullptr;
    float* d_adj_bias = nullptr;
    uint8_t* h_adj = nullptr;
    bool adj_dirty = false;   /* d_adj holds a non-neutral descriptor */
    /* log-probabilities of the rows of the current pass, at fixed addresses (the graphs hold them): [TK_MAX_ROWS] n_top per row (-1 = off) and
     * [TK_MAX_ROWS] records; h_lp_rec: pinned, the records of a pass on their way back */
    int32_t* d_lp_ntop = nullptr;
    TkTokenLogprob *d_lp_rec = nullptr, *h_lp_rec = nullptr;
    bool lp_dirty = false;     /* d_lp_ntop holds something other than all -1 */
    std::string launch_error; /* set by enqueue_* when a launcher refuses its arguments (no HIP error is raised for that) */
    int hist_cap = 0;
    bool counted_ = false; /* this session is in the device's count of live decode sessions (tk_attention_note_session) */
    float* d_scores = nullptr; /* [TK_LONG_ATT_MAX_ROWS][n_head][max_ctx], allocated when the window can reach TK_LONG_ATT_MIN_POS */
    int32_t* d_tab = nullptr;                           /* prefill schedule: [3][total rows] = seq, pos, tok */
    int32_t* d_tiles = nullptr;                         /* [1 + TK_MAX_ROWS] 16-row tiles of a multi-position pass (k_att_tiles) */
    size_t tab_cap = 0;
public:
    int last_pass_key = -1;  /* tk_pass_form_key of the last pass forward / forward_verify launched (a diagnostic: which attention a pass took) */
    uint64_t n_captures = 0; /* passes recorded into a graph so far, and the host time that took (diagnostics: TK_MI355X_BATCHER_TRACE) */
    double capture_ms = 0.0;
};

/* one production float matmul (tk_mi355x_llm_matmul_float_probe): w [rows][K] row-major values of `type` (1 F16, 30 BF16, 0 F32), rows = the sum of
 * the nseg <= 3 segments' seg_rows (each a multiple of 16), tiled per segment as install() does; x [nrows][K] through the production image
 * producer (k_quant_q8 with the type's rounding); one tk_launch_gemm_tiled with the segments side by side and K split ks ways; the slabs added
 * in ascending order; y [nrows][rows] on the host */
bool tk_llm_matmul_float_probe(int device, int type, const void* w, int64_t rows, int64_t K, int ks, int nseg, const int32_t* seg_rows, int nrows,
                               const float* x, float* y, std::string& error);

/* one production mat-vec on raw GGUF blocks (tk_mi355x_llm_gemv_probe): repack, Q8_K-quantise x [nrows][K] on the device, the launcher at
 * width nrows, the ks slabs summed in ascending order; y [nrows][rows] on the host */
bool tk_llm_gemv_probe(int device, int type, const void* blocks, int64_t rows, int64_t K, int ks, int nrows, const float* x, float* y,
                       std::string& error);

/* the Q8_0 cache's two production launches on host arrays (tk_mi355x_kv_q8_probe, include/tk/tk_mi355x_ext.h); the caller has validated everything */
struct tk_mi355x_kv_q8_probe_s;
bool tk_llm_kv_q8_probe(int device, const tk_mi355x_kv_q8_probe_s* p, std::string& error);

/* one step launcher on host arrays (tk_mi355x_llm_step_probe, include/tk/tk_mi355x_ext.h): everything validated first, device < 0 validates only */
struct tk_mi355x_llm_step_probe_s;
bool tk_llm_step_probe(int device, tk_mi355x_llm_step_probe_s* p, std::string& error);

/* the repack alone (tk_mi355x_llm_repack_probe): raw GGUF blocks [rows][K / 256 runs] -> the type's tiles (tk_llm_layout.h) on the host.
 * device >= 0: tk_launch_repack there; device < 0: tk_repack_host, the same lane function in a host loop, no GPU touched */
bool tk_llm_repack_probe(int device, int type, const void* blocks, int64_t rows, int64_t K, void* tiles, std::string& error);

#endif
