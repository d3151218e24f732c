/*
 * tk_llm_batcher.h — continuous batching behind the reference's one-sequence-per-runner API.
 *
 * The reference gives every tk_llm_runner_t its own llama context and decodes one token per call on the caller's thread
 * (src/ai_models/tk_runner_streaming.c:57-85, contract src/ai_models/tk_model_runner.h:164-181).  Behind the same calls, all runners
 * created on one model share ONE decode session here: a runner owns a sequence slot of the session's KV cache; prepare_generation /
 * generate_next_token / add_tool_response enqueue their (sequence, position, token) rows and block; one scheduler thread per model
 * coalesces whatever is ready — prompt chunks and single decode rows of different runners alike — into passes of up to 256 rows, so
 * K host threads that each drive "their" runner read the 4.3 GB of weights once per step instead of K times.
 * A row's result does not depend on which other rows share its pass (bit-identical logits at any pass width:
 * tests/test_llm_gpu.py::test_full_7b_pass_width_invariance), so a runner sees exactly the tokens it would see alone.
 *
 * Run-ahead.  generate_next_token is a host round trip per token: the owner wakes, turns the id into a piece, returns to its caller and
 * comes back with the id it was just given — while the GPU waits.  So when a sequence's sampled id has been handed to its owner, the
 * scheduler feeds that id at the next position in its very next pass WITHOUT waiting for the owner (one position ahead, never more); the
 * owner's next call then finds its row in flight or already done.  Not for rows sampled under a grammar mask (the next mask depends on
 * the accepted token), not for rows sampled under a non-neutral logit adjustment (the next window of the repetition penalties depends on the
 * accepted token, and the owner may change its bias list; this holds from the first sampled token on, whose window is still empty), not for a slot
 * whose runner has lookup decoding on (the row after a sampled id is the first row of the owner's next verify pass, which carries drafts that only the
 * owner can make: such a slot submits with `hold`, and a verify request never plans a row ahead), not after EOS, not at the end of the context.
 * A runner with log-probabilities on (submit's n_top >= 0, common/tk_token_logprob.h) KEEPS running ahead: the record of a row depends on nothing its
 * owner decides, so the run-ahead row of such a slot is planned with the slot's n_top, its record is held in the Ahead entry and handed over with the
 * id; an owner that comes back with another n_top than the row was planned with has gone another way, like one that comes back with another token.  An owner that comes back with something else (a tool response, a
 * new prompt) or not at all costs one wasted row: the cache row it wrote is overwritten before anything attends to it, because positions
 * are fed in order.  Tokens are unchanged — a row's result does not depend on when or with whom it runs.
 *
 * Prompt prefix cache (set_prefix_cache, OFF by default: with it off every prompt is fed from position 0, as the reference does after its
 * llama_kv_cache_clear, src/ai_models/tk_runner_streaming.c:31).  A cache row at position p depends only on tokens 0 .. p, and a row's bits do
 * not depend on its pass, so a row that is already in the cache for the same leading tokens is the row a recomputation would write.
 *   Records.  Per slot, the token id whose K/V row sits at each position (rec_).  Only the scheduler thread writes them, and only after a pass
 *     has completed: every row (slot, pos, tok) of the pass — request rows and run-ahead rows alike — truncates the slot's record to pos and
 *     appends tok; a failed pass clears the records of the slots it touched.  Records describe cache CONTENTS, not ownership: they survive
 *     reset_context, a new prompt and release_slot / acquire_slot, because nothing but this scheduler's passes and copies writes the cache.
 *   Keep.  When the scheduler first takes a request whose tokens are the whole context from position 0 (submit's `prefix` argument, set by
 *     prepare_generation only), the request's cursor (done_rows) skips the longest common prefix of its tokens and its slot's record, at most
 *     n - 1 rows: the last prompt token is always computed.
 *   Copy.  Each time a pass is formed, a request that enters it looks for another slot whose record matches its tokens at least
 *     TK_PREFIX_COPY_MIN positions beyond the cursor (tk_prefix_match.h: longest match, lowest slot on ties); rows [cursor, match) are copied
 *     from that slot by ONE k_kv_copy_rows launch per pass for all such requests, and the cursor moves to match.  Matching reads records as
 *     of the last completed pass; rows the pass being formed will compute are not a source, so requests that share a pass both compute.
 *   Ordering rule.  The copy launch goes on the session stream BEFORE the pass's forward, outside any graph capture: a source slot whose owner
 *     overwrites it in this very pass is read first.  Within a launch no slot is both a source and a destination (a request whose slot already
 *     serves as a source in this launch, or whose best donor is a destination of it, computes this pass and looks again in the next).
 *   Stale rows.  Positions are still fed in ascending order from the cursor, so a row beyond the cursor is overwritten before anything attends
 *     to it, exactly as for a restart at position 0.  drop_ahead needs nothing new for a cursor > 0: a PLANNED run-ahead row never ran; a DONE
 *     one is in the record already; an INFLIGHT one belongs to a pass that completes — and enters the record, at its position, for its token —
 *     before the scheduler forms the next pass, which is the first moment the new prompt is matched.  The record says the truth either way: if
 *     the new prompt continues with that very token the row is kept, otherwise the match ends before it.
 *
 * Context shift (shift()).  A runner whose context is full may drop rows behind its first n_keep and move the rest down (k_kv_shift_rows).  The
 * scheduler thread takes queued shifts at the top of an iteration, before it forms a pass: no pass is in flight then (the same thread runs them), so
 * an INFLIGHT run-ahead row of the slot has completed; drop_ahead(slot) retires what is left (a PLANNED row never runs), and the slot's record is
 * truncated to n_keep BEFORE the launch.  The moved rows were computed in a context that no longer exists — they are not "the rows a recomputation
 * would write" — so they are never kept or copied: the record ends at n_keep, and record_row does not extend a record that does not reach the row's
 * position, so it stays there until a prompt is fed from within [0, n_keep].  Rows [0, n_keep) are untouched and stay valid.  The iteration that
 * runs shifts forms no pass and launches no copy, so a slot that is being shifted is neither source nor destination of a copy of that iteration;
 * against the copies of other iterations the session stream orders it.
 *
 * Verify requests (submit_verify; lookup decoding, tk_lookup.h).  A greedy runner feeds its pending id and n - 1 drafted ids at positions pos0,
 * pos0 + 1, ... of its slot; EVERY row is sampled, and the accept rule keeps the ids picks[0 .. m] that one-row passes would have produced.  The n rows
 * enter one pass together (a request that finds fewer rows left waits for the next pass).  A pass that holds at least one verify request and in
 * which every other request is a plain greedy, unmasked, unadjusted one without log-probabilities that ends in this pass (its last row is the sampled one; run-ahead rows are
 * such rows too) goes through TkLlmSession::forward_verify, where a long context may take the run form of the long attention; any other pass goes
 * through forward() as before — forward() returns the arg max of every row of a multi-position pass too, and both paths give a row the same bits.
 * A pass without a verify request is untouched: it replays the graphs it always did.
 *   Records.  record_row runs for rows 0 .. m of a verify request only, so the slot's record ends at pos0 + m + 1: the prefix cache never keeps or
 *     copies a rejected row.
 *   Rejected rows stay in the cache beyond the owner's n_past and are overwritten before anything attends to them, because positions are fed in
 *     ascending order: the argument made above for wasted run-ahead rows.
 *   stats()' rows count all n rows of a verify request.
 *
 * Verify requests with tables (submit_verify's trailing arguments; tk_lookup_scope.h).  A runner whose lookup scope covers its temperature, grammar,
 * penalties / bias or log-probabilities gives every row of its request the tables a one-row pass at that position would have had: a mask per row, the
 * sampling state of row 0 (row i draws with counter + i), an adjustment per row, n_top for every row and a record per row.  Such a request makes its
 * pass go through forward() — the only entry that takes tables — with the tables on ALL its rows; forward() gives rows that are runs of consecutive
 * positions the attention forward_verify would (tk_pass_form_rows), so a long context still takes the run form.  A pass whose verify requests carry
 * no table and whose other requests qualify takes forward_verify as before.  Accept rule, records of the cache, rejected rows and stats are those of
 * any verify request; the log-probability records of ids 0 .. m are handed over with them.  Everything travels through forward()'s existing
 * parameters: the scheduler calls the six session members it always called.
 */
#ifndef TK_LLM_BATCHER_H
#define TK_LLM_BATCHER_H

#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "tk_llm_engine.h"

class TkLlmBatcher {
public:
    ~TkLlmBatcher();
    /* one session with `slots` sequences of `n_ctx` positions on the model's device; starts the scheduler thread */
    /* kv_type: the session's cache type (TkLlmSession::kv_type) */
    bool init(TkLlmModel* model, int slots, int n_ctx, int32_t eos, std::string* err, int kv_type = 0);
    int acquire_slot();            /* -1 when every slot is taken */
    void release_slot(int slot);
    int n_ctx() const { return n_ctx_; }
    int slots() const { return (int)slot_used_.size(); }
    /* the shared session, for its thread-safe grammar-mask registry alone (TkLlmSession::attach_grammar_state): a runner attaches a state to the mask
     * pointer it submits; the scheduler itself knows nothing of it */
    TkLlmSession* session() { return &session_; }
    /* Blocking: feed `n` tokens of sequence `slot` at positions pos0, pos0 + 1, ...; *sampled = arg max after the last one (over the
     * tokens `mask` allows, when given: (vocab + 31) / 32 words, bit t = token t).  Thread-safe; one outstanding call per slot. */
    /* samp (optional): sampling state of the sampled row — temp > 0 draws from the reference's default stochastic chain with the given
     * (seed, counter) instead of the arg max; such rows never run ahead (the next counter is the owner's) */
    /* prefix (optional; prepare_generation only): the tokens are the WHOLE context from position 0 (pos0 == 0), so rows the cache already holds
     * for them may be kept or copied when the prefix cache is on; receives what became of the n rows */
    /* adjust (optional): logit bias and repetition penalties of the sampled row (common/tk_logit_adjust.h); its arrays belong to the caller until
     * the call returns, like `mask`; checked here against the limits.  A non-neutral one keeps the row from running ahead (header comment) */
    struct PrefixRows { int32_t prompt_rows = 0, kept = 0, copied = 0; };
    /* n_top (optional): -1 = off, 0 .. TK_LOGPROB_MAX_TOP = the log-probability of the sampled id and that many alternatives into *record
     * (common/tk_token_logprob.h), filled when the call returns true; such a row still runs ahead (header comment) */
    bool submit(int slot, int pos0, const int32_t* toks, int n, const uint32_t* mask, int32_t* sampled, std::string* err, const TkSampleRow* samp = nullptr,
                PrefixRows* prefix = nullptr, const TkLogitAdjust* adjust = nullptr, bool hold = false, int32_t n_top = -1, TkTokenLogprob* record = nullptr);
    /* hold: no row runs ahead of this request's sampled id (the owner has lookup decoding on: its next call is a verify request or comes with `hold` again) */
    /* Blocking: the verify pass of lookup decoding (header comment, "Verify requests"): toks[0] is the slot's pending id, toks[1 .. n) are drafts, fed at
     * positions pos0 .. pos0 + n - 1 in ONE pass, 1 <= n <= TK_LOOKUP_MAX_DRAFT + 1; every row is sampled greedily.  ids_out (room for n) receives the
     * ids the accept rule keeps, *n_out = m + 1 of them; rows pos0 .. pos0 + m are the slot's valid cache rows afterwards */
    /* Tables (optional; tk_lookup_scope.h, header comment "Verify requests with tables"): the request of a runner that samples, is masked, adjusted or
     * asks for records.  row_masks: n_tables pointers, nullptr = that row is unmasked; samp: the sampling state of row 0, row i draws with
     * counter + i (temp <= 0: greedy); row_adjust: n_tables adjustments, checked here against the limits; n_top >= 0 with records: n_tables records,
     * records[0 .. *n_out) filled, record i for id i.  The arrays belong to the caller until the call returns.  n_tables must be n when a per-row table
     * is given; n_top >= 0 without records, or records without n_top, is refused.  Without any table the request is the one it always was */
    bool submit_verify(int slot, int pos0, const int32_t* toks, int n, int32_t* ids_out, int* n_out, std::string* err, const uint32_t* const* row_masks = nullptr,
                       const TkSampleRow* samp = nullptr, const TkLogitAdjust* row_adjust = nullptr, int32_t n_top = -1, TkTokenLogprob* records = nullptr,
                       int n_tables = 0);
    /* Blocking: context shift of sequence `slot` (common/tk_kv_shift.h, llama.cpp's rule): the first n_keep rows stay, the n_discard rows after them are
     * dropped, rows [n_keep + n_discard, n_past) move down by n_discard.  Queued like a request: the scheduler thread runs it between passes on the
     * session stream (header comment, "Context shift").  Thread-safe; the slot's owner has no other call outstanding */
    bool shift(int slot, int n_keep, int n_discard, int n_past, std::string* err);
    /* the prompt prefix cache, off by default; may change at any time, read when the scheduler first takes a prompt.  false: the model's rows are
     * not whole 16-byte words (head_dim % 8 != 0) */
    bool set_prefix_cache(bool on);
    /* totals since init: prompt rows asked for through `prefix`, of them kept in place, of them copied from another slot, copy launches */
    void prefix_stats(uint64_t* prompt_rows, uint64_t* kept, uint64_t* copied, uint64_t* copy_launches);
    /* counters for tests and bench: passes run, rows processed FOR AN OWNER (a run-ahead row counts when its owner takes it; wasted ones
     * are in *wasted), the widest pass so far */
    void stats(uint64_t* passes, uint64_t* rows, int* max_rows, uint64_t* wasted = nullptr);

private:
    struct Request {
        int slot, pos0, n, done_rows = 0;
        bool whole = false, taken = false, cached = false; /* whole context from position 0; seen by the scheduler; the cache was on at that moment */
        int kept = 0, copied = 0;
        const int32_t* toks;
        const uint32_t* mask;
        TkSampleRow samp{};
        TkLogitAdjust adj{};
        bool adjusted = false; /* adj is not neutral */
        bool hold = false;     /* no run-ahead from this row: submit's `hold`, adjusted, or penalties that are on over a still empty window (the next one is not) */
        int32_t sampled = -1;
        int32_t n_top = -1;           /* log-probabilities of the sampled row: -1 off */
        TkTokenLogprob* rec = nullptr; /* the owner's record, written before `finished` */
        bool verify = false;         /* a verify request: all n rows in one pass, every row sampled */
        /* a verify request with tables (tk_lookup_scope.h): per-row masks and adjustments of the owner, `samp` the state of row 0, n_top for every row,
         * rec an array of n records; tabled: the pass goes through forward() with these on all n rows */
        const uint32_t* const* row_masks = nullptr;
        const TkLogitAdjust* row_adjust = nullptr;
        bool tabled = false;
        std::vector<int32_t> ids;     /* what the accept rule kept of its picks (m + 1 ids) */
        bool finished = false, ok = true;
        std::string error;
        std::condition_variable cv;
    };
    /* one run-ahead row per sequence slot */
    struct Ahead {
        enum State { NONE, PLANNED, INFLIGHT, DONE } st = NONE;
        int pos = 0;
        int32_t tok = 0, sampled = -1;
        int32_t n_top = -1;   /* the slot's log-probability setting when the row was planned */
        TkTokenLogprob rec{}; /* DONE: the row's record, handed over with `sampled` */
        bool ok = true, discard = false;
        std::string error;    /* DONE and not ok: the session's error of the pass that carried the row */
        Request* waiter = nullptr;
    };
    void loop();
    void plan_ahead(int slot, int pos_done, int32_t sampled, bool masked, int32_t n_top = -1); /* mu_ held */
    void drop_ahead(int slot);                                              /* mu_ held */
    std::vector<Ahead> ahead_;
    int32_t eos_ = -1;
    uint64_t wasted_ = 0;
    TkLlmSession session_;
    int n_ctx_ = 0;
    std::vector<char> slot_used_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<Request*> queue_;
    struct ShiftReq {
        int slot, n_keep, n_discard, n_past;
        bool finished = false, ok = true;
        std::string error;
        std::condition_variable cv;
    };
    std::deque<ShiftReq*> shifts_;
    bool stop_ = false;
    bool decode_first_ = false; /* TK_MI355X_BATCHER_DECODE_FIRST=1: sampled rows before prompt rows when a pass is formed (A/B; tk_llm_batcher.cpp) */
    size_t expect_ = 0; /* requests finished by the last pass: their owners are about to submit the next token */
    uint64_t passes_ = 0, rows_ = 0;
    /* prompt prefix cache (header comment) */
    bool prefix_cache_ = false;
    std::vector<std::vector<int32_t>> rec_; /* [slot]: token id of the row at each position, capacity n_ctx */
    void record_row(int slot, int pos, int32_t tok); /* scheduler thread, mu_ held, after a completed pass */
    uint64_t prompt_rows_ = 0, kept_ = 0, copied_ = 0, copy_launches_ = 0;
    int max_rows_ = 0;
    /* TK_MI355X_BATCHER_TRACE=<file>: one line per pass (times in ms since the scheduler started: woken, pass formed, pass done; rows, of them
     * run-ahead rows, requests completed, requests still queued, graph captures so far and their host time), written when the batcher dies */
    struct PassTrace { double woke, formed, done; int rows, ahead, completing, queued_after; uint64_t captures; double capture_ms; };
    std::vector<PassTrace> trace_;
    std::string trace_path_;
    std::thread worker_;
};

#endif
