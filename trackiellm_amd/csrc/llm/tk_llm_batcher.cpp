#include "tk_llm_batcher.h"
#include "tk_lookup.h"
#include "tk_lookup_scope.h"
#include "tk_prefix_match.h"

#include <algorithm>
#include <chrono>
#include <stdio.h>
#include <stdlib.h>

TkLlmBatcher::~TkLlmBatcher() {
    {
        std::lock_guard<std::mutex> lk(mu_);
        stop_ = true;
    }
    cv_.notify_all();
    if (worker_.joinable()) worker_.join();
    if (!trace_path_.empty()) {
        if (FILE* f = fopen(trace_path_.c_str(), "a")) {
            fprintf(f, "# batcher %p: woke_ms formed_ms done_ms rows ahead completing queued_after captures capture_ms\n", (void*)this);
            for (const PassTrace& t : trace_)
                fprintf(f, "%.3f %.3f %.3f %d %d %d %d %llu %.2f\n", t.woke, t.formed, t.done, t.rows, t.ahead, t.completing, t.queued_after, (unsigned long long)t.captures, t.capture_ms);
            fclose(f);
        }
    }
}

bool TkLlmBatcher::init(TkLlmModel* model, int slots, int n_ctx, int32_t eos, std::string* err, int kv_type) {
    if (slots < 1) slots = 1;
    if (slots > TK_MAX_ROWS) slots = TK_MAX_ROWS; /* one decode row per runner must fit one pass */
    session_.kv_type = kv_type;
    if (!session_.init(model, slots, n_ctx)) { *err = session_.error; return false; }
    n_ctx_ = n_ctx;
    slot_used_.assign((size_t)slots, 0);
    ahead_.assign((size_t)slots, Ahead());
    rec_.assign((size_t)slots, std::vector<int32_t>());
    for (auto& r : rec_) r.reserve((size_t)n_ctx);
    eos_ = eos;
    if (const char* e = getenv("TK_MI355X_BATCHER_DECODE_FIRST")) decode_first_ = e[0] == '1';
    if (const char* e = getenv("TK_MI355X_BATCHER_TRACE")) { trace_path_ = e; trace_.reserve(4096); }
    worker_ = std::thread([this] { loop(); });
    return true;
}

int TkLlmBatcher::acquire_slot() {
    std::lock_guard<std::mutex> lk(mu_);
    for (size_t i = 0; i < slot_used_.size(); ++i)
        if (!slot_used_[i]) { slot_used_[i] = 1; return (int)i; }
    return -1;
}

void TkLlmBatcher::release_slot(int slot) {
    std::lock_guard<std::mutex> lk(mu_);
    if (slot >= 0 && slot < (int)slot_used_.size()) { slot_used_[(size_t)slot] = 0; drop_ahead(slot); }
}

void TkLlmBatcher::stats(uint64_t* passes, uint64_t* rows, int* max_rows, uint64_t* wasted) {
    std::lock_guard<std::mutex> lk(mu_);
    if (passes) *passes = passes_;
    if (rows) *rows = rows_;
    if (max_rows) *max_rows = max_rows_;
    if (wasted) *wasted = wasted_;
}

bool TkLlmBatcher::set_prefix_cache(bool on) {
    if (on && !session_.kv_copy_applies()) return false;
    std::lock_guard<std::mutex> lk(mu_);
    prefix_cache_ = on;
    return true;
}

void TkLlmBatcher::prefix_stats(uint64_t* prompt_rows, uint64_t* kept, uint64_t* copied, uint64_t* copy_launches) {
    std::lock_guard<std::mutex> lk(mu_);
    if (prompt_rows) *prompt_rows = prompt_rows_;
    if (kept) *kept = kept_;
    if (copied) *copied = copied_;
    if (copy_launches) *copy_launches = copy_launches_;
}

/* a completed pass wrote the row of `tok` at `pos` of `slot`: it attended to rows 0 .. pos - 1, which are what the record lists as long as the
 * record reaches pos (rows are fed in order, so it does; a row beyond the record's end is simply not recorded) */
void TkLlmBatcher::record_row(int slot, int pos, int32_t tok) {
    std::vector<int32_t>& r = rec_[(size_t)slot];
    if ((size_t)pos > r.size()) return;
    r.resize((size_t)pos);
    r.push_back(tok);
}

/* the owner of `slot` has just been handed `sampled` for position pos_done: feed it at pos_done + 1 in the next pass */
void TkLlmBatcher::plan_ahead(int slot, int pos_done, int32_t sampled, bool masked, int32_t n_top) {
    Ahead& a = ahead_[(size_t)slot];
    if (masked || sampled < 0 || sampled == eos_ || pos_done + 2 >= n_ctx_ || a.st != Ahead::NONE) return; /* the runner stops at n_past + 1 >= n_ctx */
    a = Ahead();
    a.st = Ahead::PLANNED;
    a.pos = pos_done + 1;
    a.tok = sampled;
    a.n_top = n_top; /* the owner's log-probability setting rides along: the record depends on nothing the owner decides */
}

void TkLlmBatcher::drop_ahead(int slot) {
    Ahead& a = ahead_[(size_t)slot];
    if (a.st == Ahead::NONE) return;
    if (a.st == Ahead::INFLIGHT) { a.discard = true; a.waiter = nullptr; return; } /* the pass that carries it retires it */
    if (a.st == Ahead::DONE) wasted_++;
    a = Ahead();
}

bool TkLlmBatcher::submit(int slot, int pos0, const int32_t* toks, int n, const uint32_t* mask, int32_t* sampled, std::string* err, const TkSampleRow* samp,
                          PrefixRows* prefix, const TkLogitAdjust* adjust, bool hold, int32_t n_top, TkTokenLogprob* record) {
    if (n <= 0) { *err = "nothing to feed"; return false; }
    if (const char* why = tk_logprob_check(n_top, session_.model->hp.vocab)) { *err = std::string("log-probabilities: ") + why; return false; }
    if (n_top >= 0 && !record) { *err = "log-probabilities asked for without a record to fill"; return false; }
    if (adjust)
        if (const char* why = adjust->check(session_.model->hp.vocab)) { *err = std::string("logit adjustment: ") + why; return false; }
    if (slot < 0 || slot >= (int)slot_used_.size() || pos0 < 0 || pos0 + n > n_ctx_) { *err = "rows do not fit the context window"; return false; }
    Request r;
    r.slot = slot; r.pos0 = pos0; r.n = n; r.toks = toks; r.mask = mask;
    if (samp) r.samp = *samp;
    if (adjust && !adjust->neutral()) { r.adj = *adjust; r.adjusted = true; }
    r.n_top = n_top; r.rec = record;
    r.hold = hold || r.adjusted || (adjust && (adjust->repeat != 1.0f || adjust->freq != 0.0f || adjust->present != 0.0f));
    r.whole = prefix != nullptr && pos0 == 0;
    if (prefix) *prefix = PrefixRows{n, 0, 0};
    const bool stochastic = r.samp.temp > 0.0f;
    std::unique_lock<std::mutex> lk(mu_);
    if (stop_) { *err = "scheduler stopped"; return false; }
    Ahead& a = ahead_[(size_t)slot];
    if (a.st != Ahead::NONE && !a.discard) {
        if (n == 1 && !mask && !stochastic && !r.adjusted && pos0 == a.pos && toks[0] == a.tok && n_top == a.n_top) { /* the row this call asks for is the one that ran (or runs) ahead */
            if (a.st == Ahead::DONE) {
                const bool ok = a.ok;
                const int32_t got = a.sampled;
                const std::string failed = a.error; /* of the pass that carried the row, not of whichever pass failed last */
                if (ok && n_top >= 0) *record = a.rec; /* handed over with the id */
                a = Ahead();
                if (!ok) { *err = failed; return false; }
                rows_++;
                *sampled = got;
                plan_ahead(slot, pos0, got, r.hold, n_top); /* hold: lookup or the penalties were switched on while a row ran ahead; it is the last one */
                cv_.notify_all();
                return true;
            }
            a.waiter = &r; /* PLANNED or INFLIGHT: the pass that carries the row finishes this request */
            cv_.notify_all();
            r.cv.wait(lk, [&] { return r.finished; });
            if (!r.ok) { *err = r.error; return false; }
            *sampled = r.sampled;
            return true;
        }
        drop_ahead(slot); /* the owner went another way (a tool response, a new prompt, a masked step) */
    }
    queue_.push_back(&r);
    cv_.notify_all();
    r.cv.wait(lk, [&] { return r.finished; });
    if (prefix) { prefix->kept = r.kept; prefix->copied = r.copied; }
    if (!r.ok) { *err = r.error; return false; }
    *sampled = r.sampled;
    return true;
}

bool TkLlmBatcher::submit_verify(int slot, int pos0, const int32_t* toks, int n, int32_t* ids_out, int* n_out, std::string* err, const uint32_t* const* row_masks,
                                 const TkSampleRow* samp, const TkLogitAdjust* row_adjust, int32_t n_top, TkTokenLogprob* records, int n_tables) {
    if (n < 1 || n > TK_LOOKUP_MAX_DRAFT + 1 || !toks || !ids_out || !n_out) { *err = "verify request: between 1 and 16 rows"; return false; }
    if (slot < 0 || slot >= (int)slot_used_.size() || pos0 < 0 || pos0 + n > n_ctx_) { *err = "rows do not fit the context window"; return false; }
    if (const char* why = tk_logprob_check(n_top, session_.model->hp.vocab)) { *err = std::string("log-probabilities: ") + why; return false; }
    if (n_top >= 0 && !records) { *err = "log-probabilities asked for without records to fill"; return false; }
    if (n_top < 0 && records) { *err = "verify request: records given without an n_top"; return false; }
    if ((row_masks || row_adjust || records) && n_tables != n) { *err = "verify request: a per-row table holds one entry per row"; return false; }
    for (int i = 0; i < n && row_adjust; ++i)
        if (const char* why = row_adjust[i].check(session_.model->hp.vocab)) { *err = "logit adjustment of row " + std::to_string(i) + ": " + why; return false; }
    Request r;
    r.slot = slot; r.pos0 = pos0; r.n = n; r.toks = toks; r.mask = nullptr;
    r.verify = true;
    r.hold = true;
    bool any_mask = false, any_adj = false;
    for (int i = 0; i < n; ++i) {
        any_mask = any_mask || (row_masks && row_masks[i]);
        any_adj = any_adj || (row_adjust && !row_adjust[i].neutral());
    }
    if (any_mask) r.row_masks = row_masks;
    if (any_adj) { r.row_adjust = row_adjust; r.adjusted = true; }
    if (samp && samp->temp > 0.0f) r.samp = *samp;
    r.n_top = n_top; r.rec = records;
    r.tabled = any_mask || any_adj || r.samp.temp > 0.0f || n_top >= 0;
    std::unique_lock<std::mutex> lk(mu_);
    if (stop_) { *err = "scheduler stopped"; return false; }
    drop_ahead(slot); /* a slot with lookup on plans no row ahead; one left from before lookup was switched on is retired like any other */
    queue_.push_back(&r);
    cv_.notify_all();
    r.cv.wait(lk, [&] { return r.finished; });
    if (!r.ok) { *err = r.error; return false; }
    *n_out = (int)r.ids.size();
    for (size_t i = 0; i < r.ids.size(); ++i) ids_out[i] = r.ids[i];
    return true;
}

bool TkLlmBatcher::shift(int slot, int n_keep, int n_discard, int n_past, std::string* err) {
    if (slot < 0 || slot >= (int)slot_used_.size() || n_keep < 0 || n_discard < 1 || n_keep + n_discard >= n_past || n_past > n_ctx_) { *err = "context shift: rows outside the context window"; return false; }
    ShiftReq r;
    r.slot = slot; r.n_keep = n_keep; r.n_discard = n_discard; r.n_past = n_past;
    std::unique_lock<std::mutex> lk(mu_);
    if (stop_) { *err = "scheduler stopped"; return false; }
    shifts_.push_back(&r);
    cv_.notify_all();
    r.cv.wait(lk, [&] { return r.finished; });
    if (!r.ok) { *err = r.error; return false; }
    return true;
}

void TkLlmBatcher::loop() {
    std::vector<int32_t> sq, ps, tk, am;
    std::vector<const uint32_t*> masks;
    std::vector<TkSampleRow> samps;
    std::vector<TkLogitAdjust> adjs;
    std::vector<int32_t> ntops;        /* [row of the pass]: -1, or the n_top of the request / run-ahead row that is sampled there */
    std::vector<TkTokenLogprob> recs;  /* [row of the pass]: what forward() filled for the rows that ask */
    struct Taken { Request* r; int take, last_row; };   /* `take` rows of a request end at row `last_row` of the pass */
    struct AheadRow { int slot, row; };                  /* a sequence's run-ahead row and where it sits in the pass */
    std::vector<Taken> in_pass;
    std::vector<Request*> completing;
    std::vector<AheadRow> ahead_rows;
    std::vector<ShiftReq*> shifting;
    std::vector<char> rejected; /* [row of the pass]: a verify request's row behind its last accepted one */
    /* prefix cache: the copies of the pass being formed (at most one per request of the pass), the request each serves, and the slots that are
     * a source / a destination of this launch */
    std::vector<TkKvCopyDesc> copies;
    std::vector<Request*> copy_for;
    std::vector<const int32_t*> rec_ptr(rec_.size());
    std::vector<int> rec_len(rec_.size());
    std::vector<char> is_src(rec_.size()), is_dst(rec_.size());
    copies.reserve(TK_MAX_ROWS); copy_for.reserve(TK_MAX_ROWS);
    auto any_planned = [&] {
        for (const Ahead& a : ahead_) if (a.st == Ahead::PLANNED) return true;
        return false;
    };
    const auto t_origin = std::chrono::steady_clock::now();
    auto now_ms = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_origin).count(); };
    for (;;) {
        double t_woke = 0.0;
        in_pass.clear(); completing.clear(); ahead_rows.clear(); copies.clear(); copy_for.clear();
        sq.clear(); ps.clear(); tk.clear(); masks.clear(); samps.clear(); adjs.clear(); ntops.clear();
        bool any_mask = false, any_samp = false, any_adj = false, any_lp = false;
        bool any_verify = false, all_qualify = true; /* verify requests (tk_llm_batcher.h): the pass may take forward_verify */
        {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [&] { return stop_ || !queue_.empty() || !shifts_.empty() || any_planned(); });
            t_woke = trace_path_.empty() ? 0.0 : now_ms();
            if (stop_) {
                for (Request* r : queue_) { r->ok = false; r->error = "scheduler stopped"; r->finished = true; r->cv.notify_all(); }
                queue_.clear();
                for (ShiftReq* r : shifts_) { r->ok = false; r->error = "scheduler stopped"; r->finished = true; r->cv.notify_all(); }
                shifts_.clear();
                for (Ahead& a : ahead_)
                    if (a.waiter) { a.waiter->ok = false; a.waiter->error = "scheduler stopped"; a.waiter->finished = true; a.waiter->cv.notify_all(); a.waiter = nullptr; }
                return;
            }
            /* context shifts (tk_llm_batcher.h): no pass is in flight here.  What ran ahead of the owner is retired and the record cut to the rows that
             * stay valid BEFORE the rows move; the moves run without the lock, and this iteration forms no pass */
            if (!shifts_.empty()) {
                shifting.assign(shifts_.begin(), shifts_.end());
                shifts_.clear();
                for (ShiftReq* r : shifting) {
                    drop_ahead(r->slot);
                    std::vector<int32_t>& rec = rec_[(size_t)r->slot];
                    if (rec.size() > (size_t)r->n_keep) rec.resize((size_t)r->n_keep);
                }
                lk.unlock();
                for (ShiftReq* r : shifting) {
                    r->ok = session_.kv_shift(r->slot, r->n_keep + r->n_discard, r->n_past, -r->n_discard);
                    if (!r->ok) r->error = session_.error;
                }
                lk.lock();
                for (ShiftReq* r : shifting) { /* the owner wakes under the lock and takes its request with it */
                    if (!r->ok) rec_[(size_t)r->slot].clear();
                    r->finished = true;
                    r->cv.notify_all();
                }
                continue;
            }
            /* the owners of the requests the last pass finished WITHOUT a run-ahead row (masked steps) are about to ask for their next
             * token: give them a moment so that K runners decoding in lock step share every pass (a late one simply rides the next pass) */
            if (queue_.size() < expect_ && !any_planned()) {
                /* the window grows with the number of owners expected back (waking K host threads takes time) and stays well under the cost
                 * of the pass it fills: 200 us + 8 us per expected request, at most 2.5 ms (a 256-row pass is ~8 ms, a 16-row pass ~2.3 ms) */
                const int64_t us = std::min<int64_t>(2500, 200 + 8 * (int64_t)expect_);
                cv_.wait_for(lk, std::chrono::microseconds(us), [&] { return stop_ || queue_.size() >= expect_ || !shifts_.empty(); });
                /* an expected owner shifts before it asks: serve the shift first (top of the loop); its request then joins the others' pass */
                if (!shifts_.empty()) continue;
            }
            /* FIFO: a request contributes as many of its remaining rows as the pass still holds, then the run-ahead rows.  A grammar-masked
             * request samples under its own token mask, which the arg max kernel takes per ROW: masked and unmasked requests share passes.
             * A row's result does not depend on its place in a pass or on the pass it rides.
             * TK_MI355X_BATCHER_DECODE_FIRST=1 (measured, not the default: profiles/r06_batcher_trace.txt) takes the rows that end in a sampled
             * token first — one-row requests and run-ahead rows — so that a decoding sequence rides the passes that carry other sequences'
             * prompt rows instead of waiting behind them: K cortices driven in lock step gain little (their prompts and their decode steps
             * arrive together whatever the order) and a pass that mixes one-row sequences with prompt chunks pays for 16-row attention
             * tiles that hold one row each (256-row pass: 8.7 -> 9.6 .. 12.3 ms). */
            auto add_rows = [&](Request* r, int take) {
                for (int i = 0; i < take; ++i) {
                    sq.push_back(r->slot);
                    ps.push_back(r->pos0 + r->done_rows + i);
                    tk.push_back(r->toks[r->done_rows + i]);
                    masks.push_back(nullptr);
                    samps.push_back(TkSampleRow{});
                    adjs.push_back(TkLogitAdjust{});
                    ntops.push_back(-1);
                }
                in_pass.push_back(Taken{r, take, (int)sq.size() - 1});
                any_verify = any_verify || r->verify;
                all_qualify = all_qualify && (r->verify ? !r->tabled : (r->done_rows + take == r->n && !r->mask && !(r->samp.temp > 0.0f) && !r->adjusted && r->n_top < 0));
                if (r->tabled) { /* a verify request with tables (tk_lookup_scope.h): every row is sampled under its own; take == n */
                    const size_t row0 = sq.size() - (size_t)take;
                    for (int i = 0; i < take; ++i) {
                        if (r->row_masks) masks[row0 + (size_t)i] = r->row_masks[i];
                        if (r->samp.temp > 0.0f) { samps[row0 + (size_t)i] = r->samp; samps[row0 + (size_t)i].counter = tk_lookup_row_counter(r->samp.counter, i); }
                        if (r->row_adjust && !r->row_adjust[i].neutral()) adjs[row0 + (size_t)i] = r->row_adjust[i];
                        ntops[row0 + (size_t)i] = r->n_top;
                        any_mask = any_mask || masks[row0 + (size_t)i] != nullptr;
                    }
                    completing.push_back(r);
                    any_samp = any_samp || r->samp.temp > 0.0f;
                    any_adj = any_adj || r->row_adjust != nullptr;
                    any_lp = any_lp || r->n_top >= 0;
                } else if (r->done_rows + take == r->n) {
                    completing.push_back(r);
                    masks.back() = r->mask; /* the row that is sampled */
                    samps.back() = r->samp;
                    any_mask = any_mask || r->mask != nullptr;
                    any_samp = any_samp || r->samp.temp > 0.0f;
                    adjs.back() = r->adj;
                    any_adj = any_adj || r->adjusted;
                    ntops.back() = r->n_top;
                    any_lp = any_lp || r->n_top >= 0;
                }
            };
            /* prefix cache (tk_llm_batcher.h): a whole-context request that is about to enter the pass first moves its cursor over the rows its
             * own slot holds (once), then over rows another slot holds (each pass, at the cursor where it stands) */
            std::fill(is_src.begin(), is_src.end(), 0);
            std::fill(is_dst.begin(), is_dst.end(), 0);
            for (size_t s = 0; s < rec_.size(); ++s) { rec_ptr[s] = rec_[s].data(); rec_len[s] = (int)rec_[s].size(); }
            auto use_cache = [&](Request* r) {
                if (!r->whole) return;
                if (!r->taken) {
                    r->taken = true;
                    prompt_rows_ += (uint64_t)r->n;
                    r->cached = prefix_cache_;
                    if (!r->cached) return;
                    r->kept = tk_prefix_common(r->toks, r->n, rec_ptr[(size_t)r->slot], rec_len[(size_t)r->slot]);
                    r->done_rows = r->kept;
                    kept_ += (uint64_t)r->kept;
                }
                if (!r->cached || is_src[(size_t)r->slot] || is_dst[(size_t)r->slot] || (int)copies.size() >= TK_MAX_ROWS) return;
                int match = 0;
                const int donor = tk_prefix_best_donor(r->toks, r->n, rec_ptr.data(), rec_len.data(), (int)rec_.size(), r->slot, r->done_rows, is_dst.data(), &match);
                if (donor < 0) return;
                copies.push_back(TkKvCopyDesc{donor, r->slot, r->done_rows, match - r->done_rows});
                copy_for.push_back(r);
                is_src[(size_t)donor] = 1;
                is_dst[(size_t)r->slot] = 1;
                r->copied += match - r->done_rows;
                copied_ += (uint64_t)(match - r->done_rows);
                r->done_rows = match;
            };
            const bool decode_first = decode_first_;
            if (decode_first)
                for (Request* r : queue_) {
                    if ((int)sq.size() >= TK_MAX_ROWS) break;
                    use_cache(r);
                    if (r->n - r->done_rows == 1) add_rows(r, 1); /* a verify request of one row among them */
                }
            auto add_ahead = [&] {
                for (size_t s = 0; s < ahead_.size() && (int)sq.size() < TK_MAX_ROWS; ++s) {
                    Ahead& a = ahead_[s];
                    if (a.st != Ahead::PLANNED) continue;
                    a.st = Ahead::INFLIGHT;
                    sq.push_back((int32_t)s);
                    ps.push_back(a.pos);
                    tk.push_back(a.tok);
                    masks.push_back(nullptr);
                    samps.push_back(TkSampleRow{});
                    adjs.push_back(TkLogitAdjust{});
                    ntops.push_back(a.n_top);
                    any_lp = any_lp || a.n_top >= 0;
                    all_qualify = all_qualify && a.n_top < 0; /* forward_verify reports no log-probabilities */
                    ahead_rows.push_back(AheadRow{(int)s, (int)sq.size() - 1});
                }
            };
            if (decode_first) add_ahead(); /* one per sequence whose owner holds the id they feed */
            for (Request* r : queue_) {
                if ((int)sq.size() >= TK_MAX_ROWS) break;
                use_cache(r);
                if (decode_first && r->n - r->done_rows == 1) continue; /* taken above */
                if (r->verify && r->n > TK_MAX_ROWS - (int)sq.size()) continue; /* its rows enter one pass together: the next one */
                add_rows(r, std::min(r->n - r->done_rows, TK_MAX_ROWS - (int)sq.size()));
            }
            if (!decode_first) add_ahead();
        }
        const int nrows = (int)sq.size();
        if (nrows == 0) continue;
        am.assign((size_t)nrows, -1);
        if (any_lp) recs.assign((size_t)nrows, TkTokenLogprob{});
        const double t_formed = trace_path_.empty() ? 0.0 : now_ms();
        const bool head = !completing.empty() || !ahead_rows.empty();
        /* the copies go first on the session's stream: forward() then reads the copied rows, and a source row it overwrites was read before */
        bool copied_ok = true;
        if (!copies.empty()) copied_ok = session_.enqueue_kv_copy(copies.data(), (int)copies.size());
        /* a pass with a verify request in which every request qualifies: every row is sampled, greedy, and a long context may take the run form */
        const bool ok = any_verify && all_qualify ? copied_ok && session_.forward_verify(nrows, sq.data(), ps.data(), tk.data(), -1, nullptr, am.data())
                        : copied_ok && session_.forward(nrows, sq.data(), ps.data(), tk.data(), nullptr, head ? am.data() : nullptr, head, head && any_mask ? masks.data() : nullptr,
                                        head && any_samp ? samps.data() : nullptr, head && any_adj ? adjs.data() : nullptr,
                                        head && any_lp ? ntops.data() : nullptr, head && any_lp ? recs.data() : nullptr);
        {
            std::lock_guard<std::mutex> lk(mu_);
            passes_++;
            if (nrows > max_rows_) max_rows_ = nrows;
            if (!copies.empty()) copy_launches_++;
            /* verify requests: the accept rule on the picks of their rows; the rows behind the last accepted one are not recorded */
            rejected.assign((size_t)nrows, 0);
            for (const Taken& t : in_pass) {
                if (!t.r->verify || !ok) continue;
                const int row0 = t.last_row - t.take + 1;
                t.r->ids.resize((size_t)t.take);
                const int kept = tk_lookup_accept(tk.data() + row0, am.data() + row0, t.take, eos_, t.r->ids.data());
                t.r->ids.resize((size_t)kept);
                for (int i = kept; i < t.take; ++i) rejected[(size_t)(row0 + i)] = 1;
            }
            /* records: what the cache holds now that the pass is complete — copied rows, then the pass's rows in feeding order */
            if (ok) {
                for (size_t c = 0; c < copies.size(); ++c)
                    for (int i = 0; i < copies[c].n; ++i) record_row(copies[c].dst_seq, copies[c].p0 + i, copy_for[c]->toks[copies[c].p0 + i]);
                for (int i = 0; i < nrows; ++i)
                    if (!rejected[(size_t)i]) record_row(sq[(size_t)i], ps[(size_t)i], tk[(size_t)i]);
            } else {
                for (const TkKvCopyDesc& c : copies) rec_[(size_t)c.dst_seq].clear();
                for (int i = 0; i < nrows; ++i) rec_[(size_t)sq[(size_t)i]].clear();
            }
            size_t held = 0; /* completing requests that got no run-ahead row: their owners are waited for */
            for (const Taken& t : in_pass) {
                Request* r = t.r;
                const int take = t.take, row = t.last_row + 1;
                rows_ += (uint64_t)take;
                r->done_rows += take;
                if (!ok) { r->ok = false; r->error = session_.error; r->done_rows = r->n; }
                if (r->done_rows == r->n) {
                    r->sampled = ok ? am[(size_t)row - 1] : -1;
                    if (ok && r->n_top >= 0 && r->verify) /* the records of the ids the accept rule kept, record i with id i */
                        for (size_t i = 0; i < r->ids.size(); ++i) r->rec[i] = recs[(size_t)(row - take) + i];
                    else if (ok && r->n_top >= 0) *r->rec = recs[(size_t)row - 1]; /* the owner is blocked in submit(): its record is ours to write */
                    for (auto it = queue_.begin(); it != queue_.end(); ++it)
                        if (*it == r) { queue_.erase(it); break; }
                    if (ok) plan_ahead(r->slot, r->pos0 + r->n - 1, r->sampled, r->mask != nullptr || r->samp.temp > 0.0f || r->hold, r->n_top);
                    /* an owner that was handed several ids comes back only when it has given all but the last to its caller: nobody waits for it */
                    if (!ok || (ahead_[(size_t)r->slot].st != Ahead::PLANNED && r->ids.size() <= 1)) held++;
                    r->finished = true;
                    r->cv.notify_all();
                }
            }
            for (const AheadRow& ar : ahead_rows) {
                const int s = ar.slot;
                Ahead& a = ahead_[(size_t)s];
                const int32_t got = ok ? am[(size_t)ar.row] : -1;
                if (a.discard) { wasted_++; a = Ahead(); continue; }
                if (a.waiter) { /* the owner is already waiting for exactly this row */
                    Request* w = a.waiter;
                    const int pos = a.pos;
                    if (ok && a.n_top >= 0) *w->rec = recs[(size_t)ar.row]; /* submit() matched the waiter's n_top with the row's */
                    a = Ahead();
                    w->ok = ok;
                    if (!ok) w->error = session_.error;
                    w->sampled = got;
                    rows_++;
                    if (ok) plan_ahead(s, pos, got, w->hold, w->n_top);
                    w->finished = true;
                    w->cv.notify_all();
                } else {
                    a.st = Ahead::DONE;
                    a.sampled = got;
                    if (ok && a.n_top >= 0) a.rec = recs[(size_t)ar.row]; /* held until the owner takes the id */
                    a.ok = ok;
                    if (!ok) a.error = session_.error;
                }
            }
            expect_ = held;
            if (!trace_path_.empty())
                trace_.push_back(PassTrace{t_woke, t_formed, now_ms(), nrows, (int)ahead_rows.size(), (int)completing.size(), (int)queue_.size(), session_.n_captures, session_.capture_ms});
        }
    }
}
