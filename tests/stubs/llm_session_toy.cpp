/* llm_session_toy.cpp — the members of TkLlmSession and TkLlmModel that csrc/llm/tk_llm_batcher.cpp links against, with no HIP call (llm_session_toy.h) */
#include "llm_session_toy.h"

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <condition_variable>
#include <mutex>

namespace toy {

namespace {
struct State {
    std::mutex mu;
    std::condition_variable cv;
    int max_seq = 0, max_ctx = 0;
    std::vector<Row> cache;          /* [slot][pos] */
    std::vector<long> row_pass;      /* [slot][pos] */
    std::vector<std::vector<std::pair<int, int>>> log; /* [pass] rows */
    std::vector<TkKvCopyDesc> pending_copies; /* the launch since the last pass: a failed pass leaves its destination rows undefined too */
    Totals t;
    std::vector<std::string> bad;
    std::vector<long> fail;
    long gate = -1;
    bool waiting = false;
    int live = 0;
    Row& at(int s, int p) { return cache[(size_t)s * (size_t)max_ctx + (size_t)p]; }
};
State g;

void breach(const char* what, long a = 0, long b = 0, long c = 0) { /* g.mu held */
    char buf[256];
    snprintf(buf, sizeof buf, "pass %llu: %s (%ld, %ld, %ld)", (unsigned long long)g.t.passes, what, a, b, c);
    if (g.bad.size() < 64) g.bad.push_back(buf);
}

/* the checks both pass entries share; false = the pass cannot be run at all */
bool check_rows(int nrows, const int32_t* seq, const int32_t* pos, const int32_t* tok, bool runs) {
    if (nrows < 1 || nrows > TK_MAX_ROWS) { breach("a pass of 1 .. TK_MAX_ROWS rows", nrows); return false; }
    if (!seq || !pos || !tok) { breach("null row arrays"); return false; }
    std::vector<int> last((size_t)g.max_seq, -1), last_row((size_t)g.max_seq, -1);
    for (int r = 0; r < nrows; ++r) {
        if (seq[r] < 0 || seq[r] >= g.max_seq || pos[r] < 0 || pos[r] >= g.max_ctx) { breach("a row outside the cache", r, seq[r], pos[r]); return false; }
        if (tok[r] < 0 || tok[r] >= VOCAB) { breach("a token outside the vocabulary", r, tok[r]); return false; }
        int& l = last[(size_t)seq[r]];
        if (l >= 0 && pos[r] <= l) breach("the rows of a slot do not ascend", r, seq[r], pos[r]);
        if (runs && l >= 0 && (pos[r] != l + 1 || last_row[(size_t)seq[r]] != r - 1)) breach("a verify pass whose rows of a slot are not one run", r, seq[r], pos[r]);
        l = pos[r];
        last_row[(size_t)seq[r]] = r;
    }
    return true;
}

/* pass bookkeeping in front of the rows: the gate, the log, the injected failure.  true = run the rows */
bool enter_pass(std::unique_lock<std::mutex>& lk, int nrows, const int32_t* seq, const int32_t* pos, std::string* error) {
    const long k = (long)g.t.passes;
    if (g.gate == k) {
        g.waiting = true;
        g.cv.notify_all();
        g.cv.wait(lk, [&] { return g.gate != k; });
        g.waiting = false;
    }
    g.log.emplace_back();
    for (int r = 0; r < nrows; ++r) g.log.back().push_back({seq[r], pos[r]});
    g.t.rows += (uint64_t)nrows;
    if (nrows > g.t.widest) g.t.widest = nrows;
    if (std::find(g.fail.begin(), g.fail.end(), k) != g.fail.end()) {
        /* what a failed pass leaves behind is undefined: its own rows and the rows the copy launch in front of it wrote */
        for (int r = 0; r < nrows; ++r) { Row& w = g.at(seq[r], pos[r]); w.h = mix(w.h, 0xdeadull + (uint64_t)r); w.valid = true; }
        for (const TkKvCopyDesc& c : g.pending_copies)
            for (int i = 0; i < c.n; ++i) { Row& w = g.at(c.dst_seq, c.p0 + i); w.h = mix(w.h, 0xbeefull + (uint64_t)i); }
        g.pending_copies.clear();
        g.t.failed_passes++;
        g.t.passes++;
        *error = fail_text(k);
        return false;
    }
    g.pending_copies.clear();
    return true;
}

/* feed one row: the chain hash of what it attends to */
uint64_t run_row(int s, int p, int32_t t) {
    for (int q = 0; q < p; ++q)
        if (!g.at(s, q).valid) { breach("a row attends to a row that was never written", s, p, q); break; }
    Row& w = g.at(s, p);
    w.h = feed(p ? &g.at(s, p - 1) : nullptr, t);
    w.tok = t;
    w.valid = true;
    g.row_pass[(size_t)s * (size_t)g.max_ctx + (size_t)p] = (long)g.t.passes;
    return w.h;
}
}  // namespace

uint64_t adjust_digest(const TkLogitAdjust& a) {
    uint32_t f[3];
    memcpy(f, &a.repeat, 4); memcpy(f + 1, &a.freq, 4); memcpy(f + 2, &a.present, 4);
    uint64_t d = mix(mix(mix(0x51ull, f[0]), f[1]), f[2]);
    d = mix(mix(d, (uint64_t)(uint32_t)a.n_recent), (uint64_t)(uint32_t)a.n_bias);
    for (int i = 0; i < a.n_recent; ++i) d = mix(d, (uint64_t)(uint32_t)a.recent[i]);
    for (int i = 0; i < a.n_bias; ++i) {
        uint32_t b;
        memcpy(&b, &a.bias[i], 4);
        d = mix(mix(d, (uint64_t)(uint32_t)a.bias_ids[i]), b);
    }
    return d;
}

int32_t pick(uint64_t h, const uint32_t* mask, const TkSampleRow* samp, const TkLogitAdjust* adj) {
    uint64_t b = h;
    if (samp && samp->temp > 0.0f) {
        uint32_t t;
        memcpy(&t, &samp->temp, 4);
        b = mix(mix(mix(b, samp->seed), samp->counter), t);
    }
    if (adj && !adj->neutral()) b = mix(b, adjust_digest(*adj));
    const int c = (int)(b % (uint64_t)VOCAB);
    if (!mask) return c;
    for (int i = 0; i < VOCAB; ++i) {
        const int t = (c + i) % VOCAB;
        if (mask[t >> 5] >> (t & 31) & 1u) return t;
    }
    return -1;
}

void fill_record(uint64_t h, int32_t n_top, TkTokenLogprob* rec) {
    if (n_top < 0) return;
    const uint64_t r = mix(h, 0x1090ull + (uint64_t)n_top);
    rec->logprob = -(float)(r % 4096) / 64.0f;
    rec->n_top = n_top < VOCAB ? n_top : VOCAB;
    for (int j = 0; j < rec->n_top; ++j) {
        rec->top_ids[j] = (int32_t)(((r >> 12) + 7ull * (uint64_t)j) % (uint64_t)VOCAB);
        rec->top_logprobs[j] = -(float)((r >> 20) % 1024 + (uint64_t)j) / 32.0f;
    }
}

bool same_record(const TkTokenLogprob& a, const TkTokenLogprob& b) {
    if (memcmp(&a.logprob, &b.logprob, 4) != 0 || a.n_top != b.n_top || a.n_top < 0 || a.n_top > TK_LOGPROB_MAX_TOP) return false;
    return memcmp(a.top_ids, b.top_ids, sizeof(int32_t) * (size_t)a.n_top) == 0 && memcmp(a.top_logprobs, b.top_logprobs, sizeof(float) * (size_t)a.n_top) == 0;
}

Totals totals() {
    std::lock_guard<std::mutex> lk(g.mu);
    return g.t;
}
std::vector<std::string> breaches() {
    std::lock_guard<std::mutex> lk(g.mu);
    return g.bad;
}
void reset() {
    std::lock_guard<std::mutex> lk(g.mu);
    g.t = Totals();
    g.bad.clear();
    g.log.clear();
    g.pending_copies.clear();
    g.fail.clear();
    g.gate = -1;
    if (g.live) g.bad.push_back("reset() while a session lives");
}
void fail_pass(long k) {
    std::lock_guard<std::mutex> lk(g.mu);
    g.fail.push_back(k);
}
std::string fail_text(long k) { return "toy session: injected failure of pass " + std::to_string(k); }
long last_pass_of(int slot, int pos) {
    std::lock_guard<std::mutex> lk(g.mu);
    if (slot < 0 || slot >= g.max_seq || pos < 0 || pos >= g.max_ctx) return -1;
    return g.row_pass[(size_t)slot * (size_t)g.max_ctx + (size_t)pos];
}
std::vector<std::pair<int, int>> rows_of_pass(long k) {
    std::lock_guard<std::mutex> lk(g.mu);
    if (k < 0 || k >= (long)g.log.size()) return {};
    return g.log[(size_t)k];
}
void close_gate(long k) {
    std::lock_guard<std::mutex> lk(g.mu);
    g.gate = k;
}
void open_gate() {
    std::lock_guard<std::mutex> lk(g.mu);
    g.gate = -1;
    g.cv.notify_all();
}
bool held() {
    std::lock_guard<std::mutex> lk(g.mu);
    return g.waiting;
}

}  // namespace toy

using namespace toy;

TkLlmModel::~TkLlmModel() {}

TkLlmSession::~TkLlmSession() {
    std::lock_guard<std::mutex> lk(g.mu);
    if (model) g.live--;
}

bool TkLlmSession::init(TkLlmModel* m, int seqs, int ctx) {
    std::lock_guard<std::mutex> lk(g.mu);
    if (g.live) { error = "toy session: one session at a time"; return false; }
    g.live++;
    model = m;
    max_seq = seqs;
    max_ctx = ctx;
    g.max_seq = seqs;
    g.max_ctx = ctx;
    g.cache.assign((size_t)seqs * (size_t)ctx, Row());
    g.row_pass.assign((size_t)seqs * (size_t)ctx, -1);
    return true;
}

bool TkLlmSession::forward(int nrows, const int32_t* seq, const int32_t* pos, const int32_t* tok, float* logits_host, int32_t* argmax_host, bool lm_head,
                           const uint32_t* const* row_masks, const TkSampleRow* row_samp, const TkLogitAdjust* row_adjust, const int32_t* row_ntop,
                           TkTokenLogprob* records_host) {
    std::unique_lock<std::mutex> lk(g.mu);
    if (logits_host) breach("the scheduler asks for logits");
    if (!check_rows(nrows, seq, pos, tok, false)) { g.t.passes++; g.log.emplace_back(); error = "toy session: a pass it cannot run"; return false; }
    /* the optional tables are given exactly when a row needs them */
    bool any_mask = false, any_samp = false, any_adj = false, any_lp = false;
    for (int r = 0; r < nrows; ++r) {
        any_mask = any_mask || (row_masks && row_masks[r]);
        any_samp = any_samp || (row_samp && row_samp[r].temp > 0.0f);
        any_adj = any_adj || (row_adjust && !row_adjust[r].neutral());
        any_lp = any_lp || (row_ntop && row_ntop[r] >= 0);
    }
    if ((row_masks != nullptr) != any_mask) breach("row_masks given without a masked row");
    if ((row_samp != nullptr) != any_samp) breach("row_samp given without a stochastic row");
    if ((row_adjust != nullptr) != any_adj) breach("row_adjust given without an adjusted row");
    if ((row_ntop != nullptr) != any_lp || (records_host != nullptr) != any_lp) breach("row_ntop / records_host given without a row that asks, or only one of them");
    if ((argmax_host != nullptr) != lm_head) breach("a head without a place for its picks, or the reverse");
    if (!lm_head && (row_masks || row_samp || row_adjust || row_ntop)) breach("sampling tables on a pass without a head");
    if (!enter_pass(lk, nrows, seq, pos, &error)) return false;
    for (int r = 0; r < nrows; ++r) {
        const uint64_t h = run_row(seq[r], pos[r], tok[r]);
        if (!argmax_host) continue;
        if (row_adjust && !row_adjust[r].neutral())
            if (const char* why = row_adjust[r].check(VOCAB)) breach(why, r);
        argmax_host[r] = pick(h, row_masks ? row_masks[r] : nullptr, row_samp ? &row_samp[r] : nullptr, row_adjust ? &row_adjust[r] : nullptr);
        if (row_ntop && records_host && row_ntop[r] >= 0) fill_record(h, row_ntop[r], &records_host[r]);
    }
    g.t.passes++;
    return true;
}

bool TkLlmSession::forward_verify(int nrows, const int32_t* seq, const int32_t* pos, const int32_t* tok, int form, float* logits_host, int32_t* picks_host,
                                  bool* bad_args) {
    std::unique_lock<std::mutex> lk(g.mu);
    if (bad_args) *bad_args = false;
    if (logits_host || !picks_host || form != -1) breach("the scheduler's verify pass: form -1, picks, no logits", form);
    if (!check_rows(nrows, seq, pos, tok, true)) { g.t.passes++; g.log.emplace_back(); error = "toy session: a pass it cannot run"; return false; }
    g.t.verify_passes++;
    if (!enter_pass(lk, nrows, seq, pos, &error)) return false;
    for (int r = 0; r < nrows; ++r) {
        const uint64_t h = run_row(seq[r], pos[r], tok[r]);
        if (picks_host) picks_host[r] = pick(h, nullptr, nullptr, nullptr);
    }
    g.t.passes++;
    return true;
}

bool TkLlmSession::enqueue_kv_copy(const TkKvCopyDesc* descs, int n) {
    std::lock_guard<std::mutex> lk(g.mu);
    g.t.copy_launches++;
    if (n < 1 || n > TK_MAX_ROWS || !descs) { breach("a copy launch of 1 .. TK_MAX_ROWS descriptors", n); error = "toy session: a copy launch it cannot run"; return false; }
    if (n > g.t.widest_copy) g.t.widest_copy = n;
    std::vector<char> src((size_t)g.max_seq, 0), dst((size_t)g.max_seq, 0);
    for (int i = 0; i < n; ++i) {
        const TkKvCopyDesc& c = descs[i];
        if (c.src_seq < 0 || c.src_seq >= g.max_seq || c.dst_seq < 0 || c.dst_seq >= g.max_seq || c.src_seq == c.dst_seq || c.p0 < 0 || c.n < 1 || c.p0 + c.n > g.max_ctx) {
            breach("a copy outside the cache, empty, or onto itself", c.src_seq, c.dst_seq, c.n);
            error = "toy session: a copy launch it cannot run";
            return false;
        }
        if (dst[(size_t)c.dst_seq]) breach("a slot is the destination of two copies of one launch", c.dst_seq);
        dst[(size_t)c.dst_seq] = 1;
        src[(size_t)c.src_seq] = 1;
    }
    for (int s = 0; s < g.max_seq; ++s)
        if (src[(size_t)s] && dst[(size_t)s]) breach("a slot is both a source and a destination of one launch", s);
    for (int i = 0; i < n; ++i) {
        const TkKvCopyDesc& c = descs[i];
        for (int p = c.p0; p < c.p0 + c.n; ++p) {
            if (!g.at(c.src_seq, p).valid) { breach("a copy reads a row that was never written", c.src_seq, p); break; }
        }
        for (int p = c.p0; p < c.p0 + c.n; ++p) g.at(c.dst_seq, p) = g.at(c.src_seq, p);
        g.t.copy_descs++;
        g.t.copy_rows += (uint64_t)c.n;
        g.pending_copies.push_back(c);
    }
    return true;
}

bool TkLlmSession::kv_shift(int seq, int p0, int p1, int delta, bool* bad_args) {
    std::lock_guard<std::mutex> lk(g.mu);
    if (bad_args) *bad_args = false;
    g.t.shifts++;
    if (seq < 0 || seq >= g.max_seq || !(0 <= p0 && p0 < p1 && p1 <= g.max_ctx) || delta >= 0 || p0 + delta < 0) {
        breach("shift arguments outside kv_shift's range", p0, p1, delta);
        if (bad_args) *bad_args = true;
        error = "toy session: a shift it cannot run";
        return false;
    }
    for (int p = p0; p < p1; ++p) {
        if (!g.at(seq, p).valid) { breach("a shift moves a row that was never written", seq, p); break; }
    }
    /* the rows keep the value they were computed with: as at the new position, in the old context.  The stale tail keeps its bits */
    for (int p = p0; p < p1; ++p) g.at(seq, p + delta) = g.at(seq, p);
    return true;
}
