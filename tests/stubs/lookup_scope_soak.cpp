/*
 * lookup_scope_soak.cpp — verify requests WITH TABLES (csrc/llm/tk_llm_batcher.h "Verify requests with tables", csrc/llm/tk_lookup_scope.h) through the
 * real scheduler, linked against the toy session (llm_session_toy.h), on the CPU.  Stand-alone: its own main, its own build line
 * (tests/test_lookup_scope_cpu.py), no HIP call.
 *
 *   lookup_scope_soak soak <threads> <seed> <calls> [fail_pass]
 *       Two thirds of the threads submit tabled verify requests: every row carries its own mask, sampling state (the base state, counter + i), adjustment
 *       and the request's n_top, in every combination of the four (call number mod 16; combination 0 is a request without tables).  The others
 *       drive plain traffic on their slots: prompts, one-row steps that run ahead, plain verify requests.  Every thread mirrors its own sequence
 *       with the pure functions of namespace toy and compares every id and every record exactly.
 *   lookup_scope_soak directed
 *       which session entry a pass takes, and the refusals: tables of the wrong length, n_top without records, records without n_top, limits.
 * Prints one JSON line; exit status 0 = the run ended (the line says what it found), 3 = the watchdog saw no progress, 2 = usage.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <mutex>
#include <thread>

#include "llm_session_toy.h"
#include "tk_llm_batcher.h"
#include "tk_lookup.h"
#include "tk_lookup_scope.h"

namespace {

using Ids = std::vector<int32_t>;
constexpr int MASK_WORDS = (toy::VOCAB + 31) / 32;
constexpr int N_CTX = 96;
constexpr int MAX_ROWS = TK_LOOKUP_MAX_DRAFT + 1;

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(toy::mix(seed, 0x5c09eull)) {}
    uint64_t next() { s = toy::mix(s, 0x2545f4914f6cdd1dull); return s; }
    int below(int n) { return (int)(next() % (uint64_t)n); }
    bool chance(int percent) { return below(100) < percent; }
    int32_t tok() { return (int32_t)below(toy::VOCAB); }
};

struct Counters {
    std::atomic<uint64_t> mismatches{0}, ops{0}, failed{0}, bad_error{0}, tabled{0}, by_combo[16], by_accepted[MAX_ROWS], eos_cut{0}, plain_verify{0}, steps{0}, prompts{0};
    std::mutex mu;
    std::vector<std::string> notes;
    Counters() { for (auto& v : by_combo) v = 0; for (auto& v : by_accepted) v = 0; }
    void mismatch(const std::string& what) {
        mismatches++;
        std::lock_guard<std::mutex> lk(mu);
        if (notes.size() < 12) notes.push_back(what);
    }
};

/* the tables of one request: row i's mask, adjustment (window and bias of its own) and the base sampling state */
struct Tables {
    uint32_t mask[MAX_ROWS][MASK_WORDS];
    const uint32_t* mask_ptr[MAX_ROWS];
    int32_t window[MAX_ROWS][8], bias_ids[MAX_ROWS][3];
    float bias[MAX_ROWS][3];
    TkLogitAdjust adj[MAX_ROWS];
    TkSampleRow samp;
    int32_t n_top;
    bool has_mask, has_samp, has_adj;
};

void make_tables(Rng& rng, int combo, int n, Tables* t) {
    *t = Tables{};
    t->has_mask = combo & 1; t->has_samp = combo & 2; t->has_adj = combo & 4;
    t->n_top = (combo & 8) ? rng.below(TK_LOGPROB_MAX_TOP + 1) : -1;
    t->samp = TkSampleRow{};
    if (t->has_samp) { t->samp.temp = 0.5f + 0.1f * (float)rng.below(8); t->samp.top_p = 0.95f; t->samp.min_p = 0.05f; t->samp.top_k = 40; t->samp.seed = rng.next(); t->samp.counter = (uint32_t)rng.below(100000); }
    for (int i = 0; i < n; ++i) {
        t->mask_ptr[i] = nullptr;
        if (t->has_mask && (i == 0 || !rng.chance(20))) { /* some rows of a masked request are unmasked: NULL entries */
            for (int w = 0; w < MASK_WORDS; ++w) t->mask[i][w] = (uint32_t)rng.next();
            if (toy::VOCAB % 32) t->mask[i][MASK_WORDS - 1] &= (1u << (toy::VOCAB % 32)) - 1u;
            const int one = rng.below(toy::VOCAB); /* never empty */
            t->mask[i][one >> 5] |= 1u << (one & 31);
            t->mask_ptr[i] = t->mask[i];
        }
        t->adj[i] = TkLogitAdjust{};
        t->adj[i].repeat = 1.0f; t->adj[i].freq = 0.0f; t->adj[i].present = 0.0f;
        if (t->has_adj && (i == 0 || !rng.chance(20))) { /* and some rows of an adjusted request are neutral */
            t->adj[i].repeat = 1.1f + 0.1f * (float)rng.below(4); t->adj[i].freq = 0.25f * (float)rng.below(3); t->adj[i].present = 0.5f * (float)rng.below(2);
            t->adj[i].n_recent = 1 + rng.below(8);
            for (int k = 0; k < t->adj[i].n_recent; ++k) t->window[i][k] = rng.tok();
            t->adj[i].recent = t->window[i];
            t->adj[i].n_bias = rng.below(4);
            for (int k = 0; k < t->adj[i].n_bias; ++k) { t->bias_ids[i][k] = (int32_t)((rng.below(toy::VOCAB / 3) * 3 + k) % toy::VOCAB); t->bias[i][k] = (float)rng.below(9) - 4.0f; }
            t->adj[i].bias_ids = t->bias_ids[i]; t->adj[i].bias = t->bias[i];
        }
    }
}

TkSampleRow row_samp(const Tables& t, int i) {
    TkSampleRow s = t.samp;
    s.counter = tk_lookup_row_counter(t.samp.counter, i);
    return s;
}

struct Client {
    TkLlmBatcher& b;
    Counters& c;
    int slot;
    std::vector<toy::Row> m;
    int n_past = 0;
    int32_t pending = -1;
    std::string err;
    Client(TkLlmBatcher& b_, Counters& c_, int slot_) : b(b_), c(c_), slot(slot_), m((size_t)N_CTX) {}
    std::string where(const char* what) const { return std::string(what) + " slot " + std::to_string(slot) + " n_past " + std::to_string(n_past); }
    uint64_t mirror_feed(int pos, int32_t tok) {
        m[(size_t)pos].h = toy::feed(pos ? &m[(size_t)pos - 1] : nullptr, tok);
        m[(size_t)pos].tok = tok;
        m[(size_t)pos].valid = true;
        return m[(size_t)pos].h;
    }
    bool fail(const char* what) {
        c.failed++;
        if (err.rfind("toy session: injected failure of pass ", 0) != 0) { c.bad_error++; c.mismatch(where(what) + ": error text '" + err + "'"); }
        return false;
    }
    bool feed_at(int pos0, const Ids& toks, const char* what) {
        int32_t got = -1;
        err.clear();
        const bool ok = b.submit(slot, pos0, toks.data(), (int)toks.size(), nullptr, &got, &err);
        c.ops++;
        if (!ok) return fail(what);
        uint64_t h = 0;
        for (size_t i = 0; i < toks.size(); ++i) h = mirror_feed(pos0 + (int)i, toks[i]);
        n_past = pos0 + (int)toks.size();
        const int32_t want = toy::pick(h, nullptr, nullptr, nullptr);
        if (got != want) c.mismatch(where(what) + ": id " + std::to_string(got) + ", the mirror says " + std::to_string(want));
        pending = want;
        return true;
    }
    bool prompt(Rng& rng) {
        Ids toks((size_t)(2 + rng.below(20)));
        for (int32_t& t : toks) t = rng.tok();
        c.prompts++;
        return feed_at(0, toks, "prompt");
    }
    bool step() { c.steps++; return feed_at(n_past, Ids{pending}, "step"); }
    /* the hashes of the rows that feeding toks at n_past writes, on a copy of the mirror's last row */
    std::vector<uint64_t> hashes_after(const Ids& toks) const {
        std::vector<uint64_t> hs;
        toy::Row prev;
        const toy::Row* p = n_past ? &m[(size_t)n_past - 1] : nullptr;
        for (int32_t t : toks) { prev.h = toy::feed(p, t); p = &prev; hs.push_back(prev.h); }
        return hs;
    }
    int32_t pick_of(uint64_t h, const Tables* t, int i) const {
        if (!t) return toy::pick(h, nullptr, nullptr, nullptr);
        const TkSampleRow s = row_samp(*t, i);
        return toy::pick(h, t->mask_ptr[i], &s, &t->adj[i]);
    }
    /* a verify request of n rows under the tables of `combo` (0: none); `right` of its drafts are the ids the mirror says the rows sample */
    bool verify(Rng& rng, int combo, int n, int right) {
        Tables t;
        make_tables(rng, combo, n, &t);
        const Tables* tp = combo ? &t : nullptr;
        Ids toks{pending};
        for (int i = 0; i + 1 < n; ++i) { /* draft i is what row i samples when it is to be right, another id otherwise */
            toks.push_back(0);
            const int32_t want = pick_of(hashes_after(toks)[(size_t)i], tp, i); /* the hash of row i does not depend on what stands behind it */
            toks.back() = i < right ? want : (int32_t)((want + 1 + rng.below(toy::VOCAB - 1)) % toy::VOCAB);
        }
        const std::vector<uint64_t> hs = hashes_after(toks);
        Ids picks((size_t)n), want((size_t)n, -1), got((size_t)n, -1);
        for (int i = 0; i < n; ++i) picks[(size_t)i] = pick_of(hs[(size_t)i], tp, i);
        const int n_want = tk_lookup_accept(toks.data(), picks.data(), n, toy::EOS, want.data());
        TkTokenLogprob recs[MAX_ROWS];
        memset(recs, 0xff, sizeof recs);
        int n_got = 0;
        err.clear();
        const bool ok = combo ? b.submit_verify(slot, n_past, toks.data(), n, got.data(), &n_got, &err, t.has_mask ? t.mask_ptr : nullptr, t.has_samp ? &t.samp : nullptr,
                                                t.has_adj ? t.adj : nullptr, t.n_top, t.n_top >= 0 ? recs : nullptr, t.has_mask || t.has_adj || t.n_top >= 0 ? n : 0)
                              : b.submit_verify(slot, n_past, toks.data(), n, got.data(), &n_got, &err);
        c.ops++;
        if (!ok) return fail("verify");
        got.resize((size_t)(n_got > 0 && n_got <= n ? n_got : 0));
        want.resize((size_t)n_want);
        if (got != want) c.mismatch(where("verify") + " combination " + std::to_string(combo) + ": " + std::to_string(n_got) + " ids, the mirror says " + std::to_string(n_want) + " or other ids");
        for (int i = 0; i < n_want && combo && t.n_top >= 0; ++i) {
            TkTokenLogprob wr;
            memset(&wr, 0, sizeof wr);
            toy::fill_record(hs[(size_t)i], t.n_top, &wr);
            if (!toy::same_record(recs[i], wr)) c.mismatch(where("verify") + ": record " + std::to_string(i) + " differs from the mirror's");
        }
        for (int i = n_want; i < n && combo && t.n_top >= 0; ++i) { /* records behind the kept ids stay the caller's bytes */
            const unsigned char* p = (const unsigned char*)&recs[i];
            for (size_t k = 0; k < sizeof recs[i]; ++k)
                if (p[k] != 0xff) { c.mismatch(where("verify") + ": record " + std::to_string(i) + " behind the kept ids was written"); break; }
        }
        for (int i = 0; i < n_want; ++i) mirror_feed(n_past + i, toks[(size_t)i]);
        n_past += n_want;
        pending = want.back();
        (combo ? c.tabled : c.plain_verify)++;
        c.by_combo[combo]++;
        c.by_accepted[n_want - 1]++;
        if (pending == toy::EOS && n_want < n) c.eos_cut++;
        return true;
    }
};

struct Watchdog {
    std::atomic<bool> stop{false};
    std::thread t;
    Watchdog(Counters* c, int seconds) {
        t = std::thread([=] {
            uint64_t last = c->ops;
            auto since = std::chrono::steady_clock::now();
            while (!stop) {
                std::this_thread::sleep_for(std::chrono::milliseconds(50));
                const uint64_t now = c->ops;
                if (now != last) { last = now; since = std::chrono::steady_clock::now(); continue; }
                if (std::chrono::steady_clock::now() - since < std::chrono::seconds(seconds)) continue;
                fprintf(stderr, "watchdog: no call finished for %d s after %llu calls\n", seconds, (unsigned long long)now);
                for (const std::string& s : toy::breaches()) fprintf(stderr, "  breach: %s\n", s.c_str());
                _exit(3);
            }
        });
    }
    ~Watchdog() { stop = true; t.join(); }
};

TkLlmModel* the_model() {
    static TkLlmModel model;
    model.hp.vocab = toy::VOCAB;
    model.hp.head_dim = 64;
    return &model;
}

void print_common(const Counters& c, const char* extra) {
    const std::vector<std::string> bad = toy::breaches();
    printf("{\"mismatches\": %llu, \"notes\": [", (unsigned long long)c.mismatches.load());
    for (size_t i = 0; i < c.notes.size(); ++i) printf("%s\"%s\"", i ? ", " : "", c.notes[i].c_str());
    printf("], \"breaches\": %zu, \"breach_list\": [", bad.size());
    for (size_t i = 0; i < bad.size(); ++i) printf("%s\"%s\"", i ? ", " : "", bad[i].c_str());
    printf("]%s}\n", extra);
}

int soak(int threads, uint64_t seed, int calls, long fail_pass) {
    toy::reset();
    if (fail_pass >= 0) toy::fail_pass(fail_pass);
    Counters c;
    {
        TkLlmBatcher b;
        std::string err;
        if (!b.init(the_model(), threads, N_CTX, toy::EOS, &err)) { fprintf(stderr, "init: %s\n", err.c_str()); return 2; }
        Watchdog dog(&c, 10);
        std::vector<std::thread> ts;
        for (int k = 0; k < threads; ++k)
            ts.emplace_back([&, k] {
                Rng rng(seed * 1000 + (uint64_t)k);
                Client cl(b, c, b.acquire_slot());
                const bool tabled = k % 3 != 2;
                bool live = false;
                for (int call = 0; call < calls; ++call) {
                    if (!live || cl.pending == toy::EOS || cl.n_past + MAX_ROWS + 2 >= N_CTX) { live = cl.prompt(rng); continue; }
                    if (tabled) {
                        const int n = 1 + rng.below(MAX_ROWS);
                        live = cl.verify(rng, (call + k) % 16, n, rng.chance(60) ? n - 1 : rng.below(n));
                    } else if (rng.chance(70)) {
                        live = cl.step(); /* a plain step: its row runs ahead */
                    } else {
                        const int n = 1 + rng.below(MAX_ROWS);
                        live = cl.verify(rng, 0, n, rng.below(n));
                    }
                }
                b.release_slot(cl.slot);
            });
        for (std::thread& t : ts) t.join();
    }
    const toy::Totals t = toy::totals();
    char extra[1024];
    int at = snprintf(extra, sizeof extra, ", \"tabled\": %llu, \"plain_verify\": %llu, \"steps\": %llu, \"prompts\": %llu, \"eos_cut\": %llu, \"failed_requests\": %llu, \"bad_errors\": %llu, "
                      "\"passes\": %llu, \"verify_passes\": %llu, \"failed_passes\": %llu, \"widest\": %d, \"by_combo\": [",
                      (unsigned long long)c.tabled.load(), (unsigned long long)c.plain_verify.load(), (unsigned long long)c.steps.load(), (unsigned long long)c.prompts.load(),
                      (unsigned long long)c.eos_cut.load(), (unsigned long long)c.failed.load(), (unsigned long long)c.bad_error.load(), (unsigned long long)t.passes,
                      (unsigned long long)t.verify_passes, (unsigned long long)t.failed_passes, t.widest);
    for (int i = 0; i < 16; ++i) at += snprintf(extra + at, sizeof extra - (size_t)at, "%s%llu", i ? ", " : "", (unsigned long long)c.by_combo[i].load());
    at += snprintf(extra + at, sizeof extra - (size_t)at, "], \"by_accepted\": [");
    for (int i = 0; i < MAX_ROWS; ++i) at += snprintf(extra + at, sizeof extra - (size_t)at, "%s%llu", i ? ", " : "", (unsigned long long)c.by_accepted[i].load());
    snprintf(extra + at, sizeof extra - (size_t)at, "]");
    print_common(c, extra);
    return 0;
}

/* one client, in lock step: which session entry a pass takes, and what submit_verify refuses before anything is queued */
int directed() {
    toy::reset();
    Counters c;
    std::vector<std::string> failures;
    auto expect = [&](bool cond, const char* what) { if (!cond) failures.push_back(what); };
    {
        TkLlmBatcher b;
        std::string err;
        if (!b.init(the_model(), 2, N_CTX, toy::EOS, &err)) { fprintf(stderr, "init: %s\n", err.c_str()); return 2; }
        Watchdog dog(&c, 10);
        Rng rng(7);
        Client cl(b, c, b.acquire_slot());
        int32_t first = 5, got0 = -1;
        expect(b.submit(cl.slot, 0, &first, 1, nullptr, &got0, &err, nullptr, nullptr, nullptr, true), "the prompt row");
        cl.mirror_feed(0, first);
        cl.n_past = 1;
        cl.pending = toy::pick(cl.m[0].h, nullptr, nullptr, nullptr);
        expect(got0 == cl.pending, "the prompt row's id");
        expect(cl.verify(rng, 0, 4, 3), "a verify request without tables");
        expect(toy::totals().passes == 2 && toy::totals().verify_passes == 1, "a verify request without tables takes forward_verify");
        for (int combo = 1; combo < 16 && cl.pending != toy::EOS; ++combo) {
            const uint64_t before = toy::totals().passes;
            expect(cl.verify(rng, combo, 4, 3), "a verify request with tables");
            expect(toy::totals().passes == before + 1 && toy::totals().verify_passes == 1, "a verify request with tables takes forward() in one pass");
            expect(toy::rows_of_pass((long)before).size() == 4, "all rows of a verify request enter one pass");
        }
        /* the refusals: nothing reaches the session */
        const uint64_t passes = toy::totals().passes;
        Tables t;
        make_tables(rng, 15, 4, &t);
        int32_t toks[4] = {cl.pending, 3, 4, 5}, ids[4];
        int n_ids = 0;
        TkTokenLogprob recs[4];
        expect(!b.submit_verify(cl.slot, cl.n_past, toks, 4, ids, &n_ids, &err, t.mask_ptr, nullptr, nullptr, -1, nullptr, 3), "masks of the wrong length");
        expect(!b.submit_verify(cl.slot, cl.n_past, toks, 4, ids, &n_ids, &err, t.mask_ptr), "masks without a length");
        expect(!b.submit_verify(cl.slot, cl.n_past, toks, 4, ids, &n_ids, &err, nullptr, nullptr, t.adj, -1, nullptr, 5), "adjustments of the wrong length");
        expect(!b.submit_verify(cl.slot, cl.n_past, toks, 4, ids, &n_ids, &err, nullptr, nullptr, nullptr, 3, recs, 2), "records of the wrong length");
        expect(!b.submit_verify(cl.slot, cl.n_past, toks, 4, ids, &n_ids, &err, nullptr, nullptr, nullptr, 3, nullptr, 4), "n_top without records");
        expect(!b.submit_verify(cl.slot, cl.n_past, toks, 4, ids, &n_ids, &err, nullptr, nullptr, nullptr, -1, recs, 4), "records without n_top");
        expect(!b.submit_verify(cl.slot, cl.n_past, toks, 4, ids, &n_ids, &err, nullptr, nullptr, nullptr, TK_LOGPROB_MAX_TOP + 1, recs, 4), "n_top above the limit");
        t.adj[2].n_recent = TK_ADJUST_MAX_RECENT + 1;
        expect(!b.submit_verify(cl.slot, cl.n_past, toks, 4, ids, &n_ids, &err, nullptr, nullptr, t.adj, -1, nullptr, 4), "an adjustment beyond its limits");
        expect(err.find("row 2") != std::string::npos, "the refusal names the row");
        expect(toy::totals().passes == passes, "a refused request reaches the session");
        /* and the scheduler still serves the slot */
        if (cl.pending != toy::EOS) expect(cl.verify(rng, 15, 3, 2), "a request after the refusals");
        /* a failing pass: the tabled request fails with the session's error, nothing is handed over; a new prompt, and the ids are right again */
        const long k = (long)toy::totals().passes;
        toy::fail_pass(k);
        const int n_before = cl.n_past;
        expect(!cl.verify(rng, 15, 4, 3) && cl.err == toy::fail_text(k) && c.failed == 1 && c.bad_error == 0, "a tabled request of a failing pass fails with the session's error");
        expect(cl.n_past == n_before && toy::totals().failed_passes == 1, "a failed request moves nothing");
        expect(cl.prompt(rng) && (cl.pending == toy::EOS || cl.verify(rng, 15, 4, 3)), "the slot after a failed pass");
        b.release_slot(cl.slot);
    }
    std::string extra = ", \"failures\": [";
    for (size_t i = 0; i < failures.size(); ++i) extra += std::string(i ? ", " : "") + "\"" + failures[i] + "\"";
    extra += "]";
    print_common(c, extra.c_str());
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 5 && !strcmp(argv[1], "soak")) return soak(atoi(argv[2]), (uint64_t)atoll(argv[3]), atoi(argv[4]), argc > 5 ? atol(argv[5]) : -1);
    if (argc == 2 && !strcmp(argv[1], "directed")) return directed();
    fprintf(stderr, "usage: lookup_scope_soak soak <threads> <seed> <calls> [fail_pass] | directed\n");
    return 2;
}
