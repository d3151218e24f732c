/*
 * batcher_soak.cpp — the real scheduler (csrc/llm/tk_llm_batcher.cpp) linked against the toy session (llm_session_toy.h), on the CPU.
 *
 *   batcher_soak soak RUNNERS SEED OPS [FAIL_PASS]   R runner threads, each with a seeded script; FAIL_PASS >= 0 makes that pass fail
 *   batcher_soak scenario NAME                       one directed scenario (the list is at the end of this file)
 *
 * Every runner keeps a private mirror of its own sequence, computed single-threaded with the toy's pure functions and fed from scratch for every
 * new prompt, and compares every id and every log-probability record with it the moment the scheduler returns it: exactly, there is no tolerance.
 * A script is drawn from the seed and from nothing that depends on timing (ids do not: that is the scheduler's contract).
 *
 * Accounting at quiescence (every slot released, then one held one-row request, which the scheduler thread runs after every row that was still in
 * flight).  From tk_llm_batcher.cpp: rows_ counts every row of every request when its pass completes — all n rows of a verify request, rejected ones
 * included, and the rows of a failed pass — and one per run-ahead row its owner takes; wasted_ counts every run-ahead row that ran and was not
 * taken.  A run-ahead row of a FAILED pass that its owner does take is counted in neither.  So
 *     stats().rows + wasted + (failed run-ahead rows taken) == the rows the session ran
 * with the third term 0 in a run without a failure, and at most the number of failed requests otherwise;
 *     prompt_rows >= kept + copied;     copy launches and copied rows counted by the scheduler == those the session saw.
 *
 * Prints one JSON line; exit status 0 = the run ended (the line says what it found), 3 = the watchdog saw no progress, 2 = usage.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>

#include "llm_session_toy.h"
#include "tk_llm_batcher.h"
#include "tk_lookup.h"

namespace {

using Ids = std::vector<int32_t>;
constexpr int MASK_WORDS = (toy::VOCAB + 31) / 32;

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(toy::mix(seed, 0x5eedull)) {}
    uint64_t next() { s = toy::mix(s, 0x2545f4914f6cdd1dull); return s; }
    int below(int n) { return (int)(next() % (uint64_t)n); }
    bool chance(int percent) { return below(100) < percent; }
    int32_t tok() { return (int32_t)below(toy::VOCAB); }
};

struct Counters {
    std::atomic<uint64_t> mismatches{0}, ops{0}, kept{0}, copied{0}, shifts{0}, verify_by_accepted[TK_LOOKUP_MAX_DRAFT + 1], verify_eos{0}, waiter{0}, done_rec{0},
        done_norec{0}, failed{0}, bad_error{0}, prompts{0}, tool_feeds{0}, abandoned{0}, reacquired{0}, toggles{0}, empty_window{0};
    std::mutex mu;
    std::vector<std::string> notes; /* the first mismatches, in words */
    Counters() { for (auto& v : verify_by_accepted) v = 0; }
    void mismatch(const std::string& what) {
        mismatches++;
        std::lock_guard<std::mutex> lk(mu);
        if (notes.size() < 12) notes.push_back(what);
    }
};

/* one runner's view of its slot: the calls of the scheduler, each followed by the same step on the mirror and the comparison */
struct Client {
    TkLlmBatcher& b;
    Counters& c;
    int slot;
    std::vector<toy::Row> m; /* the mirror: rows [0, n_past) */
    int n_past = 0;
    int32_t pending = -1; /* the id sampled last: fed at n_past next */
    std::string err;
    bool failed_call = false; /* the last call returned false */
    /* what the scheduler planned ahead of the last call, when the contract says it did */
    bool ahead = false;
    int32_t ahead_ntop = -1;
    struct Opt {
        const uint32_t* mask = nullptr;
        const TkSampleRow* samp = nullptr;
        const TkLogitAdjust* adj = nullptr;
        bool hold = false;
        int32_t n_top = -1;
    };
    Client(TkLlmBatcher& b_, Counters& c_, int slot_) : b(b_), c(c_), slot(slot_), m((size_t)b_.n_ctx()) {}
    std::string where(const char* what) const { return std::string(what) + " slot " + std::to_string(slot) + " n_past " + std::to_string(n_past); }
    uint64_t mirror_feed(int pos, int32_t tok) {
        m[(size_t)pos].h = toy::feed(pos ? &m[(size_t)pos - 1] : nullptr, tok);
        m[(size_t)pos].tok = tok;
        m[(size_t)pos].valid = true;
        return m[(size_t)pos].h;
    }
    bool fail(const char* what) {
        failed_call = true;
        ahead = false;
        c.failed++;
        if (err.rfind("toy session: injected failure of pass ", 0) != 0) { c.bad_error++; c.mismatch(where(what) + ": error text '" + err + "'"); }
        return false;
    }
    /* feed toks at pos0 (0 with a prompt, n_past otherwise) */
    bool feed_at(int pos0, const Ids& toks, const Opt& o, TkLlmBatcher::PrefixRows* prefix, const char* what) {
        int32_t got = -1;
        TkTokenLogprob rec;
        memset(&rec, 0xff, sizeof rec);
        const int n = (int)toks.size();
        /* which way a one-row step that finds its row run ahead is served: by the pass that carries it, or from the finished row */
        int served = 0;
        const bool adjusted = o.adj && !o.adj->neutral();
        if (ahead && !prefix && n == 1 && !o.mask && !(o.samp && o.samp->temp > 0.0f) && !adjusted && toks[0] == pending && o.n_top == ahead_ntop) {
            uint64_t passes = 0;
            b.stats(&passes, nullptr, nullptr);
            const long q = toy::last_pass_of(slot, pos0), before = toy::last_pass_of(slot, pos0 - 1);
            served = (q > before && q < (long)passes) ? 2 : 1;
        }
        err.clear();
        failed_call = false;
        const bool ok = b.submit(slot, pos0, toks.data(), n, o.mask, &got, &err, o.samp, prefix, o.adj, o.hold, o.n_top, o.n_top >= 0 ? &rec : nullptr);
        c.ops++;
        if (!ok) return fail(what);
        if (served == 1) c.waiter++;
        if (served == 2) (o.n_top >= 0 ? c.done_rec : c.done_norec)++;
        uint64_t h = 0;
        for (int i = 0; i < n; ++i) h = mirror_feed(pos0 + i, toks[(size_t)i]);
        n_past = pos0 + n;
        const int32_t want = toy::pick(h, o.mask, o.samp, o.adj);
        if (got != want) c.mismatch(where(what) + ": id " + std::to_string(got) + ", the mirror says " + std::to_string(want));
        if (o.n_top >= 0) {
            TkTokenLogprob wr;
            memset(&wr, 0, sizeof wr);
            toy::fill_record(h, o.n_top, &wr);
            if (!toy::same_record(rec, wr)) c.mismatch(where(what) + ": log-probability record differs from the mirror's");
        }
        pending = got;
        /* the header's rule for a row ahead of this one */
        const bool penalties = o.adj && (o.adj->repeat != 1.0f || o.adj->freq != 0.0f || o.adj->present != 0.0f);
        ahead = !o.mask && !(o.samp && o.samp->temp > 0.0f) && !adjusted && !penalties && !o.hold && got != toy::EOS && (n_past - 1) + 2 < b.n_ctx();
        ahead_ntop = o.n_top;
        return true;
    }
    bool prompt(const Ids& toks, const Opt& o, TkLlmBatcher::PrefixRows* out = nullptr) {
        TkLlmBatcher::PrefixRows pr;
        ahead = false;
        const bool ok = feed_at(0, toks, o, &pr, "prompt");
        c.prompts++;
        if (out) *out = pr;
        c.kept += (uint64_t)pr.kept;
        c.copied += (uint64_t)pr.copied;
        if (!ok) return false;
        if (pr.prompt_rows != (int)toks.size() || pr.kept < 0 || pr.copied < 0 || pr.kept + pr.copied > (int)toks.size() - 1)
            c.mismatch(where("prompt") + ": rows " + std::to_string(pr.prompt_rows) + " kept " + std::to_string(pr.kept) + " copied " + std::to_string(pr.copied));
        return true;
    }
    bool step(const Opt& o) { return feed_at(n_past, Ids{pending}, o, nullptr, "step"); }
    bool feed(const Ids& toks, const Opt& o) { return feed_at(n_past, toks, o, nullptr, "feed"); }
    /* what one-row greedy passes would sample after feeding toks at n_past, on a copy of the mirror's last row */
    Ids greedy_after(const Ids& toks) const {
        Ids picks;
        toy::Row prev;
        const toy::Row* p = n_past ? &m[(size_t)n_past - 1] : nullptr;
        for (int32_t t : toks) {
            prev.h = toy::feed(p, t);
            p = &prev;
            picks.push_back(toy::pick(prev.h, nullptr, nullptr, nullptr));
        }
        return picks;
    }
    /* the pending id and `drafts` as one verify request; *accepted = m */
    bool verify(const Ids& drafts, int* accepted = nullptr) {
        Ids toks{pending};
        toks.insert(toks.end(), drafts.begin(), drafts.end());
        const int n = (int)toks.size();
        Ids got((size_t)n, -1), want((size_t)n, -1);
        int n_got = 0;
        ahead = false;
        err.clear();
        failed_call = false;
        const bool ok = b.submit_verify(slot, n_past, toks.data(), n, got.data(), &n_got, &err);
        c.ops++;
        if (!ok) return fail("verify");
        const Ids picks = greedy_after(toks);
        const int n_want = tk_lookup_accept(toks.data(), picks.data(), n, toy::EOS, want.data());
        got.resize((size_t)(n_got > 0 && n_got <= n ? n_got : 0));
        want.resize((size_t)n_want);
        if (got != want) c.mismatch(where("verify") + ": " + std::to_string(n_got) + " ids, the mirror says " + std::to_string(n_want) + " or other ids");
        for (int i = 0; i < n_want; ++i) mirror_feed(n_past + i, toks[(size_t)i]);
        n_past += n_want;
        pending = want.back();
        c.verify_by_accepted[n_want - 1]++;
        if (pending == toy::EOS && n_want < n) c.verify_eos++;
        if (accepted) *accepted = n_want - 1;
        return true;
    }
    bool shift(int n_keep, int n_discard) {
        err.clear();
        failed_call = false;
        const bool ok = b.shift(slot, n_keep, n_discard, n_past, &err);
        c.ops++;
        if (!ok) return fail("shift");
        for (int p = n_keep + n_discard; p < n_past; ++p) m[(size_t)p - (size_t)n_discard] = m[(size_t)p];
        n_past -= n_discard;
        c.shifts++;
        /* the shift retires what ran ahead; the pending id is fed at the new n_past */
        ahead = false;
        return true;
    }
};

/* the watchdog: no finished call for `seconds` -> say what can be seen and leave */
struct Watchdog {
    std::atomic<bool> stop{false};
    std::thread t;
    Watchdog(TkLlmBatcher* b, Counters* c, int seconds) {
        t = std::thread([=] {
            uint64_t last = c->ops;
            auto since = std::chrono::steady_clock::now();
            while (!stop) {
                std::this_thread::sleep_for(std::chrono::milliseconds(50));
                const uint64_t now = c->ops;
                if (now != last) { last = now; since = std::chrono::steady_clock::now(); continue; }
                if (std::chrono::steady_clock::now() - since < std::chrono::seconds(seconds)) continue;
                uint64_t passes = 0, rows = 0, wasted = 0;
                int widest = 0;
                b->stats(&passes, &rows, &widest, &wasted);
                const toy::Totals t = toy::totals();
                fprintf(stderr, "watchdog: no call finished for %d s after %llu calls; scheduler passes %llu rows %llu wasted %llu widest %d; session passes %llu rows %llu held %d\n",
                        seconds, (unsigned long long)now, (unsigned long long)passes, (unsigned long long)rows, (unsigned long long)wasted, widest,
                        (unsigned long long)t.passes, (unsigned long long)t.rows, (int)toy::held());
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

/* quiescence: a held one-row request on a free slot; when it returns, every row that was in flight has been retired */
void drain(TkLlmBatcher& b, Counters& c) {
    const int slot = b.acquire_slot();
    int32_t tok = 1, got = -1;
    std::string err;
    if (slot < 0 || !b.submit(slot, 0, &tok, 1, nullptr, &got, &err, nullptr, nullptr, nullptr, true)) c.mismatch("the quiescence request failed: " + err);
    c.ops++;
    if (slot >= 0) b.release_slot(slot);
}

std::string json_list(const std::vector<std::string>& v) {
    std::string s = "[";
    for (size_t i = 0; i < v.size(); ++i) {
        s += i ? ", \"" : "\"";
        for (char ch : v[i]) s += (ch == '"' || ch == '\\') ? '\'' : ch;
        s += "\"";
    }
    return s + "]";
}

/* ---- the soak ------------------------------------------------------------------------------------------------------------------------------ */

int soak(int R, uint64_t seed, int ops, long fail_at) {
    const int n_ctx = 96, slots = R + 2;
    toy::reset();
    if (fail_at >= 0) toy::fail_pass(fail_at);
    Counters c;
    /* prompts share prefixes from a small pool, so that rows are kept and copied */
    Rng pool_rng(seed * 1000003ull + 17);
    std::vector<Ids> pool(6);
    for (Ids& p : pool) {
        p.resize((size_t)(18 + pool_rng.below(24)));
        for (int32_t& t : p) t = pool_rng.tok();
    }
    for (int i = 1; i < 6; i += 2) /* some pool entries share their own first rows with the entry before them */
        for (size_t k = 0; k < 17 && k < pool[(size_t)i].size() && k < pool[(size_t)i - 1].size(); ++k) pool[(size_t)i][k] = pool[(size_t)i - 1][k];
    int rc = 0;
    {
        TkLlmBatcher b;
        std::string err;
        if (!b.init(the_model(), slots, n_ctx, toy::EOS, &err)) { fprintf(stderr, "init: %s\n", err.c_str()); return 2; }
        b.set_prefix_cache(true);
        Watchdog dog(&b, &c, 10);
        auto runner = [&](int id) {
            Rng r(seed * 7919ull + (uint64_t)id);
            int slot = -1;
            while (slot < 0) slot = b.acquire_slot();
            auto cl = std::make_unique<Client>(b, c, slot);
            int left = ops;
            uint32_t counter = 0;
            bool cache_off = false;
            while (left > 0) {
                /* a generation: its mode holds from the prompt to its end, as a runner's settings do */
                const int mode = r.below(6); /* 0, 1 plain; 2 masked; 3 stochastic; 4 penalties and bias; 5 lookup */
                const bool shifts = r.chance(60);
                int32_t n_top = r.chance(35) ? r.below(6) : -1;
                Ids prompt = pool[(size_t)r.below(6)];
                if (r.chance(30)) prompt.resize((size_t)(8 + r.below((int)prompt.size() - 8)));
                for (int k = r.below(7); k > 0; --k) prompt.push_back(r.tok());
                const int gen0 = (int)prompt.size();
                uint32_t mask[MASK_WORDS];
                TkSampleRow samp{};
                TkLogitAdjust adj;
                Ids recent, bias_ids;
                std::vector<float> bias;
                bool lookup_on = mode == 5;
                auto options = [&]() {
                    Client::Opt o;
                    o.n_top = n_top;
                    if (mode == 2) {
                        for (uint32_t& w : mask) w = (uint32_t)r.next();
                        mask[0] |= 1u << r.below(32); /* never empty */
                        o.mask = mask;
                    }
                    if (mode == 3) {
                        samp.temp = 0.8f; samp.top_p = 0.95f; samp.min_p = 0.05f; samp.top_k = 40;
                        samp.seed = seed + (uint64_t)id;
                        samp.counter = counter++;
                        o.samp = &samp;
                    }
                    if (mode == 4) {
                        /* the window: what was generated so far, at most 8 ids — empty at the prompt's sampled row, where the penalties are on already */
                        recent.clear();
                        for (int p = std::max(gen0, cl->n_past - 8); p < cl->n_past; ++p) recent.push_back(cl->m[(size_t)p].tok);
                        if (cl->n_past >= gen0 && cl->pending >= 0) recent.push_back(cl->pending);
                        adj = TkLogitAdjust();
                        adj.repeat = 1.25f; adj.freq = 0.125f; adj.present = r.chance(50) ? 0.5f : 0.0f;
                        adj.n_recent = (int32_t)recent.size();
                        adj.recent = recent.data();
                        bias_ids.clear(); bias.clear();
                        if (r.chance(50))
                            for (int k = r.below(3); k >= 0; --k) {
                                const int32_t t = r.tok();
                                if (std::find(bias_ids.begin(), bias_ids.end(), t) == bias_ids.end()) { bias_ids.push_back(t); bias.push_back((float)r.below(9) - 4.0f); }
                            }
                        adj.n_bias = (int32_t)bias_ids.size();
                        adj.bias_ids = bias_ids.data();
                        adj.bias = bias.data();
                        if (adj.neutral()) c.empty_window++;
                        o.adj = &adj;
                    }
                    o.hold = lookup_on;
                    return o;
                };
                if (id == 0) { /* the cache goes off for one of this runner's prompts (and whatever the others start meanwhile), then on again */
                    const bool off = r.chance(25);
                    if (off != cache_off) { b.set_prefix_cache(!off); c.toggles++; cache_off = off; }
                }
                cl->n_past = 0;
                cl->pending = -1;
                --left;
                if (!cl->prompt(prompt, options())) continue;
                int budget = 4 + r.below(70);
                while (left > 0 && budget > 0 && cl->pending != toy::EOS) {
                    --left;
                    --budget;
                    if (r.chance(2)) { c.abandoned++; break; } /* the owner goes another way with a row ahead of it */
                    if (cl->n_past + 1 >= n_ctx || (shifts && cl->n_past > 24 && r.chance(3))) {
                        if (!shifts) break;
                        const int n_keep = r.below(cl->n_past / 2), n_discard = std::max(1, (cl->n_past - n_keep) / (2 + r.below(3)));
                        if (!cl->shift(n_keep, n_discard)) break;
                        continue;
                    }
                    if (r.chance(4)) n_top = r.chance(50) ? r.below(6) : -1; /* changed between steps */
                    if (mode != 5 && r.chance(3)) lookup_on = !lookup_on;        /* lookup switched on with a row ahead, and off again */
                    if (r.chance(4) && cl->n_past + 8 < n_ctx) { /* a tool response: several tokens at n_past */
                        Ids toks{cl->pending};
                        for (int k = 1 + r.below(5); k > 0; --k) toks.push_back(r.tok());
                        c.tool_feeds++;
                        if (!cl->feed(toks, options())) break;
                        continue;
                    }
                    if (lookup_on && mode == 5 && r.chance(85)) {
                        const int room = std::min(TK_LOOKUP_MAX_DRAFT, n_ctx - cl->n_past - 1);
                        const int n_draft = r.chance(40) ? room : r.below(room + 1);
                        /* drafts: the first k are what the model itself continues with, the rest are wrong */
                        Ids drafts, toks{cl->pending};
                        const int k_right = r.chance(30) ? n_draft : r.below(n_draft + 1);
                        for (int i = 0; i < n_draft; ++i) {
                            const int32_t right = cl->greedy_after(toks).back();
                            const int32_t d = i < k_right ? right : (int32_t)((right + 1 + r.below(toy::VOCAB - 1)) % toy::VOCAB);
                            drafts.push_back(d);
                            toks.push_back(d);
                        }
                        if (!cl->verify(drafts)) break;
                        continue;
                    }
                    if (!cl->step(options())) break;
                }
                if (r.chance(12)) { /* the runner moves to the lowest free slot and gives its own back: whoever asks next gets that one, with its records */
                    int s = -1;
                    while (s < 0) s = b.acquire_slot();
                    b.release_slot(cl->slot);
                    c.reacquired++;
                    cl->slot = s;
                    cl->ahead = false;
                }
            }
            b.release_slot(cl->slot);
        };
        std::vector<std::thread> threads;
        for (int i = 0; i < R; ++i) threads.emplace_back(runner, i);
        for (std::thread& t : threads) t.join();
        drain(b, c);
        uint64_t passes = 0, rows = 0, wasted = 0, prompt_rows = 0, kept = 0, copied = 0, launches = 0;
        int widest = 0;
        b.stats(&passes, &rows, &widest, &wasted);
        b.prefix_stats(&prompt_rows, &kept, &copied, &launches);
        const toy::Totals t = toy::totals();
        std::vector<std::string> acc;
        const uint64_t slack = fail_at >= 0 ? c.failed.load() : 0;
        if (rows + wasted > t.rows || rows + wasted + slack < t.rows) acc.push_back("rows " + std::to_string(rows) + " + wasted " + std::to_string(wasted) + " against the session's " + std::to_string(t.rows));
        if (passes != t.passes || widest != t.widest) acc.push_back("passes or widest pass differ from the session's");
        if (prompt_rows < kept + copied) acc.push_back("prompt_rows < kept + copied");
        if (launches != t.copy_launches || copied != t.copy_rows) acc.push_back("copy launches or copied rows differ from the session's");
        if (kept != c.kept || copied != c.copied) acc.push_back("kept or copied differ from what the runners were told");
        if (t.shifts != c.shifts) acc.push_back("shifts differ from the session's");
        std::vector<std::string> br = toy::breaches();
        printf("{\"mode\": \"soak\", \"runners\": %d, \"seed\": %llu, \"calls\": %llu, \"mismatches\": %llu, \"breaches\": %zu, \"accounting_errors\": %zu, \"passes\": %llu, \"widest\": %d, "
               "\"rows\": %llu, \"session_rows\": %llu, \"kept\": %llu, \"copied\": %llu, \"copy_launches\": %llu, \"wasted\": %llu, \"shifts\": %llu, \"verify_passes\": %llu, \"verify_by_accepted\": [",
               R, (unsigned long long)seed, (unsigned long long)c.ops.load(), (unsigned long long)c.mismatches.load(), br.size(), acc.size(), (unsigned long long)passes, widest,
               (unsigned long long)rows, (unsigned long long)t.rows, (unsigned long long)kept, (unsigned long long)copied, (unsigned long long)launches, (unsigned long long)wasted,
               (unsigned long long)c.shifts.load(), (unsigned long long)t.verify_passes);
        for (int i = 0; i <= TK_LOOKUP_MAX_DRAFT; ++i) printf("%s%llu", i ? ", " : "", (unsigned long long)c.verify_by_accepted[i].load());
        printf("], \"verify_eos\": %llu, \"waiter_handovers\": %llu, \"done_handovers_with_record\": %llu, \"done_handovers_without_record\": %llu, \"failed_requests\": %llu, "
               "\"failed_passes\": %llu, \"prompts\": %llu, \"tool_feeds\": %llu, \"abandoned\": %llu, \"slot_changes\": %llu, \"cache_toggles\": %llu, \"penalties_over_empty_window\": %llu, "
               "\"notes\": %s, \"breach_list\": %s, \"accounting\": %s}\n",
               (unsigned long long)c.verify_eos.load(), (unsigned long long)c.waiter.load(), (unsigned long long)c.done_rec.load(), (unsigned long long)c.done_norec.load(),
               (unsigned long long)c.failed.load(), (unsigned long long)t.failed_passes, (unsigned long long)c.prompts.load(), (unsigned long long)c.tool_feeds.load(),
               (unsigned long long)c.abandoned.load(), (unsigned long long)c.reacquired.load(), (unsigned long long)c.toggles.load(), (unsigned long long)c.empty_window.load(),
               json_list(c.notes).c_str(), json_list(br).c_str(), json_list(acc).c_str());
    }
    return rc;
}

/* ---- directed scenarios -------------------------------------------------------------------------------------------------------------------- */

/* a scenario's world: one scheduler, clients on the slots it asks for, and the list of what did not hold */
struct World {
    Counters c;
    std::unique_ptr<TkLlmBatcher> b;
    std::unique_ptr<Watchdog> dog;
    std::vector<std::string> failures;
    std::vector<std::unique_ptr<Client>> clients;
    World(int slots, int n_ctx, bool cache) {
        toy::reset();
        b = std::make_unique<TkLlmBatcher>();
        std::string err;
        if (!b->init(the_model(), slots, n_ctx, toy::EOS, &err)) { fprintf(stderr, "init: %s\n", err.c_str()); exit(2); }
        b->set_prefix_cache(cache);
        dog = std::make_unique<Watchdog>(b.get(), &c, 10);
    }
    Client& client() {
        clients.push_back(std::make_unique<Client>(*b, c, b->acquire_slot()));
        return *clients.back();
    }
    void expect(bool ok, const std::string& what) { if (!ok) failures.push_back(what); }
    void expect_eq(long got, long want, const std::string& what) { if (got != want) failures.push_back(what + ": " + std::to_string(got) + ", expected " + std::to_string(want)); }
    uint64_t session_rows() { return toy::totals().rows; }
    uint64_t wasted() { uint64_t w = 0; b->stats(nullptr, nullptr, nullptr, &w); return w; }
    uint64_t rows() { uint64_t r = 0; b->stats(nullptr, &r, nullptr); return r; }
    /* the scheduler's pass count reaches n: under its lock the pass's run-ahead rows are DONE by then */
    void wait_passes(uint64_t n) {
        for (int i = 0; i < 100000; ++i) {
            uint64_t p = 0;
            b->stats(&p, nullptr, nullptr);
            if (p >= n) return;
            std::this_thread::sleep_for(std::chrono::microseconds(100));
        }
        failures.push_back("pass " + std::to_string(n) + " never completed");
    }
    void wait_held() {
        for (int i = 0; i < 100000 && !toy::held(); ++i) std::this_thread::sleep_for(std::chrono::microseconds(100));
        if (!toy::held()) failures.push_back("no pass reached the gate");
    }
    /* the rows the session ran since `before`, after everything in flight has been retired (the quiescence request's own row aside) */
    long settled_rows_since(uint64_t before) {
        drain(*b, c);
        return (long)(session_rows() - before) - 1;
    }
};

Ids seq_ids(uint64_t seed, int n) {
    Rng r(seed);
    Ids v((size_t)n);
    for (int32_t& t : v) t = r.tok();
    return v;
}
/* the pick of the last row of `toks` fed from position 0 */
int32_t pick_of(const Ids& toks) {
    toy::Row prev;
    const toy::Row* p = nullptr;
    for (int32_t t : toks) { prev.h = toy::feed(p, t); p = &prev; }
    return toy::pick(prev.h, nullptr, nullptr, nullptr);
}
/* n tokens whose greedy pick is (eos = true) or is not EOS */
Ids prompt_ending(uint64_t seed, int n, bool eos) {
    for (;; ++seed) {
        Ids v = seq_ids(seed, n);
        if ((pick_of(v) == toy::EOS) == eos) return v;
    }
}
/* a prompt after which `steps` greedy steps meet no EOS, so that a scenario's step count is what it says */
Ids prompt_running(uint64_t seed, int n, int steps) {
    for (;; ++seed) {
        Ids v = seq_ids(seed, n), all = v;
        bool ok = true;
        for (int i = 0; i <= steps && ok; ++i) {
            const int32_t p = pick_of(all);
            ok = p != toy::EOS;
            all.push_back(p);
        }
        if (ok) return v;
    }
}

using Scenario = std::function<void(World&)>;
struct Named { const char* name; int slots, n_ctx; bool cache; Scenario run; };

const uint32_t ALL_BUT_EOS[MASK_WORDS] = {0xfffffffbu, 0x001fffffu};

/* "one position ahead, never more": a plain prompt of n rows costs n + 1 rows; taking the row costs one more; an untaken row is one wasted row */
void sc_ahead_one(World& w) {
    Client& a = w.client();
    const Ids p = prompt_running(11, 10, 4);
    uint64_t r0 = w.session_rows();
    a.prompt(p, {});
    w.expect_eq(w.settled_rows_since(r0), 11, "rows for a plain prompt of 10");
    for (int i = 0; i < 3; ++i) {
        r0 = w.session_rows();
        a.step({});
        w.expect_eq(w.settled_rows_since(r0), 1, "rows for a step that finds its row done");
    }
    w.expect_eq((long)w.c.done_norec.load(), 3, "steps served from a finished row");
    w.expect_eq((long)w.wasted(), 0, "wasted rows while every row ahead was taken");
    w.b->release_slot(a.slot);
    w.expect_eq((long)w.wasted(), 1, "wasted rows after the owner left a finished row behind");
    drain(*w.b, w.c);
    w.expect_eq((long)(w.rows() + w.wasted()), (long)w.session_rows(), "rows + wasted against the session's rows");
}

/* no row ahead after a masked, stochastic, adjusted or held row, after EOS, at pos + 2 >= n_ctx; nor after a row that was handed over to such a call */
void sc_no_ahead(World& w) {
    const int n_ctx = w.b->n_ctx();
    TkSampleRow samp{};
    samp.temp = 0.7f; samp.seed = 5; samp.counter = 1;
    const int32_t bias_id = 7;
    const float bias = 2.0f;
    TkLogitAdjust biased, penal;
    biased.n_bias = 1; biased.bias_ids = &bias_id; biased.bias = &bias;
    penal.repeat = 1.3f; /* penalties on over an empty window: neutral, and still no row ahead */
    struct Case { const char* name; Client::Opt o; Ids p; long rows; };
    std::vector<Case> cases;
    Client::Opt o;
    cases.push_back({"plain", o, prompt_ending(21, 9, false), 10});
    o = {}; o.mask = ALL_BUT_EOS; cases.push_back({"masked", o, prompt_ending(22, 9, false), 9});
    o = {}; o.samp = &samp; cases.push_back({"stochastic", o, seq_ids(23, 9), 9});
    o = {}; o.adj = &biased; cases.push_back({"adjusted", o, seq_ids(24, 9), 9});
    o = {}; o.adj = &penal; cases.push_back({"penalties over an empty window", o, prompt_ending(25, 9, false), 9});
    o = {}; o.hold = true; cases.push_back({"held", o, prompt_ending(26, 9, false), 9});
    o = {}; cases.push_back({"EOS", o, prompt_ending(27, 9, true), 9});
    cases.push_back({"the last row that leaves room for one ahead", o, prompt_ending(28, n_ctx - 2, false), n_ctx - 1});
    cases.push_back({"pos + 2 == n_ctx", o, prompt_ending(29, n_ctx - 1, false), n_ctx - 1});
    for (const Case& k : cases) {
        Client& a = w.client();
        const uint64_t r0 = w.session_rows();
        a.prompt(k.p, k.o);
        w.expect_eq(w.settled_rows_since(r0), k.rows, std::string("rows for a prompt whose sampled row is ") + k.name);
        if (k.rows == n_ctx - 1 && (int)k.p.size() == n_ctx - 2) { /* the row ahead sits at the last position that may be fed: nothing runs ahead of it */
            const uint64_t r1 = w.session_rows();
            a.step({});
            w.expect_eq(w.settled_rows_since(r1), 0, "rows for the step at n_ctx - 2, served from the finished row");
        }
        w.b->release_slot(a.slot);
    }
    /* a row that ran ahead is handed to a call that may not be run ahead of: held, and penalties over an empty window */
    for (int v = 0; v < 2; ++v) {
        Client& a = w.client();
        uint64_t r0 = w.session_rows();
        a.prompt(prompt_running(31 + (uint64_t)v, 9, 3), {});
        w.expect_eq(w.settled_rows_since(r0), 10, "rows for a plain prompt of 9");
        r0 = w.session_rows();
        Client::Opt s;
        if (v == 0) s.hold = true; else s.adj = &penal;
        a.step(s);
        w.expect_eq(w.settled_rows_since(r0), 0, v == 0 ? "rows for a held step served from a finished row" : "rows for a step with penalties over an empty window served from a finished row");
        w.b->release_slot(a.slot);
    }
    /* a verify request plans no row ahead */
    Client& a = w.client();
    Client::Opt h;
    h.hold = true;
    const uint64_t r0 = w.session_rows();
    a.prompt(prompt_running(33, 9, 6), h);
    const int32_t right1 = a.greedy_after(Ids{a.pending})[0], right2 = a.greedy_after(Ids{a.pending, right1})[1];
    a.verify(Ids{right1, (int32_t)((right2 + 1) % toy::VOCAB)});
    w.expect_eq(w.settled_rows_since(r0), 9 + 3, "rows for a held prompt of 9 and a verify request of 3");
    w.expect_eq((long)w.wasted(), 1, "wasted rows: the one finished row the plain case left behind");
}

/* a changed token or n_top discards the row ahead and costs exactly one wasted row, whether it is done or in flight; so does a change of owner */
void sc_discard(World& w) {
    Client& a = w.client();
    a.prompt(prompt_running(41, 8, 12), {});
    drain(*w.b, w.c);
    long wasted = 0;
    uint64_t r0 = w.session_rows();
    a.feed(Ids{(int32_t)((a.pending + 1) % toy::VOCAB)}, {}); /* another token than the one that ran ahead */
    w.expect_eq((long)w.wasted(), ++wasted, "wasted rows after a step with another token");
    w.expect_eq(w.settled_rows_since(r0), 2, "rows for that step and the row ahead of it");
    Client::Opt lp;
    lp.n_top = 3;
    a.step(lp); /* planned with n_top -1 */
    w.expect_eq((long)w.wasted(), ++wasted, "wasted rows after a step with another n_top");
    drain(*w.b, w.c);
    a.step(lp); /* planned with 3: handed over with its record */
    w.expect_eq((long)w.wasted(), wasted, "wasted rows after a step with the n_top its row was planned with");
    w.expect_eq((long)w.c.done_rec.load(), 1, "steps served from a finished row with a record");
    drain(*w.b, w.c);
    lp.n_top = 5;
    a.step(lp);
    w.expect_eq((long)w.wasted(), ++wasted, "wasted rows after n_top 3 -> 5");
    drain(*w.b, w.c);
    /* the same with the row IN FLIGHT: the next pass, which carries only that row, waits at the gate */
    toy::close_gate((long)toy::totals().passes);
    a.step(lp); /* served from the finished row; its successor is planned */
    w.wait_held();
    r0 = w.session_rows();
    {
        std::thread opener([] { std::this_thread::sleep_for(std::chrono::milliseconds(40)); toy::open_gate(); });
        a.feed(Ids{(int32_t)((a.pending + 2) % toy::VOCAB)}, lp);
        opener.join();
    }
    w.expect_eq((long)w.wasted(), ++wasted, "wasted rows after a step with another token while the row was in flight");
    w.expect_eq(w.settled_rows_since(r0), 3, "rows: the discarded row, that step, the row planned ahead of it");
    /* a change of owner while the row is in flight: release and acquire do not block, so this is the in-flight path for certain */
    toy::close_gate((long)toy::totals().passes);
    a.step(lp);
    w.wait_held();
    r0 = w.session_rows();
    w.b->release_slot(a.slot);
    Client& n = w.client();
    w.expect_eq(n.slot, a.slot, "the slot the next owner gets");
    toy::open_gate();
    n.prompt(prompt_running(43, 6, 3), {});
    w.expect_eq(w.settled_rows_since(r0), 1 + 6 + 1, "rows: the discarded row, the new owner's prompt of 6, the row ahead of it");
    w.expect_eq((long)w.wasted(), ++wasted, "wasted rows after the slot changed owner under a row in flight");
    n.step({});
    w.expect_eq((long)w.wasted(), wasted, "wasted rows after the new owner's first step");
}

/* keep: at most n - 1 rows; the record follows what the cache holds; it survives release / acquire; a prefix at pos0 != 0 is no prompt */
void sc_keep(World& w) {
    Client& a = w.client();
    const Ids p = prompt_running(51, 20, 3);
    TkLlmBatcher::PrefixRows pr;
    Client::Opt h;
    h.hold = true;
    a.prompt(p, h, &pr);
    w.expect_eq(pr.kept, 0, "kept by the first prompt");
    uint64_t r0 = w.session_rows();
    a.prompt(p, h, &pr);
    w.expect_eq(pr.kept, 19, "kept by the same prompt again (n - 1: the last token is computed)");
    w.expect_eq(w.settled_rows_since(r0), 1, "rows for it");
    Ids q = p;
    q[5] = (q[5] + 1) % toy::VOCAB;
    a.prompt(q, h, &pr);
    w.expect_eq(pr.kept, 5, "kept by a prompt that differs at position 5");
    a.prompt(p, h, &pr);
    w.expect_eq(pr.kept, 5, "kept by the first prompt after that one overwrote rows 5 ..");
    Ids longer = p;
    for (int i = 0; i < 6; ++i) longer.push_back((int32_t)(3 + i));
    a.prompt(longer, h, &pr);
    w.expect_eq(pr.kept, 20, "kept by a longer prompt");
    w.b->release_slot(a.slot);
    Client& n = w.client();
    w.expect_eq(n.slot, a.slot, "the slot the next owner gets");
    n.prompt(longer, h, &pr);
    w.expect_eq(pr.kept, 25, "kept by the next owner of the slot");
    /* a row that ran ahead is in the record, for the token it was fed */
    n.prompt(p, {}, &pr);
    drain(*w.b, w.c);
    Ids cont = p;
    cont.push_back(n.pending);
    cont.push_back(9);
    n.prompt(cont, h, &pr);
    w.expect_eq(pr.kept, 21, "kept by a prompt that continues with the id that ran ahead");
    /* prefix given with pos0 != 0: fed as asked, nothing kept, not counted as a prompt */
    uint64_t before = 0, after = 0;
    w.b->prefix_stats(&before, nullptr, nullptr, nullptr);
    n.n_past = 22;
    n.feed_at(5, Ids{1, 2 + 1, 4}, h, &pr, "prefix at pos0 5");
    w.b->prefix_stats(&after, nullptr, nullptr, nullptr);
    w.expect(pr.prompt_rows == 3 && pr.kept == 0 && pr.copied == 0 && before == after, "a prefix at pos0 != 0 reports {n, 0, 0} and is not counted");
    w.expect_eq((long)toy::totals().copy_launches, 0, "copy launches with one slot in use");
}

/* copy: from the lowest slot with the longest match, TK_PREFIX_COPY_MIN rows or more, never the last row */
void sc_copy(World& w) {
    Client &a = w.client(), &b = w.client(), &c = w.client();
    const Ids p = prompt_running(61, 30, 2);
    TkLlmBatcher::PrefixRows pr;
    Client::Opt h;
    h.hold = true;
    a.prompt(p, h);
    b.prompt(p, h, &pr);
    w.expect(pr.kept == 0 && pr.copied == 29, "the same prompt on another slot copies n - 1 rows");
    Ids q(p.begin(), p.begin() + 10);
    for (int i = 0; i < 12; ++i) q.push_back((int32_t)(40 - i));
    c.prompt(q, h, &pr);
    w.expect(pr.kept == 0 && pr.copied == 0, "a match of 10 rows is not copied");
    Ids q2(p.begin(), p.begin() + 25);
    for (int i = 0; i < 5; ++i) q2.push_back((int32_t)(40 - i));
    c.prompt(q2, h, &pr);
    w.expect(pr.kept == 10 && pr.copied == 0, "15 rows beyond the 10 it kept are fewer than a copy takes");
    Ids q3(p.begin(), p.begin() + 28);
    for (int i = 0; i < 3; ++i) q3.push_back((int32_t)(30 - i));
    c.prompt(q3, h, &pr);
    w.expect(pr.kept == 25 && pr.copied == 0, "kept its own 25 rows; 3 more are not copied");
    c.prompt(q, h, &pr);
    w.expect(pr.kept == 10 && pr.copied == 0, "back to the prompt that shares 10 rows");
    c.prompt(q3, h, &pr);
    w.expect(pr.kept == 10 && pr.copied == 18, "kept 10 of its own rows, then copied the 18 another slot offers beyond them");
    const toy::Totals t = toy::totals();
    w.expect_eq((long)t.copy_launches, 2, "copy launches");
    w.expect_eq((long)t.copy_rows, 47, "copied rows");
}

/* after a shift nothing beyond n_keep is kept or copied, and a later row does not extend the record */
void sc_shift(World& w) {
    Client &a = w.client(), &b = w.client(), &c = w.client(), &d = w.client();
    const Ids p = prompt_running(71, 40, 4), q = prompt_running(72, 40, 4);
    TkLlmBatcher::PrefixRows pr;
    Client::Opt h;
    h.hold = true;
    a.prompt(p, {}); /* with a row ahead of it that the shift retires */
    drain(*w.b, w.c);
    a.shift(8, 8);
    w.expect_eq((long)w.wasted(), 1, "wasted rows: the finished row the shift retired");
    a.step(h);
    a.step(h);
    b.prompt(p, h, &pr);
    w.expect(pr.kept == 0 && pr.copied == 0, "8 valid rows are fewer than a copy takes: nothing of a shifted slot is copied");
    a.prompt(p, h, &pr);
    w.expect_eq(pr.kept, 8, "kept by the same prompt on the shifted slot (n_keep)");
    c.prompt(q, h);
    c.shift(20, 5);
    c.step(h);
    d.prompt(q, h, &pr);
    w.expect(pr.kept == 0 && pr.copied == 20, "copied from a slot shifted with n_keep 20: exactly the rows that stayed");
    c.prompt(q, h, &pr);
    w.expect_eq(pr.kept, 20, "kept by the same prompt on that slot");
}

/* after a verify request the record ends at pos0 + m + 1: a longer prompt made of everything that was FED keeps exactly that many rows */
void sc_verify_record(World& w) {
    Client::Opt h;
    h.hold = true;
    for (int k_right : {0, 2, 6}) {
        Client& a = w.client();
        const Ids p = prompt_running(81 + (uint64_t)k_right, 10, 8); /* its continuation meets no EOS, so that exactly k_right drafts are accepted */
        int m = -1;
        a.prompt(p, h);
        Ids drafts, toks{a.pending};
        for (int i = 0; i < 6; ++i) {
            const int32_t right = a.greedy_after(toks).back();
            drafts.push_back(i < k_right ? right : (int32_t)((right + 1) % toy::VOCAB));
            toks.push_back(drafts.back());
        }
        const uint64_t r0 = w.session_rows();
        a.verify(drafts, &m);
        w.expect_eq(m, k_right, "drafts accepted");
        w.expect_eq(w.settled_rows_since(r0), 7, "rows of the verify request");
        Ids longer = p;
        longer.insert(longer.end(), toks.begin(), toks.end());
        longer.push_back(4);
        TkLlmBatcher::PrefixRows pr;
        a.prompt(longer, h, &pr);
        w.expect_eq(pr.kept, 10 + k_right + 1, "kept by a prompt that repeats every fed id: the record ends behind the last accepted row");
    }
    w.expect_eq((long)w.rows() + (long)w.wasted(), (long)w.session_rows(), "rows + wasted against the session's rows: every row of a verify request counts");
}

/* a verify request of n rows that does not fit what is left of a pass waits for the next one (TK_MI355X_BATCHER_DECODE_FIRST=1: one-row requests
 * are taken first whatever their place in the queue, so the arrangement does not depend on who queued first) */
void sc_verify_waits(World& w) {
    Client::Opt h;
    h.hold = true;
    Client& v = w.client();
    v.prompt(prompt_running(91, 5, 16), h);
    const int n_one = 245;
    std::vector<Client*> ones;
    for (int i = 0; i < n_one + 1; ++i) ones.push_back(&w.client());
    const long gate = (long)toy::totals().passes;
    toy::close_gate(gate);
    std::thread blocker([&] { ones[(size_t)n_one]->prompt(Ids{5}, h); });
    w.wait_held();
    std::vector<std::thread> ts;
    std::atomic<int> started{0};
    for (int i = 0; i < n_one; ++i) ts.emplace_back([&, i] { started++; ones[(size_t)i]->feed_at(0, Ids{(int32_t)(i % toy::VOCAB)}, h, nullptr, "one row"); });
    Ids drafts, toks{v.pending};
    for (int i = 0; i < 15; ++i) { drafts.push_back(v.greedy_after(toks).back()); toks.push_back(drafts.back()); }
    int m = -1;
    ts.emplace_back([&] { started++; v.verify(drafts, &m); });
    while (started < n_one + 1) std::this_thread::yield();
    std::this_thread::sleep_for(std::chrono::milliseconds(300)); /* every caller is inside its call; the outcome below says whether all were queued */
    toy::open_gate();
    blocker.join();
    for (std::thread& t : ts) t.join();
    const auto wide = toy::rows_of_pass(gate + 1), next = toy::rows_of_pass(gate + 2);
    w.expect_eq((long)wide.size(), n_one, "rows of the pass the verify request did not fit (245 one-row requests; 16 rows do not fit the 11 left)");
    for (auto& r : wide) w.expect(r.first != v.slot, "a row of the verify request in the pass it did not fit");
    w.expect_eq((long)next.size(), 16, "rows of the next pass");
    for (size_t i = 0; i < next.size(); ++i) w.expect(next[i].first == v.slot && next[i].second == 5 + (int)i, "the next pass is the verify request's run");
    w.expect_eq(m, 15, "drafts accepted");
    w.expect_eq((long)toy::totals().verify_passes, 1, "verify passes");
}

/* the most copies one launch can hold: every slot but the donor's and one more asks for the donor's rows in one pass */
void sc_many_copies(World& w) {
    Client::Opt h;
    h.hold = true;
    const Ids p = prompt_running(101, 20, 2);
    Client& donor = w.client();
    donor.prompt(p, h);
    const int n_req = 254;
    std::vector<Client*> rs;
    for (int i = 0; i < n_req + 1; ++i) rs.push_back(&w.client());
    toy::close_gate((long)toy::totals().passes);
    std::thread blocker([&] { rs[(size_t)n_req]->feed_at(0, Ids{5}, h, nullptr, "one row"); });
    w.wait_held();
    std::vector<std::thread> ts;
    std::vector<TkLlmBatcher::PrefixRows> pr((size_t)n_req);
    std::atomic<int> started{0};
    for (int i = 0; i < n_req; ++i) ts.emplace_back([&, i] { started++; rs[(size_t)i]->prompt(p, h, &pr[(size_t)i]); });
    while (started < n_req) std::this_thread::yield();
    std::this_thread::sleep_for(std::chrono::milliseconds(300));
    toy::open_gate();
    blocker.join();
    for (std::thread& t : ts) t.join();
    for (int i = 0; i < n_req; ++i) w.expect(pr[(size_t)i].copied == 19 && pr[(size_t)i].kept == 0, "every request copied n - 1 rows");
    const toy::Totals t = toy::totals();
    w.expect_eq(t.widest_copy, n_req, "descriptors of the widest copy launch");
    w.expect_eq((long)t.copy_launches, 1, "copy launches");
    w.expect_eq((long)t.copy_rows, 19 * n_req, "copied rows");
    w.b->release_slot(rs[(size_t)n_req]->slot);
}

/* the source / destination rule: a slot that serves as a source computes this pass; a slot that is a destination is no donor */
void sc_src_dst(World& w) {
    Client::Opt h;
    h.hold = true;
    for (int order = 0; order < 2; ++order) {
        Client &a = w.client(), &b = w.client(), &c = w.client(), &x = w.client();
        const Ids p = prompt_running(111 + (uint64_t)order, 24, 2), q = prompt_running(121 + (uint64_t)order, 24, 2);
        a.prompt(p, h);
        c.prompt(q, h);
        /* in one pass: B asks for P (A's rows) and A asks for Q (C's rows) */
        toy::close_gate((long)toy::totals().passes);
        std::thread blocker([&] { x.feed_at(0, Ids{5}, h, nullptr, "one row"); });
        w.wait_held();
        TkLlmBatcher::PrefixRows pa, pb;
        std::thread t1([&] { if (order == 0) b.prompt(p, h, &pb); else a.prompt(q, h, &pa); });
        std::this_thread::sleep_for(std::chrono::milliseconds(100));
        std::thread t2([&] { if (order == 0) a.prompt(q, h, &pa); else b.prompt(p, h, &pb); });
        std::this_thread::sleep_for(std::chrono::milliseconds(100));
        toy::open_gate();
        blocker.join(); t1.join(); t2.join();
        if (order == 0) w.expect(pb.copied == 23 && pa.copied == 0, "B copied A's rows; A, a source of that launch, computed");
        else w.expect(pa.copied == 23 && pb.copied == 0, "A copied C's rows; B, whose donor was a destination of that launch, computed");
    }
}

/* every argument the three calls refuse; none of them reaches the session */
void sc_refusals(World& w) {
    TkLlmBatcher& b = *w.b;
    const int n_ctx = b.n_ctx(), slots = b.slots();
    int32_t tok[20] = {1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21}, got = -1, ids[20];
    int n_out = 0;
    TkTokenLogprob rec;
    TkLogitAdjust bad;
    bad.repeat = 0.0f;
    auto refused = [&](bool ok, const std::string& err, const char* what) { w.expect(!ok && !err.empty(), std::string("refused: ") + what); };
    std::string e;
    refused(b.submit(0, 0, tok, 0, nullptr, &got, &e), e, "submit of no rows"); e.clear();
    refused(b.submit(0, 0, tok, 1, nullptr, &got, &e, nullptr, nullptr, nullptr, false, 21, &rec), e, "n_top 21"); e.clear();
    refused(b.submit(0, 0, tok, 1, nullptr, &got, &e, nullptr, nullptr, nullptr, false, -2, &rec), e, "n_top -2"); e.clear();
    refused(b.submit(0, 0, tok, 1, nullptr, &got, &e, nullptr, nullptr, nullptr, false, 2, nullptr), e, "n_top without a record"); e.clear();
    refused(b.submit(0, 0, tok, 1, nullptr, &got, &e, nullptr, nullptr, &bad), e, "repeat 0"); e.clear();
    refused(b.submit(-1, 0, tok, 1, nullptr, &got, &e), e, "slot -1"); e.clear();
    refused(b.submit(slots, 0, tok, 1, nullptr, &got, &e), e, "slot == slots"); e.clear();
    refused(b.submit(0, -1, tok, 1, nullptr, &got, &e), e, "pos0 -1"); e.clear();
    refused(b.submit(0, n_ctx - 2, tok, 3, nullptr, &got, &e), e, "rows past the window"); e.clear();
    refused(b.submit_verify(0, 0, tok, 0, ids, &n_out, &e), e, "verify of no rows"); e.clear();
    refused(b.submit_verify(0, 0, tok, TK_LOOKUP_MAX_DRAFT + 2, ids, &n_out, &e), e, "verify of 17 rows"); e.clear();
    refused(b.submit_verify(0, 0, nullptr, 2, ids, &n_out, &e), e, "verify without tokens"); e.clear();
    refused(b.submit_verify(0, 0, tok, 2, nullptr, &n_out, &e), e, "verify without room for ids"); e.clear();
    refused(b.submit_verify(0, 0, tok, 2, ids, nullptr, &e), e, "verify without n_out"); e.clear();
    refused(b.submit_verify(slots, 0, tok, 2, ids, &n_out, &e), e, "verify on slot == slots"); e.clear();
    refused(b.submit_verify(0, n_ctx - 1, tok, 2, ids, &n_out, &e), e, "verify past the window"); e.clear();
    refused(b.shift(-1, 2, 2, 10, &e), e, "shift of slot -1"); e.clear();
    refused(b.shift(0, -1, 2, 10, &e), e, "shift with n_keep -1"); e.clear();
    refused(b.shift(0, 2, 0, 10, &e), e, "shift with n_discard 0"); e.clear();
    refused(b.shift(0, 4, 6, 10, &e), e, "shift that leaves nothing to move"); e.clear();
    refused(b.shift(0, 2, 2, n_ctx + 1, &e), e, "shift with n_past > n_ctx"); e.clear();
    const toy::Totals t = toy::totals();
    w.expect(t.passes == 0 && t.rows == 0 && t.shifts == 0 && t.copy_launches == 0, "a refused call reaches the session");
    /* the widest calls that are taken */
    Client& a = w.client();
    Ids full = prompt_running(131, n_ctx, 0);
    a.prompt(full, {});
    a.shift(0, 1);
    w.expect_eq(a.n_past, n_ctx - 1, "n_past after a shift of a full window");
}

/* a failed pass: every request and waiter of it fails with the session's error of THAT pass, a finished run-ahead row of it fails its owner when
 * taken, the records of the slots it touched are gone (its copies' destinations too), later passes are right again */
void sc_failed_pass(World& w) {
    Client::Opt h;
    h.hold = true;
    Client &a = w.client(), &b = w.client(), &c = w.client();
    const Ids p = prompt_running(141, 20, 6), q = prompt_running(142, 20, 6);
    TkLlmBatcher::PrefixRows pr;
    a.prompt(p, {});      /* pass 0; its row ahead is pass 1 */
    w.wait_passes(2);
    b.prompt(q, h);       /* pass 2 */
    Ids px = p;
    px.push_back(3);
    toy::fail_pass(3);    /* C's prompt copies 20 rows from A and computes one: the pass fails */
    w.expect(!c.prompt(px, h, &pr) && c.err == toy::fail_text(3), "a request of the failed pass fails with the session's error");
    w.expect_eq(pr.copied, 20, "rows the failed request had copied");
    c.prompt(px, h, &pr); /* pass 4 */
    w.expect_eq(pr.kept, 0, "kept on the destination of a copy whose pass failed");
    w.expect_eq(pr.copied, 20, "copied again from the untouched source");
    /* a finished run-ahead row of a failed pass, and a later failure of another slot before its owner takes it */
    toy::fail_pass(5);
    a.step({});           /* served from pass 1's row; the row ahead of it is pass 5 and fails */
    w.wait_passes(6);
    toy::fail_pass(6);
    w.expect(!b.step(h) && b.err == toy::fail_text(6), "a one-row request of a failed pass fails with that pass's error");
    w.expect(!a.step({}) && a.err == toy::fail_text(5), "a finished run-ahead row of a failed pass fails its owner with THAT pass's error");
    a.prompt(p, {}, &pr); /* pass 7, ahead 8 */
    w.expect_eq(pr.kept, 0, "kept on a slot whose run-ahead row failed");
    w.wait_passes(9);
    b.prompt(q, h, &pr);  /* pass 9 */
    w.expect_eq(pr.kept, 0, "kept on a slot whose request failed");
    /* a waiter of a failed pass: the row ahead of A's next step waits at the gate, A asks for it, the pass fails */
    toy::close_gate(10);
    toy::fail_pass(10);
    a.step({});           /* served from pass 8's row; pass 10 carries its successor */
    w.wait_held();
    {
        std::thread opener([] { std::this_thread::sleep_for(std::chrono::milliseconds(40)); toy::open_gate(); });
        w.expect(!a.step({}) && a.err == toy::fail_text(10), "a caller waiting for a run-ahead row of a failed pass fails with the session's error");
        opener.join();
    }
    a.prompt(p, {}, &pr);
    w.expect_eq(pr.kept, 0, "kept on a slot whose awaited row failed");
    for (int i = 0; i < 4; ++i) a.step({});
    b.step(h);
    w.expect_eq((long)w.c.failed.load(), 4, "failed calls");
    w.expect_eq((long)toy::totals().failed_passes, 4, "failed passes");
}

/* a slot's context shifts while another slot's prompt, queued in front of the shift, wants its rows: shifts are served first and cut the record
 * before anything is matched, so the copy takes exactly the rows that stay valid — whichever of the two calls arrived first */
void sc_shift_under_copy(World& w) {
    Client::Opt h;
    h.hold = true;
    for (int order = 0; order < 2; ++order) {
        Client &a = w.client(), &b = w.client(), &x = w.client();
        const Ids p = prompt_running(151 + (uint64_t)order, 40, 2);
        a.prompt(p, h);
        toy::close_gate((long)toy::totals().passes);
        std::thread blocker([&] { x.feed_at(0, Ids{5}, h, nullptr, "one row"); });
        w.wait_held();
        TkLlmBatcher::PrefixRows pr;
        std::thread t1([&] { if (order == 0) b.prompt(p, h, &pr); else a.shift(20, 10); });
        std::this_thread::sleep_for(std::chrono::milliseconds(100));
        std::thread t2([&] { if (order == 0) a.shift(20, 10); else b.prompt(p, h, &pr); });
        std::this_thread::sleep_for(std::chrono::milliseconds(100));
        toy::open_gate();
        blocker.join(); t1.join(); t2.join();
        w.expect(pr.kept == 0 && pr.copied == 20, "the prompt copied exactly the n_keep rows of the slot that shifted");
        a.step(h);
        b.step(h);
    }
    w.expect_eq((long)toy::totals().shifts, 2, "shifts");
}

/* one pass that holds a verify request, a masked one-row step and a prompt chunk goes through forward() and gives every one of them what it would
 * get alone; the same pass failing fails all three with the session's error, clears their records, and the next passes are right again */
void sc_mixed_pass(World& w) {
    Client::Opt h, masked;
    h.hold = true;
    masked.mask = ALL_BUT_EOS;
    Client &v = w.client(), &m = w.client(), &p = w.client(), &x = w.client();
    const Ids pv = prompt_running(161, 12, 8), pm = prompt_running(162, 9, 4), pp = prompt_running(163, 30, 2);
    for (int failing = 0; failing < 2; ++failing) {
        TkLlmBatcher::PrefixRows pr;
        v.prompt(pv, h, &pr);
        if (failing) w.expect_eq(pr.kept, 11, "kept by the verify slot's prompt before the failure");
        m.prompt(pm, masked);
        const long gate = (long)toy::totals().passes;
        toy::close_gate(gate);
        if (failing) toy::fail_pass(gate + 1);
        std::thread blocker([&] { x.feed_at(0, Ids{5}, h, nullptr, "one row"); });
        w.wait_held();
        Ids drafts, toks{v.pending};
        for (int i = 0; i < 5; ++i) {
            const int32_t right = v.greedy_after(toks).back();
            drafts.push_back(i < 3 ? right : (int32_t)((right + 1) % toy::VOCAB));
            toks.push_back(drafts.back());
        }
        int acc = -1;
        bool ok_v = false, ok_m = false, ok_p = false;
        std::thread tv([&] { ok_v = v.verify(drafts, &acc); });
        std::thread tm([&] { ok_m = m.step(masked); });
        std::thread tp([&] { ok_p = p.prompt(pp, h); });
        std::this_thread::sleep_for(std::chrono::milliseconds(150));
        toy::open_gate();
        blocker.join(); tv.join(); tm.join(); tp.join();
        /* the second round's prompt keeps the 29 rows the first round left in its slot */
        w.expect_eq((long)toy::rows_of_pass(gate + 1).size(), 6 + 1 + (failing ? 1 : 30), "rows of the pass: the verify request's 6, the masked step, the prompt's rows");
        w.expect_eq((long)toy::totals().verify_passes, 0, "verify passes (a pass with a masked row takes forward())");
        if (!failing) {
            w.expect(ok_v && ok_m && ok_p, "the three requests of the pass succeed");
            w.expect_eq(acc, 3, "drafts accepted");
        } else {
            const std::string want = toy::fail_text(gate + 1);
            w.expect(!ok_v && !ok_m && !ok_p && v.err == want && m.err == want && p.err == want, "the three requests of the failed pass fail with the session's error");
            for (Client* k : {&v, &m, &p}) {
                k->prompt(k == &v ? pv : k == &m ? pm : pp, h, &pr);
                w.expect_eq(pr.kept, 0, "kept on a slot the failed pass touched");
                k->step(h);
            }
            w.expect_eq((long)w.c.failed.load(), 3, "failed calls");
        }
    }
}

const Named SCENARIOS[] = {
    {"ahead_one", 4, 64, false, sc_ahead_one},
    {"no_ahead", 24, 64, false, sc_no_ahead},
    {"discard", 4, 64, false, sc_discard},
    {"keep", 4, 64, true, sc_keep},
    {"copy", 4, 64, true, sc_copy},
    {"shift", 6, 64, true, sc_shift},
    {"verify_record", 6, 64, true, sc_verify_record},
    {"verify_waits", 256, 32, false, sc_verify_waits},
    {"many_copies", 256, 32, true, sc_many_copies},
    {"src_dst", 10, 64, true, sc_src_dst},
    {"shift_under_copy", 8, 64, true, sc_shift_under_copy},
    {"mixed_pass", 6, 64, true, sc_mixed_pass},
    {"refusals", 4, 64, true, sc_refusals},
    {"failed_pass", 4, 64, true, sc_failed_pass},
};

int scenario(const char* name) {
    for (const Named& s : SCENARIOS) {
        if (strcmp(s.name, name) != 0) continue;
        if (strcmp(name, "verify_waits") == 0) setenv("TK_MI355X_BATCHER_DECODE_FIRST", "1", 1);
        std::vector<std::string> failures, notes, br;
        uint64_t mismatches = 0;
        {
            World w(s.slots, s.n_ctx, s.cache);
            s.run(w);
            drain(*w.b, w.c);
            w.dog.reset();
            failures = w.failures;
            notes = w.c.notes;
            mismatches = w.c.mismatches;
            if (strcmp(name, "failed_pass") != 0 && strcmp(name, "mixed_pass") != 0 && w.c.failed) failures.push_back("a call failed");
        }
        br = toy::breaches();
        const toy::Totals t = toy::totals();
        printf("{\"mode\": \"scenario\", \"name\": \"%s\", \"mismatches\": %llu, \"breaches\": %zu, \"failures\": %s, \"notes\": %s, \"breach_list\": %s, \"passes\": %llu, \"session_rows\": %llu}\n", name,
               (unsigned long long)mismatches, br.size(), json_list(failures).c_str(), json_list(notes).c_str(), json_list(br).c_str(), (unsigned long long)t.passes, (unsigned long long)t.rows);
        return 0;
    }
    fprintf(stderr, "no scenario '%s'; the scenarios:", name);
    for (const Named& s : SCENARIOS) fprintf(stderr, " %s", s.name);
    fprintf(stderr, "\n");
    return 2;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 5 && strcmp(argv[1], "soak") == 0) return soak(atoi(argv[2]), strtoull(argv[3], nullptr, 10), atoi(argv[4]), argc >= 6 ? atol(argv[5]) : -1);
    if (argc == 3 && strcmp(argv[1], "scenario") == 0) return scenario(argv[2]);
    if (argc == 2 && strcmp(argv[1], "list") == 0) {
        for (const Named& s : SCENARIOS) printf("%s\n", s.name);
        return 0;
    }
    fprintf(stderr, "usage: batcher_soak soak RUNNERS SEED OPS [FAIL_PASS] | scenario NAME | list\n");
    return 2;
}
