/*
 * llm_session_toy.h — a stand-in for TkLlmSession that the real scheduler (csrc/llm/tk_llm_batcher.cpp) links against on the CPU.
 *
 * It models what the KV cache MEANS, not arithmetic.  Per (slot, position) the cache holds a row {tok, h, valid}; feeding (slot, pos, tok) writes
 *     h = mix(pos ? row[pos - 1].h : SEED, tok)
 * so a row's value is a chain hash of everything it attended to, as that was computed at the time.  Position enters only through order: a shifted row
 * stands "as at its new position, computed in its old context", which is what the key re-rotation of the real shift does.  Every cache mistake of the
 * scheduler therefore shows in a sampled id: a stale row left in place, a row kept after a shift, a copy from the wrong slot or range, a source
 * overwritten before it was read, rows fed out of order.  What it cannot see: arithmetic, graph replay and stream ordering inside the real session.
 *
 * The functions of namespace toy are pure, so a runner thread of tests/stubs/batcher_soak.cpp keeps a private mirror of its own sequence with them and
 * compares every id and record the scheduler returns, exactly.
 */
#ifndef LLM_SESSION_TOY_H
#define LLM_SESSION_TOY_H

#include <stdint.h>

#include <string>
#include <vector>

#include "tk_llm_engine.h"

namespace toy {

constexpr int VOCAB = 53;
constexpr int32_t EOS = 2;
constexpr uint64_t SEED = 0x9e3779b97f4a7c15ull;

struct Row {
    int32_t tok = -1;
    uint64_t h = 0;
    bool valid = false;
};

inline uint64_t mix(uint64_t h, uint64_t v) {
    uint64_t z = h ^ (v + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2));
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
/* the row that feeding `tok` behind `prev` (nullptr at position 0) writes */
inline uint64_t feed(const Row* prev, int32_t tok) { return mix(prev ? prev->h : SEED, (uint64_t)(uint32_t)tok); }

/* every field and array of a descriptor: one attached to the wrong row, or read after its owner freed it, shows in the pick */
uint64_t adjust_digest(const TkLogitAdjust& a);
/* the id a row with hash h samples.  mask: (VOCAB + 31) / 32 words or nullptr; samp: used when temp > 0; adj: used when not neutral */
int32_t pick(uint64_t h, const uint32_t* mask, const TkSampleRow* samp, const TkLogitAdjust* adj);
/* the record of a row with hash h that asks for n_top >= 0 alternatives */
void fill_record(uint64_t h, int32_t n_top, TkTokenLogprob* rec);
bool same_record(const TkTokenLogprob& a, const TkTokenLogprob& b);

/* what the session saw since reset() */
struct Totals {
    uint64_t passes = 0, verify_passes = 0, failed_passes = 0; /* forward + forward_verify calls; of them forward_verify; of them refused by fail_pass */
    uint64_t rows = 0;                                         /* rows of every pass, the failed ones included */
    int widest = 0;
    uint64_t copy_launches = 0, copy_descs = 0, copy_rows = 0;
    int widest_copy = 0; /* descriptors of the largest copy launch */
    uint64_t shifts = 0;
};
Totals totals();
std::vector<std::string> breaches(); /* one line per broken rule, with the pass number */
void reset();
/* pass number k (0-based over forward and forward_verify calls since reset) returns false with fail_text(k); may be called for several passes */
void fail_pass(long k);
std::string fail_text(long k);
/* the pass that last ran a row at (slot, pos) since reset, -1 when none */
long last_pass_of(int slot, int pos);
/* the rows of pass k as (slot, pos) pairs, for scenarios that assert how a pass was formed; empty when it has not run */
std::vector<std::pair<int, int>> rows_of_pass(long k);
/* gate: pass number k blocks on entry until open_gate(); held() is true while a pass waits there.  -1 = no gate */
void close_gate(long k);
void open_gate();
bool held();

}  // namespace toy

#endif
