/*
 * tk_prefix_match.h — the matching rules of the prompt prefix cache (tk_llm_batcher.h), host only: no device, no state.
 *
 * A record is the list of token ids whose K/V rows a sequence slot holds at positions 0, 1, ...  A cache row at position p depends only on
 * tokens 0 .. p, so wherever a prompt's tokens equal a record from position 0 on, the slot's rows ARE the rows the prompt would compute.
 */
#ifndef TK_PREFIX_MATCH_H
#define TK_PREFIX_MATCH_H

#include <stdint.h>

/* rows another slot must offer beyond the cursor before they are copied: a policy constant (a shorter copy is not worth a launch), not a measurement */
#define TK_PREFIX_COPY_MIN 16

/* length of the longest common prefix of toks[0 .. n) and rec[0 .. rec_n), at most n - 1: the last prompt token is always computed, its
 * logits are what gets sampled */
static inline int tk_prefix_common(const int32_t* toks, int n, const int32_t* rec, int rec_n) {
    int cap = n - 1 < rec_n ? n - 1 : rec_n;
    int i = 0;
    while (i < cap && toks[i] == rec[i]) ++i;
    return i;
}

/* The slot to copy rows [cursor, *match) from, or -1.  recs[s] / rec_n[s]: the record of slot s; self: the prompt's own slot (never a donor);
 * skip (optional): skip[s] != 0 bars slot s.  A donor's record equals the prompt from position 0 up to *match (the same n - 1 cap) and
 * *match - cursor >= TK_PREFIX_COPY_MIN; the longest match wins, among equal ones the lowest slot, so that runs are reproducible. */
static inline int tk_prefix_best_donor(const int32_t* toks, int n, const int32_t* const* recs, const int* rec_n, int n_slots, int self, int cursor,
                                       const char* skip, int* match) {
    int best = -1, best_m = cursor + TK_PREFIX_COPY_MIN - 1;
    for (int s = 0; s < n_slots; ++s) {
        if (s == self || (skip && skip[s])) continue;
        /* cheap refusals first: the record must reach beyond the best match so far and agree with the prompt there */
        if (rec_n[s] <= best_m || best_m >= n - 1 || recs[s][best_m] != toks[best_m]) continue;
        const int m = tk_prefix_common(toks, n, recs[s], rec_n[s]);
        if (m > best_m) { best = s; best_m = m; }
    }
    if (best >= 0) *match = best_m;
    return best;
}

#endif
