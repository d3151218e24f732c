/*
 * tk_lookup_scope.h — lookup decoding (tk_lookup.h) for a runner that samples, is masked, adjusted or asks for log-probabilities: which runner drafts,
 * and the tables of the rows of its verify pass.  Host only: no device, no state.
 *
 * A verify request feeds t = [pending, d0 .. d(n-2)] at positions p .. p + n - 1.  Row i is given exactly the tables a one-row pass at position p + i
 * would have had IF drafts d0 .. d(i-1) are the ids the runner would have sampled there:
 *   sampling    the runner's chain with counter c + i (the generator is keyed by (seed, number of tokens sampled): tk_lookup_row_counter); after the
 *               accept rule has kept m + 1 ids the runner's counter is c + m + 1;
 *   grammar     the mask of the runner's grammar state after it has accepted pending, d0 .. d(i-1), on COPIES of the state (tk_lookup_grammar_cut);
 *               the drafts are cut in front of the first one the state refuses, and in front of the first one that would complete the grammar — a
 *               runner without lookup pauses there and never feeds that id;
 *   adjustment  the runner's bias list, and the runner's window after pending, d0 .. d(i-1), cut to last_n (tk_lookup_row_window; the pending id is
 *               in the window already when the request is made);
 *   records     every row asks with the runner's n_top; record i travels with id i.
 * The accept rule (tk_lookup_accept) is unchanged: row i's pick is used only when drafts 0 .. i - 1 were confirmed, and then each of its tables equals
 * the one the runner would have built with lookup off.  A row's bits depend neither on its pass nor on its neighbours, so the ids are the same ids.
 */
#ifndef TK_LOOKUP_SCOPE_H
#define TK_LOOKUP_SCOPE_H

#include <stdint.h>

#include <vector>

/* tk_mi355x_llm_runner_set_lookup_scope: the conditions under which a runner with lookup on still drafts */
#define TK_LOOKUP_SCOPE_SAMPLED 1u  /* a temperature */
#define TK_LOOKUP_SCOPE_GRAMMAR 2u  /* a grammar mask */
#define TK_LOOKUP_SCOPE_ADJUSTED 4u /* penalties or a logit bias */
#define TK_LOOKUP_SCOPE_LOGPROBS 8u /* log-probabilities */
#define TK_LOOKUP_SCOPE_ALL 15u

/* a runner drafts iff the bit of every condition that holds is set; scope 0 is a greedy, unmasked, unadjusted runner without records only */
static inline bool tk_lookup_scope_allows(uint32_t scope, bool sampled, bool grammar, bool adjusted, bool logprobs) {
    const uint32_t need = (sampled ? TK_LOOKUP_SCOPE_SAMPLED : 0u) | (grammar ? TK_LOOKUP_SCOPE_GRAMMAR : 0u) | (adjusted ? TK_LOOKUP_SCOPE_ADJUSTED : 0u) |
                          (logprobs ? TK_LOOKUP_SCOPE_LOGPROBS : 0u);
    return (need & ~scope) == 0;
}

/* the sampling counter of row i of a verify pass of a runner whose counter is c */
static inline uint32_t tk_lookup_row_counter(uint32_t c, int i) { return c + (uint32_t)i; }

/* the penalty window of row i: the last min(last_n, n_acc + i) ids of accepted[0 .. n_acc) ++ drafts[0 .. i), oldest first, into out (room for
 * last_n).  accepted is the runner's window, the pending id last.  Returns the count, -1 on bad arguments */
static inline int tk_lookup_row_window(const int32_t* accepted, int n_acc, const int32_t* drafts, int i, int last_n, int32_t* out) {
    if (n_acc < 0 || i < 0 || last_n < 0 || (n_acc > 0 && !accepted) || (i > 0 && !drafts) || (last_n > 0 && !out)) return -1;
    const int total = n_acc + i, n = total < last_n ? total : last_n;
    for (int k = 0; k < n; ++k) {
        const int j = total - n + k;
        out[k] = j < n_acc ? accepted[j] : drafts[j - n_acc];
    }
    return n;
}

/* the grammar cut.  st: the runner's state (it has accepted the pending id); step(&state, id): advance a state by one draft, false when the state
 * refuses it (an id without a piece, EOS among them, is refused); done(state): the grammar is complete.  states receives k + 1 states — states[i] is
 * the state whose mask row i samples under — and the return value k <= nd is the number of drafts that stay */
template <class State, class Step, class Done>
static inline int tk_lookup_grammar_cut(const State& st, const int32_t* drafts, int nd, Step step, Done done, std::vector<State>* states) {
    states->clear();
    states->push_back(st);
    for (int j = 0; j < nd; ++j) {
        State next = states->back();
        if (!step(&next, drafts[j]) || done(next)) break;
        states->push_back(next);
    }
    return (int)states->size() - 1;
}

#endif
