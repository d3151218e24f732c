/*
 * tk_lookup.h — the drafting and acceptance rules of lookup decoding (tk_llm_batcher.h "Verify requests", tk_abi_llm.cpp), host only: no device,
 * no state.
 *
 * A greedy runner that has the id `c[L - 1]` pending guesses the ids that follow it from text it already holds — a prediction its host gave it,
 * then its own context — and feeds the pending id and the guesses as consecutive positions of ONE pass.  The model's own arg max of every row
 * says how many guesses it would have produced itself; those ids are exactly the ones one-row passes would have sampled, because a row's bits
 * depend neither on its pass nor on its neighbours.
 */
#ifndef TK_LOOKUP_H
#define TK_LOOKUP_H

#include <stdint.h>

#define TK_LOOKUP_MAX_DRAFT 15  /* drafts per pass: with the pending id, 16 rows */
#define TK_LOOKUP_MAX_NGRAM 8
#define TK_LOOKUP_MAX_PRED 4096 /* ids of a runner's prediction */

/* Draft rule.  ctx[0 .. n_ctx): the prompt and every id sampled so far, the pending one last; pred[0 .. n_pred): the host's prediction (may be
 * empty).  For n = ngram_max down to ngram_min (n <= n_ctx), s = the last n ids of ctx:
 *   (a) the prediction: the smallest j with pred[j .. j + n) == s and j + n < n_pred; drafts = pred[j + n .. min(n_pred, j + n + n_draft));
 *   (b) the context: the largest j with j + n <= n_ctx - 1 and ctx[j .. j + n) == s; drafts = ctx[j + n .. min(n_ctx, j + n + n_draft)).
 * The first hit wins.  Returns the number of drafts written to out (room for n_draft), 0 when nothing matches, -1 on bad arguments. */
static inline int tk_lookup_draft(const int32_t* ctx, int n_ctx, const int32_t* pred, int n_pred, int ngram_min, int ngram_max, int n_draft, int32_t* out) {
    if (n_ctx < 0 || n_pred < 0 || (n_ctx > 0 && !ctx) || (n_pred > 0 && !pred) || n_draft < 0 || n_draft > TK_LOOKUP_MAX_DRAFT || (n_draft > 0 && !out) ||
        ngram_min < 1 || ngram_min > ngram_max || ngram_max > TK_LOOKUP_MAX_NGRAM)
        return -1;
    if (n_draft == 0) return 0;
    for (int n = ngram_max; n >= ngram_min; --n) {
        if (n > n_ctx) continue;
        const int32_t* s = ctx + (n_ctx - n);
        auto same = [&](const int32_t* a) {
            for (int i = 0; i < n; ++i)
                if (a[i] != s[i]) return false;
            return true;
        };
        for (int j = 0; j + n < n_pred; ++j) {
            if (!same(pred + j)) continue;
            int k = 0;
            for (int i = j + n; i < n_pred && k < n_draft; ++i) out[k++] = pred[i];
            return k;
        }
        for (int j = n_ctx - 1 - n; j >= 0; --j) {
            if (!same(ctx + j)) continue;
            int k = 0;
            for (int i = j + n; i < n_ctx && k < n_draft; ++i) out[k++] = ctx[i];
            return k;
        }
    }
    return 0;
}

/* Accept rule.  toks[0 .. n): what the pass fed — toks[0] the pending id, toks[1 ..] the drafts; picks[0 .. n): the arg max of every row.  m = the
 * number of leading drafts the picks confirm (picks[i] == toks[i + 1] for all i < m), cut at the first pick that is EOS.  out_ids (room for n)
 * receives picks[0 .. m]; rows 0 .. m of the pass hold valid cache rows.  Returns m + 1, or -1 on bad arguments. */
static inline int tk_lookup_accept(const int32_t* toks, const int32_t* picks, int n, int32_t eos, int32_t* out_ids) {
    if (n < 1 || !toks || !picks || !out_ids) return -1;
    int m = 0;
    while (m < n - 1 && picks[m] != eos && picks[m] == toks[m + 1]) ++m;
    for (int i = 0; i <= m; ++i) out_ids[i] = picks[i];
    return m + 1;
}

#endif
