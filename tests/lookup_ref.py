"""Lookup decoding restated in Python (csrc/llm/tk_lookup.h, the runner's schedule in csrc/abi/tk_abi_llm.cpp): the draft rule, the accept rule,
and which passes a greedy runner submits for a given prompt, token stream and prediction.  Written from the rules' text with list slices, not
from the C loops."""


def draft(ctx, pred, ngram_min, ngram_max, n_draft):
    """the ids drafted behind the last id of ctx: for n = ngram_max .. ngram_min, the prediction first (smallest start), then the context (largest
    start that ends before the last id)"""
    ctx, pred = list(ctx), list(pred)
    L, P = len(ctx), len(pred)
    if n_draft <= 0:
        return []
    for n in range(ngram_max, ngram_min - 1, -1):
        if n > L:
            continue
        s = ctx[L - n:]
        hits = [j for j in range(P) if j + n < P and pred[j:j + n] == s]
        if hits:
            j = min(hits)
            return pred[j + n:min(P, j + n + n_draft)]
        hits = [j for j in range(L) if j + n <= L - 1 and ctx[j:j + n] == s]
        if hits:
            j = max(hits)
            return ctx[j + n:min(L, j + n + n_draft)]
    return []


def accept(toks, picks, eos):
    """picks[0 .. m]: m = the leading drafts the picks confirm, cut at the first EOS pick"""
    n = len(toks)
    assert n >= 1 and len(picks) == n
    m = 0
    while m < n - 1 and picks[m] == toks[m + 1]:
        m += 1
    for i in range(m + 1):
        if picks[i] == eos:
            m = i
            break
    return list(picks[:m + 1])


def schedule(prompt_ids, stream, pred, ngram_min, ngram_max, n_draft, n_ctx, eos):
    """The passes of a lookup runner without context shift.  stream: every id the plain greedy run SAMPLES after the prompt, in order — the ids it
    hands out, then the one it ends on (EOS, or the id that no longer fits the context).  A row's pick does not depend on its pass, so the pick of
    the row that feeds stream[i] is stream[i + 1] as long as the rows before it hold the plain run's ids; picks behind a refuted draft are never
    looked at, and stand as -1 here.  Returns (fed, verify_passes, drafted, accepted): fed = the tokens of every pass that carried drafts."""
    prompt_ids, stream = list(prompt_ids), list(stream)
    n_past, i = len(prompt_ids), 0  # stream[i] is pending: sampled, not fed
    fed, passes, drafted, accepted = [], 0, 0, 0
    while i < len(stream) and stream[i] != eos and n_past + 1 < n_ctx:
        d = draft(prompt_ids + stream[:i + 1], pred, ngram_min, ngram_max, n_draft)
        d = d[:max(0, n_ctx - n_past - 2)]  # every fed position q has q + 1 < n_ctx
        if not d:
            n_past, i = n_past + 1, i + 1
            continue
        toks = [stream[i]] + d
        picks = [stream[i + 1 + k] if i + 1 + k < len(stream) else -1 for k in range(len(toks))]
        ids = accept(toks, picks, eos)
        assert -1 not in ids, "the stream ends before the picks the accept rule needs"
        fed.append(toks)
        passes, drafted, accepted = passes + 1, drafted + len(d), accepted + len(ids) - 1
        n_past, i = n_past + len(ids), i + len(ids)
    return fed, passes, drafted, accepted
