"""Whisper's language detection over rows of decoder logits, restated in NumPy float64 from the comment at the head of
trackiellm_amd/csrc/common/tk_lang_pick.h (not from its code):

  per row, over the n_lang consecutive logits l[0 .. n_lang) that start at token tok0:
    1. id = first index of the maximum under `>` (a NaN is never greater); no logit above -inf: id = 0.  m = l[id]
    2. p_i = 0 where l_i is a NaN or -inf, else exp(l_i - m) (exactly 1 where l_i == m); no logit above -inf: every p_i and prob_i is 0
    3. S = the sum of the p_i
    4. prob_i = p_i / S
  where auto_row[row] != 0 the token tok0 + id is stored into slot[row]; other rows' slots stay as they are.

The library does 2 - 4 in fp32 (tk_expf, n_lang additions in index order, one division); bound() is what that may differ from here.

MUTATIONS are deliberate mistakes a kernel could make; the cases of tests/lang_pick_cases.py must tell each one from the real thing."""
import numpy as np

from token_pick_ref import EXPF_REL_ERR

EPS = 2.0 ** -24
MUTATIONS = (
    "tie_higher",      # ties go to the higher index
    "wrong_row",       # row r reads the logits of row r + 1 (the last one: row 0)
    "slot_non_auto",   # the slot is written on a row that does not detect
    "slot_off_by_one", # the token stored is tok0 + id + 1
    "sum_short",       # the sum leaves out the last language
    "drop_lane64",     # the languages from index 64 on are never read
)


def pick(logits, rows, cols, ld, tok0, n_lang, auto_row, slot, mutation=None):
    """-> (ids int32 [rows], probs float64 [rows][n_lang], slot int32 [rows])"""
    assert mutation is None or mutation in MUTATIONS
    x = np.asarray(logits, np.float32).reshape(-1)
    auto_row = np.asarray(auto_row, np.int32)
    slot = np.array(slot, np.int32, copy=True)
    ids = np.zeros(rows, np.int32)
    probs = np.zeros((rows, n_lang), np.float64)
    for r in range(rows):
        src = (r + 1) % rows if mutation == "wrong_row" else r
        l = x[src * ld + tok0: src * ld + tok0 + n_lang].astype(np.float64)
        seen = n_lang if mutation != "drop_lane64" else min(n_lang, 64)
        best, idx = -np.inf, 0
        for i in range(seen):
            if l[i] > best or (mutation == "tie_higher" and l[i] == best and l[i] > -np.inf):
                best, idx = l[i], i
        ids[r] = idx
        if best > -np.inf:
            p = np.zeros(n_lang)
            for i in range(seen):
                if l[i] > -np.inf:                                   # false for a NaN
                    p[i] = 1.0 if l[i] == l[idx] else np.exp(l[i] - l[idx])
            S = p[: n_lang - 1].sum() if mutation == "sum_short" and n_lang > 1 else p.sum()
            probs[r] = p / S
        if auto_row[r] != 0 or mutation == "slot_non_auto":
            slot[r] = tok0 + idx + (1 if mutation == "slot_off_by_one" else 0)
    return ids, probs, slot


def bound(logits, rows, ld, tok0, n_lang, ids, probs):
    """per probability, what the fp32 chain may be off the float64 value: the subtraction l_i - m rounds once (EPS |l_i - m|, a relative error
    of the exponential), tk_expf adds EXPF_REL_ERR to the term and to the terms of the sum alike (2 EXPF_REL_ERR), the n_lang additions and the
    division round once each ((n_lang + 2) EPS covers them with the sum's own share of the subtraction), and a quotient in the denormal range is
    rounded to a multiple of 2^-149 (2^-126 covers it)."""
    x = np.asarray(logits, np.float32).reshape(-1)
    out = np.zeros((rows, n_lang))
    for r in range(rows):
        l = x[r * ld + tok0: r * ld + tok0 + n_lang].astype(np.float64)
        with np.errstate(invalid="ignore"):
            d = np.where(np.isfinite(l), np.abs(l - l[ids[r]]), 0.0)
        d = np.where(np.isfinite(d), d, 0.0)
        out[r] = probs[r] * (2 * EXPF_REL_ERR + (n_lang + 2) * EPS + d * EPS) + 2.0 ** -126
    return out
