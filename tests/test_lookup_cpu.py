"""No GPU: lookup decoding's draft and accept rules (csrc/llm/tk_lookup.h behind tk_mi355x_lookup_draft / tk_mi355x_lookup_accept) against the
Python restatement tests/lookup_ref.py, on crafted cases and on seeded random streams over a small alphabet (so that n-grams repeat)."""
import ctypes as C
import random

import numpy as np
import pytest

import lookup_ref as R

EOS = 2


def both_draft(tk, ctx, pred, nmin, nmax, nd):
    got = tk.lookup_draft(ctx, pred, nmin, nmax, nd)
    assert got == R.draft(ctx, pred, nmin, nmax, nd), (ctx, pred, nmin, nmax, nd)
    return got


def both_accept(tk, toks, picks, eos=EOS):
    got = tk.lookup_accept(toks, picks, eos)
    assert got == R.accept(toks, picks, eos), (toks, picks)
    return got


def test_entries_exist(tk):
    for name in ("tk_mi355x_lookup_draft", "tk_mi355x_lookup_accept", "tk_mi355x_llm_forward_verify", "tk_mi355x_attention_plan_verify",
                 "tk_mi355x_llm_runner_set_lookup", "tk_mi355x_llm_runner_set_prediction", "tk_mi355x_llm_runner_lookup_stats"):
        assert hasattr(tk.lib(), name), name
    assert tk.lib().tk_mi355x_llm_runner_set_lookup(None, 4, 1, 3) == 1001
    assert tk.lib().tk_mi355x_llm_runner_set_prediction(None, None, 0) == 1001
    assert tk.lib().tk_mi355x_llm_runner_lookup_stats(None, None, None, None) == 1001
    assert tk.lib().tk_mi355x_llm_forward_verify(None, 1, None, None, None, -1, None, None) == 1001


def test_no_hit(tk):
    assert both_draft(tk, [5, 6, 7, 8], [], 1, 3, 4) == []
    assert both_draft(tk, [5, 6, 7, 8], [9, 10, 11], 1, 3, 4) == []
    assert both_draft(tk, [8], [], 1, 3, 4) == []      # nothing before the pending id
    assert both_draft(tk, [5, 6, 7, 8], [8], 1, 3, 4) == []  # the prediction ends with the match: nothing behind it (j + n < P)


def test_hit_only_at_ngram_min(tk):
    # the last 3 and the last 2 ids occur nowhere else; the last id does, at index 1
    assert both_draft(tk, [5, 9, 6, 7, 4, 9], [], 1, 3, 4) == [6, 7, 4, 9]
    assert both_draft(tk, [5, 9, 6, 7, 4, 9], [], 2, 3, 4) == []


def test_prediction_before_context(tk):
    ctx = [5, 6, 7, 11, 12, 6, 7]
    assert both_draft(tk, ctx, [20, 6, 7, 30, 31, 32], 2, 2, 2) == [30, 31]
    assert both_draft(tk, ctx, [], 2, 2, 2) == [11, 12]
    # a longer n-gram in the context wins over a shorter one in the prediction: n goes down, sources alternate inside one n
    assert both_draft(tk, ctx, [20, 7, 30], 1, 2, 2) == [11, 12]


def test_continuation_cut_by_the_end_of_the_source(tk):
    assert both_draft(tk, [5, 6], [4, 6, 30, 31], 1, 1, 8) == [30, 31]           # cut by P
    assert both_draft(tk, [6, 30, 5, 6], [], 1, 1, 8) == [30, 5, 6]               # cut by L: the context's continuation runs into the pending id
    assert both_draft(tk, [5, 6], [4, 6, 30, 31, 32, 33], 1, 1, 3) == [30, 31, 32]  # cut by n_draft
    assert both_draft(tk, [5, 6], [4, 6, 30], 1, 1, 0) == []


def test_repeated_ngram_smallest_in_the_prediction_largest_in_the_context(tk):
    assert both_draft(tk, [9, 6], [6, 40, 6, 41, 6, 42], 1, 1, 1) == [40]
    assert both_draft(tk, [6, 40, 6, 41, 6, 42, 6], [], 1, 1, 1) == [42]
    assert both_draft(tk, [6, 7, 40, 6, 7, 41, 9, 6, 7], [], 2, 2, 2) == [41, 9]


def test_accept_cases(tk):
    assert both_accept(tk, [10, 11, 12, 13], [11, 12, 13, 14]) == [11, 12, 13, 14]        # all drafts right
    assert both_accept(tk, [10, 11, 12, 13], [99, 12, 13, 14]) == [99]                    # the first draft wrong
    assert both_accept(tk, [10, 11, 12, 13], [11, 77, 13, 14]) == [11, 77]
    assert both_accept(tk, [10, 11, EOS, 13], [11, EOS, 13, 14]) == [11, EOS]             # an EOS pick inside a confirmed run ends it
    assert both_accept(tk, [10, 11, 12], [EOS, 12, 13]) == [EOS]
    assert both_accept(tk, [10], [33]) == [33]
    assert both_accept(tk, [10, 11], [11, EOS]) == [11, EOS]


def test_random_streams(tk):
    rng = random.Random(20260)
    for case in range(200):
        L, P = rng.randint(1, 40), rng.choice([0, 0, rng.randint(1, 30)])
        ctx = [rng.randint(3, 8) for _ in range(L)]
        pred = [rng.randint(3, 8) for _ in range(P)]
        nmin = rng.randint(1, 4)
        nmax = rng.randint(nmin, min(8, nmin + 3))
        nd = rng.randint(0, 15)
        d = both_draft(tk, ctx, pred, nmin, nmax, nd)
        assert len(d) <= nd
        toks = [ctx[-1]] + d
        # picks: the drafts confirmed up to a random point, EOS now and then
        k = rng.randint(0, len(toks))
        picks = [(toks[i + 1] if i + 1 < len(toks) and i < k else rng.randint(2, 8)) for i in range(len(toks))]
        ids = both_accept(tk, toks, picks)
        assert 1 <= len(ids) <= len(toks) and EOS not in ids[:-1]


def test_schedule_restatement_accounts_for_every_token():
    """the schedule's own arithmetic: the passes' accepted drafts and the one-row steps add up to the stream"""
    rng = random.Random(7)
    for case in range(50):
        prompt = [1] + [rng.randint(3, 6) for _ in range(rng.randint(1, 12))]
        stream = [rng.randint(3, 6) for _ in range(rng.randint(1, 60))] + [EOS]
        n_ctx = rng.choice([24, 48, 256])
        # the plain run samples while rows fit: the id sampled from position n_ctx - 2 is its last
        stream = stream[:max(1, n_ctx - len(prompt))]
        pred = stream if case % 2 else []
        fed, passes, drafted, accepted = R.schedule(prompt, stream, pred, 1, 3, 4, n_ctx, EOS)
        assert passes == len(fed) and drafted == sum(len(t) - 1 for t in fed) and accepted <= drafted
        for t in fed:
            assert 2 <= len(t) <= 5
    # a stream of distinct ids predicted exactly: every pass confirms its four drafts until the stream runs out
    stream = list(range(10, 40)) + [EOS]
    fed, passes, drafted, accepted = R.schedule([1, 3], stream, stream, 1, 3, 4, 256, EOS)
    assert fed[0] == [10, 11, 12, 13, 14] and fed[1] == [15, 16, 17, 18, 19]
    assert passes == 6 and drafted == 24 and accepted == 24
    # the same at the end of a context of 12 positions: rows 2 .. 10 may be fed, the drafts of the second pass are clipped to them
    fed, passes, drafted, accepted = R.schedule([1, 3], stream[:10], stream, 1, 3, 4, 12, EOS)
    assert fed == [[10, 11, 12, 13, 14], [15, 16, 17, 18]] and (passes, drafted, accepted) == (2, 7, 7)


def test_bad_arguments(tk):
    L = tk.lib()
    ctx = np.array([5, 6, 7, 6], np.int32)
    pred = np.array([6, 9, 9], np.int32)
    out = np.zeros(16, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.tk_mi355x_lookup_draft(p(ctx), 4, p(pred), 3, 1, 3, 4, p(out)) == 2
    assert L.tk_mi355x_lookup_draft(p(ctx), 4, None, 0, 1, 3, 4, p(out)) == 2
    assert L.tk_mi355x_lookup_draft(p(ctx), 4, p(pred), 3, 1, 3, 16, p(out)) == -1   # n_draft above 15
    assert L.tk_mi355x_lookup_draft(p(ctx), 4, p(pred), 3, 1, 3, -1, p(out)) == -1
    assert L.tk_mi355x_lookup_draft(p(ctx), 4, p(pred), 3, 0, 3, 4, p(out)) == -1    # ngram_min 0
    assert L.tk_mi355x_lookup_draft(p(ctx), 4, p(pred), 3, 3, 2, 4, p(out)) == -1    # ngram_min > ngram_max
    assert L.tk_mi355x_lookup_draft(p(ctx), 4, p(pred), 3, 1, 9, 4, p(out)) == -1    # ngram_max above 8
    assert L.tk_mi355x_lookup_draft(None, 4, p(pred), 3, 1, 3, 4, p(out)) == -1
    assert L.tk_mi355x_lookup_draft(p(ctx), -1, p(pred), 3, 1, 3, 4, p(out)) == -1
    assert L.tk_mi355x_lookup_draft(p(ctx), 4, None, 3, 1, 3, 4, p(out)) == -1
    assert L.tk_mi355x_lookup_draft(p(ctx), 4, p(pred), 3, 1, 3, 4, None) == -1
    toks = np.array([5, 6], np.int32)
    assert L.tk_mi355x_lookup_accept(p(toks), p(toks), 2, EOS, p(out)) == 1
    assert L.tk_mi355x_lookup_accept(p(toks), p(toks), 0, EOS, p(out)) == -1
    assert L.tk_mi355x_lookup_accept(None, p(toks), 2, EOS, p(out)) == -1
    assert L.tk_mi355x_lookup_accept(p(toks), None, 2, EOS, p(out)) == -1
    assert L.tk_mi355x_lookup_accept(p(toks), p(toks), 2, EOS, None) == -1
    with pytest.raises(ValueError):
        tk.lookup_draft([5, 6], [], 2, 1, 4)
