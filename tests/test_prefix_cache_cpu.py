"""Prompt prefix cache (csrc/llm/tk_llm_batcher.h), the parts that need no device: the entry points exist and refuse NULL handles, and the
matching rules (csrc/llm/tk_prefix_match.h) give the hand-derived answers on hand-written records."""
import ctypes as C

import numpy as np
import pytest

TK_ERROR_INVALID_ARGUMENT = 1001
COPY_MIN = 16   # TK_PREFIX_COPY_MIN: the issue's policy constant


def test_entry_points_exist_and_refuse_null_handles(tk):
    lib = tk.lib()
    assert lib.tk_error_to_string(TK_ERROR_INVALID_ARGUMENT) == b"TK_ERROR_INVALID_ARGUMENT"
    for name in ("tk_mi355x_llm_model_set_prefix_cache", "tk_mi355x_llm_model_prefix_cache_stats", "tk_mi355x_llm_runner_last_prompt_rows",
                 "tk_mi355x_llm_session_kv_copy", "tk_mi355x_prefix_match"):
        assert hasattr(lib, name), name
    assert lib.tk_mi355x_llm_model_set_prefix_cache(None, 1) == TK_ERROR_INVALID_ARGUMENT
    assert lib.tk_mi355x_llm_model_set_prefix_cache(None, 0) == TK_ERROR_INVALID_ARGUMENT
    n, k, c = C.c_int32(-7), C.c_int32(-7), C.c_int32(-7)
    assert lib.tk_mi355x_llm_runner_last_prompt_rows(None, C.byref(n), C.byref(k), C.byref(c)) == TK_ERROR_INVALID_ARGUMENT
    assert (n.value, k.value, c.value) == (-7, -7, -7)
    assert lib.tk_mi355x_llm_session_kv_copy(None, 0, 1, 0, 1) == TK_ERROR_INVALID_ARGUMENT
    # the totals of no model are zero, and absent outputs are allowed
    v = [C.c_uint64(9) for _ in range(4)]
    lib.tk_mi355x_llm_model_prefix_cache_stats.restype = None
    lib.tk_mi355x_llm_model_prefix_cache_stats(None, *[C.byref(x) for x in v])
    assert [x.value for x in v] == [0, 0, 0, 0]
    lib.tk_mi355x_llm_model_prefix_cache_stats(None, None, None, None, None)
    for name in ("set_prefix_cache", "prefix_cache_stats"):
        assert hasattr(tk.ModelLoader, name)
    assert hasattr(tk.LlmRunner, "last_prompt_rows") and hasattr(tk.LlmSession, "kv_copy")


def test_keep_is_the_longest_common_prefix_capped_at_n_minus_1(tk):
    toks = list(range(100, 140))                                  # n = 40
    m = lambda own: tk.prefix_match(toks, [own], self_slot=0)[0]  # noqa: E731
    assert m([]) == 0
    assert m([100]) == 1
    assert m([7] + toks[1:]) == 0                                 # differs at position 0
    assert m(toks[:25]) == 25                                     # the record ends first
    assert m(toks[:25] + [1, 2, 3]) == 25                         # ... or differs
    assert m(toks[:10] + [9] + toks[11:]) == 10                   # equal again later does not count
    assert m(toks) == 39                                          # the same prompt again: the last token is computed
    assert m(toks + [5, 6, 7]) == 39                              # a record longer than the prompt (generated rows behind it)
    assert m(toks[:39]) == 39
    assert tk.prefix_match([42], [[42, 43]], self_slot=0)[0] == 0  # n = 1: nothing to keep


def test_donor_longest_match_lowest_slot_and_the_16_position_minimum(tk):
    toks = list(range(1000, 1100))                                # n = 100
    other = [5] * 60
    # no donor: nothing matches / the only match is the prompt's own slot
    assert tk.prefix_match(toks, [[], other, other], self_slot=0)[1] == -1
    assert tk.prefix_match(toks, [toks, other], self_slot=0, cursor=0)[1] == -1
    # the minimum: a donor must reach at least 16 positions beyond the cursor
    assert tk.prefix_match(toks, [[], toks[:COPY_MIN - 1]], self_slot=0) == (0, -1, 0)
    assert tk.prefix_match(toks, [[], toks[:COPY_MIN]], self_slot=0) == (0, 1, COPY_MIN)
    assert tk.prefix_match(toks, [toks[:30], toks[:30 + COPY_MIN - 1]], self_slot=0) == (30, -1, 30)
    assert tk.prefix_match(toks, [toks[:30], toks[:30 + COPY_MIN]], self_slot=0) == (30, 1, 30 + COPY_MIN)
    # an explicit cursor (a request part of whose rows have been computed since it was first matched)
    assert tk.prefix_match(toks, [toks[:30], toks[:70]], self_slot=0, cursor=60)[1:] == (-1, 60)
    assert tk.prefix_match(toks, [toks[:30], toks[:80]], self_slot=0, cursor=60)[1:] == (1, 80)
    # a donor must match from position 0, not only beyond the cursor
    assert tk.prefix_match(toks, [toks[:30], [9] + toks[1:80]], self_slot=0)[1] == -1
    assert tk.prefix_match(toks, [toks[:30], toks[:40] + [9] + toks[41:90]], self_slot=0)[1] == -1   # 40 - 30 < 16
    assert tk.prefix_match(toks, [toks[:30], toks[:50] + [9] + toks[51:90]], self_slot=0)[1:] == (1, 50)
    # the longest match wins; among equal matches the lowest slot
    recs = [[], toks[:40], toks[:70] + [3, 3], toks[:70], toks[:55]]
    assert tk.prefix_match(toks, recs, self_slot=0) == (0, 2, 70)
    recs = [toks[:70], toks[:40], toks[:70] + [3, 3], [], toks[:70]]
    assert tk.prefix_match(toks, recs, self_slot=3) == (0, 0, 70)
    assert tk.prefix_match(toks, recs, self_slot=0, cursor=0)[1:] == (2, 70)   # the prompt's own slot never donates
    # the n - 1 cap holds for copies too: the last prompt token is computed by its owner
    assert tk.prefix_match(toks, [[], toks + [1, 2]], self_slot=0) == (0, 1, 99)
    assert tk.prefix_match(toks[:COPY_MIN], [[], toks], self_slot=0) == (0, -1, 0)          # 15 rows at most
    assert tk.prefix_match(toks[:COPY_MIN + 1], [[], toks], self_slot=0) == (0, 1, COPY_MIN)


def test_prefix_match_refuses_bad_arguments(tk):
    lib = tk.lib()
    toks = np.arange(8, dtype=np.int32)
    recs = np.zeros((2, 8), np.int32)
    lens = np.array([3, 9], np.int32)                             # longer than the stride
    out = (C.c_int32 * 3)()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.tk_mi355x_prefix_match(p(toks), 8, p(recs), p(lens), 2, 8, 0, -1, out) == -1
    lens[1] = 8
    assert lib.tk_mi355x_prefix_match(p(toks), 8, p(recs), p(lens), 2, 8, 0, -1, out) == 0
    assert lib.tk_mi355x_prefix_match(None, 8, p(recs), p(lens), 2, 8, 0, -1, out) == -1
    assert lib.tk_mi355x_prefix_match(p(toks), 0, p(recs), p(lens), 2, 8, 0, -1, out) == -1
    assert lib.tk_mi355x_prefix_match(p(toks), 8, p(recs), p(lens), 2, 8, 2, -1, out) == -1
    assert lib.tk_mi355x_prefix_match(p(toks), 8, p(recs), p(lens), 2, 8, 0, -1, None) == -1
    with pytest.raises(ValueError):
        tk.prefix_match(toks, [[1]], self_slot=4)
