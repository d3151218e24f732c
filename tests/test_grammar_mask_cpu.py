"""Grammar token masks by the per-token walk (csrc/common/tk_grammar_walk.h), on the host: tk_mi355x_grammar_mask_probe with device -1, no GPU.

The yardstick (tests/grammar_mask_cases.py) knows neither the walk nor the trie walk: token t is allowed after `prefix` iff tk_mi355x_grammar_check accepts
every byte of prefix + piece, and the end-of-sequence token iff the grammar is complete after `prefix`."""
import numpy as np
import pytest

import grammar_mask_cases as G
import trackiellm_amd as tk

TK_ERROR_INVALID_ARGUMENT = 1001
DEVICE = -1


def run_case(gbnf, prefixes, n, eos, device):
    """one probe call against the yardstick; returns (bits, undecided)"""
    bits, und = G.host(gbnf, prefixes, n, eos) if device < 0 else G.probe(gbnf, prefixes, n, eos, device)
    want = G.yardstick(gbnf, prefixes, n, eos)
    assert np.array_equal(bits, want), [(r, prefixes[r]) for r in range(len(prefixes)) if not np.array_equal(bits[r], want[r])]
    assert not und.any(), und.tolist()
    return bits, und


@pytest.mark.parametrize("n", G.SIZES)
def test_tool_grammar_at_every_vocabulary_edge(n):
    """the named states — inside a string, after a backslash, after 0, in white space, complete, deep in arrays — at the word, wave and workgroup edges"""
    bits, _ = run_case(None, G.rows_case(len(G.STATES)), n, G.eos_of(n), DEVICE)
    if n % 32:
        assert not (bits[:, -1] >> np.uint32(n % 32)).any()  # the bits above the vocabulary are 0
    if n >= 3:
        complete = [p in (b"{}", b"{ }") or p.endswith(b'"v"}}}') for p in G.rows_case(len(G.STATES))]
        assert [bool(b[0] >> 2 & 1) for b in bits] == complete  # the end-of-sequence token (id 2), whatever its piece


@pytest.mark.parametrize("rows", [1, 5, G.MAX_ROWS])
def test_row_counts(rows):
    run_case(None, G.rows_case(rows), 257, 2, DEVICE)


def test_rows_that_are_off_come_back_as_given():
    pre = list(G.rows_case(6))
    for r in (0, 3, 5):
        pre[r] = None
    n, words = 65, 3
    bits = np.full((6, words), 0xA5A5A5A5, np.uint32)
    und = np.full(6, -7, np.int32)
    G.probe(None, pre, n, 2, DEVICE, bits=bits, undecided=und)
    live = [r for r in range(6) if pre[r] is not None]
    want = G.yardstick(None, tuple(pre[r] for r in live), n, 2)
    for i, r in enumerate(live):
        assert np.array_equal(bits[r], want[i]) and und[r] == 0  # whole words written, the bits above the vocabulary 0 over the sentinel
    for r in (0, 3, 5):
        assert (bits[r] == 0xA5A5A5A5).all() and und[r] == -7


def test_operators_groups_and_repetitions():
    """the grammar of test_grammar_cpu.py::test_operators_groups_comments_and_errors: + ? * {2,3}, a group, a recursion through it"""
    run_case(G.OPERATORS, tuple(s.encode() for s in G.OPERATOR_STATES), 340, 2, DEVICE)


def overflow_case(device):
    voc = G.overflow_vocabulary()
    long_id = voc.index(b"(" * 40)
    pre = [b"", b"((", b"((x)", b"(((("]
    bits, und = tk.grammar_mask_probe(G.RECURSIVE, pre, voc, eos=-1, device=device)
    for r, p in enumerate(pre):
        want = G.yardstick_row(G.RECURSIVE, p, voc, -1)
        opens = not p.endswith(b")")  # a '(' may follow: the long run is in the language there, and beyond the walk's caps
        assert bool(want[long_id >> 5] >> (long_id & 31) & 1) == opens
        assert und[r] == (1 if opens else 0), (p, und.tolist())
        assert not bits[r, long_id >> 5] >> (long_id & 31) & 1  # undecided is written as forbidden
        want[long_id >> 5] &= ~np.uint32(1 << (long_id & 31))
        assert np.array_equal(bits[r], want), p  # every other bit is exact
    return bits, und


def test_a_piece_beyond_the_caps_is_undecided_never_guessed():
    overflow_case(DEVICE)


def test_refused_arguments():
    voc = list(G.vocabulary(33))
    bits, und = np.full((2, 2), 0x5A5A5A5A, np.uint32), np.full(2, -3, np.int32)
    ok = dict(gbnf=None, prefixes=[b"{", b"{}"], pieces=voc, eos=2, bits=bits, undecided=und, device=DEVICE)
    bad_offsets = np.arange(34, dtype=np.uint32)
    cases = [dict(prefixes=[]), dict(prefixes=[b"{"] * (G.MAX_ROWS + 1), bits=np.zeros((G.MAX_ROWS + 1, 2), np.uint32), undecided=np.zeros(G.MAX_ROWS + 1, np.int32)),
             dict(vocab=0), dict(eos=33), dict(eos=-2), dict(offsets=bad_offsets + 1), dict(offsets=bad_offsets[::-1].copy()),
             dict(offsets=np.concatenate([[0], np.full(33, 1 << 27)]).astype(np.uint32)), dict(prefixes=[b"{", b"x"]), dict(prefixes=[b"{", b'{"x'])]
    for kw in cases:
        args = dict(ok)
        args.update(kw)
        with pytest.raises(tk.TkError) as e:
            tk.grammar_mask_probe(**args)
        assert e.value.code == TK_ERROR_INVALID_ARGUMENT, kw
    with pytest.raises(tk.TkError) as e:
        tk.grammar_mask_probe(**dict(ok, gbnf='root ::= "abc'))
    assert e.value.code != TK_ERROR_INVALID_ARGUMENT  # the parser's refusal, as tk_mi355x_grammar_check reports it
    assert (bits == 0x5A5A5A5A).all() and (und == -3).all()  # nothing was written


def test_no_token_is_undecided_anywhere_in_the_golden_documents():
    """EVERY distinct prefix of the 210 golden documents under the tool-call grammar with the test vocabulary: the walk decides every token (the caps of
    tk_grammar_walk.h were chosen from this), and at every 16th prefix the whole row equals the yardstick"""
    gp = G.golden_prefixes()
    assert len(gp) > 5000
    n = 340  # the byte pieces, every multi-byte piece of the cases and the empty ones
    assert set(G.MULTI) <= set(G.vocabulary(n))
    for i in range(0, len(gp), G.MAX_ROWS):
        bits, und = G.host(None, gp[i:i + G.MAX_ROWS], n, 2)
        assert not und.any(), [(gp[i + r], int(und[r])) for r in np.nonzero(und)[0]]
        for r in range(0, len(bits), 16):
            assert np.array_equal(bits[r], G.yardstick_row(None, gp[i + r], G.vocabulary(n), 2)), gp[i + r]
