"""GPU: k_grammar_mask alone (tk_mi355x_grammar_mask_probe, device 0).  The cases of tests/test_grammar_mask_cpu.py, each ONE launch over a few thousand
tokens at the most; the result must equal the device -1 result and the yardstick (tests/grammar_mask_cases.py) bit for bit, the undecided counts included."""
import numpy as np
import pytest

import grammar_mask_cases as G
import test_grammar_mask_cpu as H

pytestmark = pytest.mark.gpu


def both(gbnf, prefixes, n, eos):
    dev_bits, dev_und = H.run_case(gbnf, prefixes, n, eos, 0)
    host_bits, host_und = G.host(gbnf, prefixes, n, eos)
    assert np.array_equal(dev_bits, host_bits) and np.array_equal(dev_und, host_und)


@pytest.mark.parametrize("n", G.SIZES)
def test_tool_grammar_at_every_vocabulary_edge(gpu, n):
    both(None, G.rows_case(len(G.STATES)), n, G.eos_of(n))


@pytest.mark.parametrize("rows", [1, 5, G.MAX_ROWS])
def test_row_counts(gpu, rows):
    both(None, G.rows_case(rows), 257, 2)


def test_rows_that_are_off_come_back_as_given(gpu):
    pre = list(G.rows_case(6))
    for r in (0, 3, 5):
        pre[r] = None
    got = G.probe(None, pre, 65, 2, 0, bits=np.full((6, 3), 0xA5A5A5A5, np.uint32), undecided=np.full(6, -7, np.int32))
    want = G.probe(None, pre, 65, 2, -1, bits=np.full((6, 3), 0xA5A5A5A5, np.uint32), undecided=np.full(6, -7, np.int32))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (got[0][[0, 3, 5]] == 0xA5A5A5A5).all() and (got[1][[0, 3, 5]] == -7).all() and not got[1][[1, 2, 4]].any()


def test_operators_groups_and_repetitions(gpu):
    both(G.OPERATORS, tuple(s.encode() for s in G.OPERATOR_STATES), 340, 2)


def test_a_piece_beyond_the_caps_is_undecided_never_guessed(gpu):
    dev = H.overflow_case(0)
    host = H.overflow_case(-1)
    assert np.array_equal(dev[0], host[0]) and np.array_equal(dev[1], host[1])


def test_golden_document_prefixes(gpu):
    """256 prefixes of the golden documents at a stride over all of them, one launch: no undecided token, the host's bits"""
    gp = G.golden_prefixes()
    pre = tuple(gp[(i * 21) % len(gp)] for i in range(G.MAX_ROWS))
    bits, und = G.probe(None, pre, 340, 2, 0)
    host_bits, host_und = G.host(None, pre, 340, 2)
    assert not und.any() and np.array_equal(bits, host_bits) and np.array_equal(und, host_und)
    for r in range(0, G.MAX_ROWS, 16):
        assert np.array_equal(bits[r], G.yardstick_row(None, pre[r], G.vocabulary(340), 2)), pre[r]
