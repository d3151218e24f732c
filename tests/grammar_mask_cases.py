"""Cases for k_grammar_mask (tk_mi355x_grammar_mask_probe), small, shared by tests/test_grammar_mask_cpu.py and tests/test_grammar_mask_gpu.py.

The yardstick is independent of the walk under test and of the trie walk: token t is allowed after `prefix` iff tk_mi355x_grammar_check accepts every byte of
prefix + piece (single bytes through tk_mi355x_grammar_next_bytes, which also answers for the NUL byte a C string cannot carry); the end-of-sequence token is
allowed iff the grammar is complete after `prefix`.  References are computed once per case and cached for both files."""
import ctypes as C
import functools
import json
import os
import random

import numpy as np

import trackiellm_amd as tk

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = [1, 31, 32, 33, 63, 64, 65, 257, 4099]  # word, wave and workgroup edges
MAX_ROWS = 256
RECURSIVE = 'root ::= "(" root ")" | "x"\n'
OPERATORS = 'root ::= item+ tail? # trailing comment\nitem ::= "ab" | [x-z]{2,3} | (\n  "(" root ")"\n)\ntail ::= "!"*\n'

IN_STRING = '{"tool_call":{"name":"ab'
ARGS = '{"tool_call":{"name":"a","arguments":{"k":'
# the states tests/test_grammar_cpu.py names, and a deep one
STATES = ["", "{", "{ \n\t", '{"', IN_STRING, IN_STRING + "\\", IN_STRING + "\\u0", ARGS + "-", ARGS + "0", ARGS + "12.5e", "{}", "{ }",
          ARGS + '[[{"tool_call":{"name":"b","arguments":{"z":[1, "q', ARGS + '[1,[2,[3,[{}, true', ARGS + '"v"}}', ARGS + '"v"}}}']
OPERATOR_STATES = ["", "ab", "x", "xy", "xyz", "(ab", "(ab(zz", "(ab(zz))", "xyzxy!", "abab"]

LONG = b'{"tool_call": {"name": "navigate", "arguments":{'
assert len(LONG) == 48
MULTI = [b"}}}", b"[[[[", b'":', "é中".encode(), b" t123", b'{"', b'"tool_call":', b'"name":', b'"arguments":', b"{}", b"  ", b"\n\n", b" \t", b"true", b"false",
         b"null", b"tru", b"e}", b'","', b'":{"', b"0.5", b"-1", b"1e5", b"01", b"00", b'\\"', b"\\u00", b"\\u12G4", b"\\x", b"abc", b'"a"', b'"a":', b'"a": ', b"}}", b"}]",
         b"],", b", ", b'": "', b'b",', b'{"tool_call":{"name":"', LONG, b'"}', b'"}}', b"}} ", b"[]", b"[1", b"1]", b"1,2", b"e+", b".5", b"-0", b"0}", b"0,", b'"\\', b"ab", b"xy",
         b"xyz", b"zz", b"(ab", b"))", b")!", b"!!", b"(x)", b"((", "café ".encode(), b"\xff\xfe", b"\x80", b" {", b"}\n"]


@functools.lru_cache(maxsize=None)
def vocabulary(n):
    """n pieces: the 256 byte pieces, the multi-byte pieces above and three empty ones, shuffled so that every size holds some of each kind; beyond them
    JSON-like pieces of 2 .. 12 bytes from a fixed generator"""
    rng = random.Random(1234)
    pool = [bytes([b]) for b in range(256)] + MULTI
    rng.shuffle(pool)
    # the small sizes still see the pieces the issue names
    head = [b"}}}", b"", b'":', b"{", b"[[[[", b" t123", b'"', b"}", "é中".encode(), b" ", b"\\", b"0", b"", b"\n", b""]
    pool = head + [p for p in pool if p not in head]
    alphabet = b'{}[]":, \n\\0123456789.eE-+truefalsnab' + "é".encode()
    while len(pool) < n:
        pool.append(bytes(rng.choice(alphabet) for _ in range(rng.randrange(2, 13))))
    return tuple(pool[:n])


def _check(gbnf, text):
    n, c = C.c_int32(), C.c_int32()
    rc = tk.lib().tk_mi355x_grammar_check(None if gbnf is None else gbnf.encode(), text, C.byref(n), C.byref(c))
    assert rc == 0, tk.lib().tk_error_get_detail()
    return n.value, bool(c.value)


def _next_bytes(gbnf, prefix):
    allowed = (C.c_uint8 * 256)()
    c = C.c_int32()
    rc = tk.lib().tk_mi355x_grammar_next_bytes(None if gbnf is None else gbnf.encode(), prefix, allowed, C.byref(c))
    assert rc == 0
    return bytes(allowed), bool(c.value)


def yardstick_row(gbnf, prefix, pieces, eos):
    """the mask words of one row by the yardstick"""
    prefix = prefix.encode() if isinstance(prefix, str) else prefix
    assert 0 not in prefix
    bits = np.zeros((len(pieces) + 31) // 32, np.uint32)
    single, complete = _next_bytes(gbnf, prefix)
    for t, p in enumerate(pieces):
        if t == eos:
            ok = complete
        elif len(p) == 0:
            ok = False
        elif len(p) == 1:
            ok = bool(single[p[0]])
        else:
            assert 0 not in p
            ok = _check(gbnf, prefix + p)[0] == len(prefix) + len(p)
        if ok:
            bits[t >> 5] |= np.uint32(1 << (t & 31))
    return bits


@functools.lru_cache(maxsize=None)
def yardstick(gbnf, prefixes, n, eos):
    pieces = vocabulary(n)
    return np.stack([yardstick_row(gbnf, p, pieces, eos) for p in prefixes])


@functools.lru_cache(maxsize=None)
def golden_prefixes():
    """every distinct accepted prefix of the 210 golden documents, in document order"""
    samples = json.load(open(os.path.join(GOLD, "tool_call_grammar_samples.json")))["samples"]
    assert len(samples) == 210
    seen, out = set(), []
    for s in samples:
        doc = s["doc"].encode()[: s["accepted_bytes"]]
        for k in range(len(doc) + 1):
            if doc[:k] not in seen and 0 not in doc[:k]:
                seen.add(doc[:k])
                out.append(doc[:k])
    return tuple(out)


def eos_of(n):
    return -1 if n < 3 else 2  # a token in the middle of a word; the smallest vocabularies run without one


def probe(gbnf, prefixes, n, eos, device, bits=None, undecided=None):
    return tk.grammar_mask_probe(gbnf, list(prefixes), list(vocabulary(n)), eos=eos, bits=bits, undecided=undecided, device=device)


@functools.lru_cache(maxsize=None)
def host(gbnf, prefixes, n, eos):
    """the device -1 result of a case, computed once: (bits, undecided)"""
    return probe(gbnf, prefixes, n, eos, -1)


def rows_case(k):
    """k states of the tool-call grammar: the named ones first, then prefixes of the golden documents at a fixed stride"""
    gp = golden_prefixes()
    more = [gp[(i * 37) % len(gp)] for i in range(max(0, k - len(STATES)))]
    return tuple(([s.encode() for s in STATES] + more)[:k])


def overflow_vocabulary():
    """byte pieces, short runs of '(' and one run longer than any cap on private entries the walk may have"""
    return [bytes([b]) for b in range(256)] + [b"(" * 5, b"((x))", b"(" * 40, b"(x", b"x)", b"()", b""]
