"""Lookup decoding for runners that sample, are masked, adjusted or ask for records (csrc/llm/tk_lookup_scope.h, the runner in csrc/abi/tk_abi_llm.cpp),
restated in Python from the rules' text.  It builds on nothing in the library but the tokenizer's byte rule: a synthetic model's id 3 + b is the byte b,
ids 0 .. 2 have no piece, any other id is the text " t<id>".

  scope_allows    which runner drafts
  row_counter     the sampling counter of row i
  row_window      the penalty window of row i
  ToolCallGrammar the tool-call language (the built-in grammar text of csrc/llm/tk_grammar.cpp) as a recogniser: dead / partial / complete
  grammar_cut     the drafts that stay under the grammar
  schedule        the passes, drafted and accepted counts of a runner for a given prompt, token stream and prediction"""
import sys

import lookup_ref as L

SAMPLED, GRAMMAR, ADJUSTED, LOGPROBS = 1, 2, 4, 8


def scope_allows(flags, sampled, grammar, adjusted, logprobs):
    """a runner with lookup on drafts iff every condition that holds has its bit"""
    holds = [(sampled, SAMPLED), (grammar, GRAMMAR), (adjusted, ADJUSTED), (logprobs, LOGPROBS)]
    return all(flags & bit for cond, bit in holds if cond)


def row_counter(c, i):
    return (c + i) & 0xFFFFFFFF


def row_window(accepted, drafts, i, last_n):
    """the runner's window (the pending id last) after drafts 0 .. i - 1, cut to last_n"""
    w = list(accepted) + list(drafts[:i])
    return w[len(w) - last_n:] if 0 < last_n < len(w) else (w if last_n > 0 else [])


def cut_by(steps):
    """steps[j]: 0 the state refuses draft j, 1 it accepts it, 2 it accepts it and is complete.  The number of drafts that stay"""
    kept = 0
    for s in steps:
        if s != 1:
            break
        kept += 1
    return kept


def piece(tok_id):
    if 3 <= tok_id < 259:
        return bytes([tok_id - 3])
    if tok_id < 3:
        return b""
    return (" t%d" % tok_id).encode()


# ---- the tool-call language --------------------------------------------------------------------------------------------------------------------
# Parsers in continuation-passing style: p(text, i, k) calls k(j) for every j at which p can end when it starts at i.  A terminal that needs a byte
# behind the end of the text marks the text as a viable prefix.

class _Run:
    partial = False
    complete = False


def _lit(s):
    bs = s.encode()

    def p(run, t, i, k):
        for n, b in enumerate(bs):
            if i + n == len(t):
                run.partial = True
                return
            if t[i + n] != b:
                return
        k(i + len(bs))
    return p


def _cls(chars, negate=False):
    members = set(chars.encode())

    def p(run, t, i, k):
        if i == len(t):
            run.partial = True
            return
        if (t[i] in members) != negate:
            k(i + 1)
    return p


def _seq(*ps):
    def p(run, t, i, k, at=0):
        if at == len(ps):
            return k(i)
        ps[at](run, t, i, lambda j: p(run, t, j, k, at + 1))
    return p


def _alt(*ps):
    def p(run, t, i, k):
        for q in ps:
            q(run, t, i, k)
    return p


def _opt(q):
    def p(run, t, i, k):
        k(i)
        q(run, t, i, k)
    return p


def _star(q):
    def p(run, t, i, k):
        k(i)
        q(run, t, i, lambda j: p(run, t, j, k) if j > i else None)
    return p


def _plus(q):
    return _seq(q, _star(q))


def _ref(name):
    return lambda run, t, i, k: _RULES[name](run, t, i, k)


_ws = _star(_cls(" \t\n"))
_digit = _cls("0123456789")
_hex = _cls("0123456789abcdefABCDEF")
_string = _seq(_lit('"'), _star(_alt(_cls('"\\', negate=True), _seq(_lit("\\"), _alt(_cls('"\\/bfnrt'), _seq(_lit("u"), _hex, _hex, _hex, _hex))))), _lit('"'), _ws)
_number = _seq(_opt(_lit("-")), _alt(_digit, _seq(_cls("123456789"), _star(_digit))), _opt(_seq(_lit("."), _plus(_digit))),
               _opt(_seq(_cls("eE"), _opt(_cls("-+")), _plus(_digit))), _ws)
_object = _seq(_lit("{"), _ws, _opt(_seq(_lit('"tool_call":'), _ws, _ref("call"))), _ws, _lit("}"))
_member = _seq(_string, _lit(":"), _ws, _ref("value"))
_RULES = {
    "root": _object,
    "call": _seq(_lit("{"), _ws, _lit('"name":'), _ws, _string, _lit(","), _ws, _lit('"arguments":'), _ws, _ref("args"), _ws, _lit("}")),
    "args": _seq(_lit("{"), _ws, _opt(_seq(_member, _star(_seq(_lit(","), _ws, _member)))), _ws, _lit("}")),
    "value": _alt(_object, _ref("array"), _string, _number, _lit("true"), _lit("false"), _lit("null")),
    "array": _seq(_lit("["), _ws, _opt(_seq(_ref("value"), _star(_seq(_lit(","), _ws, _ref("value"))))), _ws, _lit("]")),
}


class ToolCallGrammar:
    @staticmethod
    def status(text):
        """'complete': the text is a sentence; 'partial': it is not, and some sentence begins with it; 'dead' otherwise"""
        text = bytes(text)
        run = _Run()
        old = sys.getrecursionlimit()
        sys.setrecursionlimit(max(old, 20000))
        try:
            def end(j):
                if j == len(text):
                    run.complete = True
            _RULES["root"](run, text, 0, end)
        finally:
            sys.setrecursionlimit(old)
        return "complete" if run.complete else "partial" if run.partial else "dead"


def grammar_cut(text, drafts):
    """text: what the grammar has accepted, the pending id's piece included.  The drafts in front of the first one the state refuses (an id without a
    piece is refused) and of the first one that would complete the grammar"""
    kept = []
    text = bytes(text)
    for d in drafts:
        pc = piece(d)
        if not pc:
            break
        if ToolCallGrammar.status(text + pc) != "partial":
            break
        text += pc
        kept.append(d)
    return kept


def schedule(prompt_ids, stream, pred, ngram_min, ngram_max, n_draft, n_ctx, eos, grammar=False):
    """tests/lookup_ref.py's schedule for a runner inside its scope.  stream: every id the run with lookup off SAMPLES after the prompt — under its
    temperature, mask, penalties —, the one it ends on last.  Row i of a verify pass samples under the tables a one-row pass would have had, so its pick
    is stream[i + 1] as long as the rows before it hold the plain run's ids: the greedy schedule, with the drafts cut by the grammar first.  grammar: the
    stream is a tool call; the run pauses at the id that completes it, which is never fed.  Returns (fed, verify_passes, drafted, accepted)"""
    prompt_ids, stream = list(prompt_ids), list(stream)
    n_past, i = len(prompt_ids), 0
    fed, passes, drafted, accepted = [], 0, 0, 0
    said = b""  # what the grammar has accepted: the pieces of stream[0 .. i]
    while i < len(stream) and stream[i] != eos and n_past + 1 < n_ctx:
        if grammar:
            said = b"".join(piece(t) for t in stream[:i + 1])
            if ToolCallGrammar.status(said) == "complete":
                break
        d = L.draft(prompt_ids + stream[:i + 1], pred, ngram_min, ngram_max, n_draft)
        d = d[:max(0, n_ctx - n_past - 2)]
        if grammar:
            d = grammar_cut(said, d)
        if not d:
            n_past, i = n_past + 1, i + 1
            continue
        toks = [stream[i]] + d
        picks = [stream[i + 1 + k] if i + 1 + k < len(stream) else -1 for k in range(len(toks))]
        ids = L.accept(toks, picks, eos)
        assert -1 not in ids, "the stream ends before the picks the accept rule needs"
        fed.append(toks)
        passes, drafted, accepted = passes + 1, drafted + len(d), accepted + len(ids) - 1
        n_past, i = n_past + len(ids), i + len(ids)
    return fed, passes, drafted, accepted
