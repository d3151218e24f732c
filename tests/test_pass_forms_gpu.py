"""GPU: one session walks a fixed interleaving of every form of a pass (csrc/llm/tk_pass_form.h; DESIGN.md "The forms of a pass"), twice over, on the
tiny synthetic model with a 1024-position window — the geometry and window at which tests/test_llm_gpu.py reaches the long-context form.  Contexts
are put in place with kv_write, as tests/test_llm_attention_gpu.py does; no pass runs hundreds of positions.

Every step of the walk owns its sequences (variants of one pass — plain, adjusted, with log-probabilities, both — share them: they write the same
cache rows), so a step reads nothing an earlier step wrote and its result may be compared with the same step on a session that ran nothing else.

What is held:
  * logits, picks and log-probability records of both rounds are bit-equal to the same walk on a second session under TK_MI355X_NO_GRAPH=1;
  * and to every step run alone on a fresh session — a graph recorded for one step and replayed for another holds that other step's launches;
  * the first round records exactly as many graphs as tests/pass_form_ref.py counts distinct (launches, row count) pairs in the walk, the second
    round none, the eager session none at all."""
import numpy as np
import pytest

import pass_form_ref as ref

pytestmark = pytest.mark.gpu

MAX_CTX = 1024
MAX_SEQ = 20


def caps(nrows):
    """the tiny geometry (8 heads over 2 KV heads x 64) in a window beyond 512: the scratch exists, k_attention_prefill applies, the long form up to 8 rows"""
    return (True, True, nrows <= ref.TK_LONG_ATT_MAX_ROWS)


def f16_bits(rng, shape, scale):
    return (rng.standard_normal(shape, dtype=np.float32) * scale).astype(np.float16).view(np.uint16)


class Step:
    """one entry call (or a forward + decode loop): run(sess) -> the arrays it returned; seqs: the sequences whose cached rows it reads; passes: what
    the session runs for it, as cases of pass_form_ref"""

    def __init__(self, name, seqs, passes, run):
        self.name, self.seqs, self.passes, self.run = name, seqs, passes, run


VARIANTS = {"plain": (False, False), "adjust": (True, False), "logprobs": (False, True), "both": (True, True)}


def head_step(name, variant, seq, pos, vocab, repeated):
    adjust, logprobs = VARIANTS[variant]
    seq, pos = np.asarray(seq, np.int32), np.asarray(pos, np.int32)
    n = len(seq)
    tok = np.random.default_rng(sum(map(ord, name))).integers(3, vocab, n).astype(np.int32)
    specs = [dict(repeat=1.3, freq=0.2, present=0.1, recent=[5 + r, 17, 17, 200 + r], bias_ids=[9, 40 + r], bias=[2.5, -3.0]) if r % 2 == 0 else None for r in range(n)]
    n_top = [(-1 if r % 3 == 2 else 2 + r % 3) for r in range(n)]

    def run(sess):
        if logprobs:
            logits, ids, rec = sess.forward_logprobs(seq, pos, tok, n_top, adjust=specs if adjust else None)
            return [logits, ids, rec]
        if adjust:
            return list(sess.forward_adjusted(seq, pos, tok, specs))
        return list(sess.forward(seq, pos, tok))

    entry = "forward_head_repeated" if repeated else "forward_head_distinct"
    return Step(name + ":" + variant, sorted(set(int(s) for s in seq)), [(entry, n, int(pos.max()), caps(n), adjust, logprobs)], run)


def verify_step(form, seq0, pos0, vocab):
    seq, pos = np.full(3, seq0, np.int32), np.arange(pos0, pos0 + 3, dtype=np.int32)
    tok = np.random.default_rng(700 + form).integers(3, vocab, 3).astype(np.int32)
    return Step("verify%d" % form, [seq0], [("verify%d" % form, 3, pos0 + 2, caps(3), False, False)], lambda sess: list(sess.forward_verify(seq, pos, tok, form=form)))


def prefill_step(n_prompt, vocab):
    tokens = np.random.default_rng(n_prompt).integers(3, vocab, (1, n_prompt)).astype(np.int32)
    passes = [("prefill", n_prompt - 1, n_prompt - 2, caps(n_prompt - 1), False, False), ("forward_head_distinct", 1, n_prompt - 1, caps(1), False, False)]
    return Step("prefill%d" % n_prompt, [], passes, lambda sess: [sess.prefill(tokens)])


def loop_step(seq0, pos0, n_steps, vocab):
    tok = np.random.default_rng(pos0).integers(3, vocab, 1).astype(np.int32)

    def run(sess):
        _, first = sess.forward([seq0], [pos0], tok, want_logits=False)
        toks, _ = sess.decode(1, n_steps)
        return [first, toks]

    passes = [("forward_head_distinct", 1, pos0, caps(1), False, False)] + [("decode", 1, pos0 + 1 + i, caps(1), False, False) for i in range(n_steps)]
    return Step("loop", [seq0], passes, run)


def the_walk(vocab):
    """sequence 0 is prefill()'s; 1, 2: one decode row below (300) and beyond (600) the long threshold of 1 .. 4 rows; 3 .. 7 and 8 .. 12: five
    rows below (700) and beyond (800) the threshold of 5 .. 8 rows; 13, 14: three positions of one sequence below and from position 128;
    15 .. 17: the verify forms; 18: the decode loop across position 512"""
    base = {
        "d1_short": lambda v: head_step("d1_short", v, [1], [300], vocab, False),
        "d1_long": lambda v: head_step("d1_long", v, [2], [600], vocab, False),
        "d5_short": lambda v: head_step("d5_short", v, [3, 4, 5, 6, 7], [700, 690, 5, 130, 699], vocab, False),
        "d5_long": lambda v: head_step("d5_long", v, [8, 9, 10, 11, 12], [800, 20, 780, 768, 1000], vocab, False),
        "rep_short": lambda v: head_step("rep_short", v, [13, 13, 13], [50, 51, 52], vocab, True),
        "rep_tiled": lambda v: head_step("rep_tiled", v, [14, 14, 14], [200, 201, 202], vocab, True),
    }
    order = [("d1_short", "both"), ("d5_short", "plain"), ("rep_short", "adjust"), "verify0", ("d1_long", "logprobs"), "prefill200", ("d5_long", "both"),
             ("rep_tiled", "logprobs"), "verify2", ("d1_short", "plain"), ("d1_long", "adjust"), ("d5_short", "adjust"), ("d5_long", "plain"), ("rep_short", "plain"),
             ("rep_tiled", "both"), "verify4", "prefill100", ("d1_short", "adjust"), ("d1_long", "both"), ("d5_short", "logprobs"), ("d5_long", "adjust"),
             ("rep_short", "both"), ("rep_tiled", "plain"), ("d1_short", "logprobs"), ("d1_long", "plain"), ("d5_short", "both"), ("d5_long", "logprobs"),
             ("rep_short", "logprobs"), ("rep_tiled", "adjust"), "loop"]
    other = {"verify0": lambda: verify_step(0, 15, 50, vocab), "verify2": lambda: verify_step(2, 16, 200, vocab), "verify4": lambda: verify_step(4, 17, 300, vocab),
             "prefill100": lambda: prefill_step(100, vocab), "prefill200": lambda: prefill_step(200, vocab), "loop": lambda: loop_step(18, 508, 7, vocab)}
    return [other[o]() if isinstance(o, str) else base[o[0]](o[1]) for o in order]


@pytest.fixture(scope="module")
def model(gpu):
    m = gpu.LlmModel(gpu.TINY()).fill_synthetic(4)
    yield m
    m.close()


def session_with_context(gpu, model, seqs):
    """a session whose cache holds the same seeded rows [0, MAX_CTX) for the sequences asked for, whichever session it is"""
    hp = model.hparams
    sess = gpu.LlmSession(model, MAX_SEQ, MAX_CTX)
    for layer in range(hp.n_layer):
        rng = np.random.default_rng(1000 + layer)
        k, v = f16_bits(rng, (MAX_CTX, hp.n_kv_head, hp.head_dim), 0.6), f16_bits(rng, (MAX_CTX, hp.n_kv_head, hp.head_dim), 1.0)
        for s in seqs:
            sess.kv_write(layer, s, 0, np.roll(k, s, axis=0), np.roll(v, s, axis=0))
    return sess


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_every_form_interleaved_twice(gpu, model, monkeypatch):
    monkeypatch.delenv("TK_MI355X_NO_GRAPH", raising=False)
    monkeypatch.delenv("TK_MI355X_NO_LONG_ATT", raising=False)
    monkeypatch.delenv("TK_MI355X_NO_PREFILL_ATT", raising=False)
    hp = model.hparams
    walk = the_walk(hp.vocab)
    everything = sorted(set(s for st in walk for s in st.seqs))
    # the walk reaches what it is there for: every attention of a pass, with and without the head, and every head variant
    cases = [p for st in walk for p in st.passes]
    reached = {(ref.parent_pass(*c)["attn"], c[0] in ("prefill", "forward_no_head")) for c in cases}
    assert reached == {(ref.ROW, False), (ref.TILED, False), (ref.LONG, False), (ref.RUN, False), (ref.ROW, True), (ref.TILED, True)}
    want_graphs = ref.graphs_of_walk(cases)
    assert 10 < want_graphs < len(cases)

    sess = session_with_context(gpu, model, everything)
    assert sess.graph_captures == 0
    first = [st.run(sess) for st in walk]
    assert sess.graph_captures == want_graphs
    second = [st.run(sess) for st in walk]
    assert sess.graph_captures == want_graphs, "the second round recorded a graph"
    sess.close()
    for st, a, b in zip(walk, first, second):
        assert same(a, b), st.name

    monkeypatch.setenv("TK_MI355X_NO_GRAPH", "1")
    eager = session_with_context(gpu, model, everything)
    for rnd in (first, second):
        for st, a in zip(walk, rnd):
            assert same(st.run(eager), a), ("eager", st.name)
    assert eager.graph_captures == 0
    eager.close()
    monkeypatch.delenv("TK_MI355X_NO_GRAPH")

    for st, a in zip(walk, first):
        alone = session_with_context(gpu, model, st.seqs)
        got = st.run(alone)
        assert alone.graph_captures == ref.graphs_of_walk(st.passes), st.name
        alone.close()
        assert same(got, a), ("alone", st.name)
