"""GPU: lookup decoding (csrc/llm/tk_lookup.h) — the verify pass on a bare session (LlmSession.forward_verify, every attention form it can take)
against the same rows fed one per LlmSession.forward, and the feature behind tk_llm_runner_* (set_lookup / set_prediction / lookup_stats) against
the same runner with lookup off and the schedule restated in tests/lookup_ref.py.

Synthetic models tokenise bytes: ids = [1] + [3 + b ...]; id 2 ends a generation."""
import threading

import numpy as np
import pytest

import lookup_ref as R

pytestmark = pytest.mark.gpu

TK_ERROR_INVALID_ARGUMENT = 1001
EOS = 2
SEED = 4
PATH = "synthetic://tiny?seed=%d" % SEED
PROMPT = "a"  # tests/test_context_shift_gpu.py: the short prompt whose greedy stream on this seed varies most
MAX_SEQ, MAX_CTX = 3, 1100
P0S = [5, 120, 127, 505, 512, 767, 768, 1000]
RUNS = [2, 5, 8, 9]
LONG_ATT_MAX_ROWS = 8  # TK_LONG_ATT_MAX_ROWS: the widest pass the run form takes


def prompt_ids(p):
    return [1] + [3 + b for b in p.encode()]


# ---- 1. the verify pass against one-row passes ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pair(gpu):
    model = gpu.LlmModel(gpu.TINY()).fill_synthetic(SEED)
    hp = model.hparams
    a, b = gpu.LlmSession(model, MAX_SEQ, MAX_CTX), gpu.LlmSession(model, MAX_SEQ, MAX_CTX)
    rng = np.random.default_rng(77)
    shape = (hp.n_layer, MAX_SEQ, 2, MAX_CTX, hp.n_kv_head, hp.head_dim)
    # finite f16 rows for every (layer, sequence, K | V, position); keys scaled so that the softmax is neither flat nor one-hot
    rows = (rng.standard_normal(shape, dtype=np.float32) * np.array([0.6, 1.0], np.float32).reshape(1, 1, 2, 1, 1, 1)).astype(np.float16).view(np.uint16)
    stale = (rng.standard_normal(shape, dtype=np.float32) * 0.5).astype(np.float16).view(np.uint16)
    yield gpu, hp, a, b, rows, stale
    a.close()
    b.close()
    model.close()


def fill(sess, hp, rows, stale, seq, p0, n):
    """positions [0, p0) of `seq` from the seeded rows; the n rows the pass will write hold other (finite) bits first"""
    for l in range(hp.n_layer):
        if p0 > 0:
            sess.kv_write(l, seq, 0, np.ascontiguousarray(rows[l, seq, 0, :p0]), np.ascontiguousarray(rows[l, seq, 1, :p0]))
        sess.kv_write(l, seq, p0, np.ascontiguousarray(stale[l, seq, 0, p0:p0 + n]), np.ascontiguousarray(stale[l, seq, 1, p0:p0 + n]))


def new_rows(sess, hp, runs):
    return [sess.kv_read(l, s, p0, n) for l in range(hp.n_layer) for (s, p0, n) in runs]


def forms_of(gpu, hp, nrows):
    forms = [0]
    if gpu.attention_plan(nrows, hp.n_head, hp.n_kv_head, hp.head_dim, MAX_CTX, fused=False)[0] == 2:
        forms.append(2)
    if nrows <= LONG_ATT_MAX_ROWS:
        forms.append(4)
    return forms


def check_runs(pair, runs, seed):
    """runs = [(sequence, first position, rows)]: one forward_verify per form on session A, one forward per row on session B"""
    gpu, hp, a, b, rows, stale = pair
    rng = np.random.default_rng(seed)
    seq = np.concatenate([np.full(n, s, np.int32) for s, p0, n in runs])
    pos = np.concatenate([np.arange(p0, p0 + n, dtype=np.int32) for s, p0, n in runs])
    tok = rng.integers(3, hp.vocab, len(seq)).astype(np.int32)
    for s, p0, n in runs:
        fill(b, hp, rows, stale, s, p0, n)
    want_logits = np.empty((len(seq), hp.vocab), np.float32)
    want_picks = np.empty(len(seq), np.int32)
    for r in range(len(seq)):
        lg, am = b.forward(seq[r:r + 1], pos[r:r + 1], tok[r:r + 1])
        want_logits[r], want_picks[r] = lg[0], am[0]
    want_rows = new_rows(b, hp, runs)
    forms = forms_of(gpu, hp, len(seq))
    assert 0 in forms and 2 in forms and (4 in forms) == (len(seq) <= LONG_ATT_MAX_ROWS), forms
    for form in forms + [-1]:
        for s, p0, n in runs:
            fill(a, hp, rows, stale, s, p0, n)
        got_logits, got_picks = a.forward_verify(seq, pos, tok, form=form)
        assert np.array_equal(got_logits.view(np.uint32), want_logits.view(np.uint32)), (form, runs, np.abs(got_logits - want_logits).max())
        assert np.array_equal(got_picks, want_picks), (form, runs)
        for (gk, gv), (wk, wv) in zip(new_rows(a, hp, runs), want_rows):
            assert np.array_equal(gk, wk) and np.array_equal(gv, wv), (form, runs)
    return forms


@pytest.mark.parametrize("n", RUNS)
@pytest.mark.parametrize("p0", P0S)
def test_verify_pass_equals_one_row_passes(pair, p0, n):
    """a run of n rows of one sequence from position p0: logits, picks and the appended K / V rows of every layer, bit for bit, in every form.
    (505, 8) is the run form's run from below position 512 to above it, (120, 9) and (127, *) the tiled form's runs across position 128"""
    forms = check_runs(pair, [(1, p0, n)], 1000 * p0 + n)
    if n == 9:
        gpu, hp, a = pair[0], pair[1], pair[2]
        seq, pos, tok = np.full(9, 1, np.int32), np.arange(p0, p0 + 9, dtype=np.int32), np.full(9, 7, np.int32)
        with pytest.raises(gpu.TkError) as e:
            a.forward_verify(seq, pos, tok, form=4)
        assert e.value.code == TK_ERROR_INVALID_ARGUMENT and 4 not in forms


def test_verify_pass_of_three_sequences(pair):
    """runs of 3 and 4 rows of two sequences and a single row of a third, at contexts on both sides of every threshold: 8 rows, every form"""
    forms = check_runs(pair, [(0, 510, 3), (2, 1000, 4), (1, 5, 1)], 99)
    assert forms == [0, 2, 4]


def test_verify_pass_refuses_rows_that_are_not_runs(pair):
    gpu, hp, a = pair[0], pair[1], pair[2]
    tok = np.full(3, 9, np.int32)
    for seq, pos, form in [([0, 0, 0], [5, 7, 8], 0),     # a gap
                           ([0, 0, 0], [7, 6, 5], 0),     # descending
                           ([0, 1, 0], [5, 5, 6], 0),     # not contiguous
                           ([0, 0, 0], [5, 6, 7], 3),     # no such form
                           ([0, 0, 3], [5, 6, 7], 0),     # no such sequence
                           ([0, 0, 0], [1098, 1099, 1100], 2)]:
        with pytest.raises(gpu.TkError) as e:
            a.forward_verify(np.array(seq, np.int32), np.array(pos, np.int32), tok, form=form)
        assert e.value.code == TK_ERROR_INVALID_ARGUMENT, (seq, pos, form)


def test_plan_query_names_the_run_form(pair):
    gpu, hp = pair[0], pair[1]
    for nrows in (2, 5, 8, 9):
        kernels = [gpu.attention_plan_verify(nrows, hp.n_head, hp.n_kv_head, hp.head_dim, 4096, top)[0] for top in (5, 127, 128, 4000)]
        assert kernels[0] == 0 and kernels[1] == 0 and kernels[2] in (2, 4) and kernels[3] in (2, 4), (nrows, kernels)
        if nrows > LONG_ATT_MAX_ROWS:
            assert 4 not in kernels
    # a window that cannot reach the long form never names it
    assert gpu.attention_plan_verify(2, hp.n_head, hp.n_kv_head, hp.head_dim, 512, 500)[0] == 2


# ---- 2. the runner ----------------------------------------------------------------------------------------------------------------------------

class Handle:
    def __init__(self, gpu, prefix_cache=False):
        self.gpu, self.loader = gpu, gpu.ModelLoader()
        self.h = self.loader.load(PATH, force_reload=True)  # private: its scheduler and its counters are this test's alone
        if prefix_cache:
            gpu.ModelLoader.set_prefix_cache(self.h, True)
        self.runners = []

    def runner(self, ctx=256, **kw):
        r = self.gpu.LlmRunner(self.h, context_size=ctx, **kw)
        self.runners.append(r)
        return r

    def close(self):
        for r in self.runners:
            r.close()
        self.loader.unload(self.h)
        self.loader.close()


@pytest.fixture
def handle(gpu):
    h = Handle(gpu)
    yield h
    h.close()


def generate(runner, prompt, cap=600, grammar=False):
    """prepare + next_token until it ends (or `cap` calls): (pieces, the ids accepted — what was handed out, then the id the run ended on)"""
    runner.prepare(prompt, use_tool_grammar=grammar)
    pieces = []
    for _ in range(cap):
        p = runner.next_token()
        if p is None or p == "<tool_call>":
            break
        pieces.append(p)
    return pieces, runner.recent_tokens()


def lookup_case(handle, prompt, pred_of, ctx=256, params=(4, 1, 3)):
    """the plain run, then the same runner with lookup on and pred_of(plain ids) as prediction: same tokens, the restatement's counters"""
    r = handle.runner(ctx)
    pieces, ids = generate(r, prompt)
    pred = pred_of(ids)
    r.set_lookup(*params)
    r.set_prediction(pred)
    got_pieces, got_ids = generate(r, prompt)
    assert got_pieces == pieces and got_ids == ids
    stats = r.lookup_stats()
    fed, passes, drafted, accepted = R.schedule(prompt_ids(prompt), ids, pred, params[1], params[2], params[0], ctx, EOS)
    assert stats == (passes, drafted, accepted), (stats, (passes, drafted, accepted))
    return pieces, ids, stats


def test_runner_with_its_own_output_as_prediction(handle):
    pieces, ids, (passes, drafted, accepted) = lookup_case(handle, PROMPT, lambda ids: ids)
    assert len(pieces) >= 24, "the plain greedy run of this prompt and seed is too short: choose another"
    assert accepted >= 4 and 0 < passes < len(pieces)


def test_runner_with_one_wrong_id_in_the_prediction(handle):
    def planted(ids):
        bad = list(ids)
        bad[10] = 3 + (bad[10] - 3 + 1) % 250
        return bad
    pieces, ids, (passes, drafted, accepted) = lookup_case(handle, PROMPT, planted)
    assert accepted >= 4 and accepted < drafted and 0 < passes < len(pieces)


def test_runner_with_a_prediction_that_occurs_nowhere(handle):
    def nowhere(ids):
        seen = set(ids) | set(prompt_ids(PROMPT))
        return [t for t in range(3, 500) if t not in seen][:40]
    lookup_case(handle, PROMPT, nowhere)


def test_runner_drafts_from_a_prompt_that_repeats_a_phrase(handle):
    pieces, ids, (passes, drafted, accepted) = lookup_case(handle, "the cat sat. the cat sat. the cat", lambda ids: [])
    assert drafted > 0  # the last prompt ids occur earlier in the prompt: the first pass already carries drafts


def test_end_of_context(handle):
    """context 64: the NULL arrives after the same token"""
    pieces, ids, stats = lookup_case(handle, PROMPT, lambda ids: ids, ctx=64)
    assert len(pieces) == 64 - len(prompt_ids(PROMPT)) - 1 or ids[-1] == EOS


def test_end_of_context_with_context_shift(handle):
    def run(lookup, pred):
        r = handle.runner(64)
        r.set_context_shift(True, 8)
        if lookup:
            r.set_lookup(4, 1, 3)
            r.set_prediction(pred)
        r.prepare(PROMPT)
        pieces = []
        for _ in range(150):
            p = r.next_token()
            if p is None:
                break
            pieces.append(p)
        return pieces, r.recent_tokens(), r.context_shifts(), r.lookup_stats()
    pieces, ids, shifts, stats = run(False, [])
    assert shifts[0] >= 2 and stats == (0, 0, 0)
    got_pieces, got_ids, got_shifts, got_stats = run(True, ids)
    assert got_pieces == pieces and got_ids == ids and got_shifts == shifts
    assert got_stats[2] >= 4


@pytest.mark.parametrize("why", ["temperature", "penalties", "grammar"])
def test_lookup_is_inactive(handle, why):
    def run(lookup):
        r = handle.runner(256, random_seed=11)
        if why == "temperature":
            r.set_sampling(0.8)
        if why == "penalties":
            r.set_penalties(64, repeat=1.3)
        if lookup:
            r.set_lookup(4, 1, 3)
            r.set_prediction(list(range(3, 200)))  # every 1-gram of the alphabet has a continuation
        pieces, ids = generate(r, PROMPT, cap=80, grammar=why == "grammar")
        return pieces, ids, r.lookup_stats()
    pieces, ids, stats = run(False)
    got_pieces, got_ids, got_stats = run(True)
    assert got_pieces == pieces and got_ids == ids
    assert stats == (0, 0, 0) and got_stats == (0, 0, 0)


def test_lookup_runner_shares_the_model_with_a_plain_runner(handle):
    prompts = ["a", "hi there"]
    solo = [generate(handle.runner(), p, cap=120) for p in prompts]
    ra, rb = handle.runner(), handle.runner()
    ra.set_lookup(4, 1, 3)
    ra.set_prediction(solo[0][1])
    out = [None, None]

    def work(i, r):
        out[i] = generate(r, prompts[i], cap=120)
    threads = [threading.Thread(target=work, args=(i, r)) for i, r in enumerate((ra, rb))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert out[0] == solo[0] and out[1] == solo[1]
    assert ra.lookup_stats()[2] >= 4 and rb.lookup_stats() == (0, 0, 0)


def test_prefix_cache_never_keeps_a_rejected_row(gpu):
    h = Handle(gpu, prefix_cache=True)
    try:
        prompt = "the quick brown fox jumps"
        n_prompt = len(prompt_ids(prompt))
        plain = generate(h.runner(), prompt, cap=60)
        a = h.runner()
        bad = list(plain[1])
        bad[10] = 3 + (bad[10] - 3 + 1) % 250
        a.set_lookup(4, 1, 3)
        a.set_prediction(bad)
        assert generate(a, prompt, cap=60) == plain
        assert a.lookup_stats()[1] > a.lookup_stats()[2]  # drafts were rejected: their rows sit in A's slot beyond its record
        b = h.runner()
        got = generate(b, prompt, cap=60)
        rows, kept, copied = b.last_prompt_rows()
        assert rows == n_prompt and 0 < kept + copied <= n_prompt
        assert got == plain
        # a prompt that continues with the plain run's text past the planted error: whatever B takes from another slot are rows of those very ids
        longer = prompt + b"".join(plain[0][:20]).decode("latin-1")
        got = generate(h.runner(), longer, cap=30)
    finally:
        h.close()
    h = Handle(gpu)  # the same prompt on a model without the cache
    try:
        assert got == generate(h.runner(), longer, cap=30)
    finally:
        h.close()


def test_arguments(handle):
    gpu = handle.gpu
    r = handle.runner()
    pieces, ids = generate(r, PROMPT, cap=60)
    r.set_lookup(4, 1, 3)
    r.set_prediction(ids)
    for bad in [(16, 1, 3), (-1, 1, 3), (4, 0, 3), (4, 3, 2), (4, 1, 9)]:
        with pytest.raises(gpu.TkError) as e:
            r.set_lookup(*bad)
        assert e.value.code == TK_ERROR_INVALID_ARGUMENT, bad
    for bad in [[5, 512], [-1], [7] * 4097]:
        with pytest.raises(gpu.TkError) as e:
            r.set_prediction(bad)
        assert e.value.code == TK_ERROR_INVALID_ARGUMENT, bad[:2]
    # the previous setting and prediction are kept: the run drafts from them
    assert generate(r, PROMPT, cap=60) == (pieces, ids)
    passes, drafted, accepted = r.lookup_stats()
    assert accepted >= 4
    r.set_prediction([])
    r.set_lookup(0)
    assert generate(r, PROMPT, cap=60) == (pieces, ids) and r.lookup_stats() == (0, 0, 0)
