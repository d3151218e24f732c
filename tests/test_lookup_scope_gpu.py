"""GPU: lookup decoding for runners that sample, are masked, adjusted or ask for log-probabilities (csrc/llm/tk_lookup_scope.h).

1. The verify pass with tables on a bare session: LlmSession.forward_rows over several positions of a sequence — every row with its own mask,
   (seed, counter + i), window and n_top — against one forward_rows per row on a second session: logits, picks, records and the appended K / V rows
   of every layer bit for bit, and the attention form the pass took (last_pass_key) against the plan query.
2. The feature behind tk_llm_runner_* (set_lookup_scope) against the same runner with lookup off, with the schedule restated in
   tests/lookup_scope_ref.py.

Synthetic models tokenise bytes: ids = [1] + [3 + b ...]; id 2 ends a generation."""
import threading

import numpy as np
import pytest

import lookup_scope_ref as R

pytestmark = pytest.mark.gpu

TK_ERROR_INVALID_ARGUMENT = 1001
EOS = 2
SEED = 4
PATH = "synthetic://tiny?seed=%d" % SEED
PROMPT = "a"
MAX_SEQ, MAX_CTX = 3, 1100
P0S = [5, 127, 505, 767]
RUNS = [2, 5, 8, 9]
RUN_FORM = 4  # the attention number of the run form in tk_pass_form_key: 5 + 4 * attention + 2 * adjusted + with records
LOOKUP = (4, 1, 3)


def prompt_ids(p):
    return [1] + [3 + b for b in p.encode()]


# ---- 1. the verify pass with tables against one-row passes --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pair(gpu):
    model = gpu.LlmModel(gpu.TINY()).fill_synthetic(SEED)
    hp = model.hparams
    a, b = gpu.LlmSession(model, MAX_SEQ, MAX_CTX), gpu.LlmSession(model, MAX_SEQ, MAX_CTX)
    rng = np.random.default_rng(78)
    shape = (hp.n_layer, MAX_SEQ, 2, MAX_CTX, hp.n_kv_head, hp.head_dim)
    rows = (rng.standard_normal(shape, dtype=np.float32) * np.array([0.6, 1.0], np.float32).reshape(1, 1, 2, 1, 1, 1)).astype(np.float16).view(np.uint16)
    stale = (rng.standard_normal(shape, dtype=np.float32) * 0.5).astype(np.float16).view(np.uint16)
    yield gpu, hp, a, b, rows, stale
    a.close()
    b.close()
    model.close()


def fill(sess, hp, rows, stale, seq, p0, n):
    for l in range(hp.n_layer):
        if p0 > 0:
            sess.kv_write(l, seq, 0, np.ascontiguousarray(rows[l, seq, 0, :p0]), np.ascontiguousarray(rows[l, seq, 1, :p0]))
        sess.kv_write(l, seq, p0, np.ascontiguousarray(stale[l, seq, 0, p0:p0 + n]), np.ascontiguousarray(stale[l, seq, 1, p0:p0 + n]))


def new_rows(sess, hp, runs):
    return [sess.kv_read(l, s, p0, n) for l in range(hp.n_layer) for (s, p0, n) in runs]


def row_tables(hp, rng, n, tabled):
    """per row: a mask of its own, the chain at counter + i, a window and bias of its own, an n_top of its own; None / greedy / -1 where not tabled"""
    words = (hp.vocab + 31) // 32
    masks, sampling, adjust, n_top = [], [], [], []
    for i in range(n):
        if not tabled[i]:
            masks.append(None)
            sampling.append((0.0, 40, 0.95, 0.05, 0, 0))
            adjust.append(None)
            n_top.append(-1)
            continue
        m = rng.integers(0, 2 ** 32, words, dtype=np.uint64).astype(np.uint32)
        m[rng.integers(0, words)] |= np.uint32(1 << int(rng.integers(0, 32)))
        masks.append(m)
        sampling.append((0.8, 40, 0.95, 0.05, 11, 100 + i))
        adjust.append(dict(repeat=1.3, freq=0.1 * (i % 3), present=0.05 * (i % 2), recent=rng.integers(3, hp.vocab, 1 + 3 * i).tolist(),
                           bias_ids=[9 + i, 40 + 2 * i], bias=[2.5, -3.0 - i]))
        n_top.append((3 * i + 1) % 21)
    return masks, sampling, adjust, n_top


def check_runs(pair, runs, seed, tabled_of=lambda r: True):
    """runs = [(sequence, first position, rows)]: ONE forward_rows on session A, one forward_rows per row on session B.  Returns A's pass key"""
    gpu, hp, a, b, rows, stale = pair
    rng = np.random.default_rng(seed)
    seq = np.concatenate([np.full(n, s, np.int32) for s, p0, n in runs])
    pos = np.concatenate([np.arange(p0, p0 + n, dtype=np.int32) for s, p0, n in runs])
    n = len(seq)
    tok = rng.integers(3, hp.vocab, n).astype(np.int32)
    masks, sampling, adjust, n_top = row_tables(hp, rng, n, [tabled_of(r) for r in range(n)])
    for s, p0, k in runs:
        fill(a, hp, rows, stale, s, p0, k)
        fill(b, hp, rows, stale, s, p0, k)
    want_logits = np.empty((n, hp.vocab), np.float32)
    want_picks = np.empty(n, np.int32)
    want_recs = np.zeros(n, gpu.TOKEN_LOGPROB_DTYPE)
    for r in range(n):
        lg, pk, rec = b.forward_rows(seq[r:r + 1], pos[r:r + 1], tok[r:r + 1], masks[r:r + 1], sampling[r:r + 1], adjust[r:r + 1], n_top[r:r + 1])
        want_logits[r], want_picks[r], want_recs[r] = lg[0], pk[0], rec[0]
        assert (b.last_pass_key - 5) // 4 in (0, 1)  # a one-row pass ropes inside its attention
    want_rows = new_rows(b, hp, runs)
    got_logits, got_picks, got_recs = a.forward_rows(seq, pos, tok, masks, sampling, adjust, n_top)
    key = a.last_pass_key
    assert np.array_equal(got_logits.view(np.uint32), want_logits.view(np.uint32)), (runs, np.abs(got_logits - want_logits).max())
    assert np.array_equal(got_picks, want_picks), runs
    assert got_recs.tobytes() == want_recs.tobytes(), runs
    for (gk, gv), (wk, wv) in zip(new_rows(a, hp, runs), want_rows):
        assert np.array_equal(gk, wk) and np.array_equal(gv, wv), runs
    # the tables reached the rows: a masked row's pick is inside its mask, a row that asked has its record
    for r in range(n):
        if masks[r] is not None:
            assert masks[r][got_picks[r] >> 5] >> (got_picks[r] & 31) & 1, (runs, r)
        if n_top[r] >= 0:
            assert got_recs[r]["n_top"] == n_top[r], (runs, r)
    return key


@pytest.mark.parametrize("n", RUNS)
@pytest.mark.parametrize("p0", P0S)
def test_tabled_run_equals_one_row_passes(pair, p0, n):
    """n rows of one sequence from position p0, every row with tables of its own.  The pass takes the run form exactly where the plan query names
    kernel 4 for a verify pass of these rows; its key carries the adjustment and the records"""
    gpu, hp = pair[0], pair[1]
    key = check_runs(pair, [(1, p0, n)], 1000 * p0 + n)
    plan = gpu.attention_plan_verify(n, hp.n_head, hp.n_kv_head, hp.head_dim, MAX_CTX, p0 + n - 1)[0]
    assert key >= 5 and (key - 5) % 4 == 3, key
    assert ((key - 5) // 4 == RUN_FORM) == (plan == 4), (key, plan)
    assert (plan == 4) == (n <= 8 and p0 + n - 1 >= 256), (plan, p0, n)  # both sides of the threshold are among the cases


def test_three_sequences_with_tables_on_some_rows(pair):
    """runs of 3 and 4 rows of two sequences and a single row of a third, tables on every other row: the rows without tables sample greedily,
    unmasked, unadjusted, without a record"""
    key = check_runs(pair, [(0, 510, 3), (2, 1000, 4), (1, 5, 1)], 99, tabled_of=lambda r: r % 2 == 0)
    assert (key - 5) // 4 == RUN_FORM


def test_a_pass_without_repeats_keeps_its_form(pair):
    """every sequence once: forward_rows is the pass forward() always ran, whatever the context"""
    key = check_runs(pair, [(0, 900, 1), (1, 300, 1), (2, 5, 1)], 5)
    assert (key - 5) // 4 in (0, 1)


def test_forward_rows_refuses(pair):
    gpu, hp, a = pair[0], pair[1], pair[2]
    seq, pos, tok = np.zeros(3, np.int32), np.arange(5, 8, dtype=np.int32), np.full(3, 9, np.int32)
    key = a.last_pass_key
    ok_samp = [(0.8, 40, 0.95, 0.05, 1, 0)] * 3
    cases = [dict(seq=[0, 0, 3]), dict(pos=[5, 6, MAX_CTX]), dict(tok=[9, 9, hp.vocab]), dict(n_top=[0, 21, 0]), dict(n_top=[0, -2, 0]),
             dict(sampling=[(0.8, 65, 0.95, 0.05, 1, 0)] * 3), dict(sampling=ok_samp[:2] + [(0.8, 40, 0.0, 0.05, 1, 0)]),
             dict(adjust=[None, dict(repeat=1.3, recent=[hp.vocab]), None]), dict(adjust=[None, None, dict(repeat=1.3, recent=list(range(3, 260)))])]
    for kw in cases:
        args = dict(seq=seq, pos=pos, tok=tok)
        args.update(kw)
        with pytest.raises(gpu.TkError) as e:
            a.forward_rows(**args)
        assert e.value.code == TK_ERROR_INVALID_ARGUMENT, kw
    assert a.last_pass_key == key  # nothing ran
    with pytest.raises(ValueError):
        a.forward_rows(seq, pos, tok, masks=[None, None])
    with pytest.raises(ValueError):
        a.forward_rows(seq, pos, tok, masks=[None, None, np.zeros(3, np.uint32)])


# ---- 2. the runner ------------------------------------------------------------------------------------------------------------------------------

class Handle:
    def __init__(self, gpu):
        self.gpu, self.loader = gpu, gpu.ModelLoader()
        self.h = self.loader.load(PATH, force_reload=True)
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


MODES = {
    "plain": dict(),
    "temperature": dict(sampled=True),
    "grammar": dict(grammar=True),
    "penalties": dict(adjusted=True),
    "logprobs": dict(logprobs=True),
    "all": dict(sampled=True, grammar=True, adjusted=True, logprobs=True),
}


CLOSING_BRACE = 3 + ord("}")


def configure(handle, mode, ctx=256):
    m = MODES[mode]
    r = handle.runner(ctx, random_seed=11)
    if m.get("sampled"):
        r.set_sampling(0.8)
    if m.get("adjusted"):
        r.set_penalties(64, repeat=1.3)
    if m.get("logprobs"):
        r.set_logprobs(5)
    if mode == "all":
        # sampled under the grammar this model closes its call after two or three ids; a bias against the closing brace (part of "adjusted") keeps
        # the call open, so that the run is long enough to draft from
        r.set_logit_bias([CLOSING_BRACE], [-3.0])
    return r


def generate(r, prompt, mode, cap=300, stop_when=None):
    """prepare + next_token until it ends (or `cap` calls).  Returns everything a host can see: the pieces, the ids accepted, the record of every id
    (read before the call that hands the id out), the tool-call text, how the run ended and after how many calls.  stop_when(r): asked after every
    call, True ends the run early"""
    m = MODES[mode]
    r.prepare(prompt, use_tool_grammar=bool(m.get("grammar")))
    pieces, recs, end, calls = [], [], "cap", 0
    for _ in range(cap):
        if m.get("logprobs"):
            recs.append(r.last_logprobs())
        p = r.next_token()
        calls += 1
        if p is None or p == "<tool_call>":
            end = p
            break
        pieces.append(p)
        if stop_when is not None and stop_when(r):
            end = "stopped"
            break
    return dict(pieces=pieces, ids=r.recent_tokens(), recs=recs, text=r.tool_call_text(), end=end, calls=calls)


def scope_case(handle, mode, pred_of, prompt=PROMPT, ctx=256, cap=300, scope=None):
    """the run with lookup off, then the same configuration with lookup on inside its scope and pred_of(plain ids) as prediction: everything a host
    sees is equal, and the counters are the restated schedule's"""
    plain = generate(configure(handle, mode, ctx), prompt, mode, cap)
    r = configure(handle, mode, ctx)
    r.set_lookup(*LOOKUP)
    r.set_lookup_scope(**(MODES[mode] if scope is None else scope))
    pred = pred_of(plain["ids"])
    r.set_prediction(pred)
    got = generate(r, prompt, mode, cap)
    assert got == plain, (mode, [k for k in plain if got[k] != plain[k]])
    stats = r.lookup_stats()
    return plain, pred, stats


def restated(plain, pred, prompt, ctx, mode):
    """the counters of the restated schedule for a run that ended of itself: its accepted ids are every id it sampled, the one it ended on last"""
    assert plain["end"] != "cap"
    stream = list(plain["ids"])
    return R.schedule(prompt_ids(prompt), stream, pred, LOOKUP[1], LOOKUP[2], LOOKUP[0], ctx, EOS, grammar=bool(MODES[mode].get("grammar")))[1:]


@pytest.mark.parametrize("mode", ["temperature", "grammar", "penalties", "logprobs", "all"])
def test_runner_inside_its_scope_with_its_own_output_as_prediction(handle, mode):
    plain, pred, stats = scope_case(handle, mode, lambda ids: ids)
    assert len(plain["pieces"]) >= 24, "the plain run of this prompt, seed and mode is too short: choose another"
    assert stats == restated(plain, pred, PROMPT, 256, mode), (stats, restated(plain, pred, PROMPT, 256, mode))
    assert stats[2] >= 4 and 0 < stats[0] < len(plain["pieces"]), stats
    if MODES[mode].get("logprobs"):
        assert len(plain["recs"]) == plain["calls"] and all(len(alts) == 5 for _, alts in plain["recs"])


@pytest.mark.parametrize("mode", ["temperature", "all"])
def test_schedule_of_a_run_that_ends_at_the_context(handle, mode):
    """context 64: the run ends of itself, at the same token, and the counters are the restated schedule's"""
    plain, pred, stats = scope_case(handle, mode, lambda ids: ids, ctx=64)
    if plain["end"] is None and plain["ids"][-1] != EOS:
        assert len(plain["pieces"]) == 64 - len(prompt_ids(PROMPT)) - 1
    assert stats == restated(plain, pred, PROMPT, 64, mode), (stats, restated(plain, pred, PROMPT, 64, mode))
    assert stats[2] >= 4


def test_context_shift_sampled(handle):
    def run(lookup, pred):
        r = configure(handle, "temperature", 64)
        r.set_context_shift(True, 8)
        if lookup:
            r.set_lookup(*LOOKUP)
            r.set_lookup_scope(sampled=True)
            r.set_prediction(pred)
        out = generate(r, PROMPT, "temperature", cap=150)
        return out, r.context_shifts(), r.lookup_stats()
    plain, shifts, stats = run(False, [])
    assert shifts[0] >= 2 and stats == (0, 0, 0)
    got, got_shifts, got_stats = run(True, plain["ids"])
    assert got == plain and got_shifts == shifts
    assert got_stats[2] >= 4


@pytest.mark.parametrize("mode", ["temperature", "all"])
def test_one_wrong_id_in_the_prediction(handle, mode):
    def planted(ids):
        bad = list(ids)
        if mode == "all":
            # under the grammar a wrong id must still be one the mask allows, or the draft is cut and never fed: another white space, at a place the
            # first pass drafts (the 1-gram of the first sampled id matches the prediction at its start)
            tab, newline = 3 + ord("\t"), 3 + ord("\n")
            assert bad[1] in (tab, newline, 3 + ord(" ")), "the second id of this run is no white space: choose another place"
            bad[1] = tab if bad[1] != tab else newline
        else:
            bad[10] = 3 + (bad[10] - 3 + 1) % 250
        return bad
    plain, pred, (passes, drafted, accepted) = scope_case(handle, mode, planted)
    assert accepted < drafted and passes > 0 and accepted >= 4


@pytest.mark.parametrize("mode", ["temperature", "all"])
def test_a_prediction_that_matches_nowhere(handle, mode):
    def nowhere(ids):
        seen = set(ids) | set(prompt_ids(PROMPT))
        return [t for t in range(3, 500) if t not in seen][:40]
    scope_case(handle, mode, nowhere)


@pytest.mark.parametrize("mode,scope", [("temperature", dict(grammar=True, adjusted=True, logprobs=True)), ("grammar", dict(sampled=True, adjusted=True, logprobs=True)),
                                        ("penalties", dict(sampled=True, grammar=True, logprobs=True)), ("logprobs", dict(sampled=True, grammar=True, adjusted=True)),
                                        ("all", dict(sampled=True, grammar=True, adjusted=True))])
def test_a_missing_scope_bit_keeps_the_runner_inactive(handle, mode, scope):
    plain, pred, stats = scope_case(handle, mode, lambda ids: list(range(3, 200)), scope=scope, cap=80)
    assert stats == (0, 0, 0)


def test_scope_arguments(handle):
    gpu = handle.gpu
    r = handle.runner()
    assert r.lookup_scope() == 0
    r.set_lookup_scope(sampled=True, logprobs=True)
    assert r.lookup_scope() == 9
    for bad in (16, 17, 1 << 31):
        with pytest.raises(gpu.TkError) as e:
            r.set_lookup_scope_bits(bad)
        assert e.value.code == TK_ERROR_INVALID_ARGUMENT
    assert r.lookup_scope() == 9
    r.set_lookup_scope()
    assert r.lookup_scope() == 0


# a masked run of this model repeats white space until its context ends; a frequency penalty lets the closing brace win after a while.  Per mode the
# (seed, penalty) at which the plain run completes a call that is long enough to draft from
TOOL_RUNS = {"grammar": (11, 0.05), "all": (12, 0.1)}


def tool_runner(handle, lookup, pred, mode):
    seed, freq = TOOL_RUNS[mode]
    r = handle.runner(256, random_seed=seed)
    if MODES[mode].get("sampled"):
        r.set_sampling(0.8)
    if MODES[mode].get("logprobs"):
        r.set_logprobs(5)
    r.set_penalties(64, repeat=1.0, freq=freq)
    if lookup:
        r.set_lookup(*LOOKUP)
        r.set_lookup_scope(sampled=True, grammar=True, adjusted=True, logprobs=True)
        r.set_prediction(pred)
    return r


def tool_stream(r, mode, cap, stop_when=None, answer_anyway=False):
    """a grammar run, the tool response — when the call has completed, or wherever the run stands with answer_anyway —, then what follows it"""
    first = generate(r, "call the clock", mode, cap, stop_when=stop_when)
    if first["end"] != "<tool_call>" and not answer_anyway:
        return first, None
    r.add_tool_response("clock", "12:00")
    pieces, recs = [], []
    for _ in range(30):
        if MODES[mode].get("logprobs"):
            recs.append(r.last_logprobs())
        p = r.next_token()
        if p is None or p == "<tool_call>":
            break
        pieces.append(p)
    return first, dict(pieces=pieces, ids=r.recent_tokens(), recs=recs, text=r.tool_call_text())


@pytest.mark.parametrize("mode", ["grammar", "all"])
def test_tool_call_then_response_then_free_text(handle, mode):
    plain_call, plain_rest = tool_stream(tool_runner(handle, False, [], mode), mode, 250)
    assert plain_call["end"] == "<tool_call>", "the plain run does not complete its tool call: choose another bias or prompt"
    assert R.ToolCallGrammar.status(plain_call["text"]) == "complete"
    r = tool_runner(handle, True, plain_call["ids"], mode)
    got_call, got_rest = tool_stream(r, mode, 250)
    assert got_call == plain_call and got_rest == plain_rest
    assert len(plain_rest["pieces"]) > 0
    assert r.lookup_stats()[2] >= 4


@pytest.mark.parametrize("mode", ["grammar", "all"])
def test_tool_response_while_ids_are_queued(handle, mode):
    """the host answers in the middle of the call, right after a verify pass that left ids queued: they are dropped, the sampling counter and their
    records with them, and the stream is the one of the runner with lookup off that is answered after the same number of calls"""
    probe = generate(tool_runner(handle, False, [], mode), "call the clock", mode, 250)
    r = tool_runner(handle, True, probe["ids"], mode)
    seen = [0]

    def queued_now(runner):  # the last call ran a verify pass that accepted drafts: that many ids are queued
        acc = runner.lookup_stats()[2]
        grew, seen[0] = acc > seen[0], acc
        return grew
    got_call, got_rest = tool_stream(r, mode, 250, stop_when=queued_now, answer_anyway=True)
    assert got_call["end"] == "stopped", "no verify pass of this run accepted a draft: choose another bias or prompt"
    k = got_call["calls"]
    plain_call, plain_rest = tool_stream(tool_runner(handle, False, [], mode), mode, k, answer_anyway=True)
    assert plain_call["calls"] == k and plain_call["end"] == "cap"
    got_call["end"] = "cap"
    assert got_call == plain_call and got_rest == plain_rest
    assert len(plain_rest["pieces"]) > 0


def test_verify_passes_beyond_position_256(handle):
    """a prompt of 300 ids in a window that reaches the long attention: the runner's verify passes take the run form (part 1 checks the form)"""
    prompt = ("the cat sat on the mat. " * 13)[:300]
    assert len(prompt_ids(prompt)) > 256
    for mode in ("temperature", "all"):
        plain, pred, stats = scope_case(handle, mode, lambda ids: ids, prompt=prompt, ctx=1100, cap=60)
        assert stats[2] >= 4, (mode, stats)


def test_scoped_lookup_runner_shares_the_model_with_a_plain_runner(handle):
    prompts = ["a", "hi there"]
    solo = [generate(configure(handle, "temperature"), prompts[0], "temperature", cap=100), generate(handle.runner(), prompts[1], "plain", cap=100)]
    ra, rb = configure(handle, "temperature"), handle.runner()
    ra.set_lookup(*LOOKUP)
    ra.set_lookup_scope(sampled=True)
    ra.set_prediction(solo[0]["ids"])
    out = [None, None]

    def work(i, r):
        out[i] = generate(r, prompts[i], "temperature" if i == 0 else "plain", cap=100)
    threads = [threading.Thread(target=work, args=(i, r)) for i, r in enumerate((ra, rb))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert out[0] == solo[0] and out[1] == solo[1]
    assert ra.lookup_stats()[2] >= 4 and rb.lookup_stats() == (0, 0, 0)
