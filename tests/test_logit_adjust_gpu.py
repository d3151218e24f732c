"""GPU: logit bias and repetition penalties on the device — k_logit_adjust alone (tk_mi355x_logit_adjust_probe), inside a pass
(tk_mi355x_llm_forward_adjusted) and behind tk_llm_runner_*.  Expected values: the float32 NumPy restatement tests/logit_adjust_ref.py on the
raw logits (the probe's input, a plain forward's output, the oracle's logits), compared as bit patterns; ids are the first index of the
maximum of the adjusted row, or the oracle's orc_sample_row on it."""
import ctypes as C
import threading

import numpy as np
import pytest

import logit_adjust_cases as LC
import logit_adjust_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def oracle_cfg_from(hp, max_ctx, max_seq):
    return O.LlmConfig(n_layer=hp.n_layer, d_model=hp.d_model, n_head=hp.n_head, n_kv_head=hp.n_kv_head, head_dim=hp.head_dim,
                       d_ff=hp.d_ff, vocab=hp.vocab, max_ctx=max_ctx, max_seq=max_seq, rms_eps=hp.rms_eps, rope_theta=hp.rope_theta,
                       ks_qkv=hp.ks_qkv, ks_o=hp.ks_o, ks_gateup=hp.ks_gateup, ks_down=hp.ks_down, ks_out=hp.ks_out)


@pytest.mark.parametrize("rows", [1, 3, 256])
@pytest.mark.parametrize("cols", [1, 33, 1000, 32000, 65537])
def test_kernel_equals_the_numpy_reference_bit_for_bit(gpu, cols, rows):
    for c in LC.cases(cols, rows):
        got = gpu.logit_adjust_probe(c["logits"], rows, cols, c["specs"], device=0)
        want = R.adjust(c["logits"], c["specs"])
        assert np.array_equal(bits(got), bits(want)), (c["name"], np.argwhere(bits(got) != bits(want))[:4].tolist())
        host = gpu.logit_adjust_probe(c["logits"], rows, cols, c["specs"], device=-1)
        assert np.array_equal(bits(host), bits(got)), c["name"]


def test_kernel_refuses_before_it_launches(gpu):
    lg = np.ones((2, 33), np.float32)
    out = lg.copy()
    with pytest.raises(gpu.TkError) as e:
        gpu.logit_adjust_probe_into(out, 2, 33, [dict(bias_ids=[1], bias=[1.0]), dict(repeat=1.1, recent=[33])], device=0)
    assert e.value.code == 1001 and np.array_equal(out, lg)


SAMP = (0.8, 40, 0.95, 0.05, 1234, 7)
GREEDY = (0.0, 40, 0.95, 0.05, 0, 0)


@pytest.mark.parametrize("distinct", [True, False])
def test_forward_adjusted_in_one_pass(gpu, distinct):
    """rows of several sequences in one pass, neutral, adjusted and one sampled; distinct: every sequence once (the decode graphs' sibling), else
    two positions of one sequence (the several-positions graphs' sibling)"""
    model = gpu.LlmModel(gpu.TINY()).fill_synthetic(4)
    vocab = model.hparams.vocab
    rng = np.random.default_rng(5)

    def start(sess):  # three prompt tokens per sequence
        seq = np.repeat(np.arange(4, dtype=np.int32), 3)
        pos = np.tile(np.arange(3, dtype=np.int32), 4)
        sess.forward(seq, pos, np.random.default_rng(6).integers(3, vocab, 12).astype(np.int32), want_logits=False)

    sess = gpu.LlmSession(model, 4, 32)
    start(sess)
    seq = np.array([0, 1, 2, 3] if distinct else [0, 0, 1, 2], np.int32)
    pos = np.array([3, 3, 3, 3] if distinct else [3, 4, 3, 3], np.int32)
    tok = rng.integers(3, vocab, 4).astype(np.int32)
    raw, plain_ids = sess.forward(seq, pos, tok)
    top = np.argsort(-raw, axis=1, kind="stable")
    specs = [None,
             dict(repeat=1.3, freq=0.5, present=1.0e4, recent=[int(top[1, 0]), int(top[1, 1]), int(top[1, 0]), 7]),
             dict(repeat=1.0, freq=0.0, present=0.0, recent=[int(top[2, 0])] * 3),        # neutral: a window, penalties off
             dict(repeat=1.1, recent=top[3, :5].tolist(), bias_ids=[int(top[3, 0]), int(top[3, 6]), int(top[3, 100])], bias=[-np.inf, 4.0, -1.5])]
    sampling = [GREEDY, GREEDY, GREEDY, SAMP]
    got, ids = sess.forward_adjusted(seq, pos, tok, specs, sampling=sampling)
    want = R.adjust(raw, specs)
    assert np.array_equal(bits(got), bits(want))
    assert not np.array_equal(bits(want[1]), bits(raw[1])) and not np.array_equal(bits(want[3]), bits(raw[3]))
    assert ids[:3].tolist() == np.argmax(want[:3], axis=1).tolist()
    assert int(ids[3]) == O.sample_row(want[3], *SAMP) and int(ids[3]) != int(top[3, 0])
    assert int(ids[1]) not in (int(top[1, 0]), int(top[1, 1]))             # a presence penalty far above any logit moved the pick
    assert ids[[0, 2]].tolist() == plain_ids[[0, 2]].tolist()              # neutral rows: the plain pass's ids
    # sampling = NULL: every row greedy
    got2, ids2 = sess.forward_adjusted(seq, pos, tok, specs)
    assert np.array_equal(bits(got2), bits(want)) and ids2.tolist() == np.argmax(want, axis=1).tolist()
    # a pass without any adjustment afterwards: the raw logits and the plain ids again, through either entry
    raw2, ids3 = sess.forward(seq, pos, tok)
    assert np.array_equal(bits(raw2), bits(raw)) and np.array_equal(ids3, plain_ids)
    raw3, ids4 = sess.forward_adjusted(seq, pos, tok, [None, specs[2], None, None])
    assert np.array_equal(bits(raw3), bits(raw)) and np.array_equal(ids4, plain_ids)
    # refused whole: nothing of the pass runs
    with pytest.raises(gpu.TkError) as e:
        sess.forward_adjusted(seq, pos, tok, [None, None, None, dict(repeat=1.1, recent=[vocab])])
    assert e.value.code == 1001
    # the descriptors do not leak: adjusted pass, then a plain forward + decode() gives what a fresh session gives
    sess.forward_adjusted(seq, pos, tok, specs)
    dseq, dpos = np.arange(4, dtype=np.int32), np.array([4, 4, 4, 4] if distinct else [5, 4, 4, 3], np.int32)  # each sequence's next position
    dtok = rng.integers(3, vocab, 4).astype(np.int32)

    def tail(s):
        _, first = s.forward(dseq, dpos, dtok, want_logits=False)
        toks, _ = s.decode(4, 6)
        return first.tolist(), np.asarray(toks).tolist()

    used = tail(sess)
    fresh = gpu.LlmSession(model, 4, 32)
    start(fresh)
    fresh.forward(seq, pos, tok, want_logits=False)
    assert tail(fresh) == used
    sess.close(); fresh.close(); model.close()


# ---- runners ------------------------------------------------------------------------------------------------------------------------------
PROMPT, SEED, NCTX, NTOK = "hi", 4, 96, 32
PEN = dict(last_n=8, repeat=1.3, freq=0.5, present=0.25)


def prompt_ids(p):
    return [1] + [3 + b for b in p.encode()]


def generate(runner, prompt, n=NTOK, grammar=False):
    """n calls of generate_next_token; the ids are the ones the runner accepted"""
    runner.prepare(prompt, use_tool_grammar=grammar)
    for _ in range(n):
        if runner.next_token() in (None, "<tool_call>"):
            break
    return runner.recent_tokens()


class Model:
    def __init__(self, gpu, seed=SEED):
        self.gpu = gpu
        self.loader = gpu.ModelLoader()
        self.h = self.loader.load("synthetic://tiny?seed=%d" % seed, force_reload=True)  # private: its scheduler counters start at zero
        hp = gpu.LlmHParams()
        gpu.lib().tk_mi355x_llm_model_get_hparams(self.h, C.byref(hp))
        self.orc = O.OracleLlm(oracle_cfg_from(hp, NCTX, 1), seed=seed)

    def runner(self):
        return self.gpu.LlmRunner(self.h, context_size=NCTX, random_seed=11)

    def close(self):
        self.loader.unload(self.h)
        self.loader.close()
        self.orc.close()

    def reconstruct(self, prompt, n, last_n=0, repeat=1.0, freq=0.0, present=0.0, bias_ids=(), bias=(), bias_from=0):
        """the oracle's logits, the NumPy reference and the window rule: the id sampled at step i sees the ids accepted before it (the last last_n
        of them); it is accepted by the i-th generate_next_token, EOS included; the bias list applies from step bias_from on"""
        self.orc.reset()
        ids = prompt_ids(prompt)
        lg = self.orc.forward([0] * len(ids), list(range(len(ids))), ids)[0][-1]
        pos, window, rows = len(ids), [], []
        for i in range(n):
            on = i >= bias_from
            spec = dict(repeat=repeat, freq=freq, present=present, recent=window[-last_n:] if last_n else [],
                        bias_ids=list(bias_ids) if on else [], bias=list(bias) if on else [])
            adj = R.adjust_row(lg, spec)
            cur = int(np.argmax(adj))
            rows.append(adj)
            window.append(cur)
            if cur == 2 or pos + 1 >= NCTX:
                break
            lg = self.orc.forward([0], [pos], [cur])[0][0]
            pos += 1
        return window, rows


def no_repeat_within(ids, span):
    return all(ids[i] not in ids[max(0, i - span + 1):i] for i in range(len(ids)))


def test_a_neutral_penalties_change_nothing_and_still_run_ahead(gpu):
    m = Model(gpu)
    plain = m.runner()
    want = generate(plain, PROMPT)
    assert want == m.reconstruct(PROMPT, NTOK)[0] and len(want) == NTOK
    r = m.runner()
    r.set_penalties(64, 1.0, 0.0, 0.0)
    w0 = gpu.ModelLoader.run_ahead_wasted(m.h)
    for _ in range(3):  # abandoned in the middle of a generation: the row that ran ahead is wasted — there was one
        assert generate(r, PROMPT, 5) == want[:5]
    assert gpu.ModelLoader.run_ahead_wasted(m.h) > w0
    assert generate(r, PROMPT) == want
    # a penalised runner does not run ahead: nothing of it is ever wasted (a new runner: `r` and `plain` still hold the row that ran ahead of
    # their last token, which counts as wasted only when they go)
    r2 = m.runner()
    r2.set_penalties(**PEN)
    w1 = gpu.ModelLoader.run_ahead_wasted(m.h)
    for _ in range(3):
        assert len(generate(r2, PROMPT, 5)) == 5
    assert gpu.ModelLoader.run_ahead_wasted(m.h) == w1
    r2.set_penalties(0)  # off again: the plain ids
    assert generate(r2, PROMPT) == want
    plain.close(); r.close(); r2.close(); m.close()


def test_b_c_penalised_runner_equals_the_reconstruction_alone_and_in_company(gpu):
    m = Model(gpu)
    want, _ = m.reconstruct(PROMPT, NTOK, **PEN)
    plain_want, _ = m.reconstruct(PROMPT, NTOK)
    assert want != plain_want
    r = m.runner()
    r.set_penalties(**PEN)
    alone = generate(r, PROMPT)
    assert alone == want
    # (c) three other runners decode on the same model from other threads: one plain, one sampled, one under the tool grammar
    others = [m.runner() for _ in range(3)]
    others[1].set_sampling(0.8)
    out, errs = {}, []

    def work(name, runner, prompt, grammar):
        try:
            for rnd in range(2):
                out[(name, rnd)] = generate(runner, prompt, grammar=grammar)
        except Exception as e:  # noqa: BLE001
            errs.append((name, repr(e)))

    th = [threading.Thread(target=work, args=("pen", r, PROMPT, False)), threading.Thread(target=work, args=("plain", others[0], PROMPT, False)),
          threading.Thread(target=work, args=("samp", others[1], "go", False)), threading.Thread(target=work, args=("tool", others[2], "call", True))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    assert out[("pen", 0)] == want and out[("pen", 1)] == want
    assert out[("plain", 0)] == plain_want and out[("plain", 1)] == plain_want
    assert len(out[("samp", 0)]) > 0 and len(out[("tool", 0)]) > 0
    _, _, widest = gpu.ModelLoader.batch_stats(m.h)
    print("widest pass with four runners:", widest)
    for x in others + [r]:
        x.close()
    m.close()


def test_d_a_huge_presence_penalty_forbids_repeats_inside_the_window(gpu):
    m = Model(gpu)
    plain_want, _ = m.reconstruct(PROMPT, NTOK)
    assert not no_repeat_within(plain_want, 9)  # the unpenalised greedy ids of this prompt and seed do repeat (chosen on the CPU for that)
    r = m.runner()
    r.set_penalties(8, 1.0, 0.0, 1e30)
    got = generate(r, PROMPT)
    assert len(got) == NTOK or got[-1] == 2
    assert no_repeat_within(got, 9)
    assert got == m.reconstruct(PROMPT, NTOK, last_n=8, present=1e30)[0]
    r.close(); m.close()


def test_e_a_banned_token_changes_that_token_and_nothing_before_it(gpu):
    L = gpu.lib()
    m = Model(gpu)
    plain_want, _ = m.reconstruct(PROMPT, NTOK)
    # banned from the start: the first token changes
    r = m.runner()
    r.set_logit_bias([plain_want[0]], [-np.inf])
    got = generate(r, PROMPT, 8)
    want, rows = m.reconstruct(PROMPT, 8, bias_ids=[plain_want[0]], bias=[-np.inf])
    assert got == want and got[0] != plain_want[0] and plain_want[0] not in got
    # banned in the middle of a generation: the pending id was sampled before the ban, the next one is the first to see it
    k = next(i for i in range(2, NTOK) if plain_want[i] != plain_want[i - 1])  # ban plain_want[k] after k - 1 calls: ids 0 .. k - 1 stand
    r.set_logit_bias([], [])
    r.prepare(PROMPT)
    for _ in range(k - 1):
        assert r.next_token() is not None
    r.set_logit_bias([plain_want[k]], [-np.inf])
    for _ in range(4):
        r.next_token()
    got = r.recent_tokens()
    want, _ = m.reconstruct(PROMPT, k + 3, bias_ids=[plain_want[k]], bias=[-np.inf], bias_from=k)
    assert got == want and got[:k] == plain_want[:k] and got[k] != plain_want[k]
    # under the tool grammar: the arg max over allowed, unbanned tokens
    def accepted(bs):
        n, c = C.c_int32(), C.c_int32()
        assert L.tk_mi355x_grammar_check(None, bs, C.byref(n), C.byref(c)) == 0
        return n.value == len(bs)

    def piece_of(t):
        return bytes([t - 3]) if 3 <= t < 259 else (b"" if t < 3 else (" t%d" % t).encode())

    def allowed_at(lg, sofar):  # best first; EOS is allowed only where the grammar is complete, and there the runner has stopped
        return [t for t in np.argsort(-lg, kind="stable").tolist() if t != 2 and piece_of(t) and accepted(sofar + piece_of(t))]

    r.set_logit_bias([], [])
    g = generate(r, "call", 8, grammar=True)
    m.orc.reset()
    ids = prompt_ids("call")
    lg = m.orc.forward([0] * len(ids), list(range(len(ids))), ids)[0][-1]
    pos, sofar, found = len(ids), b"", None
    for s in range(len(g)):  # the first step at which the grammar leaves a choice and whose pick is new: banning it moves nothing earlier
        al = allowed_at(lg, sofar)
        assert al[0] == g[s]
        if len(al) >= 2 and g[s] not in g[:s]:
            found = (s, al[1])
            break
        sofar += piece_of(g[s])
        lg = m.orc.forward([0], [pos], [g[s]])[0][0]
        pos += 1
    assert found is not None
    s, second = found
    r.set_logit_bias([g[s]], [-np.inf])
    b = generate(r, "call", s + 1, grammar=True)
    assert b[:s] == g[:s] and b[s] == second != g[s]
    r.close(); m.close()


def test_f_the_window_survives_a_tool_response_and_empties_at_prepare(gpu):
    m = Model(gpu)
    r = m.runner()
    r.set_penalties(**PEN)
    assert r.recent_tokens() == []
    r.prepare(PROMPT)
    assert r.recent_tokens() == []          # the first id is pending, not accepted
    for _ in range(3):
        r.next_token()
    three = r.recent_tokens()
    assert three == m.reconstruct(PROMPT, 3, **PEN)[0]
    r.add_tool_response("get_time", "{\"time\": \"12:00\"}")
    assert r.recent_tokens() == three       # llama_sampling_reset is not called there: the window stands
    r.next_token()
    four = r.recent_tokens()
    assert len(four) == 4 and four[:3] == three
    # the id sampled after the tool text saw the window of three: the oracle fed the same stream says which
    m.orc.reset()
    ids = prompt_ids(PROMPT)
    m.orc.forward([0] * len(ids), list(range(len(ids))), ids, want_logits=False)
    pos = len(ids)
    for t in three:
        m.orc.forward([0], [pos], [t], want_logits=False)
        pos += 1
    tids = [3 + b for b in b"[TOOL_RESULT] name: \"get_time\", output: {\"time\": \"12:00\"} [/TOOL_RESULT]"]
    lg = m.orc.forward([0] * len(tids), list(range(pos, pos + len(tids))), tids)[0][-1]
    spec = dict(repeat=PEN["repeat"], freq=PEN["freq"], present=PEN["present"], recent=three)
    assert four[3] == int(np.argmax(R.adjust_row(lg, spec)))
    r.reset()
    assert r.recent_tokens() == four        # reset_context leaves the sampler alone too
    r.prepare(PROMPT)
    assert r.recent_tokens() == []
    # setters refuse what the limits refuse
    for bad in (dict(last_n=257), dict(last_n=-1), dict(last_n=8, repeat=0.0), dict(last_n=8, repeat=float("nan")), dict(last_n=8, freq=float("inf"))):
        with pytest.raises(gpu.TkError):
            r.set_penalties(**bad)
    for ids_, b in (([512], [1.0]), ([-1], [1.0]), ([3, 3], [1.0, 1.0]), ([3], [float("nan")]), ([3], [float("inf")]), (list(range(257)), [0.0] * 257)):
        with pytest.raises(gpu.TkError):
            r.set_logit_bias(ids_, b)
    r.close(); m.close()
