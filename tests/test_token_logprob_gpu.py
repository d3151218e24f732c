"""GPU: per-token log-probabilities on the device — k_token_logprobs alone (tk_mi355x_token_logprobs_probe), inside a pass
(tk_mi355x_llm_forward_logprobs) and behind tk_llm_runner_* (set_logprobs / last_logprobs).  The reference is the probe's host loop (device = -1) of
csrc/common/tk_token_logprob.h, which tests/test_token_logprob_cpu.py ties to the NumPy restatements; records are compared as bytes."""
import functools

import numpy as np
import pytest

import token_logprob_cases as LC

pytestmark = pytest.mark.gpu

SEED, NCTX, NTOK = 4, 96, 14
SAMP = (0.8, 40, 0.95, 0.05)
PEN = dict(last_n=8, repeat=1.3, freq=0.5, present=0.25)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(LC.cases())


def same_record(a, b):
    """two records agree in everything that is filled"""
    n = int(a["n_top"])
    return (n == int(b["n_top"]) and bits(a["logprob"]) == bits(b["logprob"]) and a["top_ids"][:n].tolist() == b["top_ids"][:n].tolist()
            and np.array_equal(bits(a["top_logprobs"][:n]), bits(b["top_logprobs"][:n])))


@pytest.mark.parametrize("name", [c["name"] for c in LC.cases()])
def test_the_kernel_equals_the_host_loop_bit_for_bit(gpu, name):
    c = next(c for c in all_cases() if c["name"] == name)
    sent = LC.sentinel_records(c["rows"])
    host = gpu.token_logprobs_probe(c["logits"], c["rows"], c["cols"], c["ids"], c["n_top"], records=sent.copy(), ld=c["ld"], device=-1)
    dev = gpu.token_logprobs_probe(c["logits"], c["rows"], c["cols"], c["ids"], c["n_top"], records=sent.copy(), ld=c["ld"], device=0)
    for r in range(c["rows"]):
        assert dev[r].tobytes() == host[r].tobytes(), (name, r, c["kinds"][r], int(c["n_top"][r]), dev[r], host[r])
        if c["n_top"][r] < 0:
            assert dev[r].tobytes() == sent[r].tobytes()


def test_the_kernel_refuses_before_it_launches(gpu):
    for name, kw in LC.refusals(gpu.lib().tk_mi355x_llm_max_rows()):
        sent = LC.sentinel_records(max(int(kw["rows"]), 1))
        rec = sent.copy()
        with pytest.raises(gpu.TkError) as e:
            gpu.token_logprobs_probe(kw["logits"], kw["rows"], kw["cols"], kw["ids"], kw["n_top"], records=rec, ld=kw["ld"], device=0, n_logits=kw.get("n_logits"))
        assert e.value.code == 1001 and rec.tobytes() == sent.tobytes(), name


# ---- a session ------------------------------------------------------------------------------------------------------------------------------
def host_records(gpu, logits, ids, n_top):
    rows, cols = logits.shape
    return gpu.token_logprobs_probe(logits, rows, cols, ids, n_top, records=LC.sentinel_records(rows), device=-1)


@pytest.mark.parametrize("distinct", [True, False])
def test_forward_logprobs_in_one_pass(gpu, distinct):
    """greedy, sampled with a seed, adjusted and off rows in one pass: the ids and logits of forward_adjusted, the records of the host loop on those
    logits; then the same rows alone and in a wide pass"""
    model = gpu.LlmModel(gpu.TINY()).fill_synthetic(SEED)
    vocab = model.hparams.vocab
    rng = np.random.default_rng(5)
    sess = gpu.LlmSession(model, 8, 32)
    seq0 = np.repeat(np.arange(8, dtype=np.int32), 3)
    sess.forward(seq0, np.tile(np.arange(3, dtype=np.int32), 8), np.random.default_rng(6).integers(3, vocab, 24).astype(np.int32), want_logits=False)
    seq = np.array([0, 1, 2, 3, 4] if distinct else [0, 0, 1, 2, 3], np.int32)
    pos = np.array([3, 3, 3, 3, 3] if distinct else [3, 4, 3, 3, 3], np.int32)
    tok = rng.integers(3, vocab, 5).astype(np.int32)
    raw, _ = sess.forward(seq, pos, tok)
    top = np.argsort(-raw, axis=1, kind="stable")
    specs = [None, None, dict(repeat=1.3, freq=0.5, present=2.0, recent=top[2, :3].tolist(), bias_ids=[int(top[2, 0]), int(top[2, 5])], bias=[-np.inf, 3.0]), None,
             dict(bias_ids=[int(top[4, 1])], bias=[-np.inf])]
    sampling = [(0.0, 40, 0.95, 0.05, 0, 0), SAMP + (1234, 7), (0.0, 40, 0.95, 0.05, 0, 0), SAMP + (99, 3), (0.0, 40, 0.95, 0.05, 0, 0)]
    n_top = np.array([20, 5, 3, -1, 0], np.int32)
    want_lg, want_ids = sess.forward_adjusted(seq, pos, tok, specs, sampling=sampling)
    sent = LC.sentinel_records(5)
    lg, ids, rec = sess.forward_logprobs(seq, pos, tok, n_top, adjust=specs, sampling=sampling, records=sent.copy())
    assert np.array_equal(bits(lg), bits(want_lg)) and ids.tolist() == want_ids.tolist()
    host = host_records(gpu, lg, ids, n_top)
    for r in range(5):
        assert rec[r].tobytes() == host[r].tobytes(), (r, rec[r], host[r])     # the sentinels past the count and of the off row included
    assert rec[3].tobytes() == sent[3].tobytes()
    assert np.isneginf(rec["top_logprobs"][2, :3]).sum() == 0 and int(top[2, 0]) not in rec["top_ids"][2, :3].tolist()   # the banned token left the top
    assert rec["top_ids"][0, 0] == ids[0] and rec["logprob"][0] == rec["top_logprobs"][0, 0]                            # greedy: the first alternative
    # adjust = sampling = None: plain greedy rows
    lg2, ids2, rec2 = sess.forward_logprobs(seq, pos, tok, n_top)
    assert np.array_equal(bits(lg2), bits(raw)) and ids2.tolist() == np.argmax(raw, axis=1).tolist()
    host2 = host_records(gpu, raw, ids2, n_top)
    assert all(same_record(rec2[r], host2[r]) for r in (0, 1, 2, 4))
    # every n_top = -1: the pass forward_adjusted runs, nothing written
    lg3, ids3, rec3 = sess.forward_logprobs(seq, pos, tok, np.full(5, -1, np.int32), adjust=specs, sampling=sampling, records=sent.copy())
    assert np.array_equal(bits(lg3), bits(want_lg)) and ids3.tolist() == want_ids.tolist() and rec3.tobytes() == sent.tobytes()
    # the same row in a 1-row pass and in a wide pass gives the same record
    if distinct:
        wseq = np.arange(8, dtype=np.int32)
        wpos = np.full(8, 3, np.int32)
        wtok = np.concatenate([tok, rng.integers(3, vocab, 3).astype(np.int32)])
        _, wids, wrec = sess.forward_logprobs(wseq, wpos, wtok, np.full(8, 20, np.int32))
        for r in (0, 4, 7):
            _, oid, orec = sess.forward_logprobs(wseq[r:r + 1], wpos[r:r + 1], wtok[r:r + 1], np.array([20], np.int32))
            assert oid[0] == wids[r] and orec[0].tobytes() == wrec[r].tobytes(), r
    # refused whole
    with pytest.raises(gpu.TkError) as e:
        sess.forward_logprobs(seq, pos, tok, np.array([0, 0, 21, 0, 0], np.int32))
    assert e.value.code == 1001
    # nothing leaks: a plain forward + decode() afterwards gives what a session that never asked gives
    dseq = np.arange(5, dtype=np.int32)
    dpos = np.array([4, 4, 4, 4, 4] if distinct else [5, 4, 4, 4, 3], np.int32)
    dtok = rng.integers(3, vocab, 5).astype(np.int32)

    def tail(s):
        _, first = s.forward(dseq, dpos, dtok, want_logits=False)
        toks, _ = s.decode(5, 4)
        return first.tolist(), np.asarray(toks).tolist()

    sess.forward_logprobs(seq, pos, tok, n_top, adjust=specs, sampling=sampling)
    used = tail(sess)
    fresh = gpu.LlmSession(model, 8, 32)
    fresh.forward(seq0, np.tile(np.arange(3, dtype=np.int32), 8), np.random.default_rng(6).integers(3, vocab, 24).astype(np.int32), want_logits=False)
    fresh.forward(seq, pos, tok, want_logits=False)
    assert tail(fresh) == used
    sess.close(); fresh.close(); model.close()


# ---- runners ----------------------------------------------------------------------------------------------------------------------------------
def prompt_ids(p):
    return [1] + [3 + b for b in p.encode()]


class Model:
    def __init__(self, gpu):
        self.gpu = gpu
        self.loader = gpu.ModelLoader()
        self.h = self.loader.load("synthetic://tiny?seed=%d" % SEED, force_reload=True)

    def runner(self):
        return self.gpu.LlmRunner(self.h, context_size=NCTX, random_seed=11)

    def close(self):
        self.loader.unload(self.h)
        self.loader.close()


def generate(runner, prompt, n=NTOK, grammar=False, records=None):
    """n calls of next_token; the accepted ids; records (a list): last_logprobs() of every sampled id — the id accepted by the call that follows"""
    runner.prepare(prompt, use_tool_grammar=grammar)
    if records is not None:
        records.append(runner.last_logprobs())
    for _ in range(n):
        if runner.next_token() in (None, "<tool_call>"):
            break
        if records is not None:
            records.append(runner.last_logprobs())
    return runner.recent_tokens()


MODES = {"greedy": {}, "temperature": dict(sampling=SAMP), "grammar": dict(grammar=True), "penalties": dict(pen=PEN)}


def configure(r, mode):
    if "sampling" in mode:
        r.set_sampling(*mode["sampling"])
    if "pen" in mode:
        r.set_penalties(**mode["pen"])


@pytest.mark.parametrize("mode", sorted(MODES))
def test_a_runner_with_logprobs_emits_the_same_stream_and_a_sessions_records(gpu, mode):
    cfg = MODES[mode]
    prompt = "call" if cfg.get("grammar") else "hi"
    k = 5
    m = Model(gpu)
    off = m.runner()
    configure(off, cfg)
    want = generate(off, prompt, grammar=cfg.get("grammar", False))
    on = m.runner()
    configure(on, cfg)
    on.set_logprobs(k)
    recs = []
    got = generate(on, prompt, grammar=cfg.get("grammar", False), records=recs)
    assert got == want and len(got) >= 3
    assert len(recs) >= len(got)            # one record per accepted id (and one for the id still pending, if the loop ran out)
    # a separate session over the same tokens
    model = gpu.LlmModel(gpu.TINY()).fill_synthetic(SEED)
    sess = gpu.LlmSession(model, 1, NCTX)
    ids = prompt_ids(prompt)
    sess.forward([0] * (len(ids) - 1), list(range(len(ids) - 1)), ids[:-1], want_logits=False)
    fed, pos = ids[-1], len(ids) - 1
    for i, cur in enumerate(got):
        adjust = [dict(recent=got[max(0, i - PEN["last_n"]):i], repeat=PEN["repeat"], freq=PEN["freq"], present=PEN["present"])] if "pen" in cfg else None
        sampling = [cfg["sampling"] + (11, i)] if "sampling" in cfg else None
        lg, sid, srec = sess.forward_logprobs([0], [pos], [fed], [k], adjust=adjust, sampling=sampling)
        if cfg.get("grammar"):
            # the session samples without the mask; the record's distribution does not depend on it: the host loop on these logits with the runner's id
            srec = host_records(gpu, lg, np.array([cur], np.int32), np.array([k], np.int32))
        else:
            assert int(sid[0]) == cur, (mode, i)
        lp, alts = recs[i]
        assert bits(np.float32(lp)) == bits(srec["logprob"][0]), (mode, i, lp, float(srec["logprob"][0]))
        assert [a[0] for a in alts] == srec["top_ids"][0, :k].tolist(), (mode, i)
        assert np.array_equal(bits(np.array([a[1] for a in alts], np.float32)), bits(srec["top_logprobs"][0, :k])), (mode, i)
        if mode == "greedy":
            assert alts[0][0] == cur and alts[0][1] == lp
        fed, pos = cur, pos + 1
    if cfg.get("grammar"):      # a forbidden token may be the model's favourite: somewhere the first alternative is not the id the grammar let through
        assert any(recs[i][1][0][0] != got[i] for i in range(len(got)))
    sess.close(); model.close()
    off.close(); on.close(); m.close()


def test_two_runners_with_different_n_top_each_get_their_own(gpu):
    import threading
    m = Model(gpu)
    a, b, c = m.runner(), m.runner(), m.runner()
    a.set_logprobs(2)
    b.set_logprobs(20)
    out, errs = {}, []

    def work(name, r, with_records):
        try:
            recs = [] if with_records else None
            out[name] = (generate(r, "hi", records=recs), recs)
        except Exception as e:  # noqa: BLE001
            errs.append((name, repr(e)))

    th = [threading.Thread(target=work, args=("a", a, True)), threading.Thread(target=work, args=("b", b, True)), threading.Thread(target=work, args=("c", c, False))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    assert out["a"][0] == out["b"][0] == out["c"][0]
    ra, rb = out["a"][1], out["b"][1]
    assert len(ra) == len(rb) >= 3
    for (lpa, alta), (lpb, altb) in zip(ra, rb):
        assert len(alta) == 2 and len(altb) == 20
        assert lpa == lpb and alta == altb[:2]
    # a change of n_top in the middle of a generation takes effect from the next sampled token
    a.prepare("hi")
    assert len(a.last_logprobs()[1]) == 2
    a.set_logprobs(0)
    assert len(a.last_logprobs()[1]) == 2      # the pending id was sampled before the change
    a.next_token()
    assert a.last_logprobs()[1] == []
    for r in (a, b, c):
        r.close()
    m.close()


def test_lookup_does_nothing_while_logprobs_are_on(gpu):
    m = Model(gpu)
    plain = m.runner()
    want = generate(plain, "hi")
    r = m.runner()
    r.set_lookup(8, 1, 3)
    r.set_prediction(want)                     # a perfect prediction: with lookup active every pass would carry drafts
    r.set_logprobs(3)
    recs = []
    assert generate(r, "hi", records=recs) == want
    assert r.lookup_stats() == (0, 0, 0) and len(recs) >= len(want)
    r.set_logprobs(-1)                         # off again: lookup drafts, the stream stands
    assert generate(r, "hi") == want
    assert r.lookup_stats()[1] > 0
    plain.close(); r.close(); m.close()


def test_last_logprobs_errors_and_the_setter_keeps_its_setting(gpu):
    m = Model(gpu)
    r = m.runner()
    with pytest.raises(gpu.TkError):           # off
        r.last_logprobs()
    r.prepare("hi")
    with pytest.raises(gpu.TkError):           # still off, though something was sampled
        r.last_logprobs()
    r.set_logprobs(4)
    with pytest.raises(gpu.TkError):           # on, nothing sampled since
        r.last_logprobs()
    for bad in (-2, 21, 1000):
        with pytest.raises(gpu.TkError) as e:
            r.set_logprobs(bad)
        assert e.value.code == 1001
    r.next_token()
    assert len(r.last_logprobs()[1]) == 4      # the setting of 4 was kept
    r.set_logprobs(-1)
    with pytest.raises(gpu.TkError):
        r.last_logprobs()
    r.close(); m.close()
