"""GPU: eight runners with eight different features on ONE scheduler (one model handle, one context size, prefix cache on), each on a thread of its
own, against the same runner driven alone, one after the other, on a fresh handle of the same model without the cache.  The scheduler's contract —
"a runner sees exactly the tokens it would see alone" (csrc/llm/tk_llm_batcher.h) — is tested feature by feature elsewhere and, for the scheduling
itself, on the CPU against a toy session (tests/test_batcher_cpu.py); this test ties the toy's premise to the real session: with masks, stochastic
rows, penalties, log-probability records, verify passes, context shifts, kept and copied prompt rows all in flight at once, nothing changes.

Synthetic models tokenise bytes: ids = [1] + [3 + b ...]; id 2 ends a generation."""
import ctypes as C
import threading
import time

import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

SEED = 4
EOS = 2
PATH = "synthetic://tiny?seed=%d" % SEED
CTX = 64          # one context size: runners of one handle share a scheduler per context size
SHARED = "the quick brown fox ju"   # 23 ids: more than a copy takes (TK_PREFIX_COPY_MIN 16)
STEPS = 24
JOIN_S = 120


def prompt_ids(p):
    return [1] + [3 + b for b in p.encode()]


def generate(r, prompt, steps, grammar=False, each=None):
    """prepare + up to `steps` next_token: (pieces, the ids accepted since prepare, what `each` returned after prepare and after every token)"""
    r.prepare(prompt, use_tool_grammar=grammar)
    pieces, extra = [], [each(r)] if each else []
    for _ in range(steps):
        p = r.next_token()
        if p is None or p == "<tool_call>":
            pieces.append(p)
            break
        pieces.append(p)
        if each:
            extra.append(each(r))
    return pieces, r.recent_tokens(), extra


def plain(r, pred):
    return generate(r, SHARED + "mps", STEPS)


def grammar(r, pred):
    return generate(r, "call", 40, grammar=True)


def stochastic(r, pred):
    r.set_sampling(0.8)
    return generate(r, SHARED + "st", STEPS)


def penalties(r, pred):
    r.set_penalties(32, repeat=1.3, freq=0.1, present=0.1)
    r.set_logit_bias([3 + ord("e"), 3 + ord(" ")], [-2.0, 1.5])
    return generate(r, "hello there", STEPS)


def logprobs(r, pred):
    r.set_logprobs(3)
    return generate(r, SHARED + "lp", STEPS, each=lambda r: r.last_logprobs())


def lookup(r, pred):
    r.set_lookup(4, 1, 3)
    r.set_prediction(pred)
    out = generate(r, "a", STEPS)
    return out + (r.lookup_stats(),)


def shift(r, pred):
    r.set_context_shift(True, 8)
    out = generate(r, "a", 100)
    return out + (r.context_shifts(),)


def reprompt(r, pred):
    first = generate(r, SHARED + "mp", 5)              # abandoned with a row ahead of it
    return first, generate(r, SHARED + "mps over", 12)


FEATURES = [plain, grammar, stochastic, penalties, logprobs, lookup, shift, reprompt]


def oracle_greedy(gpu, h, prompt, steps):
    """the ids a greedy runner hands out for `prompt`: the oracle's arg max chain, up to `steps` ids, without the EOS that ends it"""
    hp = gpu.LlmHParams()
    gpu.lib().tk_mi355x_llm_model_get_hparams(h, C.byref(hp))
    orc = O.OracleLlm(O.LlmConfig(n_layer=hp.n_layer, d_model=hp.d_model, n_head=hp.n_head, n_kv_head=hp.n_kv_head, head_dim=hp.head_dim, d_ff=hp.d_ff,
                                  vocab=hp.vocab, max_ctx=CTX, max_seq=1, rms_eps=hp.rms_eps, rope_theta=hp.rope_theta, ks_qkv=hp.ks_qkv, ks_o=hp.ks_o,
                                  ks_gateup=hp.ks_gateup, ks_down=hp.ks_down, ks_out=hp.ks_out), seed=SEED)
    ids = prompt_ids(prompt)
    _, am = orc.forward([0] * len(ids), list(range(len(ids))), ids, want_logits=False)
    cur, out = int(am[-1]), []
    while cur != EOS and len(out) < steps:
        out.append(cur)
        _, am = orc.forward([0], [len(ids) + len(out) - 1], [cur], want_logits=False)
        cur = int(am[0])
    return out


def test_eight_features_on_one_scheduler(gpu):
    loader = gpu.ModelLoader()
    solo_h = loader.load(PATH, force_reload=True)
    mix_h = loader.load(PATH, force_reload=True)
    assert solo_h.value != mix_h.value
    gpu.ModelLoader.set_prefix_cache(mix_h, True)
    runners = []
    try:
        want_plain, want_lookup = oracle_greedy(gpu, solo_h, SHARED + "mps", STEPS), oracle_greedy(gpu, solo_h, "a", STEPS)
        pred = want_lookup  # the lookup runner's prediction: what it is going to say
        t0 = time.time()
        solo = []
        for i, f in enumerate(FEATURES):
            r = gpu.LlmRunner(solo_h, context_size=CTX, random_seed=11 + i)
            solo.append(f(r, pred))
            r.close()
        t1 = time.time()
        runners = [gpu.LlmRunner(mix_h, context_size=CTX, random_seed=11 + i) for i in range(len(FEATURES))]
        mix, errors = [None] * len(FEATURES), []
        gate = threading.Barrier(len(FEATURES))

        def work(i):
            try:
                gate.wait(30)
                mix[i] = FEATURES[i](runners[i], pred)
            except BaseException as e:  # reported by the test's own thread
                errors.append((FEATURES[i].__name__, repr(e)))

        threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(len(FEATURES))]
        for t in threads:
            t.start()
        deadline = time.time() + JOIN_S
        for t in threads:
            t.join(max(0.0, deadline - time.time()))
        stuck = [FEATURES[i].__name__ for i, t in enumerate(threads) if t.is_alive()]
        t2 = time.time()
        if stuck:
            runners = []  # their calls never returned: nothing can be closed under them
        assert not stuck, "runners that never came back from the scheduler: %s" % stuck
        assert not errors, errors
        passes, rows, widest = gpu.ModelLoader.batch_stats(mix_h)
        print("alone %.2f s, together %.2f s; together: %d passes, %d rows, widest %d; prefix cache %s; run-ahead rows wasted %d" %
              (t1 - t0, t2 - t1, passes, rows, widest, gpu.ModelLoader.prefix_cache_stats(mix_h), gpu.ModelLoader.run_ahead_wasted(mix_h)))
        for f, a, b in zip(FEATURES, solo, mix):
            assert a == b, f.__name__
        # the features did what their names say
        by = dict(zip((f.__name__ for f in FEATURES), solo))
        assert len(by["plain"][0]) >= 12, "the plain run of this prompt and seed is too short: choose another"
        assert by["grammar"][0] and all(p is not None for p in by["grammar"][0][:-1])
        assert len(by["logprobs"][2]) >= 2 and all(len(tops) == 3 for _, tops in by["logprobs"][2])
        assert by["lookup"][3][2] >= 4, by["lookup"][3]      # drafts accepted
        assert by["shift"][3][0] >= 1, by["shift"][3]        # context shifts
        assert by["reprompt"][0][0] and by["reprompt"][1][0]
        # the plain and the lookup runner against the oracle's greedy ids
        for name, want in (("plain", want_plain), ("lookup", want_lookup)):
            pieces, ids = by[name][0], by[name][1]
            handed = [p for p in pieces if p is not None]
            assert len(handed) == len(want) and ids[:len(handed)] == want, name
    finally:
        for r in runners:
            r.close()
        loader.unload(solo_h)
        loader.unload(mix_h)
        loader.close()
