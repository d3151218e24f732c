"""GPU: grammar masks built on the device behind tk_llm_runner_* (tk_mi355x_llm_runner_set_device_mask), and a GBNF grammar per runner
(tk_mi355x_llm_runner_set_grammar), on synthetic://tiny.

The same runner configuration is run with the device mask off and on: everything a host can see must be equal.  The fixtures follow
tests/test_lookup_scope_gpu.py.  Synthetic models tokenise bytes: ids = [1] + [3 + b ...]; id 2 ends a generation; ids from 259 on have the piece " t<id>"."""
import ctypes as C
import threading

import pytest

pytestmark = pytest.mark.gpu

TK_ERROR_INVALID_ARGUMENT = 1001
SEED = 4
PATH = "synthetic://tiny?seed=%d" % SEED
LOOKUP = (4, 1, 3)
CLOSING_BRACE = 3 + ord("}")
LIST_GRAMMAR = 'root ::= "[" [0-9]+ ("," [0-9]+)* "]"\n'
# every byte of a piece " t<id>" pushes three return positions (root -> a -> b -> root): the five bytes of " t300" need more private stack entries than
# the walk holds (csrc/common/tk_grammar_walk.h), so that token is undecided at the first position, where the grammar allows it
DEEP_GRAMMAR = 'root ::= [ t0-9] a ")" | "x"\na ::= b "]"\nb ::= root "}"\n'
LONG_PIECE = 300


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


def grammar_check(gpu, gbnf, text):
    n, c = C.c_int32(), C.c_int32()
    assert gpu.lib().tk_mi355x_grammar_check(None if gbnf is None else gbnf.encode(), text, C.byref(n), C.byref(c)) == 0
    return n.value, bool(c.value)


def generate(r, prompt, grammar=True, logprobs=False, cap=250):
    """prepare + next_token until the run ends: the pieces, the accepted ids, the records, the tool-call text and how it ended"""
    r.prepare(prompt, use_tool_grammar=grammar)
    pieces, recs, end = [], [], "cap"
    for _ in range(cap):
        if logprobs:
            recs.append(r.last_logprobs())
        p = r.next_token()
        if p is None or p == "<tool_call>":
            end = p
            break
        pieces.append(p)
    return dict(pieces=pieces, ids=r.recent_tokens(), recs=recs, text=r.tool_call_text(), end=end)


def rest_of(r, logprobs=False):
    pieces, recs = [], []
    for _ in range(30):
        if logprobs:
            recs.append(r.last_logprobs())
        p = r.next_token()
        if p is None or p == "<tool_call>":
            break
        pieces.append(p)
    return dict(pieces=pieces, ids=r.recent_tokens(), recs=recs, text=r.tool_call_text())


CASES = {
    "greedy": dict(),
    "temperature": dict(temp=0.7),
    "penalties": dict(penalties=(64, 1.3, 0.05, 0.0), logprobs=True),
    "lookup": dict(penalties=(64, 1.0, 0.05, 0.0), lookup=True),
}


def configure(handle, case, device, seed=11, pred=None):
    c = CASES[case]
    r = handle.runner(256, random_seed=seed)
    if "temp" in c:
        r.set_sampling(c["temp"])
        r.set_logit_bias([CLOSING_BRACE], [-3.0])  # sampled under the grammar this model closes its call at once: keep it open for a while
    if "penalties" in c:
        r.set_penalties(c["penalties"][0], repeat=c["penalties"][1], freq=c["penalties"][2], present=c["penalties"][3])
    if c.get("logprobs"):
        r.set_logprobs(5)
    if c.get("lookup"):
        r.set_lookup(*LOOKUP)
        r.set_lookup_scope(sampled=True, grammar=True, adjusted=True, logprobs=True)
        r.set_prediction(pred or [])
    r.set_device_mask(device)
    return r


@pytest.mark.parametrize("case", ["greedy", "temperature", "penalties"])
def test_same_output_with_the_device_mask_on_and_off(handle, case):
    lp = bool(CASES[case].get("logprobs"))
    host_r = configure(handle, case, False)
    host = generate(host_r, "a", logprobs=lp, cap=120)
    assert host_r.mask_stats()[0] == 0 and host_r.mask_stats()[1] > 0
    dev_r = configure(handle, case, True)
    dev = generate(dev_r, "a", logprobs=lp, cap=120)
    assert dev == host, [k for k in host if dev[k] != host[k]]
    assert len(host["ids"]) >= 3
    device_rows, host_rows, redone = dev_r.mask_stats()
    assert device_rows >= len(host["ids"]) and host_rows == 0 and redone == 0, (device_rows, host_rows, redone)


def test_lookup_inside_the_grammar_scope_with_its_own_output_as_prediction(handle):
    """the rows of a scoped verify request carry their states too; the prediction is the run's own output, so drafts are accepted"""
    plain = generate(configure(handle, "penalties", False, pred=None), "call the clock", logprobs=True)
    host_r = configure(handle, "lookup", False, pred=plain["ids"])
    host = generate(host_r, "call the clock")
    dev_r = configure(handle, "lookup", True, pred=plain["ids"])
    dev = generate(dev_r, "call the clock")
    assert dev == host
    assert dev_r.lookup_stats() == host_r.lookup_stats() and dev_r.lookup_stats()[2] >= 4
    device_rows, host_rows, redone = dev_r.mask_stats()
    assert device_rows > dev_r.lookup_stats()[0] and host_rows == 0 and redone == 0


def test_tool_response_followed_by_free_text(handle):
    out = []
    for device in (False, True):
        r = configure(handle, "lookup", device)
        call = generate(r, "call the clock")
        assert call["end"] == "<tool_call>", "the run does not complete its tool call: choose another penalty or prompt"
        stats = r.mask_stats()
        r.add_tool_response("clock", "12:00")
        out.append((call, rest_of(r), r.mask_stats() == stats))  # free text: no mask rows at all behind the call
        assert (stats[0] > 0 and stats[1] == 0) if device else (stats[0] == 0 and stats[1] > 0)
    assert out[0] == out[1] and out[0][2] and len(out[0][1]["pieces"]) > 0


def test_an_undecided_token_makes_the_runner_submit_again_under_a_host_mask(handle):
    out = []
    for device in (False, True):
        r = handle.runner(256, random_seed=3)
        r.set_grammar(DEEP_GRAMMAR)
        r.set_logit_bias([LONG_PIECE], [50.0])
        r.set_device_mask(device)
        out.append(generate(r, "a", cap=40))
        device_rows, host_rows, redone = r.mask_stats()
        assert (redone > 0 and host_rows >= redone) if device else (redone == 0 and device_rows == 0)
    assert out[0] == out[1]
    assert out[0]["ids"][0] == LONG_PIECE and out[0]["text"].startswith(b" t300")


@pytest.mark.parametrize("device", [False, True])
def test_set_grammar(handle, device):
    gpu = handle.gpu
    r = handle.runner(256, random_seed=5)
    r.set_device_mask(device)
    r.set_penalties(64, repeat=1.0, freq=0.3)  # lets "]" win after a few digits
    r.set_grammar(LIST_GRAMMAR)
    out = generate(r, "a", cap=200)
    n, complete = grammar_check(gpu, LIST_GRAMMAR, out["text"])
    assert n == len(out["text"]) and len(out["text"]) >= 3
    assert out["end"] == "<tool_call>" and complete, out
    assert (r.mask_stats()[0] > 0) == device
    # refusals: a text that does not parse leaves the grammar as it is; no change during a generation
    with pytest.raises(gpu.TkError) as e:
        r.set_grammar('root ::= "abc')
    assert e.value.code == TK_ERROR_INVALID_ARGUMENT
    again = generate(r, "a", cap=200)
    assert again == out
    r.prepare("a", use_tool_grammar=True)
    with pytest.raises(gpu.TkError):
        r.set_grammar(None)
    while r.next_token() not in (None, "<tool_call>"):
        pass
    # NULL restores the tool-call grammar
    r.set_grammar(None)
    r.set_penalties(64, repeat=1.0, freq=0.05)
    tool = generate(r, "call the clock")
    assert tool["text"].startswith(b"{") and grammar_check(gpu, None, tool["text"])[0] == len(tool["text"])
    fresh = handle.runner(256, random_seed=5)
    fresh.set_penalties(64, repeat=1.0, freq=0.05)
    assert generate(fresh, "call the clock") == tool


def test_a_runner_without_the_device_mask_shares_the_model_with_one_that_has_it(handle):
    prompts = ["call the clock", "hi there"]
    solo = [generate(configure(handle, "penalties", False), prompts[0], logprobs=True), generate(configure(handle, "greedy", False), prompts[1], cap=60)]
    ra, rb = configure(handle, "penalties", True), configure(handle, "greedy", False)
    out = [None, None]

    def work(i, r):
        out[i] = generate(r, prompts[i], logprobs=(i == 0), cap=250 if i == 0 else 60)
    threads = [threading.Thread(target=work, args=(i, r)) for i, r in enumerate((ra, rb))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert out[0] == solo[0] and out[1] == solo[1]
    assert ra.mask_stats()[0] > 0 and ra.mask_stats()[1] == 0 and rb.mask_stats()[0] == 0 and rb.mask_stats()[1] > 0
