#!/usr/bin/env python3
"""The Q8_0 KV cache against the F16 one (developer tool, needs an MI355X; profiles/kv_q8.txt): on the synthetic Mistral-7B Q4_K_M, interleaved,
ROUNDS rounds each —
  runner    one runner's tok/s at a short context and behind a prompt of ~2 100 tokens, a model handle of each cache type
  launch    the decode launch set of one layer (TkLlmSession::time_attention) at 16, 64 and 256 rows over 2 100 cached positions, a session of each
            type: F16 = the fused attention the plan names, Q8_0 = the append launch + kernel 6
  bytes     cache bytes of 16 x 32 768 and 256 x 4 096 slots for both types, and whether a 256 x 4 096 session allocates on the card
  logits    the largest logit difference between a Q8_0 and an F16 session on the two-layer tiny model over one 200-token prompt (information only)
Sections are chosen on the command line (default: all)."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trackiellm_amd as tk  # noqa: E402

ROUNDS = int(os.environ.get("TK_KVQ8_ROUNDS", "4"))
NAMES = {0: "F16", 1: "Q8_0"}
want = set(sys.argv[1:]) or {"runner", "launch", "bytes", "logits"}


def tok_s(runner, prompt, n=96):
    runner.prepare(prompt)
    for _ in range(8):
        runner.next_token()
    t = time.time()
    k = 0
    for _ in range(n):
        if runner.next_token() is None:
            break
        k += 1
    return k / (time.time() - t)


if "runner" in want:
    loader = tk.ModelLoader()
    handles, runners = {}, {}
    for kv in (0, 1):
        handles[kv] = loader.load("synthetic://mistral-7b?seed=4", force_reload=True)
        tk.ModelLoader.set_kv_cache_type(handles[kv], kv)
        tk.ModelLoader.set_runner_slots(handles[kv], 1)
        runners[kv] = tk.LlmRunner(handles[kv], context_size=4096)
    for name, prompt in (("short context (184-token prompt)", "The user is in a room. " * 8), ("~2 100 cached positions", "The user is in a room. " * 91)):
        res = {0: [], 1: []}
        for _ in range(ROUNDS):
            for kv in (0, 1):
                res[kv].append(tok_s(runners[kv], prompt))
        for kv in (0, 1):
            print("runner, %s, %s: tok/s per round %s" % (name, NAMES[kv], " ".join("%.1f" % v for v in res[kv])), flush=True)
    for kv in (0, 1):
        runners[kv].close()
        loader.unload(handles[kv])
    loader.close()

if "launch" in want or "bytes" in want:
    model = tk.LlmModel(tk.MISTRAL_7B()).fill_synthetic(4)
    hp = model.hparams

if "launch" in want:
    ctx = 2100
    sess = {kv: tk.LlmSession(model, 256, 2112, kv_type=kv) for kv in (0, 1)}
    f = tk.lib().tk_mi355x_llm_time_attention
    for rows in (16, 64, 256):
        res = {0: [], 1: []}
        for _ in range(ROUNDS):
            for kv in (0, 1):
                ms, nb = C.c_float(0), C.c_double(0)
                tk.check(f(sess[kv].h, rows, ctx, 32, C.byref(ms), C.byref(nb)))
                res[kv].append((ms.value * 1000.0, nb.value))
        for kv in (0, 1):
            plan = tk.attention_plan(rows, hp.n_head, hp.n_kv_head, hp.head_dim, 2112, kv_type=kv)
            print("launch set, %d rows x %d positions, %s (plan %s): us per round %s; %.1f MB streamed" %
                  (rows, ctx, NAMES[kv], plan, " ".join("%.1f" % v[0] for v in res[kv]), res[kv][0][1] / 1e6), flush=True)
    for s in sess.values():
        s.close()

if "bytes" in want:
    per_pos = {0: 2 * hp.n_layer * hp.n_kv_head * hp.head_dim * 2, 1: 2 * hp.n_layer * hp.n_kv_head * hp.head_dim * 34 // 32}
    for slots, window in ((16, 32768), (256, 4096)):
        print("cache bytes, %d x %d: %s" % (slots, window, ", ".join("%s %.1f GB" % (NAMES[kv], slots * window * per_pos[kv] / 1e9) for kv in (0, 1))), flush=True)
    for kv in (1, 0):
        try:
            s = tk.LlmSession(model, 256, 4096, kv_type=kv)
            print("256 x 4096 %s session: allocated, kv_bytes %.1f GB" % (NAMES[kv], s.kv_bytes() / 1e9), flush=True)
            s.close()
        except tk.TkError as e:
            print("256 x 4096 %s session: refused: %s" % (NAMES[kv], e.detail), flush=True)

if "launch" in want or "bytes" in want:
    model.close()

if "logits" in want:
    tiny = tk.LlmModel(tk.TINY()).fill_synthetic(4)
    n = 200
    tok = np.random.default_rng(1).integers(3, tiny.hparams.vocab, n).astype(np.int32)
    out = {}
    for kv in (0, 1):
        s = tk.LlmSession(tiny, 1, 256, kv_type=kv)
        out[kv] = s.forward(np.zeros(n, np.int32), np.arange(n, dtype=np.int32), tok)
        s.close()
    d = np.abs(out[0][0] - out[1][0])
    print("tiny two-layer model, one %d-token prompt: largest |logit(Q8_0) - logit(F16)| = %.3g (logits span %.3g .. %.3g); arg max differs at %d of %d positions" %
          (n, d.max(), out[0][0].min(), out[0][0].max(), int((out[0][1] != out[1][1]).sum()), n), flush=True)
    tiny.close()
