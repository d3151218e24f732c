#!/usr/bin/env python3
"""One runner with a long context window through the reference entry points — developer tool, needs an MI355X.  The synthetic Mistral-7B Q4_K_M,
two runner slots, context_size TK_LW_CTX (default 32768): for each prompt length of TK_LW_DEPTHS (default 2100,8000,16000,32000 tokens) the time
tk_llm_runner_prepare_generation takes and the rate of the TK_LW_TOKENS (default 48) tokens generated behind it, the attention plan of that
decode step, and the KV cache the model's scheduler holds."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trackiellm_amd as tk  # noqa: E402

CTX = int(os.environ.get("TK_LW_CTX", "32768"))
DEPTHS = [int(v) for v in os.environ.get("TK_LW_DEPTHS", "2100,8000,16000,32000").split(",")]
N = int(os.environ.get("TK_LW_TOKENS", "48"))
SLOTS = 2
hp = tk.MISTRAL_7B()
loader = tk.ModelLoader()
h = loader.load("synthetic://mistral-7b?seed=4")
tk.ModelLoader.set_runner_slots(h, SLOTS)
t = time.time()
runner = tk.LlmRunner(h, context_size=CTX)
kv = 2 * hp.n_layer * SLOTS * CTX * hp.n_kv_head * hp.head_dim * 2
print("context_size %d, %d runner slots: KV cache %.2f GB (2 x %d layers x %d x %d positions x %d f16), resident-form limit of the geometry %d; runner created in %.2f s" %
      (CTX, SLOTS, kv / 1e9, hp.n_layer, SLOTS, CTX, hp.n_kv_head * hp.head_dim, tk.attention_resident_limit(hp.n_head, hp.n_kv_head, hp.head_dim), time.time() - t), flush=True)
for depth in DEPTHS:
    text = "".join(chr(97 + (i * 7 + depth) % 26) for i in range(depth - 1))  # one token per byte and the BOS
    t = time.time()
    runner.prepare(text)
    first = runner.next_token()
    t_prep = time.time() - t
    rows = runner.last_prompt_rows()[0]
    for _ in range(4):
        runner.next_token()
    t = time.time()
    n = 0
    for _ in range(N):
        if runner.next_token() is None:
            break
        n += 1
    dt = time.time() - t
    plan = tk.attention_plan(1, hp.n_head, hp.n_kv_head, hp.head_dim, CTX, True, top_position=min(rows + 5, CTX - 1))
    print("prompt of %d tokens: prepare + first token %.3f s (%.0f prompt tok/s); then %d tokens at %.3f ms per token, %.1f tok/s; decode-step attention plan %s%s" %
          (rows, t_prep, rows / t_prep, n, 1000 * dt / max(n, 1), n / dt if dt > 0 else 0.0, plan, "" if first is not None else " (the stream ended at once)"), flush=True)
runner.close()
loader.unload(h)
loader.close()
