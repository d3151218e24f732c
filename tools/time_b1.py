#!/usr/bin/env python3
"""One runner through the reference entry points (developer tool, needs an MI355X): tk_model_loader_load_model ->
tk_llm_runner_prepare_generation -> N x tk_llm_runner_generate_next_token on the synthetic Mistral-7B Q4_K_M, ms per token.
TK_MI355X_NO_FUSE=1 keeps the norm / SwiGLU producers as launches of their own (A/B); under rocprofv3 --kernel-trace --stats the per-kernel
durations of the decode step come out (ROC_AQL_QUEUE_SIZE=524288 for the graph path, DESIGN.md "Profiling").
--prefix-cache (default off) switches the model's prompt prefix cache on; either way a second turn (the same preamble, another ending) is prepared
after the decode loop and its prepare_generation latency and the model's prefix_cache_stats are printed.
--penalties LAST_N,REPEAT (default none) gives the runner repetition penalties: an adjusted runner does not run ahead, so this measures the
extra launch, the table upload and above all one host round trip per token (profiles/sampler_adjust.txt)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trackiellm_amd as tk  # noqa: E402

N = int(os.environ.get("TK_B1_TOKENS", "128"))
loader = tk.ModelLoader()
h = loader.load("synthetic://mistral-7b?seed=4")
prefix_cache = "--prefix-cache" in sys.argv
tk.ModelLoader.set_prefix_cache(h, prefix_cache)
runner = tk.LlmRunner(h, context_size=int(os.environ.get("TK_B1_CTX", "512")))  # TK_B1_CTX=4096: the window of the reference's default runner
penalties = "none"
if "--penalties" in sys.argv:
    penalties = sys.argv[sys.argv.index("--penalties") + 1]
    last_n, repeat = penalties.split(",")
    runner.set_penalties(int(last_n), float(repeat))
t = time.time()
runner.prepare("The user is in a room. " * 8)
t_first = time.time() - t
for _ in range(8):
    runner.next_token()
t = time.time()
n = 0
for _ in range(N):
    if runner.next_token() is None:
        break
    n += 1
dt = time.time() - t
print(f"one runner: {n} tokens, {1000 * dt / max(n, 1):.3f} ms per token, {n / dt:.1f} tok/s (TK_MI355X_NO_FUSE={os.environ.get('TK_MI355X_NO_FUSE', '0')}, penalties {penalties})", flush=True)
t = time.time()
runner.prepare("The user is in a room. " * 7 + "The user is in a hall. ")
t_second = time.time() - t
print(f"prepare_generation: first turn {1000 * t_first:.2f} ms, second turn {1000 * t_second:.2f} ms; last_prompt_rows (rows, kept, copied) = {runner.last_prompt_rows()}; "
      f"prefix cache {'on' if prefix_cache else 'off'}: (prompt rows, kept, copied, copy launches) = {tk.ModelLoader.prefix_cache_stats(h)}", flush=True)
runner.close()
loader.unload(h)
loader.close()
