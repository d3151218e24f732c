#!/usr/bin/env python3
"""Per-token log-probabilities (tk_mi355x_llm_runner_set_logprobs): what they cost — developer tool, needs an MI355X.

    python tools/time_token_logprobs.py [--rounds 4] [--parent-lib /path/to/the/parent/commit's/libtrackie_mi355x.so] [--parent-first] [--skip-runner]

1. ONE runner on full synthetic 7B (Q4_K_M), 256 tokens per generation.  Configurations, interleaved round by round in one call, their order rotated
   every round:
       parent   the parent commit's library (only with --parent-lib), the runner as it was
       off      this library, log-probabilities off
       n0       n_top = 0: the log-probability of the produced id
       n20      n_top = 20: and twenty alternatives
   Each library lives in a child process of its own that keeps its model and runner.  A window is the generate_next_token loop alone
   (prepare_generation is outside it), host clock.  Prints tok/s per round and the range per configuration; the ids of all must be equal.
2. The kernel alone (tk_mi355x_time_token_logprobs) at 1, 16 and 256 rows x 32000 with n_top 0 and 20, beside the lm_head launch of the same width
   (tk_mi355x_llm_time_gemv, which = 3): device events around 200 launches after a warm-up."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOKENS = 256
PATH = "synthetic://mistral-7b?seed=4"
PROMPT = "scene door left person"


def child():
    sys.path.insert(0, ROOT)
    import trackiellm_amd as tk
    loader = tk.ModelLoader()
    handle = loader.load(PATH, force_reload=True)
    runner = tk.LlmRunner(handle, context_size=4096)
    print(json.dumps({"ready": True}), flush=True)
    for line in sys.stdin:
        cmd = json.loads(line)
        if cmd.get("quit"):
            break
        if "n_top" in cmd:
            runner.set_logprobs(cmd["n_top"])
        runner.prepare(PROMPT)
        n, lp = 0, 0.0
        t0 = time.perf_counter()
        while n < TOKENS and runner.next_token() is not None:
            n += 1
            if cmd.get("n_top", -1) >= 0:
                lp += runner.last_logprobs()[0]  # what a host that asked does: reads every record
        dt = time.perf_counter() - t0
        print(json.dumps({"tokens": n, "seconds": dt, "ids": runner.recent_tokens(), "mean_logprob": lp / max(n, 1)}), flush=True)
    runner.close()
    loader.unload(handle)
    loader.close()


class Child:
    def __init__(self, lib):
        env = dict(os.environ)
        if lib:
            env["TK_MI355X_LIB"] = lib
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, env=env, text=True)
        assert json.loads(self.p.stdout.readline())["ready"]

    def run(self, **cmd):
        self.p.stdin.write(json.dumps(cmd) + "\n")
        self.p.stdin.flush()
        line = self.p.stdout.readline()
        if not line:
            raise RuntimeError("the child process ended (exit status %s)" % self.p.wait())
        return json.loads(line)

    def close(self):
        self.p.stdin.write(json.dumps({"quit": True}) + "\n")
        self.p.stdin.flush()
        self.p.wait()


def runner_rounds(args):
    # two processes of ONE library differ by a fraction of a per cent (where each one's weights and cache land): --parent-first swaps which of the two
    # is created first, so that an offset that follows the process can be told from one that follows the library
    parent = Child(args.parent_lib) if args.parent_lib and args.parent_first else None
    new = Child(None)
    if args.parent_lib and not parent:
        parent = Child(args.parent_lib)
    try:
        configs = {"off": dict(n_top=-1), "n0": dict(n_top=0), "n20": dict(n_top=20)}
        plain = new.run(**configs["off"])
        for cfg in configs.values():
            new.run(**cfg)  # warm-up: the graphs of each configuration
        if parent:
            parent.run()
        rates = {k: [] for k in (["parent"] if parent else []) + list(configs)}
        order = list(rates)
        mean_lp = {}
        for rnd in range(args.rounds):
            for k in order[rnd % len(order):] + order[:rnd % len(order)]:  # the order rotates: no configuration always follows the same one
                r = parent.run() if k == "parent" else new.run(**configs[k])
                assert r["ids"] == plain["ids"], "%s: ids differ from the plain run" % k
                rates[k].append(r["tokens"] / r["seconds"])
                mean_lp[k] = r["mean_logprob"]
        print("one runner, 7B Q4_K_M, %d tokens per generation, %d interleaved rounds:" % (plain["tokens"], args.rounds))
        for k, v in rates.items():
            print("  %-7s %s tok/s   range %.1f - %.1f%s" % (k, " ".join("%.1f" % x for x in v), min(v), max(v),
                                                              "   mean logprob %.4f" % mean_lp[k] if k in ("n0", "n20") else ""), flush=True)
    finally:
        new.close()
        if parent:
            parent.close()


def kernel_alone():
    sys.path.insert(0, ROOT)
    import trackiellm_amd as tk
    model = tk.LlmModel(tk.MISTRAL_7B()).fill_synthetic(4)
    sess = tk.LlmSession(model, 1, 64)
    print("the kernel alone, rows x 32000, us per launch (200 launches after a warm-up), beside the lm_head launch of the same width:")
    for rows in (1, 16, 256):
        head_ms, _ = sess.time_gemv(0, 3, rows, 200)
        t0 = tk.time_token_logprobs(rows, 32000, 0, 200)
        t20 = tk.time_token_logprobs(rows, 32000, 20, 200)
        print("  rows %3d   n_top 0: %7.1f   n_top 20: %7.1f   lm_head: %7.1f   (n_top 20 / lm_head = %.2f)" % (rows, 1e3 * t0, 1e3 * t20, 1e3 * head_ms, t20 / head_ms), flush=True)
    sess.close()
    model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-first", action="store_true", help="create the parent library's process before this library's")
    ap.add_argument("--skip-runner", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child()
    if not args.skip_runner:
        runner_rounds(args)
    if not args.skip_kernel:
        kernel_alone()


if __name__ == "__main__":
    main()
