#!/usr/bin/env python3
"""Lookup decoding behind tk_llm_runner_*: ONE runner on full synthetic 7B, 256 tokens per generation, at a short context and over ~2 100 cached
positions — developer tool, needs an MI355X.

    python tools/time_lookup.py [--rounds 4] [--parent-lib /path/to/the/parent/commit's/libtrackie_mi355x.so]
                                [--temperature 0.7] [--grammar] [--brace-bias B]

--temperature T (> 0) runs the reference's runner: temperature T with the default chain, seed 11; --grammar arms the tool-call grammar; both put the
lookup configurations inside the runner's scope (tk_mi355x_llm_runner_set_lookup_scope), "off" being lookup on with scope 0.  --brace-bias adds a
logit bias on the closing brace (a synthetic model under the grammar either closes its call at once or never).  With a scope the tool also prints the
host time spent building the per-row masks beside the time spent in the verify requests (tk_mi355x_llm_runner_lookup_host_ms).

Configurations, interleaved round by round in one call, their order rotated every round:
    parent    the parent commit's library (only with --parent-lib), the runner as it was
    off       this library, lookup off
    cost      lookup (4, 1, 3) with a prediction that never matches: what a host pays that predicts wrongly
    ceiling   lookup (4, 1, 3) with the plain run's own ids as prediction: every draft right
Each library lives in a child process of its own (a process loads one library) that keeps its model and runner; the driver alternates between
them.  A window is the generate_next_token loop alone (prepare_generation is outside it), host clock; every call ends in a stream synchronise.
Prints tok/s per round and the range per configuration; the ids of all configurations must be equal."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOKENS = 256
PATH = "synthetic://mistral-7b?seed=4"
CONTEXTS = {"short": 16, "long": 2100}  # prompt bytes: a synthetic model tokenises bytes


def prompt_of(n):
    words = ["scene", "door", "left", "person", "two", "metres", "table", "ahead", "chair", "right", "clear", "path"]
    out, i = [], 0
    while sum(len(w) + 1 for w in out) < n:
        out.append(words[(i * 7 + i // 5) % len(words)])
        i += 1
    return " ".join(out)[:n]


def child():
    sys.path.insert(0, ROOT)
    import trackiellm_amd as tk
    loader = tk.ModelLoader()
    handle = loader.load(PATH, force_reload=True)
    print(json.dumps({"ready": True}), flush=True)
    for line in sys.stdin:
        cmd = json.loads(line)
        if cmd.get("quit"):
            break
        # a runner per generation: the sampling counter counts from the runner's creation, so every generation draws the same stream; the session,
        # its cache and its graphs belong to the model and stay
        runner = tk.LlmRunner(handle, context_size=4096, random_seed=11)
        if cmd.get("temperature", 0.0) > 0.0:
            runner.set_sampling(cmd["temperature"])
        if cmd.get("brace_bias") is not None:
            runner.set_logit_bias([3 + ord("}")], [cmd["brace_bias"]])
        if "lookup" in cmd:
            runner.set_lookup(*cmd["lookup"])
            runner.set_prediction(cmd["prediction"])
            if "scope" in cmd:  # the parent library has no scope: it is never sent one
                runner.set_lookup_scope_bits(cmd["scope"])
        runner.prepare(prompt_of(cmd["prompt_bytes"]), use_tool_grammar=bool(cmd.get("grammar")))
        n = 0
        t0 = time.perf_counter()
        while n < TOKENS:
            p = runner.next_token()
            if p is None or p == "<tool_call>":
                break
            n += 1
        dt = time.perf_counter() - t0
        stats = runner.lookup_stats() if "lookup" in cmd else (0, 0, 0)
        host = runner.lookup_host_ms() if "scope" in cmd else (0.0, 0.0)
        print(json.dumps({"tokens": n, "seconds": dt, "ids": runner.recent_tokens(), "stats": stats, "host_ms": host}), flush=True)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-first", action="store_true", help="create the parent library's process before this library's")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--temperature", type=float, default=0.0)
    ap.add_argument("--grammar", action="store_true")
    ap.add_argument("--brace-bias", type=float, default=None)
    args = ap.parse_args()
    if args.child:
        return child()
    # two processes of ONE library differ by a fraction of a per cent (where each one's weights and cache land): --parent-first swaps which of the two
    # is created first, so that an offset that follows the process can be told from one that follows the library
    parent = Child(args.parent_lib) if args.parent_lib and args.parent_first else None
    new = Child(None)
    if args.parent_lib and not parent:
        parent = Child(args.parent_lib)
    try:
        base = dict(temperature=args.temperature, grammar=args.grammar, brace_bias=args.brace_bias)
        scoped = args.temperature > 0.0 or args.grammar or args.brace_bias is not None
        scope = dict(scope=15) if scoped else {}
        for name, nbytes in CONTEXTS.items():
            plain = new.run(prompt_bytes=nbytes, **base)  # warm-up of the plain passes, and the prediction
            ids = plain["ids"][:plain["tokens"]]
            seen = set(plain["ids"]) | set(3 + b for b in prompt_of(nbytes).encode()) | {1, 2}
            never = [t for t in range(300, 2000) if t not in seen][:64]
            configs = {"off": dict(lookup=(0, 1, 3), prediction=[]), "cost": dict(lookup=(4, 1, 3), prediction=never, **scope), "ceiling": dict(lookup=(4, 1, 3), prediction=ids, **scope)}
            if scoped:  # scope off: lookup on, the scope 0 — the runner is inactive, as it was before the scope existed
                configs["off"] = dict(lookup=(4, 1, 3), prediction=ids, scope=0)
            for cfg in configs.values():
                cfg.update(base)
                new.run(prompt_bytes=nbytes, **cfg)  # warm-up: the verify passes' graphs
            if parent:
                parent.run(prompt_bytes=nbytes, **base)
            rates = {k: [] for k in (["parent"] if parent else []) + list(configs)}
            last = {}
            order = list(rates)
            for rnd in range(args.rounds):
                for k in order[rnd % len(order):] + order[:rnd % len(order)]:  # the order rotates: no configuration always follows the same one
                    r = parent.run(prompt_bytes=nbytes, **base) if k == "parent" else new.run(prompt_bytes=nbytes, **configs[k])
                    assert r["ids"] == plain["ids"], "%s: ids differ from the plain run" % k
                    rates[k].append(r["tokens"] / r["seconds"])
                    last[k] = r
            print("%s context (%d prompt tokens, %d tokens generated):" % (name, nbytes + 1, plain["tokens"]))
            for k, v in rates.items():
                s = last.get(k, {}).get("stats", (0, 0, 0))
                h = last.get(k, {}).get("host_ms", (0.0, 0.0))
                print("  %-8s %s tok/s   range %.0f - %.0f   verify passes %d, drafted %d, accepted %d%s" %
                      (k, " ".join("%.0f" % x for x in v), min(v), max(v), s[0], s[1], s[2],
                       "   masks %.2f ms beside %.2f ms in the requests (%.3f / %.3f per pass)" % (h[0], h[1], h[0] / max(s[0], 1), h[1] / max(s[0], 1)) if scoped and s[0] else ""), flush=True)
    finally:
        new.close()
        if parent:
            parent.close()


if __name__ == "__main__":
    main()
