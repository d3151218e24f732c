#!/usr/bin/env python3
"""Lookup decoding behind tk_llm_runner_*: ONE runner on full synthetic 7B, 256 tokens per generation, at a short context and over ~2 100 cached
positions — developer tool, needs an MI355X.

    python tools/time_lookup.py [--rounds 4] [--parent-lib /path/to/the/parent/commit's/libtrackie_mi355x.so]

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
    runner = tk.LlmRunner(handle, context_size=4096)
    print(json.dumps({"ready": True}), flush=True)
    for line in sys.stdin:
        cmd = json.loads(line)
        if cmd.get("quit"):
            break
        if "lookup" in cmd:
            runner.set_lookup(*cmd["lookup"])
            runner.set_prediction(cmd["prediction"])
        runner.prepare(prompt_of(cmd["prompt_bytes"]))
        n = 0
        t0 = time.perf_counter()
        while n < TOKENS and runner.next_token() is not None:
            n += 1
        dt = time.perf_counter() - t0
        stats = runner.lookup_stats() if "lookup" in cmd else (0, 0, 0)
        print(json.dumps({"tokens": n, "seconds": dt, "ids": runner.recent_tokens(), "stats": stats}), flush=True)
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
        for name, nbytes in CONTEXTS.items():
            plain = new.run(prompt_bytes=nbytes)  # warm-up of the plain passes, and the prediction
            ids = plain["ids"][:plain["tokens"]]
            seen = set(plain["ids"]) | set(3 + b for b in prompt_of(nbytes).encode()) | {1, 2}
            never = [t for t in range(300, 2000) if t not in seen][:64]
            configs = {"off": dict(lookup=(0, 1, 3), prediction=[]), "cost": dict(lookup=(4, 1, 3), prediction=never), "ceiling": dict(lookup=(4, 1, 3), prediction=ids)}
            for cfg in configs.values():
                new.run(prompt_bytes=nbytes, **cfg)  # warm-up: the verify passes' graphs
            if parent:
                parent.run(prompt_bytes=nbytes)
            rates = {k: [] for k in (["parent"] if parent else []) + list(configs)}
            last = {}
            order = list(rates)
            for rnd in range(args.rounds):
                for k in order[rnd % len(order):] + order[:rnd % len(order)]:  # the order rotates: no configuration always follows the same one
                    r = parent.run(prompt_bytes=nbytes) if k == "parent" else new.run(prompt_bytes=nbytes, **configs[k])
                    assert r["ids"] == plain["ids"], "%s: ids differ from the plain run" % k
                    rates[k].append(r["tokens"] / r["seconds"])
                    last[k] = r
            print("%s context (%d prompt tokens, %d tokens generated):" % (name, nbytes + 1, plain["tokens"]))
            for k, v in rates.items():
                s = last.get(k, {}).get("stats", (0, 0, 0))
                print("  %-8s %s tok/s   range %.0f - %.0f   verify passes %d, drafted %d, accepted %d" %
                      (k, " ".join("%.0f" % x for x in v), min(v), max(v), s[0], s[1], s[2]), flush=True)
    finally:
        new.close()
        if parent:
            parent.close()


if __name__ == "__main__":
    main()
