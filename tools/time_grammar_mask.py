#!/usr/bin/env python3
"""Grammar masks built on the device (k_grammar_mask, csrc/common/tk_grammar_walk.h) — developer tool, needs an MI355X.

    python tools/time_grammar_mask.py [--rounds 4] [--skip-runner] [--parent-lib /path/to/the/parent/commit's/libtrackie_mi355x.so] [--parent-first]
                                      [--brace-bias -3]

1. The launch alone (tk_mi355x_time_grammar_mask): 1 and 5 rows x the 32 000 pieces of the synthetic 7B vocabulary under the tool-call grammar at four
   states — white space, inside a string, after "{", complete.  The device path is the state upload plus the launch, 200 rounds between two events;
   beside it, in the same process, the host's TkGrammarState::mask for the same state (one row; a pass of n rows pays n of them).
2. ONE runner on full synthetic 7B under the tool grammar, 256 tokens per generation, at a short context and over ~2 100 cached positions, as
   tools/time_lookup.py --grammar --brace-bias B runs it.  Configurations, interleaved round by round in one call, their order rotated every round:
       parent      the parent commit's library (only with --parent-lib), the runner as it was
       off         this library, device mask off
       on          this library, device mask on
       on+lookup   device mask on, lookup (4, 1, 3) inside the grammar scope with the plain run's own ids as prediction
       off+lookup  the same lookup with host masks
   Each library lives in a child process of its own that keeps its model; the driver alternates between them.  A window is the generate_next_token
   loop alone, host clock.  The ids of all configurations must be equal."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOKENS = 256
PATH = "synthetic://mistral-7b?seed=4"
VOCAB = 32000
CONTEXTS = {"short": 16, "long": 2100}
STATES = {"white space": '{ \n', "inside a string": '{"tool_call":{"name":"ab', 'after "{"': "{", "complete": "{}"}


def prompt_of(n):
    words = ["scene", "door", "left", "person", "two", "metres", "table", "ahead", "chair", "right", "clear", "path"]
    out, i = [], 0
    while sum(len(w) + 1 for w in out) < n:
        out.append(words[(i * 7 + i // 5) % len(words)])
        i += 1
    return " ".join(out)[:n]


def synthetic_pieces():
    """the pieces of a synthetic model's tokenizer: ids 3 .. 258 are the bytes, 0 .. 2 have none, the others read " t<id>" """
    return [bytes([i - 3]) if 3 <= i < 259 else b"" if i < 3 else (" t%d" % i).encode() for i in range(VOCAB)]


def launch_alone():
    sys.path.insert(0, ROOT)
    import trackiellm_amd as tk
    pieces = synthetic_pieces()
    print("the launch alone, %d tokens (ms; device = state upload + launch, host = TkGrammarState::mask for one row):" % VOCAB)
    for name, prefix in STATES.items():
        for rows in (1, 5):
            dev, host = tk.time_grammar_mask(prefix, pieces, rows=rows, eos=2, iters=200)
            print("  %-16s %d row%s   device %.4f   host %.3f per row, %.3f for the pass   (%.0f x)" %
                  (name, rows, " " if rows == 1 else "s", dev, host, host * rows, host * rows / dev), flush=True)


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
        runner = tk.LlmRunner(handle, context_size=4096, random_seed=11)
        if cmd.get("brace_bias") is not None:
            runner.set_logit_bias([3 + ord("}")], [cmd["brace_bias"]])
        if "lookup" in cmd:
            runner.set_lookup(*cmd["lookup"])
            runner.set_prediction(cmd["prediction"])
            runner.set_lookup_scope_bits(15)
        if "device_mask" in cmd:  # the parent library has no such entry: it is never sent one
            runner.set_device_mask(cmd["device_mask"])
        runner.prepare(prompt_of(cmd["prompt_bytes"]), use_tool_grammar=True)
        n = 0
        t0 = time.perf_counter()
        while n < TOKENS:
            p = runner.next_token()
            if p is None or p == "<tool_call>":
                break
            n += 1
        dt = time.perf_counter() - t0
        stats = runner.mask_stats() if "device_mask" in cmd else (0, 0, 0)
        print(json.dumps({"tokens": n, "seconds": dt, "ids": runner.recent_tokens(), "mask_stats": stats}), flush=True)
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


def runner(args):
    parent = Child(args.parent_lib) if args.parent_lib and args.parent_first else None
    new = Child(None)
    if args.parent_lib and not parent:
        parent = Child(args.parent_lib)
    try:
        base = dict(brace_bias=args.brace_bias)
        for name, nbytes in CONTEXTS.items():
            plain = new.run(prompt_bytes=nbytes, device_mask=False, **base)  # warm-up of the plain passes, and the prediction
            ids = plain["ids"][:plain["tokens"]]
            look = dict(lookup=(4, 1, 3), prediction=ids)
            configs = {"off": dict(device_mask=False), "on": dict(device_mask=True), "on+lookup": dict(device_mask=True, **look), "off+lookup": dict(device_mask=False, **look)}
            for cfg in configs.values():
                cfg.update(base)
                new.run(prompt_bytes=nbytes, **cfg)  # warm-up: the verify passes' graphs, the vocabulary and grammar images
            if parent:
                parent.run(prompt_bytes=nbytes, **base)
            rates = {k: [] for k in (["parent"] if parent else []) + list(configs)}
            last = {}
            order = list(rates)
            for rnd in range(args.rounds):
                for k in order[rnd % len(order):] + order[:rnd % len(order)]:
                    r = parent.run(prompt_bytes=nbytes, **base) if k == "parent" else new.run(prompt_bytes=nbytes, **configs[k])
                    assert r["ids"] == plain["ids"], "%s: ids differ from the plain run" % k
                    rates[k].append(r["tokens"] / r["seconds"])
                    last[k] = r
            print("%s context (%d prompt tokens, %d tokens generated):" % (name, nbytes + 1, plain["tokens"]))
            for k, v in rates.items():
                m = last[k]["mask_stats"]
                print("  %-10s %s tok/s   range %.0f - %.0f   mask rows: %d device, %d host, %d requests redone" %
                      (k, " ".join("%.0f" % x for x in v), min(v), max(v), m[0], m[1], m[2]), flush=True)
    finally:
        new.close()
        if parent:
            parent.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-first", action="store_true", help="create the parent library's process before this library's")
    ap.add_argument("--skip-runner", action="store_true")
    ap.add_argument("--skip-launch", action="store_true")
    ap.add_argument("--brace-bias", type=float, default=-3.0)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child()
    if not args.skip_launch:
        # in a child of its own: the runner part starts its processes from one that has not opened the device
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--launch-only"])
    if not args.skip_runner:
        runner(args)


if __name__ == "__main__":
    if "--launch-only" in sys.argv:
        launch_alone()
    else:
        main()
