#!/usr/bin/env python3
"""What a context shift costs, and what it replaces, at Mistral-7B cache geometry (developer tool, needs an MI355X); writes profiles/context_shift.txt.

    python tools/time_kv_shift.py [--parent DIR] [--also NAME=DIR[=WHAT] ...] [--out FILE] [--rounds 4] [--bench-rounds 4]

Context 4096, n_keep 64: the runner shifts at n_past 4095, drops (4095 - 64) / 2 = 2015 rows and moves rows [2079, 4095) down by 2015, which leaves
2080 tokens in the context.
  (a) device-event time of that one launch of k_kv_shift_rows after a warm-up; bytes read + written from the shapes; the copy rate they give
  (b) what a host pays today instead: prepare_generation of a 2080-token prompt — with --parent, measured on that checkout (the commit before the
      feature, built), otherwise on this one (the prompt path is the same code)
  (c) one runner's tok/s with the policy off (tools/time_b1.py), this checkout against --parent, alternating, the order rotated every round,
      `rounds` rounds (TK_B1_TOKENS in the environment sets the tokens timed per run); --also NAME=DIR=WHAT adds further built checkouts to the
      rotation (the parent plus a part of the change: which part costs what); WHAT, a sentence on what the build holds, goes into the file
  (d) bench.py --gpus 1 --steps 8 --warmup 2, this checkout against --parent, the order swapped every round, --bench-rounds rounds
(c) and (d) need --parent; every child is a fresh process, one at a time."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTX, N_KEEP = 4096, 64
N_PAST = CTX - 1
N_DISCARD = (N_PAST - N_KEEP) // 2
SURVIVE = N_PAST - N_DISCARD


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def prepare_child():
    """child of (b): the time of prepare_generation with SURVIVE tokens, three prompts that differ from their first byte, after one short warm-up"""
    sys.path.insert(0, os.getcwd())
    import trackiellm_amd as tk
    loader = tk.ModelLoader()
    h = loader.load("synthetic://mistral-7b?seed=4")
    runner = tk.LlmRunner(h, context_size=CTX)
    runner.prepare("warm up " * 40)
    out = []
    for i in range(3):
        prompt = (chr(65 + i) + "the user is in a room. " * 100)[:SURVIVE - 1]  # ids = BOS + bytes
        t = time.time()
        runner.prepare(prompt)
        out.append(1000 * (time.time() - t))
    print("PREPARE_MS " + json.dumps(out), flush=True)
    runner.close()
    loader.unload(h)
    loader.close()


def run(cwd, argv, want):
    """a fresh python in `cwd`; returns the last output line that starts with `want`"""
    p = subprocess.run([sys.executable] + argv, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    for line in reversed(p.stdout.splitlines()):
        if line.startswith(want):
            print("[%s] %s" % (cwd, line[:200]), flush=True)
            return line
    raise RuntimeError("%s in %s: no line starts with %r\n%s" % (argv, cwd, want, p.stdout[-2000:]))


def main():
    parent = arg("--parent", None)
    out_path = arg("--out", os.path.join(ROOT, "profiles", "context_shift.txt"))
    rounds = int(arg("--rounds", "4"))
    sys.path.insert(0, ROOT)
    import trackiellm_amd as tk
    lines = ["Context shift (csrc/common/tk_kv_shift.h, k_kv_shift_rows) — measurements, 1 x MI355X (%d CUs), synthetic Mistral-7B Q4_K_M." % tk.lib().tk_mi355x_device_cu_count(0),
             "Written by tools/time_kv_shift.py.  Context %d, n_keep %d: the shift at n_past %d drops %d rows and moves rows [%d, %d) down, %d tokens survive." %
             (CTX, N_KEEP, N_PAST, N_DISCARD, N_KEEP + N_DISCARD, N_PAST, SURVIVE), ""]
    hp = tk.MISTRAL_7B()
    model = tk.LlmModel(hp).fill_synthetic(4)
    sess = tk.LlmSession(model, 1, CTX)
    # a fresh cache is all zeros, on which both f16 conversions leave through their first branch: time the move on keys and values as a model
    # writes them (seeded, normal f16 range, std 1, every sign and exponent mixed within a wave), another draw per layer
    rng = np.random.default_rng(4)
    for layer in range(hp.n_layer):
        k = rng.standard_normal((N_PAST, hp.n_kv_head, hp.head_dim), dtype=np.float32).astype(np.float16).view(np.uint16)
        v = rng.standard_normal((N_PAST, hp.n_kv_head, hp.head_dim), dtype=np.float32).astype(np.float16).view(np.uint16)
        sess.kv_write(layer, 0, 0, k, v)
    ms, nbytes = sess.time_kv_shift(0, N_KEEP + N_DISCARD, N_PAST, -N_DISCARD, 20)
    want_bytes = 2 * 2 * hp.n_layer * hp.n_kv_head * (N_PAST - N_KEEP - N_DISCARD) * hp.head_dim * 2
    assert nbytes == want_bytes
    lines += ["(a) one launch (device events, 20 launches after a warm-up; the cache holds seeded normal f16 values, std 1, in rows [0, %d)): %.4f ms; %d layers x %d KV heads x (K, V) x %d rows x %d f16, read + written = %.3f GB;" %
              (N_PAST, ms, hp.n_layer, hp.n_kv_head, N_PAST - N_KEEP - N_DISCARD, hp.head_dim, nbytes / 1e9),
              "    as a copy rate %.0f GB/s = %.1f %% of the 8 TB/s roofline (%d workgroups: one per (layer, KV head, K | V) run, because a run's source and destination"
              % (nbytes / ms / 1e6, 100 * nbytes / ms / 1e6 / 8000, 2 * hp.n_layer * hp.n_kv_head),
              "    may overlap and nothing orders two workgroups)", ""]
    sess.close()
    model.close()
    where = parent or ROOT
    got = run(where, [os.path.abspath(__file__), "--prepare-child"], "PREPARE_MS ")
    prep = json.loads(got[len("PREPARE_MS "):])
    lines += ["(b) what a host pays today instead — tk_llm_runner_prepare_generation of a %d-token prompt at context_size %d, host clock, %s:" %
              (SURVIVE, CTX, "on the parent commit" if parent else "on this commit (no --parent given)"),
              "    " + ", ".join("%.1f ms" % v for v in prep) + "   (three prompts that differ from their first byte, after a short warm-up prompt)",
              "    a shift is %.0f times cheaper than the quickest of them" % (min(prep) / ms), ""]
    if parent:
        both = (("parent", parent), ("this", ROOT))
        # --also NAME=DIR (repeatable): further built checkouts timed in the same rotation, e.g. the parent plus a part of the change
        also = [(sys.argv[i + 1].split("=", 2) + [""])[:3] for i, a in enumerate(sys.argv) if a == "--also"]
        builds = (both[0],) + tuple((n, d) for n, d, _ in also) + (both[1],)
        lines += ["The builds below: `parent` is the commit before the feature, `this` the feature's commit, policy never set."]
        lines += ["    `%s`: %s" % (n, what or "(no description given)") for n, _, what in also] + [""]
        b1 = {name: [] for name, _ in builds}
        for r in range(rounds):  # the order rotates every round, so that no build always follows the same one
            row = []
            for i in range(len(builds)):
                name, cwd = builds[(i + r) % len(builds)]
                line = run(cwd, ["tools/time_b1.py"], "one runner:")
                b1[name].append(float(line.split(" ms per token, ")[1].split(" tok/s")[0]))
                row.append("%s %.1f" % (name, b1[name][-1]))
            lines.append("round %2d, tok/s in the order run:   %s" % (r + 1, "   ".join(row)))
        lines += ["", "(c) one runner, policy off, %s tokens timed per run, tok/s over the %d rounds:" % (os.environ.get("TK_B1_TOKENS", "128"), rounds)]
        for name, _ in builds:
            v = sorted(b1[name])
            mean = sum(v) / len(v)
            sd = (sum((x - mean) ** 2 for x in v) / max(1, len(v) - 1)) ** 0.5
            lines.append("    %-8s min %.1f   max %.1f   median %.1f   mean %.2f   standard error of the mean %.2f" %
                         (name, v[0], v[-1], (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2, mean, sd / len(v) ** 0.5))
        lines.append("")
        bench = {"parent": [], "this": []}
        bench_rounds = int(arg("--bench-rounds", "4"))
        for r in range(bench_rounds):
            for name, cwd in (both if r % 2 == 0 else both[::-1]):
                line = run(cwd, ["bench.py", "--gpus", "1", "--steps", "8", "--warmup", "2"], "{")
                bench[name].append(json.loads(line)["value"])
        lines.append("(d) bench.py --gpus 1 --steps 8 --warmup 2, %d rounds, the order swapped every round (cycles/s):" % bench_rounds)
        for name in ("parent", "this"):
            v = bench[name]
            lines.append("    %-8s %s   min %.2f   max %.2f   mean %.2f" % (name, ", ".join("%.2f" % x for x in v), min(v), max(v), sum(v) / len(v)))
    else:
        lines.append("(c), (d): not measured (no --parent checkout given)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    if "--prepare-child" in sys.argv:
        prepare_child()
    else:
        main()
