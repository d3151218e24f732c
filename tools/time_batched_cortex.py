#!/usr/bin/env python3
"""K cortex handles on one model file, one data-dependent cycle each through tk_cortex_* only (bench.py: reference_abi_batched_cortex) —
developer tool, needs an MI355X.    python tools/time_batched_cortex.py 16,64,256 [tokens per cycle] [--progress] [--prefix-cache]
--prefix-cache (default off) switches the model's prompt prefix cache on through the model handle before the cortices are created (they find the
same resident model) and prints the model's prefix_cache_stats beside each timing."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import trackiellm_amd as tk  # noqa: E402
import bench  # noqa: E402

progress = "--progress" in sys.argv
prefix_cache = "--prefix-cache" in sys.argv
argv = [a for a in sys.argv[1:] if a not in ("--progress", "--prefix-cache")]
ks = [int(v) for v in (argv[0] if argv else "16,64").split(",")]
N = int(argv[1]) if len(argv) > 1 else 128
for K in ks:
    # the handle the cortices' own loaders will find (models are shared per path and device): the cache is switched through it.  Held for one K
    # only, so that every K starts from a fresh model and one shared session of its own size, as without this handle
    loader = tk.ModelLoader()
    h = loader.load("synthetic://mistral-7b?seed=4")
    tk.ModelLoader.set_prefix_cache(h, prefix_cache)
    res = bench.reference_abi_batched_cortex(tk, K, N, progress=progress)
    res["prefix_cache"] = dict(zip(("on", "prompt_rows", "kept", "copied", "copy_launches"), (prefix_cache,) + tk.ModelLoader.prefix_cache_stats(h)))
    print(json.dumps(res), flush=True)
    loader.unload(h)
    loader.close()
