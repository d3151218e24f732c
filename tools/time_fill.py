#!/usr/bin/env python3
"""Load-time work on one MI355X: the synthetic Mistral-7B Q4_K_M fill bench.py performs (k_synth_blocks per matrix, k_repack of each into
W4A8 tiles) and the repack of one 4096 x 4096 matrix per tiled type.

    python tools/time_fill.py [repeats]

The fill is a host clock around fill_synthetic between two device synchronises (the fill only enqueues).  The repack figure is the wall time
of tk_mi355x_llm_repack_probe: allocation, the copy of the blocks in, ONE k_repack launch and the copy of the tiles out, so it bounds the
kernel from above; kernel times proper come from `rocprofv3 --kernel-trace --stats -- python tools/time_fill.py 1` in a run of its own.
Prints one JSON line."""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import trackiellm_amd as tk
from trackiellm_amd import llm as L

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 3
if tk.lib().tk_mi355x_device_count() <= 0:
    sys.exit("time_fill.py needs a HIP device")
hip = ctypes.CDLL("libamdhip64.so")


def sync():
    if hip.hipDeviceSynchronize() != 0:
        sys.exit("hipDeviceSynchronize failed")


res = {"fill_synthetic_mistral_7b_q4_k_m_s": [], "repack_probe_4096x4096_ms": {}}
for _ in range(repeats):
    m = tk.LlmModel(tk.MISTRAL_7B())
    sync()
    t0 = time.perf_counter()
    m.fill_synthetic(4)
    sync()
    res["fill_synthetic_mistral_7b_q4_k_m_s"].append(round(time.perf_counter() - t0, 4))
    m.close()
rng = np.random.default_rng(1)
rows = K = 4096
names = {v: k[5:] for k, v in vars(L).items() if k.startswith("TYPE_") and isinstance(v, int)}
for t in sorted(L.TILE_BYTES):
    blocks = rng.integers(0, 256, rows * K // (32 if t in L.TYPES_OF_32 else 256) * L.BLOCK_BYTES[t], dtype=np.uint8)
    ms = []
    for _ in range(repeats + 1):  # the first call loads the kernel
        t0 = time.perf_counter()
        tk.repack_probe(t, blocks, rows, K)
        ms.append(round((time.perf_counter() - t0) * 1e3, 2))
    res["repack_probe_4096x4096_ms"][names[t]] = ms[1:]
print(json.dumps(res), flush=True)
