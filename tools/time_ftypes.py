#!/usr/bin/env python3
"""The k-quant recipes against Q4_K_M on the MI355X (developer tool, needs the GPU): full synthetic Mistral-7B in the Q4_K_M, Q5_K_M,
Q3_K_S and Q3_K_M recipes, one after the other in one process.
Per recipe: the weight bytes a decode step streams, the decode-step time at 16, 64, 128 and 256 rows (a 32-token prompt per sequence, then greedy steps through the captured
pass, HIP events around the loop), and the stand-alone gate | up mat-vec of layer 0 at 16 rows (tk_mi355x_llm_time_gemv: weight bytes
plus activation and slab bytes over kernel time), so each type's mat-vec rate stands beside the Q4_K one.
    python tools/time_ftypes.py [steps]"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trackiellm_amd as tk  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 32
wb = tk.lib().tk_mi355x_llm_model_weight_bytes
wb.restype = C.c_uint64
base = {}
base_bytes = 0
for name, ftype in (("Q4_K_M", tk.FTYPE_Q4_K_M), ("Q5_K_M", tk.FTYPE_Q5_K_M), ("Q3_K_S", tk.FTYPE_Q3_K_S), ("Q3_K_M", tk.FTYPE_Q3_K_M)):
    model = tk.LlmModel(tk.MISTRAL_7B(), device=0).fill_synthetic(4, ftype=ftype)
    nbytes = wb(model.h)
    base_bytes = base_bytes if name != "Q4_K_M" else nbytes
    print(f"{name}: {nbytes / 1e9:.3f} GB of weights streamed per decode step, x{nbytes / base_bytes:.3f} of Q4_K_M", flush=True)
    for rows in (16, 64, 128, 256):
        sess = tk.LlmSession(model, rows, 32 + steps + 16)
        prompts = np.random.default_rng(1).integers(3, model.hparams.vocab, (rows, 32)).astype(np.int32)
        prompts[:, 0] = 1
        sess.prefill(prompts)
        sess.decode(rows, 4)
        _, ms = sess.decode(rows, steps)
        rel = f", x{ms / base[rows]:.3f} of Q4_K_M" if rows in base and name != "Q4_K_M" else ""
        base.setdefault(rows, ms)
        print(f"{name} {rows:3d} rows: {ms:.3f} ms per decode step, weights at {nbytes / ms / 1e9:.2f} TB/s{rel}", flush=True)
        if rows == 16:
            gms, gbytes = sess.time_gemv(0, 0, 16, 50)
            print(f"{name} ffn_gate|up mat-vec, layer 0, 16 rows: {gms * 1e3:.1f} us, {gbytes / gms / 1e9:.2f} TB/s = {gbytes / gms / 1e9 / 8:.3f} of 8 TB/s",
                  flush=True)
        sess.close()
    model.close()
