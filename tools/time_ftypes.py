#!/usr/bin/env python3
"""The k-quant recipes against Q4_K_M on the MI355X (developer tool, needs the GPU): full synthetic Mistral-7B models in the named
recipes, all resident in one process and timed INTERLEAVED: every repeat walks the widths 16, 64, 128 and 256 rows and, per width, every
recipe in turn, so a drift of the machine lands on all recipes alike.
Per recipe: the weight bytes a decode step streams and the stand-alone gate | up mat-vec of layer 0 at 16 rows (tk_mi355x_llm_time_gemv:
weight bytes plus activation and slab bytes over kernel time).  Per width and recipe: the median decode-step time over the repeats (a
32-token prompt per sequence, 4 warm-up steps, then greedy steps through the captured pass, HIP events around the loop) and its ratio to
Q4_K_M's median; for Q4_K_M also the spread of its repeats, the yardstick for every ratio beside it.
The float recipes (F16, BF16, F32: every matrix and token_embd in the type, on the exact fp32 MFMA GEMM) have no W4A8 mat-vec to time alone; with
F16 among the recipes, BF16 and F32 are also printed as ratios to F16's median; TQ1_0 and TQ2_0 also as ratios to Q2_K's and to each other's.
    python tools/time_ftypes.py [steps [repeats [recipe ...]]]      recipes: TQ1_0 TQ2_0 IQ4_NL IQ4_XS Q4_0 Q4_1 Q5_0 Q5_1 Q8_0 Q2_K Q2_K_S Q3_K_S Q3_K_M Q4_K_S Q5_K_S Q5_K_M F16 BF16 F32"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trackiellm_amd as tk  # noqa: E402

FTYPES = {"TQ1_0": tk.FTYPE_TQ1_0, "TQ2_0": tk.FTYPE_TQ2_0, "IQ4_NL": tk.FTYPE_IQ4_NL, "IQ4_XS": tk.FTYPE_IQ4_XS, "Q4_0": tk.FTYPE_Q4_0, "Q5_0": tk.FTYPE_Q5_0, "Q8_0": tk.FTYPE_Q8_0, "Q2_K": tk.FTYPE_Q2_K, "Q2_K_S": tk.FTYPE_Q2_K_S, "Q3_K_S": tk.FTYPE_Q3_K_S, "Q3_K_M": tk.FTYPE_Q3_K_M, "Q4_K_S": tk.FTYPE_Q4_K_S,
          "Q4_K_M": tk.FTYPE_Q4_K_M, "Q5_K_S": tk.FTYPE_Q5_K_S, "Q5_K_M": tk.FTYPE_Q5_K_M}
TTYPES = {"Q4_1": tk.TYPE_Q4_1, "Q5_1": tk.TYPE_Q5_1}  # recipes by tensor type (fill_synthetic_type): no file type of fill_synthetic makes them
FLOATS = {"F16": tk.TYPE_F16, "BF16": tk.TYPE_BF16, "F32": tk.TYPE_F32}  # the float checkpoint recipes (fill_synthetic(f16=True), fill_synthetic_float)
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 32
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
names = ["Q4_K_M"] + [n for n in (sys.argv[3:] or ["Q5_K_M", "Q3_K_S", "Q3_K_M", "Q2_K", "Q2_K_S"]) if n != "Q4_K_M"]
for n in names:
    if n not in FTYPES and n not in TTYPES and n not in FLOATS:
        sys.exit(f"unknown recipe {n}; known: {' '.join(list(FTYPES) + list(TTYPES) + list(FLOATS))}")
wb = tk.lib().tk_mi355x_llm_model_weight_bytes
wb.restype = C.c_uint64
WIDTHS = (16, 64, 128, 256)

models, nbytes = {}, {}
for name in names:
    model = tk.LlmModel(tk.MISTRAL_7B(), device=0)
    if name in FLOATS:
        models[name] = model.fill_synthetic(4, f16=True) if name == "F16" else model.fill_synthetic_float(4, FLOATS[name])
    else:
        models[name] = model.fill_synthetic_type(4, TTYPES[name]) if name in TTYPES else model.fill_synthetic(4, ftype=FTYPES[name])
    nbytes[name] = wb(models[name].h)
    print(f"{name}: {nbytes[name] / 1e9:.3f} GB of weights streamed per decode step, x{nbytes[name] / nbytes['Q4_K_M']:.3f} of Q4_K_M", flush=True)

ms = {(n, r): [] for n in names for r in WIDTHS}
for rep in range(repeats):
    for rows in WIDTHS:
        for name in names:
            model = models[name]
            sess = tk.LlmSession(model, rows, 32 + steps + 16)
            prompts = np.random.default_rng(1).integers(3, model.hparams.vocab, (rows, 32)).astype(np.int32)
            prompts[:, 0] = 1
            sess.prefill(prompts)
            sess.decode(rows, 4)
            _, t = sess.decode(rows, steps)
            ms[(name, rows)].append(t)
            if rows == 16 and rep == 0 and name not in FLOATS:
                gms, gbytes = sess.time_gemv(0, 0, 16, 50)
                print(f"{name} ffn_gate|up mat-vec, layer 0, 16 rows: {gms * 1e3:.1f} us, {gbytes / gms / 1e9:.2f} TB/s = {gbytes / gms / 1e9 / 8:.3f} of 8 TB/s",
                      flush=True)
            sess.close()

for rows in WIDTHS:
    base = float(np.median(ms[("Q4_K_M", rows)]))
    for name in names:
        v = ms[(name, rows)]
        med = float(np.median(v))
        tail = (f", repeats {min(v):.3f} .. {max(v):.3f} ms: spread {100 * (max(v) - min(v)) / med:.1f} % of the median" if name == "Q4_K_M"
                else f", x{med / base:.3f} of Q4_K_M (repeats x{min(v) / base:.3f} .. x{max(v) / base:.3f})")
        if name in ("BF16", "F32") and "F16" in names:
            f16 = ms[("F16", rows)]
            fm = float(np.median(f16))
            tail += f"; x{med / fm:.3f} of F16 (F16's repeats span {100 * (max(f16) - min(f16)) / fm:.1f} % of its median)"
        if name in ("TQ1_0", "TQ2_0"):  # against the nearest 2-bit type of the same run, and TQ1_0 (installed as TQ2_0 tiles) against TQ2_0
            for other in ("Q2_K", "TQ2_0"):
                if other in names and other != name:
                    o = ms[(other, rows)]
                    om = float(np.median(o))
                    tail += f"; x{med / om:.3f} of {other} ({other}'s repeats span {100 * (max(o) - min(o)) / om:.1f} % of its median)"
        print(f"{name} {rows:3d} rows: {med:.3f} ms per decode step (median of {repeats}), weights at {nbytes[name] / med / 1e9:.2f} TB/s{tail}", flush=True)
for m in models.values():
    m.close()
