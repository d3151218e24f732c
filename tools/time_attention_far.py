#!/usr/bin/env python3
"""k_attention_far beside the resident forms — developer tool, needs an MI355X.  A 7B-geometry session (32 / 8 / 128, 2 layers, 256 sequences) with
a window of 8192 positions, the largest the resident forms take, timed by tk_mi355x_llm_time_attention (the fused decode launch: for the far
form that is k_qkv_rope_append + k_attention_far) in three settings, one session alive at a time:
  resident   what such a session runs today: k_attention_narrow up to 16 rows, k_attention above
  ring       the same under TK_MI355X_NO_NARROW_ATT=1: k_attention at every width
  far        TK_MI355X_ATT_RESIDENT_MAX=64: k_attention_far at every width
over 1 / 16 / 256 rows x 128 / 2048 / 8000 cached positions, TK_FAR_ROUNDS (default 3) interleaved rounds; per cell the median, the far form's
ratio to each resident setting, and K/V bytes per second (algorithmic: rows x positions x n_kv_head x head_dim x 2 B x 2; the far form reads the keys twice,
1.5 x that)."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trackiellm_amd as tk  # noqa: E402

WINDOW = 8192
ROWS, CTXS = (1, 16, 256), (128, 2048, 8000)
SETTINGS = {"resident": {}, "ring": {"TK_MI355X_NO_NARROW_ATT": "1"}, "far": {"TK_MI355X_ATT_RESIDENT_MAX": "64"}}
KNOBS = ("TK_MI355X_NO_NARROW_ATT", "TK_MI355X_ATT_RESIDENT_MAX")
rounds = int(os.environ.get("TK_FAR_ROUNDS", "3"))

hp = tk.MISTRAL_7B()
hp.n_layer = 2
model = tk.LlmModel(hp).fill_synthetic(4)
ms = {(s, r, c): [] for s in SETTINGS for r in ROWS for c in CTXS}
plans = {}
kvb = {}
for _ in range(rounds):
    for name, env in SETTINGS.items():
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
        sess = tk.LlmSession(model, 256, WINDOW)
        for r in ROWS:
            plans[name, r] = tk.attention_plan(r, hp.n_head, hp.n_kv_head, hp.head_dim, WINDOW, True)
            for c in CTXS:
                t, b = sess.time_attention(r, c, 8 if r * c > 500000 else 64)
                ms[name, r, c].append(t)
                kvb[r, c] = b
        sess.close()
print("window %d, %d rounds; plan (kernel, query heads per workgroup, positions per slot, slots) per setting and width:" % (WINDOW, rounds))
for name in SETTINGS:
    print("  %-8s %s" % (name, "  ".join("%d rows %s" % (r, plans[name, r]) for r in ROWS)))
print("%5s %6s | %12s %12s %12s | %9s %9s | %s" % ("rows", "ctx", "resident us", "ring us", "far us", "far/res", "far/ring", "K/V GB/s resident, ring, far (far's own bytes: x 1.5)"))
for r in ROWS:
    for c in CTXS:
        m = {s: statistics.median(ms[s, r, c]) for s in SETTINGS}
        gb = {s: kvb[r, c] / m[s] / 1e6 for s in SETTINGS}
        print("%5d %6d | %12.1f %12.1f %12.1f | %9.2f %9.2f | %.0f, %.0f, %.0f (%.0f)" %
              (r, c, 1000 * m["resident"], 1000 * m["ring"], 1000 * m["far"], m["far"] / m["resident"], m["far"] / m["ring"], gb["resident"], gb["ring"], gb["far"], 1.5 * gb["far"]))
model.close()
