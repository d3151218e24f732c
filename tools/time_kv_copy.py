#!/usr/bin/env python3
"""The prefix cache's copy kernel (k_kv_copy_rows) against the form it replaces, at Mistral-7B cache geometry (developer tool, needs an MI355X):
rows [0, n) of one sequence onto 1 or 64 others, as one launch and as one hipMemcpy2DAsync per (destination, layer, K | V), alternating on one
stream, device events around each.    python tools/time_kv_copy.py [rows,rows,...] [destinations,...] [iterations]
Under `rocprofv3 --kernel-trace --stats -- python tools/time_kv_copy.py ...` the kernel's own durations come out (bytes over them = GB/s)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import trackiellm_amd as tk  # noqa: E402

rows = [int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "430,2000").split(",")]
dsts = [int(v) for v in (sys.argv[2] if len(sys.argv) > 2 else "1,64").split(",")]
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 5
hp = tk.MISTRAL_7B()
model = tk.LlmModel(hp).fill_synthetic(4)
sess = tk.LlmSession(model, max(dsts) + 1, max(max(rows), 64))
print("device CUs:", tk.lib().tk_mi355x_device_cu_count(0), flush=True)
for n in rows:
    for d in dsts:
        k, m, nbytes = sess.time_kv_copy(n, d, iters)
        print(f"{n} rows -> {d} destination(s): {nbytes / 1e9:.3f} GB moved (read + written); k_kv_copy_rows {k:.3f} ms = {nbytes / k / 1e6:.0f} GB/s (1 launch); "
              f"hipMemcpy2DAsync form {m:.3f} ms = {nbytes / m / 1e6:.0f} GB/s ({2 * hp.n_layer * d} calls)", flush=True)
sess.close()
model.close()
