#!/usr/bin/env python3
"""The verify pass of lookup decoding on full synthetic 7B: k_attention_prefill's tiles (form 2) against the run form of the long-context attention
(form 4), forced through LlmSession.forward_verify's `form` argument — developer tool, needs an MI355X.

    python tools/time_verify_forms.py [rounds] [calls per window]

Rows 2, 5 and 8 of ONE sequence at contexts 256, 512, 1024, 2048 and 4000; per (rows, context) the two forms alternate for `rounds` rounds, each
window = `calls` whole passes (host clock around calls that end in a stream synchronise) after one untimed call per form (graph capture).  Prints
ms per pass for every round and, per row count, the lowest context from which form 4 wins in EVERY round at that context and all longer ones."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import trackiellm_amd as tk  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 30
ROWS, CTXS = (2, 5, 8), (256, 512, 1024, 2048, 4000)
model = tk.LlmModel(tk.MISTRAL_7B()).fill_synthetic(4)
hp = model.hparams
rng = np.random.default_rng(9)
sess = tk.LlmSession(model, 1, 4096)
sess.prefill(rng.integers(3, hp.vocab, (1, 4000)).astype(np.int32))  # real rows under every context that is timed
wins = {}
for rows in ROWS:
    for ctx in CTXS:
        seq = np.zeros(rows, np.int32)
        pos = np.arange(ctx, ctx + rows, dtype=np.int32)
        tok = rng.integers(3, hp.vocab, rows).astype(np.int32)
        picks = {}
        for form in (2, 4):
            picks[form] = sess.forward_verify(seq, pos, tok, form=form, want_logits=False)[1]
        assert np.array_equal(picks[2], picks[4]), (rows, ctx)
        ms = {2: [], 4: []}
        for _ in range(rounds):
            for form in (2, 4):
                t0 = time.perf_counter()
                for _ in range(calls):
                    sess.forward_verify(seq, pos, tok, form=form, want_logits=False)
                ms[form].append((time.perf_counter() - t0) * 1000.0 / calls)
        wins[(rows, ctx)] = all(b < a for a, b in zip(ms[2], ms[4]))
        print("%d rows at %4d: form 2 %s ms   form 4 %s ms   %s" % (rows, ctx, " ".join("%.3f" % v for v in ms[2]), " ".join("%.3f" % v for v in ms[4]),
                                                                    "form 4 wins every round" if wins[(rows, ctx)] else "-"), flush=True)
for rows in ROWS:
    first = None
    for ctx in reversed(CTXS):
        if not wins[(rows, ctx)]:
            break
        first = ctx
    print("%d rows: form 4 from context %s" % (rows, first if first is not None else "nowhere"))
sess.close()
model.close()
