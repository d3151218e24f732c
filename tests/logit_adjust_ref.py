"""float32 NumPy restatement of the logit adjustment (bias, then repetition penalties), written from its definition:

    1. for each j:  logits[bias_ids[j]] = logits[bias_ids[j]] + bias[j]              (ids unique within a row)
    2. for every distinct token t of `recent`, c = its number of occurrences:
         l = logits[t];  l = l * repeat if l <= 0 else l / repeat;  l = l - (float(c) * freq + present)

every operation one correctly rounded float32 operation (NumPy float32 scalars).  A row with no bias entry and (an empty window or
repeat == 1, freq == 0, present == 0) is neutral: returned as it came.

MUTATIONS: one plausible implementation error each, for the CPU test that shows the cases discriminate."""
import collections

import numpy as np

F = np.float32
MUTATIONS = ("repeat_divides_negatives", "presence_per_occurrence", "bias_after_penalties", "duplicates_twice")


def spec_fields(spec):
    spec = spec or {}
    recent = np.asarray(spec.get("recent", ()) if spec.get("recent") is not None else (), np.int64).reshape(-1)
    bias_ids = np.asarray(spec.get("bias_ids", ()) if spec.get("bias_ids") is not None else (), np.int64).reshape(-1)
    bias = np.asarray(spec.get("bias", ()) if spec.get("bias") is not None else (), np.float32).reshape(-1)
    return recent, bias_ids, bias, F(spec.get("repeat", 1.0)), F(spec.get("freq", 0.0)), F(spec.get("present", 0.0))


def adjust_row(logits, spec, mut=()):
    """one row; spec: None or the dict trackiellm_amd.logit_adjust_rows takes"""
    out = np.array(logits, dtype=np.float32, copy=True)
    recent, bias_ids, bias, repeat, freq, present = spec_fields(spec)
    if bias_ids.size == 0 and (recent.size == 0 or (repeat == 1 and freq == 0 and present == 0)):
        return out

    def add_bias():
        for t, b in zip(bias_ids.tolist(), bias):
            out[t] = F(out[t]) + F(b)

    with np.errstate(all="ignore"):
        if "bias_after_penalties" not in mut:
            add_bias()
        counts = collections.Counter(recent.tolist())
        visits = recent.tolist() if "duplicates_twice" in mut else list(counts)
        for t in visits:
            c = counts[t]
            v = F(out[t])
            if "repeat_divides_negatives" in mut:
                v = v / repeat
            else:
                v = v * repeat if v <= 0 else v / repeat
            pres = F(c) * present if "presence_per_occurrence" in mut else present
            v = v - (F(c) * freq + pres)
            out[t] = v
        if "bias_after_penalties" in mut:
            add_bias()
    return out


def adjust(logits, specs, mut=()):
    """[rows][cols] -> adjusted copy"""
    logits = np.asarray(logits, np.float32)
    return np.stack([adjust_row(logits[r], specs[r], mut) for r in range(logits.shape[0])])


def is_neutral(spec):
    recent, bias_ids, _, repeat, freq, present = spec_fields(spec)
    return bias_ids.size == 0 and (recent.size == 0 or (repeat == 1 and freq == 0 and present == 0))
