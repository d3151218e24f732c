"""References for k_token_logprobs (csrc/common/tk_token_logprob.h), written from the header's comment, not from its code.

Reference A, `record32`: a float32 NumPy restatement in the header's term order — m the logit of the first token in the sampler's order, terms
tk_expf(l_i - m) (through the oracle library's orc_expf, as tests/test_token_pick_cpu.py calls it), 1024 lane sums ascending from +0, a six-level xor
butterfly inside each wave of 64, the sixteen wave sums in ascending order, tk_logf (orc_logf), two subtractions.  Expected to match bit for bit.

Reference B, `record64`: a float64 log-softmax over the whole row.  The implemented summation order is the one tests/token_pick_ref.logprob_bound
describes (a lane chain of at most ceil(cols / 1024) terms, 6 butterfly levels, 15 joins), so its allowed distance is
logprob_bound(z, z_tok, cols, hot=False), constants unchanged.  A -inf logit has log-probability -inf on both sides, exactly.

The top list is an exact decision in both: the first min(n_top, cols) tokens by (logit descending with -0 below +0, id ascending).

`mut`: mutation switches, one plausible kernel error each; tests/test_token_logprob_cpu.py shows that each changes at least one case."""
import functools

import numpy as np

from token_pick_ref import logprob_bound, order_key  # noqa: F401

LANES, WAVE, MAX_TOP = 1024, 64, 20

MUTATIONS = (
    "ties_high_id",   # ties to the higher id
    "no_max",         # the sum without the maximum subtracted
    "grammar_mask",   # the grammar mask honoured: forbidden tokens leave the distribution and the list
    "temperature",    # the temperature applied to the logits
)


@functools.lru_cache(maxsize=None)
def _fn():
    import oracle_lib as O
    L = O.lib()
    return np.vectorize(lambda v: L.orc_expf(float(v)), otypes=[np.float32]), (lambda v: np.float32(L.orc_logf(float(v))))


def top_order(x, mut=()):
    ids = np.arange(len(x))
    return np.lexsort((-ids if "ties_high_id" in mut else ids, -order_key(x)))


def record32(x, tok, n_top, mut=(), mask_ids=None, temp=None):
    """(logprob float32, ids, logprobs float32) of one live row"""
    expf, logf = _fn()
    x = np.ascontiguousarray(x, np.float32)
    if "temperature" in mut:
        x = (x / np.float32(temp)).astype(np.float32)
    live = np.ones(len(x), bool)
    if "grammar_mask" in mut:
        live[:] = False
        live[np.asarray(mask_ids)] = True
    order = top_order(x, mut)
    order = order[live[order]]
    m = np.float32(0.0) if "no_max" in mut else x[order[0]]
    with np.errstate(invalid="ignore", over="ignore"):
        d = (x - m).astype(np.float32)
        e = np.where(live, expf(d), np.float32(0.0)).astype(np.float32)
        pad = (-len(e)) % LANES
        chunks = np.concatenate([e, np.zeros(pad, np.float32)]).reshape(-1, LANES)
        valid = np.concatenate([np.ones(len(e), bool), np.zeros(pad, bool)]).reshape(-1, LANES)
        v = np.zeros(LANES, np.float32)
        for c, ok in zip(chunks, valid):                   # lane t adds its terms i = t, t + 1024, ... in ascending order
            v = np.where(ok, (v + c).astype(np.float32), v)
        t = np.arange(LANES)
        for dist in (32, 16, 8, 4, 2, 1):                  # inside each wave: lane t takes lane t ^ dist
            v = (v + v[t ^ dist]).astype(np.float32)
        S = v[0]
        for w in range(1, LANES // WAVE):                  # the wave sums in ascending order
            S = np.float32(S + v[WAVE * w])
        logS = logf(S)
        lp = ((x - m).astype(np.float32) - logS).astype(np.float32)
    top = order[:min(n_top, len(order))]
    return lp[tok], top.astype(np.int32), lp[top]


def record64(x, tok, n_top):
    """(logprob float64, its bound, ids, logprobs float64, their bounds) of one live row"""
    x32 = np.ascontiguousarray(x, np.float32)
    z = x32.astype(np.float64)
    with np.errstate(divide="ignore"):
        lsm = (z - z.max()) - np.log(np.exp(z - z.max()).sum())
    top = top_order(x32)[:min(n_top, len(z))]

    def bound(i):
        return 0.0 if np.isneginf(z[i]) else logprob_bound(z, z[i], len(z), hot=False)

    return lsm[tok], bound(tok), top.astype(np.int32), lsm[top], np.array([bound(i) for i in top])
