"""k_attention_far's order of operations restated in float64, for tests/test_attention_far_cpu.py: one (row, block of GQ query heads) workgroup
over T cached positions in chunks of CH, and the same row in k_attention's resident order, so that the argument of the kernel's header comment —
a score depends only on (q, key row), a maximum not on the order it is taken in, and the partial sums are the same chains — can be checked as
equal BITS, and so that a mistake in the two-pass walk can be switched on and shown to move them.

MUTATIONS:
  max_without_last_chunk  pass A stops one chunk early: the maximum is taken over the wrong chunk set
  pv_descending           pass B walks a value chunk from its last position to its first (the chunks still ascend)
  drop_at_chunk_edge      the last position of every full chunk never enters the PV and denominator sums
"""
import numpy as np

TSPLIT = 4
MUTATIONS = ("max_without_last_chunk", "pv_descending", "drop_at_chunk_edge")


def scores(q, k, scale):
    """[T][GQ]: one fma-like chain over head_dim per (position, head), ascending, then times scale — the same chain wherever it is formed"""
    s = np.zeros((k.shape[0], q.shape[0]), np.float64)
    for d in range(q.shape[1]):
        s = s + k[:, d:d + 1] * q[None, :, d]
    return s * scale


def _join(acc, l):
    a = ((acc[0] + acc[1]) + acc[2]) + acc[3]
    ll = ((l[0] + l[1]) + l[2]) + l[3]
    return a / ll[:, None]


def resident(q, k, v):
    """k_attention: every score, the maximum, every probability; then PV and the denominator as four interleaved partial sums (position mod 4),
    each in ascending position order.  q [GQ][hd], k / v [T][hd] -> [GQ][hd]"""
    gq, hd = q.shape
    s = scores(q, k, 1.0 / np.sqrt(np.float64(hd)))
    p = np.exp(s - s.max(axis=0))
    acc, l = np.zeros((TSPLIT, gq, hd)), np.zeros((TSPLIT, gq))
    for t in range(k.shape[0]):
        acc[t % TSPLIT] = acc[t % TSPLIT] + p[t][:, None] * v[t][None, :]
        l[t % TSPLIT] = l[t % TSPLIT] + p[t]
    return _join(acc, l)


def far(q, k, v, ch, mutation=None):
    """k_attention_far with ch positions per ring slot"""
    assert ch % TSPLIT == 0 and mutation in (None,) + MUTATIONS
    gq, hd = q.shape
    T = k.shape[0]
    scale = 1.0 / np.sqrt(np.float64(hd))
    nchunk = -(-T // ch)
    # pass A: only the per-head maximum survives
    m = np.full(gq, -np.inf)
    for c in range(nchunk - 1 if mutation == "max_without_last_chunk" and nchunk > 1 else nchunk):
        m = np.maximum(m, scores(q, k[c * ch:(c + 1) * ch], scale).max(axis=0))
    # pass B: the chunk's scores once more, its probabilities, its values into the sums that persist across the chunks
    acc, l = np.zeros((TSPLIT, gq, hd)), np.zeros((TSPLIT, gq))
    for c in range(nchunk):
        t_end = min(T - c * ch, ch)
        p = np.exp(scores(q, k[c * ch:c * ch + t_end], scale) - m)
        for j in range(TSPLIT):  # wave j: positions = j (mod 4)
            walk = list(range(j, t_end, TSPLIT))
            if mutation == "pv_descending":
                walk.reverse()
            for rr in walk:
                if mutation == "drop_at_chunk_edge" and rr == ch - 1:
                    continue
                acc[j] = acc[j] + p[rr][:, None] * v[c * ch + rr][None, :]
                l[j] = l[j] + p[rr]
    return _join(acc, l)


def rows(T, gq, hd, seed):
    """q, k, v of one workgroup: keys scaled as attention_geometry_cases does, so that the softmax is neither flat nor one-hot"""
    rng = np.random.default_rng([seed, T, gq, hd])
    q = rng.standard_normal((gq, hd))
    k = (rng.standard_normal((T, hd)) * 0.6).astype(np.float16).astype(np.float64)
    v = rng.standard_normal((T, hd)).astype(np.float16).astype(np.float64)
    return q, k, v


def lds_bytes(gq, head_dim, max_ctx, chunk):
    """tk_attention_lds_bytes of tk_llm_kernels.hip: the resident form's workgroup"""
    W = gq * head_dim
    ring = 2 * chunk * head_dim * 2
    epilogue = (TSPLIT * W + TSPLIT * 4 + W) * 4
    red = 4 * 4 * 4 if chunk > 64 else 0
    if head_dim in (64, 128):
        return max(ring, epilogue) + gq * max(max_ctx, head_dim + head_dim // 2) * 4 + red
    return max(ring, epilogue) + (gq * max_ctx + W) * 4 + red + head_dim * 2


def resident_limit(n_head, n_kv_head, head_dim, max_dyn_lds=160 * 1024, max_context=32768):
    """the largest window whose whole group of score rows fits beside a 64-position ring"""
    grp = n_head // n_kv_head
    return max(w for w in range(1, max_context + 1) if lds_bytes(grp, head_dim, w, 64) <= max_dyn_lds)
