"""Crafted rows for the logit adjustment (tests/test_logit_adjust_cpu.py on the host loop, tests/test_logit_adjust_gpu.py on the kernel).

A row KIND fixes the window (0, 1, 64 or 256 ids; all equal, all distinct or mixed), the number of bias entries (0, 1 or 256, with -inf among
them and some on tokens that are also in the window) and the penalty values; neutral kinds sit between adjusted ones.  The logits of every row
mix ordinary positive and negative values with +0.0, -0.0, -inf, values near FLT_MAX and a denormal-range value, so that the tokens a row touches
meet each of them.  No case can produce a NaN (no inf - inf): results are compared as bit patterns."""
import numpy as np

ON = (1.3, 0.5, 0.25)
KINDS = (
    None,                                                                          # neutral: nothing given
    dict(nr=64, style="mixed", nb=0, pen=ON),
    dict(nr=0, style="mixed", nb=1, pen=(1.0, 0.0, 0.0)),                           # bias alone
    dict(nr=64, style="mixed", nb=0, pen=(1.0, 0.0, 0.0)),                          # neutral: a window, penalties off
    dict(nr=1, style="equal", nb=0, pen=(1.1, 0.0, 0.0)),
    dict(nr=256, style="equal", nb=0, pen=ON),                                      # one token, c = 256
    dict(nr=256, style="distinct", nb=256, pen=(0.7, -0.25, 0.0), overlap=True),
    None,
    dict(nr=64, style="equal", nb=1, pen=ON, overlap=True),                         # the bias entry sits on the window's token
    dict(nr=64, style="distinct", nb=256, pen=ON, overlap=True),
    dict(nr=256, style="mixed", nb=1, pen=(1.0, 0.0, 1e30)),
    dict(nr=1, style="equal", nb=256, pen=(1.0, 0.5, 0.0), overlap=True),
    dict(nr=0, style="mixed", nb=256, pen=ON),                                      # penalties on over an empty window
    dict(nr=64, style="mixed", nb=64, pen=(1.0, 0.0, 0.0), overlap=True),           # penalties off, not neutral: the bias applies
    dict(nr=0, style="mixed", nb=0, pen=ON),                                        # neutral: penalties on, nothing to penalise
    dict(nr=256, style="mixed", nb=256, pen=(1.1, 0.0, 0.0), overlap=True),
)
SPECIALS = np.array([0.0, -0.0, -np.inf, 3.0e38, -3.0e38, 1.0e-38, 3.4028234e38], np.float32)


def make_logits(rng, rows, cols):
    x = (rng.standard_normal((rows, cols)) * 5.0).astype(np.float32)
    special = rng.random((rows, cols)) < 0.35
    x[special] = SPECIALS[rng.integers(0, SPECIALS.size, int(special.sum()))]
    return x


def make_spec(rng, kind, cols):
    if kind is None:
        return None
    nr, nb = kind["nr"], min(kind["nb"], cols)
    if kind["style"] == "equal":
        recent = np.full(nr, rng.integers(0, cols), np.int32)
    elif kind["style"] == "distinct" and nr <= cols:
        recent = rng.permutation(cols)[:nr].astype(np.int32)
    else:  # mixed: a few tokens many times, the rest once or twice
        pool = rng.integers(0, cols, max(1, nr // 3))
        recent = pool[rng.integers(0, pool.size, nr)].astype(np.int32)
    ids = rng.permutation(cols)[:nb].astype(np.int32)
    if kind.get("overlap") and nr > 0 and nb > 0:  # some entries on tokens of the window, still unique
        want = np.unique(recent)[: max(1, nb // 2)]
        rest = ids[~np.isin(ids, want)]
        ids = np.concatenate([want, rest])[:nb].astype(np.int32)
        assert np.unique(ids).size == nb and np.isin(ids, recent).any()
    bias = (rng.standard_normal(nb) * 4.0).astype(np.float32)
    if nb:
        bias[rng.random(nb) < 0.2] = -np.inf
        bias[0] = -np.inf if nb == 1 and kind.get("overlap") else bias[0]
        if nb >= 4:
            bias[1], bias[2], bias[3] = 3.0e38, -3.0e38, 0.0
    r, f, p = kind["pen"]
    return dict(repeat=r, freq=f, present=p, recent=recent, bias_ids=ids, bias=bias)


def make_case(cols, rows, first_kind=0, seed=0):
    """rows whose kinds walk KINDS from first_kind on"""
    rng = np.random.default_rng([cols, rows, first_kind, seed])
    specs = [make_spec(rng, KINDS[(first_kind + r) % len(KINDS)], cols) for r in range(rows)]
    return dict(name="v%d_r%d_k%d" % (cols, rows, first_kind), cols=cols, rows=rows, logits=make_logits(rng, rows, cols), specs=specs)


def cases(cols, rows):
    """launches of `rows` rows that together visit every kind"""
    n = len(KINDS)
    return [make_case(cols, rows, k) for k in range(0, n, rows)] if rows < n else [make_case(cols, rows)]
