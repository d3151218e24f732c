"""Crafted rows for k_token_logprobs (tk_mi355x_token_logprobs_probe), small.  A case is one launch: `rows` rows of `cols` logits `ld` apart in a flat
array whose gaps hold NaN sentinels (nothing may read them), the chosen id and n_top of every row, and IN/OUT records that arrive full of sentinels —
the rows that are off and the entries past a record's filled count must come back untouched.

Every row also carries what only a MUTANT of the reference reads (tests/token_logprob_ref.py): the ids a grammar mask would allow and a temperature."""
import numpy as np

MAX_TOP = 20
REC_DTYPE = np.dtype([("logprob", np.float32), ("n_top", np.int32), ("top_ids", np.int32, (MAX_TOP,)), ("top_logprobs", np.float32, (MAX_TOP,))])
S_LOGPROB, S_NTOP, S_ID, S_LP = np.float32(777.25), -12345, -7, np.float32(555.5)
TEMP = 0.7
NINF = np.float32(-np.inf)


def sentinel_records(rows):
    rec = np.zeros(rows, REC_DTYPE)
    rec["logprob"], rec["n_top"], rec["top_ids"], rec["top_logprobs"] = S_LOGPROB, S_NTOP, S_ID, S_LP
    return rec


def _row(kind, cols, rng):
    """-> (logits float32 [cols], chosen id or None = the first token)"""
    if kind == "normal":
        return (4.0 * rng.standard_normal(cols)).astype(np.float32), None
    if kind == "equal":                                    # every log-probability is -log(cols), the list is 0, 1, 2, ...
        return np.full(cols, 1.375, np.float32), int(rng.integers(cols))
    if kind == "levels":                                   # four levels: ties across lanes and waves, and at the n_top-th place
        return rng.choice(np.array([2.5, 2.0, -1.0, -3.25], np.float32), cols), int(rng.integers(cols))
    if kind == "tie_at_cut":                               # exactly 19 above a plateau: the 20th place is a tie, broken by id
        x = np.full(cols, 0.5, np.float32)
        x[rng.choice(cols, min(19, cols - 1), replace=False)] = 3.0 if cols > 1 else 0.5
        return x, int(cols - 1)
    if kind == "zeros":                                    # -0 and +0 at the top: +0 stands before -0 whatever the ids
        x = (-1.0 - np.abs(rng.standard_normal(cols))).astype(np.float32)
        at = rng.choice(cols, min(6, cols), replace=False)
        x[at] = np.where(np.arange(len(at)) % 2 == 0, np.float32(-0.0), np.float32(0.0))
        return x, int(at[0])
    if kind == "ninf":                                     # a third of the row banned
        x = (3.0 * rng.standard_normal(cols)).astype(np.float32)
        x[rng.random(cols) < 0.33] = NINF
        x[int(rng.integers(cols))] = 1.0                   # at least one finite logit
        return x, None
    if kind == "chosen_ninf":                              # the chosen id is a banned one: its log-probability is -inf
        x = (3.0 * rng.standard_normal(cols)).astype(np.float32)
        if cols == 1:
            return x, 0
        ban = int(rng.integers(cols))
        x[ban] = NINF
        return x, ban
    if kind == "dominant":                                 # one logit 100 above the rest: every other term is exactly 0, S = 1, log S = 0
        x = np.full(cols, -50.0, np.float32) - rng.integers(0, 4, cols).astype(np.float32)
        x[int(rng.integers(cols))] = 50.0
        return x, None
    raise ValueError(kind)


KINDS = ("normal", "equal", "levels", "tie_at_cut", "zeros", "ninf", "chosen_ninf", "dominant")


def make_case(name, cols, kinds, n_tops, ld=None, seed=0):
    rows = len(kinds)
    ld = cols if ld is None else ld
    rng = np.random.default_rng(1000 * cols + seed)
    flat = np.full((rows - 1) * ld + cols + (ld - cols), np.nan, np.float32)
    ids = np.zeros(rows, np.int32)
    masks = []
    for r, kind in enumerate(kinds):
        x, tok = _row(kind, cols, rng)
        if tok is None:
            from token_pick_ref import order_key
            tok = int(np.lexsort((np.arange(cols), -order_key(x)))[0])
        flat[r * ld:r * ld + cols] = x
        ids[r] = tok
        allowed = np.arange(1, cols, 2) if cols > 1 else np.arange(1)   # what a grammar mask would allow: the odd ids (mutants only)
        masks.append(np.union1d(allowed, [tok]))
    return dict(name=name, rows=rows, cols=cols, ld=ld, logits=flat, ids=ids, n_top=np.asarray(n_tops, np.int32), kinds=tuple(kinds), masks=masks, temp=TEMP)


def row_of(case, r):
    return case["logits"][r * case["ld"]:r * case["ld"] + case["cols"]]


def cases(max_rows=256):
    out = []
    for k, cols in enumerate((1, 2, 63, 64, 65, 1023, 1024, 1025, 2049)):
        ld = cols + (0, 3, 17)[k % 3]
        # three rows: a live row, an off row between live rows, every n_top of -1, 0, 1, 20 (20 > cols on the small ones)
        out.append(make_case("c%d_a" % cols, cols, ("normal", "levels", "equal"), (20, -1, 1), ld=ld, seed=1))
        out.append(make_case("c%d_b" % cols, cols, ("tie_at_cut", "zeros", "ninf"), (20, 20, 0), ld=ld, seed=2))
        out.append(make_case("c%d_c" % cols, cols, ("chosen_ninf", "dominant", "levels"), (1, 20, 20), ld=ld, seed=3))
        out.append(make_case("c%d_one" % cols, cols, (KINDS[k % len(KINDS)],), (20,), seed=4))                      # one row
    out.append(make_case("c32000", 32000, ("normal",), (20,), seed=5))
    out.append(make_case("c32000_ties", 32000, ("levels",), (20,), seed=6))
    out.append(make_case("c32769", 32769, ("levels", "normal"), (20, 3), ld=32771, seed=8))   # one past 32 x 1024: the kernel's 64-register form
    out.append(make_case("c65536", 65536, ("tie_at_cut",), (20,), seed=9))                      # the largest vocabulary
    kinds = [KINDS[r % len(KINDS)] for r in range(max_rows)]
    out.append(make_case("c65_wide", 65, kinds, [(-1, 0, 1, 20, 7)[r % 5] for r in range(max_rows)], ld=70, seed=7))  # the widest launch
    return out


def refusals(max_rows=256):
    """[(name, kwargs of token_logprobs_probe)]: each breaks exactly one rule of the probe"""
    def base(**kw):
        lg = np.linspace(-1.0, 1.0, 2 * 8).astype(np.float32)
        d = dict(logits=lg, rows=2, cols=8, ld=8, ids=np.array([1, 2], np.int32), n_top=np.array([3, 0], np.int32))
        d.update(kw)
        return d

    def with_logit(i, v):
        lg = np.linspace(-1.0, 1.0, 16).astype(np.float32)
        lg[i] = v
        return lg

    return [("rows 0", base(rows=0)), ("rows above the limit", base(rows=max_rows + 1, logits=np.zeros((max_rows + 1) * 8, np.float32), ids=np.zeros(max_rows + 1, np.int32), n_top=np.zeros(max_rows + 1, np.int32))),
            ("cols 0", base(cols=0, ld=8)), ("cols above 65536", base(rows=1, cols=65537, ld=65537, logits=np.zeros(65537, np.float32))),
            ("ld < cols", base(ld=7)), ("logits too short", base(n_logits=15)),
            ("id below 0", base(ids=np.array([-1, 2], np.int32))), ("id == cols", base(ids=np.array([1, 8], np.int32))),
            ("n_top -2", base(n_top=np.array([-2, 0], np.int32))), ("n_top 21", base(n_top=np.array([3, 21], np.int32))),
            ("a NaN in a live row", base(logits=with_logit(3, np.nan))), ("+inf in a live row", base(logits=with_logit(12, np.inf))),
            ("no finite logit in a live row", base(logits=np.concatenate([np.full(8, -np.inf), np.zeros(8)]).astype(np.float32)))]


def accepted_oddities():
    """what the probe must take: a NaN in a row that is OFF is never read"""
    lg = np.linspace(-1.0, 1.0, 16).astype(np.float32)
    lg[3] = np.nan
    return [("a NaN in an off row", dict(logits=lg, rows=2, cols=8, ld=8, ids=np.array([1, 2], np.int32), n_top=np.array([-1, 2], np.int32)))]
