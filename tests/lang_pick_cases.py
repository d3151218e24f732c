"""Crafted rows for Whisper's language detection (tests/test_lang_detect_cpu.py on the host loop, tests/test_lang_detect_gpu.py on the kernel).

A row KIND fixes what the language slice of the row holds: where its maximum sits (index 0, 63, 64, n_lang - 1: both sides of the boundary between
a lane's two elements), ties (the first index wins, also across that boundary), -0 against +0 (equal under `>`), -inf and NaN entries (probability
exactly 0; a NaN never wins, not even at index 0), rows with nothing above -inf (id 0, all zeros), differences up to 80 (the bound of the
probability check) and beyond tk_expf's range (terms of exactly 0; quotients in the denormal range).  Everything OUTSIDE the slice — the columns
in front of tok0 and behind tok0 + n_lang, and the padding between rows when ld > cols — holds values that would win or poison the sum (+inf,
NaN, 1e30), so a kernel that reads a column too many shows.  auto_row mixes zero and non-zero (not only 1); slots are planted with values no
token has."""
import numpy as np

KINDS = ("plain", "tie", "tie_across", "zeros_mp", "zeros_pm", "neg_inf", "nan", "all_neg_inf", "max_first", "max_63", "max_64", "max_last",
         "spread_80", "beyond_exp", "all_nan", "nan_and_neg_inf", "denormal_quotient")
BOUNDED = {"plain", "tie", "tie_across", "zeros_mp", "zeros_pm", "neg_inf", "nan", "all_neg_inf", "max_first", "max_63", "max_64", "max_last",
           "spread_80", "all_nan", "nan_and_neg_inf"}                          # |l_i - m| <= 80 wherever l_i is finite
N_LANGS = (1, 63, 64, 65, 99, 100, 128)
ROWS = (1, 2, 17)
OUTSIDE = np.array([np.inf, np.nan, 1.0e30, 3.0e38], np.float32)


def make_row(rng, kind, n):
    l = (rng.standard_normal(n) * 4.0).astype(np.float32).clip(-30.0, 30.0)
    top = np.float32(l.max() + 3.0)

    def at(i):
        return min(i, n - 1)
    if kind == "tie":                                                            # three copies of the maximum: the first one wins
        for i in sorted(set([at(n // 3), at(n // 2), at(n - 1)])):
            l[i] = top
    elif kind == "tie_across":                                                   # a lane's second element ties with a lower lane's first
        l[at(70)] = top
        l[at(9)] = top
        l[at(64 + 9)] = top
    elif kind in ("zeros_mp", "zeros_pm"):                                       # everything else below zero; -0.0 and +0.0 are one value under `>`
        l = -np.abs(l) - np.float32(1.0)
        a, b = at(n // 4), at(3 * n // 4)
        l[b] = np.float32(0.0) if kind == "zeros_mp" else np.float32(-0.0)
        l[a] = np.float32(-0.0) if kind == "zeros_mp" else np.float32(0.0)       # written last: n == 1 keeps the lower index's value
    elif kind == "neg_inf":
        l[rng.random(n) < 0.3] = -np.inf
        l[at(n // 2)] = top
        if n > 1:
            l[0] = -np.inf
    elif kind == "nan":
        l[rng.random(n) < 0.3] = np.nan
        l[at(n // 2)] = top
        if n > 1:
            l[0] = np.nan                                                        # a NaN in front never stands
    elif kind == "all_neg_inf":
        l[:] = -np.inf
    elif kind == "max_first":
        l[0] = top
    elif kind == "max_63":
        l[at(63)] = top
    elif kind == "max_64":
        l[at(64)] = top
    elif kind == "max_last":
        l[n - 1] = top
    elif kind == "spread_80":
        l = (-rng.random(n) * 80.0).astype(np.float32)
        l[at(n // 5)] = np.float32(0.0)
    elif kind == "beyond_exp":                                                   # differences past -87: terms of exactly 0
        l = (-rng.random(n) * 200.0).astype(np.float32)
        l[at(2 * n // 3)] = np.float32(7.5)
    elif kind == "all_nan":
        l[:] = np.nan
    elif kind == "nan_and_neg_inf":
        l[:] = np.where(rng.random(n) < 0.5, np.nan, -np.inf).astype(np.float32)
    elif kind == "denormal_quotient":                                            # many terms of 1, some of exp(-86.9): p / S falls below 2^-126
        l[:] = np.float32(3.0)
        l[rng.random(n) < 0.25] = np.float32(3.0 - 86.9)
        l[at(1)] = np.float32(3.0 - 86.5)
    return l


def make_case(n_lang, rows, first_kind=0, seed=0):
    """one launch: rows whose kinds walk KINDS from first_kind on"""
    rng = np.random.default_rng([n_lang, rows, first_kind, seed])
    front, back = int(rng.integers(0, 4)), int(rng.integers(0, 4))
    cols = front + n_lang + back
    ld = cols + (0 if (n_lang + rows + first_kind) % 2 else 5)
    x = OUTSIDE[rng.integers(0, OUTSIDE.size, (rows, ld))]
    kinds = [KINDS[(first_kind + r) % len(KINDS)] for r in range(rows)]
    for r, k in enumerate(kinds):
        x[r, front: front + n_lang] = make_row(rng, k, n_lang)
    auto_row = rng.choice(np.array([0, 1, 2, -1], np.int32), rows)
    if rows >= 2:
        auto_row[0], auto_row[1] = (0, 7) if first_kind % 2 else (1, 0)
    slot = (-1000 - np.arange(rows)).astype(np.int32)
    flat = x.reshape(-1)[: (rows - 1) * ld + cols].copy()                         # the last row has no padding behind it
    return dict(name="n%d_r%d_k%d" % (n_lang, rows, first_kind), n_lang=n_lang, rows=rows, cols=cols, ld=ld, tok0=front, logits=flat,
                auto_row=auto_row, slot=slot, kinds=kinds, bounded=np.array([k in BOUNDED for k in kinds]))


def cases(n_lang, rows):
    """launches of `rows` rows that together visit every kind"""
    n = len(KINDS)
    return [make_case(n_lang, rows, k) for k in range(0, n, rows)] if rows < n else [make_case(n_lang, rows)]


def all_cases(rows_list=ROWS):
    return [c for n in N_LANGS for rows in rows_list for c in cases(n, rows)]
