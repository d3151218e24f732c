"""The crafted logit rows of tests/test_token_pick_gpu.py (one dict per launch) — shared with tests/test_token_pick_cpu.py, which proves on the
CPU that they discriminate.  Nothing here touches a device.

NaN rows, and rows whose largest allowed logit is -inf under SAMPLING (or under a log-probability), are left out on purpose: their arithmetic is
NaN on every side and is not a contract.  Greedy picks over -inf rows are in."""
import functools

import numpy as np

import token_pick_ref as R

VOCABS_ALL = (1, 31, 32, 33, 63, 64, 65, 1000, 1023, 1024, 1025)
VOCABS_LLM = VOCABS_ALL + (8193, 32000, 65535, 65536)   # k_argmax steps 8 x 1024: second outer trip and clamped tail loads at 8193
SEED_BIG = 2 ** 63 + 12345
NINF = np.float32(-np.inf)
GAP = np.float32(1e30)      # sentinel in the ld > cols gap: a kernel that read it would pick it
PICK_ARGMAX, PICK_ARGMAX_ROWS, PICK_ROWS, PICK_ROWS_FILTERED = 0, 1, 2, 3


def _u_vec(seed, counters):
    """token_pick_ref.splitmix_u over an array of counters"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (counters.astype(np.uint64) + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return (z >> np.uint64(40)).astype(np.float64) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def counter_with_u(seed, lo, hi, multiple_of=None):
    """the first counter whose draw u lies in [lo, hi) (and is a non-zero multiple of `multiple_of`): a search of splitmix64 on the CPU"""
    for base in range(0, 1 << 26, 1 << 20):
        c = np.arange(base, base + (1 << 20), dtype=np.uint64)
        u = _u_vec(seed, c)
        hit = (u >= lo) & (u < hi)
        if multiple_of is not None:
            hit &= (np.round(u / multiple_of) * multiple_of == u) & (u > 0)
        if hit.any():
            c = int(c[np.argmax(hit)])
            assert lo <= R.splitmix_u(seed, c) < hi
            return c
    raise AssertionError("no such counter")


def S(temp=0.8, top_k=40, top_p=0.95, min_p=0.05, seed=0, counter=0):
    """one row's sampling state (temperature 0: greedy)"""
    return (float(np.float32(temp)), int(top_k), float(np.float32(top_p)), float(np.float32(min_p)), int(seed), int(counter))


GREEDY = S(0.0, 0, 1.0, 0.0, 7, 41)   # a greedy row that carries a seed and a counter: the counter must stay


def llm_case(name, logits, masks=None, allow_row=None, samp=None, null=(), expect=None):
    """one k_argmax launch; bookkeeping arrays start from values a kernel cannot produce by accident.  null: pointers handed over as NULL"""
    logits = np.ascontiguousarray(logits, np.float32)
    rows = logits.shape[0]
    stride = rows + 2
    nsteps = np.arange(rows, dtype=np.int32) % 3
    c = dict(name=name, logits=logits, masks=None if masks is None else np.ascontiguousarray(masks, np.uint32),
             allow_row=None if allow_row is None else np.asarray(allow_row, np.int32), samp=samp,
             tok=-1000 - np.arange(rows, dtype=np.int32), pos=(10 * np.arange(rows) + 3).astype(np.int32), nsteps=nsteps,
             hist=np.full(5 * stride + 3, -77, np.int32), hist_stride=stride, expect=expect or {})
    for n in null:
        c[n] = None
    assert samp is None or len(samp) == rows
    return c


def _rng(*key):
    return np.random.default_rng([20240611, *key])


def _random_mask(rng, V, keep=0.5, junk=False, drop=None):
    ids = [i for i in range(V) if rng.random() < keep and i != drop]
    if not ids:
        ids = [V - 1 if drop != V - 1 else 0]
    return R.mask_words(V, ids, junk)


def _generic_llm(V):
    """eight rows in one launch: greedy, greedy under two masks (the row's maximum disallowed; junk bits past V), sampled with five parameter sets,
    with and without masks, seeds 0 and 2^63 + 12345"""
    rng = _rng(1, V)
    x = (rng.standard_normal((8, V)) * 3).astype(np.float32)
    drop = lambda r: int(np.argmax(x[r])) if V > 1 else None   # noqa: E731
    masks = np.stack([_random_mask(rng, V, 0.5, drop=drop(1)), _random_mask(rng, V, 0.3, junk=True, drop=drop(2)), R.mask_words(V, range(V))])
    samp = [GREEDY, GREEDY, GREEDY, S(0.8, 40, 0.95, 0.05, 0, 3), S(1.0, 0, 1.0, 0.0, SEED_BIG, 9), S(100.0, 1000, 1.0, 0.0, 0, 2 ** 32 - 1),
            S(1e-3, 2, 0.5, 0.0, SEED_BIG, 0), S(0.7, 64, 0.9, 0.1, 11, 5)]
    return llm_case("generic_v%d" % V, x, masks, [-1, 0, 1, -1, 0, 1, -1, 2], samp)


TIE_PAIRS = ((5, 1029), (5, 9), (70, 1030), (6, 70), (0, 2099), (1500, 2047))


def _tie_rows(V=2100):
    """equal maxima at: one thread's chain (i, i + 1024); two lanes of a wave; two waves with the lower id in the higher wave (70: thread 70, wave 1;
    1030: thread 6, wave 0); two waves with the lower id in the lower wave; the first and the last index; two chains of different waves beyond the
    first trip; every element equal"""
    x = (_rng(2).standard_normal((len(TIE_PAIRS) + 1, V)) * 2).astype(np.float32)
    for r, (a, b) in enumerate(TIE_PAIRS):
        x[r, a] = x[r, b] = 50.0
    x[-1] = 1.25
    return x


def _special_rows(V=1000):
    x = np.full((5, V), NINF, np.float32)
    x[0, 777] = -3.0                                        # -inf everywhere except one place
    # row 1: -inf everywhere
    x[2] = -3.0e38; x[2, 333] = -1.0e38                     # large negative finite values
    x[3] = np.float32(-3.4028234e38)                        # every element the lowest finite float
    x[4] = (_rng(3).standard_normal(V) * 2).astype(np.float32); x[4, :500] = NINF   # half the row -inf
    return x


@functools.lru_cache(maxsize=None)
def llm_cases():
    cases = [_generic_llm(V) for V in VOCABS_LLM]
    # ---- greedy ties, without a mask and under an all-ones mask (which must change nothing)
    t = _tie_rows()
    n = len(t)
    cases.append(llm_case("ties", np.concatenate([t, t]), R.mask_words(2100, range(2100))[None], [-1] * n + [0] * n,
                          expect={r: e for r, e in enumerate([5, 5, 70, 6, 0, 1500, 0] * 2)}))
    # ---- special logits, greedy (every row) and sampled (rows with a finite maximum)
    sp = _special_rows()
    cases.append(llm_case("special_greedy", sp, expect={0: 777, 1: 0, 2: 333, 3: 0}))
    cases.append(llm_case("special_sampled", sp[[0, 2, 3, 4]], samp=[S(0.8, 40, 0.95, 0.05, 0, 1), S(1.0, 0, 1.0, 0.0, 0, 2), S(1.0, 0, 1.0, 0.0, SEED_BIG, 3),
                                                                    S(1.0, 0, 1.0, 0.0, 0, 4)], expect={0: 777, 1: 333}))
    z = np.array([[-0.0, 0.0], [0.0, -0.0]] * 3, np.float32)
    cases.append(llm_case("signed_zeros", z, samp=[GREEDY, GREEDY, S(1.0, 1), S(1.0, 1), S(1.0, 2, 1.0, 0.0, 0, counter_with_u(0, 0.0, 0.4)),
                                                    S(1.0, 2, 1.0, 0.0, 0, counter_with_u(0, 0.6, 1.0))],
                          expect={0: 0, 1: 0, 2: 1, 3: 0, 4: 1, 5: 1}))   # greedy: the first index; the sampler ranks +0 first (rows 4, 5: first / second candidate)
    # ---- masks at a vocabulary whose last word is partly past it
    V = 1000
    rng = _rng(4)
    x = (rng.standard_normal((10, V)) * 3).astype(np.float32)
    top = [int(np.argmax(x[r])) for r in range(10)]
    x[6, 100:200] = NINF
    masks = np.stack([R.mask_words(V, [999]), R.mask_words(V, [0]), R.mask_words(V, [i for i in range(V) if i != top[3]]),
                      R.mask_words(V, [i for i in range(V) if i != top[4] and i % 3]), R.mask_words(V, range(100, 200)),
                      R.mask_words(V, range(960, 1000), junk=True), R.mask_words(V, range(V))])
    x[9] = x[8]
    cases.append(llm_case("masks_greedy", x, masks, [-1, 0, 1, 2, 3, -1, 4, 5, 6, -1],
                          expect={1: 999, 2: 0, 6: 100}))      # row 6: every allowed token -inf -> the first allowed index
    samp = [S(1.0, 40, 0.95, 0.05, 0, 1), S(1.0, 40, 1.0, 0.0, 0, 2), S(1.0, 40, 1.0, 0.0, SEED_BIG, 3), S(1.0, 0, 1.0, 0.0, 5, 4), S(2.0, 64, 0.9, 0.0, 5, 5), GREEDY,
            S(1.0, 40, 1.0, 0.0, 5, 6), S(100.0, 64, 1.0, 0.0, 5, counter_with_u(5, 0.85, 0.95)), S(1.5, 40, 0.95, 0.05, 9, 7), S(1.5, 40, 0.95, 0.05, 9, 7)]
    x2 = x.copy(); x2[6, 100:200] = x[5, 100:200]
    masks2 = masks.copy(); masks2[4] = R.mask_words(V, [3, 500, 640, 641, 999])                      # five allowed, below top_k = 40
    cases.append(llm_case("masks_sampled", x2, masks2, [-1, 0, 1, 2, 3, -1, 4, 5, 6, -1], samp, expect={1: 999, 2: 0}))
    # a row whose junk bits sit right before a row of much larger logits: honouring them would read on into that row
    xj = np.stack([np.linspace(0, 1, 33, dtype=np.float32), np.full(33, 100, np.float32)])
    cases.append(llm_case("mask_junk_before_larger_row", np.concatenate([xj, xj]), R.mask_words(33, range(33), junk=True)[None], [0, -1, 0, -1],
                          [GREEDY, GREEDY, S(1.0, 0, 1.0, 0.0, 0, 1), GREEDY], expect={0: 32}))
    # ---- sampler
    x = (_rng(5).standard_normal((16, V)) * 3).astype(np.float32)
    hi, lo = counter_with_u(0, 1 - 2.0 ** -10, 1 - 2.0 ** -12), counter_with_u(0, 0.0, 2.0 ** -10)
    hi_b, lo_b = counter_with_u(SEED_BIG, 1 - 2.0 ** -10, 1 - 2.0 ** -12), counter_with_u(SEED_BIG, 0.0, 2.0 ** -10)
    far = counter_with_u(0, 0.85, 0.95)
    samp = [S(1.0, k, 1.0, 0.0, 0, 10 + k) for k in (0, 1, 2, 40, 64, 1000)] + \
           [S(100.0, 0, 1.0, 0.0, 0, far), S(100.0, 1000, 1.0, 0.0, 0, far),    # top_k 0 = 64 and top_k 1000 = 64: a flat distribution and u ~ 0.9 land far down the list
            S(1.0, 40, 0.01, 0.0, 0, far),                                        # top-p so small that one token survives
            S(1.0, 40, 1.0, 1.0, 0, far),                                         # min_p = 1
            S(1e-3, 40, 1.0, 0.0, 0, far), S(100.0, 40, 0.95, 0.05, SEED_BIG, 77),
            S(1.0, 0, 1.0, 0.0, 0, lo), S(1.0, 0, 1.0, 0.0, 0, hi), S(1.0, 64, 1.0, 0.0, SEED_BIG, lo_b), S(3.0, 64, 1.0, 0.0, SEED_BIG, hi_b)]
    cases.append(llm_case("sampler_parameters", x, samp=samp, expect={1: int(np.argmax(x[1])), 8: int(np.argmax(x[8])), 9: int(np.argmax(x[9])),
                                                                     12: int(np.argmax(x[12]))}))
    # a tie at the K-th place: 30 larger logits, then a run of 100 equal ones straddling place 64; flat weights and u ~ 0.9 pick inside the run
    x = np.full((2, V), -20.0, np.float32)
    x[:, 3:93:3] = 4.0 + np.arange(30, dtype=np.float32) / 64
    x[:, 200:300] = 3.5
    cases.append(llm_case("kth_tie_run", x, samp=[S(100.0, 64, 1.0, 0.0, 0, far), S(100.0, 0, 1.0, 0.0, SEED_BIG, hi_b)]))
    x = np.full((3, 65536), -20.0, np.float32)
    x[0, 3:93:3] = 4.0 + np.arange(30, dtype=np.float32) / 64
    x[0, 300:350] = 3.5; x[0, 40000:40050] = 3.5                                    # the same run split between low and high ids
    x[1] = 0.75                                                                     # all 65536 logits equal: ids 0 .. 63
    x[2] = 0.75
    cases.append(llm_case("kth_tie_split_and_all_equal", x, samp=[S(100.0, 64, 1.0, 0.0, 0, far), S(1.0, 0, 1.0, 0.0, 0, far), S(1.0, 40, 1.0, 0.0, 0, hi)],
                          expect={2: 39}))
    # comparisons that are exact in float32 and float64 alike (reference B abstains on them by its own rule; the hand-derived id is asserted):
    k64 = counter_with_u(0, 1 / 64, 1.0, multiple_of=1 / 64)                        # u = k / 64 over 64 equal weights: c_(k-1) = k = u W is not > u W
    ku = int(round(R.splitmix_u(0, k64) * 64))
    half = counter_with_u(0, 0.6, 1.0)
    cases.append(llm_case("exact_draw_tie", np.full((1, 64), 0.5, np.float32), samp=[S(1.0, 0, 1.0, 0.0, 0, k64)], expect={0: ku}))
    cases.append(llm_case("exact_top_p_tie", np.full((1, 2), 2.0, np.float32), samp=[S(1.0, 0, 0.5, 0.0, 0, half)], expect={0: 0}))   # c_0 = 0.5 >= top_p: one survives
    # min-p after top-p: p = .5 .3 .15 .05, top_p .82 keeps three (.5 .8 .95), min_p .2 (threshold .1) drops none of them; u ~ 0.9 > .8 / .95 picks the third
    x = np.full((1, 65), -30.0, np.float32)
    x[0, [7, 2, 40, 64]] = np.log(np.array([0.5, 0.3, 0.15, 0.05])).astype(np.float32)
    cases.append(llm_case("min_p_after_top_p", x, samp=[S(1.0, 40, 0.82, 0.2, 0, counter_with_u(0, 0.88, 0.97))], expect={0: 40}))
    # ---- each optional pointer NULL in turn (V = 65: greedy, masked greedy, sampled, masked sampled)
    x = (_rng(6).standard_normal((4, 65)) * 3).astype(np.float32)
    m = np.stack([_random_mask(_rng(7), 65, 0.4, junk=True)])
    samp = [GREEDY, GREEDY, S(1.0, 40, 0.95, 0.05, 3, 8), S(1.2, 0, 1.0, 0.0, SEED_BIG, 9)]
    for null in (("tok",), ("pos",), ("hist",), ("hist", "nsteps"), ("samp",), ("tok", "pos", "hist", "nsteps", "samp")):
        cases.append(llm_case("null_" + "_".join(null), x, m, [-1, 0, -1, 0], samp, null=null))
    cases.append(llm_case("null_masks", x, None, [-1] * 4, samp))
    cases.append(llm_case("null_masks_allow_row", x, None, None, samp))
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return cases


# ------------------------------------------------------------------------------------------ the ASR picks


def asr_case(name, kind, x, cols, temperature=0.0, seed=0, counter0=0, want_lp=False, compare_lp=True, expect=None, **filt):
    x = np.ascontiguousarray(x, np.float32)
    return dict(name=name, kind=kind, logits=x, rows=x.shape[0], cols=cols, ld=x.shape[1], temperature=float(np.float32(temperature)), seed=seed,
                counter0=counter0, want_lp=want_lp, compare_lp=compare_lp, expect=expect or {}, **filt)


def _with_gap(x, gap=5):
    """rows of pitch cols + gap, the gap filled with a sentinel larger than every logit"""
    return np.concatenate([x, np.full((x.shape[0], gap), GAP, np.float32)], axis=1)


def walk_rows(V, BEG, EOT, TID0):
    """the state-machine walk of tests/test_oracle_audio.py (text below EOT, specials EOT + 1 .. BEG - 1 always suppressed, timestamps from BEG, the
    first timestamp at most BEG + TID0), every step one row with the state the step before left; at V = 40, BEG = 30, EOT = 20 it is that test's
    vocabulary.  Returns logits, suppress, states in, expected tokens, expected states out."""
    sup = np.zeros(V, np.uint8)
    sup[EOT + 1:BEG] = 1
    sup[7] = 1
    T = lambda k: BEG + k   # noqa: E731
    rows = []

    def row(st, want_tok, want_st, **at):
        x = np.full(V, -5.0, np.float32)
        for i, v in at.items():
            x[int(i[1:])] = v
        rows.append((x, st, want_tok, want_st))

    # (a) first token: best timestamp beyond max_initial_ts, a suppressed text token largest of all, timestamps' sum beats the text
    row([0, 0, 0, 0, 0, 0, 0, 1000], T(2), [1, 1, 0, 1, 4, 1, 0, 1000], **{"i7": 30.0, "i%d" % T(8): 10.0, "i%d" % T(2): 5.0, "i3": 4.0})
    # (b) last token a timestamp and (fewer than two tokens) so was the one before: NO TIMESTAMP allowed
    row([1, 1, 0, 1, 4, 1, 0, 1000], 5, [2, 0, 1, 1, 4, 1, 0, 1000], **{"i%d" % T(5): 50.0, "i5": 1.0, "i6": 0.5})
    # (c) timestamps must not go back: BEG + 1 < BEG + seek_delta / 2 is masked although it is the largest
    row([2, 0, 1, 1, 4, 1, 0, 1000], T(5), [3, 1, 0, 1, 10, 3, 0, 1000], **{"i%d" % T(1): 40.0, "i%d" % T(5): 6.0, "i%d" % T(6): 5.9, "i4": 6.2})
    # (d) a timestamp after a text token: NO TEXT allowed, only its pair or the end of text
    row([3, 1, 0, 1, 10, 3, 0, 1000], EOT, [4, 0, 1, 1, 10, 3, 1, 1000], **{"i2": 20.0, "i%d" % EOT: 3.0, "i%d" % T(7): 1.0})
    # (e) a finished row stands still and emits eot
    row([4, 0, 1, 1, 10, 3, 1, 1000], EOT, [4, 0, 1, 1, 10, 3, 1, 1000], **{"i2": 20.0})
    # (f) text wins when its best token beats the timestamps' sum
    row([0, 0, 0, 0, 0, 0, 0, 1000], 9, [1, 0, 0, 0, 0, 0, 0, 1000], **{"i9": 8.0, "i%d" % T(0): 5.0, "i%d" % T(1): 5.0})
    # (g) end of text before any timestamp: a failure on a long utterance, a one-token result on a short one
    row([0, 0, 0, 0, 0, 0, 0, 1000], EOT, [1, 0, 0, 0, 0, 0, 2, 1000], **{"i%d" % EOT: 9.0})
    row([0, 0, 0, 0, 0, 0, 0, 100], EOT, [1, 0, 0, 0, 0, 1, 1, 100], **{"i%d" % EOT: 9.0})
    # (h) a short utterance ends with its first closing timestamp
    row([3, 0, 0, 0, 0, 0, 0, 110], T(6), [4, 1, 0, 1, 12, 4, 1, 110], **{"i%d" % T(6): 9.0})
    # (j) has_ts with seek_delta 10: timestamps from BEG + 5; the best one sits at BEG + 7, inside [BEG + seek_delta / 2, BEG + seek_delta)
    row([2, 0, 0, 1, 10, 1, 0, 1000], T(7), [3, 1, 0, 1, 14, 3, 0, 1000], **{"i%d" % T(7): 9.0, "i%d" % T(9): 6.0, "i4": 2.0})
    # (k) the timestamps' summed probability EQUALS the best text token's (one timestamp with the text's logit, the other allowed ones -inf: the sum is
    #     exactly one term in float32 and float64 alike): text stays, and the first maximum is the text token
    row([0, 0, 0, 0, 0, 0, 0, 1000], 4, [1, 0, 0, 0, 0, 0, 0, 1000], **{"i4": 5.0, "i%d" % T(0): 5.0, "i%d" % T(1): NINF, "i%d" % T(2): NINF, "i%d" % T(3): NINF})
    x, st, tok, st2 = (np.array(v) for v in zip(*rows))
    return x.astype(np.float32), sup, st.astype(np.int32), tok.astype(np.int32), st2.astype(np.int32)


def _generic_filtered(V):
    """random logits through the filter at every vocabulary size: a fresh row, a row after text, after (text, timestamp), after two timestamps"""
    rng = _rng(8, V)
    beg = V // 2 if V >= 31 else V
    eot = max(beg - 1, 0)
    sup = (rng.random(V) < 0.1).astype(np.uint8)
    sup[eot] = 0
    if beg < V:
        sup[beg:beg + 4] = 0
    sts = [[0, 0, 0, 0, 0, 0, 0, 1000]]
    if V >= 31:
        sts += [[2, 0, 1, 1, 4, 1, 0, 1000], [3, 1, 0, 1, 6, 3, 0, 1000], [2, 1, 1, 1, 4, 2, 0, 1000], [5, 0, 0, 0, 0, 0, 1, 1000]]
        sup[0:3] = 0
    tid0 = 3 if beg < V else -1
    x = (rng.standard_normal((len(sts), V)) * 3).astype(np.float32)
    return x, sup, np.array(sts, np.int32), beg, eot, tid0


@functools.lru_cache(maxsize=None)
def asr_cases():
    cases = []
    for V in VOCABS_ALL:
        x = _with_gap((_rng(9, V).standard_normal((3, V)) * 3).astype(np.float32))
        cases.append(asr_case("argmax_rows_v%d" % V, PICK_ARGMAX_ROWS, x, V))
        for T in (0.0, 1.0) + ((0.7,) if V == 1000 else ()):                                          # 0.7: the division by the temperature rounds
            cases.append(asr_case("pick_rows_v%d_t%g_lp" % (V, T), PICK_ROWS, x, V, T, SEED_BIG if V % 2 else 0, 17, want_lp=True))
        if V in (33, 1025):
            for T in (0.0, 1.0):
                cases.append(asr_case("pick_rows_v%d_t%g" % (V, T), PICK_ROWS, x, V, T, 3, 2 ** 32 - 2))   # counter0 + row wraps
        fx, sup, st, beg, eot, tid0 = _generic_filtered(V)
        for T in (0.0, 1.0) + ((0.7,) if V == 1000 else ()):
            cases.append(asr_case("filtered_v%d_t%g" % (V, T), PICK_ROWS_FILTERED, _with_gap(fx), V, T, 5, 100, want_lp=True, suppress=sup, state=st, beg=beg,
                                  eot=eot, tid0=tid0))
    t = _tie_rows()
    want = {r: e for r, e in enumerate([5, 5, 70, 6, 0, 1500, 0])}
    cases.append(asr_case("argmax_rows_ties", PICK_ARGMAX_ROWS, _with_gap(t), 2100, expect=want))
    cases.append(asr_case("pick_rows_ties", PICK_ROWS, _with_gap(t), 2100, want_lp=True, expect=want))
    sp = _special_rows()
    want = {0: 777, 1: 0, 2: 333, 3: 0}
    cases.append(asr_case("argmax_rows_special", PICK_ARGMAX_ROWS, sp, 1000, expect=want))
    cases.append(asr_case("pick_rows_special", PICK_ROWS, sp, 1000, expect=want))                     # row 1: nothing above -inf -> index 0
    cases.append(asr_case("pick_rows_special_lp", PICK_ROWS, sp[[0, 2, 3, 4]], 1000, want_lp=True, expect={0: 777, 1: 333, 2: 0}))
    cases.append(asr_case("pick_rows_all_ninf_lp", PICK_ROWS, sp[[1]], 1000, want_lp=True, compare_lp=False, expect={0: 0}))   # its logprob is NaN: not compared
    z = np.array([[-0.0, 0.0], [0.0, -0.0]], np.float32)
    cases.append(asr_case("argmax_rows_signed_zeros", PICK_ARGMAX_ROWS, z, 2, expect={0: 0, 1: 0}))
    cases.append(asr_case("pick_rows_signed_zeros", PICK_ROWS, z, 2, want_lp=True, expect={0: 0, 1: 0}))
    # the filter's state machine: the oracle test's toy vocabulary, then 1000 tokens with beg = 500 (inside a mask word) and beg = 512 (on a word boundary)
    for V, BEG, EOT in ((40, 30, 20), (1000, 500, 490), (1000, 512, 490)):
        x, sup, st, tok, st2 = walk_rows(V, BEG, EOT, 3)
        cases.append(asr_case("filtered_walk_v%d_beg%d" % (V, BEG), PICK_ROWS_FILTERED, _with_gap(x), V, want_lp=True, suppress=sup, state=st, beg=BEG, eot=EOT, tid0=3,
                              expect=dict(enumerate(tok.tolist())), expect_state=st2))
        # temperature 1 with the mask entering the draw: after (a) no timestamp is allowed; eight rows = eight counters
        x = np.tile(np.linspace(-1, 1, V, dtype=np.float32), (8, 1))
        st0 = np.tile(np.array([1, 1, 0, 1, 4, 1, 0, 1000], np.int32), (8, 1))
        cases.append(asr_case("filtered_hot_v%d_beg%d" % (V, BEG), PICK_ROWS_FILTERED, x, V, 1.0, 5, 0, want_lp=True, suppress=sup, state=st0, beg=BEG, eot=EOT, tid0=3))
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return cases


def refusals(max_rows):
    """(name, token_pick_probe keyword arguments) the hook must refuse with TK_ERROR_INVALID_ARGUMENT before anything is launched"""
    x = np.linspace(-1, 1, 2 * 40, dtype=np.float32).reshape(2, 40)
    m = np.stack([R.mask_words(40, range(40)), R.mask_words(40, [3])])
    z = lambda n=2: np.zeros(n, np.int32)   # noqa: E731
    llm = dict(kind=PICK_ARGMAX, logits=x, rows=2, cols=40, masks=m, allow_row=[0, 1], tok=z(), pos=z(), nsteps=z(), hist=np.zeros(8, np.int32), hist_stride=2)
    wide = np.zeros((1, 65537), np.float32)
    pick = dict(kind=PICK_ROWS, logits=x, rows=2, cols=40, tok=z(), logprob=np.zeros(2, np.float32))
    sup = np.zeros(40, np.uint8)
    st = np.zeros((2, 8), np.int32)
    filt = dict(pick, kind=PICK_ROWS_FILTERED, suppress=sup, state=st, beg=30, eot=20, tid0=3)
    samp = lambda t: [S(t), S(0.0)]   # noqa: E731
    from trackiellm_amd import sampling_rows
    out = [("mask index = n_masks", dict(llm, allow_row=[0, 2])), ("mask index -2", dict(llm, allow_row=[-2, 0])),
           ("mask index without masks", dict(llm, masks=None, allow_row=[0, -1])),
           ("k_argmax: ld > cols", dict(llm, ld=41, logits=np.zeros((2, 41), np.float32))), ("ld < cols", dict(pick, ld=39)),
           ("rows 0", dict(llm, rows=0)), ("rows > max", dict(llm, rows=max_rows + 1, logits=np.zeros((max_rows + 1, 40), np.float32), masks=None, allow_row=None,
                                                             tok=z(max_rows + 1), pos=None, nsteps=None, hist=None)),
           ("pick rows 0", dict(pick, rows=0)), ("logits too short", dict(pick, logits=x.reshape(-1)[:-1])),
           ("sampled row beyond 65536", dict(kind=PICK_ARGMAX, logits=wide, rows=1, cols=65537, samp=sampling_rows([S(1.0)]), tok=z(1))),
           ("hot pick beyond 65536", dict(kind=PICK_ROWS, logits=wide, rows=1, cols=65537, tok=z(1), temperature=1.0)),
           ("filtered beyond 65536", dict(kind=PICK_ROWS_FILTERED, logits=wide, rows=1, cols=65537, tok=z(1), suppress=np.zeros(65537, np.uint8), state=st[:1], beg=30,
                                          eot=20)),
           ("hist too small for nsteps", dict(llm, nsteps=[0, 4])), ("nsteps negative", dict(llm, nsteps=[-1, 0])), ("hist without nsteps", dict(llm, nsteps=None)),
           ("hist_stride < rows", dict(llm, hist_stride=1))]
    for bad in (-1.0, float("nan"), float("inf")):
        out += [("sampling temperature %r" % bad, dict(llm, samp=sampling_rows(samp(bad)))), ("pick temperature %r" % bad, dict(pick, temperature=bad)),
                ("filter temperature %r" % bad, dict(filt, temperature=bad))]
    out += [("argmax_rows with logprob", dict(pick, kind=PICK_ARGMAX_ROWS)), ("filter: nothing allowed", dict(filt, suppress=np.ones(40, np.uint8))),
            ("filter: NaN logit", dict(filt, logits=np.where(np.arange(80).reshape(2, 40) == 45, np.nan, x).astype(np.float32))),
            ("filter: eot outside", dict(filt, eot=40)), ("filter: beg outside", dict(filt, beg=41)), ("filter: no state", dict(filt, state=None)),
            ("unknown kind", dict(pick, kind=4))]
    accepted = [("k_argmax greedy beyond 65536", dict(kind=PICK_ARGMAX, logits=wide, rows=1, cols=65537, samp=sampling_rows([S(0.0)]), tok=z(1))),
                ("base k_argmax", llm), ("base pick", pick), ("base filter", filt)]
    return out, accepted
