"""References for the five token-selection kernels (k_argmax, sample_row, k_argmax_rows, k_pick_rows, k_pick_rows_filtered).

Reference A is the oracle (oracle_lib: sample_row, pick_row, whisper_filter_pick), compared bit for bit.  This file is reference B: plain NumPy in
float64, written from the comments above the kernels (csrc/llm/tk_llm_kernels.hip "sampling", csrc/nn/tk_nn_kernels.hip above k_pick_rows and
k_pick_rows_filtered), not from the oracle's source.  It owns nothing of the kernels' arithmetic order: the candidate list, the greedy pick, the masks
and the filtered pick's allowed set are exact decisions and never abstain; the three float32 comparisons of the sampler (c >= top_p,
p_i < min_p p_0, c > u W) are decided here in float64 and reported as `abstain` when the float64 margin is below MARGIN relative.

Every function takes `mut`, a set of mutation switches: each one is one plausible kernel error.  tests/test_token_pick_cpu.py shows that every switch
changes the answer of at least one case the GPU file runs."""
import numpy as np

EPS = 2.0 ** -24          # float32 unit roundoff
MARGIN = 1e-4             # relative float64 margin under which reference B does not decide a float32 comparison
MAX_K = 64
# tk_logf documents no error (csrc/common/tk_exact_math.h).  Measured on the CPU against numpy.float64 over S in [1, 65536] (the range of a sum of
# exponentials whose largest term is 1 over at most 65536 tokens): 5.4e-7 at its worst over a million arguments; held here under 2^-20 (1 ulp of a
# result in [8, 16)), absolute.  tk_expf: relative 2^-22 — dropping r^7 / 7! at |r| = ln 2 / 2 is 1.7e-7 of exp(r), the roundings of the reduction and
# the polynomial make up the rest; measured 1.91 x 2^-23 at its worst over 1.7 million arguments in [-87, 0] (the header said 1 ulp until this
# measurement).  test_tk_logf_and_tk_expf_error_is_inside_the_constants_of_the_bound measures both again on every run.
LOGF_ABS_ERR = 2.0 ** -20
EXPF_REL_ERR = 2.0 ** -22

MUTATIONS = (
    "tie_chain_later", "tie_lane_higher", "tie_wave_higher", "tie_wave_lower",  # greedy: a merge preferring the later chain element / higher lane / a wave
    "ties_high_id",          # sampler order and the ASR greedy picks: ties to the higher id
    "kth_from_high",         # the tie at the K-th place filled from the high ids
    "zero_equal",            # -0 and +0 one key in the sampler's order
    "mask_wrong_row",        # mask bits read from another row's mask
    "junk_bits",             # bits past `vocab` in the last mask word honoured
    "top_p_gt",              # top-p: c > top_p instead of c >= top_p
    "draw_ge",               # draw: c >= u W instead of c > u W
    "min_p_first",           # min-p (renormalised) before top-p
    "top_k0_is_1",           # top_k = 0 meaning 1 instead of 64
    "top_k_unclamped",       # top_k > 64 not clamped
    "counter_on_greedy",     # counter advanced on greedy rows
    "pos_not_advanced",
    "hist_plus_one",         # hist written at nsteps + 1
    "ts_rule_ge",            # filtered: timestamps win at lp_ts >= m_tx
    "straddle_word_whole",   # filtered: the mask word straddling `beg` cleared whole
    "ts_lo_no_half",         # filtered: ts_lo = beg + seek_delta
    "prev_not_shifted",      # filtered: state slot 2 keeps its value
)


def splitmix_u(seed, counter):
    """u in [0, 1): the top 24 bits of splitmix64 keyed by (seed, counter), times 2^-24"""
    M = (1 << 64) - 1
    z = (int(seed) + 0x9E3779B97F4A7C15 * (int(counter) + 1)) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    z ^= z >> 31
    return (z >> 40) * 2.0 ** -24


def order_key(x, zero_equal=False):
    """int64 whose order is the float32 order with -0 < +0 (zero_equal: -0 == +0)"""
    b = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    mag = b & 0x7FFFFFFF
    return np.where(b < 0, -mag - (0 if zero_equal else 1), mag)


def mask_words(vocab, allowed_ids, junk=False):
    """(vocab + 31) / 32 uint32 words with the bits of allowed_ids set; junk: the bits past vocab in the last word set too"""
    w = np.zeros((vocab + 31) // 32, np.uint32)
    for i in allowed_ids:
        w[i >> 5] |= np.uint32(1 << (i & 31))
    if junk and vocab % 32:
        w[-1] |= np.uint32((0xFFFFFFFF << (vocab % 32)) & 0xFFFFFFFF)
    return w


def allowed_of(flat, r, vocab, masks, mi, mut=()):
    """ids a row may pick and their logits.  flat: the launch's packed logits; a mutant that honours bits past vocab reads on into the next row"""
    if masks is None or mi < 0:
        ids = np.arange(vocab)
    else:
        if "mask_wrong_row" in mut:
            mi = (mi + 1) % len(masks)
        n = 32 * masks.shape[1] if "junk_bits" in mut else vocab
        i = np.arange(n)
        ids = i[((masks[mi][i >> 5] >> (i & 31).astype(np.uint32)) & 1) == 1]
    at = r * vocab + ids
    vals = np.where(at < flat.size, flat[np.minimum(at, flat.size - 1)], np.float32(-np.inf)).astype(np.float32)
    return ids, vals


def greedy_pick(ids, vals, mut=()):
    """first index of the maximum (any -inf, -0 == +0); no candidate: 0"""
    if len(ids) == 0:
        return 0
    tie = ids[vals == vals.max()]
    if "ties_high_id" in mut:
        return int(tie.max())
    chain = tie % 1024
    per_chain = {}
    for i, c in zip(tie.tolist(), chain.tolist()):                      # a thread walks i = t, t + 1024, ... ascending
        per_chain[c] = max(per_chain.get(c, i), i) if "tie_chain_later" in mut else min(per_chain.get(c, i), i)
    per_wave = {}
    for c, i in per_chain.items():                                      # 64 chains per wave
        w = c // 64
        if w not in per_wave:
            per_wave[w] = (c, i)
        elif "tie_lane_higher" in mut:
            per_wave[w] = max(per_wave[w], (c, i))
        else:
            per_wave[w] = min(per_wave[w], (c, i), key=lambda ci: ci[1])
    if "tie_wave_higher" in mut:
        return per_wave[max(per_wave)][1]
    if "tie_wave_lower" in mut:
        return per_wave[min(per_wave)][1]
    return min(i for _, i in per_wave.values())


def candidates(ids, vals, top_k, mut=()):
    """the first K = min(top_k or 64, 64, allowed) tokens by (logit descending with -0 < +0, id ascending)"""
    K = top_k if top_k > 0 else (1 if "top_k0_is_1" in mut else MAX_K)
    if "top_k_unclamped" not in mut:
        K = min(K, MAX_K)
    K = min(K, len(ids))
    key = order_key(vals, "zero_equal" in mut)
    order = np.lexsort((-ids if "ties_high_id" in mut else ids, -key))
    if "kth_from_high" in mut and K > 0:
        kth = key[order[K - 1]]
        above = order[key[order] > kth]
        ties = order[key[order] == kth]
        return ids[np.concatenate([above, ties[len(ties) - (K - len(above)):]])]
    return ids[order[:K]]


def _close(a, b):
    return abs(a - b) < MARGIN * abs(b) if b != 0 else a == 0


def sample_pick(ids, vals, temp, top_k, top_p, min_p, seed, counter, mut=()):
    """one draw of the canonical sampler in float64 -> (id, abstain, candidate ids in order)"""
    if len(ids) == 0:
        return 0, False, np.zeros(0, np.int64)
    cand = candidates(ids, vals, top_k, mut)
    look = dict(zip(ids.tolist(), vals.tolist()))
    l = np.array([look[i] for i in cand.tolist()], np.float64)
    e = np.exp(l - l[0])
    p = e / e.sum()
    n, abstain = len(cand), False

    def top_p_cut(p, n):
        nonlocal abstain
        if not top_p < 1.0:
            return n
        c = 0.0
        for i in range(n):
            c += p[i]
            abstain = abstain or _close(c, top_p)
            if (c > top_p) if "top_p_gt" in mut else (c >= top_p):
                return i + 1
        return n

    def min_p_cut(p, n):
        nonlocal abstain
        if not min_p > 0.0:
            return n
        while n > 1:
            abstain = abstain or _close(p[n - 1], min_p * p[0])
            if not p[n - 1] < min_p * p[0]:
                break
            n -= 1
        return n

    if "min_p_first" in mut:
        n = min_p_cut(p, n)
        n = top_p_cut(p / p[:n].sum(), n)
    else:
        n = min_p_cut(p, top_p_cut(p, n))
    w = np.exp((l[:n] - l[0]) / np.float64(np.float32(temp)))
    target = splitmix_u(seed, counter) * w.sum()
    c, pick = 0.0, n - 1
    for i in range(n):
        c += w[i]
        abstain = abstain or _close(c, target)
        if (c >= target) if "draw_ge" in mut else (c > target):
            pick = i
            break
    return int(cand[pick]), abstain, cand


def ref_argmax_launch(case, mut=()):
    """what ONE k_argmax launch leaves behind: tok / pos / nsteps / hist / counters as the caller handed them in, moved on by one token per row"""
    x = case["logits"]
    rows, vocab = x.shape
    flat = x.reshape(-1)
    samp = case.get("samp")
    given = lambda k, fill: np.array(case[k]) if case.get(k) is not None else fill   # noqa: E731
    out = dict(tok=given("tok", np.zeros(rows, np.int32)), pos=given("pos", np.zeros(rows, np.int32)), nsteps=given("nsteps", None), hist=given("hist", None),
               counter=None if samp is None else np.array([s[5] for s in samp], np.uint32), abstain=np.zeros(rows, bool), sampled=np.zeros(rows, bool),
               cands=[None] * rows)
    stride = case["hist_stride"]
    for r in range(rows):
        mi = -1 if case.get("allow_row") is None else int(case["allow_row"][r])
        ids, vals = allowed_of(flat, r, vocab, case.get("masks"), mi, mut)
        if samp is not None and samp[r][0] > 0.0:
            temp, top_k, top_p, min_p, seed, counter = samp[r]
            tok, out["abstain"][r], out["cands"][r] = sample_pick(ids, vals, temp, top_k, top_p, min_p, seed, counter, mut)
            out["sampled"][r] = True
            out["counter"][r] = (int(out["counter"][r]) + 1) & 0xFFFFFFFF   # a uint32 on the device
        else:
            tok = greedy_pick(ids, vals, mut)
            if samp is not None and "counter_on_greedy" in mut:
                out["counter"][r] = (int(out["counter"][r]) + 1) & 0xFFFFFFFF   # a uint32 on the device
        out["tok"][r] = tok
        if "pos_not_advanced" not in mut:
            out["pos"][r] += 1
        if out["hist"] is not None:                                       # without a history the step counts stay too
            n = int(out["nsteps"][r])
            out["hist"][(n + (1 if "hist_plus_one" in mut else 0)) * stride + r] = tok
            out["nsteps"][r] = n + 1
    for k in ("tok", "pos"):
        if case.get(k) is None:
            out[k + "_unseen"], out[k] = out[k], None                     # computed, but the launch has nowhere to put it
    return out


def logprob64(z_allowed, z_tok):
    """z_tok - log sum exp z over the allowed tokens, float64"""
    z = np.asarray(z_allowed, np.float64)
    m = z.max()
    return float((z_tok - m) - np.log(np.exp(z - m).sum()))                 # the maximum first: it may be 3.4e38 in magnitude


def logprob_bound(z_allowed, z_tok, cols, hot, div_first=False):
    """|float32 kernel logprob - float64| for lp = (z_tok - max) - log S, S = sum exp(z_i - max), term by term (first order, 1 % for the rest):
    the argument z_i - max is one rounded subtraction, EPS |z_i - max|; at a temperature one rounded division more, of the difference
    (k_pick_rows: EPS |z_i - max| again) or of the logit itself before the subtraction (div_first, k_pick_rows_filtered: EPS |z_i|; the
    rounding of the maximum shifts z_tok and log S alike and cancels).  That absolute error of the argument is a relative error of exp;
    tk_expf adds EXPF_REL_ERR.  The additions: a chain of at most ceil(cols / 1024) terms, a 6-level butterfly and 15 sequential joins of
    non-negative numbers, each rounding once: (chain + 6 + 15) EPS of S.  log S: the relative error of S, plus tk_logf's own error.  z_tok
    carries its argument's error; the last subtraction rounds once: EPS |lp|."""
    raw = np.asarray(z_allowed, np.float64)
    z = raw - raw.max()
    zt = z_tok - raw.max()
    arg = lambda d, v: EPS * abs(d) + (0.0 if not hot else EPS * abs(v) if div_first else EPS * abs(d))   # noqa: E731
    term = np.exp(z)
    S = term.sum()
    fin = np.isfinite(z)                                                   # a -inf logit is a term of exactly 0 on both sides
    rel_S = float((term[fin] * (arg(z[fin], raw[fin]) + EXPF_REL_ERR)).sum() / S) + (-(-cols // 1024) + 6 + 15) * EPS
    lp = zt - np.log(S)
    return 1.01 * (rel_S + LOGF_ABS_ERR + arg(zt, z_tok) + EPS * abs(lp))


def ref_pick_row(x, temperature, seed, counter, mut=()):
    """k_argmax_rows / k_pick_rows on one row -> (token, abstain)"""
    ids = np.arange(len(x))
    if temperature > 0.0:
        tok, abstain, _ = sample_pick(ids, x, temperature, 0, 1.0, 0.0, seed, counter, mut)
    else:
        tok, abstain = greedy_pick(ids, x, mut), False
    return tok, abstain


def filtered_allowed(cols, suppress, st, beg, eot, tid0, mut=()):
    """A0 of k_pick_rows_filtered's comment: not in the static table; first token: no timestamp above beg + tid0; last token a timestamp: (the one
    before too: no timestamp) / (otherwise: nothing below eot); has_ts: no timestamp below beg + seek_delta / 2"""
    n_tok, has_ts, seek_delta = int(st[0]), int(st[3]), int(st[4])
    last_ts = n_tok > 0 and st[1] != 0
    prev_ts = n_tok < 2 or st[2] != 0
    i = np.arange(cols)
    ok = np.asarray(suppress) == 0
    ts = i >= beg
    if last_ts and prev_ts:
        ok &= ~ts
    if last_ts and not prev_ts:
        ok &= i >= eot
    if n_tok == 0 and tid0 >= 0:
        ok &= ~(ts & (i > beg + tid0))
    if has_ts:
        ok &= ~(ts & (i < beg + (seek_delta if "ts_lo_no_half" in mut else seek_delta // 2)))
    return ok


def ref_filtered_row(x, suppress, st, beg, eot, tid0, temperature, seed, counter, mut=()):
    """one row of k_pick_rows_filtered in float64 -> dict(tok, state, live, abstain, allowed (final set A), a0, ts_margin = lp_ts - m_tx)"""
    st = np.array(st, np.int32)
    if st[6] != 0:
        return dict(tok=eot, state=st, live=False, abstain=False, allowed=None, a0=None, ts_margin=None)
    cols = len(x)
    ok = filtered_allowed(cols, suppress, st, beg, eot, tid0, mut)
    a0 = ok.copy()
    hot = temperature > 0.0
    z = np.asarray(x, np.float64) / (np.float64(np.float32(temperature)) if hot else 1.0)
    i = np.arange(cols)
    with np.errstate(divide="ignore", invalid="ignore"):
        lse = lambda v: v.max() + np.log(np.exp(v - v.max()).sum()) if len(v) else -np.inf   # noqa: E731
        lp = z - lse(z[ok])
        lp_ts = lse(lp[ok & (i >= beg)])
        m_tx = lp[ok & (i < beg)].max() if (ok & (i < beg)).any() else -np.inf
        margin = float(lp_ts - m_tx)
    if (lp_ts >= m_tx) if "ts_rule_ge" in mut else (lp_ts > m_tx):
        ok &= i >= beg
        if "straddle_word_whole" in mut and beg % 32:
            ok &= i >= (beg // 32 + 1) * 32
    ids = i[ok]
    if hot:
        tok, abstain, _ = sample_pick(ids, np.asarray(x, np.float32)[ok], temperature, 0, 1.0, 0.0, seed, counter, mut)
    else:
        tok, abstain = greedy_pick(ids, np.asarray(x, np.float32)[ok], mut), False
    # whisper_full's bookkeeping of the sampled token
    n = int(st[0])
    hts, sd, rl, status, seek_end = int(st[3]), int(st[4]), int(st[5]), 0, int(st[7])
    if tok > beg:
        sd_new = 2 * (tok - beg)
        if hts and sd > sd_new and rl < n:
            status = 2
        else:
            sd, rl, hts = sd_new, n + 1, 1
    if status == 0 and (tok == eot or (hts and sd + 100 >= seek_end)):
        if rl == 0:
            if sd + 100 >= seek_end:
                rl = n + 1
            else:
                status = 2
        if status == 0:
            status = 1
    was_last = 1 if (n > 0 and st[1] != 0) else 0
    new = np.array([n + 1, 1 if tok >= beg else 0, int(st[2]) if "prev_not_shifted" in mut else was_last, hts, sd, rl, status, seek_end], np.int32)
    return dict(tok=tok, state=new, live=True, abstain=abstain, allowed=ok, a0=a0, ts_margin=margin if np.isfinite(margin) else None)


# ------------------------------------------------------------------------------------------ whole launches, on either reference


def ref_asr_launch(case, mut=()):
    """reference B over one launch of k_argmax_rows (kind 1), k_pick_rows (2) or k_pick_rows_filtered (3) -> dict(tok, state, live, abstain, sampled)"""
    rows, cols, kind = case["rows"], case["cols"], case["kind"]
    T = case["temperature"] if kind != 1 else 0.0
    out = dict(tok=np.zeros(rows, np.int32), state=None if kind != 3 else np.array(case["state"]), live=np.ones(rows, bool), abstain=np.zeros(rows, bool),
               sampled=np.full(rows, T > 0.0), a0=[None] * rows)
    for r in range(rows):
        x = case["logits"][r, :cols]
        counter = (case["counter0"] + r) & 0xFFFFFFFF
        if kind != 3:
            out["tok"][r], out["abstain"][r] = ref_pick_row(x, T, case["seed"], counter, mut)
            continue
        f = ref_filtered_row(x, case["suppress"], case["state"][r], case["beg"], case["eot"], case["tid0"], T, case["seed"], counter, mut)
        out["tok"][r], out["state"][r], out["live"][r], out["abstain"][r], out["a0"][r] = f["tok"], f["state"], f["live"], f["abstain"], f["a0"]
        out["sampled"][r] = f["live"] and T > 0.0
    return out


def oracle_argmax_launch(case):
    """reference A over one k_argmax launch: the oracle's id per row, the bookkeeping of ref_argmax_launch around it"""
    import oracle_lib as O
    out = ref_argmax_launch(case)
    tok = out["tok"] if out["tok"] is not None else out["tok_unseen"]
    samp = case.get("samp")
    for r in range(case["logits"].shape[0]):
        mi = -1 if case.get("allow_row") is None else int(case["allow_row"][r])
        allow = case["masks"][mi] if mi >= 0 else None
        temp, top_k, top_p, min_p, seed, counter = samp[r] if samp is not None else (0.0, 0, 1.0, 0.0, 0, 0)
        tok[r] = O.sample_row(case["logits"][r], temp, top_k, top_p, min_p, seed, counter, allow)
        if out["hist"] is not None:
            out["hist"][int(case["nsteps"][r]) * case["hist_stride"] + r] = tok[r]
    return out


def oracle_asr_launch(case):
    """reference A over one ASR pick launch -> dict(tok, logprob (float32, 0 on rows that stand still) or None, state)"""
    import oracle_lib as O
    rows, cols, kind = case["rows"], case["cols"], case["kind"]
    tok = np.zeros(rows, np.int32)
    lp = np.zeros(rows, np.float32) if case["want_lp"] else None
    state = None if kind != 3 else np.array(case["state"], np.int32)
    for r in range(rows):
        x = np.ascontiguousarray(case["logits"][r, :cols])
        counter = (case["counter0"] + r) & 0xFFFFFFFF
        if kind == 3:
            tok[r], v = O.whisper_filter_pick(x, case["suppress"], state[r], case["beg"], case["eot"], case["tid0"], case["temperature"], case["seed"], counter)
        else:
            tok[r], v = O.pick_row(x, case["temperature"] if kind == 2 else 0.0, case["seed"], counter, want_logprob=case["want_lp"])
        if lp is not None:
            lp[r] = np.float32(v)
    return dict(tok=tok, logprob=lp, state=state)


def logprob_reference(case, r, tok, a0=None):
    """(float64 log-probability of `tok` on row r, bound on a float32 kernel's distance from it); a0: the filtered pick's allowed set"""
    x = case["logits"][r, :case["cols"]].astype(np.float64)
    hot = case["temperature"] > 0.0
    z = x / np.float64(np.float32(case["temperature"])) if hot else x
    za = z if a0 is None else z[a0]
    return logprob64(za, z[tok]), logprob_bound(za, z[tok], case["cols"], hot, div_first=a0 is not None)
