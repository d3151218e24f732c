"""CPU: the log-probability record's definition (csrc/common/tk_token_logprob.h) through the probe's host loop (device = -1), no GPU touched.

- the host loop equals the float32 NumPy restatement bit for bit and stands inside the float64 bound on every case of tests/token_logprob_cases.py,
  off rows and the entries past a record's count untouched;
- the list is the prefix of the sampler's candidate list for an unmasked row (tests/token_pick_ref.candidates: the oracle library exposes the
  sampler's pick, not its candidate order);
- every refusal of the probe, with the arrays untouched;
- every mutation switch of the reference changes at least one case."""
import functools

import numpy as np
import pytest

import token_logprob_cases as LC
import token_logprob_ref as R
import token_pick_ref as PR


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(LC.cases())


@functools.lru_cache(maxsize=None)
def expected(name, mut=""):
    """per live row of a case: reference A's (logprob, ids, logprobs), computed once and shared"""
    c = next(c for c in all_cases() if c["name"] == name)
    m = (mut,) if mut else ()
    return {r: R.record32(LC.row_of(c, r), int(c["ids"][r]), int(c["n_top"][r]), m, c["masks"][r], c["temp"]) for r in range(c["rows"]) if c["n_top"][r] >= 0}


def check_records(c, rec, sent):
    """rec against reference A, bit for bit, and the sentinels"""
    want = expected(c["name"])
    for r in range(c["rows"]):
        if c["n_top"][r] < 0:
            assert rec[r].tobytes() == sent[r].tobytes(), (c["name"], r, "an off row was written")
            continue
        lp, ids, lps = want[r]
        n = min(int(c["n_top"][r]), c["cols"])
        assert rec["n_top"][r] == n == len(ids), (c["name"], r, int(rec["n_top"][r]), n)
        assert bits(rec["logprob"][r]) == bits(lp), (c["name"], r, c["kinds"][r], float(rec["logprob"][r]), float(lp))
        assert rec["top_ids"][r, :n].tolist() == ids.tolist(), (c["name"], r, c["kinds"][r])
        assert np.array_equal(bits(rec["top_logprobs"][r, :n]), bits(lps)), (c["name"], r, c["kinds"][r])
        assert np.all(rec["top_ids"][r, n:] == LC.S_ID) and np.all(rec["top_logprobs"][r, n:] == LC.S_LP), (c["name"], r, "entries past the count were written")


def run_probe(tk, c, device):
    sent = LC.sentinel_records(c["rows"])
    lg = c["logits"].copy()
    rec = tk.token_logprobs_probe(lg, c["rows"], c["cols"], c["ids"], c["n_top"], records=sent.copy(), ld=c["ld"], device=device)
    assert lg.tobytes() == c["logits"].tobytes()
    return rec, sent


@pytest.mark.parametrize("name", [c["name"] for c in LC.cases()])
def test_host_loop_equals_the_float32_restatement_and_stands_inside_the_float64_bound(tk, name):
    c = next(c for c in all_cases() if c["name"] == name)
    rec, sent = run_probe(tk, c, -1)
    check_records(c, rec, sent)
    worst = 0.0
    for r in range(c["rows"]):
        if c["n_top"][r] < 0:
            continue
        n = int(rec["n_top"][r])
        lp, b, ids, lps, bs = R.record64(LC.row_of(c, r), int(c["ids"][r]), int(c["n_top"][r]))
        assert rec["top_ids"][r, :n].tolist() == ids.tolist()
        for got, want, bound in [(rec["logprob"][r], lp, b)] + list(zip(rec["top_logprobs"][r, :n], lps, bs)):
            if np.isneginf(want):
                assert np.isneginf(got), (name, r)
                continue
            err = abs(float(got) - float(want))
            assert err <= bound, (name, r, c["kinds"][r], float(got), float(want), err, bound)
            worst = max(worst, err / bound)
        if c["kinds"][r] == "equal":   # every log-probability is -log(cols) inside the bound, ids ascending
            assert rec["top_ids"][r, :n].tolist() == list(range(n))
            assert abs(float(rec["logprob"][r]) + np.log(c["cols"])) <= b
        if c["kinds"][r] == "chosen_ninf" and c["cols"] > 1:
            assert np.isneginf(rec["logprob"][r])
        if c["kinds"][r] == "dominant" and c["cols"] > 1 and n > 1:
            assert rec["top_logprobs"][r, 0] == 0.0 and np.all(rec["top_logprobs"][r, 1:n] <= -100.0)
    print(name, "worst error / bound = %.2f" % worst)


def test_the_list_is_the_prefix_of_the_samplers_candidates(tk):
    seen = 0
    for c in all_cases():
        rec, _ = run_probe(tk, c, -1)
        for r in range(c["rows"]):
            n = int(c["n_top"][r])
            if n < 1:
                continue
            x = LC.row_of(c, r)
            cand = PR.candidates(np.arange(c["cols"]), x, 0)       # top_k 0: the 64 first tokens of an unmasked row
            k = min(n, c["cols"])
            assert rec["top_ids"][r, :k].tolist() == cand[:k].tolist(), (c["name"], r, c["kinds"][r])
            if c["kinds"][r] == "zeros":                            # +0 before -0, then ids ascending inside each
                top = x[rec["top_ids"][r, :min(k, 6)]]
                sign = np.signbit(top[top == 0.0])
                assert np.array_equal(sign, np.sort(sign)), (c["name"], r)
            seen += 1
    assert seen >= 40


def test_the_probe_refuses_with_the_arrays_untouched(tk):
    max_rows = tk.lib().tk_mi355x_llm_max_rows()
    for name, kw in LC.refusals(max_rows):
        rows = max(int(kw["rows"]), 1)
        sent = LC.sentinel_records(rows)
        rec, lg = sent.copy(), kw["logits"].copy()
        with pytest.raises(tk.TkError) as e:
            tk.token_logprobs_probe(lg, kw["rows"], kw["cols"], kw["ids"], kw["n_top"], records=rec, ld=kw["ld"], device=-1, n_logits=kw.get("n_logits"))
        assert e.value.code == 1001, name
        assert rec.tobytes() == sent.tobytes() and lg.tobytes() == kw["logits"].tobytes(), name
    for name, kw in LC.accepted_oddities():
        rec = tk.token_logprobs_probe(kw["logits"], kw["rows"], kw["cols"], kw["ids"], kw["n_top"], records=LC.sentinel_records(kw["rows"]), ld=kw["ld"], device=-1)
        assert rec[0].tobytes() == LC.sentinel_records(1)[0].tobytes() and rec["n_top"][1] == 2, name


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_mutant_of_the_reference_is_noticed_by_a_case(mut):
    def flat(name, m):
        return [(r, bits(lp).tolist(), ids.tolist(), bits(lps).tolist()) for r, (lp, ids, lps) in sorted(expected(name, m).items())]

    noticed = [c["name"] for c in all_cases() if flat(c["name"], "") != flat(c["name"], mut)]
    print(mut, "noticed by", noticed[:6])
    assert noticed, "no case notices the mutation %r: a case is missing" % mut
