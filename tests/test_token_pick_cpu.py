"""CPU: the cases of tests/test_token_pick_gpu.py discriminate, and the oracle (reference A) stands inside everything the GPU file asks of the kernels.

- every mutation switch of tests/token_pick_ref.py (one plausible kernel error each) changes the answer of at least one GPU case;
- reference B (float64 NumPy) and the oracle agree on every row B decides, B abstains on at most 5 % of the sampled rows, hand-derived ids hold;
- the oracle's log-probabilities lie inside the bound derived from the kernels' summation order at every GPU case;
- the test hook refuses what it must without touching a device (device = -1)."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import token_pick_cases as TC
import token_pick_ref as R


@functools.lru_cache(maxsize=None)
def answers(mut):
    """everything a launch leaves behind, per case, under one mutation switch (or none)"""
    m = (mut,) if mut else ()
    out = {}
    for c in TC.llm_cases():
        o = R.ref_argmax_launch(c, m)
        out[c["name"]] = [None if o[k] is None else o[k].tolist() for k in ("tok", "pos", "nsteps", "hist", "counter")]
    for c in TC.asr_cases():
        o = R.ref_asr_launch(c, m)
        out[c["name"]] = [o["tok"].tolist(), None if o["state"] is None else o["state"].tolist()]
    return out


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_mutant_is_noticed_by_a_gpu_case(mut):
    base, got = answers(""), answers(mut)
    noticed = [n for n in base if base[n] != got[n]]
    print(mut, "noticed by", noticed[:6])
    assert noticed, "no case of the GPU list notices the mutation %r: a case is missing" % mut


def test_reference_b_and_the_oracle_agree_and_abstentions_stay_under_five_percent():
    sampled = abstained = 0
    for c in TC.llm_cases():
        a, b = R.oracle_argmax_launch(c), R.ref_argmax_launch(c)
        ta, tb = (o["tok"] if o["tok"] is not None else o["tok_unseen"] for o in (a, b))
        decided = ~b["abstain"]
        assert np.array_equal(ta[decided], tb[decided]), (c["name"], ta, tb, b["abstain"])
        for r, want in c["expect"].items():
            assert ta[r] == want, (c["name"], r, int(ta[r]), want)
        sampled += int(b["sampled"].sum())
        abstained += int(b["abstain"].sum())
    for c in TC.asr_cases():
        a, b = R.oracle_asr_launch(c), R.ref_asr_launch(c)
        decided = ~b["abstain"]
        assert np.array_equal(a["tok"][decided], b["tok"][decided]), (c["name"], a["tok"], b["tok"], b["abstain"])
        if c["kind"] == TC.PICK_ROWS_FILTERED:
            assert np.array_equal(a["state"][decided], b["state"][decided]), (c["name"], a["state"], b["state"])
            if "expect_state" in c:
                assert np.array_equal(a["state"], c["expect_state"]), c["name"]
        for r, want in c["expect"].items():
            assert a["tok"][r] == want, (c["name"], r, int(a["tok"][r]), want)
        sampled += int(b["sampled"].sum())
        abstained += int(b["abstain"].sum())
    print("reference B abstains on %d of %d sampled rows (%.2f %%)" % (abstained, sampled, 100.0 * abstained / sampled))
    assert sampled >= 200 and abstained <= 0.05 * sampled


def test_the_filters_timestamp_rule_is_never_close():
    """the filtered pick's allowed set never abstains: lp_ts - m_tx is either exactly zero (the hand-made tie of the walk, row (k)) or far from it"""
    for c in TC.asr_cases():
        if c["kind"] != TC.PICK_ROWS_FILTERED:
            continue
        for r in range(c["rows"]):
            f = R.ref_filtered_row(c["logits"][r, :c["cols"]], c["suppress"], c["state"][r], c["beg"], c["eot"], c["tid0"], c["temperature"], c["seed"], c["counter0"] + r)
            if f["live"] and f["ts_margin"] is not None:
                assert f["ts_margin"] == 0.0 or abs(f["ts_margin"]) > 1e-3, (c["name"], r, f["ts_margin"])
                assert f["ts_margin"] != 0.0 or (c["name"].startswith("filtered_walk") and r == 10)


def test_tk_logf_and_tk_expf_error_is_inside_the_constants_of_the_bound():
    S = np.unique(np.concatenate([np.geomspace(1.0, 65536.0, 20000), np.arange(1.0, 4097.0), 1.0 + 2.0 ** -np.arange(1, 24)]).astype(np.float32))
    L = O.lib()
    err = max(abs(float(L.orc_logf(float(s))) - float(np.log(np.float64(s)))) for s in S)
    print("tk_logf: worst |error| over S in [1, 65536] = %.3g (constant %.3g)" % (err, R.LOGF_ABS_ERR))
    assert err <= R.LOGF_ABS_ERR
    X = np.concatenate([-np.geomspace(1e-6, 87.0, 20000), [0.0]]).astype(np.float32)
    rel = max(abs(float(L.orc_expf(float(x))) / float(np.exp(np.float64(x))) - 1.0) for x in X)
    print("tk_expf: worst relative error on [-87, 0] = %.3g (constant %.3g)" % (rel, R.EXPF_REL_ERR))
    assert rel <= R.EXPF_REL_ERR


def test_the_oracles_logprobs_are_inside_the_bound_at_every_gpu_case():
    worst = {}
    for c in TC.asr_cases():
        if not (c["want_lp"] and c["compare_lp"]):
            continue
        a, b = R.oracle_asr_launch(c), R.ref_asr_launch(c)
        for r in range(c["rows"]):
            if not b["live"][r]:
                assert a["logprob"][r] == 0.0
                continue
            want, bound = R.logprob_reference(c, r, int(a["tok"][r]), b["a0"][r])
            err = abs(float(a["logprob"][r]) - want)
            assert err <= bound, (c["name"], r, float(a["logprob"][r]), want, err, bound)
            fam = ("k_pick_rows" if c["kind"] == TC.PICK_ROWS else "k_pick_rows_filtered") + (" hot" if c["temperature"] > 0 else "")
            if fam not in worst or err / bound > worst[fam][0] / worst[fam][1]:
                worst[fam] = (err, bound, c["name"])
    for fam, (err, bound, name) in sorted(worst.items()):
        print("%s: worst error / bound = %.3g / %.3g = %.2f (%s)" % (fam, err, bound, err / bound, name))
    assert len(worst) == 4


def test_the_hook_refuses_without_touching_a_device(tk):
    refused, accepted = TC.refusals(tk.lib().tk_mi355x_llm_max_rows())
    for name, kw in refused:
        with pytest.raises(tk.TkError) as e:
            tk.token_pick_probe(device=-1, **kw)
        assert e.value.code == 1001, name
    for name, kw in accepted:
        out = tk.token_pick_probe(device=-1, **kw)
        assert all(np.array_equal(out[k], np.asarray(kw[k], out[k].dtype).reshape(out[k].shape)) for k in out if out[k] is not None), name
