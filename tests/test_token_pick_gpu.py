"""Every token-selection kernel alone, ONE launch at a time (tk_mi355x_token_pick_probe) on crafted logit rows: k_argmax (greedy, greedy under per-row
masks, stochastic through sample_row), k_argmax_rows, k_pick_rows, k_pick_rows_filtered.

Reference A, bit for bit: the oracle (orc_sample_row, orc_pick_row, orc_whisper_filter_pick) — ids, decode state, log-probabilities as uint32.
Reference B, independent: tests/token_pick_ref.py (float64 NumPy written from the kernels' comments) — every id it decides (it abstains where one of
its own float64 comparisons is closer than 1e-4 relative; tests/test_token_pick_cpu.py caps that at 5 % of the sampled rows), and ids derived by hand.
Bookkeeping: tok, pos + 1, hist[nsteps], nsteps + 1, counter + 1 on sampled rows only, and every other byte of the in/out arrays as the caller left it.
Log-probabilities also against float64 inside the bound derived from the kernels' summation order.
tests/test_token_pick_cpu.py shows that each of the modelled kernel errors changes the answer of at least one of these cases.

NaN rows, and rows whose largest allowed logit is -inf under sampling or under a log-probability, are left out: their arithmetic is NaN on both
sides and is not a contract (one such row runs for its id alone).  No input here is meant to fault the device."""
import numpy as np
import pytest

import token_pick_cases as TC
import token_pick_ref as R

pytestmark = pytest.mark.gpu

LP_SENTINEL = np.float32(-123.0)
LLM = {c["name"]: c for c in TC.llm_cases()}
ASR = {c["name"]: c for c in TC.asr_cases()}


def launch_llm(gpu, c, **kw):
    samp = None if c["samp"] is None else gpu.sampling_rows(c["samp"])
    rows, vocab = c["logits"].shape
    return samp, gpu.token_pick_probe(gpu.PICK_ARGMAX, c["logits"], rows, vocab, masks=c["masks"], allow_row=c["allow_row"], samp=samp, tok=c["tok"],
                                      pos=c["pos"], nsteps=c["nsteps"], hist=c["hist"], hist_stride=c["hist_stride"], **kw)


@pytest.mark.parametrize("name", list(LLM))
def test_k_argmax(gpu, name):
    c = LLM[name]
    samp0, got = launch_llm(gpu, c)
    a, b = R.oracle_argmax_launch(c), R.ref_argmax_launch(c)
    for k in ("tok", "pos", "nsteps", "hist"):                              # whole arrays: the cells around hist[nsteps][row] keep their sentinel
        assert (got[k] is None) == (a[k] is None)
        if got[k] is not None:
            assert np.array_equal(got[k], a[k]), (k, got[k].tolist(), a[k].tolist())
    if samp0 is not None:
        want = samp0.copy()
        want["counter"] = a["counter"]                                      # + 1 on sampled rows only; every other byte as handed in
        assert got["samp"].tobytes() == want.tobytes(), (got["samp"], want)
    if got["tok"] is not None:
        decided = ~b["abstain"]
        assert np.array_equal(got["tok"][decided], b["tok"][decided]), (got["tok"].tolist(), b["tok"].tolist(), b["abstain"].tolist())
        for r, want in c["expect"].items():
            assert got["tok"][r] == want, (r, int(got["tok"][r]), want)


def launch_asr(gpu, c):
    rows = c["rows"]
    filt = {k: c[k] for k in ("suppress", "state", "beg", "eot", "tid0")} if c["kind"] == TC.PICK_ROWS_FILTERED else {}
    return gpu.token_pick_probe(c["kind"], c["logits"], rows, c["cols"], ld=c["ld"], tok=np.full(rows, -9, np.int32), temperature=c["temperature"], seed=c["seed"],
                                counter0=c["counter0"], logprob=np.full(rows, LP_SENTINEL) if c["want_lp"] else None, **filt)


@pytest.mark.parametrize("name", list(ASR))
def test_asr_picks(gpu, name):
    c = ASR[name]
    got = launch_asr(gpu, c)
    a, b = R.oracle_asr_launch(c), R.ref_asr_launch(c)
    assert np.array_equal(got["tok"], a["tok"]), (got["tok"].tolist(), a["tok"].tolist())
    decided = ~b["abstain"]
    assert np.array_equal(got["tok"][decided], b["tok"][decided]), (got["tok"].tolist(), b["tok"].tolist())
    for r, want in c["expect"].items():
        assert got["tok"][r] == want, (r, int(got["tok"][r]), want)
    if c["kind"] == TC.PICK_ROWS_FILTERED:
        assert np.array_equal(got["state"], a["state"]), (got["state"].tolist(), a["state"].tolist())   # rows that stand still included
        assert np.array_equal(got["state"][decided], b["state"][decided])
        if "expect_state" in c:
            assert np.array_equal(got["state"], c["expect_state"])
    if c["want_lp"] and c["compare_lp"]:
        live = b["live"]
        assert np.array_equal(got["logprob"][live].view(np.uint32), a["logprob"][live].view(np.uint32)), (got["logprob"].tolist(), a["logprob"].tolist())
        assert np.all(got["logprob"][~live] == LP_SENTINEL)                 # a finished row writes no log-probability (the oracle answers 0.0 there)


def test_logprobs_are_inside_the_float64_bound(gpu):
    worst = {}
    for c in TC.asr_cases():
        if not (c["want_lp"] and c["compare_lp"]):
            continue
        got, b = launch_asr(gpu, c), R.ref_asr_launch(c)
        for r in np.flatnonzero(b["live"]):
            want, bound = R.logprob_reference(c, r, int(got["tok"][r]), b["a0"][r])
            err = abs(float(got["logprob"][r]) - want)
            assert err <= bound, (c["name"], r, float(got["logprob"][r]), want, err, bound)
            fam = ("k_pick_rows" if c["kind"] == TC.PICK_ROWS else "k_pick_rows_filtered") + (" hot" if c["temperature"] > 0 else "")
            if fam not in worst or err / bound > worst[fam][0] / worst[fam][1]:
                worst[fam] = (err, bound, c["name"])
    for fam, (err, bound, name) in sorted(worst.items()):
        print("%s: worst error / bound = %.3g / %.3g = %.2f (%s)" % (fam, err, bound, err / bound, name))
    assert len(worst) == 4


def test_an_all_ones_mask_and_no_mask_pick_the_same(gpu):
    c = LLM["masks_sampled"]
    _, got = launch_llm(gpu, c)
    assert got["tok"][8] == got["tok"][9]                                   # rows 8 / 9: the same logits and state under an all-ones mask / under none
    c = LLM["ties"]
    _, got = launch_llm(gpu, c)
    assert np.array_equal(got["tok"][:7], got["tok"][7:])


def test_the_hook_refuses_on_the_device_too(gpu):
    refused, accepted = TC.refusals(gpu.lib().tk_mi355x_llm_max_rows())
    for device in (0, -1):                                                  # device = -1 answers the same without a device
        for name, kw in refused:
            with pytest.raises(gpu.TkError) as e:
                gpu.token_pick_probe(device=device, **kw)
            assert e.value.code == 1001, (name, device)
    for name, kw in accepted:
        gpu.token_pick_probe(device=-1, **kw)
    with pytest.raises(gpu.TkError) as e:
        gpu.token_pick_probe(device=99, **accepted[1][1])
    assert e.value.code == 1001
