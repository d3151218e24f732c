"""CPU: the launches of tests/test_perception_edges_gpu.py discriminate, and the oracle (reference A) stands inside everything the GPU file asks of the
kernels at the two ends of the perception streams.

- reference A (the oracle's host functions) equals reference B (tests/edge_ref.py) where B is exact and lies inside B's bound elsewhere, at every case,
  sentinels included; both meet every hand-written expectation; no element abstains (asserted: the share is 0, the cap 1 %);
- tk_log10f against float64 log10 over every argument the cases send and a dense sweep of [1e-10, 1e6]: edge_ref.LOG10_ABS is twice the worst error;
- every case passes the hook's validation at device = -1 with the launcher's answer it names, and nothing is written; every refusal is refused;
- every mutation switch of reference B (one plausible kernel error each) changes what at least one case leaves behind by more than the bound."""
import numpy as np
import pytest

import edge_cases as EC
import edge_ref as R
import oracle_lib as O

OP_OF = {"frames": ("frames",), "power": ("power",), "logmel": ("logmel_finish",), "vad": ("vad_head",), "preprocess": ("preprocess",),
         "depth": ("depth_minmax", "depth_metric"), "points": ("depth_to_points",), "box": ("box_attributes",)}


def agree(c, a, b):
    """reference A against B's expectation of every in/out array; the worst error / bound"""
    worst = 0.0
    for name, (want, bound) in b.items():
        worst = max(worst, R.compare(a[name], want, bound))
    return worst


def bounds_of(b):
    return {k: (np.zeros(len(v[0])) if v[1] is None else v[1]) for k, v in b.items()}


def test_reference_a_is_inside_reference_b_at_every_case_and_both_meet_the_hand_values():
    worst, hand, elements = {}, {}, {}
    for c in EC.every_case():
        a, b = EC.reference_a(c), R.expected(c)
        try:
            ratio = agree(c, a, b)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (c["name"], e))
        EC.check_hand(c, {k: v[0] for k, v in b.items()}, bounds_of(b))
        hand[c["op"]] = hand.get(c["op"], 0) + EC.check_hand(c, a, bounds_of(b))
        elements[c["op"]] = elements.get(c["op"], 0) + sum(len(v[0]) for v in b.values())
        if ratio >= worst.get(c["op"], (0.0, ""))[0]:
            worst[c["op"]] = (ratio, c["name"])
    for op in EC.GROUPS:
        print("%s: %d cases, %d elements, 0 abstain (0.00 %%, cap 1 %%), %d hand-checked, the oracle's worst error / bound = %.2f (%s)" %
              (op, len(EC.group(op)), elements[op], hand[op], worst[op][0], worst[op][1]))
        assert hand[op] >= EC.MIN_HAND[op], (op, hand[op])
    assert set(worst) == set(EC.GROUPS)


def test_tk_log10f_is_within_half_the_bound_the_gpu_test_uses():
    args = [np.maximum(c["y"][:c["B"] * c["per_b"]], np.float32(1e-10)) for c in EC.group("logmel_finish")]
    args.append((10.0 ** np.linspace(-10, 6, 2_000_001)).astype(np.float32))
    args.append(np.nextafter(np.float32(1.0), np.float32(0)) * np.linspace(1, 1 - 1e-4, 100001).astype(np.float32))
    x = np.concatenate(args)
    x = x[x >= np.float32(1e-10)]
    err = np.abs(O.log10f(x).astype(np.float64) - np.log10(x.astype(np.float64)))
    i = int(np.argmax(err))
    print("tk_log10f: worst |error| against float64 over %d arguments = %.3e at %r; edge_ref.LOG10_ABS = %.3e" % (len(x), err[i], x[i], R.LOG10_ABS))
    assert err[i] * 2 <= R.LOG10_ABS * (1 + 1e-3) and err[i] * 2 >= R.LOG10_ABS * 0.98, "LOG10_ABS must be twice the measured worst error %.4e" % err[i]


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_mutant_is_noticed_by_a_gpu_case(mut):
    noticed = []
    for c in EC.every_case(OP_OF[mut.split("_")[0]]):
        a, b = EC.reference_a(c), R.expected(c, (mut,))
        try:
            agree(c, a, b)
        except AssertionError:
            noticed.append(c["name"])
    print(mut, "noticed by", len(noticed), "cases, first:", noticed[:3])
    assert noticed, "no case of the GPU list notices the mutation %r: a case is missing" % mut


def test_every_case_passes_the_hooks_validation_without_a_device(tk):
    kernels = {}
    for c in EC.every_case():
        got, kernel = EC.probe(tk, c, -1)
        assert kernel == c["kernel"], (c["name"], kernel, c["kernel"])
        assert EC.same_bits(got["y"], c["y"]) and (c["y2"] is None or EC.same_bits(got["y2"], c["y2"])), c["name"]   # validate only: nothing written
        kernels.setdefault(c["op"], set()).add(kernel)
    assert kernels["preprocess"] == {tk.PREPROCESS_CANONICAL, tk.PREPROCESS_SCALED}
    # the launcher's grid cap, read out of the launcher: one map takes a second and a partial third trip of the grid-stride loop
    for op in ("postprocess_depth", "depth_to_points"):
        assert max(kernels[op]) == EC.GRID_CAP
        big = max(c["width"] * c["height"] for c in EC.group(op))
        assert 2 * EC.GRID_CAP * 256 < big < 3 * EC.GRID_CAP * 256


def test_the_hook_refuses_without_touching_a_device(tk):
    for name, op, kw in EC.refusals():
        with pytest.raises(tk.TkError) as e:
            tk.edge_probe(getattr(tk, "EDGE_" + op), device=-1, **kw)
        assert e.value.code == 1001, name


def test_the_composed_log_mel_of_the_oracle_is_inside_the_float64_restatement():
    """frames -> DFT -> power -> mel -> finish on crafted utterances: the oracle's mel against an rfft, its own Hann window and a Slaney bank written from
    the formula.  Quiet bins make the bound loose: on the noise rows at least 90 % of the elements must have a bound below 1e-3 output units."""
    ohp = O.whisper_tiny_test()
    orc = O.OracleWhisper(ohp, seed=6)
    for call, names, pcm in EC.composed_utterances():
        _, mel, _, _ = orc.transcribe(pcm, 1)
        want, bound = R.logmel_composed(pcm, 160 * 2 * ohp.n_audio_ctx, 2 * ohp.n_audio_ctx, ohp.n_mels)
        ratio, share = EC.check_composed(names, mel, want, bound)
        print("%s: the oracle's worst error / bound = %.3f; share of elements with a bound below 1e-3: %s" % (call, ratio, ", ".join("%s %.3f" % p for p in zip(names, share))))
        for name, s in zip(names, share):
            assert "noise" not in name or s >= 0.9, (name, s)


def test_reference_a_gives_the_compiled_references_recorded_answers():
    """the oracle against what the reference's own compiled pre-processor and classifiers answered (tests/golden/edge_reference_answers.npz): every
    threshold colour, the density-threshold boxes, the tiny frames"""
    for op, least in (("box_attributes", 200000), ("preprocess", 4000)):
        n = sum(EC.check_recorded(op, i, c, EC.reference_a(c)) for i, c in enumerate(EC.group(op)))
        print("%s: %d recorded elements equal" % (op, n))
        assert n >= least, (op, n)
