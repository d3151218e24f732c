"""The kernels at the two ends of the perception streams alone, ONE launch at a time (tk_mi355x_edge_probe): k_frames, k_power, k_logmel_finish, k_vad_head,
k_preprocess, k_preprocess_scaled, k_depth_minmax, k_depth_metric, k_postprocess_depth, k_depth_to_points, k_box_attributes — at the clip lengths
around the reflect padding, row counts around the 1024-thread reductions, maps past the capped grid, and colours and edge densities ON the
classifiers' thresholds (tests/edge_cases.py).

Reference A, bit for bit: the oracle's own host functions on the same arrays (the min / max pair as values: a map that holds +0.0 and -0.0 has two
equal minima).  Reference B (tests/edge_ref.py, NumPy from the kernels' comments): exact where the operation is exact, float64 inside bounds built
term by term elsewhere.  Both compare the WHOLE in/out arrays: the sentinel past the written region must come back.  The compiled reference's
recorded answers (tests/golden/edge_reference_answers.npz) are compared for the box cases and the packed RGB8 pre-processor cases.  Hand-written expectations are
checked at every case, and each family must check at least edge_cases.MIN_HAND elements that way.  The launcher's answer (which pre-processor
kernel, how many blocks of the depth grids) is asserted at every launch.  tests/test_perception_edges_cpu.py shows that each modelled kernel error
is noticed by at least one of these launches.  One more test runs the log-mel front end as the engine composes it, through Asr.transcribe_tokens, on
crafted utterances against an independent float64 STFT and Slaney bank.

Worst error / bound on the MI355X (every kernel also matched the oracle bit for bit): k_postprocess_depth 0.97, k_depth_to_points 0.82, k_depth_metric
0.70, k_vad_head 0.53, k_logmel_finish 0.32, k_preprocess / k_preprocess_scaled 0.11, the exact ops 0."""
import numpy as np
import pytest

import edge_cases as EC
import edge_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("group", EC.GROUPS)
def test_edges(gpu, group):
    worst, hand, recorded, kernels = (0.0, ""), 0, 0, set()
    cases = EC.group(group)
    for index, c in enumerate(cases):
        got, kernel = EC.probe(gpu, c, 0)
        assert kernel == c["kernel"], (c["name"], kernel, c["kernel"])
        kernels.add(kernel)
        a, b = EC.reference_a(c), R.expected(c)
        for name, want in a.items():
            assert EC.same_bits(got[name], want, zero_sign_free=group == "depth_minmax" or name == "y2"), "%s: %s differs from the oracle" % (c["name"], name)
        try:
            ratio = max(R.compare(got[name], want, bound) for name, (want, bound) in b.items())
        except AssertionError as e:
            raise AssertionError("%s: %s" % (c["name"], e))
        hand += EC.check_hand(c, got, {k: (np.zeros(len(v[0])) if v[1] is None else v[1]) for k, v in b.items()})
        recorded += EC.check_recorded(group, index, c, got)
        if ratio >= worst[0]:
            worst = (ratio, c["name"])
    print("%s: %d launches, launcher answers %s, %d hand-checked elements, worst error / bound = %.2f (%s)" % (group, len(cases), sorted(kernels)[:4], hand, worst[0], worst[1]))
    assert hand >= EC.MIN_HAND[group], (group, hand)
    assert recorded >= {"box_attributes": 200000, "preprocess": 4000}.get(group, 0), (group, recorded)   # the compiled reference's recorded answers
    assert worst[0] <= 1.0


def test_scale_zero_is_scale_one_over_255(gpu):
    """scale = 0 ("unset") selects the canonical kernel and gives the bits of scale = 1/255"""
    zero = {c["name"].rsplit(" scale ", 1)[0]: c for c in EC.group("preprocess") if c["name"].endswith(" scale 0")}
    unit = {c["name"].rsplit(" scale ", 1)[0]: c for c in EC.group("preprocess") if c["name"].endswith(" scale 1/255")}
    assert len(zero) >= 10 and set(zero) == set(unit)
    for name in zero:
        (y0, k0), (y1, k1) = EC.probe(gpu, zero[name], 0), EC.probe(gpu, unit[name], 0)
        assert k0 == k1 == gpu.PREPROCESS_CANONICAL and EC.same_bits(y0["y"], y1["y"]), name


def test_the_composed_log_mel(gpu):
    """the front end as the engine composes it (Asr.transcribe_tokens): bit-equal to the oracle's, and inside the float64 restatement's bound"""
    ohp = O.whisper_tiny_test()
    asr = gpu.Asr(hp=gpu.WhisperHP(*[getattr(ohp, n) for n, _ in ohp._fields_]), seed=6, max_batch=7)
    orc = O.OracleWhisper(ohp, seed=6)
    for call, names, pcm in EC.composed_utterances():
        _, mel, _, _ = asr.transcribe_tokens(pcm, 1)
        assert np.array_equal(mel, orc.transcribe(pcm, 1)[1]), call
        want, bound = R.logmel_composed(pcm, 160 * 2 * ohp.n_audio_ctx, 2 * ohp.n_audio_ctx, ohp.n_mels)
        ratio, share = EC.check_composed(names, mel, want, bound)
        print("composed log-mel, %s: worst error / bound = %.3f" % (call, ratio))
        for name, s in zip(names, share):
            assert "noise" not in name or s >= 0.9, (name, s)


def test_the_hook_refuses_on_the_device_too(gpu):
    for device in (0, -1):
        for name, op, kw in EC.refusals():
            with pytest.raises(gpu.TkError) as e:
                gpu.edge_probe(getattr(gpu, "EDGE_" + op), device=device, **kw)
            assert e.value.code == 1001, (name, device)
