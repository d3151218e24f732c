"""The perception streams' row and layout kernels alone, ONE launch at a time (tk_mi355x_nn_row_probe): k_conv_stem, k_im2col, k_im2col_v4, k_im2col1d,
k_maxpool5, k_upsample2x, k_copy_cols, k_layernorm (with and without the tiled GEMM's operand image), k_softmax_rows, k_softmax_rows_reg,
k_softmax_rows_wave, k_add_rows, k_embed_rows — at pitches wider than the extent, unaligned bases, odd sizes around 256 / 2048 and the softmax
launcher's 1024-row threshold, rows that are no multiple of 16.

Reference A, bit for bit (NaN positions included): the oracle's own steps (tests/nn_row_cases.py: reference_a); the stem against im2col + the GEMM
oracle, the chain it claims to evaluate.  Reference B (tests/nn_row_ref.py, NumPy from the kernels' comments): gathers and single adds exactly,
layernorm / softmax / the stem in float64 inside bounds derived term by term.  Both compare the WHOLE in/out arrays: pitch columns, rows past the
extent and image rows past `rows` hold a sentinel that must come back.  The launcher's kernel code is asserted at every launch.
tests/test_nn_rows_cpu.py shows that each modelled kernel error is noticed by at least one of these launches.

Worst error / bound on the MI355X (every kernel also matched the oracle bit for bit): the three softmax kernels 0.80, k_layernorm 0.48, k_conv_stem 0.13,
k_attend1 0.02 (its bound carries the score chain's error through the exponent at scores of +/-80)."""
import numpy as np
import pytest

import nn_row_cases as NC
import nn_row_ref as R

pytestmark = pytest.mark.gpu


def same_bits(got, want):
    """bit for bit, except that any NaN matches any NaN (payloads are not a contract, positions are)"""
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


@pytest.mark.parametrize("group", NC.GROUP_NAMES)
def test_rows(gpu, group):
    worst, plain, kernels = (0.0, ""), (0.0, ""), set()
    launches = NC.group(group)
    for l in launches:
        y, img, kernel = NC.probe(gpu, l, 0)
        assert kernel == l["kernel"], (l["name"], kernel, l["kernel"])
        kernels.add(kernel)
        ya, ia = NC.reference_a(l)
        if ya is not None:
            assert same_bits(y, ya), l["name"]
            assert ia is None or same_bits(img, ia), l["name"]
        if l["oracle_only"]:
            assert ya is not None
            continue
        want, bound, want_img, img_bound = R.expected(l)
        try:
            ratio = R.compare(y, want, bound)
            if want_img is not None:
                ratio = max(ratio, R.compare(img, want_img, img_bound))
        except AssertionError as e:
            raise AssertionError("%s: %s" % (l["name"], e))
        if ratio > worst[0]:
            worst = (ratio, l["name"])
        if l["plain"] and ratio > plain[0]:
            plain = (ratio, l["name"])
    print("%s: %d launches, kernels %s, worst error / bound = %.2f (%s)" % (group, len(launches), sorted(kernels), worst[0], worst[1]))
    if plain[1]:
        print("%s, small scores only: worst error / bound = %.3f (%s)" % (group, plain[0], plain[1]))


def test_all_three_softmax_kernels_and_both_im2col_kernels_are_taken():
    soft = {l["kernel"] for l in NC.every_launch(("softmax_rows",))}
    im = {l["kernel"] for l in NC.group("im2col")}
    assert soft == {NC.SOFTMAX_GENERIC, NC.SOFTMAX_REG, NC.SOFTMAX_WAVE} and im == {NC.IM2COL_ELEMENT, NC.IM2COL_V4}


def test_the_hook_refuses_on_the_device_too(gpu):
    for device in (0, -1):
        for name, op, kw in NC.refusals():
            with pytest.raises(gpu.TkError) as e:
                gpu.nn_row_probe(getattr(gpu, "ROW_" + op.upper()), device=device, **kw)
            assert e.value.code == 1001, (name, device)
