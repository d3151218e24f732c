"""CPU: the launches of tests/test_nn_rows_gpu.py discriminate, and the oracle (reference A) stands inside everything the GPU file asks of the kernels.

- the oracle lies inside reference B's bound (tests/nn_row_ref.py) at every launch, and equals it where B is exact;
- every mutation switch of reference B (one plausible kernel error each) leaves the oracle's answer outside the bound at one launch at least;
- the two modelled errors float64 cannot see — the softmax sum taken in reversed order, a padding tap of the stem skipped instead of entering the
  chain as a = 0 — are switches of the oracle (tests/nn_row_cases.py: ORACLE_MUTATIONS): each changes reference A's BITS at one launch at least;
- the validate-only answers of the hook (device = -1): the launcher's kernel code at every launch — all three softmax kernels and both im2col kernels
  are reached — and its refusals."""
import numpy as np
import pytest

import nn_row_cases as NC
import nn_row_ref as R

OP_OF = {"softmax": "softmax_rows", "layernorm": "layernorm", "conv": "conv_stem", "im2col": "im2col", "maxpool": "maxpool5", "add": "add_rows", "embed": "embed_rows",
         "attend1": "attend1"}


def test_the_oracle_is_inside_reference_b_at_every_launch():
    worst = {}
    for l in NC.every_launch():
        if l["oracle_only"]:
            continue
        ya, ia = NC.reference_a(l)
        y, bound, img, img_bound = R.expected(l)
        if ya is None:                                                      # a pure gather the oracle has no step for: B is exact and stands alone
            assert bound is None
            continue
        ratio = R.compare(ya, y, bound)
        if img is not None:
            ratio = max(ratio, R.compare(ia, img, img_bound))
        key = l["op"] + (" (small scores)" if l["plain"] else "")
        if bound is not None and ratio > worst.get(key, (0.0, ""))[0]:
            worst[key] = (ratio, l["name"])
    for op, (ratio, name) in sorted(worst.items()):
        print("%s: the oracle's worst error / bound = %.2f (%s)" % (op, ratio, name))
    assert set(worst) == {"attend1", "attend1 (small scores)", "conv_stem", "layernorm", "softmax_rows"}


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_mutant_is_noticed_by_a_gpu_launch(mut):
    noticed = []
    for l in NC.every_launch((OP_OF[mut.split("_")[0]],)):
        if l["oracle_only"]:
            continue
        ya, ia = NC.reference_a(l)
        y, bound, img, img_bound = R.expected(l, (mut,))
        if ya is None:                                                      # gathers: the unmutated reference B is the answer
            ya = R.expected(l)[0]
        try:
            R.compare(ya, y, bound)
            if img is not None:
                R.compare(ia, img, img_bound)
        except AssertionError:
            noticed.append(l["name"])
    print(mut, "noticed by", len(noticed), "launches, first:", noticed[:3])
    assert noticed, "no launch of the GPU list notices the mutation %r: a case is missing" % mut


@pytest.mark.parametrize("mut", NC.ORACLE_MUTATIONS)
def test_every_mutant_of_the_oracle_changes_its_bits_at_a_gpu_launch(mut):
    """the GPU file asks for reference A's bits (NaN positions included), so a kernel with one of these errors fails where the mutant differs"""
    noticed = []
    for l in NC.every_launch((OP_OF[mut.split("_")[0]],)):
        good, bad = NC.reference_a(l)[0], NC.reference_a(l, mut)[0]
        nan = np.isnan(good)
        if not (np.array_equal(np.isnan(bad), nan) and np.array_equal(good[~nan].view(np.uint32), bad[~nan].view(np.uint32))):
            noticed.append(l["name"])
    print(mut, "noticed by", len(noticed), "launches, first:", noticed[:3])
    assert noticed, "no launch of the GPU list notices the oracle's mutant %r: a case is missing" % mut


def test_the_launchers_kernel_codes_without_a_device(tk):
    seen = {}
    for l in NC.every_launch():
        y, img, kernel = NC.probe(tk, l, -1)
        assert kernel == l["kernel"], (l["name"], kernel, l["kernel"])
        assert np.array_equal(y, l["y"], equal_nan=True)                   # validate only: nothing written
        seen.setdefault(l["op"], set()).add(kernel)
    assert seen["softmax_rows"] == {0, 1, 2} and seen["im2col"] == {0, 1}
    assert any(l["a_offset"] for l in NC.group("im2col")) and any(l["a_offset"] for l in NC.group("attend1"))


def test_the_hook_refuses_without_touching_a_device(tk):
    for name, op, kw in NC.refusals():
        with pytest.raises(tk.TkError) as e:
            tk.nn_row_probe(getattr(tk, "ROW_" + op.upper()), device=-1, **kw)
        assert e.value.code == 1001, name
    for name, op, kw in NC.accepted():
        assert tk.nn_row_probe(getattr(tk, "ROW_" + op.upper()), device=-1, **kw)[2] == 0, name
