"""GPU: every op of the node-by-node ONNX executor (csrc/nn/tk_onnx_exec*.hip) alone, one small graph per case, against the float64 NumPy
reference of tests/onnx_ops_ref.py — at the attribute branches, shapes and domain edges the whole-network tests never reach.  Shapes the
executor infers are compared too.  The criteria are derived ones (onnx_ops_ref.check): bit-identical for moves, selects and single
correctly rounded operations; gamma(n + 2) S for fma chains; the accuracies tests/test_oracle_llm.py pins for exp / log / tanh; 2e-5 of the
tensor's scale only where nothing tighter is pinned (erf, LayerNormalization, bilinear Resize, LSTM).  A case the executor must refuse
asserts the words of its error text.  Every test's assertion message carries the worst error / bound it saw per op."""
import numpy as np
import pytest

import onnx_ops_cases as OC
import onnx_ops_ref as R

pytestmark = pytest.mark.gpu


def run_group(gpu, tmp_path, group):
    from trackiellm_amd._lib import TkError
    worst, failures, n_refused = {}, [], 0
    for c in OC.cases_of(group):
        path = tmp_path / (c.name.replace("/", "_") + ".onnx")
        path.write_bytes(c.model())
        try:
            got = gpu.onnx_run(path, c.feeds, c.outputs)
        except TkError as e:
            if c.refuse and all(w in e.detail for w in c.refuse):
                n_refused += 1
            else:
                failures.append("%s: %s" % (c.id, ("refused, but its text lacks %r: %s" % (c.refuse, e.detail)) if c.refuse else "refused: " + e.detail))
            continue
        if c.refuse and not c.either:
            failures.append("%s: must be refused (%r), but ran" % (c.id, c.refuse))
            continue
        refs = R.run(c.spec, c.feeds, c.floats, c.ints, c.opset)  # a wrong-length attribute that was not refused fails here: it was ignored
        for o in c.outputs:
            ref, kind = refs[o], R.kind_of(c.producer(o))
            if got[o].shape != ref.shape:
                failures.append("%s: %s has shape %s, the reference %s" % (c.id, o, got[o].shape, ref.shape))
                continue
            ok, ratio = R.check(kind, got[o], ref)
            w = float(ratio.max()) if ratio.size else 0.0
            if w >= worst.get(kind, (-1.0, ""))[0]:
                worst[kind] = (w, c.id)
            if not ok.all():
                i = int(np.argmax(~ok.reshape(-1)))
                failures.append("%s: %s (%s): %d of %d elements outside the bound, worst error / bound %.3g; first at %d: got %r, reference %r"
                                % (c.id, o, kind, int((~ok).sum()), ok.size, w, i, got[o].reshape(-1)[i], ref.v.reshape(-1)[i]))
    report = "worst error / bound per op in '%s' (%d refused as required): " % (group, n_refused) + "; ".join(
        "%s %.3g (%s)" % (k, v[0], v[1]) for k, v in sorted(worst.items()))
    print(report)
    assert not failures, "\n".join(failures) + "\n" + report


@pytest.mark.parametrize("group", OC.GROUPS)
def test_op_group_against_the_float64_reference(gpu, tmp_path, group):
    run_group(gpu, tmp_path, group)


def test_hook_reports_the_executors_text_and_unknown_names(gpu, tmp_path):
    """the hook itself: an unsupported op comes back with its name, an output name the graph never produced is an error, and a rank-0 feed
    keeps rank 0 (the result of scalar + scalar has no dimensions)"""
    from trackiellm_amd._lib import TkError
    import onnx_util as OU
    p = tmp_path / "m.onnx"
    p.write_bytes(OU.model(OU.spec_nodes([OC.nd("Add", ["a", "b"], ["y"])]), [], [OU.value_info("a", 1, []), OU.value_info("b", 1, [])], [OU.value_info("y", 1, [])]))
    got = gpu.onnx_run(p, {"a": np.float32(1.5).reshape(()), "b": np.float32(2.25).reshape(())}, ["y"])
    assert got["y"].shape == () and got["y"] == np.float32(3.75)
    with pytest.raises(TkError, match="nothing"):
        gpu.onnx_run(p, {"a": np.zeros(2, np.float32), "b": np.zeros(2, np.float32)}, ["nothing"])
    with pytest.raises(TkError, match="do not broadcast"):
        gpu.onnx_run(p, {"a": np.zeros(2, np.float32), "b": np.zeros(3, np.float32)}, ["y"])
    p.write_bytes(OU.model(OU.spec_nodes([OC.nd("Celu", ["a"], ["y"])]), [], [OU.value_info("a", 1, [2])], [OU.value_info("y", 1, [2])]))
    with pytest.raises(TkError, match="Celu"):
        gpu.onnx_run(p, {"a": np.zeros(2, np.float32)}, ["y"])
