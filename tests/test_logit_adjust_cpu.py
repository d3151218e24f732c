"""CPU: the logit adjustment's one definition (csrc/common/tk_logit_adjust.h) through tk_mi355x_logit_adjust_probe with device = -1 — the
per-row function in a host loop — against the float32 NumPy restatement tests/logit_adjust_ref.py, bit for bit; every refusal leaves the
logits untouched; and each modelled error of logit_adjust_ref.MUTATIONS changes the expected output of at least one case."""
import numpy as np
import pytest

import logit_adjust_cases as LC
import logit_adjust_ref as R

VOCABS = (1, 33, 1000, 32000)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("cols", VOCABS)
def test_host_loop_equals_the_numpy_reference_bit_for_bit(tk, cols):
    c = LC.make_case(cols, 2 * len(LC.KINDS), seed=1)  # every kind twice, neutral rows between adjusted ones
    got = tk.logit_adjust_probe(c["logits"], c["rows"], cols, c["specs"], device=-1)
    want = R.adjust(c["logits"], c["specs"])
    assert not np.isnan(want).any()
    assert np.array_equal(bits(got), bits(want))
    neutral = [r for r in range(c["rows"]) if R.is_neutral(c["specs"][r])]
    changed = [r for r in range(c["rows"]) if not np.array_equal(bits(want[r]), bits(c["logits"][r]))]
    assert len(neutral) >= 8 and not set(neutral) & set(changed)
    assert np.array_equal(bits(got[neutral]), bits(c["logits"][neutral]))  # byte for byte
    assert len(changed) >= (c["rows"] - len(neutral)) // 2                 # the adjusted kinds do something at this vocabulary


def test_hand_derived_row(tk):
    """signed zeros, -inf, counts and a bias under a penalty, by hand"""
    lg = np.array([2.0, -2.0, 0.0, -0.0, -np.inf, 1.0, 3.0, 5.0], np.float32)
    spec = dict(repeat=2.0, freq=0.5, present=0.25, recent=[0, 1, 1, 2, 3, 4, 6, 6, 6], bias_ids=[6, 7, 5], bias=[1.0, -np.inf, 0.5])
    got = tk.logit_adjust_probe(lg, 1, 8, [spec], device=-1)[0]
    # 0: 2 / 2 - 0.75; 1: -2 * 2 - 1.25; 2: +0 * 2 - 0.75; 3: -0 * 2 - 0.75; 4: -inf; 5: bias only; 6: (3 + 1) / 2 - 1.75; 7: banned
    want = np.array([0.25, -5.25, -0.75, -0.75, -np.inf, 1.5, 0.25, -np.inf], np.float32)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(R.adjust_row(lg, spec)), bits(want))
    # the sign of a zero that is only multiplied survives: repeat alone
    z = tk.logit_adjust_probe(np.array([0.0, -0.0], np.float32), 1, 2, [dict(repeat=1.5, recent=[0, 1])], device=-1)[0]
    assert bits(z).tolist() == [0x00000000, 0x80000000]


REFUSALS = {
    "n_recent 257": dict(repeat=1.1, recent=np.zeros(257, np.int32)),
    "n_bias 257": dict(bias_ids=np.arange(257) % 33, bias=np.zeros(257, np.float32)),
    "repeat 0": dict(repeat=0.0, recent=[1]),
    "repeat negative": dict(repeat=-1.1, recent=[1]),
    "repeat nan": dict(repeat=float("nan"), recent=[1]),
    "repeat inf": dict(repeat=float("inf"), recent=[1]),
    "freq nan": dict(freq=float("nan"), recent=[1]),
    "present inf": dict(present=float("inf"), recent=[1]),
    "bias nan": dict(bias_ids=[3], bias=[float("nan")]),
    "bias +inf": dict(bias_ids=[3], bias=[float("inf")]),
    "window id -1": dict(repeat=1.1, recent=[4, -1]),
    "window id vocab": dict(repeat=1.1, recent=[4, 33]),
    "bias id -1": dict(bias_ids=[-1], bias=[1.0]),
    "bias id vocab": dict(bias_ids=[33], bias=[1.0]),
    "duplicate bias ids": dict(bias_ids=[5, 7, 5], bias=[1.0, 1.0, 1.0]),
    "null window": dict(repeat=1.1, n_recent=3),
    "null bias ids": dict(n_bias=2, bias=[1.0, 1.0]),
    "null bias": dict(n_bias=2, bias_ids=[1, 2]),
    "negative n_recent": dict(n_recent=-1),
    "negative n_bias": dict(n_bias=-1),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_leave_the_logits_untouched(tk, name):
    rng = np.random.default_rng(7)
    lg = rng.standard_normal((3, 33)).astype(np.float32)
    good = dict(repeat=1.3, freq=0.5, present=0.25, recent=[1, 2, 2], bias_ids=[0, 2], bias=[1.0, -np.inf])
    for bad_row in (0, 2):  # rows before the bad one must not have been adjusted either
        specs = [good, good, good]
        specs[bad_row] = REFUSALS[name]
        out = lg.copy()
        with pytest.raises(tk.TkError) as e:
            tk.logit_adjust_probe_into(out, 3, 33, specs, device=-1)
        assert e.value.code == 1001
        assert np.array_equal(bits(out), bits(lg))


def test_shape_refusals(tk):
    lg = np.ones((2, 33), np.float32)
    ok = [None, dict(bias_ids=[1], bias=[1.0])]
    for kw in (dict(rows=0, cols=33), dict(rows=257, cols=33), dict(rows=2, cols=0), dict(rows=2, cols=33, n_logits=65)):
        out = lg.copy()
        with pytest.raises(tk.TkError) as e:
            tk.logit_adjust_probe_into(out, kw["rows"], kw["cols"], ok if kw["rows"] == 2 else ok * 129, device=-1, n_logits=kw.get("n_logits"))
        assert e.value.code == 1001 and np.array_equal(out, lg)
    import ctypes as C
    f = tk.lib().tk_mi355x_logit_adjust_probe
    f.argtypes = [C.c_int, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    tab, keep = tk.logit_adjust_rows(ok)
    assert f(-1, 2, 33, None, 66, C.cast(tab, C.c_void_p)) == 1001
    assert f(-1, 2, 33, lg.ctypes.data, 66, None) == 1001
    assert f(-1, 2, 33, lg.ctypes.data, 66, C.cast(tab, C.c_void_p)) == 0 and lg[1, 1] == 2.0


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_modelled_error_changes_a_case(mut):
    noticed = []
    for cols in VOCABS:
        c = LC.make_case(cols, 2 * len(LC.KINDS), seed=1)
        base, got = R.adjust(c["logits"], c["specs"]), R.adjust(c["logits"], c["specs"], (mut,))
        noticed += ["%s row %d" % (c["name"], r) for r in range(c["rows"]) if not np.array_equal(bits(base[r]), bits(got[r]))]
    print(mut, "noticed by", noticed[:6])
    assert noticed, "no case notices the modelled error %r: a case is missing" % mut


def test_runner_setters_exist_and_forward_adjusted_is_exported(tk):
    for name in ("tk_mi355x_llm_runner_set_penalties", "tk_mi355x_llm_runner_set_logit_bias", "tk_mi355x_llm_runner_recent_tokens",
                 "tk_mi355x_llm_forward_adjusted", "tk_mi355x_logit_adjust_probe"):
        assert hasattr(tk.lib(), name)
    L = tk.lib()
    assert L.tk_mi355x_llm_runner_set_penalties(None, 64, 1, 0, 0) == 1001
    assert L.tk_mi355x_llm_runner_set_logit_bias(None, 0, None, None) == 1001
    assert L.tk_mi355x_llm_runner_recent_tokens(None, None, 0) == -1
    assert L.tk_mi355x_llm_forward_adjusted(None, 1, None, None, None, None, None, None, None) == 1001
