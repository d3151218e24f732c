"""Whisper's language detection without a device: the host loop of tk_mi355x_lang_pick_probe (device = -1: the per-row function of
csrc/common/tk_lang_pick.h, the one k_lang_pick runs) against tests/lang_pick_ref.py, a float64 restatement written from that header's comment;
every refusal of the probe; the language table's two lookups."""
import ctypes as C

import numpy as np
import pytest

import lang_pick_cases as LC
import lang_pick_ref as R

INVALID = 1001   # TK_ERROR_INVALID_ARGUMENT


def run(tk, c, device=-1):
    return tk.lang_pick_probe(c["logits"], c["rows"], c["cols"], c["tok0"], c["n_lang"], c["auto_row"], c["slot"], ld=c["ld"], device=device)


def ref(c, mutation=None):
    return R.pick(c["logits"], c["rows"], c["cols"], c["ld"], c["tok0"], c["n_lang"], c["auto_row"], c["slot"], mutation)


def differs(c, got, want):
    """does the library's answer `got` fall outside what the restatement `want` allows?  Decisions exactly, probabilities of bounded rows by the bound"""
    ids, probs, slot = got
    wids, wprobs, wslot = want
    if not np.array_equal(ids, wids) or not np.array_equal(slot, wslot):
        return True
    tol = R.bound(c["logits"], c["rows"], c["ld"], c["tok0"], c["n_lang"], wids, wprobs)
    b = c["bounded"]
    return bool((np.abs(probs.astype(np.float64) - wprobs)[b] > tol[b]).any())


@pytest.mark.parametrize("n_lang", LC.N_LANGS)
def test_the_host_loop_decides_like_the_restatement_and_its_probabilities_are_inside_the_bound(tk, n_lang):
    worst = 0.0
    for rows in LC.ROWS:
        for c in LC.cases(n_lang, rows):
            ids, probs, slot = run(tk, c)
            wids, wprobs, wslot = ref(c)
            assert np.array_equal(ids, wids), (c["name"], ids, wids)
            assert np.array_equal(slot, wslot), (c["name"], slot, wslot)
            untouched = c["auto_row"] == 0
            assert np.array_equal(slot[untouched], c["slot"][untouched]) and np.array_equal(slot[~untouched], c["tok0"] + ids[~untouched])
            tol = R.bound(c["logits"], c["rows"], c["ld"], c["tok0"], n_lang, wids, wprobs)
            err = np.abs(probs.astype(np.float64) - wprobs)
            b = c["bounded"]
            if b.any():
                worst = max(worst, float((err[b] / tol[b]).max()))
            assert (err[b] <= tol[b]).all(), (c["name"], float((err[b] / tol[b]).max()))
            x = c["logits"]
            for r, kind in enumerate(c["kinds"]):
                l = x[r * c["ld"] + c["tok0"]: r * c["ld"] + c["tok0"] + n_lang]
                dead = ~(l > -np.inf)                                                  # -inf and NaN entries: a probability of exactly 0
                assert not probs[r][dead].any() and not np.isnan(probs[r]).any(), (c["name"], r, kind)
                if dead.all():
                    assert ids[r] == 0 and not probs[r].any(), (c["name"], r, kind)     # nothing above -inf: id 0, all zeros
                else:
                    assert not dead[ids[r]] and l[ids[r]] == l[~dead].max() and ids[r] == np.flatnonzero(l == l[ids[r]])[0], (c["name"], r, kind)
                    assert abs(float(probs[r].astype(np.float64).sum()) - 1.0) < 1e-5
    print("n_lang %d: worst error / bound = %.3f" % (n_lang, worst))


def test_every_kind_of_row_and_both_sides_of_a_lane_pair_are_among_the_cases(tk):
    seen, max_at = set(), set()
    for c in LC.all_cases():
        seen.update(c["kinds"])
        ids, _, _ = ref(c)
        max_at.update((c["n_lang"], int(i)) for i in ids)
        assert c["ld"] >= c["cols"] and c["logits"].size == (c["rows"] - 1) * c["ld"] + c["cols"]
    assert seen == set(LC.KINDS)
    assert {(128, 0), (128, 63), (128, 64), (128, 127), (99, 98), (65, 64), (64, 63), (1, 0)} <= max_at
    assert any(c["ld"] > c["cols"] for c in LC.all_cases()) and any(c["ld"] == c["cols"] for c in LC.all_cases())
    assert any((c["auto_row"] == 0).any() and (c["auto_row"] != 0).any() for c in LC.all_cases())


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_of_the_restatement_is_told_from_the_host_loop_by_some_case(tk, mutation):
    caught = [c["name"] for c in LC.all_cases() if differs(c, run(tk, c), ref(c, mutation))]
    assert caught, mutation
    assert not [c["name"] for c in LC.all_cases() if differs(c, run(tk, c), ref(c))]      # the unmutated restatement: no case differs


def raw_probe(tk, rows, cols, ld, logits, n_logits, tok0, n_lang, auto_row, slot, ids, probs, device=-1):
    f = tk.lib().tk_mi355x_lang_pick_probe
    f.argtypes = [C.c_int, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    p = lambda a: None if a is None else a.ctypes.data
    return f(device, rows, cols, ld, p(logits), n_logits, tok0, n_lang, p(auto_row), p(slot), p(ids), p(probs))


def test_the_probe_refuses_what_it_must_before_it_writes_anything(tk):
    rows, cols, ld, tok0, n_lang = 3, 110, 112, 4, 99
    rng = np.random.default_rng(5)
    x = rng.standard_normal((rows - 1) * ld + cols).astype(np.float32)
    x[0] = x[tok0 + n_lang] = x[ld - 1] = np.inf                                          # +inf OUTSIDE the slices is nobody's business
    auto = np.ones(rows, np.int32)
    good = dict(rows=rows, cols=cols, ld=ld, logits=x, n_logits=x.size, tok0=tok0, n_lang=n_lang)

    def call(**kw):
        a = dict(good, **kw)
        slot, ids, probs = np.full(max(rows, 1), -7, np.int32), np.full(max(rows, 1), -7, np.int32), np.full((max(rows, 1), 128), -7.0, np.float32)
        arrs = dict(auto_row=auto, slot=slot, ids=ids, probs=probs)
        arrs.update({k: a.pop(k) for k in list(a) if k in arrs})
        rc = raw_probe(tk, a["rows"], a["cols"], a["ld"], a["logits"], a["n_logits"], a["tok0"], a["n_lang"], arrs["auto_row"], arrs["slot"], arrs["ids"], arrs["probs"])
        return rc, slot, ids, probs

    rc, slot, ids, probs = call()
    assert rc == 0 and (slot == tok0 + ids).all() and (ids >= 0).all()
    with_inf = x.copy()
    with_inf[ld + tok0 + n_lang - 1] = np.inf                                              # the last language of row 1
    big = np.zeros(4097 * 8, np.float32)
    refusals = dict(rows_0=dict(rows=0), rows_neg=dict(rows=-1), rows_4097=dict(rows=4097, cols=8, ld=8, tok0=0, n_lang=8, logits=big, n_logits=big.size),
                    n_lang_0=dict(n_lang=0), n_lang_129=dict(n_lang=129, cols=200, ld=200), tok0_neg=dict(tok0=-1), slice_past_cols=dict(tok0=cols - n_lang + 1),
                    ld_below_cols=dict(ld=cols - 1), short_logits=dict(n_logits=x.size - 1), inf_in_slice=dict(logits=with_inf),
                    null_logits=dict(logits=None), null_auto_row=dict(auto_row=None), null_slot=dict(slot=None), null_ids=dict(ids=None), null_probs=dict(probs=None))
    for name, kw in refusals.items():
        rc, slot, ids, probs = call(**kw)
        assert rc == INVALID, name
        assert (slot == -7).all() and (ids == -7).all() and (probs == -7.0).all(), name    # nothing written
    rc, _, _, _ = call(rows=4096, cols=8, ld=8, tok0=0, n_lang=8, logits=big, n_logits=4096 * 8,
                       auto_row=np.zeros(4096, np.int32), slot=np.zeros(4096, np.int32), ids=np.zeros(4096, np.int32), probs=np.zeros((4096, 8), np.float32))
    assert rc == 0                                                                         # the limits themselves are inside
    with pytest.raises(tk.TkError) as e:
        tk.lang_pick_probe(x, rows, cols, tok0, 129, auto, np.zeros(rows, np.int32), ld=ld, device=-1)
    assert e.value.code == INVALID


def test_the_language_table_round_trips_and_knows_its_ends(tk):
    codes = [tk.whisper_lang_code(i) for i in range(100)]
    assert all(codes) and len(set(codes)) == 100
    assert [tk.whisper_lang_id(c) for c in codes] == list(range(100))
    assert (codes[0], codes[1], codes[2], codes[8], codes[98], codes[99]) == ("en", "zh", "de", "pt", "su", "yue")   # the published tokenizer order
    assert tk.whisper_lang_code(-1) is None and tk.whisper_lang_code(100) is None
    assert tk.whisper_lang_id("xx") == -1 and tk.whisper_lang_id("auto") == -1 and tk.whisper_lang_id("") == -1 and tk.whisper_lang_id(None) == -1
