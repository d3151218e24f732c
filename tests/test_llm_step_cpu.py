"""CPU: the cases of tests/test_llm_step_gpu.py discriminate, and the oracle (reference A) stands inside everything the GPU file asks of the kernels.

- every mutation switch of tests/llm_step_ref.py (one plausible kernel error each) changes what some GPU case leaves behind;
- the image decoders (reshapes) and the image encoder (index arithmetic) of reference B invert each other;
- reference B (float64 NumPy) and the oracle agree on every value B decides; B abstains on at most 1 % of the int8 values of any case and on no
  crafted one; the hand-written expectations hold; the oracle's floats (ad, af, q, x after a fold) lie inside the bounds derived from the operation order;
- tk_divf, tk_sqrtf and tk_siluf are inside the constants those bounds use, measured against float64 on every run;
- the test hook refuses what it must without touching a device (device = -1), a norm row above the LDS opt-in among it."""
import ctypes as C

import numpy as np
import pytest

import llm_step_cases as SC
import llm_step_ref as R
import oracle_lib as O

FAMILY = {"image": ("tie_last", "tie_high_lane", "sign_lost", "round_half_away", "bsum_trunc", "abs_images_swapped", "slot_tile_mix", "slabs_descending",
                    "slab_into_x_first", "slab_pitch_nrows", "fold_writes_x_without_slabs", "norm_weight_chunk0", "mean_over_ngrp", "af_round_none"),
          "fold": ("slabs_descending", "slab_into_x_first", "slab_pitch_nrows"),
          "rope": ("slabs_descending", "slab_pitch_nrows", "rope_cos_sin_swapped", "rope_half_split", "rope_on_v", "cache_pos_major"),
          "tiles": ("tiles_len_off_by_one", "tiles_run_not_reset"), "embed": ("embed_block_of_next_row",)}


def leaves_behind(c, mut, tk=None):
    """everything a launch leaves behind under one mutation switch (or none), as reference B has it"""
    m = (mut,) if mut else ()
    if c["op"] in R.REF:
        r = R.ref_image_launch(c, m)
        out = [v.tobytes() for v in r["raw"].values() if v is not None]
        return out + ([r["x"].tobytes()] if "x" in r else [])
    if c["op"] == "fold":
        return [R.ref_residual_fold(c, m)["x"].tobytes()]
    if c["op"] == "rope":
        r = R.ref_rope_append(c, m)
        with np.errstate(over="ignore"):                                     # a mutant may leave the f16 range
            kc, vc = R.expected_caches(c, r, r["k"].astype(np.float16).view(np.uint16), r["v"].astype(np.float16).view(np.uint16))
        return [r["q"].astype(np.float32).tobytes(), kc.tobytes(), vc.tobytes()]
    if c["op"] == "tiles":
        return [R.ref_att_tiles(c, m)["tiles"].tobytes()]
    return [R.ref_embed(c, SC.decode_table(tk, c["type"], c["embd"], c["K"]), m)["x"].tobytes()]


def family_cases(fam, tk):
    return {"image": SC.image_cases, "fold": SC.fold_cases, "rope": SC.rope_cases, "tiles": SC.tiles_cases, "embed": lambda: SC.embed_cases(tk)[:6]}[fam]()


_BASE = {}


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_mutant_is_noticed_by_a_gpu_case(tk, mut):
    assert any(mut in v for v in FAMILY.values())
    noticed = []
    for fam, muts in FAMILY.items():
        if mut not in muts:
            continue
        for c in family_cases(fam, tk):
            if c["name"] not in _BASE:
                _BASE[c["name"]] = leaves_behind(c, "", tk)
            if leaves_behind(c, mut, tk) != _BASE[c["name"]]:
                noticed.append(c["name"])
                break                                                       # one case per family is enough to show it
    print(mut, "noticed by", noticed)
    assert noticed, "no case of the GPU list notices the mutation %r: a case is missing" % mut


def test_every_mutation_has_a_family():
    assert set(R.MUTATIONS) == {m for v in FAMILY.values() for m in v}


def test_the_image_decoders_invert_the_encoder():
    rng = np.random.default_rng(3)
    for K, nrows in ((256, 256), (768, 17), (2304, 33)):
        q = rng.integers(-127, 128, (nrows, K)).astype(np.int8)
        d = rng.standard_normal((nrows, K // 256)).astype(np.float32)
        sums = rng.integers(-4064, 4065, (nrows, K // 32))
        sums[0, :4] = (-4064, 4064, -1, -63)
        af = rng.standard_normal((nrows, K)).astype(np.float32)
        raw = R.encode_image(K, nrows, SC.FILL, q, d, sums, af)
        assert np.array_equal(R.decode_aq(raw["aq"], K)[:nrows], q) and np.all(R.decode_aq(raw["aq"], K)[nrows:] == SC.FILL)
        assert np.array_equal(R.decode_ad(raw["ad"], K)[:nrows], d)
        s, lo, hi = R.decode_abs(raw["abs"], K)
        assert np.array_equal(s[:nrows], sums) and lo[:nrows].min() >= 0 and lo[:nrows].max() <= 63 and np.all(lo[nrows:] == SC.FILL)
        s16, hh, ll = R.decode_abs16(raw["abs16"], K)
        assert np.array_equal(s16[:nrows], sums.astype(np.float64)) and set(np.unique(ll[:nrows]).tolist()) <= {0.0, 1.0}
        assert np.array_equal(R.decode_af(raw["af"], K)[:nrows], af)
        assert sum(int((v.view(np.uint8) != SC.FILL).sum()) for v in raw.values()) <= nrows * (K + K // 64 + K // 16 + K // 8 + 4 * K)   # nothing outside the rows' own bytes


def test_reference_b_and_the_oracle_agree_abstentions_stay_under_one_percent_and_the_floats_are_inside_their_bounds():
    worst, hand, fracs = {}, 0, []
    for c in SC.image_cases():
        a, b = R.oracle_image_launch(c), R.ref_image_launch(c)
        fracs.append(R.compare_with_b(c, b, a["q"], a["d"], a["sums"], a["af"], a["x"], worst))
        hand += R.check_expectations(c, a["q"], a["d"], a["sums"])
        K = c["K"]                                                          # and the decoders on the oracle's raw images give the oracle's values back
        assert np.array_equal(R.decode_aq(a["raw"]["aq"], K)[:c["nrows"]], a["q"]) and np.array_equal(R.decode_abs(a["raw"]["abs"], K)[0][:c["nrows"]], a["sums"])
    for c in SC.fold_cases():
        a, b = R.oracle_fold_launch(c), R.ref_residual_fold(c)
        assert np.array_equal(a["x"].view(np.uint32), b["x"].view(np.uint32)), c["name"]
        want, bound = R.fold_bound(np.asarray(c["x"]).reshape(R.M, -1)[:c["nrows"]], c["partial"], c["ks"], c["n_total"], c["nrows"], c["K"])
        ratio = float((np.abs(a["x"][:c["nrows"]].astype(np.float64) - want) / bound).max())
        assert ratio <= 1.0, (c["name"], ratio)
        if ratio > worst.setdefault("fold", {}).get("x", (-1.0, ""))[0]:
            worst["fold"]["x"] = (ratio, c["name"])
    for c in SC.rope_cases():
        a, b = R.oracle_rope_launch(c), R.ref_rope_append(c)
        R.compare_rope(c, b, a["qbuf"], a["kcache"], a["vcache"], worst)
    R.print_worst(worst)
    print("reference B abstains on at most %.3f %% of a case's int8 values; %d hand-written expectations held" % (100.0 * max(fracs), hand))
    assert hand >= 200


def test_tk_divf_tk_sqrtf_and_tk_siluf_are_inside_the_constants_of_the_bounds():
    L = O.lib()
    L.orc_divf.restype = C.c_float
    L.orc_divf.argtypes = [C.c_float, C.c_float]
    rng = np.random.default_rng(1)
    A = np.concatenate([np.geomspace(1e-6, 1e6, 4000), rng.uniform(0.5, 2.0, 4000)]).astype(np.float32)
    B = np.concatenate([rng.uniform(0.5, 4.0, 4000), np.geomspace(1e-6, 1e6, 4000)]).astype(np.float32)
    div = max(abs(float(L.orc_divf(float(a), float(b))) / (float(a) / float(b)) - 1.0) for a, b in zip(A, B))
    inv = max(abs(float(L.orc_divf(-127.0, float(b))) / (-127.0 / float(b)) - 1.0) for b in B)
    print("tk_divf: worst relative error %.3g, of -127 / x %.3g (constant %.3g)" % (div, inv, R.DIVF_REL_ERR))
    assert max(div, inv) <= R.DIVF_REL_ERR
    S = np.concatenate([np.geomspace(1e-12, 1e12, 20000), rng.uniform(1.0, 4.0, 20000)]).astype(np.float32)
    sq = max(abs(float(L.orc_sqrtf(float(s))) / float(np.sqrt(np.float64(s))) - 1.0) for s in S)
    print("tk_sqrtf: worst relative error %.3g (constant %.3g)" % (sq, R.SQRTF_REL_ERR))
    assert sq <= R.SQRTF_REL_ERR
    G = np.concatenate([np.linspace(-90.0, 90.0, 36001), rng.uniform(-12.0, 12.0, 20000), np.geomspace(1e-8, 1.0, 2000), -np.geomspace(1e-8, 1.0, 2000)]).astype(np.float32)
    got = O.swiglu(G, np.ones_like(G)).astype(np.float64)
    g = G.astype(np.float64)
    want = g / (1.0 + np.exp(-g))
    excess = np.abs(got - want) - R.SILUF_ABS_ERR
    rel = float((excess[want != 0] / np.abs(want[want != 0])).max())
    print("tk_siluf: worst relative error beyond %.0e absolute on [-90, 90]: %.3g (constant %.3g)" % (R.SILUF_ABS_ERR, rel, R.SILUF_REL_ERR))
    assert rel <= R.SILUF_REL_ERR and got[G == 0].tolist() == [0.0] * int((G == 0).sum())


def test_tiles_hand_written_tables_and_embed_tables(tk):
    for c in SC.tiles_cases():
        b = R.ref_att_tiles(c)["tiles"]
        if c["expect_tiles"] is not None:
            want = np.array([len(c["expect_tiles"])] + c["expect_tiles"], np.int32)
            assert np.array_equal(b[:len(want)], want), c["name"]
            assert np.all(b[len(want):] == SC.TILE_FILL)
    for ttype in (tk.TYPE_Q4_K, tk.TYPE_Q6_K):                              # where the oracle has a decoder of its own it agrees with the table's
        blocks = SC.embed_table(tk, ttype, 256)
        assert np.array_equal(SC.decode_table(tk, ttype, blocks, 256).view(np.uint32), O.dequant_rows(ttype, blocks, SC.EMBED_VOCAB, 256).view(np.uint32))
    assert len(SC.embed_types(tk)) == 17 and len(SC.embed_cases(tk)) == 34


def test_the_hook_refuses_without_touching_a_device(tk):
    refused, accepted = SC.refusals(tk)
    for name, op, kw in refused:
        with pytest.raises(tk.TkError) as e:
            tk.llm_step_probe(op, device=-1, **kw)
        assert e.value.code == 1001, name
    for name, op, kw in accepted:
        out = tk.llm_step_probe(op, device=-1, **kw)                        # validated only: every in/out array as it was handed in
        for k, v in out.items():
            if v is not None and k in kw and kw[k] is not None:
                assert v.tobytes() == np.asarray(kw[k]).tobytes(), (name, k)
    for c in SC.image_cases() + SC.fold_cases() + SC.rope_cases() + SC.tiles_cases() + SC.embed_cases(tk):   # and no GPU case is a shape the hook refuses
        op, kw = SC.probe_kwargs(tk, c)
        tk.llm_step_probe(op, device=-1, **kw)
    for c in SC.fused_cases() + SC.wide_cases():
        op, kw = SC.twin_kwargs(tk, c)
        tk.llm_step_probe(op, device=-1, **kw)
    assert len(SC.fused_cases()) == 42 and len(SC.wide_cases()) == 4
