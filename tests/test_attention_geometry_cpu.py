"""What tests/test_attention_geometry_gpu.py relies on, checked without a GPU:

  * the table: names, windows and positions are consistent, and the instantiations the cases claim are exactly the list written out below;
  * the oracle: for each geometry a ragged pass equals its rows evaluated one at a time;
  * the comparison can see a subtly wrong kernel.  Attention leaves the kernel only as a Q8 image, so an error that moves no q and no block
    scale is invisible by contract; for EVERY case of the table two deliberately wrong oracles (oracle_lib.attention_mutant: the four PV /
    denominator partial sums joined as (a0 + a2) + (a1 + a3); the score of position T - 2 left out) must give logits that differ in bits from
    the canonical ones in at least one row of the case;
  * the swizzle of a key row's 16-byte pieces (att_swizzle_mask in tk_llm_kernels.hip), restated: for every head_dim a model may have it is a
    permutation of the row's pieces and the reader undoes what the writers did.  The rule it replaced, piece ^ (row & (pieces - 1)), is shown
    to leave the row at head_dim 192."""
import numpy as np
import pytest

import attention_geometry_cases as G
import oracle_lib as O


def oracle_for(geometry, window, max_seq):
    nh, nkv, hd = G.GEOMETRIES[geometry]
    return O.OracleLlm(O.tiny_config(n_head=nh, n_kv_head=nkv, head_dim=hd, max_ctx=window, max_seq=max_seq, **G.MODEL), seed=4)


def load(orc, geometry, p):
    for s, (off, n) in p["preload"].items():
        k, v = G.kv_rows(geometry, off, n)
        orc.kv_write(0, s, 0, k, v)


# every instantiation a model the loader accepts can reach on 256 CUs, by the geometry that reaches it
COVERAGE = {
    "g4_d64": ["k_attention<4, fused, 64, 32>", "k_attention<4, fused, 64, 64>", "k_attention<4, unfused, 64, 32>", "k_attention<4, unfused, 64, 64>",
               "k_attention_prefill<64>", "k_att_scores_long<64> + k_att_pv_chain<64> + k_att_pv_join<64>"],
    "g2_d128": ["k_attention<2, fused, 128, 128>", "k_attention<2, fused, 128, 32>", "k_attention<2, fused, 128, 64>", "k_attention<2, unfused, 128, 128>",
                "k_attention<2, unfused, 128, 32>", "k_attention<2, unfused, 128, 64>", "k_attention_narrow(grp 2)", "k_attention_prefill<128>",
                "k_att_scores_long<128> + k_att_pv_chain<128> + k_att_pv_join<128>"],
    "g1_d256": ["k_attention<1, fused, 0, 32>", "k_attention<1, fused, 0, 64>", "k_attention<1, unfused, 0, 32>", "k_attention<1, unfused, 0, 64>"],
    "g2_d256": ["k_attention<2, fused, 0, 64>", "k_attention<2, unfused, 0, 64>"],
    "g2_d256_6kv": ["k_attention<2, fused, 0, 32>", "k_attention<2, fused, 0, 64>", "k_attention<2, unfused, 0, 32>", "k_attention<2, unfused, 0, 64>"],
    "g4_d256": ["k_attention<2, fused, 0, 64>", "k_attention<2, unfused, 0, 64>", "k_attention<4, fused, 0, 32>", "k_attention<4, fused, 0, 64>",
                "k_attention<4, unfused, 0, 32>", "k_attention<4, unfused, 0, 64>"],
    "g4_d192": ["k_attention<4, fused, 0, 64>", "k_attention<4, unfused, 0, 64>"],
}


@pytest.mark.parametrize("geometry", list(G.GEOMETRIES))
def test_table_is_consistent_and_names_what_it_claims(geometry):
    nh, nkv, hd = G.GEOMETRIES[geometry]
    assert nh % nkv == 0 and nh // nkv in (1, 2, 4) and hd % 64 == 0 and (nh // nkv * hd) % 256 == 0 and hd <= 256   # TkLlmModel::init takes it
    cs = G.cases(geometry)
    assert len({c["name"] for c in cs}) == len(cs)
    seen = set()
    for c in cs:
        assert {1, 2, 16, 200, 256} <= set(G.DECODE_PLAN[geometry])
        for p in G.passes(c):
            assert p["pos"].min() >= 0 and p["top"] < c["window"] and p["seq"].max() < p["bystander"] < G.max_seq(c) and p["seq"].size <= 256
            assert all(n <= c["window"] for _, n in p["preload"].values())
            assert (len(set(p["seq"].tolist())) == p["seq"].size) == c["fused"]
        seen.add(G.instantiation(geometry, c["plan"], c["fused"]))
        if c["kind"].startswith("decode"):     # every context length, in some pass of the case
            want = set(G.WINDOWS[c["window"]] + (G.WIDE_ONLY[c["window"]] if c["width"] > 8 else []))
            assert want == {int(x) for p in G.passes(c) for x in p["pos"]}
    assert sorted(seen) == sorted(COVERAGE[geometry])


def test_every_kernel_group_head_dim_class_and_slot_size_is_claimed_by_a_case():
    plans = [(c["plan"], c["fused"], G.hd_class(g)) for g in G.GEOMETRIES for c in G.cases(g)]
    assert {p[0] for p, _, _ in plans} == {G.RING, G.NARROW, G.PREFILL, G.LONG}
    ring = {(p[1], fused, hd, p[2]) for p, fused, hd in plans if p[0] == G.RING}
    assert {r[0] for r in ring} == {1, 2, 4} and {r[2] for r in ring} == {0, 64, 128} and {r[3] for r in ring} == {32, 64, 128}
    for gq, hd in ((1, 0), (2, 0), (4, 0), (2, 128), (4, 64)):   # both forms of every (group, head_dim class) a model can have, at every slot size
        for fused in (True, False):
            assert {r[3] for r in ring if r[:3] == (gq, fused, hd)} == ({32, 64, 128} if (gq, hd) == (2, 128) else {32, 64}), (gq, hd, fused)


@pytest.mark.parametrize("geometry", list(G.GEOMETRIES))
def test_oracle_ragged_pass_equals_its_rows_one_at_a_time(geometry):
    """the 200-row pass of the 260-position window: logits, id and the appended K / V row of every row, against an oracle that sees that row alone"""
    case = next(c for c in G.cases(geometry) if c["name"] == "w260_rows200")
    p = G.passes(case)[0]
    both, single = oracle_for(geometry, 260, 200), oracle_for(geometry, 260, 200)
    load(both, geometry, p)
    load(single, geometry, p)
    want, wam = both.forward(p["seq"], p["pos"], p["tok"])
    for r in range(p["seq"].size):
        s, at = int(p["seq"][r]), int(p["pos"][r])
        got, gam = single.forward([s], [at], [p["tok"][r]])
        assert np.array_equal(got[0].view(np.uint32), want[r].view(np.uint32)), (r, at)
        assert gam[0] == wam[r]
        a, b = both.kv_read(0, s, 0, min(at + 2, 260)), single.kv_read(0, s, 0, min(at + 2, 260))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    both.close()
    single.close()


@pytest.mark.parametrize("geometry", list(G.GEOMETRIES))
def test_each_mutant_changes_the_logits_of_every_case(geometry):
    """the rows that stand for a case (sub_pass: rows of a decode pass do not see each other) under the canonical oracle and under each mutant"""
    oracles = {}
    blind = []
    done = set()
    for c in G.cases(geometry):
        if c["passes_of"] in done:      # the same rows as a case already shown, through another kernel: the oracle's side is the same
            assert c["env"]
            continue
        done.add(c["passes_of"])
        key = c["window"]
        if key not in oracles:
            oracles[key] = oracle_for(geometry, key, 16)
        orc = oracles[key]
        differs = {O.ATT_MUTANT_JOIN_ORDER: False, O.ATT_MUTANT_SKIP_T2: False}
        for p in G.passes(c):
            sp = G.sub_pass(c, p)
            load(orc, geometry, sp)
            want, _ = orc.forward(sp["seq"], sp["pos"], sp["tok"])
            for which in differs:
                if not differs[which]:
                    with O.attention_mutant(which):
                        got, _ = orc.forward(sp["seq"], sp["pos"], sp["tok"])
                    differs[which] = not np.array_equal(got.view(np.uint32), want.view(np.uint32))
            if not blind and c is G.cases(geometry)[0]:                      # the switch is off again
                again, _ = orc.forward(sp["seq"], sp["pos"], sp["tok"])
                assert np.array_equal(again.view(np.uint32), want.view(np.uint32))
            if all(differs.values()):
                break
        blind += [(c["name"], which) for which, seen in differs.items() if not seen]
    for orc in oracles.values():
        orc.close()
    assert not blind, blind


# ------------------------------------------------------------------------------------------ the key rows' swizzle
def lds_row_after_staging(head_dim, row, mask):
    """att_stage: LDS piece slot cs of row `row` receives the row's piece cs ^ (row & mask); -1 where the source lies outside the row"""
    ppr = head_dim // 8
    src = [cs ^ (row & mask) for cs in range(ppr)]
    return [s if 0 <= s < ppr else -1 for s in src]


def lds_row_after_patch(head_dim, row, mask):
    """the own-row patch: thread t < ppr stores piece t of the row's own key into slot t ^ (row & mask)"""
    ppr = head_dim // 8
    slots = [-1] * (2 * ppr)                                   # room to see a store past the row
    for t in range(ppr):
        slots[t ^ (row & mask)] = t
    return slots


def pieces_the_reader_sees(head_dim, row, mask, lds_row):
    """the score loop reads slot i ^ (row & mask) and takes it for piece i"""
    ppr = head_dim // 8
    return [lds_row[i ^ (row & mask)] if (i ^ (row & mask)) < len(lds_row) else -1 for i in range(ppr)]


def test_swizzle_is_a_permutation_and_reader_and_writers_agree():
    dims = G.accepted_head_dims()
    assert dims == [64, 128, 192, 256]
    for hd in dims + [320, 384, 448, 512]:                    # the arithmetic holds for every multiple of 64, accepted or not
        ppr, mask = hd // 8, G.swizzle_mask(hd)
        assert ppr % (mask + 1) == 0 and (mask + 1) & mask == 0
        for row in range(128):
            staged = lds_row_after_staging(hd, row, mask)
            assert sorted(staged) == list(range(ppr)), (hd, row)
            patched = lds_row_after_patch(hd, row, mask)
            assert patched[ppr:] == [-1] * ppr and sorted(patched[:ppr]) == list(range(ppr)), (hd, row)
            assert patched[:ppr] == staged
            assert pieces_the_reader_sees(hd, row, mask, staged) == list(range(ppr)), (hd, row)
    assert [G.swizzle_mask(hd) for hd in dims] == [7, 15, 7, 31]


def test_the_rule_before_the_fix_leaves_the_row_at_head_dim_192():
    """piece ^ (row & (ppr - 1)) with ppr = 24: piece 8 of row 16 is fetched from piece 24 — the next position's bytes — and the patch stores
    there; at the power-of-two sizes the two rules are the same"""
    old = lambda hd: hd // 8 - 1
    assert (8 ^ (16 & old(192))) == 24
    assert -1 in lds_row_after_staging(192, 16, old(192))
    assert lds_row_after_patch(192, 16, old(192))[24] == 8
    for hd in (64, 128, 256):
        assert old(hd) == G.swizzle_mask(hd)
    bad = [hd for hd in range(64, 513, 64) if any(-1 in lds_row_after_staging(hd, row, old(hd)) for row in range(128))]
    assert bad == [192, 320, 384, 448]
