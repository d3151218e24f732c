"""CPU: the cases of tests/test_yolo_post_gpu.py discriminate, and the oracle (reference A) stands inside everything the GPU file asks of the kernels.

- every mutation switch of tests/yolo_post_ref.py (one plausible kernel error each) changes the answer of at least one GPU case;
- the oracle's decoded boxes and scores lie inside reference B's bounds at every case, its ranked list and survivors equal B's on every frame B
  decides, no crafted frame abstains and at most 1 in 20 random frames does; hand-derived answers hold;
- the test hook refuses what it must without touching a device (device = -1)."""
import functools

import numpy as np
import pytest

import yolo_post_cases as YC
import yolo_post_ref as R


@functools.lru_cache(maxsize=None)
def answers(mut):
    """the discrete answer of every frame of every case under one mutation switch (or none)"""
    m = (mut,) if mut else ()
    out = {}
    for c in YC.cases():
        out[c["name"]] = [(np.flatnonzero(p["valid"]).tolist(), d["cls"][p["valid"]].tolist(), p["order"].tolist(), p["kept"].tolist(),
                           np.round(d["box"][p["kept"]], 3).tolist()) for d, p in R.run_case(c, m)]
    return out


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_mutant_is_noticed_by_a_gpu_case(mut):
    base, got = answers(""), answers(mut)
    noticed = [n for n in base if base[n] != got[n]]
    print(mut, "noticed by", noticed[:8])
    assert noticed, "no case of the GPU list notices the mutation %r: a case is missing" % mut


def test_the_oracle_is_inside_reference_b_and_abstentions_stay_under_one_in_twenty():
    random_frames = abstained = 0
    worst = {0: [0.0, 0.0], 1: [0.0, 0.0]}
    for c in YC.cases():
        a = YC.oracle_frames(c)
        for f, (dec, res) in enumerate(R.run_case(c)):
            if c["random"]:
                random_frames += 1
                abstained += int(res["abstain"])
            else:
                assert not res["abstain"], (c["name"], f, res["why"])        # crafted frames: integer grid, binary fractions
            rb, rs = R.compare_frame(a[f], dec, res)
            worst[c["kind"]] = [max(worst[c["kind"]][0], rb), max(worst[c["kind"]][1], rs)]
            want = c["expect"].get(f, {})
            if "n_cand" in want:
                assert a[f]["n_cand"] == want["n_cand"], (c["name"], f)
            if "kept" in want:
                assert a[f]["kept"]["anchor"].tolist() == want["kept"], (c["name"], f)
            if "order_head" in want:
                assert a[f]["order"][:len(want["order_head"])].tolist() == want["order_head"], (c["name"], f)
    print("reference B abstains on %d of %d random frames" % (abstained, random_frames))
    print("oracle, k_yolo_decode (DFL + sigmoid): worst box error / bound = %.2f, worst score error / bound = %.2f" % tuple(worst[0]))
    print("oracle, k_yolo_decode_out (centre -/+ size / 2: one rounding): worst box error / bound = %.2f" % worst[1][0])
    assert random_frames >= 20 and abstained * 20 <= random_frames


def test_every_edge_the_kernels_have_is_reached():
    cs = YC.cases()
    n_cand = {p["n_cand"] for c in cs for _, p in R.run_case(c)}
    assert {0, 1, 63, 64, 65, 2047, 2048} <= n_cand
    assert any(int(p["valid"].sum()) > 2048 for c in cs for _, p in R.run_case(c))          # more candidates than the cap
    assert any(p["n_kept"] == 500 and p["n_cand"] > 500 for c in cs for _, p in R.run_case(c))
    assert {c["n_anchors"] for c in cs if c["kind"] == 1} >= {1, 255, 256, 257, 2049, 3000}
    assert {c["n_anchors"] for c in cs if c["kind"] == 0} == {21, 126, 2100}
    assert {c["nc"] for c in cs} >= {1, 4, 80}
    assert any(c["kind"] == 0 and any(l > 64 + c["nc"] for l in c["ld"]) for c in cs)


def test_the_hook_refuses_without_touching_a_device(tk):
    refused, accepted = YC.refusals()
    for name, kw in refused:
        with pytest.raises(tk.TkError) as e:
            tk.detector_post_probe(device=-1, **kw)
        assert e.value.code == 1001, name
    for name, kw in accepted:
        out = tk.detector_post_probe(device=-1, **kw)
        assert all(np.all(v.view(np.uint8) == 0xFF) for v in out.values() if v is not None), name   # validate only: nothing written
