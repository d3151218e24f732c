"""The detector's post-processing kernels alone, ONE decode + rank + mask + scan sequence per launch (tk_mi355x_detector_post_probe) on crafted frames:
k_yolo_decode (raw head maps), k_yolo_decode_out (a graph's decoded output), k_yolo_rank, k_yolo_mask, k_yolo_scan.

Reference A, bit for bit: the oracle (orc_yolo_post_ranked / orc_yolo_post_out_ranked) — every anchor's decoded record, the ranked list, the survivors.
Reference B, independent: tests/yolo_post_ref.py (float64 NumPy written from the kernels' comments) — decoded boxes and scores inside bounds derived
term by term, the candidate set, classes, ranked list and survivors on every frame B decides (tests/test_yolo_post_cpu.py: no crafted frame and at
most 1 in 20 random frames abstains), the suppression matrix bit by bit where the ranked list is short, and answers derived by hand.
Stale buffers: the six in/out arrays start as 0xFF bytes; order beyond n_cand, kept beyond n_kept and every word of the suppression matrix outside
[n_cand rows] x [ceil(n_cand / 64) words] must still hold them.
tests/test_yolo_post_cpu.py shows that each of the modelled kernel errors changes the answer of at least one of these cases.

Worst error / bound on the MI355X: k_yolo_decode boxes 0.77, scores 0.61 (the oracle's figures: the kernels match it bit for bit);
k_yolo_decode_out boxes 1.00 (one correctly rounded subtraction against half an ulp)."""
import functools

import numpy as np
import pytest

import yolo_post_cases as YC
import yolo_post_ref as R

pytestmark = pytest.mark.gpu
CASES = YC.by_name()


@functools.lru_cache(maxsize=None)
def references(name):
    c = CASES[name]
    small = all(int(np.count_nonzero(c["out"][f, 4:].max(axis=0) > c["conf"])) <= 300 for f in range(c["B"])) if c["kind"] == 1 else c["n_anchors"] <= 300
    return YC.oracle_frames(c), R.run_case(c, want_pairs=small)


def launch(gpu, c, **kw):
    if c["kind"] == 0:
        return gpu.detector_post_probe(c["B"], c["nc"], c["n_anchors"], c["conf"], c["iou"], heads=c["heads"], ld=c["ld"], in_w=c["in_w"], in_h=c["in_h"], **kw)
    return gpu.detector_post_probe(c["B"], c["nc"], c["n_anchors"], c["conf"], c["iou"], out=c["out"], **kw)


def stale(x):
    return bool(np.all(np.ascontiguousarray(x).view(np.uint8) == 0xFF))


@pytest.mark.parametrize("name", list(CASES))
def test_detector_post(gpu, name):
    c = CASES[name]
    got = launch(gpu, c)
    ref_a, ref_b = references(name)
    for f in range(c["B"]):
        a, (dec, res) = ref_a[f], ref_b[f]
        n, nk = int(got["n_cand"][f]), int(got["n_kept"][f])
        print(name, "frame", f, "candidates", n, "survivors", nk, "(reference B abstains)" if res["abstain"] else "")
        # reference A: bit for bit
        assert got["cand"][f].tobytes() == a["cand"].tobytes()
        assert n == a["n_cand"] and np.array_equal(got["order"][f, :n], a["order"])
        assert nk == a["n_kept"] and got["kept"][f, :nk].tobytes() == a["kept"].tobytes()
        # what an earlier call left beyond this call's counts is neither read (the answers above) nor written
        assert stale(got["order"][f, n:]) and stale(got["kept"][f, nk:])
        words = (n + 63) // 64
        assert stale(got["mask"][f, n:]) and stale(got["mask"][f, :n, words:])
        bits = np.unpackbits(got["mask"][f, :n, :words].view(np.uint8).reshape(n, words * 8), axis=1, bitorder="little") if n else np.zeros((0, 0), np.uint8)
        assert not np.any(np.tril(bits[:, :n])) and not np.any(bits[:, n:])     # bit j of row i only for i < j < n_cand
        # reference B
        rb, rs = R.compare_frame(dict(cand=got["cand"][f], order=got["order"][f], n_cand=n, kept=got["kept"][f], n_kept=nk), dec, res)
        print("  %s: worst box error / bound = %.2f, worst score error / bound = %.2f" % ("k_yolo_decode" if c["kind"] == 0 else "k_yolo_decode_out", rb, rs))
        if res["pairs"] is not None and not res["abstain"]:
            decided = res["pairs"] >= 0
            assert np.array_equal(bits[:, :n][decided], res["pairs"][decided].astype(np.uint8))
        want = c["expect"].get(f, {})
        if "n_cand" in want:
            assert n == want["n_cand"]
        if "kept" in want:
            assert got["kept"]["anchor"][f, :nk].tolist() == want["kept"]
        if "order_head" in want:
            assert got["order"][f, :len(want["order_head"])].tolist() == want["order_head"]


def test_the_suppressor_at_rank_3_sets_the_first_bit_of_word_1_and_the_last_bit_of_word_31(gpu):
    got = launch(gpu, CASES["k1_suppressor_rank3"])
    row = got["mask"][0, 3]
    assert row[0] == np.uint64(1) << np.uint64(63) and row[1] == np.uint64(1) and row[31] == np.uint64(1) << np.uint64(63) and not np.any(row[2:31])


def test_the_answer_does_not_depend_on_what_the_buffers_held(gpu):
    for name in ("k1_batch_2100_0_65", "k0_64x96_random"):
        c = CASES[name]
        a, b = launch(gpu, c), launch(gpu, c, stale=0x00, with_mask=False)
        for f in range(c["B"]):
            n, nk = int(a["n_cand"][f]), int(a["n_kept"][f])
            assert n == b["n_cand"][f] and nk == b["n_kept"][f]
            assert np.array_equal(a["order"][f, :n], b["order"][f, :n]) and a["kept"][f, :nk].tobytes() == b["kept"][f, :nk].tobytes()
            assert a["cand"][f].tobytes() == b["cand"][f].tobytes()


def test_the_hook_refuses_on_the_device_too(gpu):
    refused, accepted = YC.refusals()
    for device in (0, -1):
        for name, kw in refused:
            with pytest.raises(gpu.TkError) as e:
                gpu.detector_post_probe(device=device, **kw)
            assert e.value.code == 1001, (name, device)
    with pytest.raises(gpu.TkError) as e:
        gpu.detector_post_probe(device=99, **accepted[0][1])
    assert e.value.code == 1001
