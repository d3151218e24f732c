"""Every step kernel of the LLM stream alone, ONE launch at a time (tk_mi355x_llm_step_probe) on crafted rows: k_embed, k_rmsnorm_q8, k_residual_fold,
k_swiglu_q8<1> / <8>, k_quant_q8, k_qkv_rope_append, k_att_pv_join<64> / <128>, k_att_tiles, and quantize_chunk8, the Q8 image writer under five of them;
and the twins: the mat-vec launch's norm and SwiGLU prologues against the stand-alone kernels, the 32x32x32 kernel's SwiGLU epilogue against k_swiglu_q8.

Reference A, bit for bit: the oracle's own steps (orc_slab_sum, orc_rmsnorm, orc_swiglu, orc_divf, orc_rope_pair, orc_q8k_quantize, orc_round_through,
orc_f32_to_f16 — the functions orc_llm_forward calls), laid out by the image encoder of tests/llm_step_ref.py: every byte of every image, cache and
table, the bytes a launch must not touch included (all pre-filled with a sentinel).
Reference B, independent: tests/llm_step_ref.py (float64 NumPy written from the layout's and the kernels' comments): the raw images decoded by
reshaping, every q, sub-block sum, f16 cache half and tile entry it decides (it abstains within 1.3e-3 of a half-integer of iscale * x on elements that
are not crafted; tests/test_llm_step_cpu.py caps that at 1 % of a case), the hand-written expectations of the crafted rows, and the floats (ad, af,
qbuf, x after a fold) inside bounds derived from the documented operation order.  The worst error / bound per op is printed.
tests/test_llm_step_cpu.py shows that each of the modelled kernel errors changes what at least one of these cases leaves behind.

Rows with NaN or Inf and blocks whose maximum makes -127 / max overflow are left out: undefined on both sides, no contract.  No case is a shape the
hook ought to refuse (the CPU file runs every case through the hook's validation), and none is meant to fault the device."""
import numpy as np
import pytest

import llm_step_cases as SC
import llm_step_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu


def launch(gpu, c):
    op, kw = SC.probe_kwargs(gpu, c)
    return gpu.llm_step_probe(op, **kw)


def image_family(gpu, cases):
    worst, hand = {}, 0
    for c in cases:
        got = launch(gpu, c)
        a, b = R.oracle_image_launch(c), R.ref_image_launch(c)
        K, nrows = c["K"], c["nrows"]
        for name, want in a["raw"].items():                                # reference A: the raw images whole, sentinels past the rows' own bytes included
            if want is not None:
                bad = np.flatnonzero(got[name].view(np.uint8) != want.view(np.uint8))
                assert bad.size == 0, (c["name"], name, bad[:8], got[name].view(np.uint8)[bad[:8]], want.view(np.uint8)[bad[:8]])
        if a["x"] is not None:
            assert np.array_equal(got["x"].view(np.uint32), a["x"].reshape(-1).view(np.uint32)), (c["name"], "x")
        q, d = R.decode_aq(got["aq"], K)[:nrows], R.decode_ad(got["ad"], K)[:nrows]
        sums, lo, hi = R.decode_abs(got["abs"], K)
        sums16, hh, ll = R.decode_abs16(got["abs16"], K)
        assert lo[:nrows].min() >= 0 and lo[:nrows].max() <= 63 and np.isin(ll[:nrows], (0.0, 1.0)).all(), c["name"]
        assert np.array_equal(sums16[:nrows], sums[:nrows].astype(np.float64)), (c["name"], "2 hh + ll against 64 h + l")
        assert np.array_equal(sums[:nrows], q.astype(np.int64).reshape(nrows, K // 32, 32).sum(axis=2)), (c["name"], "the sums of the launch's own q")
        af = R.decode_af(got["af"], K)[:nrows] if c["want_af"] else None
        x = got["x"].reshape(R.M, K) if c["op"] == "rmsnorm" else None
        R.compare_with_b(c, b, q, d, sums[:nrows], af, x, worst)
        hand += R.check_expectations(c, q, d, sums[:nrows])
    R.print_worst(worst)
    return hand


def test_k_rmsnorm_q8(gpu):
    assert image_family(gpu, SC.rmsnorm_cases()) >= 100


def test_k_swiglu_q8(gpu):
    assert image_family(gpu, SC.swiglu_cases()) >= 50


def test_k_quant_q8(gpu):
    assert image_family(gpu, SC.quant_cases()) >= 100


def test_k_att_pv_join(gpu):
    assert image_family(gpu, SC.pv_join_cases()) >= 10


def test_k_residual_fold(gpu):
    worst = {}
    for c in SC.fold_cases():
        got = launch(gpu, c)["x"]
        a, b = R.oracle_fold_launch(c), R.ref_residual_fold(c)
        assert np.array_equal(got.view(np.uint32), a["x"].reshape(-1).view(np.uint32)), c["name"]      # the rows past nrows as they went in
        assert np.array_equal(got.view(np.uint32), b["x"].reshape(-1).view(np.uint32)), c["name"]
        want, bound = R.fold_bound(np.asarray(c["x"]).reshape(R.M, -1)[:c["nrows"]], c["partial"], c["ks"], c["n_total"], c["nrows"], c["K"])
        ratio = float((np.abs(got.reshape(R.M, -1)[:c["nrows"]].astype(np.float64) - want) / bound).max())
        assert ratio <= 1.0, (c["name"], ratio)
        if ratio > worst.setdefault("fold", {}).get("x", (-1.0, ""))[0]:
            worst["fold"]["x"] = (ratio, c["name"])
    R.print_worst(worst)


def test_k_qkv_rope_append(gpu):
    worst = {}
    for c in SC.rope_cases():
        got = launch(gpu, c)
        a, b = R.oracle_rope_launch(c), R.ref_rope_append(c)
        for k in ("qbuf", "kcache", "vcache"):                             # whole: every half outside the rows written keeps its sentinel
            bad = np.flatnonzero(got[k] != a[k].reshape(-1)) if k != "qbuf" else np.flatnonzero(got[k].view(np.uint32) != a[k].reshape(-1).view(np.uint32))
            assert bad.size == 0, (c["name"], k, bad[:8])
        R.compare_rope(c, b, got["qbuf"], got["kcache"], got["vcache"], worst)
    R.print_worst(worst)


def test_k_att_tiles(gpu):
    for c in SC.tiles_cases():
        got = launch(gpu, c)["tiles"]
        assert np.array_equal(got, R.ref_att_tiles(c)["tiles"]), (c["name"], got[:8])
        if c["expect_tiles"] is not None:
            want = np.array([len(c["expect_tiles"])] + c["expect_tiles"], np.int32)
            assert np.array_equal(got[:len(want)], want) and np.all(got[len(want):] == SC.TILE_FILL), c["name"]


def test_k_embed(gpu):
    for c in SC.embed_cases(gpu):
        got = launch(gpu, c)["x"]
        want = R.ref_embed(c, SC.decode_table(gpu, c["type"], c["embd"], c["K"]))["x"]
        assert np.array_equal(got.view(np.uint32), want.reshape(-1).view(np.uint32)), c["name"]


def oracle_slab_sums(y, ks, nrows):
    """[nrows][TWIN_ROWS]: the K-split slabs of y [ks][M][TWIN_ROWS] added in ascending order"""
    n = SC.TWIN_ROWS
    return np.stack([O.slab_sum(y[r * n:], ks, R.M * n, n) for r in range(nrows)])


@pytest.mark.parametrize("twin", ["norm", "swiglu"])
def test_the_fused_producers_equal_the_stand_alone_kernels(gpu, twin):
    """k_rmsnorm_q8 / k_swiglu_q8 followed by a plain mat-vec launch, and the mat-vec launch that forms its image itself (TkGemvArgs::fuse 1 / 2), on the
    same rows: the same slabs bit for bit, the same updated residual rows, and the oracle's mat-vec on the oracle's image"""
    for c in SC.fused_cases():
        if c["twin"] != twin:
            continue
        op, kw = SC.twin_kwargs(gpu, c)
        got = gpu.llm_step_probe(op, **kw)
        nrows, K, ks = c["nrows"], c["K"], c["gemv_ks"]
        assert np.array_equal(got["y_a"].view(np.uint32), got["y_b"].view(np.uint32)), (c["name"], np.flatnonzero(got["y_a"] != got["y_b"])[:8])
        ya = got["y_a"].reshape(ks, R.M, SC.TWIN_ROWS)
        assert np.all(ya[:, nrows:] == SC.Y_FILL) and not np.any(ya[:, :nrows] == SC.Y_FILL), (c["name"], "slab rows past the pass's")
        a = R.oracle_image_launch(c)
        if twin == "norm":
            xa, xb = got["x"].reshape(R.M, K), got["x_b"].reshape(R.M, K)
            assert np.array_equal(xa.view(np.uint32), a["x"].view(np.uint32)), (c["name"], "x of the stand-alone norm")
            assert np.array_equal(xb[:nrows].view(np.uint32), a["x"][:nrows].view(np.uint32)) and np.all(xb[nrows:] == SC.Y_FILL), (c["name"], "fx_out")
        want = np.stack([O.gemv_q8(c["wtype"], c["wblocks"], SC.TWIN_ROWS, K, ks, a["v"][r]) for r in range(nrows)])
        assert np.array_equal(oracle_slab_sums(got["y_a"], ks, nrows).view(np.uint32), want.view(np.uint32)), (c["name"], "orc_gemv_q8 on the oracle's image")


def test_the_wide_swiglu_epilogue_equals_k_swiglu_q8(gpu):
    """the 32x32x32 kernel's SwiGLU epilogue followed by k_quant_q8, and the plain gate | up launch followed by k_swiglu_q8, at 193 and 256 rows: the two Q8
    images byte for byte, and both the oracle's"""
    for c in SC.wide_cases():
        op, kw = SC.twin_kwargs(gpu, c)
        got = gpu.llm_step_probe(op, **kw)
        nrows, D, FF = c["nrows"], c["K"], c["wrows"]
        for k in ("aq", "ad", "abs", "abs16"):
            assert got[k].tobytes() == got[k + "_b"].tobytes(), (c["name"], k)
        x = c["x"].reshape(nrows, D)
        nb = len(c["wblocks"]) // 2
        v = np.stack([O.swiglu(O.gemv_q8(c["wtype"], c["wblocks"][:nb], FF, D, 1, x[r]), O.gemv_q8(c["wtype"], c["wblocks"][nb:], FF, D, 1, x[r])) for r in range(nrows)])
        q, d, sums = zip(*[O.q8k_quantize(v[r]) for r in range(nrows)])
        want = R.encode_image(FF, nrows, c["fill"], np.stack(q), np.stack(d), np.stack(sums))
        for k in ("aq", "ad", "abs", "abs16"):
            assert got[k].tobytes() == want[k].tobytes(), (c["name"], k, "the oracle's image")


def test_the_hook_refuses_on_a_machine_with_a_device_too(gpu):
    refused, accepted = SC.refusals(gpu)
    for name, op, kw in refused:                                            # validation comes before the device is touched: device = -1 and 0 answer alike
        for device in (-1, 0):
            with pytest.raises(gpu.TkError) as e:
                gpu.llm_step_probe(op, device=device, **kw)
            assert e.value.code == 1001, (name, device)
    with pytest.raises(gpu.TkError) as e:
        gpu.llm_step_probe(accepted[0][1], device=99, **accepted[0][2])
    assert e.value.code == 1001
