"""GPU: BF16 and F32 float matrices (GGML types 30 and 0) on the exact fp32 MFMA GEMM, bit for bit.  The contract is restated in tests/bf16_ref.py
(ggml's CPU arithmetic: a BF16 weight is its bits << 16 against bf16-rounded activations, an F32 weight as stored against unrounded ones; per
K-split slab one fmaf chain over k ascending from +0, the slabs added in ascending order) and pinned on the CPU by tests/test_bf16_f32_cpu.py.
Here the production pieces are held to it: tk_mi355x_llm_matmul_float_probe (tiling, operand-image producer, launcher, slab fold) against the
restatement and, independently, against float64 sums of torch-decoded operands; whole tiny models against anchors computed from their weights (the
layer-0 V rows, the logits); and the routes by which such a model comes to exist against each other.  Type 1 (F16) runs through the same probe
harness as the control."""
import ctypes as C

import numpy as np
import pytest

import bf16_ref as R
import gguf_util
import oracle_lib as O
from kquant_gpu_util import WIDTHS, install, oracle_cfg_from

pytestmark = pytest.mark.gpu

TYPES = [R.BF16, R.F32]
PROBE_TYPES = [R.BF16, R.F32, R.F16]
# K-split 1 / 2 / 4 over ranges of 256 k, and one range of 1024 k: ring slots of 128 k (up to 128 rows per block) and of 64 k (from 129 rows)
PROBE_SHAPES = [(256, 1), (512, 2), (1024, 4), (1024, 1)]
PROBE_NROWS = [1, 15, 16, 17, 32, 33, 128, 129, 256]        # every M-tile count the launcher picks (1, 2, 4, 8, 16) and both sides of each edge
SEG_ROWS = [16, 48, 128]                                    # one, two or three of them side by side in one launch
MODEL_WIDTHS = [1, 16, 33, 256]


def pow2(e):
    return np.float32(2.0) ** np.float32(e)


def edge_weights(ttype, rng, rows, K):
    """[rows][K] fp32 values, exact in the type: whole rows of edge cases at rows 0 .. 9 (inside every segment layout), again from row 16 and from
    row 64 on (the second and third segment), the rest general"""
    w = (0.02 * rng.standard_normal((rows, K))).astype(np.float32)
    if ttype != R.F32:
        w = R.decode(ttype, R.encode(ttype, w))
    sign = np.where(np.arange(K) % 2 == 0, 1.0, -1.0).astype(np.float32)
    e = np.zeros((10, K), np.float32)
    e[0] = 0.0 * sign                                                    # +0 and -0 alternating
    if ttype == R.F16:
        tiny, big_sub, top, lo, hi = pow2(-24), np.float32(1023) * pow2(-24), np.float32(65504.0), pow2(-10), pow2(10)
    else:
        tiny, big_sub, top, lo, hi = pow2(-133), np.float32(127) * pow2(-133), R.bf16_to_f32(np.array([0x7F7F], np.uint16))[0], pow2(-30), pow2(30)
    e[1] = tiny * sign                                                   # the smallest subnormal of the 2-byte type, both signs
    e[2] = big_sub * sign                                                # ... and the largest
    e[3, 5::256] = top                                                   # max-finite, at most one per 256 k (|a| <= 1/8: no overflow)
    e[3, 133::512] *= -1.0
    e[4, 0::2], e[4, 1::2] = hi, -lo                                     # neighbours 2^60 (f16: 2^20) apart and of opposite sign
    e[5, 0::2], e[5, 1::2] = -lo, hi
    if ttype == R.F16:
        e[6] = tiny * sign * rng.integers(1, 4, K).astype(np.float32)
    else:                                                                # products ~2^-136 and their partial sums: fp32-subnormal
        e[6] = pow2(-130) * sign * rng.integers(1, 4, K).astype(np.float32)
    e[7] = w[7] * sign * np.sign(w[7])                                   # general magnitudes, strictly alternating sign
    e[8] = np.abs(w[8])                                                  # one sign: the chain only grows
    e[9, :] = 0.0                                                        # one live weight per 256 k, at a position that walks
    for r in range(K // 256):
        e[9, 256 * r + (37 * r + 11) % 256] = np.float32(0.0234375)
    for at in (0, 16, 64):
        if at + 10 <= rows:
            w[at:at + 10] = e
    assert np.array_equal(R.decode(ttype, R.encode(ttype, w)).view(np.uint32), w.view(np.uint32))
    return w


def edge_activations(rng, n, K):
    """[n][K], |a| <= 1/8: whole rows of edge cases at rows 0 .. 7 (inside the 15-row pass), again from row 16, 128 and 248 on, the rest general.
    Every value that is no subnormal is a multiple of 2^-16: its product with the smallest bf16 subnormal (2^-133) is then a multiple of 2^-149, so
    the chains that run wholly below 2^-126 are exact sums in the reference too, and the float64 bound holds there without an exception for
    underflow.  The subnormal values stand beside normal ones in their rows, whose products dominate sum |a w|."""
    x = (np.rint(rng.standard_normal((n, K)) * 2.0 ** 10) * 2.0 ** -16).astype(np.float32)
    x = np.clip(x, -0.12, 0.12).astype(np.float32)
    x = (np.rint(x * 2.0 ** 16) * 2.0 ** -16).astype(np.float32)
    sgn = rng.integers(0, 2, K).astype(np.uint32) << 31
    m7 = rng.integers(0, 128, K).astype(np.uint32) << 16
    e = np.zeros((8, K), np.float32)
    expo = rng.integers(119, 124, K).astype(np.uint32) << 23             # 2^-8 .. 2^-4: the tie bit is 2^-16 or above
    e[0] = (sgn | expo | m7 | 0x8000).view(np.float32)                   # exact ties at the 8th mantissa bit, kept half odd and even
    top = np.uint32(123) << 23                                           # [2^-4, 2^-3): mantissa bits 11 and up are multiples of 2^-16
    e[1] = (sgn | top | m7 | np.where(np.arange(K) % 2 == 0, 0x8800, 0x7800).astype(np.uint32)).view(np.float32)    # just above / below a tie
    e[2] = (sgn | top | 0x7F8000 | (rng.integers(0, 16, K).astype(np.uint32) << 11)).view(np.float32)               # round up into the next binade
    e[3] = x[3]
    e[3, 1::2] = (sgn[1::2] | rng.integers(1, 0x800000, K // 2).astype(np.uint32)).view(np.float32)                 # fp32 subnormals at every other k
    e[4] = 0.0                                                           # an all-zero row
    e[5] = x[5]
    e[5, 0::4] = (sgn[0::4] | np.uint32(0x00008000)).view(np.float32)    # ties between zero and the smallest bf16 subnormal; -0 beside them
    e[5, 2::4] = -0.0
    e[6] = np.float32(0.109375)                                          # all equal: every partial sum of a chain is another multiple
    e[7] = np.where(np.arange(K) % 4 < 2, 0.0625, -0.0625).astype(np.float32)   # + + - -: against weights of alternating sign the chain turns back every other step
    for at in (0, 16, 128, 248):
        x[at:at + 8] = e
    assert np.abs(x).max() <= 0.125
    normal = np.abs(x) >= 2.0 ** -126
    assert np.array_equal(np.rint(x[normal].astype(np.float64) * 2.0 ** 16), x[normal].astype(np.float64) * 2.0 ** 16)
    r = R.round_act(R.BF16, x)
    assert (r[0] != x[0]).all() and (r[1] != x[1]).all() and (np.abs(r[2]) == 0.125).all() and (np.abs(r[0]).view(np.uint32) >> 16 & 1 == 0).all()
    return x


_case = {}


def probe_case(ttype, K, ks):
    """weights [192][K] (stored form), activations [256][K], the restatement's result [256][192], and — by torch's decode and rounding, summed in
    float64 — the exact result with its running-error bound; computed once"""
    key = (ttype, K, ks)
    if key not in _case:
        import torch
        rng = np.random.default_rng(1000 * ttype + K + ks)
        rows = sum(SEG_ROWS)
        w = edge_weights(ttype, rng, rows, K)
        stored = R.encode(ttype, w)
        x = edge_activations(rng, 256, K)
        want = R.matmul(ttype, stored, x, ks)
        assert np.isfinite(want).all()
        if ttype == R.BF16:
            w64 = torch.from_numpy(stored.view(np.int16).copy()).view(torch.bfloat16).double()
            a64 = torch.from_numpy(x.copy()).to(torch.bfloat16).double()
        elif ttype == R.F16:
            w64 = torch.from_numpy(stored.view(np.int16).copy()).view(torch.float16).double()
            a64 = torch.from_numpy(x.copy()).to(torch.float16).double()
        else:
            w64, a64 = torch.from_numpy(stored.copy()).double(), torch.from_numpy(x.copy()).double()
        y64 = (a64 @ w64.T).numpy()
        bound = (K + ks) * 2.0 ** -24 * (a64.abs() @ w64.abs().T).numpy()
        if ttype != R.F16:   # the edge cases are what they claim to be
            assert (np.abs(want[:, 6]) < 2.0 ** -126).mean() > 0.9 and (want[:8, 6] != 0).sum() >= 5   # subnormal results, not flushed
            assert np.abs(want[:, 3]).max() > 1e35                                                     # max-finite weights reach the result
        assert not want[4].any() and not want[:, 0].any()
        _case[key] = (stored, x, want, y64, bound, {})
    return _case[key]


def probe_outputs(gpu, ttype, K, ks):
    """the probe's output for every (segments, rows) of the case, run once"""
    stored, x, want, y64, bound, got = probe_case(ttype, K, ks)
    if not got:
        for nseg in (1, 2, 3):
            rows = sum(SEG_ROWS[:nseg])
            for n in PROBE_NROWS:
                got[(nseg, n)] = gpu.matmul_float_probe(ttype, stored[:rows], K, ks, x[:n], seg_rows=SEG_ROWS[:nseg])
    return got


@pytest.mark.parametrize("K,ks", PROBE_SHAPES)
@pytest.mark.parametrize("ttype", PROBE_TYPES)
def test_probe_equals_the_restated_contract(gpu, ttype, K, ks):
    """tiling, the operand-image producer with the type's rounding, one launch of one, two and three segments, K split ks ways, the slabs folded in
    ascending order: bit for bit the restatement, at every row count class and with whole rows of edge-case weights and activations"""
    stored, x, want, _, _, _ = probe_case(ttype, K, ks)
    got = probe_outputs(gpu, ttype, K, ks)
    for (nseg, n), y in got.items():
        rows = sum(SEG_ROWS[:nseg])
        assert y.shape == (n, rows) and np.isfinite(y).all()
        w = want[:n, :rows]
        bad = np.argwhere(y.view(np.uint32) != w.view(np.uint32))
        assert bad.size == 0, (R.NAME[ttype], K, ks, nseg, n, len(bad), bad[:8].tolist(), [(float(y[i, j]), float(w[i, j])) for i, j in bad[:4]])


@pytest.mark.parametrize("K,ks", PROBE_SHAPES)
@pytest.mark.parametrize("ttype", PROBE_TYPES)
def test_probe_is_within_the_running_error_bound_of_the_float64_sum(gpu, ttype, K, ks):
    """the same outputs against sums taken in float64 over operands that torch decoded and rounded (not tests/bf16_ref.py):
    |y - y64| <= (K + ks) 2^-24 sum |a_k w_k| for every output of every case, none excluded"""
    _, _, _, y64, bound, _ = probe_case(ttype, K, ks)
    got = probe_outputs(gpu, ttype, K, ks)
    for (nseg, n), y in got.items():
        rows = sum(SEG_ROWS[:nseg])
        err = np.abs(y.astype(np.float64) - y64[:n, :rows])
        over = np.argwhere(err > bound[:n, :rows])
        assert over.size == 0, (R.NAME[ttype], K, ks, nseg, n, len(over), over[:8].tolist(), [(float(err[i, j]), float(bound[i, j])) for i, j in over[:4]])


# ---- whole models ----

def stored_matrix(src, layer, which):
    t, buf = src.get_tensor(layer, which)
    return t, buf.view(np.float32 if t == R.F32 else np.uint16)


def rmsnorm_rows(x, w, eps):
    return np.stack([O.rmsnorm(r, w, eps) for r in np.ascontiguousarray(x, np.float32)])


def v_rows_want(src, hp, tok):
    """f16(ref(W_v, round(rmsnorm(embd_row(tok), attn_norm)))) of layer 0, as f16 bits [n][kv dim]: V carries no rope"""
    a = rmsnorm_rows(src.values[(-1, 0)][tok], src.values[(0, 0)], hp.rms_eps)
    t, wv = stored_matrix(src, 0, 3)
    return R.matmul(t, wv.reshape(hp.n_kv_head * hp.head_dim, hp.d_model), a, hp.ks_qkv).astype(np.float16).view(np.uint16)


def v_rows_got(sess, n):
    return np.stack([sess.kv_read(0, r, 0, 1)[1].reshape(-1) for r in range(n)])


def float_model(gpu, ttype, seed=4, type_of=None):
    model = gpu.LlmModel(gpu.TINY())
    hp = model.hparams
    cfg = oracle_cfg_from(hp, 4, 256)
    src = R.FloatSource(ttype, cfg, seed=seed, type_of=type_of)
    install(model, src, hp.n_layer)
    return model, hp, cfg, src


@pytest.mark.parametrize("ttype", TYPES)
def test_model_anchors_v_rows_and_logits(gpu, ttype):
    """a tiny model of the type loaded by set_tensor, at pass widths 1, 16, 33 and 256: the layer-0 V-cache rows are the reference product of W_v with
    the rounded RMS norm of the embedding rows (embedding decode, producer rounding, the q | k | v launch and its slab fold), and the logits are the
    reference product of the output matrix with the rounded final norm of the residual stream forward_stage hands out"""
    model, hp, cfg, src = float_model(gpu, ttype)
    assert (hp.d_model, hp.d_ff, hp.vocab, hp.n_layer) == (256, 512, 512, 2)
    rng = np.random.default_rng(21)
    for n in MODEL_WIDTHS:
        sess = gpu.LlmSession(model, n, 4)
        seq, pos = np.arange(n, dtype=np.int32), np.zeros(n, np.int32)
        tok = rng.integers(0, hp.vocab, n).astype(np.int32)
        logits, am = sess.forward(seq, pos, tok)
        got_v = v_rows_got(sess, n)
        want_v = v_rows_want(src, hp, tok)
        assert np.array_equal(got_v, want_v), (R.NAME[ttype], n, int((got_v != want_v).sum()))
        xf = np.zeros((n, hp.d_model), np.float32)
        sess.forward_stage(seq, pos, 0, hp.n_layer, tok=tok, x_out=xf)
        assert np.isfinite(xf).all() and xf.any()
        t, wo = stored_matrix(src, -1, 2)
        want = R.matmul(t, wo.reshape(hp.vocab, hp.d_model), rmsnorm_rows(xf, src.values[(-1, 1)], hp.rms_eps), hp.ks_out)
        assert np.isfinite(logits).all()
        assert np.array_equal(logits.view(np.uint32), want.view(np.uint32)), (R.NAME[ttype], n, np.abs(logits - want).max())
        assert np.array_equal(am, want.argmax(axis=1))
        sess.close()


def logits_at(gpu, model, hp, n, toks):
    """two positions of n sequences in passes of n rows"""
    sess = gpu.LlmSession(model, n, 4)
    seq = np.arange(n, dtype=np.int32)
    out = [sess.forward(seq, np.full(n, p, np.int32), toks[p][:n])[0].copy() for p in range(2)]
    sess.close()
    return out


@pytest.mark.parametrize("ttype", TYPES)
def test_logits_do_not_depend_on_the_width_the_fusion_switch_or_the_stage_split(gpu, monkeypatch, ttype):
    model, hp, cfg, src = float_model(gpu, ttype)
    rng = np.random.default_rng(22)
    toks = [rng.integers(0, hp.vocab, 256).astype(np.int32) for _ in range(2)]
    monkeypatch.setenv("TK_MI355X_NO_FUSE", "0")
    ref = logits_at(gpu, model, hp, 256, toks)
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all() and not np.array_equal(ref[0], ref[1])
    for no_fuse in ("0", "1"):
        monkeypatch.setenv("TK_MI355X_NO_FUSE", no_fuse)
        for n in WIDTHS:
            got = logits_at(gpu, model, hp, n, toks)
            for p in range(2):
                assert np.array_equal(got[p].view(np.uint32), ref[p][:n].view(np.uint32)), (R.NAME[ttype], no_fuse, n, p)
    monkeypatch.setenv("TK_MI355X_NO_FUSE", "0")
    # layers [0, 1) then [1, 2) with the stream handed over on the host = the whole pass
    for n in (1, 33):
        sess = gpu.LlmSession(model, n, 4)
        seq, pos = np.arange(n, dtype=np.int32), np.zeros(n, np.int32)
        whole, mid, split = (np.zeros((n, hp.d_model), np.float32) for _ in range(3))
        sess.forward_stage(seq, pos, 0, 2, tok=toks[0][:n], x_out=whole)
        sess.forward_stage(seq, pos, 0, 1, tok=toks[0][:n], x_out=mid)
        sess.forward_stage(seq, pos, 1, 2, x_in=mid, x_out=split)
        assert np.array_equal(whole.view(np.uint32), split.view(np.uint32)) and not np.array_equal(whole, mid)
        am = sess.forward_stage(seq, pos, 1, 2, x_in=mid, head=True)
        assert np.array_equal(am, ref[0][:n].argmax(axis=1))
        sess.close()


def borrowed(gpu, handle):
    """a loader's model handle as an LlmModel that does not own it"""
    m = gpu.LlmModel.__new__(gpu.LlmModel)
    m.h = handle
    return m


@pytest.mark.parametrize("ttype", TYPES)
def test_gguf_set_tensor_and_synthetic_routes(gpu, tmp_path, ttype):
    """the same weights through a GGUF file and through set_tensor give the same logits bits; the runner's greedy ids on the file are the arg-max
    loop of forward(); weight_bytes is 2 / 4 bytes per matrix element (layer matrices and output: tk_mi355x_llm_model_weight_bytes has always counted what a decode step
    streams through the matmuls, not the norm rows or token_embd, and keeps that definition for these types); synthetic://tiny-bf16 / -f32 is
    fill_synthetic_float's model; a handle filled in one float type may be filled again in another"""
    model, hp, cfg, src = float_model(gpu, ttype)
    path = str(tmp_path / "tiny.gguf")
    gguf_util.write_llama_gguf(path, src, O.tiny_config())
    from_file = gpu.LlmModel(gguf=path)
    fh = from_file.hparams
    assert fh.as_dict() == hp.as_dict()
    elems = hp.vocab * hp.d_model + hp.n_layer * sum(r * c for r, c in R.shapes(cfg).values())
    assert model.weight_bytes == from_file.weight_bytes == R.BYTES[ttype] * elems
    rng = np.random.default_rng(23)
    toks = [rng.integers(0, hp.vocab, 256).astype(np.int32) for _ in range(2)]
    a, b = logits_at(gpu, model, hp, 40, toks), logits_at(gpu, from_file, hp, 40, toks)
    for p in range(2):
        assert np.isfinite(a[p]).all() and np.array_equal(a[p].view(np.uint32), b[p].view(np.uint32)), p
    # tk_model_loader + tk_llm_runner on the file against forward()'s arg max, one row at a time
    ids = np.zeros(16, np.int32)
    n_ids = gpu.lib().tk_mi355x_gguf_tokenize(path.encode(), b"hello world", 1, ids.ctypes.data_as(C.c_void_p), 16)
    assert 2 <= n_ids <= 16
    sess = gpu.LlmSession(model, 1, 64)
    for p in range(n_ids):
        _, am = sess.forward([0], [p], [int(ids[p])])
    cur = int(am[0])
    loader = gpu.ModelLoader()
    h = loader.load(path)
    runner = gpu.LlmRunner(h, context_size=64)
    runner.prepare("hello world")
    said = 0
    for i in range(6):
        piece = runner.next_token()
        if cur == 2:
            assert piece is None
            break
        assert piece == gguf_util.expected_piece(hp.vocab, cur), (i, cur, piece)
        said += 1
        _, am = sess.forward([0], [n_ids + i], [cur])
        cur = int(am[0])
    assert said >= 1
    runner.close()
    loader.unload(h)
    sess.close()
    # the synthetic recipe: the loader's name for it, two fills alike, another model than the f16 recipe or the other float type
    name = "synthetic://tiny-bf16?seed=4" if ttype == R.BF16 else "synthetic://tiny-f32?seed=4"
    h = loader.load(name)
    by_name = borrowed(gpu, h)
    filled = gpu.LlmModel(gpu.TINY()).fill_synthetic_float(4, ttype)
    assert by_name.weight_bytes == filled.weight_bytes == R.BYTES[ttype] * elems
    s1, s2 = logits_at(gpu, by_name, hp, 16, toks), logits_at(gpu, filled, hp, 16, toks)
    assert np.isfinite(s1[0]).all() and np.array_equal(s1[0].view(np.uint32), s2[0].view(np.uint32)) and np.array_equal(s1[1].view(np.uint32), s2[1].view(np.uint32))
    f16 = logits_at(gpu, gpu.LlmModel(gpu.TINY()).fill_synthetic(4, f16=True), hp, 16, toks)
    other = logits_at(gpu, gpu.LlmModel(gpu.TINY()).fill_synthetic_float(4, R.F32 if ttype == R.BF16 else R.BF16), hp, 16, toks)
    assert not np.array_equal(s1[0], f16[0]) and not np.array_equal(s1[0], other[0])
    # the three recipes hold the same seeded values, rounded differently: they stay close
    assert np.abs(s1[0] - f16[0]).max() < 0.05 * np.abs(f16[0]).max()
    by_name.h = C.c_void_p()
    loader.unload(h)
    loader.close()
    for bad in (1, 2, 12, 14, 29, -1):
        with pytest.raises(gpu.TkError):
            gpu.LlmModel(gpu.TINY()).fill_synthetic_float(4, bad)
    # refilling a handle: the f16 recipe, then this type on the same handle, gives this type's model
    again = gpu.LlmModel(gpu.TINY()).fill_synthetic(4, f16=True)
    again.fill_synthetic_float(4, ttype)
    assert again.weight_bytes == R.BYTES[ttype] * elems
    s3 = logits_at(gpu, again, hp, 16, toks)
    assert np.array_equal(s3[0].view(np.uint32), s2[0].view(np.uint32)) and np.array_equal(s3[1].view(np.uint32), s2[1].view(np.uint32))


# ---- mixing and embedding ----

def test_two_float_types_among_the_matrices_fail_the_load(gpu, tmp_path):
    """F16 q beside BF16 k: set_tensor refuses the second, the GGUF load fails, and both name the two types; a float type beside quantised ones and
    any token_embd type are fine"""
    model = gpu.LlmModel(gpu.TINY())
    hp = model.hparams
    cfg = oracle_cfg_from(hp, 4, 4)
    mixed = lambda layer, which: R.F16 if (layer, which) == (0, 1) else R.BF16
    src = R.FloatSource(R.BF16, cfg, type_of=mixed)
    model.set_tensor(0, 1, *src.get_tensor(0, 1))
    with pytest.raises(gpu.TkError) as ei:
        model.set_tensor(0, 2, *src.get_tensor(0, 2))
    assert "F16" in ei.value.detail and "BF16" in ei.value.detail and "one float type" in ei.value.detail
    with pytest.raises(gpu.TkError) as ei:
        model.set_tensor(1, 8, R.F32, np.zeros((hp.d_model, hp.d_ff), np.float32))
    assert "F32" in ei.value.detail and "F16" in ei.value.detail
    # replacing the one float matrix by another type is no mix; token_embd does not count
    model.set_tensor(0, 1, *R.FloatSource(R.BF16, cfg).get_tensor(0, 1))
    model.set_tensor(0, 2, *src.get_tensor(0, 2))
    model.set_tensor(-1, 0, R.F16, np.zeros((hp.vocab, hp.d_model), np.float16))
    model.set_tensor(-1, 0, R.F32, np.zeros((hp.vocab, hp.d_model), np.float32))
    path = str(tmp_path / "mixed.gguf")
    gguf_util.write_llama_gguf(path, src, O.tiny_config())
    with pytest.raises(gpu.TkError) as ei:
        gpu.LlmModel(gguf=path)
    assert "F16" in ei.value.detail and "BF16" in ei.value.detail and "attn_" in ei.value.detail


def test_q4_k_m_model_with_a_bf16_or_f32_embedding(gpu):
    """token_embd is free of the one-float-type rule and of the matrices' types: a Q4_K_M model with a BF16, an F32 and an F16 token_embd holding the
    same values (exact in all three: eight significant bits, f16's normal range) gives the same layer-0 V rows and logits"""
    hp0 = gpu.TINY()
    rng = np.random.default_rng(31)
    m8 = rng.integers(128, 256, (hp0.vocab, hp0.d_model)).astype(np.float32)
    emb = (m8 * np.float32(2.0) ** rng.integers(-14, -8, (hp0.vocab, hp0.d_model)).astype(np.float32) * rng.choice([-1.0, 1.0], (hp0.vocab, hp0.d_model))).astype(np.float32)
    assert np.array_equal(R.decode(R.BF16, R.encode(R.BF16, emb)), emb) and np.array_equal(R.decode(R.F16, R.encode(R.F16, emb)), emb)
    tok = rng.integers(0, hp0.vocab, 33).astype(np.int32)
    seq, pos = np.arange(33, dtype=np.int32), np.zeros(33, np.int32)
    out = {}
    for t in (R.F16, R.BF16, R.F32):
        model = gpu.LlmModel(hp0).fill_synthetic(4)
        model.set_tensor(-1, 0, t, R.encode(t, emb))
        sess = gpu.LlmSession(model, 33, 4)
        logits, _ = sess.forward(seq, pos, tok)
        out[t] = (logits.copy(), v_rows_got(sess, 33))
        assert np.isfinite(logits).all()
        sess.close()
    plain = gpu.LlmModel(hp0).fill_synthetic(4)
    sess = gpu.LlmSession(plain, 33, 4)
    assert not np.array_equal(sess.forward(seq, pos, tok)[0], out[R.F16][0])       # the embedding is what was set
    sess.close()
    for t in (R.BF16, R.F32):
        assert np.array_equal(out[t][1], out[R.F16][1]), R.NAME[t]
        assert np.array_equal(out[t][0].view(np.uint32), out[R.F16][0].view(np.uint32)), R.NAME[t]


# ---- LoRA ----

@pytest.mark.parametrize("container", ["ggla", "gguf"])
@pytest.mark.parametrize("ttype", TYPES)
def test_lora_into_a_float_matrix(gpu, tmp_path, ttype, container):
    """a rank-4 adapter on layer 0's attn_v and on the output matrix of a model of the type, merged while the matrices are installed: w' = w + scale *
    delta stored through the type's conversion (tests/bf16_ref.py: lora_merge).  The merged weights are read back one column at a time: token t's
    embedding row is one-hot at k = t % d_model and the attention-output and ffn_down matrices are zero, so the residual stream stays the embedding
    row, the normed activation is one-hot, and logit n of row t is ONE product a_k w'[n][k] (exact for BF16) — all 256 columns of the output matrix
    in one pass, equal to the restatement on the reference-merged weights; the V rows read attn_v the same way
    (rounded to f16 by the cache).  The read-back goes through the model's own pass and not through tk_mi355x_llm_matmul_float_probe: the probe
    takes weights from the host and cannot reach a matrix that a model has installed and merged"""
    rng = np.random.default_rng(41)
    model = gpu.LlmModel(gpu.TINY())
    hp = model.hparams
    cfg = oracle_cfg_from(hp, 4, 256)
    src = R.FloatSource(ttype, cfg, seed=6)
    D, KVD, V = hp.d_model, hp.n_kv_head * hp.head_dim, hp.vocab
    for l in range(hp.n_layer):
        for which in (4, 8):                                               # attn_output and ffn_down: +0 everywhere
            r, c = R.shapes(cfg)[which]
            src.t[(l, which)] = (ttype, R.encode(ttype, np.zeros((r, c), np.float32)).view(np.uint8).reshape(-1))
    onehot = np.zeros((V, D), np.float32)
    onehot[np.arange(V), np.arange(V) % D] = 1.0
    src.t[(-1, 0)] = (ttype, R.encode(ttype, onehot).view(np.uint8).reshape(-1))
    factors = {(0, 3): ((rng.standard_normal((4, D)) * 0.01).astype(np.float32), (rng.standard_normal((KVD, 4)) * 0.01).astype(np.float32)),
               (-1, 2): ((rng.standard_normal((4, D)) * 0.01).astype(np.float32), (rng.standard_normal((V, 4)) * 0.01).astype(np.float32))}
    path = str(tmp_path / ("a." + container))
    if container == "ggla":
        gguf_util.write_lora_ggla(path, 4, 8, factors)
    else:
        gguf_util.write_lora_gguf(path, 8.0, factors)
    model.set_lora(path)
    install(model, src, hp.n_layer)
    assert model.lora_merged == 2
    merged = {}
    for (layer, which), (A, B) in factors.items():
        t, stored = stored_matrix(src, layer, which)
        merged[(layer, which)] = R.lora_merge(ttype, stored.reshape(B.shape[0], D), A, B, 8.0 / 4)
        assert not np.array_equal(merged[(layer, which)].reshape(-1), stored)
    n = 256
    seq, pos, tok = np.arange(n, dtype=np.int32), np.zeros(n, np.int32), np.arange(n, dtype=np.int32)
    sess = gpu.LlmSession(model, n, 4)
    logits, _ = sess.forward(seq, pos, tok)
    xf = np.zeros((n, D), np.float32)
    sess.forward_stage(seq, pos, 0, hp.n_layer, tok=tok, x_out=xf)
    assert np.array_equal(xf, onehot[:n])                                  # the stream is still the embedding rows
    a_out = rmsnorm_rows(xf, src.values[(-1, 1)], hp.rms_eps)
    assert ((a_out != 0).sum(axis=1) == 1).all() and (a_out.argmax(axis=1) == np.arange(n) % D).all()
    want = R.matmul(ttype, merged[(-1, 2)], a_out, 1)
    assert np.array_equal(logits.view(np.uint32), want.view(np.uint32)), np.abs(logits - want).max()
    unmerged = R.matmul(ttype, stored_matrix(src, -1, 2)[1].reshape(V, D), a_out, 1)
    assert (unmerged != want).mean() > 0.5                                 # the adapter reaches most weights
    if ttype == R.BF16:                                                    # one exact product per logit: the weight itself, read back
        ak = R.round_act(ttype, a_out)[np.arange(n), np.arange(n) % D]
        assert np.array_equal(logits.T, R.decode(ttype, merged[(-1, 2)])[:, :n] * ak[None, :])
    a_v = rmsnorm_rows(onehot[:n], src.values[(0, 0)], hp.rms_eps)
    want_v = R.matmul(ttype, merged[(0, 3)], a_v, hp.ks_qkv).astype(np.float16).view(np.uint16)
    assert np.array_equal(v_rows_got(sess, n), want_v)
    sess.close()
