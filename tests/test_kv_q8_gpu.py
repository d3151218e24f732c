"""GPU: the Q8_0 KV cache (csrc/common/tk_kv_q8.h) — the production append and attention launches alone (tk_mi355x_kv_q8_probe at device 0 against
its host loops at device -1, bit for bit), a Q8_0 session against the oracle and an F16 session on rows that quantise without loss, the append
path against the restatement tests/kv_q8_ref.py of the rows an F16 session holds, the independence of a row's bits from the pass that wrote it,
the session and model surface, and runners on a Q8_0 model.

There is no closeness test against the f16 cache, on purpose: the first three fix the quantiser as ggml's and the attention as the oracle's
arithmetic on the dequantised values, exactly; what remains is the accuracy of Q8_0 itself."""
import numpy as np
import pytest

import attention_geometry_cases as G
import kv_q8_ref as R
import oracle_lib as O
from test_kv_q8_cpu import crafted_blocks, empty_cache, quantise_and_check, seeded_rows, SHAPE
from test_llm_gpu import oracle_cfg_from

pytestmark = pytest.mark.gpu

TK_ERROR_INVALID_ARGUMENT, TK_ERROR_NOT_IMPLEMENTED = 1001, 1003
WIDTHS = (1, 2, 16, 129, 256)
SEED = 4
PATH = "synthetic://tiny?seed=%d" % SEED


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. the probe: one production launch against the host loops -----------------------------------------------------------------------------------

@pytest.mark.parametrize("head_dim", G.accepted_head_dims())
def test_append_launch_equals_the_host_quantiser(gpu, head_dim):
    seq, pos = np.array([0, 2, 2, 1], np.int32), np.array([0, 39, 7, 20], np.int32)
    for case, scale in enumerate((0.02, 1.0, 40.0)):
        k16, v16 = seeded_rows(4, SHAPE[2], head_dim, scale, 2 * case), seeded_rows(4, SHAPE[2], head_dim, scale, 2 * case + 1)
        host = quantise_and_check(gpu, k16, v16, seq, pos, case % 2, head_dim, device=-1)
        dev = quantise_and_check(gpu, k16, v16, seq, pos, case % 2, head_dim, device=0)  # sentinel-filled arrays: bystander rows keep it
        assert all(np.array_equal(a, b) for a, b in zip(host, dev))
    blocks = crafted_blocks()
    rows = np.zeros((3, SHAPE[2], head_dim), np.uint16)
    for r in range(3):
        for kvh in range(SHAPE[2]):
            for b in range(head_dim // 32):
                rows[r, kvh, 32 * b:32 * b + 32] = blocks[(2 * r + kvh + b) % len(blocks)]
    rows[2, 1] = 0  # an all-zero row
    quantise_and_check(gpu, rows, rows[::-1].copy(), [1, 1, 0], [3, 4, 39], 1, head_dim, device=0)


@pytest.mark.parametrize("geometry", list(G.GEOMETRIES))
def test_attention_launch_equals_the_host_loop(gpu, geometry):
    nh, nkv, hd = G.GEOMETRIES[geometry]
    nseq = 5  # rows share sequences (the launch only reads); sequence 4 is nobody's
    for window in (260, 261):
        shape = (1, nseq, nkv, window)
        rng = np.random.default_rng([3, window, nkv, hd])
        kq, kd = R.quantize((rng.standard_normal(shape + (hd,), dtype=np.float32) * np.float32(G.K_SCALE)).astype(np.float16).view(np.uint16))
        vq, vd = R.quantize((rng.standard_normal(shape + (hd,), dtype=np.float32) * np.float32(G.V_SCALE)).astype(np.float16).view(np.uint16))
        before = [a.copy() for a in (kq, kd, vq, vd)]
        for width in WIDTHS:
            plan = gpu.attention_plan(width, nh, nkv, hd, window, kv_type=gpu.KV_Q8_0)
            assert plan[0] == 6 and plan[2] in (32, 64)
            ch = plan[2]
            lengths = [1, ch - 1, ch, ch + 1, 2 * ch + 1, window]  # both sides of every chunk edge, and the window's last position
            seq = (np.arange(width) % 4).astype(np.int32)
            pos = np.array([lengths[(r + width) % len(lengths)] - 1 for r in range(width)], np.int32)
            q = rng.standard_normal((width, nh, hd), dtype=np.float32)
            host = gpu.kv_q8_attention_probe(kq, kd, vq, vd, seq, pos, q, device=-1, fill=np.float32(-77.0))
            dev = gpu.kv_q8_attention_probe(kq, kd, vq, vd, seq, pos, q, device=0, fill=np.float32(-77.0))
            bad = np.flatnonzero((bits(host) != bits(dev)).reshape(width, -1).any(axis=1))
            assert bad.size == 0, (geometry, window, width, ch, [(int(r), int(pos[r])) for r in bad[:8]], float(np.abs(host - dev).max()))
            assert np.isfinite(dev).all() and (dev != -77.0).any()
        assert all(np.array_equal(a, b) for a, b in zip((kq, kd, vq, vd), before))  # the launch only reads the cache


# ---- 2. a Q8_0 session against the oracle and an F16 session, on rows that quantise without loss -----------------------------------------------

class Rig:
    """one geometry's one-layer model (test_attention_geometry_gpu.py's), optionally with attn_k and attn_v zero on the GPU and in the oracle: then a
    pass's own rows are zero and quantise without loss"""

    def __init__(self, gpu, geometry, zero_kv):
        self.gpu, self.geometry = gpu, geometry
        nh, nkv, hd = G.GEOMETRIES[geometry] if isinstance(geometry, str) else geometry   # a name of the table, or (n_head, n_kv_head, head_dim)
        m = G.MODEL
        self.model = gpu.LlmModel(gpu.LlmHParams(m["n_layer"], m["d_model"], nh, nkv, hd, m["d_ff"], m["vocab"], 1e-5, 10000.0, 0, 0, 0, 0, 1)).fill_synthetic(4)
        self.hp = self.model.hparams
        self.zero_kv = zero_kv
        self.zeros = {}
        if zero_kv:
            orc = O.OracleLlm(oracle_cfg_from(self.hp, 8, 1), seed=4)
            for which in (O.L_K, O.L_V):
                t, buf = orc.get_tensor(0, which)
                self.zeros[which] = (t, np.zeros_like(buf))
                self.model.set_tensor(0, which, t, self.zeros[which][1])
            orc.close()
        self.open = []

    def session(self, max_seq, window, kv_type):
        s = self.gpu.LlmSession(self.model, max_seq, window, kv_type=kv_type)
        self.open.append(s)
        return s

    def oracle(self, max_seq, window):
        o = O.OracleLlm(oracle_cfg_from(self.hp, window, max_seq), seed=4)
        for which, (t, z) in self.zeros.items():
            o.set_tensor(0, which, t, z)
        self.open.append(o)
        return o

    def close(self):
        for x in self.open:
            x.close()
        self.model.close()


@pytest.fixture(scope="module", params=list(G.GEOMETRIES))
def zero_rig(request, gpu):
    r = Rig(gpu, request.param, True)
    yield r
    r.close()


def run_lossless_pass(rig, trio, seq, pos, tok, preload, tag):
    """preload {sequence: rows}: lossless rows [0, rows) into all three; the pass; logits as bits and ids of the Q8_0 session = the oracle's = the F16 session's"""
    q8, f16, orc = trio
    hp = rig.hp
    for s, n in preload.items():
        k = R.lossless_rows((n, hp.n_kv_head, hp.head_dim), 2 * s + 1000 * n)
        v = R.lossless_rows((n, hp.n_kv_head, hp.head_dim), 2 * s + 1 + 1000 * n)
        for x in trio:
            x.kv_write(0, s, 0, k, v)
    want, wid = orc.forward(seq, pos, tok)
    got, gid = q8.forward(seq, pos, tok)
    ref, rid = f16.forward(seq, pos, tok)
    assert np.array_equal(bits(got), bits(want)), (tag, "oracle", float(np.abs(got - want).max()))
    assert np.array_equal(bits(got), bits(ref)), (tag, "f16 session", float(np.abs(got - ref).max()))
    assert np.array_equal(gid, wid) and np.array_equal(gid, rid), tag


def test_q8_session_equals_oracle_and_f16_session_on_lossless_rows(zero_rig):
    rig, gpu, hp = zero_rig, zero_rig.gpu, zero_rig.hp
    rng = np.random.default_rng(9)
    for window in (260, 261):
        nseq = 256
        trio = (rig.session(nseq, window, gpu.KV_Q8_0), rig.session(nseq, window, gpu.KV_F16), rig.oracle(nseq, window))
        # decode passes: one row per sequence at the table's context lengths; both windows see narrow and wide passes
        for width in ((1, 16, 129) if window == 260 else (2, 256)):
            assert gpu.attention_plan(width, hp.n_head, hp.n_kv_head, hp.head_dim, window, kv_type=gpu.KV_Q8_0)[0] == 6
            lengths = G.WINDOWS[window]
            pos = np.array([lengths[(r + 3 * width) % len(lengths)] for r in range(width)], np.int32)
            seq = np.arange(width, dtype=np.int32)
            tok = rng.integers(3, hp.vocab, width).astype(np.int32)
            run_lossless_pass(rig, trio, seq, pos, tok, {int(s): int(p) for s, p in zip(seq, pos) if p > 0}, (rig.geometry, window, "decode", width))
        # multi-position passes of the existing generator (several new positions of a sequence in one pass)
        cases = [c for c in G.groups(rig.geometry)["unfused"] if c["start"] in (31, 159)]
        assert len(cases) >= 4
        for case in cases:
            for p in G.passes(case):
                starts = {int(s): int(p["pos"][p["seq"] == s].min()) for s in np.unique(p["seq"])}
                run_lossless_pass(rig, trio, p["seq"], p["pos"], p["tok"], {s: n for s, n in starts.items() if n > 0}, (rig.geometry, window, case["name"]))
        for x in trio:
            x.close()
            rig.open.remove(x)


# ---- 3. the append path: the rows a pass writes are the restatement of the rows an F16 session holds ---------------------------------------------

@pytest.mark.parametrize("geometry", list(G.GEOMETRIES))
def test_appended_rows_are_the_quantised_f16_rows(gpu, geometry):
    rig = Rig(gpu, geometry, False)
    try:
        hp, window, nseq = rig.hp, 64, 6
        q8, f16 = rig.session(nseq, window, gpu.KV_Q8_0), rig.session(nseq, window, gpu.KV_F16)
        rng = np.random.default_rng(21)
        by_k, by_v = R.lossless_rows((window, hp.n_kv_head, hp.head_dim), 1), R.lossless_rows((window, hp.n_kv_head, hp.head_dim), 2)
        for s in (q8, f16):
            s.kv_write(0, 5, 0, by_k, by_v)  # the bystander sequence
        # a decode pass (rows of five sequences at position 0: one layer, so a row depends on its own token and position only), then a multi-position pass
        passes = [(np.arange(5), np.zeros(5, int)), (np.repeat(np.arange(3), 9), np.tile(np.arange(1, 10), 3))]
        for seq, pos in passes:
            seq, pos = seq.astype(np.int32), pos.astype(np.int32)
            tok = rng.integers(3, hp.vocab, seq.size).astype(np.int32)
            q8.forward(seq, pos, tok, want_logits=False)
            f16.forward(seq, pos, tok, want_logits=False)
            for s in np.unique(seq):
                p0, n = int(pos[seq == s].min()), int((seq == s).sum())
                fk, fv = f16.kv_read(0, int(s), p0, n)
                kq, kd, vq, vd = q8.kv_read_q8(0, int(s), p0, n)
                assert fk.any() and fv.any()
                assert not R.inverse_overflows(fk).any() and not R.inverse_overflows(fv).any()
                wk, wkd = R.quantize(fk)
                wv, wvd = R.quantize(fv)
                assert np.array_equal(kq, wk) and np.array_equal(kd, wkd) and np.array_equal(vq, wv) and np.array_equal(vd, wvd), (geometry, int(s), p0, n)
        kq, kd, vq, vd = q8.kv_read_q8(0, 5, 0, window)
        wk, wkd = R.quantize(by_k)
        wv, wvd = R.quantize(by_v)
        assert np.array_equal(kq, wk) and np.array_equal(kd, wkd) and np.array_equal(vq, wv) and np.array_equal(vd, wvd)
        # rows behind the appended ones were never written
        kq, kd, _, _ = q8.kv_read_q8(0, 0, 10, 5)
        assert not kq.any() and not kd.any()
    finally:
        rig.close()


# ---- 4. a row's bits depend neither on its pass nor on its neighbours ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny(gpu):
    model = gpu.LlmModel(gpu.TINY()).fill_synthetic(SEED)
    yield gpu, model
    model.close()


def test_logits_and_cache_rows_do_not_depend_on_the_form_of_the_pass(tiny):
    gpu, model = tiny
    hp = model.hparams
    assert hp.n_layer == 2  # layer-1 rows depend on the Q8_0 attention of layer 0
    n = 40
    tok = np.random.default_rng(40).integers(3, hp.vocab, n).astype(np.int32)
    sess = gpu.LlmSession(model, 4, 48, kv_type=gpu.KV_Q8_0)
    try:
        pos = np.arange(n, dtype=np.int32)

        def run(s, cuts, verify_tail=0):
            out = []
            for a, b in zip(cuts[:-1], cuts[1:]):
                f = sess.forward_verify if (verify_tail and b == n) else sess.forward
                out.append(f(np.full(b - a, s, np.int32), pos[a:b], tok[a:b])[0])
            return np.concatenate(out)

        ways = [run(0, [0, n]), run(1, list(range(0, n, 7)) + [n]), run(2, list(range(n + 1))), run(3, [0, n - 5, n], verify_tail=5)]
        rows = [[sess.kv_read_q8(l, s, 0, n) for l in range(hp.n_layer)] for s in range(4)]
        for s in range(1, 4):
            assert np.array_equal(bits(ways[s]), bits(ways[0])), ("logits", s, float(np.abs(ways[s] - ways[0]).max()))
            for l in range(hp.n_layer):
                assert all(np.array_equal(a, b) for a, b in zip(rows[s][l], rows[0][l])), ("cache rows", s, l)
        assert rows[0][1][0].any() and rows[0][1][1].any()
    finally:
        sess.close()


# ---- 5. the surface -------------------------------------------------------------------------------------------------------------------------------

def test_session_surface(tiny):
    gpu, model = tiny
    hp = model.hparams
    q8, f16 = gpu.LlmSession(model, 3, 600, kv_type=gpu.KV_Q8_0), gpu.LlmSession(model, 3, 600)
    try:
        L = gpu.lib()
        assert L.tk_mi355x_llm_session_kv_type(q8.h) == 1 and L.tk_mi355x_llm_session_kv_type(f16.h) == 0
        assert f16.kv_bytes() == 2 * hp.n_layer * 3 * 600 * hp.n_kv_head * hp.head_dim * 2 and q8.kv_bytes() * 32 == f16.kv_bytes() * 17
        rows = [(R.lossless_rows((600, hp.n_kv_head, hp.head_dim), 10 * l + s), seeded_rows(600, hp.n_kv_head, hp.head_dim, 1.0, 10 * l + s)) for l in range(hp.n_layer) for s in range(3)]
        for l in range(hp.n_layer):
            for s in range(3):
                q8.kv_write(l, s, 0, *rows[3 * l + s])

        def snapshot():
            return [q8.kv_read_q8(l, s, 0, 600) for l in range(hp.n_layer) for s in range(3)]

        before = snapshot()
        for (k, v), (kq, kd, vq, vd) in zip(rows, before):  # kv_write quantised by the one definition
            assert np.array_equal(kq, R.quantize(k)[0]) and np.array_equal(kd, R.quantize(k)[1]) and np.array_equal(vq, R.quantize(v)[0]) and np.array_equal(vd, R.quantize(v)[1])
        # kv_copy: rows [7, 7 + 530) of sequence 0 onto sequence 2, values and scales of both caches, nothing else
        q8.kv_copy(0, 2, 7, 530)
        after = snapshot()
        for l in range(hp.n_layer):
            for i, (a, b0, b2) in enumerate(zip(after[3 * l + 2], before[3 * l], before[3 * l + 2])):
                want = b2.copy()
                want[7:537] = b0[7:537]
                assert np.array_equal(a, want), ("kv_copy", l, i)
            for s in (0, 1):
                assert all(np.array_equal(a, b) for a, b in zip(after[3 * l + s], before[3 * l + s]))
        # refusals, with nothing changed
        seq, pos, tok = np.zeros(3, np.int32), np.arange(520, 523, dtype=np.int32), np.array([5, 6, 7], np.int32)

        def refused(code, words, fn, *a, **kw):
            with pytest.raises(gpu.TkError) as e:
                fn(*a, **kw)
            assert e.value.code == code and words in e.value.detail, (e.value.code, e.value.detail)

        refused(TK_ERROR_INVALID_ARGUMENT, "Q8_0", q8.kv_read, 0, 0, 0, 4)
        refused(TK_ERROR_NOT_IMPLEMENTED, "Q8_0 KV cache", q8.kv_shift, 0, 8, 40, -4)
        refused(TK_ERROR_INVALID_ARGUMENT, "tiled", q8.forward_verify, seq, pos, tok, form=2)
        refused(TK_ERROR_INVALID_ARGUMENT, "run form", q8.forward_verify, seq, pos, tok, form=4)
        refused(TK_ERROR_NOT_IMPLEMENTED, "Q8_0 KV cache", q8.forward_stage, seq[:1], pos[:1], 0, 1, tok=tok[:1], x_out=np.zeros((1, hp.d_model), np.float32))
        refused(TK_ERROR_INVALID_ARGUMENT, "kv_type", gpu.LlmSession, model, 1, 16, kv_type=2)
        with pytest.raises(gpu.TkError):
            f16.kv_read_q8(0, 0, 0, 4)
        assert all(np.array_equal(a, b) for x, y in zip(snapshot(), after) for a, b in zip(x, y))
        # form -1 of a verify pass resolves to the per-row form where an F16 session of this window takes the run form
        assert gpu.attention_plan_verify(3, hp.n_head, hp.n_kv_head, hp.head_dim, 600, 522)[0] == 4
        _, picks = q8.forward_verify(seq, pos, tok, form=-1)
        _, picks0 = q8.forward_verify(seq, pos, tok, form=0)
        assert np.array_equal(picks, picks0)
    finally:
        q8.close()
        f16.close()


# ---- 6. runners on a Q8_0 model -------------------------------------------------------------------------------------------------------------------

class Handle:
    def __init__(self, gpu, kv=None, prefix_cache=False):
        self.gpu, self.loader = gpu, gpu.ModelLoader()
        self.h = self.loader.load(PATH, force_reload=True)
        if kv is not None:
            gpu.ModelLoader.set_kv_cache_type(self.h, kv)
        if prefix_cache:
            gpu.ModelLoader.set_prefix_cache(self.h, True)
        self.runners = []

    def runner(self, ctx=256):
        r = self.gpu.LlmRunner(self.h, context_size=ctx)
        self.runners.append(r)
        return r

    def close(self):
        for r in self.runners:
            r.close()
        self.loader.unload(self.h)
        self.loader.close()


def generate(runner, prompt, cap=48):
    runner.prepare(prompt)
    pieces = []
    for _ in range(cap):
        p = runner.next_token()
        if p is None or p == "<tool_call>":
            break
        pieces.append(p)
    return pieces, runner.recent_tokens()


def test_runners_on_a_q8_model(tiny):
    gpu, model = tiny
    prompt = "the quick brown fox jumps over"
    ids = [1] + [3 + b for b in prompt.encode()]
    h = Handle(gpu, kv="q8_0")
    try:
        r = h.runner()
        pieces, got = generate(r, prompt)
        assert len(got) >= 8
        # a bare Q8_0 session driven row by row gives the same greedy ids
        sess = gpu.LlmSession(model, 1, 256, kv_type=gpu.KV_Q8_0)
        try:
            cur = None
            for p, t in enumerate(ids):
                _, cur = sess.forward([0], [p], [t], want_logits=False)
            want = []
            for i in range(len(got)):
                want.append(int(cur[0]))
                _, cur = sess.forward([0], [len(ids) + i], [want[-1]], want_logits=False)
        finally:
            sess.close()
        assert got == want
        # lookup decoding on: the same tokens, and drafts were verified (several positions of the sequence in one pass over the Q8_0 cache)
        r.set_lookup(4, 1, 3)
        r.set_prediction(got)
        assert generate(r, prompt) == (pieces, got)
        assert r.lookup_stats()[2] >= 4
        # context shift is refused; the setter is refused once a runner exists, by number and by name; an unknown name is refused by name
        with pytest.raises(gpu.TkError) as e:
            r.set_context_shift(True)
        assert e.value.code == TK_ERROR_NOT_IMPLEMENTED and "Q8_0 KV cache" in e.value.detail
        r.set_context_shift(False)
        for kv in (gpu.KV_F16, "f16"):
            with pytest.raises(gpu.TkError) as e:
                gpu.ModelLoader.set_kv_cache_type(h.h, kv)
            assert e.value.code == TK_ERROR_INVALID_ARGUMENT and "before the first" in e.value.detail
        with pytest.raises(gpu.TkError) as e:
            gpu.ModelLoader.set_kv_cache_type(h.h, "q4_0")
        assert "q4_0" in e.value.detail
    finally:
        h.close()
    # prefix cache on: the same tokens, and the copied-row counter moves
    h = Handle(gpu, kv=gpu.KV_Q8_0, prefix_cache=True)
    try:
        assert generate(h.runner(), prompt) == (pieces, got)
        b = h.runner()
        assert generate(b, prompt) == (pieces, got)
        rows, kept, copied = b.last_prompt_rows()
        assert rows == len(ids) and copied >= 16
        assert gpu.ModelLoader.prefix_cache_stats(h.h)[2] >= copied
    finally:
        h.close()
    # a model left at the default gives the tokens an F16 session gives
    h = Handle(gpu)
    try:
        _, plain = generate(h.runner(), prompt)
    finally:
        h.close()
    sess = gpu.LlmSession(model, 1, 256)
    try:
        cur = None
        for p, t in enumerate(ids):
            _, cur = sess.forward([0], [p], [t], want_logits=False)
        want = []
        for i in range(len(plain)):
            want.append(int(cur[0]))
            _, cur = sess.forward([0], [len(ids) + i], [want[-1]], want_logits=False)
    finally:
        sess.close()
    assert plain == want
