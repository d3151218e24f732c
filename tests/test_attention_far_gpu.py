"""k_attention_far — the per-row attention of a session whose window has no room in LDS for a score row — and the other attention forms in
windows beyond the resident form's limit, against the oracle and BIT FOR BIT, on the rig of test_attention_geometry_gpu.py (a one-layer synthetic
model, kv_write on the session and the oracle alike, forward).

  - beside the resident form: TK_MI355X_ATT_RESIDENT_MAX=64 sends every geometry of attention_geometry_cases.py through the far kernel in windows
    of 260 and 261 positions, decode passes of 1 .. 256 rows and multi-position passes; a session without the knob runs the same passes;
  - beyond the limit: group 4 x 256 in a window of 6144 and 32 / 8 / 128 in one of 8448, sessions that could not be created before;
  - the long-context form, its run variant and the tiled prefill with the top position above 8192;
  - a cache of more than 2^31 elements; a runner with a 12 288-position context.

Per pass: logits as uint32, ids, the cache rows the pass may touch and a bystander sequence."""
import functools

import numpy as np
import pytest

import attention_geometry_cases as G
import oracle_lib as O
from gguf_util import write_llama_gguf
from test_llm_gpu import oracle_cfg_from

pytestmark = pytest.mark.gpu

KNOB = "TK_MI355X_ATT_RESIDENT_MAX"
FAR = 5
SMALL_WINDOWS = (260, G.ODD_WINDOW)
SMALL_WIDTHS = (1, 2, 16, 129, 256)
POOL = 1031


def make_model(gpu, nh, nkv, hd):
    m = G.MODEL
    return gpu.LlmModel(gpu.LlmHParams(m["n_layer"], m["d_model"], nh, nkv, hd, m["d_ff"], m["vocab"], 1e-5, 10000.0, 0, 0, 0, 0, 1)).fill_synthetic(4)


@functools.lru_cache(maxsize=None)
def pool(nkv, hd):
    rng = np.random.default_rng([29, nkv, hd])
    k = (rng.standard_normal((POOL, nkv, hd), dtype=np.float32) * np.float32(G.K_SCALE)).astype(np.float16).view(np.uint16)
    v = (rng.standard_normal((POOL, nkv, hd), dtype=np.float32) * np.float32(G.V_SCALE)).astype(np.float16).view(np.uint16)
    return k, v


def pool_rows(nkv, hd, offset, n):
    """rows offset .. offset + n - 1 (mod POOL) of a seeded pool of f16 key and value rows [n][n_kv_head][head_dim]"""
    k, v = pool(nkv, hd)
    idx = (offset + np.arange(n)) % POOL
    return k[idx], v[idx]


def same_bits(got, want, what):
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    assert bad.size == 0, (what, bad[:8].tolist(), float(np.abs(got - want).max()))


def check_cache(sess, orc, seq, n, what):
    gk, gv = sess.kv_read(0, seq, 0, n)
    wk, wv = orc.kv_read(0, seq, 0, n)
    assert np.array_equal(gk, wk) and np.array_equal(gv, wv), what


# ---------------------------------------------------------------------------------------------------------------------------------------
# the far form beside the resident one, small windows
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=list(G.GEOMETRIES))
def small(request, gpu):
    nh, nkv, hd = G.GEOMETRIES[request.param]
    model = make_model(gpu, nh, nkv, hd)
    made = []

    def session(max_seq, window):
        made.append(gpu.LlmSession(model, max_seq, window))
        return made[-1]

    def oracle(max_seq, window):
        made.append(O.OracleLlm(oracle_cfg_from(model.hparams, window, max_seq), seed=4))
        return made[-1]

    yield request.param, model, session, oracle
    for x in made:
        x.close()
    model.close()


def run_beside(gpu, geometry, model, far, res, orc, case, env, monkeypatch):
    """every pass of a case: in the session that takes the far form (under `env`), in the one that does not, and on the oracle"""
    hp = model.hparams
    window = case["window"]
    kernels = set()
    for p in G.passes(case):
        by = p["bystander"]
        bk, bv = G.kv_rows(geometry, 11 * by + 5, window)
        for s in (far, res):
            s.kv_write(0, by, 0, bk, bv)
        for sq, (off, n) in p["preload"].items():
            k, v = G.kv_rows(geometry, off, n)
            for s in (far, res, orc):
                s.kv_write(0, sq, 0, k, v)
        want, wam = orc.forward(p["seq"], p["pos"], p["tok"])
        with monkeypatch.context() as mp:
            for name, value in env.items():
                mp.setenv(name, value)
            plan = gpu.attention_plan(p["seq"].size, hp.n_head, hp.n_kv_head, hp.head_dim, window, case["fused"], top_position=p["top"])
            assert plan[0] == FAR and plan[3] == 2 and plan[2] in (32, 64), (case["name"], plan)
            kernels.add(plan[1:3])
            got, gam = far.forward(p["seq"], p["pos"], p["tok"])
        with monkeypatch.context() as mp:
            for name, value in env.items():
                if name != KNOB:
                    mp.setenv(name, value)
            assert gpu.attention_plan(p["seq"].size, hp.n_head, hp.n_kv_head, hp.head_dim, window, case["fused"], top_position=p["top"])[0] in (0, 1)
            rgot, ram = res.forward(p["seq"], p["pos"], p["tok"])
        same_bits(got, want, (case["name"], "far form against the oracle"))
        same_bits(rgot, got, (case["name"], "resident form against the far form"))
        assert np.array_equal(gam, wam) and np.array_equal(ram, wam), case["name"]
        for sq, (off, n) in p["preload"].items():
            for s in (far, res):
                check_cache(s, orc, sq, n, (case["name"], sq, n))
        for s in (far, res):
            gk, gv = s.kv_read(0, by, 0, window)
            assert np.array_equal(gk, bk) and np.array_equal(gv, bv), (case["name"], "bystander", by)
    return kernels


@pytest.mark.parametrize("window", SMALL_WINDOWS)
def test_far_form_beside_the_resident_form_decode(small, gpu, window, monkeypatch):
    """1, 2, 16, 129 and 256 rows, one per sequence, at 0, 1, 31 .. 33, 63 .. 65, 127 .. 129, 190 .. 193, 255 .. 257 and the window's last position"""
    geometry, model, session, oracle = small
    with monkeypatch.context() as mp:   # the far session's launches are described (and recorded) under the knob
        mp.setenv(KNOB, "64")
        far = session(G.DECODE_SEQS, window)
    res, orc = session(G.DECODE_SEQS, window), oracle(G.DECODE_SEQS, window)
    seen = set()
    for width in SMALL_WIDTHS:
        case = G._case(geometry, "decode_w%d" % window, "far_w%d_rows%d" % (window, width), window, None, width=width)
        seen |= run_beside(gpu, geometry, model, far, res, orc, case, {KNOB: "64"}, monkeypatch)
    if gpu.lib().tk_mi355x_device_cu_count(0) == 256:   # 256 rows x n_kv_head workgroups: 32-position slots where that is more than 4 x 256
        assert {c for _, c in seen} == ({32, 64} if G.GEOMETRIES[geometry][1] > 4 else {64}), seen


def test_far_form_beside_the_resident_form_multi_position(small, gpu, monkeypatch):
    """several new positions of each sequence in one pass, from 0, 31, 97 and 159 cached positions, under TK_MI355X_NO_PREFILL_ATT=1 so that they
    reach the per-row form: k_qkv_rope_append, then k_attention_far"""
    geometry, model, session, oracle = small
    env = {KNOB: "64", "TK_MI355X_NO_PREFILL_ATT": "1"}
    far, res, orc = session(16, 260), session(16, 260), oracle(16, 260)
    n = 0
    for start in G.UNFUSED_STARTS:
        for shape in G.UNFUSED_PLAN[geometry]:
            case = G._case(geometry, "unfused", "far_from%d_%dx%d" % (start, shape[0], shape[1]), 260, None, fused=False, shape=shape, start=start)
            run_beside(gpu, geometry, model, far, res, orc, case, env, monkeypatch)
            n += 1
    assert n == 12


# ---------------------------------------------------------------------------------------------------------------------------------------
# beyond the resident form's limit
# ---------------------------------------------------------------------------------------------------------------------------------------
class Deep:
    """one geometry in one window beyond its limit: the model, a session of 17 sequences and its oracle"""
    SEQS = 17

    def __init__(self, gpu, nh, nkv, hd, window, env=None):
        self.gpu, self.window, self.geom = gpu, window, (nh, nkv, hd)
        self.limit = gpu.attention_resident_limit(nh, nkv, hd)
        assert self.limit < window
        self.model = make_model(gpu, nh, nkv, hd)
        self.sess = gpu.LlmSession(self.model, self.SEQS, window)   # refused before the far form existed
        self.orc = O.OracleLlm(oracle_cfg_from(self.model.hparams, window, self.SEQS), seed=4)
        self.loaded = {}
        self.salt = 0

    def load(self, seq, n):
        """the first n positions of a sequence from the pool (an offset of its own per call), on the session and the oracle"""
        self.salt += 1
        k, v = pool_rows(self.geom[1], self.geom[2], 53 * seq + 7 * self.salt, n)
        self.sess.kv_write(0, seq, 0, k, v)
        self.orc.kv_write(0, seq, 0, k, v)
        return k, v

    def plan(self, rows, top, fused=True):
        nh, nkv, hd = self.geom
        return self.gpu.attention_plan(rows, nh, nkv, hd, self.window, fused, top_position=top)

    def plan_verify(self, rows, top):
        nh, nkv, hd = self.geom
        return self.gpu.attention_plan_verify(rows, nh, nkv, hd, self.window, top)

    def decode_pass(self, pos, want_kernel, what):
        """row i = sequence i at pos[i]; the sequence behind the last one is the bystander"""
        pos = np.asarray(pos, np.int32)
        n = pos.size
        seq = np.arange(n, dtype=np.int32)
        tok = np.random.default_rng([n, int(pos[0])]).integers(3, G.MODEL["vocab"], n).astype(np.int32)
        kept = {}
        for s in range(n):
            kept[s] = self.load(s, min(int(pos[s]) + 2, self.window))
        self.salt += 1
        bk, bv = pool_rows(self.geom[1], self.geom[2], 11 * n + self.salt, self.window)
        self.sess.kv_write(0, n, 0, bk, bv)
        assert self.plan(n, int(pos.max()))[0] == want_kernel, (what, self.plan(n, int(pos.max())))
        want, wam = self.orc.forward(seq, pos, tok)
        got, gam = self.sess.forward(seq, pos, tok)
        same_bits(got, want, what)
        assert np.array_equal(gam, wam), what
        for s in range(n):
            m = min(int(pos[s]) + 2, self.window)
            check_cache(self.sess, self.orc, s, m, (what, s))
            if pos[s] + 1 < m:   # the row behind the appended one is still the loaded one
                gk, gv = self.sess.kv_read(0, s, int(pos[s]) + 1, 1)
                assert np.array_equal(gk[0], kept[s][0][pos[s] + 1]) and np.array_equal(gv[0], kept[s][1][pos[s] + 1]), (what, s)
        gk, gv = self.sess.kv_read(0, n, 0, self.window)
        assert np.array_equal(gk, bk) and np.array_equal(gv, bv), (what, "bystander")

    def chunk_pass(self, rows, top, want_kernel, what, verify_form=None):
        """`rows` consecutive positions of sequence 0 ending at `top`, as a prompt chunk (forward) or a verify pass of the given form"""
        pos = np.arange(top - rows + 1, top + 1, dtype=np.int32)
        seq = np.zeros(rows, np.int32)
        tok = np.random.default_rng([rows, top]).integers(3, G.MODEL["vocab"], rows).astype(np.int32)
        self.load(0, min(top + 2, self.window))
        self.salt += 1
        bk, bv = pool_rows(self.geom[1], self.geom[2], 5 + self.salt, self.window)
        self.sess.kv_write(0, 1, 0, bk, bv)
        want, wam = self.orc.forward(seq, pos, tok)
        if verify_form is None:
            assert self.plan(rows, top, fused=False)[0] == want_kernel, (what, self.plan(rows, top, fused=False))
            got, gam = self.sess.forward(seq, pos, tok)
        else:
            assert self.plan_verify(rows, top)[0] == want_kernel, (what, self.plan_verify(rows, top))
            got, gam = self.sess.forward_verify(seq, pos, tok, form=verify_form)
        same_bits(got, want, what)
        assert np.array_equal(gam, wam), what
        check_cache(self.sess, self.orc, 0, min(top + 2, self.window), what)
        gk, gv = self.sess.kv_read(0, 1, 0, self.window)
        assert np.array_equal(gk, bk) and np.array_equal(gv, bv), (what, "bystander")

    def close(self):
        self.sess.close()
        self.orc.close()
        self.model.close()


def edge_positions(limit, window, rows):
    """limit - 1, limit, limit + 1 and the window's last position first, then contexts short and long"""
    more = [0, 1, 63, 64, 65, 4095, limit // 2, 127, 128, 129, 2047, window - 2]
    return ([limit - 1, limit, limit + 1, window - 1] + more)[:rows] if rows > 1 else [window - 1]


@pytest.fixture(scope="module")
def deep_g4_d256(gpu):
    d = Deep(gpu, 24, 6, 256, 6144)
    yield d
    d.close()


@pytest.fixture(scope="module")
def deep_mistral(gpu):
    d = Deep(gpu, 32, 8, 128, 8448)
    yield d
    d.close()


@pytest.fixture(scope="module")
def deep_g4_d64(gpu):
    d = Deep(gpu, 32, 8, 64, 9472)
    yield d
    d.close()


def test_group_4x256_in_a_window_of_6144(deep_g4_d256):
    """the smallest limit class (5856): the far form at 1, 9 and 16 rows (the long-context form does not take head_dim 256), rows at limit - 1,
    limit, limit + 1 and the window's last position; a 16-position chunk ending at the window's last position takes the far form per row"""
    d = deep_g4_d256
    assert d.limit == 5856
    for rows in (1, 9, 16):
        for turn in range(4 if rows == 1 else 1):   # one row: each of the four edge positions in turn
            pos = [[d.limit - 1, d.limit, d.limit + 1, d.window - 1][turn]] if rows == 1 else edge_positions(d.limit, d.window, rows)
            d.decode_pass(pos, FAR, ("g4_d256", rows, pos[0]))
    d.chunk_pass(16, d.window - 1, FAR, "g4_d256 chunk of 16")


def test_mistral_geometry_in_a_window_of_8448(deep_mistral, gpu, monkeypatch):
    """32 / 8 / 128 beyond 8192: 9 and 16 rows take the far form, one row the long-context form — and the far form under TK_MI355X_NO_LONG_ATT=1, in
    a session of its own; a 16-position chunk ending at the window's last position is tiled"""
    d = deep_mistral
    assert d.limit == 8192
    for rows in (9, 16):
        pos = edge_positions(d.limit, d.window, rows)
        d.decode_pass(pos, FAR, ("mistral", rows))
    d.decode_pass([d.window - 1], 3, ("mistral", 1, "long-context form"))
    d.chunk_pass(16, d.window - 1, 2, "mistral chunk of 16")
    monkeypatch.setenv("TK_MI355X_NO_LONG_ATT", "1")
    sess = gpu.LlmSession(d.model, d.SEQS, d.window)
    kept, d.sess = d.sess, sess
    try:
        for p in (d.limit - 1, d.limit, d.limit + 1, d.window - 1):
            d.decode_pass([p], FAR, ("mistral", 1, p))
    finally:
        d.sess = kept
        sess.close()


@pytest.mark.parametrize("which", ["mistral_8448", "g4_d64_9472"])
def test_forms_never_run_this_deep(which, request):
    """the long-context form at 1, 4, 5 and 8 rows, its run variant through forward_verify (form 4, 5 rows) and the tiled prefill (form 2, 16 rows),
    all with the top position above 8192"""
    d = request.getfixturevalue("deep_mistral" if which == "mistral_8448" else "deep_g4_d64")
    top = d.window - 1
    assert top > 8192 and d.limit < d.window
    for rows in (1, 4, 5, 8):
        pos = [top] + [top - delta for delta in (1, 63, 64, 65, 200, 300, 8000)[:rows - 1]]
        d.decode_pass(pos, 3, (which, "long", rows))
    d.chunk_pass(5, top, 4, (which, "run form"), verify_form=4)
    d.chunk_pass(5, 8300, 4, (which, "run form at 8300"), verify_form=-1)
    d.chunk_pass(16, top, 2, (which, "tiled, verify form 2"), verify_form=2)
    d.chunk_pass(16, top - 3, 2, (which, "tiled, prompt chunk"))


# ---------------------------------------------------------------------------------------------------------------------------------------
# a cache above 2^31 elements
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_cache_above_2_to_31_elements(gpu):
    """1 layer, 8 KV heads x 128, window 32 768, 65 sequences: 65 x 8 x 32768 x 128 = 2^31 + 2^25 elements per cache.  Sequences 0 and 64 hold the
    same rows in their top 300 positions; one row of each at position 32 767 in one pass gives the same logits, those of a one-sequence oracle"""
    W, NSEQ, TOPN = 32768, 65, 300
    nh, nkv, hd = 32, 8, 128
    assert NSEQ * nkv * W * hd > 2 ** 31
    model = make_model(gpu, nh, nkv, hd)
    sess = gpu.LlmSession(model, NSEQ, W)
    orc = O.OracleLlm(oracle_cfg_from(model.hparams, W, 1), seed=4)
    try:
        k, v = pool_rows(nkv, hd, 77, TOPN)
        p0 = W - TOPN
        for s in (0, 64):
            sess.kv_write(0, s, p0, k, v)
        tok = np.array([41, 41], np.int32)

        def oracle_row():
            orc.reset()
            orc.kv_write(0, 0, p0, k, v)
            return orc.forward([0], [W - 1], tok[:1])

        want, wam = oracle_row()
        wk, wv = orc.kv_read(0, 0, p0, TOPN)
        assert np.array_equal(wk[:-1], k[:-1]) and not np.array_equal(wk[-1], k[-1])
        # two rows: the long-context form
        assert gpu.attention_plan(2, nh, nkv, hd, W, True, top_position=W - 1)[0] == 3
        got, gam = sess.forward([0, 64], [W - 1, W - 1], tok)
        same_bits(got[:1], want, "sequence 0, two rows")
        same_bits(got[1:], want, "sequence 64, two rows")
        assert gam[0] == wam[0] and gam[1] == wam[0]
        for s in (0, 64):
            gk, gv = sess.kv_read(0, s, p0, TOPN)
            assert np.array_equal(gk, wk) and np.array_equal(gv, wv), s
        # nine rows — short bystanders in between — take the far form
        for s in (0, 64):
            sess.kv_write(0, s, p0, k, v)
        seq = np.array([0, 1, 2, 3, 4, 5, 6, 7, 64], np.int32)
        pos = np.array([W - 1, 0, 1, 2, 3, 4, 5, 6, W - 1], np.int32)
        assert gpu.attention_plan(9, nh, nkv, hd, W, True, top_position=W - 1)[0] == FAR
        got, gam = sess.forward(seq, pos, np.full(9, 41, np.int32))
        same_bits(got[:1], want, "sequence 0, nine rows")
        same_bits(got[8:], want, "sequence 64, nine rows")
        gk, gv = sess.kv_read(0, 64, p0, TOPN)
        assert np.array_equal(gk, wk) and np.array_equal(gv, wv)
        # sequence 63, next to it, is untouched: never written, all zero
        for q0, n in ((0, 64), (W - TOPN, TOPN)):
            zk, zv = sess.kv_read(0, 63, q0, n)
            assert not zk.any() and not zv.any()
        # a prefix-cache copy from sequence 64 to 1 near the top: a bit copy of those rows, nothing else of sequence 1
        before_k, before_v = sess.kv_read(0, 1, W - 2 * TOPN, TOPN)
        sess.kv_copy(64, 1, p0, TOPN)
        ck, cv = sess.kv_read(0, 1, p0, TOPN)
        assert np.array_equal(ck, wk) and np.array_equal(cv, wv)
        ak, av = sess.kv_read(0, 1, W - 2 * TOPN, TOPN)
        assert np.array_equal(ak, before_k) and np.array_equal(av, before_v)
        # a context shift of sequence 64 by -128 near the top: what the same move gives on a cache of one sequence (kv_shift_probe), where the
        # flat index stays far below 2^31
        half = hd // 2
        theta = np.power(10000.0, -2.0 * np.arange(half) / hd)
        ang = np.arange(W, dtype=np.float64)[:, None] * theta[None, :]
        kc = np.zeros((1, 1, nkv, W, hd), np.uint16)
        vc = np.zeros_like(kc)
        kc[0, 0, :, p0:] = wk.transpose(1, 0, 2)
        vc[0, 0, :, p0:] = wv.transpose(1, 0, 2)
        cs, sn = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
        import math
        cs[128] = [math.cos(128.0 * t) for t in theta]   # the row the move rotates by, from the C library the session's table comes from
        sn[128] = [math.sin(128.0 * t) for t in theta]
        ek, ev = gpu.kv_shift_probe(kc, vc, cs, sn, 0, p0, W, -128, device=-1)   # the per-row function in a host loop
        sess.kv_shift(64, p0, W, -128)
        sk, sv = sess.kv_read(0, 64, p0 - 128, TOPN + 128)
        assert np.array_equal(sk, ek[0, 0, :, p0 - 128:].transpose(1, 0, 2)) and np.array_equal(sv, ev[0, 0, :, p0 - 128:].transpose(1, 0, 2))
        zk, zv = sess.kv_read(0, 63, W - TOPN, TOPN)
        assert not zk.any() and not zv.any()
    finally:
        sess.close()
        orc.close()
        model.close()


def test_a_window_above_32768_is_refused_with_a_message_that_says_so(gpu):
    model = make_model(gpu, 16, 8, 128)
    try:
        with pytest.raises(gpu.TkError) as e:
            gpu.LlmSession(model, 1, 32769)
        assert "32768" in str(e.value)
    finally:
        model.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# runner
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_runner_with_a_context_of_12288(gpu, tmp_path):
    """a tiny GGUF (32 / 8 / 128: the limit is 8192): a runner with context_size 12 288 is created, and a 64-token prompt plus 32 tokens gives the ids
    a context_size 4096 runner gives; with context shift off, generation ends at the window's end"""
    CTX = 12288
    cfg = O.tiny_config()
    orc = O.OracleLlm(cfg, seed=4)
    path = str(tmp_path / "tiny.gguf")
    write_llama_gguf(path, orc, cfg)
    orc.close()
    loader = gpu.ModelLoader()
    h = loader.load(path)
    runners = []
    try:
        hp = gpu.LlmHParams()
        gpu.lib().tk_mi355x_llm_model_get_hparams(h, __import__("ctypes").byref(hp))
        assert gpu.attention_resident_limit(hp.n_head, hp.n_kv_head, hp.head_dim) < CTX
        gpu.ModelLoader.set_runner_slots(h, 2)
        prompt = " ".join(["hello world"] * 32)   # llama SPM: bos and 32 x ("▁hello", "▁world")
        pieces = {}
        for ctx in (CTX, 4096):
            r = gpu.LlmRunner(h, context_size=ctx)
            runners.append(r)
            r.set_logit_bias([2], [-np.inf])      # no EOS: the stream has its 32 tokens
            r.prepare(prompt)
            assert r.last_prompt_rows()[0] == 65
            pieces[ctx] = [r.next_token() for _ in range(32)]
            assert None not in pieces[ctx]
        assert pieces[CTX] == pieces[4096]
        # context shift is off by default: a prompt that leaves 100 positions free, and the generation ends at the window's end
        r = runners[0]
        r.prepare(" ".join(["hello world"] * ((CTX - 101) // 2)))
        n_prompt = r.last_prompt_rows()[0]
        assert n_prompt == CTX - 101
        n = 0
        while r.next_token() is not None:
            n += 1
            assert n <= 101
        assert n == CTX - n_prompt - 1 and r.context_shifts()[0] == 0
    finally:
        for r in runners:
            r.close()
        loader.unload(h)
        loader.close()
