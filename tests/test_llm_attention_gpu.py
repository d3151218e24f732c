"""GPU parity of the attention instantiations the BASELINE configs actually run (VERDICT r02 "weak" 1-2, r04 "weak" 2): head_dim 128, 32 query /
8 KV heads — the Mistral-7B geometry — at context lengths that wrap the two-slot LDS-DMA ring, cross chunk boundaries and use the swizzled key
rows past slot 0, against the oracle, logits BIT FOR BIT.  Which kernel a pass takes is the LAUNCHER's answer (tk_mi355x_attention_plan), not a
copy of its rule; on an MI355X (256 CUs):

  1, 2, 16 rows   k_attention_narrow                  (one runner; the north-star point's decode passes: <= one workgroup per CU)
  32 rows         k_attention<2, fused, 128, 64>   (17 .. 63-row passes)
  64 rows         k_attention<4, fused, 128, 64>
  256 rows        k_attention<4, fused, 128, 32>   (the headline bench's decode passes)
  256 rows        k_attention<4, not fused, 128, 32>  (prefill-shaped: several positions of one sequence in a pass, k_qkv_rope_append first)

and, with the reference's context window (n_ctx 4096, /root/reference/src/ai_models/tk_runner_lifecycle.c:48; a 2048-token prompt budget,
/root/reference/src/cortex/tk_cortex_main.c:1334), decode steps and a prefill chunk at 2047 .. 4000 cached positions.

One decode step per context length is enough because both sides load the same seeded f16 K / V rows first (tk_mi355x_llm_session_kv_write,
orc_llm_kv_write): what `llama_decode` does over a filled KV cache (/root/reference/src/ai_models/tk_runner_streaming.c:34,77).
Plus BASELINE configs[1] whole: the full 32-layer 7B model, 64-token prompt + 128 greedy tokens, ids against the oracle."""
import numpy as np
import pytest

import oracle_lib as O
from test_llm_gpu import oracle_cfg_from

pytestmark = pytest.mark.gpu

MAX_CTX = 192
CTXS = [31, 32, 33, 63, 64, 65, 127, 128, 191]


@pytest.fixture(autouse=True)
def narrow_attention_even_when_sessions_share_the_device(monkeypatch):
    """two module-scoped sessions of this file are alive at once; with more than one decode session on a device the launcher prefers the ring
    form (it shares a CU with other streams' launches: test_narrow_attention_yields_when_sessions_share_the_device).  This file is about the
    instantiations a LONE runner takes, so the narrow form is asked for explicitly."""
    monkeypatch.setenv("TK_MI355X_NO_NARROW_ATT", "0")


def f16_bits(rng, shape, scale):
    return (rng.standard_normal(shape, dtype=np.float32) * scale).astype(np.float16).view(np.uint16)


@pytest.fixture(scope="module")
def mistral1(gpu):
    """one Mistral-7B-shaped layer (4096 / 14336 / 32000, 32q / 8kv x 128, production K-split plan) on both sides, 256 sequences"""
    hp = gpu.MISTRAL_7B()
    hp.n_layer = 1
    model = gpu.LlmModel(hp).fill_synthetic(4)
    hp = model.hparams
    assert (hp.n_head, hp.n_kv_head, hp.head_dim) == (32, 8, 128)
    sess = gpu.LlmSession(model, 256, MAX_CTX)
    orc = O.OracleLlm(oracle_cfg_from(hp, MAX_CTX, 256), seed=4)
    yield gpu, model, sess, orc, hp
    sess.close()
    model.close()
    orc.close()


def load_kv(sess, orc, hp, rng, seqs, ctx):
    """the same random K / V rows for positions [0, ctx) of every sequence in `seqs`, product and oracle alike.  Keys are scaled so that
    the scores spread over several units (a softmax that is neither flat nor one-hot)."""
    for s in seqs:
        k = f16_bits(rng, (ctx, hp.n_kv_head, hp.head_dim), 0.6)
        v = f16_bits(rng, (ctx, hp.n_kv_head, hp.head_dim), 1.0)
        sess.kv_write(0, int(s), 0, k, v)
        orc.kv_write(0, int(s), 0, k, v)


# nrows -> the instantiation an MI355X (256 CUs) runs, as (kernel, gq, chunk, slots); chunk None = whatever fits the window
EXPECTED_PLAN = {1: (1, 2, None, 1), 2: (1, 2, None, 1), 16: (1, 2, None, 1), 32: (0, 2, 64, 2), 64: (0, 4, 64, 2), 256: (0, 4, 32, 2)}


def check_plan(gpu, hp, nrows, max_ctx, fused=True):
    """the launcher's own choice; on a 256-CU device it must be the instantiation this file says it covers"""
    plan = gpu.attention_plan(nrows, hp.n_head, hp.n_kv_head, hp.head_dim, max_ctx, fused)
    ncu = gpu.lib().tk_mi355x_device_cu_count(0)
    if ncu == 256 and fused:
        want = EXPECTED_PLAN[nrows]
        assert plan[:2] == want[:2] and plan[3] == want[3] and (want[2] is None or plan[2] == want[2]), (nrows, plan, want)
    return plan


def decode_step_case(gpu, sess, orc, hp, nrows, ctx, max_ctx, seed):
    rng = np.random.default_rng(seed)
    seq = np.arange(nrows, dtype=np.int32)
    load_kv(sess, orc, hp, rng, seq, ctx)
    pos = np.full(nrows, ctx, np.int32)
    tok = rng.integers(3, hp.vocab, nrows).astype(np.int32)
    want, wam = orc.forward(seq, pos, tok)
    got, gam = sess.forward(seq, pos, tok)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (nrows, ctx, np.abs(got - want).max())
    assert np.array_equal(gam, wam)
    for s in sorted({0, nrows // 2, nrows - 1}):  # the fused prologue appended this row's own K / V at position ctx
        gk, gv = sess.kv_read(0, s, ctx, 1)
        wk, wv = orc.kv_read(0, s, ctx, 1)
        assert np.array_equal(gk, wk) and np.array_equal(gv, wv)
    # the cache rows loaded through the hook read back unchanged (the hook itself is honest)
    gk, _ = sess.kv_read(0, nrows - 1, 0, ctx)
    wk, _ = orc.kv_read(0, nrows - 1, 0, ctx)
    assert np.array_equal(gk, wk)


@pytest.mark.parametrize("ctx", CTXS)
@pytest.mark.parametrize("nrows", [1, 2, 16, 32, 64, 256])
def test_decode_attention_at_mistral_geometry_bit_exact(mistral1, nrows, ctx):
    """one decode row per sequence at position `ctx` over `ctx` cached positions, every pass width class of EXPECTED_PLAN (asserted from the
    launcher's answer).  Logits, ids and the appended K / V row equal the oracle's."""
    gpu, model, sess, orc, hp = mistral1
    check_plan(gpu, hp, nrows, MAX_CTX)
    decode_step_case(gpu, sess, orc, hp, nrows, ctx, MAX_CTX, 1000 * nrows + ctx)


LONG_CTX = 4096  # the reference's window (tk_runner_lifecycle.c:48)


@pytest.fixture(scope="module")
def mistral_long(gpu):
    """one Mistral-7B-shaped layer with the reference's 4096-position window, 32 sequences"""
    hp = gpu.MISTRAL_7B()
    hp.n_layer = 1
    model = gpu.LlmModel(hp).fill_synthetic(4)
    hp = model.hparams
    sess = gpu.LlmSession(model, 32, LONG_CTX)
    orc = O.OracleLlm(oracle_cfg_from(hp, LONG_CTX, 32), seed=4)
    yield gpu, model, sess, orc, hp
    sess.close()
    model.close()
    orc.close()


@pytest.mark.parametrize("nrows,ctx", [(1, 2048), (16, 2047), (16, 2100), (16, 4000), (32, 2048), (32, 3001), (1, 512), (2, 777), (1, 4094), (4, 2049), (3, 511),
                                       (8, 768), (8, 3001), (5, 767), (1, 447)])
def test_decode_attention_past_2048_cached_positions(mistral_long, nrows, ctx, monkeypatch):
    """a decode step over 447 .. 4094 cached positions inside a 4096-position window, both ways.  The session's choice — 1 .. 4 rows from
    position 512, 5 .. 8 rows from 768 — is the long-context form (kernel 3: q / k / v finishing + scores over (row, KV head,
    64-position block) workgroups, one PV chain per (row, head, class) wave, join).  Wider passes, and every pass under TK_MI355X_NO_LONG_ATT=1 (a fresh session:
    passes are captured per session), run the fused kernels: the narrow kernel walks the context chunk by chunk (its resident chunk is ~220
    positions at this window: up to eighteen chunks), the ring kernel wraps its two slots 30 to 60 times.  All equal the oracle bit for bit."""
    gpu, model, sess, orc, hp = mistral_long
    long_form = nrows <= 8 and ctx >= (768 if nrows > 4 else 512)
    assert (gpu.attention_plan(nrows, hp.n_head, hp.n_kv_head, hp.head_dim, LONG_CTX, True, top_position=ctx)[0] == 3) == long_form
    assert gpu.attention_plan(nrows, hp.n_head, hp.n_kv_head, hp.head_dim, LONG_CTX, True, top_position=511)[0] != 3
    decode_step_case(gpu, sess, orc, hp, nrows, ctx, LONG_CTX, 7000 * nrows + ctx)
    if not long_form or (ctx % 2 == 0 and ctx != 2048):
        return                                                       # the fused kernels' share: wide passes, the odd contexts and the 2048 cases
    monkeypatch.setenv("TK_MI355X_NO_LONG_ATT", "1")
    assert gpu.attention_plan(nrows, hp.n_head, hp.n_kv_head, hp.head_dim, LONG_CTX, True, top_position=ctx)[0] != 3
    plan = check_plan(gpu, hp, nrows, LONG_CTX) if nrows in EXPECTED_PLAN else gpu.attention_plan(nrows, hp.n_head, hp.n_kv_head, hp.head_dim, LONG_CTX, True)
    if plan[0] == 1:
        assert plan[2] < 2047  # several chunks
    fused = gpu.LlmSession(model, nrows, LONG_CTX)
    seq = np.arange(nrows, dtype=np.int32)
    for sq in seq:
        k, v = sess.kv_read(0, int(sq), 0, ctx)
        fused.kv_write(0, int(sq), 0, k, v)
    rng = np.random.default_rng(7000 * nrows + ctx)
    for sq in seq:                                                   # decode_step_case drew the cache rows first: skip past them
        f16_bits(rng, (ctx, hp.n_kv_head, hp.head_dim), 0.6); f16_bits(rng, (ctx, hp.n_kv_head, hp.head_dim), 1.0)
    tok = rng.integers(3, hp.vocab, nrows).astype(np.int32)
    pos = np.full(nrows, ctx, np.int32)
    want, wam = orc.forward(seq, pos, tok)                           # the same row again: the oracle's cache row at `ctx` is rewritten with itself
    got, gam = fused.forward(seq, pos, tok)
    fused.close()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (nrows, ctx, np.abs(got - want).max())
    assert np.array_equal(gam, wam)


def test_prefill_chunk_starting_past_2048_positions(mistral_long):
    """8 sequences x 32 new positions in ONE pass over 2048 cached positions each (k_qkv_rope_append + k_attention_prefill: two 16-row tiles
    per sequence, 33 key blocks of 64 positions): T runs from 2049 to 2080 inside one launch"""
    gpu, model, sess, orc, hp = mistral_long
    nseq, npos, ctx0 = 8, 32, 2048
    assert gpu.attention_plan(nseq * npos, hp.n_head, hp.n_kv_head, hp.head_dim, LONG_CTX, False)[0] == 2   # k_attention_prefill
    rng = np.random.default_rng(4242)
    load_kv(sess, orc, hp, rng, range(nseq), ctx0)
    seq = np.repeat(np.arange(nseq, dtype=np.int32), npos)
    pos = np.tile(np.arange(ctx0, ctx0 + npos, dtype=np.int32), nseq)
    tok = rng.integers(3, hp.vocab, nseq * npos).astype(np.int32)
    want, wam = orc.forward(seq, pos, tok)
    got, gam = sess.forward(seq, pos, tok)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.abs(got - want).max()
    assert np.array_equal(gam, wam)


@pytest.mark.parametrize("ctx0", [0, 31, 97, 159])
def test_prefill_shaped_attention_at_mistral_geometry_bit_exact(mistral1, ctx0):
    """8 sequences x 32 new positions = 256 rows in ONE pass over `ctx0` cached positions each: rows of one sequence see each other causally,
    so the pass takes k_qkv_rope_append + k_attention_prefill (16 rows of a sequence per workgroup); T runs from ctx0 + 1 to ctx0 + 32 inside
    one launch."""
    gpu, model, sess, orc, hp = mistral1
    nseq, npos = 8, 32
    rng = np.random.default_rng(77 + ctx0)
    if ctx0:
        load_kv(sess, orc, hp, rng, range(nseq), ctx0)
    seq = np.repeat(np.arange(nseq, dtype=np.int32), npos)
    pos = np.tile(np.arange(ctx0, ctx0 + npos, dtype=np.int32), nseq)
    tok = rng.integers(3, hp.vocab, nseq * npos).astype(np.int32)
    want, wam = orc.forward(seq, pos, tok)
    got, gam = sess.forward(seq, pos, tok)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (ctx0, np.abs(got - want).max())
    assert np.array_equal(gam, wam)
    gk, gv = sess.kv_read(0, nseq - 1, ctx0, npos)
    wk, wv = orc.kv_read(0, nseq - 1, ctx0, npos)
    assert np.array_equal(gk, wk) and np.array_equal(gv, wv)


def test_kv_hook_argument_errors(mistral1):
    gpu, model, sess, orc, hp = mistral1
    k = np.zeros((4, hp.n_kv_head, hp.head_dim), np.uint16)
    with pytest.raises(gpu.TkError):
        sess.kv_write(1, 0, 0, k, k)            # layer out of range
    with pytest.raises(gpu.TkError):
        sess.kv_write(0, 256, 0, k, k)          # sequence out of range
    with pytest.raises(gpu.TkError):
        sess.kv_write(0, 0, MAX_CTX - 3, k, k)  # runs past the context
    assert gpu.lib().tk_mi355x_llm_session_kv_write(None, 0, 0, 0, 1, None, None) == 1001


def test_narrow_attention_yields_when_sessions_share_the_device(mistral1, monkeypatch):
    """round 6: a narrow-attention workgroup takes a whole CU, so with several decode sessions alive on a device (the fused bench's three groups)
    the launcher's answer is the ring form, which co-resides with the other streams' mat-vec workgroups; one session alone keeps the narrow
    form.  Both are bit-identical (every case of this file runs whichever the plan names), so only the plan is asserted here."""
    gpu, model, sess, orc, hp = mistral1
    ncu = gpu.lib().tk_mi355x_device_cu_count(0)
    if ncu != 256:
        pytest.skip("plan expectations are for 256 CUs")
    monkeypatch.delenv("TK_MI355X_NO_NARROW_ATT", raising=False)
    alive_before = gpu.attention_plan(16, hp.n_head, hp.n_kv_head, hp.head_dim, MAX_CTX, True)
    extra = [gpu.LlmSession(model, 16, MAX_CTX) for _ in range(2)]
    shared = gpu.attention_plan(16, hp.n_head, hp.n_kv_head, hp.head_dim, MAX_CTX, True)
    assert shared[0] == 0 and shared[1] == 2 and shared[2] == 128           # k_attention<2, fused, 128, 128, 2>
    for s in extra:
        s.close()
    assert gpu.attention_plan(16, hp.n_head, hp.n_kv_head, hp.head_dim, MAX_CTX, True) == alive_before
    monkeypatch.setenv("TK_MI355X_NO_NARROW_ATT", "0")
    assert gpu.attention_plan(16, hp.n_head, hp.n_kv_head, hp.head_dim, MAX_CTX, True)[0] == 1   # asked for explicitly
    monkeypatch.setenv("TK_MI355X_NO_NARROW_ATT", "1")
    assert gpu.attention_plan(16, hp.n_head, hp.n_kv_head, hp.head_dim, MAX_CTX, True)[0] == 0


def test_full_7b_prompt64_decode128_ids_match_oracle(gpu):
    """BASELINE configs[1] end to end, the workload the headline metric is quoted on: full 32-layer Mistral-7B Q4_K_M geometry (synthetic
    weights, seed 4), a seeded 64-token prompt (BOS first), batched prefill, then 128 greedy tokens through the captured
    decode graph — every id equal to the oracle's (64 prompt rows in one oracle pass + 128 single-row passes: ~15-20 s of CPU)."""
    model = gpu.LlmModel(gpu.MISTRAL_7B()).fill_synthetic(4)
    hp = model.hparams
    P, N = 64, 128
    rng = np.random.default_rng(3)
    prompt = rng.integers(3, hp.vocab, P).astype(np.int32)
    prompt[0] = 1
    sess = gpu.LlmSession(model, 1, P + N + 8)
    first = sess.prefill(prompt[None, :])
    toks, _ = sess.decode(1, N)
    got = [int(first[0])] + [int(t) for t in toks[:N - 1, 0]]
    sess.close()
    model.close()
    orc = O.OracleLlm(oracle_cfg_from(hp, P + N + 8, 1), seed=4)
    _, am = orc.forward(np.zeros(P, np.int32), np.arange(P, dtype=np.int32), prompt, want_logits=False)
    cur, want = int(am[-1]), []
    for i in range(N):
        want.append(cur)
        if i + 1 < N:
            _, am = orc.forward([0], [P + i], [cur], want_logits=False)
            cur = int(am[0])
    orc.close()
    assert got == want
    assert len(set(got)) > 8


def _ragged_pass(hp, rng, runs, ctx0s):
    seq = np.concatenate([np.full(n, s, np.int32) for s, n in enumerate(runs)])
    pos = np.concatenate([np.arange(c, c + n, dtype=np.int32) for c, n in zip(ctx0s, runs)])
    tok = rng.integers(3, hp.vocab, seq.size).astype(np.int32)
    return seq, pos, tok


@pytest.mark.parametrize("runs,ctx0s", [
    ([1, 5, 16, 17, 33, 63, 100, 21], [0, 150, 7, 64, 33, 0, 91, 128]),        # tiles of 1 .. 16 rows, runs that end mid-tile, 256 rows
    ([180, 76], [0, 60]),                                                       # one long prompt chunk: 12 tiles of one sequence
    ([3, 2, 40], [5, 0, 129]),                                                  # a narrow pass (45 rows)
    ([2] * 32, [(37 * i) % 150 for i in range(32)]),                            # 32 tiles on a grid of 12 tile slots: workgroups walk tiles
])
def test_multi_position_passes_ragged_runs_bit_exact(mistral1, runs, ctx0s, monkeypatch):
    """k_attention_prefill on passes as the batcher builds them — prompt chunks of several sequences, run lengths that are no multiple of
    16, every sequence over its own cached context — against the oracle bit for bit, and the k_attention form
    (TK_MI355X_NO_PREFILL_ATT=1, a fresh session: passes are captured per session) gives the same bits"""
    gpu, model, sess, orc, hp = mistral1
    rng = np.random.default_rng(9000 + sum(runs))
    for s, c in enumerate(ctx0s):
        if c:
            load_kv(sess, orc, hp, rng, [s], c)
    seq, pos, tok = _ragged_pass(hp, rng, runs, ctx0s)
    assert gpu.attention_plan(seq.size, hp.n_head, hp.n_kv_head, hp.head_dim, MAX_CTX, False)[0] == 2
    want, wam = orc.forward(seq, pos, tok)
    got, gam = sess.forward(seq, pos, tok)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.abs(got - want).max()
    assert np.array_equal(gam, wam)
    # the per-row form on the same pass
    monkeypatch.setenv("TK_MI355X_NO_PREFILL_ATT", "1")
    assert gpu.attention_plan(seq.size, hp.n_head, hp.n_kv_head, hp.head_dim, MAX_CTX, False)[0] == 0
    old = gpu.LlmSession(model, len(runs), MAX_CTX)
    for s, c in enumerate(ctx0s):
        if c:
            k, v = sess.kv_read(0, s, 0, c)
            old.kv_write(0, s, 0, k, v)
    ogot, oam = old.forward(seq, pos, tok)
    old.close()
    assert np.array_equal(ogot.view(np.uint32), want.view(np.uint32)) and np.array_equal(oam, wam)


def test_prompt_chunks_of_a_long_prompt_bit_exact(mistral_long):
    """a 700-token prompt fed as the runner feeds it — chunks of 256, 256 and 188 rows of ONE sequence, each chunk attending to everything before
    it (k_attention_prefill: 16 tiles per chunk, up to 11 key blocks) — logits of the last chunk and the cache rows equal to the oracle's"""
    gpu, model, sess, orc, hp = mistral_long
    rng = np.random.default_rng(31337)
    n = 700
    tok = rng.integers(3, hp.vocab, n).astype(np.int32)
    for lo in range(0, n, 256):
        hi = min(n, lo + 256)
        seq = np.full(hi - lo, 3, np.int32)
        pos = np.arange(lo, hi, dtype=np.int32)
        want, wam = orc.forward(seq, pos, tok[lo:hi])
        got, gam = sess.forward(seq, pos, tok[lo:hi])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (lo, np.abs(got - want).max())
        assert np.array_equal(gam, wam)
    gk, gv = sess.kv_read(0, 3, 0, n)
    wk, wv = orc.kv_read(0, 3, 0, n)
    assert np.array_equal(gk, wk) and np.array_equal(gv, wv)
