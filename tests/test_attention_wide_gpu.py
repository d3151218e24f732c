"""Wide decode passes (193 .. 256 rows: k_attention<4, fused, 128, 32>, the headline bench's decode launch) where the cases of
test_llm_attention_gpu.py stop: every row of a pass there has the same context length.  Here, against the oracle and BIT FOR BIT
(logits as uint32, ids, the appended K / V row of EVERY row):

  * ragged positions inside one pass — rows at 0, 1, 31, 32, 33, 63, 64, 65, 127, 128 and 190 cached positions side by side, so
    workgroups that are resident together walk different numbers of chunks, one of them has an empty context, and the row's own
    K / V patch lands in either ring slot and at either end of a chunk;
  * 193, 200 and 255 rows, not only 256;
  * a session of 200 positions and one of 520: the kernel's LDS layout (score array, the q staged inside it) depends on the capacity;
  * the bench's own loop: 64-token prompts, then 128 graph-replayed greedy steps at 256 rows — every id of every row.

The oracle side of the same cases runs without a GPU first (the two tests that are not marked): a ragged pass must equal its rows
evaluated one at a time, and a batched greedy loop must equal its sequences run alone."""
import numpy as np
import pytest

import oracle_lib as O
from test_llm_gpu import oracle_cfg_from

RAGGED = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 190]
WIDTHS = [193, 200, 255, 256]
CAPACITIES = [200, 520]


def ragged_positions(nrows, shift):
    """row i sits at RAGGED[(i + shift) % 11]: 11 is odd, so neighbouring rows (and the 8 KV-head workgroups of each) never agree"""
    return np.array([RAGGED[(i + shift) % len(RAGGED)] for i in range(nrows)], np.int32)


def f16_bits(rng, shape, scale):
    return (rng.standard_normal(shape, dtype=np.float32) * scale).astype(np.float16).view(np.uint16)


# ------------------------------------------------------------------------------------------ the oracle alone (CPU)
def test_oracle_ragged_pass_equals_its_rows_one_at_a_time():
    """tiny GQA geometry (4 query heads per KV head, as Mistral): one pass of 255 rows at ragged positions over seeded K / V rows gives, row
    for row, the logits, id and appended K / V of a pass that holds that row alone"""
    nrows, cap = 255, 200
    cfg = O.tiny_config(n_head=8, n_kv_head=2, head_dim=64, d_model=512, max_ctx=cap, max_seq=nrows)
    both, single = O.OracleLlm(cfg, seed=4), O.OracleLlm(cfg, seed=4)
    rng = np.random.default_rng(5)
    pos = ragged_positions(nrows, 3)
    for layer in range(cfg.n_layer):
        for s in range(nrows):
            if pos[s]:
                k, v = f16_bits(rng, (pos[s], 2, 64), 0.6), f16_bits(rng, (pos[s], 2, 64), 1.0)
                both.kv_write(layer, s, 0, k, v)
                single.kv_write(layer, s, 0, k, v)
    tok = rng.integers(3, cfg.vocab, nrows).astype(np.int32)
    seq = np.arange(nrows, dtype=np.int32)
    want, wam = both.forward(seq, pos, tok)
    for s in range(nrows):
        got, gam = single.forward([s], [pos[s]], [tok[s]])
        assert np.array_equal(got[0].view(np.uint32), want[s].view(np.uint32)), (s, pos[s])
        assert gam[0] == wam[s]
        for layer in range(cfg.n_layer):
            a, b = both.kv_read(layer, s, int(pos[s]), 1), single.kv_read(layer, s, int(pos[s]), 1)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_oracle_batched_greedy_loop_equals_sequences_alone():
    """prompt pass + greedy steps from position 64, 8 sequences in one pass per step against each sequence in an oracle of its own"""
    nseq, P, N = 8, 64, 24
    cfg = O.tiny_config(n_head=8, n_kv_head=2, head_dim=64, d_model=512, max_ctx=P + N + 8, max_seq=nseq)
    rng = np.random.default_rng(6)
    prompts = rng.integers(3, cfg.vocab, (nseq, P)).astype(np.int32)
    prompts[:, 0] = 1
    want = oracle_greedy(O.OracleLlm(cfg, seed=4), prompts, N)
    for s in range(nseq):
        cfg1 = O.tiny_config(n_head=8, n_kv_head=2, head_dim=64, d_model=512, max_ctx=P + N + 8, max_seq=1)
        alone = oracle_greedy(O.OracleLlm(cfg1, seed=4), prompts[s:s + 1], N)
        assert np.array_equal(alone[:, 0], want[:, s]), s
    assert want.shape == (N + 1, nseq) and len({tuple(want[:, s]) for s in range(nseq)}) > 1  # the sequences do differ


def oracle_greedy(orc, prompts, n_steps):
    """ids [1 + n_steps][nseq]: row 0 is the id the prompt pass picks (what prefill returns), row i the id of decode step i - 1"""
    nseq, P = prompts.shape
    seq = np.arange(nseq, dtype=np.int32)
    for s in range(nseq):
        orc.forward(np.full(P - 1, s, np.int32), np.arange(P - 1, dtype=np.int32), prompts[s, :P - 1], want_logits=False)
    _, cur = orc.forward(seq, np.full(nseq, P - 1, np.int32), prompts[:, P - 1], want_logits=False)
    out = [cur.copy()]
    for i in range(n_steps):
        _, cur = orc.forward(seq, np.full(nseq, P + i, np.int32), cur, want_logits=False)
        out.append(cur.copy())
    return np.stack(out)


# ------------------------------------------------------------------------------------------ the product against it (GPU)
@pytest.fixture(scope="module")
def mistral1(gpu):
    """one Mistral-7B-shaped layer (4096 / 14336 / 32000, 32q / 8kv x 128, production K-split plan), 256 sequences"""
    hp = gpu.MISTRAL_7B()
    hp.n_layer = 1
    model = gpu.LlmModel(hp).fill_synthetic(4)
    hp = model.hparams
    assert (hp.n_head, hp.n_kv_head, hp.head_dim) == (32, 8, 128)
    yield gpu, model, hp
    model.close()


@pytest.fixture(scope="module", params=CAPACITIES)
def wide(request, mistral1):
    gpu, model, hp = mistral1
    cap = request.param
    sess = gpu.LlmSession(model, 256, cap)
    orc = O.OracleLlm(oracle_cfg_from(hp, cap, 256), seed=4)
    yield gpu, sess, orc, hp, cap
    sess.close()
    orc.close()


def check_wide_plan(gpu, hp, nrows, cap):
    plan = gpu.attention_plan(nrows, hp.n_head, hp.n_kv_head, hp.head_dim, cap, True)
    if gpu.lib().tk_mi355x_device_cu_count(0) == 256:
        assert tuple(plan[:4]) == (0, 4, 32, 2), (nrows, plan)  # k_attention<4, fused, 128, 32>, two ring slots


@pytest.mark.gpu
@pytest.mark.parametrize("nrows", WIDTHS)
def test_ragged_positions_in_one_wide_pass_bit_exact(wide, nrows):
    """one decode row per sequence, the rows of the pass at the RAGGED positions mixed (a session of 520 positions adds 255, 256, 300 and 519
    cached positions to the mix): logits, ids and every row's appended K / V equal the oracle's"""
    gpu, sess, orc, hp, cap = wide
    check_wide_plan(gpu, hp, nrows, cap)
    rng = np.random.default_rng(100 * nrows + cap)
    pos = ragged_positions(nrows, nrows)
    if cap > 256:
        for i, extra in enumerate([255, 256, 300, cap - 1]):
            pos[(37 * (i + 1)) % nrows] = extra
    seq = np.arange(nrows, dtype=np.int32)
    for s in seq:
        if pos[s]:
            k = f16_bits(rng, (pos[s], hp.n_kv_head, hp.head_dim), 0.6)
            v = f16_bits(rng, (pos[s], hp.n_kv_head, hp.head_dim), 1.0)
            sess.kv_write(0, int(s), 0, k, v)
            orc.kv_write(0, int(s), 0, k, v)
    tok = rng.integers(3, hp.vocab, nrows).astype(np.int32)
    want, wam = orc.forward(seq, pos, tok)
    got, gam = sess.forward(seq, pos, tok)
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    assert bad.size == 0, (nrows, cap, [(int(r), int(pos[r])) for r in bad[:8]], np.abs(got - want).max())
    assert np.array_equal(gam, wam)
    for s in seq:
        gk, gv = sess.kv_read(0, int(s), int(pos[s]), 1)
        wk, wv = orc.kv_read(0, int(s), int(pos[s]), 1)
        assert np.array_equal(gk, wk) and np.array_equal(gv, wv), (int(s), int(pos[s]))
    for s in (int(np.argmax(pos)), nrows - 1):  # the rows loaded through the hook are untouched
        if pos[s]:
            gk, gv = sess.kv_read(0, s, 0, int(pos[s]))
            wk, wv = orc.kv_read(0, s, 0, int(pos[s]))
            assert np.array_equal(gk, wk) and np.array_equal(gv, wv)


@pytest.mark.gpu
@pytest.mark.parametrize("nrows", [193, 200, 255])
def test_uniform_context_at_odd_widths_bit_exact(wide, nrows):
    """every row at 128 cached positions (the bench's mid-decode point), at widths whose last 32-row M-tile is ragged"""
    gpu, sess, orc, hp, cap = wide
    check_wide_plan(gpu, hp, nrows, cap)
    rng = np.random.default_rng(7 * nrows + cap)
    ctx = 128
    seq = np.arange(nrows, dtype=np.int32)
    for s in seq:
        k = f16_bits(rng, (ctx, hp.n_kv_head, hp.head_dim), 0.6)
        v = f16_bits(rng, (ctx, hp.n_kv_head, hp.head_dim), 1.0)
        sess.kv_write(0, int(s), 0, k, v)
        orc.kv_write(0, int(s), 0, k, v)
    pos = np.full(nrows, ctx, np.int32)
    tok = rng.integers(3, hp.vocab, nrows).astype(np.int32)
    want, wam = orc.forward(seq, pos, tok)
    got, gam = sess.forward(seq, pos, tok)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (nrows, cap, np.abs(got - want).max())
    assert np.array_equal(gam, wam)
    for s in (0, nrows // 2, nrows - 1):
        gk, gv = sess.kv_read(0, s, ctx, 1)
        wk, wv = orc.kv_read(0, s, ctx, 1)
        assert np.array_equal(gk, wk) and np.array_equal(gv, wv)


@pytest.mark.gpu
def test_128_graph_replayed_steps_at_256_rows_from_position_64(gpu):
    """the headline's loop on one layer: 256 seeded 64-token prompts, batched prefill, then 128 greedy steps through the captured decode
    graph (positions 64 .. 191, session capacity 200 as the bench's) — every id of every row equals the oracle's.  The attention geometry
    is Mistral-7B's (d_model 4096, 32 query / 8 KV heads of 128); the MLP and the vocabulary are narrow (d_ff 2048, 4096 tokens) because the
    oracle walks 49 000 rows on the CPU here and attention is what this file is about."""
    hp = gpu.MISTRAL_7B()
    hp.n_layer, hp.d_ff, hp.vocab = 1, 2048, 4096
    model = gpu.LlmModel(hp).fill_synthetic(4)
    hp = model.hparams
    assert (hp.d_model, hp.n_head, hp.n_kv_head, hp.head_dim) == (4096, 32, 8, 128)
    nseq, P, N, cap = 256, 64, 128, 200
    check_wide_plan(gpu, hp, nseq, cap)
    rng = np.random.default_rng(11)
    prompts = rng.integers(3, hp.vocab, (nseq, P)).astype(np.int32)
    prompts[:, 0] = 1
    sess = gpu.LlmSession(model, nseq, cap)
    first = sess.prefill(prompts)
    toks, _ = sess.decode(nseq, N)
    sess.close()
    model.close()
    got = np.concatenate([first[None, :], toks])
    orc = O.OracleLlm(oracle_cfg_from(hp, cap, nseq), seed=4)
    want = oracle_greedy(orc, prompts, N)
    orc.close()
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:8].tolist())
    assert len({tuple(want[:, s]) for s in range(0, nseq, 16)}) > 1
