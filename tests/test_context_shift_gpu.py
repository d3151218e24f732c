"""GPU: context shift (csrc/common/tk_kv_shift.h) — k_kv_shift_rows alone (tk_mi355x_kv_shift_probe), on a session's cache (LlmSession.kv_shift) and
behind tk_llm_runner_* (set_context_shift).

Expected values.  The kernel: the host loop of the same per-row function, which tests/test_context_shift_cpu.py pins to the exact restatement
tests/kv_shift_ref.py, and that restatement itself.  The runner: a stream built by hand from entry points that existed before the feature —
LlmSession.forward, kv_read, kv_write into a FRESH session — with the restatement doing the move on the host and llama.cpp's rule applied in the
test (HandStream).  Synthetic models tokenise bytes: ids = [1] + [3 + b ...]; id 2 ends a generation."""
import threading
import time

import numpy as np
import pytest

import kv_shift_ref as R
from test_context_shift_cpu import HEAD_DIMS, MAX_CTX, MOVES, shape_of, tables, check_move

pytestmark = pytest.mark.gpu

TK_ERROR_INVALID_ARGUMENT = 1001
TK_ERROR_INFERENCE_FAILED = 4002
BLOCK_ROWS = 128  # TK_KV_SHIFT_BLOCK_ROWS: rows a workgroup of k_kv_shift_rows holds in registers between its barrier and its stores
EOS = 2
CTX = 64
SEED = 4
PATH = "synthetic://tiny?seed=%d" % SEED


# ---- 4. the kernel against the host loop ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("head_dim", HEAD_DIMS)
def test_kernel_equals_the_host_loop_and_the_restatement(gpu, head_dim):
    cs, sn = tables(head_dim)
    for case, (p0, p1, delta) in enumerate(MOVES):
        k, v = R.seeded_caches(shape_of(head_dim), seed=100 * head_dim + case)
        gk, gv = check_move(gpu, k, v, cs, sn, case % 3, p0, p1, delta, device=0)
        hk, hv = gpu.kv_shift_probe(k, v, cs, sn, case % 3, p0, p1, delta, device=-1)
        assert R.same_f16_bits(gk, hk) and np.array_equal(gv, hv), (head_dim, p0, p1, delta)


@pytest.mark.parametrize("head_dim", [64, 192, 256])
@pytest.mark.parametrize("d", [BLOCK_ROWS - 1, BLOCK_ROWS, BLOCK_ROWS + 1, 1])
def test_kernel_walks_blocks_that_overlap(gpu, head_dim, d):
    """a move of five row blocks and three rows whose distance is the block, one less, one more, and one row: the only place where a block's stores
    land on rows that a neighbouring block reads.  One layer, two sequences, two KV heads, max_ctx six blocks and sixteen rows"""
    max_ctx = 6 * BLOCK_ROWS + 16
    shape = (1, 2, 2, max_ctx, head_dim)
    cs, sn = tables(head_dim, max_ctx)
    p0 = BLOCK_ROWS + 5
    p1 = p0 + 5 * BLOCK_ROWS + 3
    assert p1 <= max_ctx and p0 - d >= 0
    k, v = R.seeded_caches(shape, seed=head_dim + d)
    gk, gv = check_move(gpu, k, v, cs, sn, 1, p0, p1, -d, device=0)
    hk, hv = gpu.kv_shift_probe(k, v, cs, sn, 1, p0, p1, -d, device=-1)
    assert R.same_f16_bits(gk, hk) and np.array_equal(gv, hv)


def test_kernel_refuses_before_it_launches(gpu):
    cs, sn = tables(64)
    k, v = R.seeded_caches(shape_of(64), seed=9)
    k0, v0 = k.copy(), v.copy()
    for move in [(0, 8, 40, 0), (0, 8, 40, -9), (0, 8, MAX_CTX + 1, -1), (0, 8, 8, -1), (3, 8, 40, -1)]:
        with pytest.raises(gpu.TkError) as e:
            gpu.kv_shift_probe_into(k, v, cs, sn, *move, device=0)
        assert e.value.code == TK_ERROR_INVALID_ARGUMENT and np.array_equal(k, k0) and np.array_equal(v, v0)


# ---- 5. the session entry -------------------------------------------------------------------------------------------------------------------

def _fill(sess, hp, max_ctx, seed):
    rng = np.random.default_rng(seed)
    img = {}
    for layer in range(hp.n_layer):
        for slot in range(3):
            k = rng.integers(0, 65536, (max_ctx, hp.n_kv_head, hp.head_dim)).astype(np.uint16)
            v = rng.integers(0, 65536, (max_ctx, hp.n_kv_head, hp.head_dim)).astype(np.uint16)
            k[rng.integers(0, max_ctx, 40), rng.integers(0, hp.n_kv_head, 40), rng.integers(0, hp.head_dim, 40)] = rng.choice(R.SPECIAL_F16, 40)
            k[:, 0, 0] = R.SPECIAL_F16[np.arange(max_ctx) % len(R.SPECIAL_F16)]
            sess.kv_write(layer, slot, 0, k, v)
            img[(layer, slot)] = (k, v)
    return img


@pytest.mark.parametrize("shape", ["tiny", "7b_row"])
def test_session_kv_shift_equals_the_restatement(gpu, shape):
    """LlmSession.kv_shift against kv_write / kv_read with the session's own rope table restated (float64 pow, cos, sin, rounded to fp32): the
    destination rows equal kv_shift_ref bit for bit, every other row of the sequence (the stale tail included) and both other slots keep their bits"""
    max_ctx = 64
    if shape == "tiny":
        hp = gpu.TINY()
    else:
        hp = gpu.MISTRAL_7B()
        hp.n_layer = 1
    model = gpu.LlmModel(hp).fill_synthetic(4)
    hp = model.hparams
    assert (hp.head_dim, hp.n_kv_head) == ((64, 2) if shape == "tiny" else (128, 8))
    cs, sn = R.rope_table(max_ctx, hp.head_dim, hp.rope_theta)
    sess = gpu.LlmSession(model, 3, max_ctx)
    for case, (p0, p1, delta) in enumerate([(1, 2, -1), (8, 64, -1), (32, 64, -32), (36, 63, -28), (63, 64, -63)]):
        img = _fill(sess, hp, max_ctx, seed=10 * case + (1 if shape == "tiny" else 2))
        slot = case % 3
        sess.kv_shift(slot, p0, p1, delta)
        for layer in range(hp.n_layer):
            for s in range(3):
                gk, gv = sess.kv_read(layer, s, 0, max_ctx)
                k, v = img[(layer, s)]
                if s == slot:
                    wk, wv = R.kv_shift_rows_ref(k, v, cs, sn, p0, p1, delta)
                    assert R.same_f16_bits(gk, wk) and np.array_equal(gv, wv), (shape, p0, p1, delta, layer)
                    keep = np.ones(max_ctx, bool)
                    keep[p0 + delta:p1 + delta] = False
                    assert np.array_equal(gk[keep], k[keep]) and not np.array_equal(gk, k)
                else:
                    assert np.array_equal(gk, k) and np.array_equal(gv, v), (shape, p0, p1, delta, layer, s)
    before = {key: sess.kv_read(key[0], key[1], 0, max_ctx) for key in img}
    for args in [(0, 8, 40, 0), (0, 8, 40, 1), (0, 8, 40, -9), (0, 8, max_ctx + 1, -1), (0, 8, 8, -1), (0, 9, 8, -1), (0, -1, 8, -1), (-1, 8, 40, -1), (3, 8, 40, -1),
                 (0, 8, 40, -2**31)]:
        with pytest.raises(gpu.TkError) as e:
            sess.kv_shift(*args)
        assert e.value.code == TK_ERROR_INVALID_ARGUMENT, args
    for key in img:
        gk, gv = sess.kv_read(key[0], key[1], 0, max_ctx)
        assert np.array_equal(gk, before[key][0]) and np.array_equal(gv, before[key][1])
    sess.close()
    model.close()


# ---- 6. what a shift means, without the restatement ------------------------------------------------------------------------------------------

def test_a_shifted_layer0_key_is_the_key_of_its_token_at_the_new_position(gpu):
    """A layer-0 key depends only on its token and its position: k = f16(rot_p(x)), x the token's fp32 key projection.  Sequence 0 is fed 24 tokens
    and its rows [12, 24) are shifted by -8; sequence 1 is fed four other tokens and then the same twelve at positions 4 .. 15.
    Bound on |shifted - direct| for one element of a pair.  The shifted key is f16(rot_-8(k0 pair)) with k0 = f16(rot_(p+8)(x)): rot_-8 after
    rot_(p+8) is rot_p, so against the direct f16(rot_p(x)) it carries (1) the two final f16 roundings, half an ulp of each result; (2) k0's own
    rounding errors, at most half an ulp of each half of the k0 pair, which the rotation spreads over both halves with weights |cos|, |sin| <= 1: their
    sum; (3) fp32 effects: three table entries with 2^-24 relative error each, two rotations of a product, an fma and a table lookup each, each
    at most 2^-23 of the pair's |a| + |b|: 16 x 2^-24 = 2^-20 of |a| + |b| covers them with room.  Values are copies: bit for bit."""
    model = gpu.LlmModel(gpu.TINY()).fill_synthetic(SEED)
    hp = model.hparams
    sess = gpu.LlmSession(model, 2, 32)
    rng = np.random.default_rng(11)
    toks = rng.integers(3, hp.vocab, 24).astype(np.int32)
    other = rng.integers(3, hp.vocab, 4).astype(np.int32)
    sess.forward(np.zeros(24, np.int32), np.arange(24, dtype=np.int32), toks, want_logits=False)
    sess.forward(np.ones(16, np.int32), np.arange(16, dtype=np.int32), np.concatenate([other, toks[12:]]), want_logits=False)
    k0, _ = sess.kv_read(0, 0, 12, 12)
    sess.kv_shift(0, 12, 24, -8)
    ks, vs = sess.kv_read(0, 0, 4, 12)
    kd, vd = sess.kv_read(0, 1, 4, 12)
    assert np.array_equal(vs, vd)
    f = lambda a: a.view(np.float16).astype(np.float64)
    hu = lambda a: 0.5 * np.spacing(np.abs(a.view(np.float16))).astype(np.float64)
    pair0 = hu(k0)[..., 0::2] + hu(k0)[..., 1::2]
    mag = np.abs(f(k0))[..., 0::2] + np.abs(f(k0))[..., 1::2]
    bound = hu(ks) + hu(kd) + np.repeat(pair0 + 2.0 ** -20 * mag, 2, axis=-1)
    err = np.abs(f(ks) - f(kd))
    print("largest |shifted - direct| / bound:", float((err / bound).max()), "elements that differ:", int((ks != kd).sum()), "of", ks.size)
    assert np.isfinite(f(ks)).all() and (err <= bound).all()
    assert not np.array_equal(ks, k0)  # the keys were rotated, not copied
    sess.close()
    model.close()


# ---- the hand-built stream --------------------------------------------------------------------------------------------------------------------

def prompt_ids(p):
    return [1] + [3 + b for b in p.encode()]


def tool_ids(name, output):
    return [3 + b for b in ('[TOOL_RESULT] name: "%s", output: %s [/TOOL_RESULT]' % (name, output)).encode()]


class HandStream:
    """tk_llm_runner_* restated on one bare session of one sequence: prepare, next_token, add_tool_response and llama.cpp's shift rule, the move
    done on the HOST by kv_shift_ref between kv_read of the old session and kv_write into a fresh one"""

    def __init__(self, gpu, model, n_keep, ctx=CTX):
        self.gpu, self.model, self.n_keep, self.ctx = gpu, model, n_keep, ctx
        self.hp = model.hparams
        self.cs, self.sn = R.rope_table(ctx, self.hp.head_dim, self.hp.rope_theta)
        self.sess = gpu.LlmSession(model, 1, ctx)
        self.n_past, self.pending, self.accepted, self.shifts, self.discarded, self.on = 0, -1, [], 0, 0, True

    def _feed(self, toks):
        n = len(toks)
        _, am = self.sess.forward(np.zeros(n, np.int32), np.arange(self.n_past, self.n_past + n, dtype=np.int32), np.asarray(toks, np.int32), want_logits=False)
        self.n_past += n
        self.pending = int(am[-1])

    def prepare(self, prompt):
        ids = prompt_ids(prompt)
        self.n_prompt = len(ids)
        self.n_past, self.accepted, self.shifts, self.discarded = 0, [], 0, 0
        self._feed(ids)

    def _shift(self, need):
        n_keep = self.n_prompt if self.n_keep < 0 else self.n_keep
        n_discard = (self.n_past - n_keep) // 2 if self.n_past >= n_keep else 0
        if not self.on or n_discard <= 0 or self.n_past - n_discard + need >= self.ctx:
            return False
        fresh = self.gpu.LlmSession(self.model, 1, self.ctx)
        for layer in range(self.hp.n_layer):
            k, v = self.sess.kv_read(layer, 0, 0, self.ctx)
            k, v = R.kv_shift_rows_ref(k, v, self.cs, self.sn, n_keep + n_discard, self.n_past, -n_discard)
            fresh.kv_write(layer, 0, 0, k[:self.n_past - n_discard], v[:self.n_past - n_discard])
        self.sess.close()
        self.sess = fresh
        self.n_past -= n_discard
        self.shifts += 1
        self.discarded += n_discard
        return True

    def next_token(self):
        """False where generate_next_token returns NULL"""
        tid = self.pending
        if tid >= 0:
            self.accepted.append(tid)
        if tid < 0 or tid == EOS:
            return False
        if self.n_past + 1 >= self.ctx and not self._shift(1):
            return False
        self._feed([tid])
        return True

    def add_tool_response(self, name, output):
        toks = tool_ids(name, output)
        if self.n_past + len(toks) >= self.ctx and not self._shift(len(toks)):
            return False
        self._feed(toks)
        return True

    def close(self):
        self.sess.close()


class Handle:
    def __init__(self, gpu, slots=None, prefix_cache=False):
        self.gpu, self.loader = gpu, gpu.ModelLoader()
        self.h = self.loader.load(PATH, force_reload=True)  # private: its scheduler and its counters are this test's alone
        if slots:
            gpu.ModelLoader.set_runner_slots(self.h, slots)
        if prefix_cache:
            gpu.ModelLoader.set_prefix_cache(self.h, True)
        self.runners = []

    def runner(self, ctx=CTX):
        r = self.gpu.LlmRunner(self.h, context_size=ctx)
        self.runners.append(r)
        return r

    def close(self):
        for r in self.runners:
            r.close()
        self.loader.unload(self.h)
        self.loader.close()


def run_until(runner, shifts, extra, cap=400):
    """next_token until `shifts` shifts have happened, then `extra` more calls; returns the accepted ids"""
    runner_calls = 0
    while runner.context_shifts()[0] < shifts:
        assert runner.next_token() is not None, "the generation ended after %d calls, before shift %d" % (runner_calls, shifts)
        runner_calls += 1
        assert runner_calls < cap
    for _ in range(extra):
        assert runner.next_token() is not None
    return runner.recent_tokens()


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------------------------

PROMPT7, PROMPT9, KEEP7 = "a", "hi", 8  # "a": of the short prompts tried on the CPU oracle the one whose greedy stream varies most (12 distinct ids in 110)


def _hand_stream7(gpu):
    model = gpu.LlmModel(gpu.TINY()).fill_synthetic(SEED)
    hs = HandStream(gpu, model, KEEP7)
    hs.prepare(PROMPT7)
    while hs.shifts < 2:
        assert hs.next_token(), "the hand-built stream of this prompt and seed meets EOS before its second shift: choose another prompt"
    for _ in range(5):
        assert hs.next_token()
    out = (list(hs.accepted), hs.shifts, hs.discarded)
    hs.close()
    model.close()
    return out


@pytest.mark.parametrize("path", ["run-ahead", "no-run-ahead"])
def test_runner_goes_on_past_the_end_of_its_context(gpu, path):
    """context_size 64, greedy, n_keep 8, prompt of 2 ids: the first shift comes at n_past 63 (27 rows dropped), the second 27 tokens later.  The
    accepted ids equal the hand-built stream.  Plain, the row that fills the context (position 62) is a run-ahead row; with a -inf bias on an id
    the stream never holds the runner does not run ahead and every row is a request.  Without the feature next_token() is None after 61 tokens.
    The prompt's plain greedy stream holds no EOS in its first 110 ids at context_size 512 (CPU oracle, seed 4); past the first shift the stream is
    another one, and the hand-built stream itself asserts that it meets none"""
    want, shifts, discarded = _hand_stream7(gpu)
    assert shifts == 2 and discarded == 54 and EOS not in want
    h = Handle(gpu)
    r = h.runner()
    r.set_context_shift(True, KEEP7)
    if path == "no-run-ahead":
        unused = next(i for i in range(3, 512) if i not in want)
        r.set_logit_bias([unused], [-np.inf])
    r.prepare(PROMPT7)
    got = run_until(r, 2, 5)
    assert r.context_shifts() == (2, 54)
    assert got == want, [i for i, (a, b) in enumerate(zip(got, want)) if a != b][:4]
    wasted = gpu.ModelLoader.run_ahead_wasted(h.h)
    assert wasted == 0 if path == "no-run-ahead" else True
    r.prepare(PROMPT7)  # the counters restart with the prompt
    assert r.context_shifts() == (0, 0)
    with pytest.raises(gpu.TkError) as e:
        r.set_context_shift(True, -2)
    assert e.value.code == TK_ERROR_INVALID_ARGUMENT
    h.close()


def test_keep_minus_one_is_the_prompt(gpu):
    """n_keep = -1 resolves to the last prompt's token count when the shift happens"""
    prompt = "keep all of me"
    model = gpu.LlmModel(gpu.TINY()).fill_synthetic(SEED)
    hs = HandStream(gpu, model, -1)
    hs.prepare(prompt)
    while hs.shifts < 1:
        assert hs.next_token()
    for _ in range(4):
        assert hs.next_token()
    n = len(prompt_ids(prompt))
    assert hs.discarded == (CTX - 1 - n) // 2
    h = Handle(gpu)
    r = h.runner()
    r.set_context_shift(True, -1)
    r.prepare(prompt)
    assert run_until(r, 1, 4) == hs.accepted and r.context_shifts() == (1, hs.discarded)
    hs.close()
    model.close()
    h.close()


# ---- 8. off is off ----------------------------------------------------------------------------------------------------------------------------

def _until_none(r, cap=200):
    n = 0
    while r.next_token() is not None:
        n += 1
        assert n < cap
    return n


def _settled_stats(gpu, handle, quiet_reads=10, limit_s=5.0):
    """batch_stats once the scheduler is idle: the same answer `quiet_reads` times in a row, a millisecond apart (a TINY pass takes far less)"""
    last, same, t_end = gpu.ModelLoader.batch_stats(handle), 0, time.monotonic() + limit_s
    while same < quiet_reads:
        assert time.monotonic() < t_end, "the scheduler's counters never settled"
        time.sleep(0.001)
        cur = gpu.ModelLoader.batch_stats(handle)
        same = same + 1 if cur == last else 0
        last = cur
    return last


def test_off_is_off(gpu):
    want, _, _ = _hand_stream7(gpu)
    n_prompt = len(prompt_ids(PROMPT7))
    long_output = "x" * 20
    h_never, h_off = Handle(gpu), Handle(gpu)
    never, off = h_never.runner(), h_off.runner()
    off.set_context_shift(True, KEEP7)
    off.set_context_shift(False, KEEP7)
    for r in (never, off):
        r.prepare(PROMPT7)
        assert _until_none(r) == CTX - 1 - n_prompt  # n_past + 1 >= n_ctx at n_past 63: where it stops today
        assert r.recent_tokens() == want[:CTX - n_prompt] and r.context_shifts() == (0, 0)
        assert r.next_token() is None
        r.prepare(PROMPT7)
        for _ in range(20):
            assert r.next_token() is not None
        with pytest.raises(gpu.TkError) as e:  # 20 tokens after the prompt, then 68 rows: they do not fit
            r.add_tool_response("t", long_output)
        assert e.value.code == TK_ERROR_INFERENCE_FAILED and "exceeds the context window" in e.value.detail
    # a second pair of handles: the same 12-token generation leaves the same scheduler counters and the same rows.  With a -inf bias on an unused id
    # neither runner runs ahead and the passes are exactly 1 (prompt) + 12; plain, the row that runs ahead of the 12th token is planned, in flight or
    # done when the owner returns — on either handle, as before the feature — and once it is done nothing more is planned (a row runs ahead only of a
    # token that was asked for), so the counters are read when they have stopped changing: 14 passes on both
    unused = next(i for i in range(3, 512) if i not in want)
    for biased in (True, False):
        a, b = Handle(gpu), Handle(gpu)
        ra, rb = a.runner(), b.runner()
        rb.set_context_shift(True, KEEP7)
        rb.set_context_shift(False, 0)
        for r in (ra, rb):
            if biased:
                r.set_logit_bias([unused], [-np.inf])
            r.prepare(PROMPT7)
            for _ in range(12):
                assert r.next_token() is not None
        assert ra.recent_tokens() == rb.recent_tokens() == want[:12]
        sa, sb = _settled_stats(gpu, a.h), _settled_stats(gpu, b.h)
        print("biased" if biased else "plain", "batch_stats (passes, rows, widest): never set", sa, "set to off", sb)
        assert sa[1:] == sb[1:] == (n_prompt + 12, n_prompt)
        assert sa[0] == sb[0] == (13 if biased else 14)
        a.close()
        b.close()
    for x in (h_never, h_off):
        x.close()


# ---- 9. a tool response that needs the room -----------------------------------------------------------------------------------------------------

def test_tool_response_fits_after_one_shift(gpu):
    """prompt of 3 ids and 15 tokens: n_past 18.  A response of 50 ids does not fit (18 + 50 >= 64); one shift (n_keep 8, 5 rows dropped) makes room
    (13 + 50 < 64).  A response of 68 ids is longer than n_ctx - n_keep: it fails and nothing has moved — the ids that follow equal those of the
    session-level twin, which made the same moves (none) and whose cache is read back"""
    model = gpu.LlmModel(gpu.TINY()).fill_synthetic(SEED)
    h = Handle(gpu)
    for output, fits in (("ok", True), ("x" * 20, False)):
        hs = HandStream(gpu, model, KEEP7)
        r = h.runner()
        r.set_context_shift(True, KEEP7)
        hs.prepare(PROMPT9)
        r.prepare(PROMPT9)
        for _ in range(15):
            assert hs.next_token() and r.next_token() is not None
        assert hs.n_past == 18 and len(tool_ids("t", output)) == (50 if fits else 68)
        twin_before = [hs.sess.kv_read(layer, 0, 0, hs.n_past) for layer in range(hs.hp.n_layer)]
        if fits:
            assert hs.add_tool_response("t", output)
            r.add_tool_response("t", output)
            assert r.context_shifts() == (1, 5) == (hs.shifts, hs.discarded) and hs.n_past == 13 + 50
        else:
            assert not hs.add_tool_response("t", output)
            with pytest.raises(gpu.TkError) as e:
                r.add_tool_response("t", output)
            assert e.value.code == TK_ERROR_INFERENCE_FAILED
            assert r.context_shifts() == (0, 0) and hs.n_past == 18
            for layer, (k, v) in enumerate(twin_before):
                gk, gv = hs.sess.kv_read(layer, 0, 0, hs.n_past)
                assert np.array_equal(gk, k) and np.array_equal(gv, v)
        for _ in range(8):  # with the response in n_past is 63: the next call shifts again
            assert hs.next_token() and r.next_token() is not None
        assert r.recent_tokens() == hs.accepted and r.context_shifts() == (hs.shifts, hs.discarded)
        assert hs.shifts == (2 if fits else 0)
        hs.close()
        r.close()
        h.runners.remove(r)
    h.close()
    model.close()


# ---- 10. the prefix cache never keeps or copies a moved row -----------------------------------------------------------------------------------

def _ascii(n, salt):
    rng = np.random.default_rng(2000 + salt)
    return "".join(chr(c) for c in rng.integers(97, 123, n))


def test_prefix_cache_forgets_the_rows_a_shift_moved(gpu):
    """prefix cache on, two slots.  A prepares 59 bytes (60 ids) and shifts at n_past 63: its context is then ids[0:8] + ids[35:60] + three generated
    ids.  B prepares the string whose ids are the first 33 of those — 25 of them beyond n_keep, all of them rows A's slot holds, but moved there
    from another context: B copies at most n_keep rows and its tokens equal a cache-off runner's.  A then prepares its old prompt: at most n_keep
    rows are kept, tokens equal cache off"""
    P = _ascii(59, 1)
    on, off = Handle(gpu, slots=2, prefix_cache=True), Handle(gpu, slots=2)
    a, b = on.runner(), on.runner()
    a_off, b_off = off.runner(), off.runner()
    for r in (a, a_off):
        r.set_context_shift(True, KEEP7)
        r.prepare(P)
        for _ in range(6):
            assert r.next_token() is not None
        assert r.context_shifts() == (1, 27)
    assert a.recent_tokens() == a_off.recent_tokens()
    assert a.last_prompt_rows() == (60, 0, 0)
    Q = P[0:7] + P[34:59]
    assert prompt_ids(Q) == prompt_ids(P)[0:8] + prompt_ids(P)[35:60] and len(prompt_ids(Q)) - KEEP7 >= 24

    def gen(r, prompt, n=12):
        r.prepare(prompt)
        for _ in range(n):
            if r.next_token() is None:
                break
        return r.recent_tokens()

    want_b, got_b = gen(b_off, Q), gen(b, Q)
    rows, kept, copied = b.last_prompt_rows()
    print("B's prompt rows, kept, copied:", rows, kept, copied)
    assert rows == 33 and kept == 0 and copied <= KEEP7
    assert got_b == want_b and len(want_b) == 12
    want_a, got_a = gen(a_off, P, 3), gen(a, P, 3)
    rows, kept, copied = a.last_prompt_rows()
    print("A's old prompt rows, kept, copied:", rows, kept, copied)
    assert rows == 60 and kept <= KEEP7 and kept + copied <= 33  # B's slot holds Q: ids[0:8] of it are P's too
    assert got_a == want_a and len(want_a) == 3
    on.close()
    off.close()


# ---- 11. four runners, four threads ---------------------------------------------------------------------------------------------------------

def test_four_runners_shift_each_at_its_own_moment(gpu):
    prompts = ["a", "four runners b", "the third of four runners has more", "d: " + _ascii(40, 3)]
    keeps = [0, 8, -1, 16]
    h = Handle(gpu, slots=4)

    def drive(r, i, out):
        r.set_context_shift(True, keeps[i])
        r.prepare(prompts[i])
        out[i] = (run_until(r, 2, 3), r.context_shifts())

    alone = [None] * 4
    for i in range(4):
        r = h.runner()
        drive(r, i, alone)
        r.close()
        h.runners.remove(r)
    runners = [h.runner() for _ in range(4)]
    together, errs = [None] * 4, []

    def work(i):
        try:
            drive(runners[i], i, together)
        except BaseException as e:  # noqa: BLE001
            errs.append((i, repr(e)))

    th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    assert together == alone
    assert len({c[1][1] for c in alone}) == 4  # four different amounts dropped: four different moments
    _, _, widest = gpu.ModelLoader.batch_stats(h.h)
    print("widest pass with four runners:", widest, "rows dropped per runner:", [c[1][1] for c in alone])
    h.close()
