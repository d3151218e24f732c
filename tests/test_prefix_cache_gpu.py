"""Prompt prefix cache behind tk_llm_runner_* (csrc/llm/tk_llm_batcher.h): rows the shared KV cache already holds for a prompt's leading tokens
are kept (same slot) or copied by k_kv_copy_rows (another slot) instead of being recomputed.

The yardstick of every comparison is a run with the cache OFF — the path the rest of the suite pins to the oracle — on a handle of its own
(force_reload: a private copy of the same synthetic weights), never the cached path against itself.  Synthetic models tokenise bytes, ids =
[1] + [3 + b ...], so for ASCII prompts every expected row count is exact: 1 + bytes."""
import threading

import numpy as np
import pytest

from trackiellm_amd._lib import TkError

pytestmark = pytest.mark.gpu

TK_ERROR_INVALID_ARGUMENT = 1001
CTX = 512
NTOK = 12


def n_ids(prompt):
    return 1 + len(prompt.encode())


def generate(runner, prompt, n=NTOK, grammar=False):
    runner.prepare(prompt, grammar)
    out = []
    for _ in range(n):
        p = runner.next_token()
        if p is None:
            break
        out.append(p)
    return out


def text(n, salt):
    """n bytes of printable ASCII, different for every salt from the first byte on"""
    rng = np.random.default_rng(1000 + salt)
    body = "".join(chr(c) for c in rng.integers(97, 123, n))
    return (chr(65 + salt % 26) + body)[:n]


class Handles:
    """two private copies of one synthetic model: `on` with the prefix cache, `off` without (today's path)"""

    def __init__(self, gpu, path="synthetic://tiny?seed=4", slots=None):
        self.gpu, self.loader = gpu, gpu.ModelLoader()
        self.off = self.loader.load(path, force_reload=True)
        self.on = self.loader.load(path, force_reload=True)
        assert self.off.value != self.on.value
        for h in (self.off, self.on):
            if slots:
                gpu.ModelLoader.set_runner_slots(h, slots)
        gpu.ModelLoader.set_prefix_cache(self.on, True)
        self.runners = []

    def runner(self, h, **kw):
        r = self.gpu.LlmRunner(h, context_size=kw.pop("context_size", CTX), **kw)
        self.runners.append(r)
        return r

    def close(self):
        for r in self.runners:
            r.close()
        self.loader.unload(self.off)
        self.loader.unload(self.on)
        self.loader.close()


# ---- 1. the kernel, on a bare session ------------------------------------------------------------------------------------------------

SPECIAL_F16 = np.array([0x7C00, 0xFC00, 0x7E00, 0xFE01, 0x7FFF, 0xFFFF, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0000, 0x8000, 0x7BFF, 0x0400], np.uint16)


def _fill(sess, hp, max_ctx, seed):
    """distinct seeded f16 bit patterns (NaN, Inf and denormal ones among them) in slots 0, 1, 2 of every layer; returns the host image"""
    rng = np.random.default_rng(seed)
    img = {}
    for layer in range(hp.n_layer):
        for slot in range(3):
            k = rng.integers(0, 65536, (max_ctx, hp.n_kv_head, hp.head_dim)).astype(np.uint16)
            v = rng.integers(0, 65536, (max_ctx, hp.n_kv_head, hp.head_dim)).astype(np.uint16)
            k[rng.integers(0, max_ctx, 40), rng.integers(0, hp.n_kv_head, 40), rng.integers(0, hp.head_dim, 40)] = rng.choice(SPECIAL_F16, 40)
            v[rng.integers(0, max_ctx, 40), rng.integers(0, hp.n_kv_head, 40), rng.integers(0, hp.head_dim, 40)] = rng.choice(SPECIAL_F16, 40)
            k[:, 0, 0] = SPECIAL_F16[np.arange(max_ctx) % len(SPECIAL_F16)]     # every row carries one for certain
            sess.kv_write(layer, slot, 0, k, v)
            img[(layer, slot)] = (k, v)
    return img


def _read_all(sess, hp, max_ctx):
    return {(layer, slot): sess.kv_read(layer, slot, 0, max_ctx) for layer in range(hp.n_layer) for slot in range(3)}


@pytest.mark.parametrize("shape", ["tiny", "7b_row"])
def test_kv_copy_is_a_bit_copy_of_exactly_the_rows_asked_for(gpu, shape):
    """LlmSession.kv_copy against kv_write / kv_read: the destination range equals the source bit for bit; every other position of the
    destination, the whole source and a third slot are unchanged.  TINY (head_dim 64, 2 KV heads, 2 layers) and one layer of the 7B row shape
    (head_dim 128, 8 KV heads)."""
    max_ctx = 64
    if shape == "tiny":
        hp = gpu.TINY()
    else:
        hp = gpu.MISTRAL_7B()
        hp.n_layer = 1
    model = gpu.LlmModel(hp).fill_synthetic(4)
    hp = model.hparams
    assert (hp.head_dim, hp.n_kv_head) == ((64, 2) if shape == "tiny" else (128, 8))
    sess = gpu.LlmSession(model, 3, max_ctx)
    for case, (p0, n) in enumerate([(0, 1), (0, max_ctx), (7, 1), (5, 59), (max_ctx - 1, 1)]):
        img = _fill(sess, hp, max_ctx, seed=10 * case + (1 if shape == "tiny" else 2))
        sess.kv_copy(0, 1, p0, n)
        got = _read_all(sess, hp, max_ctx)
        for layer in range(hp.n_layer):
            for c in (0, 1):                                                    # K, V
                src, dst, third = img[(layer, 0)][c], img[(layer, 1)][c], img[(layer, 2)][c]
                want = dst.copy()
                want[p0:p0 + n] = src[p0:p0 + n]
                assert not np.array_equal(want, dst)                            # the copy has something to change
                assert np.array_equal(got[(layer, 1)][c], want), (shape, p0, n, layer, c)
                assert np.array_equal(got[(layer, 0)][c], src), (shape, p0, n, layer, c)
                assert np.array_equal(got[(layer, 2)][c], third), (shape, p0, n, layer, c)
    # a source serves a second destination, and the other direction works too
    img = _fill(sess, hp, max_ctx, seed=99)
    sess.kv_copy(0, 2, 3, 20)
    sess.kv_copy(2, 1, 0, 30)
    got = _read_all(sess, hp, max_ctx)
    for layer in range(hp.n_layer):
        for c in (0, 1):
            s2 = img[(layer, 2)][c].copy()
            s2[3:23] = img[(layer, 0)][c][3:23]
            s1 = img[(layer, 1)][c].copy()
            s1[0:30] = s2[0:30]
            assert np.array_equal(got[(layer, 2)][c], s2) and np.array_equal(got[(layer, 1)][c], s1) and np.array_equal(got[(layer, 0)][c], img[(layer, 0)][c])
    # bad arguments: refused, nothing changes
    before = _read_all(sess, hp, max_ctx)
    for args in [(0, 0, 0, 1), (1, 1, 3, 4), (0, 1, 0, max_ctx + 1), (0, 1, max_ctx, 1), (0, 1, 60, 5), (0, 1, -1, 2), (0, 1, 0, 0), (0, 1, 0, -3), (-1, 1, 0, 1),
                 (0, -1, 0, 1), (3, 1, 0, 1), (0, 3, 0, 1), (0, 1, 2**31 - 1, 2)]:
        with pytest.raises(TkError) as e:
            sess.kv_copy(*args)
        assert e.value.code == TK_ERROR_INVALID_ARGUMENT, args
    after = _read_all(sess, hp, max_ctx)
    for key in before:
        assert np.array_equal(before[key][0], after[key][0]) and np.array_equal(before[key][1], after[key][1])
    sess.close()
    model.close()


# ---- 2. keep: one runner, turn to turn ------------------------------------------------------------------------------------------------

def test_a_runner_keeps_the_rows_its_slot_already_holds(gpu):
    """P+X, P+Y, P+Y again, P alone (|P| = 100 bytes, X != Y from their first byte), 12 greedy tokens after each: the ids of every turn equal a
    cache-off runner's; kept = 0, 1 + |P|, n - 1, n - 1; batch_stats' rows fall by exactly the kept rows."""
    hs = Handles(gpu)
    P, X, Y = text(100, 0), text(9, 1), text(11, 2)
    assert X[0] != Y[0] and len(P) == 100
    script = [P + X, P + Y, P + Y, P]
    want_kept = [0, 1 + len(P), n_ids(P + Y) - 1, n_ids(P) - 1]
    r_off, r_on = hs.runner(hs.off), hs.runner(hs.on)
    kept_total = 0
    for turn, prompt in enumerate(script):
        want = generate(r_off, prompt)
        got = generate(r_on, prompt)
        assert len(want) == NTOK and got == want, f"turn {turn}: the cache changed a token"
        assert r_on.last_prompt_rows() == (n_ids(prompt), want_kept[turn], 0), turn
        assert r_off.last_prompt_rows() == (n_ids(prompt), 0, 0), turn
        kept_total += want_kept[turn]
    _, rows_off, _ = gpu.ModelLoader.batch_stats(hs.off)
    _, rows_on, _ = gpu.ModelLoader.batch_stats(hs.on)
    assert rows_off == sum(n_ids(p) for p in script) + NTOK * len(script)
    assert rows_off - rows_on == kept_total > 0
    assert gpu.ModelLoader.prefix_cache_stats(hs.on) == (sum(n_ids(p) for p in script), kept_total, 0, 0)
    assert gpu.ModelLoader.prefix_cache_stats(hs.off)[1:] == (0, 0, 0)
    # switched off again: the next prompt is recomputed from position 0, same tokens
    gpu.ModelLoader.set_prefix_cache(hs.on, False)
    assert generate(r_on, P + Y) == generate(r_off, P + Y)
    assert r_on.last_prompt_rows() == (n_ids(P + Y), 0, 0)
    hs.close()


# ---- 3. generated rows are cache rows like any other ----------------------------------------------------------------------------------

def _usable(piece):
    """a piece that tokenises back to the token it came from: one ASCII byte of the byte vocabulary (multi-byte display pieces of the upper
    vocabulary, " t300", would come back as five byte tokens)"""
    return isinstance(piece, bytes) and len(piece) == 1 and 0 < piece[0] < 128


def test_generated_rows_are_kept_too(gpu):
    """prompt Q, 8 generated pieces g, then the string Q + g[0..5] + Z is prepared: the rows of Q AND of the generated tokens are kept.  A
    generated piece can be put back into a prompt only when it is a single ASCII byte (the tiny model's vocabulary is half display pieces
    that do not round-trip), so of several candidate prompts the one whose generation starts with the most such pieces is taken, its j
    leading usable pieces (at most 6) are appended, and kept >= 1 + |Q| + j with j >= 1 is required; ids equal cache off."""
    hs = Handles(gpu)
    r_off, r_on = hs.runner(hs.off), hs.runner(hs.on)
    best_q, best_j, best_g = None, -1, None
    for i in range(48):                                             # the cache-off runner picks the prompt: the yardstick path
        q = "candidate %d: %s" % (i, text(20, 50 + i))
        g = generate(r_off, q, 8)
        assert len(g) == 8
        j = 0
        while j < 6 and _usable(g[j]):
            j += 1
        if j > best_j:
            best_q, best_j, best_g = q, j, g
    print("generated pieces that round-trip: j =", best_j, "for", repr(best_q), best_g)
    assert best_j >= 1, "no candidate prompt makes the tiny model start with an ASCII byte: choose other candidates"
    assert generate(r_on, best_q, 8) == best_g
    first_other = best_g[best_j]
    z = "Z tail" if first_other != b"Z" else "Y tail"             # Z differs from the piece generated next: the match ends where Z begins
    follow = best_q + b"".join(best_g[:best_j]).decode("ascii") + z
    want = generate(r_off, follow)
    got = generate(r_on, follow)
    assert got == want and len(want) == NTOK
    n, kept, copied = r_on.last_prompt_rows()
    print("follow-up prompt rows, kept, copied:", n, kept, copied)
    assert n == n_ids(follow) and copied == 0
    assert kept >= 1 + len(best_q) + best_j
    assert kept == 1 + len(best_q) + best_j                         # and no further: Z is not what was generated
    hs.close()


# ---- 4. copy: runner to runner ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("len_y", [9, 24])
def test_a_runner_copies_the_rows_another_slot_holds(gpu, len_y):
    """A prepares P+X (|P| = 320 bytes: more than one 256-row pass, k_attention_prefill from position 128), then B prepares P+Y: B copies
    1 + |P| rows and keeps none.  Then A prepares P+Y+W (W's first byte is not what B generated first, so the match with B ends at Y): A
    keeps its own 1 + |P| rows and copies the |Y| rows B holds beyond them when |Y| >= 16, nothing when |Y| < 16.  Ids equal cache off."""
    hs = Handles(gpu)
    P, X, Y = text(320, 3), text(13, 4), text(len_y, 5)
    assert X[0] != Y[0]
    a_off, b_off, a_on, b_on = hs.runner(hs.off), hs.runner(hs.off), hs.runner(hs.on), hs.runner(hs.on)
    want_a1, want_b = generate(a_off, P + X), generate(b_off, P + Y)
    assert len(want_a1) == NTOK and len(want_b) == NTOK
    W = ("w" if want_b[0] != b"w" else "v") + text(6, 6)
    want_a2 = generate(a_off, P + Y + W)
    assert generate(a_on, P + X) == want_a1
    assert a_on.last_prompt_rows() == (n_ids(P + X), 0, 0)
    assert generate(b_on, P + Y) == want_b
    assert b_on.last_prompt_rows() == (n_ids(P + Y), 0, 1 + len(P))
    assert generate(a_on, P + Y + W) == want_a2
    assert a_on.last_prompt_rows() == (n_ids(P + Y + W), 1 + len(P), len_y if len_y >= 16 else 0)
    rows, kept, copied, launches = gpu.ModelLoader.prefix_cache_stats(hs.on)
    assert (rows, kept, copied) == (n_ids(P + X) + n_ids(P + Y) + n_ids(P + Y + W), 1 + len(P), 1 + len(P) + (len_y if len_y >= 16 else 0))
    assert launches == (2 if len_y >= 16 else 1)
    _, rows_off, _ = gpu.ModelLoader.batch_stats(hs.off)
    _, rows_on, _ = gpu.ModelLoader.batch_stats(hs.on)
    assert rows_off - rows_on == kept + copied
    hs.close()


# ---- 5. under load ---------------------------------------------------------------------------------------------------------------------

def _load_script(hs, h):
    K, TURNS = 8, 3
    pre = text(150, 7)
    runners = [hs.runner(h, random_seed=1234 + i) for i in range(K)]
    runners[1].set_sampling(0.8)
    out = [[None] * TURNS for _ in range(K)]

    def drive(i):
        for t in range(TURNS):
            prompt = pre + " runner %d %s turn %d %s" % (i, "ab" * i, t, text(5 + i, 20 + t))
            out[i][t] = generate(runners[i], prompt, grammar=(i == 0))
    th = [threading.Thread(target=drive, args=(i,)) for i in range(K)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    return out


def test_eight_runners_on_eight_threads_get_the_cache_off_tokens(gpu):
    """8 runners, 8 threads, three turns each, a common 150-byte preamble + a tail of their own; runner 0 under the tool grammar, runner 1
    with the stochastic sampler and a fixed seed.  Every runner's pieces per turn equal what the same script gave with the cache off."""
    hs = Handles(gpu, slots=8)
    want = _load_script(hs, hs.off)
    got = _load_script(hs, hs.on)
    assert all(w is not None for ws in want for w in ws)
    assert got == want
    rows, kept, copied, launches = gpu.ModelLoader.prefix_cache_stats(hs.on)
    passes, _, _ = gpu.ModelLoader.batch_stats(hs.on)
    print("under load: prompt rows, kept, copied, copy launches, passes:", rows, kept, copied, launches, passes)
    assert kept + copied <= rows
    assert copied > 0
    assert 0 < launches <= passes
    assert gpu.ModelLoader.prefix_cache_stats(hs.off)[1:] == (0, 0, 0)
    hs.close()


# ---- 6. off is off ---------------------------------------------------------------------------------------------------------------------

def test_never_switched_on_nothing_is_kept_or_copied(gpu):
    loader = gpu.ModelLoader()
    h = loader.load("synthetic://tiny?seed=4", force_reload=True)
    a, b = gpu.LlmRunner(h, context_size=CTX), gpu.LlmRunner(h, context_size=CTX)
    P = text(60, 8)
    script = [(a, P + " one"), (b, P + " one"), (a, P + " one"), (b, P + " two")]
    for r, prompt in script:
        assert len(generate(r, prompt)) == NTOK
        assert r.last_prompt_rows() == (n_ids(prompt), 0, 0)
    assert gpu.ModelLoader.prefix_cache_stats(h) == (sum(n_ids(p) for _, p in script), 0, 0, 0)
    _, rows, _ = gpu.ModelLoader.batch_stats(h)
    assert rows == sum(n_ids(p) for _, p in script) + NTOK * len(script)
    a.close()
    b.close()
    loader.unload(h)
    loader.close()


# ---- 7. full size ----------------------------------------------------------------------------------------------------------------------

def test_full_7b_second_prompt_keeps_its_prefix(gpu):
    """synthetic://mistral-7b (32 layers, 8 KV heads, 128-wide rows): a 300-byte prompt, then the same prompt with its last 20 bytes changed,
    16 ids each, equal to cache off; a second runner that sends the first prompt again copies it."""
    p1 = text(300, 9)
    p2 = p1[:280] + text(20, 10)
    assert p1[280] != p2[280]
    loader = gpu.ModelLoader()
    want = []
    h = loader.load("synthetic://mistral-7b?seed=4", force_reload=True)
    r = gpu.LlmRunner(h, context_size=CTX)
    for p in (p1, p2, p1):
        want.append(generate(r, p, 16))
        assert len(want[-1]) == 16
    r.close()
    loader.unload(h)
    h = loader.load("synthetic://mistral-7b?seed=4", force_reload=True)
    gpu.ModelLoader.set_prefix_cache(h, True)
    r, r2 = gpu.LlmRunner(h, context_size=CTX), gpu.LlmRunner(h, context_size=CTX)
    assert generate(r, p1, 16) == want[0]
    assert r.last_prompt_rows() == (301, 0, 0)
    assert generate(r, p2, 16) == want[1]
    assert r.last_prompt_rows() == (301, 281, 0)
    assert generate(r2, p1, 16) == want[2]                          # slot 0 now holds p2: 281 rows of p1 are there to copy
    assert r2.last_prompt_rows() == (301, 0, 281)
    r.close()
    r2.close()
    loader.unload(h)
    loader.close()
