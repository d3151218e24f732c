"""GPU: the Q8_0 KV cache where its saving counts — windows of thousands of positions, many sequences — and at every head geometry.

  1. one production attention launch (tk_mi355x_kv_q8_probe, device 0) in windows of 4099 .. 32 768 positions against the host loop (device -1),
     bit for bit, on general (lossy) rows; tests/test_kv_q8_cpu.py shows on the host loop alone that the deep positions of these very rows count;
  2. every instantiation of k_attention_far<.., true> the launcher can select is launched, compared, and named in a literal;
  3. Q8_0 sessions in the windows of tests/test_attention_far_gpu.py against the oracle and an F16 session, on rows that quantise without loss;
  4. a Q8_0 cache whose int8 arrays exceed 2^31 bytes;
  5. k_kv_copy_rows_q8 at every head geometry (2, 4, 6 and 8 scales per row), odd starts and counts, and under a runner's prefix cache at head_dim 256.

The comparisons are exact throughout: uint32 for outputs and logits, array_equal for cache rows."""
import numpy as np
import pytest

import attention_geometry_cases as G
import kv_q8_ref as R
import oracle_lib as O
from gguf_util import write_llama_gguf
from test_attention_far_gpu import edge_positions, pool_rows
from test_kv_q8_cpu import DEEP_KEY_EXPONENTS, seeded_rows
from test_kv_q8_gpu import Rig, bits, generate, run_lossless_pass

pytestmark = pytest.mark.gpu

TK_ERROR_INVALID_ARGUMENT = 1001

# ---- 1 and 2. the probe in deep windows; every instantiation ---------------------------------------------------------------------------------------

# the host loop's fused multiply-adds per case, counted: n_head * head_dim * 2 * sum over the rows of every pass of (position + 1).  A deep case has
# passes of 1 row (3 of them), 9 rows (2) and 256 rows (1), R.probe_passes; with window W and the deep chunk edge E that sum is 4 W + 7 E + 31 429
HOST_FMAS = {
    "g4_d256_w6144": 1.19e9,    # 96 325 positions x 24 heads x 256 x 2
    "g2_d128_w8448": 0.44e9,    # 105 541 x 16 x 128 x 2
    "g4_d64_w8448": 0.44e9,     # 105 541 x 32 x 64 x 2
    "g4_d192_w4099": 0.24e9,    # 75 153 x 8 x 192 x 2
    "g1_d256_w4100": 0.31e9,    # 75 157 x 8 x 256 x 2
    "g2_d128_w32768": 0.14e9,   # 2 rows, at 32 767 and 31: 32 800 x 16 x 128 x 2
    "g2_d256_6kv_rows171": 0.2e9, "mistral_rows64": 0.2e9, "mistral_rows129": 0.2e9,   # windows of 260 positions
}

# (plan gq, head_dim class, plan chunk) of every k_attention_far<GQ, HD, CH, true> that tk_attention_plan_q8 can name on 256 CUs, by hand from its rules
# (gq = 2 for a group of 4 with 2 * head_dim % 256 == 0 while rows * n_kv_head < 512; 32-position slots once n_head / gq * rows > 1024), rows 1 .. 256:
#   g4_d64       32 / 8 / 64    gq 4;                           8 * rows > 1024 from 129 rows                  (4, 64, 64) (4, 64, 32)
#   g2_d128      16 / 8 / 128   gq 2;                           8 * rows > 1024 from 129 rows                  (2, 128, 64) (2, 128, 32)
#   g1_d256       8 / 8 / 256   gq 1;                           8 * rows > 1024 from 129 rows                  (1, 0, 64) (1, 0, 32)
#   g2_d256       8 / 4 / 256   gq 2;                           4 * rows <= 1024                               (2, 0, 64)
#   g2_d256_6kv  12 / 6 / 256   gq 2;                           6 * rows > 1024 from 171 rows                  (2, 0, 64) (2, 0, 32)
#   g4_d256      24 / 6 / 256   gq 2 to 85 rows (12 * 85 = 1020), then gq 4; 6 * rows > 1024 from 171 rows     (2, 0, 64) (4, 0, 64) (4, 0, 32)
#   g4_d192       8 / 2 / 192   gq 4 (384 % 256 != 0);          2 * rows <= 1024                               (4, 0, 64)
#   Mistral      32 / 8 / 128   gq 2 to 63 rows (16 * 63 = 1008), then gq 4; 8 * rows > 1024 from 129 rows     (2, 128, 64) (4, 128, 64) (4, 128, 32)
# — all twelve distinct kernels of k_attention_far_q8_fns
Q8_INSTANTIATIONS = {(1, 0, 32), (1, 0, 64), (2, 0, 32), (2, 0, 64), (2, 128, 32), (2, 128, 64), (4, 0, 32), (4, 0, 64), (4, 64, 32), (4, 64, 64), (4, 128, 32), (4, 128, 64)}

SEEN = {}     # instantiation -> the (case, width) passes whose launch was compared with the host loop
DONE = set()  # cases run in this process


def run_probe_case(gpu, name):
    """every pass of one case: the launch against the host loop as uint32, output written, the cache arrays unchanged"""
    geometry, W = (R.SMALL_PROBE[name][0], R.SMALL_WINDOW) if name in R.SMALL_PROBE else R.DEEP_PROBE[name]
    nh, nkv, hd = geometry
    cache = R.general_cache(geometry, W)
    assert cache[0].shape == (1, R.DEEP_SEQS, nkv, W, hd) and cache[0].size <= 2 ** 31
    before = [a.copy() for a in cache]
    fmas = 0
    for i, (seq, pos) in enumerate(R.probe_passes(name)):
        width = seq.size
        assert seq.max() < R.DEEP_SEQS - 1 and pos.max() < W   # the last sequence is nobody's
        plan = gpu.attention_plan(width, nh, nkv, hd, W, kv_type=gpu.KV_Q8_0)
        assert plan[0] == 6 and plan[2] in (32, 64) and plan[3] == 2, (name, width, plan)
        q = R.probe_q(name, i, width, nh, hd)
        host = gpu.kv_q8_attention_probe(*cache, seq, pos, q, device=-1, fill=np.float32(-77.0))
        dev = gpu.kv_q8_attention_probe(*cache, seq, pos, q, device=0, fill=np.float32(-77.0))
        bad = np.flatnonzero((bits(host) != bits(dev)).reshape(width, -1).any(axis=1))
        assert bad.size == 0, (name, width, plan, [(int(r), int(pos[r])) for r in bad[:8]], float(np.abs(host - dev).max()))
        assert np.isfinite(dev).all() and (dev != -77.0).all() and np.isfinite(host).all() and (host != -77.0).all()
        SEEN.setdefault((plan[1], R.hd_class(hd), plan[2]), []).append((name, width))
        fmas += nh * hd * 2 * int((pos.astype(np.int64) + 1).sum())
    assert all(np.array_equal(a, b) for a, b in zip(cache, before)), name   # the launch only reads: sequence 2 and every other row
    print("%s: %.3g host fmas" % (name, fmas))
    assert fmas <= HOST_FMAS[name], (name, fmas)
    DONE.add(name)


@pytest.mark.parametrize("name", list(R.DEEP_PROBE))
def test_attention_launch_equals_the_host_loop_in_deep_windows(gpu, name):
    """general rows (key scale R.DEEP_K_SCALE = 0.6), 3 sequences; passes of 1, 9 and 256 rows with rows at the window's last position, at
    window - 2, at E - 1, E, E + 1 for a chunk edge E = 64 * 61 or 64 * 90 (slot 122 or 180 of the 32-position form), and short contexts beside
    them in the same pass; 4 deep rows at most in the wide pass.  Window 32 768: 2 rows, at 32 767 and at 31"""
    run_probe_case(gpu, name)


@pytest.mark.parametrize("name", list(R.SMALL_PROBE))
def test_attention_launch_equals_the_host_loop_where_no_deep_pass_goes(gpu, name):
    """windows of 260 positions at the widths that take the three instantiations the deep passes leave out: <2, 0, 32> (12 / 6 / 256 from 171
    rows), <4, 128, 64> and <4, 128, 32> (32 / 8 / 128 — no geometry of the table is a group of 4 at head_dim 128 — at 64 and 129 rows)"""
    run_probe_case(gpu, name)


def test_every_q8_instantiation_is_launched_and_compared(gpu):
    # the two rules restated, over every pass width: the literal is what they reach
    reach = set()
    for nh, nkv, hd in list(G.GEOMETRIES.values()) + [R.MISTRAL]:
        for rows in range(1, 257):
            gq = nh // nkv
            if gq == 4 and (2 * hd) % 256 == 0 and rows * nkv < 512:
                gq = 2
            reach.add((gq, R.hd_class(hd), 32 if (nh // gq) * rows > 1024 else 64))
    assert reach == Q8_INSTANTIATIONS
    for name in list(R.DEEP_PROBE) + list(R.SMALL_PROBE):   # run alone, this test runs the cases itself
        if name not in DONE:
            run_probe_case(gpu, name)
    if gpu.lib().tk_mi355x_device_cu_count(0) == 256:
        assert set(SEEN) == Q8_INSTANTIATIONS, (sorted(Q8_INSTANTIATIONS - set(SEEN)), sorted(set(SEEN) - Q8_INSTANTIATIONS))
        deep = {k for k, v in SEEN.items() if any(n in R.DEEP_PROBE for n, _ in v)}
        assert deep == Q8_INSTANTIATIONS - {(2, 0, 32), (4, 128, 64), (4, 128, 32)}, sorted(deep)


# ---- 3. Q8_0 sessions in deep windows ---------------------------------------------------------------------------------------------------------------

def quantised(rows):
    return R.quantize(rows[0]) + R.quantize(rows[1])   # (k, v) f16 bits -> (kq, kd, vq, vd)


def same_rows(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got, want))


class DeepQ8:
    """one geometry in one window beyond its resident limit, attn_k and attn_v zero: a Q8_0 session, an F16 session and the oracle, 17 sequences;
    lossless rows from a pool of G.POOL positions (keys with exponents of their own), a new offset per load"""
    SEQS = 17

    def __init__(self, gpu, geometry, window, key_exponents=(-10, -4)):
        self.gpu, self.window = gpu, window
        self.rig = Rig(gpu, geometry, True)
        hp = self.hp = self.rig.hp
        self.geom = (hp.n_head, hp.n_kv_head, hp.head_dim)
        self.limit = gpu.attention_resident_limit(*self.geom)
        assert self.limit < window
        self.q8 = self.rig.session(self.SEQS, window, gpu.KV_Q8_0)
        self.trio = (self.q8, self.rig.session(self.SEQS, window, gpu.KV_F16), self.rig.oracle(self.SEQS, window))
        self.orc = self.trio[2]
        self.kpool = R.lossless_rows((G.POOL, hp.n_kv_head, hp.head_dim), 1, exponents=key_exponents)
        self.vpool = R.lossless_rows((G.POOL, hp.n_kv_head, hp.head_dim), 2)
        self.salt = 0

    def rows(self, seq, n):
        self.salt += 1
        idx = (53 * seq + 7 * self.salt + np.arange(n)) % G.POOL
        return self.kpool[idx], self.vpool[idx]

    def load(self, seq, n, into=None):
        kv = self.rows(seq, n)
        for x in into or self.trio:
            x.kv_write(0, seq, 0, *kv)
        return kv

    def deep_positions_count(self):
        """through the oracle alone: at the window's last position, another lossless V row at pos - 1, and then at pos // 2, changes the logits' bits"""
        pos = self.window - 1
        k, v = self.rows(0, self.window)
        tok = np.array([41], np.int32)
        self.orc.kv_write(0, 0, 0, k, v)
        base, _ = self.orc.forward([0], [pos], tok)
        for at in (pos - 1, pos // 2):
            other = v.copy()
            other[at] = v[at - 7]   # another row of the pool
            assert not np.array_equal(other[at], v[at])
            self.orc.kv_write(0, 0, 0, k, other)
            moved, _ = self.orc.forward([0], [pos], tok)
            assert (bits(moved) != bits(base)).any(), (self.geom, self.window, "the V row at", at, "does not reach the logits")

    def bystander(self, seq):
        """general rows over a whole window of the Q8_0 session: what kv_write left is what the pass must leave"""
        self.salt += 1
        rows = pool_rows(self.geom[1], self.geom[2], 11 * seq + self.salt, self.window)
        self.q8.kv_write(0, seq, 0, *rows)
        snap = self.q8.kv_read_q8(0, seq, 0, self.window)
        assert same_rows(snap, quantised(rows)), (self.geom, "kv_write over the window")
        return snap

    def check_after(self, appended, kept, by, snap, what):
        """appended {sequence: (first position, count)}: those rows are the quantised zero rows, the row behind them still holds its preloaded bits,
        the bystander is unchanged"""
        for s, (p0, n) in appended.items():
            got = self.q8.kv_read_q8(0, s, p0, n)
            assert not any(a.any() for a in got), (what, s, "appended rows")
            if p0 + n < kept[s][0].shape[0]:
                got = self.q8.kv_read_q8(0, s, p0 + n, 1)
                assert same_rows(got, quantised((kept[s][0][p0 + n:p0 + n + 1], kept[s][1][p0 + n:p0 + n + 1]))), (what, s, "the row behind")
            if p0 > 0:
                got = self.q8.kv_read_q8(0, s, p0 - 1, 1)
                assert same_rows(got, quantised((kept[s][0][p0 - 1:p0], kept[s][1][p0 - 1:p0]))), (what, s, "the row before")
        assert same_rows(self.q8.kv_read_q8(0, by, 0, self.window), snap), (what, "bystander")

    def plan(self, rows):
        plan = self.gpu.attention_plan(rows, *self.geom, self.window, kv_type=self.gpu.KV_Q8_0)
        assert plan[0] == 6
        return plan

    def decode_pass(self, pos, what):
        """row i = sequence i at pos[i]; the sequence behind the last one is the bystander"""
        pos = np.asarray(pos, np.int32)
        n = pos.size
        seq = np.arange(n, dtype=np.int32)
        tok = np.random.default_rng([n, int(pos[0])]).integers(3, G.MODEL["vocab"], n).astype(np.int32)
        kept = {s: self.load(s, min(int(pos[s]) + 2, self.window)) for s in range(n)}
        snap = self.bystander(n)
        self.plan(n)
        run_lossless_pass(self.rig, self.trio, seq, pos, tok, {}, what)
        self.check_after({s: (int(pos[s]), 1) for s in range(n)}, kept, n, snap, what)

    def chunk_passes(self, rows, what):
        """`rows` consecutive positions of sequence 0 ending at the window's last position: as a prompt chunk through forward in all three, then
        through forward_verify in the session's own form and in the per-row form, whose logits are the oracle's and whose picks are equal"""
        top = self.window - 1
        pos = np.arange(top - rows + 1, top + 1, dtype=np.int32)
        seq = np.zeros(rows, np.int32)
        tok = np.random.default_rng([rows, top]).integers(3, G.MODEL["vocab"], rows).astype(np.int32)
        appended = {0: (int(pos[0]), rows)}
        kept = {0: self.load(0, self.window)}
        snap = self.bystander(1)
        self.plan(rows)
        run_lossless_pass(self.rig, self.trio, seq, pos, tok, {}, (what, "forward"))
        self.check_after(appended, kept, 1, snap, (what, "forward"))
        want, wid = self.orc.forward(seq, pos, tok)   # the rows of the pass are zero rows again: the same logits
        picks = {}
        for form in (-1, 0):
            self.q8.kv_write(0, 0, 0, *kept[0])
            got, picks[form] = self.q8.forward_verify(seq, pos, tok, form=form)
            assert np.array_equal(bits(got), bits(want)), (what, "forward_verify", form, float(np.abs(got - want).max()))
            self.check_after(appended, kept, 1, snap, (what, "forward_verify", form))
        assert np.array_equal(picks[-1], picks[0]) and np.array_equal(picks[0], wid), what

    def close(self):
        self.rig.close()


DEEP_SESSIONS = {   # the windows of tests/test_attention_far_gpu.py; the deepest one with key rows of small exponents (scales down to 2^-14)
    "g4_d256_w6144": ("g4_d256", 6144, (-10, -4)),
    "mistral_w8448": (R.MISTRAL, 8448, (-10, -4)),
    "g4_d64_w9472": ("g4_d64", 9472, DEEP_KEY_EXPONENTS),
}


@pytest.fixture(scope="module", params=list(DEEP_SESSIONS))
def deep_q8(request, gpu):
    geometry, window, key_exponents = DEEP_SESSIONS[request.param]
    d = DeepQ8(gpu, geometry, window, key_exponents)
    yield request.param, d
    d.close()


def test_deep_positions_reach_the_oracles_logits(deep_q8):
    """the condition of the comparisons below, through the oracle alone: the default exponents of lossless_rows (-10 .. -4) do not collapse the
    softmax at these depths, nor do the smaller ones (-14 .. -10) the 9472-position window takes for its keys"""
    deep_q8[1].deep_positions_count()


def test_q8_session_equals_oracle_and_f16_session_in_deep_windows(deep_q8):
    """decode passes of 1, 9 and 16 rows at edge_positions (the resident limit - 1, the limit, limit + 1, the window's last position, then
    contexts short and long), a 16-position chunk ending at the window's last position through forward and through forward_verify: logits as
    uint32 and ids of the Q8_0 session, the oracle and the F16 session; after each pass the bystander, the appended rows and their neighbours"""
    name, d = deep_q8
    for rows in (1, 9, 16):
        d.decode_pass(edge_positions(d.limit, d.window, rows), (name, "decode", rows))
    d.chunk_passes(16, (name, "chunk of 16"))


# ---- 4. a Q8_0 cache above 2^31 bytes per array -----------------------------------------------------------------------------------------------------

def test_q8_cache_above_2_to_31_bytes(gpu):
    """1 layer, 32 / 8 / 128, window 32 768, 65 sequences: 65 x 8 x 32768 x 128 = 2^31 + 2^25 bytes per int8 array, so a value offset of sequence
    64 does not fit in 32 bits.  Sequences 0 and 64 hold the same lossless rows in their top 300 positions (attn_k and attn_v zero: the appended
    row is lossless too); one row of each at position 32 767 in one pass gives the same logits, those of a one-sequence oracle"""
    W, NSEQ, TOPN = 32768, 65, 300
    nh, nkv, hd = R.MISTRAL
    assert NSEQ * nkv * W * hd > 2 ** 31
    rig = Rig(gpu, R.MISTRAL, True)
    try:
        sess = rig.session(NSEQ, W, gpu.KV_Q8_0)
        f16_bytes = 2 * rig.hp.n_layer * NSEQ * W * nkv * hd * 2
        assert sess.kv_bytes() * 32 == f16_bytes * 17
        orc = rig.oracle(1, W)
        p0 = W - TOPN
        k, v = R.lossless_rows((TOPN, nkv, hd), 77), R.lossless_rows((TOPN, nkv, hd), 78)
        written = quantised((k, v))
        after_pass = [a.copy() for a in written]   # a pass at the window's last position leaves a zero row there
        for a in after_pass:
            a[-1] = 0
        tok = np.full(9, 41, np.int32)
        orc.kv_write(0, 0, p0, k, v)
        want, wid = orc.forward([0], [W - 1], tok[:1])

        def named_rows(got, ids, at, what):
            for r in at:
                assert np.array_equal(bits(got[r]), bits(want[0])), (what, r, float(np.abs(got[r] - want[0]).max()))
                assert ids[r] == wid[0], (what, r)
            for s in (0, 64):
                assert same_rows(sess.kv_read_q8(0, s, p0, TOPN), after_pass), (what, s)

        for s in (0, 64):
            sess.kv_write(0, s, p0, k, v)
        assert same_rows(sess.kv_read_q8(0, 64, p0, TOPN), written) and same_rows(sess.kv_read_q8(0, 0, p0, TOPN), written)
        assert gpu.attention_plan(2, nh, nkv, hd, W, kv_type=gpu.KV_Q8_0)[0] == 6
        got, ids = sess.forward([0, 64], [W - 1, W - 1], tok[:2])
        named_rows(got, ids, (0, 1), "two rows")
        # nine rows, short bystanders in between
        for s in (0, 64):
            sess.kv_write(0, s, p0, k, v)
        got, ids = sess.forward([0, 1, 2, 3, 4, 5, 6, 7, 64], [W - 1, 0, 1, 2, 3, 4, 5, 6, W - 1], tok)
        named_rows(got, ids, (0, 8), "nine rows")
        # sequence 63, next to it, was never written: all zero, values and scales
        for q0, n in ((0, 64), (p0, TOPN)):
            assert not any(a.any() for a in sess.kv_read_q8(0, 63, q0, n))
        # a copy near the top from sequence 64 onto sequence 1, whose 300 rows below hold general rows
        below = seeded_rows(TOPN, nkv, hd, 1.0, 5), seeded_rows(TOPN, nkv, hd, 1.0, 6)
        sess.kv_write(0, 1, p0 - TOPN, *below)
        sess.kv_copy(64, 1, p0, TOPN)
        assert same_rows(sess.kv_read_q8(0, 1, p0, TOPN), after_pass)
        assert same_rows(sess.kv_read_q8(0, 1, p0 - TOPN, TOPN), quantised(below))
        assert same_rows(sess.kv_read_q8(0, 64, p0, TOPN), after_pass)
        assert not any(a.any() for a in sess.kv_read_q8(0, 63, p0, TOPN)) and not any(a.any() for a in sess.kv_read_q8(0, 2, p0, TOPN))
    finally:
        rig.close()


# ---- 5. k_kv_copy_rows_q8 at every head geometry -----------------------------------------------------------------------------------------------------

COPY_WINDOW, COPY_SEQS = G.ODD_WINDOW, 4
# (src, dst, p0, n): one row, an odd start, an odd start and an odd count over more than one sweep — rows 7 .. 259, and 255 rows from 5 —, the window
COPIES = [(0, 1, 0, 1), (3, 2, 1, 1), (2, 0, 7, 253), (0, 3, 5, 255), (1, 3, 0, 261)]


@pytest.mark.parametrize("geometry", list(G.GEOMETRIES))
def test_kv_copy_at_every_head_geometry(gpu, geometry):
    """2 layers, 4 sequences of distinct general rows, window 261: after each copy the destination holds its rows with [p0, p0 + n) replaced by
    the source's in all four arrays of both layers, and nothing else moved.  Scales per row: 2, 4, 6 (rows of 12 bytes: scale runs are 4-byte
    aligned only) and 8.  253 rows at head_dim 256 are 4048 16-byte words a run, more than the 1024 words one workgroup sweeps.  255 rows from row 7
    would end one row behind the window: refused, with src == dst and a start at the window's end, and nothing changes"""
    nh, nkv, hd = G.GEOMETRIES[geometry]
    m = G.MODEL
    model = gpu.LlmModel(gpu.LlmHParams(2, m["d_model"], nh, nkv, hd, m["d_ff"], m["vocab"], 1e-5, 10000.0, 0, 0, 0, 0, 1)).fill_synthetic(4)
    sess = gpu.LlmSession(model, COPY_SEQS, COPY_WINDOW, kv_type=gpu.KV_Q8_0)
    try:
        state = {}
        for l in range(2):
            for s in range(COPY_SEQS):
                rows = seeded_rows(COPY_WINDOW, nkv, hd, (0.05, 1.0, 7.0, 0.6)[s], 10 * l + s), seeded_rows(COPY_WINDOW, nkv, hd, 1.0, 100 + 10 * l + s)
                sess.kv_write(l, s, 0, *rows)
                state[l, s] = [a.copy() for a in sess.kv_read_q8(l, s, 0, COPY_WINDOW)]
                assert same_rows(state[l, s], quantised(rows))

        def check(what):
            for (l, s), want in state.items():
                got = sess.kv_read_q8(l, s, 0, COPY_WINDOW)
                for name, a, b in zip(("kq", "kd", "vq", "vd"), got, want):
                    assert np.array_equal(a, b), (geometry, what, "layer", l, "sequence", s, name, np.argwhere(a != b)[:4].tolist())

        for src, dst, p0, n in COPIES:
            sess.kv_copy(src, dst, p0, n)
            for l in range(2):
                for a, b in zip(state[l, dst], state[l, src]):
                    assert not np.array_equal(a[p0:p0 + n], b[p0:p0 + n])
                    a[p0:p0 + n] = b[p0:p0 + n]
            check((src, dst, p0, n))
        for args in ((1, 1, 0, 4), (2, 0, 7, 255), (0, 1, 200, 62), (0, 1, 261, 1)):   # src == dst; n > window - p0
            with pytest.raises(gpu.TkError) as e:
                sess.kv_copy(*args)
            assert e.value.code == TK_ERROR_INVALID_ARGUMENT, (args, e.value.code)
        check("refusals")
    finally:
        sess.close()
        model.close()


def test_prefix_cache_copies_q8_rows_at_head_dim_256(gpu, tmp_path):
    """a two-layer GGUF of 8 / 4 / 256 as a Q8_0 model with the prefix cache on: a second runner's prompt rows are copied from the first one's slot
    (k_kv_copy_rows_q8 with 8 scales per row) and it says what the first one said, which is what a runner of the same model without the prefix
    cache says"""
    cfg = O.tiny_config(n_head=8, n_kv_head=4, head_dim=256)
    orc = O.OracleLlm(cfg, seed=4)
    path = str(tmp_path / "d256.gguf")
    write_llama_gguf(path, orc, cfg)
    orc.close()
    prompt = " ".join(["hello world"] * 12)   # bos and 24 pieces
    loader = gpu.ModelLoader()
    off, on = loader.load(path, force_reload=True), loader.load(path, force_reload=True)
    runners = []
    try:
        assert off.value != on.value
        for h in (off, on):
            gpu.ModelLoader.set_kv_cache_type(h, "q8_0")
        gpu.ModelLoader.set_prefix_cache(on, True)

        def run(h):
            r = gpu.LlmRunner(h, context_size=256)
            runners.append(r)
            r.set_logit_bias([2], [-np.inf])   # no EOS: every stream has its 24 tokens
            out = generate(r, prompt, cap=24)
            assert len(out[1]) == 24
            return r, out

        _, want = run(off)
        a, first = run(on)
        b, second = run(on)
        assert first == want and second == want
        rows, kept, copied = b.last_prompt_rows()
        assert rows == 25 and copied >= 16, (rows, kept, copied)
        assert gpu.ModelLoader.prefix_cache_stats(on)[2] >= copied
    finally:
        for r in runners:
            r.close()
        loader.unload(off)
        loader.unload(on)
        loader.close()
