"""Attention at every head geometry the model loader accepts, against the oracle and BIT FOR BIT: the passes of attention_geometry_cases.py
(native groups of 1, 2 and 4 query heads per KV head; head_dim 64, 128 and the run-time head_dim instantiations at 192 and 256; ring slots of
32, 64 and 128 positions; fused and unfused; the narrow, tiled-prefill and long-context kernels; session windows of 260, 520 and 1024).

Per pass: logits as uint32, ids, and the cache — every sequence of the pass is read back from position 0 through the row AFTER the last one
the pass appends (the preloaded rows, the appended rows, the row behind them), and a bystander sequence next to the last one of the pass is
read back whole.  Which kernel a pass takes is the launcher's answer (tk_mi355x_attention_plan_at); on a 256-CU device it must be the
instantiation the case claims, on another device the results are compared all the same.

What test_attention_geometry_cpu.py shows without a GPU: the table names every reachable instantiation, and a comparison of this kind sees a
reordered partial-sum join and a dropped position in every case."""
import numpy as np
import pytest

import attention_geometry_cases as G
import oracle_lib as O
from gguf_util import write_llama_gguf
from test_llm_gpu import oracle_cfg_from

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def narrow_attention_even_when_sessions_share_the_device(monkeypatch):
    """several sessions of a geometry are alive at once, and with more than one on a device the launcher leaves the narrow kernel for the ring
    form; the table's claims are a lone runner's (the ring-only cases set 1 themselves)"""
    monkeypatch.setenv("TK_MI355X_NO_NARROW_ATT", "0")


class Rig:
    """one geometry's model, with its sessions and oracles by (window, sequences), made on first use"""

    def __init__(self, gpu, geometry):
        self.gpu, self.geometry = gpu, geometry
        nh, nkv, hd = G.GEOMETRIES[geometry]
        m = G.MODEL
        self.model = gpu.LlmModel(gpu.LlmHParams(m["n_layer"], m["d_model"], nh, nkv, hd, m["d_ff"], m["vocab"], 1e-5, 10000.0, 0, 0, 0, 0, 1)).fill_synthetic(4)
        self.hp = self.model.hparams
        assert (self.hp.n_head, self.hp.n_kv_head, self.hp.head_dim) == (nh, nkv, hd)
        self.sessions, self.oracles = {}, {}
        self.cus = gpu.lib().tk_mi355x_device_cu_count(0)

    def session(self, window, max_seq):
        if (window, max_seq) not in self.sessions:
            self.sessions[window, max_seq] = self.gpu.LlmSession(self.model, max_seq, window)
        return self.sessions[window, max_seq]

    def oracle(self, window, max_seq):
        if (window, max_seq) not in self.oracles:
            self.oracles[window, max_seq] = O.OracleLlm(oracle_cfg_from(self.hp, window, max_seq), seed=4)
        return self.oracles[window, max_seq]

    def close(self):
        for s in self.sessions.values():
            s.close()
        for o in self.oracles.values():
            o.close()
        self.model.close()


@pytest.fixture(scope="module", params=list(G.GEOMETRIES))
def rig(request, gpu):
    r = Rig(gpu, request.param)
    yield r
    r.close()


def check_plan(rig, case, p):
    """the launcher's own answer for this pass; on 256 CUs it is what the case claims to cover"""
    hp = rig.hp
    plan = rig.gpu.attention_plan(p["seq"].size, hp.n_head, hp.n_kv_head, hp.head_dim, case["window"], case["fused"], top_position=p["top"])
    if rig.cus == 256:
        assert all(w is None or g == w for g, w in zip(plan, case["plan"])), (case["name"], p["seq"].size, p["top"], plan, case["plan"])
    return plan


def run_pass(rig, sess, orc, case, p):
    geometry = rig.geometry
    window = case["window"]
    by = p["bystander"]
    bk, bv = G.kv_rows(geometry, 11 * by + 5, window)
    sess.kv_write(0, by, 0, bk, bv)
    for s, (off, n) in p["preload"].items():
        k, v = G.kv_rows(geometry, off, n)
        sess.kv_write(0, s, 0, k, v)
        orc.kv_write(0, s, 0, k, v)
    want, wam = orc.forward(p["seq"], p["pos"], p["tok"])
    got, gam = sess.forward(p["seq"], p["pos"], p["tok"])
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    assert bad.size == 0, (case["name"], [(int(r), int(p["seq"][r]), int(p["pos"][r])) for r in bad[:8]], float(np.abs(got - want).max()))
    assert np.array_equal(gam, wam), case["name"]
    for s, (off, n) in p["preload"].items():    # the rows loaded before the pass, the rows it appended, and the row behind them
        gk, gv = sess.kv_read(0, s, 0, n)
        wk, wv = orc.kv_read(0, s, 0, n)
        assert np.array_equal(gk, wk) and np.array_equal(gv, wv), (case["name"], s, n)
        mine = p["pos"][p["seq"] == s]
        if mine.max() + 1 < n:                  # the oracle agrees by construction; the row behind the last appended one is the preloaded one
            k, v = G.kv_rows(geometry, off, n)
            assert np.array_equal(gk[mine.max() + 1:], k[mine.max() + 1:]) and np.array_equal(gv[mine.max() + 1:], v[mine.max() + 1:])
    gk, gv = sess.kv_read(0, by, 0, window)
    assert np.array_equal(gk, bk) and np.array_equal(gv, bv), (case["name"], "bystander", by)


def run_group(rig, kind, monkeypatch, only=lambda case: True):
    """every case of a group: in the rig's session, or — a group with an environment of its own — in a fresh one (passes are captured per session)"""
    todo = [c for c in G.groups(rig.geometry).get(kind, []) if only(c)]
    if not todo:
        return 0
    env = todo[0]["env"]
    assert all(c["env"] == env and c["window"] == todo[0]["window"] for c in todo)
    window, nseq = todo[0]["window"], G.max_seq(todo[0])
    orc = rig.oracle(window, nseq)
    with monkeypatch.context() as mp:
        for name, value in env.items():
            mp.setenv(name, value)
        sess = rig.gpu.LlmSession(rig.model, nseq, window) if env else rig.session(window, nseq)
        try:
            for case in todo:
                for p in G.passes(case):
                    check_plan(rig, case, p)
                    run_pass(rig, sess, orc, case, p)
        finally:
            if env:
                sess.close()
    return len(todo)


@pytest.mark.parametrize("rows", ["up_to_128_rows", "above_128_rows"])
@pytest.mark.parametrize("window", list(G.WINDOWS))
def test_ragged_decode_passes_bit_exact(rig, window, rows, monkeypatch):
    """one decode row per sequence, the rows of a pass at the table's context lengths side by side, at 1, 2 and 16 rows, on both sides of every
    pass-width threshold of the geometry, and at 200 and 256 rows; in the 261-position window (no multiple of 4: the arrays behind the score array
    of the run-time head_dim layout start off a 16-byte boundary) at 2 and 200 rows"""
    n = run_group(rig, "decode_w%d" % window, monkeypatch, only=lambda c: (c["width"] <= 128) == (rows == "up_to_128_rows"))
    assert n >= (1 if window == G.ODD_WINDOW else 3 if rows == "up_to_128_rows" else 2)


def test_ring_form_where_the_narrow_kernel_would_run(rig, monkeypatch):
    """TK_MI355X_NO_NARROW_ATT=1: k_attention<2, fused, 128, 128> for a native group of 2 (other geometries have no narrow kernel to leave)"""
    assert run_group(rig, "decode_ring_only", monkeypatch) == len(G.DECODE_PLAN_RING_ONLY.get(rig.geometry, {}))


def test_multi_position_passes_bit_exact(rig, monkeypatch):
    """several new positions of each sequence in one pass, from 0, 31, 97 and 159 cached positions: the unfused k_attention instantiations below
    position 128, k_attention_prefill from there where it applies (head_dim 192 and 256 keep k_attention<*, unfused, 0, *>)"""
    assert run_group(rig, "unfused", monkeypatch) == 12


def test_multi_position_passes_in_the_per_row_form_bit_exact(rig, monkeypatch):
    """the same passes from 159 cached positions under TK_MI355X_NO_PREFILL_ATT=1: k_attention unfused over three to six ring slots"""
    assert run_group(rig, "unfused_per_row", monkeypatch) == 3


def test_long_context_form_bit_exact(rig, monkeypatch):
    """1, 4, 5 and 8 rows whose top position is 511, 512, 767, 768 or 1000 in a 1024-position window (head_dim 64 and 128): the long-context trio
    from its thresholds — 1 .. 4 rows from position 512, 5 .. 8 rows from 768 — and the fused kernels below them"""
    assert run_group(rig, "long", monkeypatch) == (len(G.LONG_CASES) if rig.geometry in G.LONG_GEOMETRIES else 0)


def test_fused_kernels_where_the_long_context_form_would_run_bit_exact(rig, monkeypatch):
    """the passes the long-context form takes, under TK_MI355X_NO_LONG_ATT=1: the ring walks 8 to 16 slots, the narrow kernel several chunks"""
    assert run_group(rig, "long_fused", monkeypatch) == (sum(G.LONG_CASES.values()) if rig.geometry in G.LONG_GEOMETRIES else 0)


def test_decode_over_700_and_1000_positions_at_head_dim_256_bit_exact(rig, monkeypatch):
    """where the long-context form does not apply (head_dim 256) a decode step over 700 and 1000 cached positions walks 11 and 16 ring slots"""
    assert run_group(rig, "deep", monkeypatch) == (len(G.DEEP_CASES) if rig.geometry in G.DEEP_GEOMETRIES else 0)


def test_head_dim_above_256_is_refused_at_create_and_at_load(gpu, tmp_path):
    """k_attention's value phase forms 256 dims per head: a wider head would compute something else, so the loader says no, naming the rule"""
    for nh, nkv, hd in ((1, 1, 512), (4, 1, 320), (2, 1, 384)):
        with pytest.raises(gpu.TkError) as e:
            gpu.LlmModel(gpu.LlmHParams(1, 256, nh, nkv, hd, 256, 512, 1e-5, 10000.0, 0, 0, 0, 0, 1))
        assert "head_dim must be at most 256" in str(e.value)
    cfg = O.tiny_config(n_layer=1, d_ff=256, n_head=1, n_kv_head=1, head_dim=512, max_ctx=8, max_seq=1)
    orc = O.OracleLlm(cfg, seed=4)
    path = str(tmp_path / "wide_head.gguf")
    write_llama_gguf(path, orc, cfg)
    orc.close()
    with pytest.raises(gpu.TkError) as e:
        gpu.LlmModel(gguf=path)
    assert "head_dim must be at most 256" in str(e.value)
