"""Helpers shared by the k-quant GPU tests (test_q5k_gpu.py, test_q3k_gpu.py, test_q2k_gpu.py): the pieces that were the same text in each.
What differs between the files stays in them: test_q5k_gpu.py's check_widths (no finiteness assert) and the two q8_rows."""
import numpy as np

import oracle_lib as O


def oracle_cfg_from(hp, max_ctx, max_seq):
    return O.LlmConfig(n_layer=hp.n_layer, d_model=hp.d_model, n_head=hp.n_head, n_kv_head=hp.n_kv_head, head_dim=hp.head_dim,
                       d_ff=hp.d_ff, vocab=hp.vocab, max_ctx=max_ctx, max_seq=max_seq, rms_eps=hp.rms_eps, rope_theta=hp.rope_theta,
                       ks_qkv=hp.ks_qkv, ks_o=hp.ks_o, ks_gateup=hp.ks_gateup, ks_down=hp.ks_down, ks_out=hp.ks_out)


def shapes(cfg):
    D, QD, KVD, FF = cfg.d_model, cfg.n_head * cfg.head_dim, cfg.n_kv_head * cfg.head_dim, cfg.d_ff
    return {1: (QD, D), 2: (KVD, D), 3: (KVD, D), 4: (D, QD), 6: (FF, D), 7: (FF, D), 8: (D, FF)}


def install(model, src, n_layer):
    for which in (O.T_TOKEN_EMBD, O.T_OUT_NORM, O.T_OUTPUT):
        model.set_tensor(-1, which, *src.get_tensor(-1, which))
    for l in range(n_layer):
        for which in range(9):
            model.set_tensor(l, which, *src.get_tensor(l, which))


WIDTHS = [1, 2, 16, 24, 40, 128, 200, 256]


def check_widths(gpu, model, hp, orc, monkeypatch, tag):
    """logits and ids bit-identical to the oracle at every width in WIDTHS (and at 1, 2 rows with the producers as launches of their own),
    two positions through the KV cache"""
    rng = np.random.default_rng(11)
    for no_fuse in ("0", "1"):
        monkeypatch.setenv("TK_MI355X_NO_FUSE", no_fuse)
        for n in (WIDTHS if no_fuse == "0" else [1, 2]):
            sess = gpu.LlmSession(model, n, 8)
            orc.reset()
            seq = np.arange(n, dtype=np.int32)
            for p in range(2):
                tok = rng.integers(3, hp.vocab, n).astype(np.int32)
                pos = np.full(n, p, np.int32)
                want, wam = orc.forward(seq, pos, tok)
                got, gam = sess.forward(seq, pos, tok)
                assert np.isfinite(want).all() and np.isfinite(got).all(), (tag, n, p)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (tag, n, p, np.abs(got - want).max())
                assert np.array_equal(gam, wam), (tag, n, p)
            sess.close()


def logits_in_passes(gpu, model, hp, width, toks):
    """256 sequences, two positions, in passes of `width` rows (each pass its own slice of the sequences)"""
    sess = gpu.LlmSession(model, 256, 4)
    out = []
    for p in range(2):
        rows = []
        for r0 in range(0, 256, width):
            seq = np.arange(r0, r0 + width, dtype=np.int32)
            got, _ = sess.forward(seq, np.full(width, p, np.int32), toks[p][r0:r0 + width])
            rows.append(got.copy())
        out.append(np.concatenate(rows))
    sess.close()
    return out
