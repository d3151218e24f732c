"""CPU: Q5_K (GGML type 13) — the NumPy codec against hand-computed blocks, and the GGUF reader's size checks for the type."""
import ctypes as C
import struct

import numpy as np

import gguf_util as G
import oracle_lib as O
import q5k_ref as R


def probe(path):
    import trackiellm_amd as tk
    hp = tk.LlmHParams()
    nv = C.c_int32(0)
    return tk.lib().tk_mi355x_gguf_probe(path.encode(), C.byref(hp), C.byref(nv))


def hand_block():
    b = np.zeros(176, np.uint8)
    b[0:2] = np.array([0.5], np.float16).view(np.uint8)     # d
    b[2:4] = np.array([0.25], np.float16).view(np.uint8)    # dmin
    b[4] = 3; b[8] = 2                                      # sub-block 0: sc 3, m 2
    b[5] = 63 | 0x40; b[9] = 63                             # sub-block 1: sc 63, m 63 (bit 6 of byte 5 is sub-block 5's sc high bits)
    b[13] = 0x01                                            # sub-block 5: sc = 1 | (1 << 4) = 17, m 0
    b[16 + 0] = 0x01 | 0x02 | 0x20                          # qh[0]: high bit of weights 0, 32, 160
    b[48 + 0] = 0x7F                                        # qs[0]: weight 0 low 15, weight 32 low 7
    b[48 + 64] = 0x90                                       # qs[64]: weight 128 low 0, weight 160 low 9
    return b


def test_codec_decodes_hand_computed_block():
    q = R.quants(hand_block())[0]
    assert (q[0], q[32], q[128], q[160], q[1]) == (31, 23, 0, 25, 0)
    w = R.dequant(hand_block())[0]
    assert w[0] == 0.5 * 3 * 31 - 0.25 * 2 and w[1] == -0.5                  # 46.0, then q = 0: -dmin m
    assert w[32] == 0.5 * 63 * 23 - 0.25 * 63 and w[160] == 0.5 * 17 * 25
    assert w[128] == 0.0 and w[200] == 0.0


def q8_rows(x):
    qs, ds, bs = zip(*[O.q8k_quantize(r) for r in x])
    return np.stack(qs), np.stack(ds), np.stack(bs)


def test_numpy_matvec_restatement_equals_the_oracle_on_q4k_blocks():
    """the NumPy Q5_K mat-vec (tests/q5k_ref.py, the reference of the GPU probe tests) on Q4_K blocks re-encoded with qh = 0 gives
    oracle_lib.gemv_q8's Q4_K bits, K-split included"""
    rng = np.random.default_rng(5)
    rows, K = 64, 2048
    w = (rng.standard_normal((rows, K)) * 0.02).astype(np.float32)
    b4 = O.quantize_rows(O.TYPE_Q4_K, w)
    x = rng.standard_normal((3, K)).astype(np.float32)
    q8, d8, bs = q8_rows(x)
    for ks in (1, 4):
        got = R.gemv(R.q4k_to_q5k(b4), rows, K, ks, q8, d8, bs)
        for r in range(3):
            want = O.gemv_q8(O.TYPE_Q4_K, b4, rows, K, ks, x[r])
            assert np.array_equal(got[r].view(np.uint32), want.view(np.uint32)), (ks, r)


def mixed_gguf(path):
    """a tiny llama GGUF whose attn_v / ffn_down of layer 0 are Q5_K (the Q4_K_S pattern), beside Q4_K and Q6_K tensors"""
    cfg = O.tiny_config()
    orc = O.OracleLlm(cfg, seed=4)

    class Q5(object):
        def get_tensor(self, layer, which):
            t, buf = orc.get_tensor(layer, which)
            if layer == 0 and which in (3, 8) and t == 12:
                return 13, R.q4k_to_q5k(buf)
            return t, buf
    G.write_llama_gguf(path, Q5(), cfg)


def test_gguf_reader_refuses_short_q5k_data(tmp_path):
    p = str(tmp_path / "short.gguf")
    mixed_gguf(p)
    raw = bytearray(open(p, "rb").read())
    # the last tensor of the file is blk.1.ffn_down; make layer 0's Q5_K ffn_down claim a K that runs past the end of the file
    name = G._s("blk.0.ffn_down.weight")
    at = raw.index(name) + len(name)
    assert struct.unpack_from("<I", raw, at)[0] == 2
    dims_at, type_at = at + 4, at + 4 + 16
    assert struct.unpack_from("<I", raw, type_at)[0] == 13
    b = bytearray(raw)
    struct.pack_into("<QQ", b, dims_at, 512 * 64, 256)   # 64x the columns: the block count times 176 B exceeds the data region
    (tmp_path / "short_q5k.gguf").write_bytes(bytes(b))
    assert probe(str(tmp_path / "short_q5k.gguf")) == 3004
    b = bytearray(raw)
    struct.pack_into("<QQ", b, dims_at, 1 << 63, 4)       # element count wraps
    (tmp_path / "wrap_q5k.gguf").write_bytes(bytes(b))
    assert probe(str(tmp_path / "wrap_q5k.gguf")) == 3004
    b = bytearray(raw)
    struct.pack_into("<QQ", b, dims_at, 1 << 40, 1 << 8)  # does not wrap, describes far more than the file holds
    (tmp_path / "huge_q5k.gguf").write_bytes(bytes(b))
    assert probe(str(tmp_path / "huge_q5k.gguf")) == 3004
