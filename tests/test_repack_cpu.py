"""CPU: the W4A8 tile bytes of every tiled type, pinned directly.  tk_mi355x_llm_repack_probe with device < 0 runs the repack's lane function
(tk_repack_lane, the body of the one k_repack kernel) in a host loop; its tiles are held, byte for byte, against tests/golden/repack_tiles.npz,
recorded on an MI355X from the per-type repack kernels that function replaced (tests/repack_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import repack_cases as RC
import trackiellm_amd.llm as L

INVALID = 1001  # TK_ERROR_INVALID_ARGUMENT


@pytest.mark.parametrize("ttype", RC.TYPES, ids=[RC.NAMES[t] for t in RC.TYPES])
def test_host_repack_matches_recorded_tiles(tk, ttype):
    want = RC.expected()[RC.NAMES[ttype]]
    assert want.shape == (RC.ROWS // 16, RC.K // 256, L.TILE_BYTES[ttype])
    got = tk.repack_probe(ttype, RC.blocks_of(ttype), RC.ROWS, RC.K, device=-1)
    assert RC.first_difference(got, want) is None, f"{RC.NAMES[ttype]}: {RC.first_difference(got, want)}"


def test_iq4_nl_tiles_are_the_q4_0_tiles_of_the_same_bytes(tk):
    b = RC.blocks_of(L.TYPE_IQ4_NL)
    assert np.array_equal(b, RC.blocks_of(L.TYPE_Q4_0))
    nl, q40 = (tk.repack_probe(t, b, RC.ROWS, RC.K, device=-1) for t in (L.TYPE_IQ4_NL, L.TYPE_Q4_0))
    assert RC.first_difference(nl, q40) is None, RC.first_difference(nl, q40)
    assert np.array_equal(RC.expected()["IQ4_NL"], RC.expected()["Q4_0"])


def test_every_tile_byte_is_written(tk):
    """the planes and the tail cover the tile: a buffer of 0xA5 and one of 0x5A come back equal"""
    for ttype in RC.TYPES:
        b = RC.blocks_of(ttype)
        outs = []
        for fill in (0xA5, 0x5A):
            tiles = np.full((RC.ROWS // 16, RC.K // 256, L.TILE_BYTES[ttype]), fill, np.uint8)
            rc = tk.lib().tk_mi355x_llm_repack_probe(-1, ttype, b.ctypes.data_as(C.c_void_p), C.c_int64(RC.ROWS), C.c_int64(RC.K), tiles.ctypes.data_as(C.c_void_p))
            assert rc == 0
            outs.append(tiles)
        assert RC.first_difference(outs[0], outs[1]) is None, f"{RC.NAMES[ttype]}: a byte is left unwritten: {RC.first_difference(outs[0], outs[1])}"


@pytest.mark.parametrize("device", [-1, 0])
def test_refusals_come_before_any_device(tk, device):
    """bad arguments are TK_ERROR_INVALID_ARGUMENT whether or not a device is named (this test runs where there is none)"""
    fn = tk.lib().tk_mi355x_llm_repack_probe
    fn.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    buf = np.zeros(1 << 20, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    assert fn(device, L.TYPE_Q4_K, None, 32, 512, p) == INVALID
    assert fn(device, L.TYPE_Q4_K, p, 32, 512, None) == INVALID
    for ttype in (L.TYPE_F32, L.TYPE_F16, L.TYPE_BF16, 4, 9, 15, 36, -1):  # float types have no tile; the others are no type of this build
        assert fn(device, ttype, p, 32, 512, p) == INVALID, ttype
    for rows, K in ((0, 512), (8, 512), (40, 512), (-16, 512), (32, 0), (32, 128), (32, 384), (32, -256), (32, 65536 + 256), (1 << 21, 256), (1 << 16, 2048)):
        assert fn(device, L.TYPE_Q4_K, p, rows, K, p) == INVALID, (rows, K)
    assert b"repack probe" in tk.lib().tk_error_get_detail()
