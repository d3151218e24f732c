"""The repack fixture's inputs (tests/golden/repack_tiles.npz): per tiled type a 32 x 512 matrix of random block bytes — two row tiles by two
256-k runs, the smallest shape at which the row-tile index, the run index and the run stride are all non-zero.  Every type reads the head of
ONE byte stream ("blocks" in the fixture: np.random.default_rng(SEED).integers(0, 256, ...), kept in the file so that the inputs do not hang on
NumPy's generator), so IQ4_NL and Q4_0, whose blocks have the same size, hold the same bytes.  Random bytes put live bits in every field of
every block; any byte is a legal TQ1_0 base-3 byte.  The expected tiles were recorded from the twelve per-type repack kernels this
project had before they became one template, and are not regenerated from the code under test."""
import os

import numpy as np

import trackiellm_amd.llm as L

ROWS, K, SEED = 32, 512, 20261019
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "repack_tiles.npz")
NAMES = {L.TYPE_Q4_0: "Q4_0", L.TYPE_Q4_1: "Q4_1", L.TYPE_Q5_0: "Q5_0", L.TYPE_Q5_1: "Q5_1", L.TYPE_Q8_0: "Q8_0", L.TYPE_Q2_K: "Q2_K", L.TYPE_Q3_K: "Q3_K",
         L.TYPE_Q4_K: "Q4_K", L.TYPE_Q5_K: "Q5_K", L.TYPE_Q6_K: "Q6_K", L.TYPE_IQ4_NL: "IQ4_NL", L.TYPE_IQ4_XS: "IQ4_XS", L.TYPE_TQ1_0: "TQ1_0", L.TYPE_TQ2_0: "TQ2_0"}
TYPES = sorted(NAMES)


_fixture = None


def expected():
    """the fixture, loaded once: "blocks" and one array of tiles [2][2][tile bytes] per type name"""
    global _fixture
    if _fixture is None:
        with np.load(FIXTURE) as z:
            _fixture = {k: z[k] for k in z.files}
        for a in _fixture.values():
            a.setflags(write=False)
    return _fixture


def blocks_of(ttype):
    """the type's 32 x 512 weights as raw block bytes: the head of the seeded stream"""
    n = ROWS * K // (32 if ttype in L.TYPES_OF_32 else 256) * L.BLOCK_BYTES[ttype]
    return expected()["blocks"][:n].copy()


def first_difference(got, want):
    """None when equal, else a message naming the first differing byte as (row tile, run, offset in the tile)"""
    if got.shape != want.shape:
        return f"shape {got.shape} against {want.shape}"
    at = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    if at.size == 0:
        return None
    rt, run, off = np.unravel_index(at[0], want.shape)
    return f"{at.size} bytes differ, the first at row tile {rt}, run {run}, tile offset {off}: {got[rt, run, off]} against {want[rt, run, off]}"
