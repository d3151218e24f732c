"""GPU: the one k_repack kernel writes, per tiled type, the tile bytes recorded from the per-type kernels it replaced
(tests/golden/repack_tiles.npz, tests/repack_cases.py): one launch per type, byte for byte."""
import numpy as np
import pytest

import repack_cases as RC
import trackiellm_amd.llm as L

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ttype", RC.TYPES, ids=[RC.NAMES[t] for t in RC.TYPES])
def test_device_repack_matches_recorded_tiles(gpu, ttype):
    want = RC.expected()[RC.NAMES[ttype]]
    got = gpu.repack_probe(ttype, RC.blocks_of(ttype), RC.ROWS, RC.K, device=0)
    assert RC.first_difference(got, want) is None, f"{RC.NAMES[ttype]}: {RC.first_difference(got, want)}"


def test_iq4_nl_tiles_are_the_q4_0_tiles_of_the_same_bytes(gpu):
    b = RC.blocks_of(L.TYPE_IQ4_NL)
    nl, q40 = (gpu.repack_probe(t, b, RC.ROWS, RC.K, device=0) for t in (L.TYPE_IQ4_NL, L.TYPE_Q4_0))
    assert RC.first_difference(nl, q40) is None, RC.first_difference(nl, q40)
