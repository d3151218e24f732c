"""What tests/test_attention_far_gpu.py rests on, without a GPU: the window limits of the resident attention form as the library reports them, the
plan on both sides of a limit, and — on a float64 restatement of k_attention_far's two-pass order (attention_far_ref.py) — that the order gives
k_attention's bits at every tested length and that a bit-exact comparison sees each of three mistakes the two-pass walk could make."""
import numpy as np
import pytest

import attention_far_ref as R
import attention_geometry_cases as G

# (n_head, n_kv_head, head_dim) -> the largest window of the resident form, worked out by hand from tk_attention_lds_bytes(group, head_dim, window, 64)
# <= 160 KiB: ring 2 x 64 x head_dim x 2 B; 4 B per query head of the group and position; at head_dim 256 also q (group x 256 x 4 B) and the own key row
LIMITS = {
    (32, 8, 128): 8192,    # (163840 - 32768) / 16
    (32, 8, 64): 9216,     # (163840 - 16384) / 16
    (24, 6, 256): 5856,    # (163840 - 65536 - 4096 - 512) / 16
    (16, 8, 128): 16384,   # (163840 - 32768) / 8
}
LENGTHS = sorted(set(p + 1 for w in (260, G.ODD_WINDOW) for p in G.WINDOWS[w]))   # cached positions of the GPU test's decode rows, the row itself included


def test_resident_limit_of_the_four_geometries(tk):
    for geom, want in LIMITS.items():
        assert R.resident_limit(*geom) == want, geom
        assert tk.attention_resident_limit(*geom) == want, geom
    assert tk.attention_resident_limit(7, 2, 128) == 0   # no whole group


def test_a_window_at_the_limit_and_one_above_it_are_told_apart(tk, monkeypatch):
    monkeypatch.delenv("TK_MI355X_ATT_RESIDENT_MAX", raising=False)
    for (nh, nkv, hd), limit in LIMITS.items():
        for rows in (1, 16, 64, 256):
            for fused in (True, False):
                at = tk.attention_plan(rows, nh, nkv, hd, limit, fused, device=-1)
                above = tk.attention_plan(rows, nh, nkv, hd, limit + 1, fused, device=-1)
                assert at[0] in (0, 1, 2) and above[0] in (5, 2), (nh, nkv, hd, rows, fused, at, above)
                top = limit   # the last position of the wider window
                assert tk.attention_plan(rows, nh, nkv, hd, limit + 1, fused, device=-1, top_position=100)[0] == 5
                assert tk.attention_plan(rows, nh, nkv, hd, limit, fused, device=-1, top_position=100)[0] in (0, 1)
                if not fused and hd in (64, 128):
                    assert above[0] == 2 and tk.attention_plan(rows, nh, nkv, hd, limit + 1, False, device=-1, top_position=top)[0] == 2
    with pytest.raises(tk.TkError):
        tk.attention_plan(1, 32, 8, 128, 0, True, device=-1)


def test_the_knob_moves_the_limit_down_only(tk, monkeypatch):
    monkeypatch.setenv("TK_MI355X_ATT_RESIDENT_MAX", "64")
    assert tk.attention_plan(16, 32, 8, 128, 64, True, device=-1)[0] in (0, 1)
    assert tk.attention_plan(16, 32, 8, 128, 65, True, device=-1)[0] == 5
    assert tk.attention_plan(16, 16, 8, 128, 260, True, device=-1) == (5, 2, 64, 2)     # the narrow kernel steps aside as well
    assert tk.attention_plan(256, 32, 8, 64, 260, True, device=-1) == (5, 4, 32, 2)
    monkeypatch.setenv("TK_MI355X_ATT_RESIDENT_MAX", "100000")
    assert tk.attention_plan(16, 32, 8, 128, 8193, True, device=-1)[0] == 5
    assert tk.attention_resident_limit(32, 8, 128) == 8192


@pytest.mark.parametrize("gq,hd", [(4, 64), (2, 128), (1, 256)])
def test_two_pass_order_gives_the_resident_bits_and_mutations_show(gq, hd):
    seen = {m: [] for m in R.MUTATIONS}
    for T in LENGTHS:
        q, k, v = R.rows(T, gq, hd, seed=23)
        want = R.resident(q, k, v).view(np.uint64)
        for ch in (32, 64):
            got = R.far(q, k, v, ch).view(np.uint64)
            assert np.array_equal(got, want), (T, ch)
            nchunk = -(-T // ch)
            s = R.scores(q, k, 1.0 / np.sqrt(np.float64(hd)))
            for m in R.MUTATIONS:
                moved = not np.array_equal(R.far(q, k, v, ch, mutation=m).view(np.uint64), want)
                # where the mistake changes what is computed at all: a head's maximum in the chunk left out; a class with three positions in a
                # chunk (two terms commute); a full chunk
                if m == "max_without_last_chunk":
                    can = nchunk > 1 and bool((s.argmax(axis=0) >= (nchunk - 1) * ch).any())
                elif m == "pv_descending":
                    can = any(min(T - c * ch, ch) >= 2 * R.TSPLIT + 1 for c in range(nchunk))
                else:
                    can = T >= ch
                assert moved == can, (m, T, ch)
                if moved:
                    seen[m].append((T, ch))
    for m in R.MUTATIONS:   # each is seen at several of the tested lengths, with either slot size
        assert len({t for t, _ in seen[m]}) >= 3 and {c for _, c in seen[m]} == {32, 64}, (m, seen[m])
