"""CPU: the Q8_0 KV cache's one definition (csrc/common/tk_kv_q8.h) through tk_mi355x_kv_q8_probe with device = -1 — the host loops, no GPU.

The quantiser against the float32 restatement tests/kv_q8_ref.py, bit for bit, on seeded rows, on blocks crafted to sit on every rounding edge and
at every head_dim the model loader accepts; the host attention loop against attention_far_ref.far (float64) on the dequantised values within the
forward bound of its fp32 chains, with a mutation that the bound must catch; and every refusal leaves the arrays untouched.

The header's host functions also run in a stand-alone program (tests/stubs/kv_q8_check.cpp) built here with -fsanitize=address,undefined: its rows
equal the restatement, its attention the probe's, and its roundf is checked at nextafter(0.5, 0) — a value of x * id that no f16 row reaches
(just_below_half() has the search), so the probe itself meets the nearest reachable neighbour below one half."""
import os
import subprocess

import numpy as np
import pytest

import attention_far_ref as F
import attention_geometry_cases as G
import kv_q8_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trackiellm_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HEAD_DIMS = G.accepted_head_dims()
SHAPE = (2, 3, 2, 40)  # layers, sequences, KV heads, window


def empty_cache(head_dim, shape=SHAPE, fill=0x5A):
    """cache arrays pre-filled with a sentinel: (kq, kd, vq, vd)"""
    kq = np.full(shape + (head_dim,), fill, np.int8)
    kd = np.full(shape + (head_dim // 32,), 0x5A5A, np.uint16)
    return kq, kd, kq.copy(), kd.copy()


def quantise_and_check(tk, k16, v16, seq, pos, layer, head_dim, device=-1):
    """mode 0 on sentinel-filled arrays: the rows named hold the restatement's bits, every other row the sentinel"""
    base = empty_cache(head_dim)
    got = tk.kv_q8_quantize_probe(*base, seq, pos, k16, v16, layer=layer, device=device)
    want = [a.copy() for a in base]
    wk, wkd = R.quantize(k16)
    wv, wvd = R.quantize(v16)
    for r, (s, p) in enumerate(zip(seq, pos)):
        want[0][layer, s, :, p], want[1][layer, s, :, p] = wk[r], wkd[r]
        want[2][layer, s, :, p], want[3][layer, s, :, p] = wv[r], wvd[r]
    for name, g, w in zip(("kq", "kd", "vq", "vd"), got, want):
        assert np.array_equal(g, w), (name, head_dim, np.argwhere(g != w)[:4])
    return got


def seeded_rows(n, n_kv, head_dim, scale, seed):
    rng = np.random.default_rng([7, seed, head_dim])
    return (rng.standard_normal((n, n_kv, head_dim), dtype=np.float32) * np.float32(scale)).astype(np.float16).view(np.uint16)


def f16(x):
    return np.asarray(x, np.float64).astype(np.float16)


def block_with(first, amax):
    """one block of 32 f16 values: `first` values, then amax, then small filler"""
    vals = list(first) + [amax]
    vals += [amax / 64.0 * ((i % 5) - 2) for i in range(32 - len(vals))]
    b = f16(vals)
    assert np.array_equal(b.astype(np.float64), np.asarray(vals)), "crafted values must be f16 numbers"
    return b


def just_below_half():
    """(x, amax) f16 whose float32(x * (1 / (amax / 127))) is the largest value below 0.5 that a cache row can reach.  nextafter(0.5, 0) itself is
    out of reach — an exhaustive search over every f16 pair finds none: the product of an 11-bit x and the 24-bit id never rounds onto it — so the
    probe sees the nearest reachable neighbour, and tk_kv_q8_roundf meets nextafter(0.5, 0) itself in the stand-alone program (kv_q8_check round)"""
    am = np.arange(0x3C00, 0x4000, dtype=np.uint16).view(np.float16).astype(np.float32)  # one binade of amax: the others repeat it
    inv = np.float32(1.0) / (am / np.float32(127.0)).astype(np.float32)
    x0 = (np.float32(0.5) / inv).astype(np.float16).view(np.uint16)
    best = (0.0, 0.0, 0.0)
    for k in (-1, 0, 1):
        x = (x0 + np.uint16(k & 0xFFFF)).astype(np.uint16).view(np.float16)
        p = (x.astype(np.float32) * inv).astype(np.float32)
        p = np.where(p < np.float32(0.5), p, np.float32(0))
        i = int(p.argmax())
        best = max(best, (float(p[i]), float(x[i]), float(am[i])))
    assert 0.4999 < best[0] < 0.5
    return best[1], best[2]


def crafted_blocks():
    """blocks whose x * id lands on the edges of roundf, of the sign and of the maximum search"""
    e = 2.0 ** -6
    a = 127 * e  # d = 2^-6, id = 64: x * id = x / e exactly
    out = [block_with([m * e for m in (0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 126.5, -126.5)], a)]
    x, am = just_below_half()
    out.append(block_with([x, -x], am))
    out.append(block_with([-a, 0.5 * e], a / 2))            # the extreme negative is the maximum: q = -127
    out.append(block_with([a, -a], a / 2))                  # +a before -a tied for amax
    out.append(block_with([-a, a], a / 2))                  # and the other order
    out.append(f16(np.zeros(32)))                           # an all-zero block
    blocks = np.stack(out).view(np.uint16)
    # the search's own claim, and the edge values themselves, in the restatement's arithmetic
    q, _ = R.quantize(blocks)
    assert q[0, :8].tolist() == [1, -1, 2, -2, 3, -3, 127, -127] and q[1, :2].tolist() == [0, 0] and q[2, 0] == -127
    assert q[3, :2].tolist() == [127, -127] and q[4, :2].tolist() == [-127, 127] and not q[5].any()
    return blocks


@pytest.fixture(scope="module")
def check_bin(tmp_path_factory):
    """tests/stubs/kv_q8_check.cpp: the header's host functions in a stand-alone program under the address and undefined-behaviour sanitizers"""
    out = str(tmp_path_factory.mktemp("kv_q8") / "kv_q8_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-mfma", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), "-I" + os.path.join(CSRC, "common"),
                           os.path.join(ROOT, "tests", "stubs", "kv_q8_check.cpp"), "-o", out])
    return out


def test_roundf_of_the_header_equals_the_restatement_at_every_edge(check_bin):
    lines = subprocess.run([check_bin, "round"], stdout=subprocess.PIPE, check=True, text=True, timeout=60).stdout.split()
    v = np.array([int(x, 16) for x in lines[0::2]], np.uint32).view(np.float32)
    got = np.array([int(x, 16) for x in lines[1::2]], np.uint32).view(np.float32)
    assert np.nextafter(np.float32(0.5), np.float32(0)) in v and np.float32(126.5) in v
    assert np.array_equal(got, R.roundf(v)), (v, got)
    assert np.array_equal(got, np.sign(v) * np.floor(np.abs(v.astype(np.float64)) + 0.5))  # roundf, in exact arithmetic


def test_stand_alone_host_loops_under_the_sanitizers(tk, check_bin, tmp_path):
    """the crafted blocks as rows of 64 through tk_kv_q8_row and tk_kv_q8_attention_row in the sanitized program: its rows equal the restatement,
    its attention the probe's host loop (one definition, two builds)"""
    blocks = crafted_blocks()
    rows = np.concatenate([blocks, blocks[::-1]], axis=1)  # [6][64]
    path = tmp_path / "rows.bin"
    rows.tofile(path)
    lines = subprocess.run([check_bin, "rows", str(path), "64"], stdout=subprocess.PIPE, check=True, text=True, timeout=60).stdout.splitlines()
    wq, wd = R.quantize(rows)
    for t, ln in enumerate(lines[:len(rows)]):
        q, d = ln[4:].split(" | ")
        assert np.array_equal(np.array(q.split(), int), wq[t]) and np.array_equal(np.array(d.split(), int), wd[t]), t
    cache = [a[None, None, None] for a in (wq, wd, wq, wd)]
    for ln in lines[len(rows):]:
        gq = int(ln.split()[1])
        out = np.array([int(x, 16) for x in ln.split()[2:]], np.uint32)
        q = R.value(wq, wd)[np.arange(gq) % len(rows)]
        got = tk.kv_q8_attention_probe(*[np.ascontiguousarray(a) for a in cache], [0], [len(rows) - 1], q[None], device=-1)
        assert np.array_equal(got.view(np.uint32).ravel(), out), gq


def test_roundf_of_the_restatement_is_exact_at_the_halves():
    v = np.array([0.5, -0.5, np.nextafter(np.float32(0.5), np.float32(0)), 1.5, 2.5, 126.5, -126.5, 0.49999997, 127.0, 0.0], np.float32)
    assert R.roundf(v).tolist() == [1, -1, 0, 2, 3, 127, -127, 0, 127, 0]
    assert np.trunc(np.float32(0.49999997) + np.float32(0.5)) == 1.0  # the form the contract rules out does go wrong there


def test_lossless_rows_quantise_without_loss():
    rows = R.lossless_rows((5, 3, 2, 256), 1)
    q, d = R.quantize(rows)
    assert np.array_equal(R.value(q, d), rows.view(np.float16).astype(np.float32))
    assert (np.abs(q.reshape(5, 3, 2, 8, 32)).max(axis=-1) == 127).all()
    e = np.log2(d.view(np.float16).astype(np.float64))
    assert np.array_equal(e, np.round(e)) and e.min() >= -10 and e.max() <= -4


DEEP_KEY_EXPONENTS = (-14, -10)  # the key rows of the deep session tests (tests/test_kv_q8_deep_gpu.py)


def test_lossless_rows_of_another_exponent_range_quantise_without_loss():
    """the range the deep session tests take for their key rows, and the widest one lossless_rows accepts: quantise, dequantise, identical; the
    default range draws what it drew before the argument existed"""
    for lo, hi in (DEEP_KEY_EXPONENTS, (-14, 8)):
        rows = R.lossless_rows((7, 3, 2, 256), 5, exponents=(lo, hi))
        q, d = R.quantize(rows)
        assert not R.inverse_overflows(rows).any()
        assert np.array_equal(R.value(q, d), rows.view(np.float16).astype(np.float32))
        assert (np.abs(q.reshape(7, 3, 2, 8, 32)).max(axis=-1) == 127).all()
        e = np.log2(d.view(np.float16).astype(np.float64))
        assert np.array_equal(e, np.round(e)) and e.min() == lo and e.max() == hi
    assert np.array_equal(R.lossless_rows((5, 2, 64), 3), R.lossless_rows((5, 2, 64), 3, exponents=(-10, -4)))
    same_draws = R.lossless_rows((5, 2, 64), 3, exponents=(-11, -5)).view(np.float16).astype(np.float64) * 2.0
    assert np.array_equal(same_draws, R.lossless_rows((5, 2, 64), 3).view(np.float16).astype(np.float64))


@pytest.mark.parametrize("head_dim", HEAD_DIMS)
def test_quantiser_equals_the_restatement_on_seeded_rows(tk, head_dim):
    seq, pos = np.array([0, 2, 2, 1], np.int32), np.array([0, 39, 7, 20], np.int32)
    for case, scale in enumerate((0.02, 1.0, 40.0)):
        k16 = seeded_rows(4, SHAPE[2], head_dim, scale, 2 * case)
        v16 = seeded_rows(4, SHAPE[2], head_dim, scale, 2 * case + 1)
        assert not R.inverse_overflows(k16).any() and not R.inverse_overflows(v16).any()
        quantise_and_check(tk, k16, v16, seq, pos, case % 2, head_dim)


@pytest.mark.parametrize("head_dim", HEAD_DIMS)
def test_quantiser_on_crafted_blocks(tk, head_dim):
    blocks = crafted_blocks()
    nb = head_dim // 32
    live = seeded_rows(1, 1, 32, 1.0, 5)[0, 0]
    rows = np.zeros((4, SHAPE[2], head_dim), np.uint16)
    for r in range(3):  # rows 0 .. 2: the crafted blocks in turn, an all-zero block between live ones where there is room
        for kvh in range(SHAPE[2]):
            for b in range(nb):
                rows[r, kvh, 32 * b:32 * b + 32] = blocks[(2 * r + kvh + b) % len(blocks)]
    if nb >= 3:
        rows[2, 0, :32], rows[2, 0, 32:64], rows[2, 0, 64:96] = live, 0, live
    # row 3 stays all zero
    seq, pos = np.array([1, 1, 0, 2], np.int32), np.array([3, 4, 39, 0], np.int32)
    kq, kd, vq, vd = quantise_and_check(tk, rows, rows[::-1].copy(), seq, pos, 1, head_dim)
    assert not kq[1, 2, :, 0].any() and not kd[1, 2, :, 0].any()  # the all-zero row: zeros and a zero scale


def attention_case(T, gq, head_dim, seed, lossless=False):
    """one (row, block of gq heads) over T positions of a cache of one sequence and one KV head: q, the cache arrays, the dequantised k, v"""
    q, k, v = F.rows(T, gq, head_dim, seed)
    shape = (1, 1, 1, T + 3)
    kq, kd, vq, vd = empty_cache(head_dim, shape, fill=0)
    k16 = np.zeros((T + 3, 1, head_dim), np.uint16)
    v16 = np.zeros_like(k16)
    k16[:T, 0], v16[:T, 0] = k.astype(np.float16).view(np.uint16), v.astype(np.float16).view(np.uint16)
    wk, wkd = R.quantize(k16)
    wv, wvd = R.quantize(v16)
    kq[0, 0, 0], kd[0, 0, 0], vq[0, 0, 0], vd[0, 0, 0] = wk[:, 0], wkd[:, 0], wv[:, 0], wvd[:, 0]
    return q.astype(np.float32), (kq, kd, vq, vd), R.value(wk[:T, 0], wkd[:T, 0]).astype(np.float64), R.value(wv[:T, 0], wvd[:T, 0]).astype(np.float64)


def bound(T, head_dim, v):
    """the standard forward bound of the fp32 chains: a score is a chain of head_dim fmas, the sums chains of T / 4 terms and a join; every
    output is a convex combination of values, so errors scale with max |v|"""
    return (T + head_dim + 16) * 2.0 ** -23 * np.abs(v).max()


@pytest.mark.parametrize("gq", (1, 2, 4))
@pytest.mark.parametrize("T", (1, 31, 32, 33, 64, 65, 129, 260))
def test_host_attention_loop_lies_within_the_bound_of_the_float64_form(tk, T, gq):
    head_dim = 64
    q, cache, k, v = attention_case(T, gq, head_dim, 11)
    got = tk.kv_q8_attention_probe(*cache, [0], [T - 1], q[None], device=-1)[0]
    want = F.far(q.astype(np.float64), k, v, 32)
    err = np.abs(got.astype(np.float64) - want).max()
    print("T %d gq %d: max error %.3g, bound %.3g" % (T, gq, err, bound(T, head_dim, v)))
    assert np.isfinite(got).all() and err <= bound(T, head_dim, v)


def test_the_bound_sees_a_dropped_position(tk):
    T, gq, head_dim = 65, 4, 64
    q, cache, k, v = attention_case(T, gq, head_dim, 11)
    got = tk.kv_q8_attention_probe(*cache, [0], [T - 1], q[None], device=-1)[0]
    broken = F.far(q.astype(np.float64), k, v, 32, mutation="drop_at_chunk_edge")
    assert np.abs(got.astype(np.float64) - broken).max() > bound(T, head_dim, v)


def test_host_attention_reads_only_the_rows_positions_and_heads_it_is_given(tk):
    """two sequences, two KV heads, rows at different positions: every row equals the one-row call on its own run, bystander rows keep the sentinel"""
    head_dim, n_kv, gq = 64, 2, 2
    shape = (2, 3, n_kv, 40)
    rng = np.random.default_rng(5)
    k16 = (rng.standard_normal(shape + (head_dim,), dtype=np.float32) * np.float32(0.6)).astype(np.float16).view(np.uint16)
    v16 = rng.standard_normal(shape + (head_dim,), dtype=np.float32).astype(np.float16).view(np.uint16)
    kq, kd = R.quantize(k16)
    vq, vd = R.quantize(v16)
    q = rng.standard_normal((3, n_kv * gq, head_dim), dtype=np.float32)
    seq, pos = [2, 0, 2], [39, 0, 17]
    got = tk.kv_q8_attention_probe(kq, kd, vq, vd, seq, pos, q, layer=1, device=-1)
    for r in range(3):
        for kvh in range(n_kv):
            one = [np.ascontiguousarray(a[1:2, seq[r]:seq[r] + 1, kvh:kvh + 1]) for a in (kq, kd, vq, vd)]
            alone = tk.kv_q8_attention_probe(*one, [0], [pos[r]], q[r:r + 1, kvh * gq:(kvh + 1) * gq], device=-1)
            assert np.array_equal(got[r, kvh * gq:(kvh + 1) * gq].view(np.uint32), alone[0].view(np.uint32)), (r, kvh)


# ---- the host loop at depth ---------------------------------------------------------------------------------------------------------------------

DEEP_FROM = 3000  # a row of a deep probe pass at or above this position is a deep row


def one_run(run, kvh, T):
    """positions [0, T) of one KV head of general_run()'s arrays as a cache of one layer, one sequence and one KV head"""
    return [np.ascontiguousarray(a[kvh, :T][None, None, None]) for a in run]


@pytest.mark.parametrize("name", list(R.DEEP_PROBE))
def test_deep_probe_rows_depend_on_their_deep_positions(tk, name):
    """the condition under which the bit-for-bit comparison of tests/test_kv_q8_deep_gpu.py says something about deep positions, on the host loop
    alone: for every deep row of every pass of the case (one KV head of it, row r takes head r % n_kv_head; the heads of a row share nothing) the
    output bits of EVERY query head of the group change when the int8 values of the V row at T - 1 change, again when those of the V row at T / 2
    do, and again when one K scale at T / 2 + 1 doubles.  Holds at DEEP_K_SCALE = 0.6, the key scale of the other attention tests: the scores'
    standard deviation is 0.6 whatever the head_dim (|q| = sqrt(head_dim), times 0.6 / sqrt(head_dim)), a softmax close to flat over thousands of
    positions.  Host cost: 4 runs x group x T x head_dim x 2 fmas per deep row, 0.6 G fmas for the largest case"""
    (nh, nkv, hd), W = R.DEEP_PROBE[name]
    grp = nh // nkv
    runs = {s: R.general_run((nh, nkv, hd), W, s) for s in (0, 1)}
    seen = set()
    for i, (seq, pos) in enumerate(R.probe_passes(name)):
        q = R.probe_q(name, i, seq.size, nh, hd)
        for r in np.flatnonzero(pos >= DEEP_FROM):
            T, kvh = int(pos[r]) + 1, int(r) % nkv
            if (int(seq[r]), T, kvh) in seen:   # the same run under another q: shown once
                continue
            seen.add((int(seq[r]), T, kvh))
            cache = one_run(runs[int(seq[r])], kvh, T)
            qr = np.ascontiguousarray(q[r:r + 1, kvh * grp:(kvh + 1) * grp])
            last = tk.kv_q8_attention_probe(*cache, [0], [T - 1], qr, device=-1, fill=np.float32(-77.0))
            assert np.isfinite(last).all() and (last != -77.0).all()
            for what in ("V row at T - 1", "V row at T / 2", "K scale at T / 2 + 1"):
                if what == "K scale at T / 2 + 1":
                    assert 0 < cache[1][0, 0, 0, T // 2 + 1, 0] < 0x7800
                    cache[1][0, 0, 0, T // 2 + 1, 0] += 0x0400   # the next power of two
                else:
                    t = T - 1 if what == "V row at T - 1" else T // 2
                    cache[2][0, 0, 0, t] = ~cache[2][0, 0, 0, t]
                    cache[2][0, 0, 0, t][cache[2][0, 0, 0, t] == -128] = 127   # values a quantised row can hold
                out = tk.kv_q8_attention_probe(*cache, [0], [T - 1], qr, device=-1, fill=np.float32(-77.0))
                moved = (out.view(np.uint32) != last.view(np.uint32)).reshape(grp, hd).any(axis=1)
                assert moved.all(), (name, i, int(r), T, what, moved.tolist())
                last = out
    assert len(seen) >= (1 if W == 32768 else 5)


def float64_attention(q, k, v):
    """-> (out, bound, scale), [gq][head_dim] float64: the attention of q [gq][hd] over the dequantised k, v [T][hd], the forward bound of
    tk_kv_q8_attention_row's fp32 arithmetic on it, and the size of what an output sums, sum_t p_t |v_t| (see the test below)"""
    from nn_row_ref import EXPF_REL, SQRT_REL, U
    T, hd = k.shape
    scale = 1.0 / np.sqrt(np.float64(hd))
    s = (k @ q.T) * scale                                                                       # [T][gq]
    s_err = hd * U * (np.abs(k) @ np.abs(q).T) * scale + np.abs(s) * (SQRT_REL + 2 * U)
    top = s.argmax(axis=0)
    dlt = s - s.max(axis=0)
    assert dlt.min() > -80.0                                                                    # tk_expf flushes nothing
    e = np.exp(dlt)
    p = e / e.sum(axis=0)
    out = p.T @ v
    terms = p.T @ np.abs(v)                                                                     # sum_t p_t |v_t|
    eta = np.abs(dlt) * U + s_err + s_err[top, np.arange(q.shape[0])]                           # relative error of a probability from its exponent
    from_scores = (p * eta).T @ np.abs(v) + (p * eta).sum(axis=0)[:, None] * terms              # numerator and denominator, first order
    return out, (T / 4 + 5) * U * terms + EXPF_REL * terms + from_scores, terms


@pytest.mark.parametrize("T", (8448, 32768))
def test_host_attention_loop_at_depth_lies_within_a_derived_bound_of_float64(tk, T):
    """one (row, KV head) of g2_d128 — two query heads, head_dim 128 — over T positions of general rows, against a float64 NumPy attention over
    R.value(q, scale): scores, max, exp, PV, division.  The bound per output element, first order in U = 2^-24, has three parts:

      PV     an output is N / l; N is four interleaved fma chains of T / 4 terms by position mod 4, joined by three adds, then one division: a term
             passes through at most T / 4 + 5 roundings, so |error| <= (T / 4 + 5) U sum_t |p_t v_t| (p_t = e_t / l; the element values d * q are exact)
      exp    tk_expf's documented relative error 2^-22 on every e_t: 2^-22 sum_t |p_t v_t|
      score  a score is a chain of head_dim fmas times att_scale = tk_divf(1, tk_sqrtf(head_dim)): |error| <= head_dim U sum_i |q_i k_ti| att_scale
             + |s_t| (2^-23 + 2 U), as nn_row_ref.attend1_64 has it; with the rounding of s_t - m and the same error of the maximum it is the
             relative error eta_t of e_t, which enters the numerator as sum_t p_t eta_t |v_t| and the denominator as (sum_t p_t eta_t) sum_t p_t |v_t|

    The bound must itself stay below 1e-3 of the output's scale sum_t p_t |v_t| — the size of what the output sums; the output is smaller, its terms
    cancel — so that a loose bound cannot hide an error: at T = 32 768 the PV part alone is 4.9e-4 of it.  Measured (printed):
    T = 8448: max error 3.3e-08, bound 1.95e-04 .. 2.17e-04, at most 2.7e-04 of the scale; T = 32 768: max error 5.4e-08, bound 4.87e-04 ..
    5.13e-04, at most 6.4e-04 of the scale (outputs up to 0.033 and 0.018).  The errors of the chains average out; the bound is the worst case.
    tests/test_kv_q8_deep_gpu.py ties the launch to this loop bit for bit."""
    gq, head_dim = 2, 128
    q, cache, k, v = attention_case(T, gq, head_dim, 23)
    got = tk.kv_q8_attention_probe(*cache, [0], [T - 1], q[None], device=-1, fill=np.float32(-77.0))[0].astype(np.float64)
    want, bnd, scale = float64_attention(q.astype(np.float64), k, v)
    err = np.abs(got - want)
    print("T %d: max error %.3g, bound %.3g .. %.3g, bound / scale at most %.3g, max |out| %.3g" % (T, err.max(), bnd.min(), bnd.max(), (bnd / scale).max(), np.abs(want).max()))
    assert np.isfinite(got).all() and (got != -77.0).all()
    assert (bnd < 1e-3 * scale).all()
    assert (err < bnd).all(), (T, float((err / bnd).max()))
    # what the bound does see at this depth: the upper half of the window left out
    half, _, _ = float64_attention(q.astype(np.float64), k[:T // 2], v[:T // 2])
    assert (np.abs(got - half) > bnd).any()


REFUSALS = ["null_kq", "null_kd", "null_vq", "null_vd", "null_rows", "head_dim_48", "values_short", "scales_short", "rows_short", "row_outside", "bad_mode", "null_q", "null_out",
            "group_of_3"]


@pytest.mark.parametrize("name", REFUSALS)
def test_refusals_write_nothing(tk, name):
    head_dim = 64
    base = empty_cache(head_dim)
    arrays = [a.copy() for a in base]
    k16 = seeded_rows(2, SHAPE[2], head_dim, 1.0, 3)
    q = np.ones((2, 4, head_dim), np.float32)
    out = np.full((2, 4, head_dim), 7.0, np.float32)
    seq, pos = [0, 1], [1, 2]
    kw = dict(layer=0, k16=k16, v16=k16.copy(), device=-1)
    mode = 0
    if name.startswith("null_k") or name.startswith("null_v"):
        arrays[("null_kq", "null_kd", "null_vq", "null_vd").index(name)] = None
    elif name == "null_rows":
        kw["k16"] = None
    elif name == "head_dim_48":
        kw["head_dim"] = 48
    elif name == "values_short":
        kw["n_values"] = arrays[0].size - 1
    elif name == "scales_short":
        kw["n_scales"] = arrays[1].size - 1
    elif name == "rows_short":
        kw["n_rows_elems"] = k16.size - 1
    elif name == "row_outside":
        pos = [1, SHAPE[3]]
    elif name == "bad_mode":
        mode = 2
    else:
        mode, kw = 1, dict(layer=0, q=None if name == "null_q" else q, out=None if name == "null_out" else out, device=-1)
        if name == "group_of_3":
            kw["q"], kw["out"] = np.ones((2, 6, head_dim), np.float32), np.full((2, 6, head_dim), 7.0, np.float32)
    with pytest.raises(tk.TkError):
        tk.kv_q8_probe_into(mode, arrays[0], arrays[1], arrays[2], arrays[3], seq, pos, **kw)
    for a, b in zip(arrays, base):
        assert a is None or np.array_equal(a, b)
    assert (out == 7.0).all()


def test_entries_exist_and_answer_without_a_device(tk):
    L = tk.lib()
    for name in ("tk_mi355x_llm_session_create_kv", "tk_mi355x_llm_session_kv_type", "tk_mi355x_llm_session_kv_bytes", "tk_mi355x_llm_session_kv_read_q8",
                 "tk_mi355x_llm_model_set_kv_cache_type", "tk_mi355x_llm_model_set_kv_cache_type_by_name", "tk_mi355x_attention_plan_kv", "tk_mi355x_kv_q8_probe"):
        assert hasattr(L, name), name
    assert L.tk_mi355x_llm_session_kv_type(None) == -1
    assert L.tk_mi355x_llm_model_set_kv_cache_type(None, 1) != 0 and L.tk_mi355x_llm_model_set_kv_cache_type_by_name(None, b"q8_0") != 0
    # kernel 6 for a Q8_0 session at every pass, the existing answer for F16 (device < 0: a 256-CU device assumed)
    for nrows in (1, 16, 256):
        assert tk.attention_plan(nrows, 32, 8, 128, 4096, device=-1, kv_type=tk.KV_Q8_0)[0] == 6
        assert tk.attention_plan(nrows, 32, 8, 128, 4096, device=-1, kv_type=tk.KV_F16) == tk.attention_plan(nrows, 32, 8, 128, 4096, device=-1)
    assert tk.attention_plan(256, 32, 8, 64, 260, device=-1, kv_type=1)[1:] == (4, 32, 2) and tk.attention_plan(1, 32, 8, 64, 260, device=-1, kv_type=1)[1:] == (4, 64, 2)
    with pytest.raises(tk.TkError):
        tk.attention_plan(1, 32, 8, 128, 4096, device=-1, kv_type=2)
