"""CPU: the context shift's one definition (csrc/common/tk_kv_shift.h) through tk_mi355x_kv_shift_probe with device = -1 — the per-row function in
a host loop — against the exact NumPy restatement tests/kv_shift_ref.py, bit for bit (a NaN as a NaN); against the float64 rotation within a bound
derived from its three roundings; at every head geometry the model loader accepts; and every refusal leaves the arrays untouched."""
import ctypes as C

import numpy as np
import pytest

import kv_shift_ref as R

HEAD_DIMS = (64, 128, 192, 256)
MAX_CTX = 80
# (p0, p1, delta): one row by one; everything but eight rows by one (full overlap); the upper half onto the lower (none); one row of overlap
# short of that; a middle range by its own distance from 0; the last row onto row 0
MOVES = [(1, 2, -1), (8, 80, -1), (40, 80, -40), (41, 80, -39), (5, 64, -5), (79, 80, -79)]
THETA = 10000.0


def shape_of(head_dim, max_ctx=MAX_CTX):
    return (2, 3, 2, max_ctx, head_dim)  # two layers, three sequences, two KV heads


_tables = {}


def tables(head_dim, max_ctx=MAX_CTX):
    if (head_dim, max_ctx) not in _tables:
        _tables[(head_dim, max_ctx)] = R.rope_table(max_ctx, head_dim, THETA)
    return _tables[(head_dim, max_ctx)]


def check_move(tk, k, v, cs, sn, seq, p0, p1, delta, device=-1):
    """the probe against the restatement on one move; returns the probe's arrays"""
    gk, gv = tk.kv_shift_probe(k, v, cs, sn, seq, p0, p1, delta, device=device)
    wk, wv = R.kv_shift_ref(k, v, cs, sn, seq, p0, p1, delta)
    assert R.same_f16_bits(gk, wk), (k.shape, seq, p0, p1, delta)
    assert np.array_equal(gv, wv), (k.shape, seq, p0, p1, delta)
    # outside the destination range of `seq`, and in the other sequences, nothing changed — not even a NaN's payload
    keep = np.ones(k.shape, bool)
    keep[:, seq, :, p0 + delta:p1 + delta] = False
    assert np.array_equal(gk[keep], k[keep]) and np.array_equal(gv[keep], v[keep])
    return gk, gv


def test_the_vector_fma_equals_rational_arithmetic():
    """the restatement's own exactness: fma_f16_f32 against one rounding of the exact rational sum, on seeded operands and on sums built to sit near
    a fp32 midpoint (where rounding to float64 first and to fp32 after goes wrong)"""
    rng = np.random.default_rng(3)
    x = rng.standard_normal(400).astype(np.float16).astype(np.float32)
    y = rng.uniform(-1, 1, 400).astype(np.float32)
    z = (rng.standard_normal(400) * rng.choice([1e-3, 1.0, 1e3], 400)).astype(np.float32)
    # z + x * y with x * y far below z's last bit but not zero, z's last bit set or clear: the fma is z nudged, never a tie
    x = np.concatenate([x, np.full(4, 2.0 ** -14, np.float32)])
    y = np.concatenate([y, np.array([2.0 ** -40, -2.0 ** -40, 2.0 ** -40, -2.0 ** -40], np.float32)])
    z = np.concatenate([z, np.array([1.0, 1.0, 1.0 + 2.0 ** -23, 1.0 + 2.0 ** -23], np.float32)])
    # exact midpoints and midpoints missed by a bit float64 cannot hold: 1 + 2^-24 (+- x * y of 2^-70)
    x = np.concatenate([x, np.array([1.0, 2.0 ** -14, 2.0 ** -14, 1.0], np.float32)])
    y = np.concatenate([y, np.array([2.0 ** -24, 2.0 ** -56, -2.0 ** -56, 3 * 2.0 ** -24], np.float32)])
    z = np.concatenate([z, np.array([1.0, 1.0 + 2.0 ** -23, 1.0 + 2.0 ** -23, 1.0], np.float32)])
    got = R.fma_f16_f32(x, y, z)
    want = np.array([R.fma_scalar(a, b, c) for a, b, c in zip(x, y, z)], np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[-4] == np.float32(1.0) and got[-1] == np.float32(1.0 + 2.0 ** -22)  # ties go to even


@pytest.mark.parametrize("head_dim", HEAD_DIMS)
def test_host_loop_equals_the_restatement_on_every_move(tk, head_dim):
    """checks 1 and 2: seeded bit patterns with the special f16 patterns in every row; every move of MOVES, in each of the three sequences in turn;
    everything outside the destination range and both other sequences unchanged bit for bit"""
    cs, sn = tables(head_dim)
    for case, (p0, p1, delta) in enumerate(MOVES):
        k, v = R.seeded_caches(shape_of(head_dim), seed=100 * head_dim + case)
        gk, _ = check_move(tk, k, v, cs, sn, case % 3, p0, p1, delta)
        nan_in = (k[:, case % 3, :, p0:p1] & 0x7FFF) > 0x7C00
        nan_out = (gk[:, case % 3, :, p0 + delta:p1 + delta] & 0x7FFF) > 0x7C00
        pair_in = nan_in[..., 0::2] | nan_in[..., 1::2]
        assert nan_in.any() and (nan_out[..., 0::2] & nan_out[..., 1::2])[pair_in].all()  # a NaN stays a NaN (and takes its pair with it)


@pytest.mark.parametrize("head_dim", HEAD_DIMS)
def test_identity_and_quarter_turn_tables(tk, head_dim):
    """cos = 1, sin = 0: every key of a pair of finite values comes back with its own bits, denormals included.  Two things follow from the formula
    and are not the kernel's to mend: an infinity times the zero sine is a NaN, so pairs that hold an Inf or a NaN are left out; and a zero comes
    back as a zero whose sign is that of (-0) + (+-0 from the other half times the zero sine), so zeros are compared as values.
    cos = 0, sin = 1: pairs swap with one sign flipped, k' = (b, -a), zeros again as values"""
    half = head_dim // 2
    one, zero = np.ones((MAX_CTX, half), np.float32), np.zeros((MAX_CTX, half), np.float32)
    k, v = R.seeded_caches(shape_of(head_dim), seed=7 + head_dim)
    p0, p1, delta = 8, 80, -3
    src = k[:, 1, :, p0:p1]
    special = (src & 0x7C00) == 0x7C00  # Inf or NaN
    pair_ok = ~(special[..., 0::2] | special[..., 1::2])
    gk, _ = check_move(tk, k, v, one, zero, 1, p0, p1, delta)
    dst = gk[:, 1, :, p0 + delta:p1 + delta]
    for half_of_pair in (slice(0, None, 2), slice(1, None, 2)):
        want, got = src[..., half_of_pair][pair_ok], dst[..., half_of_pair][pair_ok]
        nz = (want & 0x7FFF) != 0
        assert nz.sum() > 1000 and np.array_equal(got[nz], want[nz]) and ((got[~nz] & 0x7FFF) == 0).all()
    gk, _ = check_move(tk, k, v, zero, one, 1, p0, p1, delta)
    dst = gk[:, 1, :, p0 + delta:p1 + delta]
    # a * 0 + b = b except that -0 + +0 = +0: compare values (zeros of either sign are equal), and the bits wherever the source is no zero
    a, b = src[..., 0::2][pair_ok], src[..., 1::2][pair_ok]
    e, o = dst[..., 0::2][pair_ok], dst[..., 1::2][pair_ok]
    assert np.array_equal(e.view(np.float16), b.view(np.float16)) and np.array_equal(o.view(np.float16), -a.view(np.float16))
    nz_b, nz_a = (b & 0x7FFF) != 0, (a & 0x7FFF) != 0
    assert np.array_equal(e[nz_b], b[nz_b]) and np.array_equal(o[nz_a], a[nz_a] ^ 0x8000)


@pytest.mark.parametrize("head_dim", HEAD_DIMS)
def test_host_loop_lies_within_the_bound_of_the_float64_rotation(tk, head_dim):
    """|k' - exact| <= half an f16 ulp of k' + 2^-23 (|a c| + |b s|), from the three roundings: the product a c to fp32 (at most 2^-24 |a c|), the
    fma to fp32 (at most 2^-24 of its result, which is at most |a c| + |b s| in magnitude; the product's own error inside that result is second
    order, 2^-48 |a c|, and is not carried) and the result to f16 (half an ulp of the f16 it becomes).  The exact rotation is taken in float64, of the
    fp32 table entries"""
    cs, sn = tables(head_dim)
    k, v = R.seeded_caches(shape_of(head_dim), seed=50 + head_dim, finite=True)
    for p0, p1, delta in [(8, 80, -1), (41, 80, -39), (79, 80, -79)]:
        d = -delta
        gk, _ = tk.kv_shift_probe(k, v, cs, sn, 2, p0, p1, delta, device=-1)
        src = k[:, 2, :, p0:p1].view(np.float16).astype(np.float64)
        got16 = gk[:, 2, :, p0 - d:p1 - d].view(np.float16)
        a, b = src[..., 0::2], src[..., 1::2]
        c, s = cs[d].astype(np.float64), sn[d].astype(np.float64)
        exact = np.empty_like(src)
        exact[..., 0::2] = a * c + b * s
        exact[..., 1::2] = b * c - a * s
        mag = np.empty_like(src)
        mag[..., 0::2] = np.abs(a * c) + np.abs(b * s)
        mag[..., 1::2] = np.abs(b * c) + np.abs(a * s)
        assert np.isfinite(got16).all()
        bound = 0.5 * np.spacing(np.abs(got16)).astype(np.float64) + 2.0 ** -23 * mag
        err = np.abs(got16.astype(np.float64) - exact)
        print("head_dim", head_dim, "move", (p0, p1, delta), "largest error / bound:", float((err / bound).max()))
        assert (err <= bound).all()
        assert (err > 0.25 * np.spacing(np.abs(got16)).astype(np.float64)).any()  # the rounding to f16 is really there: the check is no tautology


def test_a_move_that_overlaps_itself_reads_every_row_before_it_is_overwritten(tk):
    """(8, 80, -1) moves 72 rows onto themselves shifted by one: a walk in the wrong order would smear row 8 over the whole range.  V is a copy, so
    row p + delta must equal the ORIGINAL row p for every p"""
    cs, sn = tables(64)
    k, v = R.seeded_caches(shape_of(64), seed=5)
    _, gv = tk.kv_shift_probe(k, v, cs, sn, 0, 8, 80, -1, device=-1)
    assert np.array_equal(gv[:, 0, :, 7:79], v[:, 0, :, 8:80]) and not np.array_equal(v[:, 0, :, 8], v[:, 0, :, 9])


REFUSALS = {
    "delta 0": dict(move=(0, 8, 40, 0)),
    "delta positive": dict(move=(0, 8, 40, 3)),
    "p0 + delta negative": dict(move=(0, 8, 40, -9)),
    "p1 beyond max_ctx": dict(move=(0, 8, MAX_CTX + 1, -1)),
    "p0 equals p1": dict(move=(0, 8, 8, -1)),
    "p0 above p1": dict(move=(0, 9, 8, -1)),
    "p0 negative": dict(move=(0, -1, 8, -1)),
    "sequence -1": dict(move=(-1, 8, 40, -1)),
    "sequence max_seq": dict(move=(3, 8, 40, -1)),
    "null kcache": dict(null="k"),
    "null vcache": dict(null="v"),
    "null cos": dict(null="cos"),
    "null sin": dict(null="sin"),
    "head_dim 60": dict(head_dim=60),
    "head_dim 12": dict(head_dim=12),
    "head_dim 0": dict(head_dim=0),
    "head_dim 264": dict(head_dim=264),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_leave_the_arrays_untouched(tk, name):
    """check 3: TK_ERROR_INVALID_ARGUMENT and not a bit changed"""
    spec = REFUSALS[name]
    cs, sn = tables(64)
    k, v = R.seeded_caches(shape_of(64), seed=9)
    k0, v0 = k.copy(), v.copy()
    seq, p0, p1, delta = spec.get("move", (0, 8, 40, -1))
    null = spec.get("null")
    with pytest.raises(tk.TkError) as e:
        tk.kv_shift_probe_into(None if null == "k" else k, None if null == "v" else v, None if null == "cos" else cs, None if null == "sin" else sn, seq, p0, p1,
                               delta, device=-1, head_dim=spec.get("head_dim"))
    assert e.value.code == 1001
    assert np.array_equal(k, k0) and np.array_equal(v, v0)
    # the same arguments without the fault are taken
    tk.kv_shift_probe_into(k, v, cs, sn, 0, 8, 40, -1, device=-1)
    assert not np.array_equal(k, k0)


def test_entries_exist_and_refuse_null_handles(tk):
    L = tk.lib()
    for name in ("tk_mi355x_llm_session_kv_shift", "tk_mi355x_kv_shift_probe", "tk_mi355x_llm_runner_set_context_shift", "tk_mi355x_llm_runner_context_shifts",
                 "tk_mi355x_llm_time_kv_shift"):
        assert hasattr(L, name)
    assert L.tk_mi355x_llm_session_kv_shift(None, 0, 1, 2, -1) == 1001
    assert L.tk_mi355x_llm_runner_set_context_shift(None, 1, 8) == 1001
    assert L.tk_mi355x_llm_runner_set_context_shift(None, 1, -2) == 1001  # with a live runner: tests/test_context_shift_gpu.py
    assert L.tk_mi355x_llm_runner_context_shifts(None, None, None) == 1001
    assert hasattr(tk.LlmSession, "kv_shift") and hasattr(tk.LlmRunner, "set_context_shift") and hasattr(tk.LlmRunner, "context_shifts")
    assert C.sizeof(C.c_int64) == 8
