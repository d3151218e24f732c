"""The token-selection kernels one launch at a time: the test hooks tk_mi355x_token_pick_probe, tk_mi355x_logit_adjust_probe and
tk_mi355x_lang_pick_probe."""
import ctypes as C

import numpy as np

from ._lib import check, lib

PICK_ARGMAX, PICK_ARGMAX_ROWS, PICK_ROWS, PICK_ROWS_FILTERED = 0, 1, 2, 3
WH_STATE_INTS = 8
# tk_mi355x_sampling_t as a NumPy record (the kernels' TkSampleRow)
SAMPLING_DTYPE = np.dtype([("temperature", "<f4"), ("top_p", "<f4"), ("min_p", "<f4"), ("top_k", "<i4"), ("seed", "<u8"), ("counter", "<u4"),
                           ("reserved", "<u4")])


class TokenPickProbe(C.Structure):  # tk_mi355x_token_pick_probe_t
    _fields_ = [(n, C.c_int32) for n in ("kind", "rows", "cols", "ld")] + [("logits", C.c_void_p), ("n_logits", C.c_int64), ("masks", C.c_void_p),
                ("allow_row", C.c_void_p), ("n_masks", C.c_int32), ("hist_stride", C.c_int32), ("samp", C.c_void_p), ("tok", C.c_void_p),
                ("pos", C.c_void_p), ("nsteps", C.c_void_p), ("hist", C.c_void_p), ("n_hist", C.c_int64), ("temperature", C.c_float),
                ("counter0", C.c_uint32), ("seed", C.c_uint64), ("logprob", C.c_void_p), ("suppress", C.c_void_p), ("state", C.c_void_p)] + \
               [(n, C.c_int32) for n in ("beg", "eot", "tid0", "reserved")]


def sampling_rows(rows):
    """[(temperature, top_k, top_p, min_p, seed, counter)] -> a SAMPLING_DTYPE array"""
    a = np.zeros(len(rows), SAMPLING_DTYPE)
    for r, (temp, top_k, top_p, min_p, seed, counter) in enumerate(rows):
        a[r] = (temp, top_p, min_p, top_k, seed, counter, 0)
    return a


def token_pick_probe(kind, logits, rows, cols, ld=None, masks=None, allow_row=None, samp=None, tok=None, pos=None, nsteps=None, hist=None, hist_stride=0,
                     temperature=0.0, seed=0, counter0=0, logprob=None, suppress=None, state=None, beg=0, eot=0, tid0=-1, n_masks=None, device=0):
    """ONE launch of a token-selection kernel (tk_mi355x_token_pick_probe).  logits: float32, rows `ld` apart.  masks: uint32 [n_masks][(cols + 31) / 32].
    samp (SAMPLING_DTYPE), tok, pos, nsteps, hist (int32), logprob (float32) and state (int32 [rows][8]) are IN/OUT: COPIES are launched on and returned
    in a dict under the same names (None stays None: a NULL pointer).  device < 0: validation only."""
    def own(x, dtype):
        return None if x is None else np.array(x, dtype=dtype, order="C", copy=True)

    def addr(x):
        return None if x is None else x.ctypes.data

    logits = np.ascontiguousarray(logits, np.float32).reshape(-1)
    masks = None if masks is None else np.ascontiguousarray(masks, np.uint32)
    allow_row = None if allow_row is None else np.ascontiguousarray(allow_row, np.int32)
    suppress = None if suppress is None else np.ascontiguousarray(suppress, np.uint8)
    io = dict(samp=own(samp, SAMPLING_DTYPE), tok=own(tok, np.int32), pos=own(pos, np.int32), nsteps=own(nsteps, np.int32), hist=own(hist, np.int32),
              logprob=own(logprob, np.float32), state=own(state, np.int32))
    words = (cols + 31) // 32
    if masks is not None and (n_masks is None) and masks.size % max(words, 1):
        raise ValueError("token_pick_probe: masks must hold whole masks of (cols + 31) / 32 words")
    for name, per_row in (("samp", 1), ("tok", 1), ("pos", 1), ("nsteps", 1), ("logprob", 1), ("state", WH_STATE_INTS)):
        if rows >= 1 and io[name] is not None and io[name].size != rows * per_row:
            raise ValueError("token_pick_probe: %s must have %d entries" % (name, rows * per_row))
    if (rows >= 1 and allow_row is not None and allow_row.size != rows) or (suppress is not None and suppress.size != cols):
        raise ValueError("token_pick_probe: allow_row must have `rows` entries and suppress `cols`")
    p = TokenPickProbe()
    p.kind, p.rows, p.cols, p.ld = kind, rows, cols, cols if ld is None else ld
    p.logits, p.n_logits = logits.ctypes.data, logits.size
    p.masks, p.allow_row = addr(masks), addr(allow_row)
    p.n_masks = (0 if masks is None else masks.size // words) if n_masks is None else n_masks
    p.hist_stride, p.n_hist = hist_stride, 0 if io["hist"] is None else io["hist"].size
    p.samp, p.tok, p.pos, p.nsteps, p.hist = addr(io["samp"]), addr(io["tok"]), addr(io["pos"]), addr(io["nsteps"]), addr(io["hist"])
    p.temperature, p.counter0, p.seed = temperature, counter0, seed
    p.logprob, p.suppress, p.state = addr(io["logprob"]), addr(suppress), addr(io["state"])
    p.beg, p.eot, p.tid0 = beg, eot, tid0
    lib().tk_mi355x_token_pick_probe.argtypes = [C.c_int, C.POINTER(TokenPickProbe)]
    check(lib().tk_mi355x_token_pick_probe(device, C.byref(p)))
    return io


class LogitAdjust(C.Structure):  # tk_mi355x_logit_adjust_t
    _fields_ = [("repeat", C.c_float), ("freq", C.c_float), ("present", C.c_float), ("n_recent", C.c_int32), ("recent", C.c_void_p),
                ("n_bias", C.c_int32), ("bias_ids", C.c_void_p), ("bias", C.c_void_p)]


def logit_adjust_rows(specs):
    """[None | dict(repeat=1, freq=0, present=0, recent=None, bias_ids=None, bias=None, n_recent=None, n_bias=None)] -> (a LogitAdjust array, the
    NumPy arrays it points into: keep them alive as long as the array is used).  None = a neutral row.  n_recent / n_bias default to the arrays'
    lengths; given, they are passed as they are (a count without an array is a NULL pointer with that count)."""
    tab, keep = (LogitAdjust * len(specs))(), []
    for r, sp in enumerate(specs):
        sp = sp or {}
        arrs = []
        for name, dtype in (("recent", np.int32), ("bias_ids", np.int32), ("bias", np.float32)):
            a = sp.get(name)
            a = None if a is None else np.ascontiguousarray(a, dtype).reshape(-1)
            arrs.append(a)
            keep.append(a)
        recent, bias_ids, bias = arrs
        n_recent = sp.get("n_recent", 0 if recent is None else recent.size)
        n_bias = sp.get("n_bias", 0 if bias_ids is None else bias_ids.size)
        tab[r] = LogitAdjust(sp.get("repeat", 1.0), sp.get("freq", 0.0), sp.get("present", 0.0), n_recent, None if recent is None else recent.ctypes.data,
                             n_bias, None if bias_ids is None else bias_ids.ctypes.data, None if bias is None else bias.ctypes.data)
    return tab, keep


def logit_adjust_probe(logits, rows, cols, adjust, device=0, n_logits=None):
    """ONE launch of k_logit_adjust (tk_mi355x_logit_adjust_probe) on a COPY of logits (float32, [rows][cols] packed), which is returned; adjust:
    the specs of logit_adjust_rows, one per row.  device < 0: the same per-row function in a host loop, no GPU touched.  A refusal raises TkError
    with the copy untouched: pass a float32 array as `out` through logit_adjust_probe_into to see that"""
    out = np.array(logits, dtype=np.float32, order="C", copy=True).reshape(-1)
    logit_adjust_probe_into(out, rows, cols, adjust, device=device, n_logits=n_logits)
    return out.reshape(rows, cols) if out.size == rows * cols else out


def logit_adjust_probe_into(out, rows, cols, adjust, device=0, n_logits=None):
    """logit_adjust_probe in place on the C-contiguous float32 array `out`"""
    if out.dtype != np.float32 or not out.flags["C_CONTIGUOUS"]:
        raise ValueError("logit_adjust_probe_into: out must be a C-contiguous float32 array")
    tab, keep = logit_adjust_rows(adjust)
    f = lib().tk_mi355x_logit_adjust_probe
    f.argtypes = [C.c_int, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    check(f(device, rows, cols, out.ctypes.data, out.size if n_logits is None else n_logits, C.cast(tab, C.c_void_p) if len(adjust) else None))
    del keep


def lang_pick_probe(logits, rows, cols, tok0, n_lang, auto_row, slot, ld=None, device=0, n_logits=None):
    """ONE launch of k_lang_pick (tk_mi355x_lang_pick_probe): Whisper's language detection over the n_lang logits from column tok0 on of every row.
    logits: float32, rows `ld` apart.  auto_row [rows]: != 0 = the row stores its token tok0 + id into its slot.  slot [rows] is IN/OUT: a COPY is
    launched on and returned.  -> (ids [rows], probs [rows][n_lang], slot).  device < 0: the same per-row function in a host loop, no GPU touched"""
    logits = np.ascontiguousarray(logits, np.float32).reshape(-1)
    auto_row = np.ascontiguousarray(auto_row, np.int32).reshape(-1)
    slot = np.array(slot, dtype=np.int32, order="C", copy=True).reshape(-1)
    if rows >= 1 and (auto_row.size != rows or slot.size != rows):
        raise ValueError("lang_pick_probe: auto_row and slot must have `rows` entries")
    ids = np.full(max(rows, 1), -1, np.int32)
    probs = np.full((max(rows, 1), max(min(n_lang, 128), 1)), -1.0, np.float32)
    f = lib().tk_mi355x_lang_pick_probe
    f.argtypes = [C.c_int, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    check(f(device, rows, cols, cols if ld is None else ld, logits.ctypes.data, logits.size if n_logits is None else n_logits, tok0, n_lang, auto_row.ctypes.data,
            slot.ctypes.data, ids.ctypes.data, probs.ctypes.data))
    return ids, probs, slot
