"""What a pass of TkLlmSession launched BEFORE csrc/llm/tk_pass_form.h existed, restated from that code: five mutable members
(tiled_pass, long_pass, run_pass, adjust_pass, logprob_pass) set by the entries, eight graph array families indexed by the UNRESOLVED members, and
the gating inside enqueue_range() that turned them into launches.  tests/test_pass_form_cpu.py holds the header's resolvers and key against this
over a whole domain; tests/test_pass_forms_gpu.py counts the graphs a walk may record with it.

A case is (entry, nrows, top, caps, adjust, logprobs); caps = (has_scores, prefill_geometry, long_geometry_at_nrows):
  has_scores              the session allocated d_scores
  prefill_geometry        tk_attention_prefill_applies(...)
  long_geometry_at_nrows  tk_attention_long_applies(nrows, ...)
"""
import itertools

TK_TILED_ATT_FROM_POS = 128
TK_LONG_ATT_MAX_ROWS = 8
TK_LONG_ATT_MIN_POS = 512

ENTRIES = ["forward_head_distinct", "forward_head_repeated", "forward_no_head", "prefill", "decode", "verify-1", "verify0", "verify2", "verify4"]
NROWS = [1, 4, 5, 8, 9, 16, 256]
TOPS = [0, 127, 128, 255, 256, 511, 512, 767, 768]
CAPS = list(itertools.product([False, True], repeat=3))

ROW, TILED, LONG, RUN = 0, 1, 2, 3


def long_att_min_pos(nrows):
    return 768 if nrows > 4 else TK_LONG_ATT_MIN_POS


def verify_run_min_pos(nrows):
    return 256


def verify_form(nrows, top, caps):
    """TkLlmSession::verify_form"""
    has_scores, prefill_geometry, long_geometry = caps
    if has_scores and long_geometry and top >= verify_run_min_pos(nrows):
        return 4
    if top >= TK_TILED_ATT_FROM_POS and prefill_geometry:
        return 2
    return 0


def parent_pass(entry, nrows, top, caps, adjust=False, logprobs=False):
    """None when the entry refused the arguments, else a dict:
    family, index   the graph array and the index into it that the entry replayed (family None: an entry that never replays)
    attn            the attention enqueue_range() launched
    launches        (launches of one layer that vary, launches of the head)"""
    has_scores, prefill_geometry, long_geometry = caps
    # choose_attention_top()
    tiled_pass = top >= TK_TILED_ATT_FROM_POS
    long_pass = has_scores and nrows <= TK_LONG_ATT_MAX_ROWS and top >= long_att_min_pos(nrows)
    run_pass = adjust_pass = logprob_pass = False
    if entry in ("forward_head_distinct", "forward_head_repeated"):
        distinct = entry == "forward_head_distinct"
        lm_head, fused_attn = True, distinct
        adjust_pass, logprob_pass = adjust, logprobs
        family, index = ("graph_exec", (long_pass,)) if distinct else ("graph_head_nf", (tiled_pass,))
        if adjust:
            family = family + "_adj"
        if logprobs:
            family, index = ("graph_exec_lp", (adjust, long_pass)) if distinct else ("graph_head_nf_lp", (adjust, tiled_pass))
    elif entry in ("forward_no_head", "prefill"):
        # forward(lm_head = false) captured with fused_attn = false whatever the rows; prefill()'s chunks hold several positions of a sequence
        lm_head, fused_attn = False, False
        family, index = "graph_prefill", (tiled_pass,)
    elif entry == "decode":
        lm_head, fused_attn = True, True
        family, index = "graph_exec", (long_pass,)
    elif entry.startswith("verify"):
        form = int(entry[len("verify"):])
        if form == -1:
            form = verify_form(nrows, top, caps)
        if form == 2 and not prefill_geometry:
            return None
        if form == 4 and not (has_scores and long_geometry):
            return None
        lm_head, fused_attn = True, False
        tiled_pass, long_pass, run_pass = form == 2, False, form == 4
        family, index = "graph_verify", (form // 2,)
    else:
        raise ValueError(entry)
    # enqueue_range()
    run_attn = (not fused_attn) and run_pass and has_scores and long_geometry
    tiled_attn = (not fused_attn) and (not run_attn) and tiled_pass and prefill_geometry
    long_attn = fused_attn and long_pass and has_scores and long_geometry
    per_pass = ("k_att_tiles",) if tiled_attn else ()
    layer = () if fused_attn else ("k_qkv_rope_append",)
    if long_attn or run_attn:
        layer += ("attention_long(run)" if run_attn else "attention_long",)
        attn = RUN if run_attn else LONG
    elif tiled_attn:
        layer += ("k_attention_prefill",)
        attn = TILED
    else:
        layer += ("k_attention<fused>" if fused_attn else "k_attention",)
        attn = ROW
    head = ()
    if lm_head:
        head = ("lm_head",) + (("k_logit_adjust",) if adjust_pass else ()) + ("k_argmax",) + (("k_token_logprobs",) if logprob_pass else ())
    return {"family": family, "index": index, "attn": attn, "launches": (per_pass, layer, head)}


def domain():
    for entry, nrows, top, caps, adjust, logprobs in itertools.product(ENTRIES, NROWS, TOPS, CAPS, [False, True], [False, True]):
        yield entry, nrows, top, caps, adjust, logprobs


def graphs_of_walk(passes):
    """the graphs a session must record for a walk: passes = [(entry, nrows, top, caps, adjust, logprobs)], one graph per distinct (launches, row
    count)"""
    seen = set()
    for entry, nrows, top, caps, adjust, logprobs in passes:
        p = parent_pass(entry, nrows, top, caps, adjust, logprobs)
        assert p is not None, (entry, nrows, top, caps)
        seen.add((p["launches"], nrows))
    return len(seen)


def parent_plan_at(launcher_kernel, fused, nrows, top, caps):
    """out[0] of tk_mi355x_attention_plan_at: launcher_kernel = tk_attention_plan's (0 k_attention, 1 narrow, 2 k_attention_prefill); has_scores
    stands for max_ctx > TK_LONG_ATT_MIN_POS"""
    has_scores, prefill_geometry, long_geometry = caps
    if fused:
        return 3 if has_scores and long_geometry and top >= long_att_min_pos(nrows) else launcher_kernel
    return 0 if launcher_kernel == 2 and top < 128 else launcher_kernel


def parent_plan_verify(launcher_kernel, nrows, top, caps):
    """out[0] of tk_mi355x_attention_plan_verify"""
    has_scores, prefill_geometry, long_geometry = caps
    if has_scores and long_geometry and top >= verify_run_min_pos(nrows):
        return 4
    return parent_plan_at(launcher_kernel, False, nrows, top, caps)


def plan_caps_possible(nrows, caps, launcher_kernel):
    """the plan entries work their caps out themselves: tk_attention_long_applies refuses more than TK_LONG_ATT_MAX_ROWS rows, and the launcher
    plans k_attention_prefill (2) exactly where tk_attention_prefill_applies (narrow, 1, aside)"""
    has_scores, prefill_geometry, long_geometry = caps
    return (not long_geometry or nrows <= TK_LONG_ATT_MAX_ROWS) and (launcher_kernel == 1 or (launcher_kernel == 2) == prefill_geometry)
