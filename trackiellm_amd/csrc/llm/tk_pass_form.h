/*
 * tk_pass_form.h — the one description of a pass of TkLlmSession (tk_llm_engine.h), host only: no device, no state.
 *
 * A pass is layers of (q|k|v, rope/append, attention, o, gate|up, down) and, with the head, (norm + lm_head, [adjust], pick, [log-probabilities]).
 * What varies between passes is written down here once: whoever runs a pass describes it as a TkPassForm, enqueue_range() launches what the form
 * says, and the session's graph cache is indexed by tk_pass_form_key() — so two passes share a graph exactly when they are the same launches.
 * DESIGN.md "The forms of a pass" has the table entry -> form.  TK_MI355X_NO_FUSE is no part of the form: it is read when a pass is recorded.
 */
#ifndef TK_PASS_FORM_H
#define TK_PASS_FORM_H

#include "tk_llm_kernels.h" /* TK_LONG_ATT_MAX_ROWS, tk_long_att_min_pos, tk_verify_run_min_pos */

/* a pass that holds several positions of a sequence takes k_attention_prefill (16 rows of a sequence per workgroup) from this top position on;
 * shorter contexts keep k_attention's per-row form (3 us per launch quicker below ~128 positions, profiles/r05_prefill_attention.txt) */
#define TK_TILED_ATT_FROM_POS 128

/* the RESOLVED attention of a pass; all four are bit-identical, so the choice never shows in a result */
enum TkPassAttn {
    TK_ATT_ROW = 0, /* k_attention, one workgroup per (row, KV group) */
    TK_ATT_TILED,   /* k_att_tiles once per pass, then k_attention_prefill */
    TK_ATT_LONG,    /* the long-context form of a pass that holds every sequence once: append + scores + PV launches spread over the chip */
    TK_ATT_RUN      /* the run variant of the long-context form: several consecutive positions of a sequence (verify passes, and forward() with the head
                     * over rows that are such runs: tk_pass_form_rows) */
};

struct TkPassForm {
    bool head;              /* final norm + lm_head + pick */
    bool rope_in_attention; /* every sequence at most once in the pass: the attention launch ropes and appends the rows itself; false: a
                             * k_qkv_rope_append launch of its own in front of it.  TILED and RUN need false, LONG needs true */
    TkPassAttn attn;
    bool adjust;            /* k_logit_adjust in front of the pick (head only) */
    bool logprobs;          /* k_token_logprobs behind the pick (head only) */
};

/* what the session knows when it describes a pass */
struct TkPassCaps {
    bool has_scores;             /* the long-context scratch exists: the window can reach TK_LONG_ATT_MIN_POS and the geometry fits */
    bool prefill_geometry;       /* tk_attention_prefill_applies */
    bool long_geometry_at_nrows; /* tk_attention_long_applies at the pass's row count */
};

/* a pass that holds every sequence once */
static inline TkPassAttn tk_pass_attn_once(int nrows, int top, const TkPassCaps& c) {
    return c.has_scores && c.long_geometry_at_nrows && nrows <= TK_LONG_ATT_MAX_ROWS && top >= tk_long_att_min_pos(nrows) ? TK_ATT_LONG : TK_ATT_ROW;
}
/* a pass that may hold several positions of a sequence */
static inline TkPassAttn tk_pass_attn_several(int top, const TkPassCaps& c) {
    return top >= TK_TILED_ATT_FROM_POS && c.prefill_geometry ? TK_ATT_TILED : TK_ATT_ROW;
}

/* the form forward_verify(form = -1) takes for nrows rows whose highest position is `top`: 4 from tk_verify_run_min_pos(nrows) where the run form
 * applies, else 2 from TK_TILED_ATT_FROM_POS where k_attention_prefill applies, else 0 */
static inline int tk_verify_form(int nrows, int top, const TkPassCaps& c) {
    if (c.has_scores && c.long_geometry_at_nrows && top >= tk_verify_run_min_pos(nrows)) return 4;
    return tk_pass_attn_several(top, c) == TK_ATT_TILED ? 2 : 0;
}
/* nullptr, or why forward_verify refuses a form given by number */
#define TK_PASS_STR_(x) #x
#define TK_PASS_STR(x) TK_PASS_STR_(x)
static inline const char* tk_verify_form_error(int form, const TkPassCaps& c) {
    if (form != 0 && form != 2 && form != 4) return "verify pass: form must be -1, 0, 2 or 4";
    if (form == 2 && !c.prefill_geometry) return "verify pass: the tiled attention form does not take this head geometry";
    if (form == 4 && !(c.has_scores && c.long_geometry_at_nrows))
        return "verify pass: the run form takes at most " TK_PASS_STR(TK_LONG_ATT_MAX_ROWS) " rows, head_dim 64 or 128, and a context window beyond " TK_PASS_STR(TK_LONG_ATT_MIN_POS) " positions";
    return nullptr;
}
static inline TkPassAttn tk_verify_attn(int form) { return form == 4 ? TK_ATT_RUN : form == 2 ? TK_ATT_TILED : TK_ATT_ROW; }

/* a pass over host-described or device-advanced rows whose highest position is `top`.  once: every sequence at most once AND the caller wants
 * rope/append inside the attention launch (forward() without the head does not: it shares the prompt chunks' graphs) */
static inline TkPassForm tk_pass_form(bool head, bool once, int nrows, int top, const TkPassCaps& c, bool adjust = false, bool logprobs = false) {
    return TkPassForm{head, once, once ? tk_pass_attn_once(nrows, top, c) : tk_pass_attn_several(top, c), head && adjust, head && logprobs};
}
/* a verify pass of form 0 / 2 / 4 is a sampling pass that holds several positions of a sequence, with the attention given */
static inline TkPassForm tk_pass_form_verify(int form) { return TkPassForm{true, false, tk_verify_attn(form), false, false}; }
/* forward() with the head, described row by row.  once: every sequence at most once — tk_pass_form's form.  Otherwise some sequence stands at several
 * positions; runs: the rows also keep forward_verify's layout rule (each sequence's rows consecutive, ascending, contiguous).  Such a pass is a verify
 * pass whose rows may carry masks, sampling states, adjustments and log-probabilities (tk_lookup_scope.h), so it takes the attention a verify pass of
 * these rows takes: the run form where tk_verify_form says 4, else the tiles or the per-row form as before */
static inline TkPassForm tk_pass_form_rows(bool once, bool runs, int nrows, int top, const TkPassCaps& c, bool adjust = false, bool logprobs = false) {
    if (once || !runs || tk_verify_form(nrows, top, c) != 4) return tk_pass_form(true, once, nrows, top, c, adjust, logprobs);
    return TkPassForm{true, false, TK_ATT_RUN, adjust, logprobs};
}

/* the kernel number tk_mi355x_attention_plan_at / _plan_verify report: the launcher's own plan (0 k_attention, 1 its narrow form, 2
 * k_attention_prefill) with the pass's choice on top — 3 the long-context form, 4 its run variant, 0 for a tiled plan below TK_TILED_ATT_FROM_POS */
static inline int tk_plan_kernel_at(int launcher_kernel, bool fused, int nrows, int top, const TkPassCaps& c) {
    if (fused) return tk_pass_attn_once(nrows, top, c) == TK_ATT_LONG ? 3 : launcher_kernel;
    return launcher_kernel == 2 && tk_pass_attn_several(top, c) != TK_ATT_TILED ? 0 : launcher_kernel;
}
static inline int tk_plan_kernel_verify(int launcher_kernel, int nrows, int top, const TkPassCaps& c) {
    return tk_verify_form(nrows, top, c) == 4 ? 4 : tk_plan_kernel_at(launcher_kernel, false, nrows, top, c);
}

/* dense key of a form: two forms have the same key iff enqueue_range() issues the same launches for them.  Five attention shapes — (rope in
 * attention: ROW, LONG), (rope apart: ROW, TILED, RUN) —, alone without the head, times adjust x logprobs with it */
#define TK_PASS_FORM_KEYS 25
static inline int tk_pass_form_key(const TkPassForm& f) {
    const int att = f.rope_in_attention ? (f.attn == TK_ATT_LONG ? 1 : 0) : f.attn == TK_ATT_TILED ? 3 : f.attn == TK_ATT_RUN ? 4 : 2;
    return f.head ? 5 + 4 * att + (f.adjust ? 2 : 0) + (f.logprobs ? 1 : 0) : att;
}

#endif
