/*
 * tk_grammar_walk.h — may a token follow a grammar state?  One definition for the host and for one lane of k_grammar_mask (host + device).
 *
 * TkGrammarState::mask() (llm/tk_grammar.h) walks the vocabulary's trie against the parse stacks on the host.  The same answer decomposes per token:
 * token t is allowed iff walking its bytes through TkGrammarState::step from the current stacks leaves a stack alive.  That walk is restated here
 * over plain arrays, iteratively and in bounded storage, so that k_grammar_mask (llm/tk_llm_kernels.hip) runs it with one lane per token and
 * tk_grammar_mask_row runs it in a host loop: both give the same bits.
 *
 * Grammar image (TkGrammar::flatten).  Every rule's elements back to back in ONE array; a position is an index into it (a 16-bit number: a grammar
 * of more than TK_GW_MAX_ELEMS elements has no image).  rule_off[n_rules + 1] = where each rule starts; elems[i] = type | value << 2 with the types
 * of TkGrammar (END 0, ALT 1, RULE 2: value = rule id, SET 3: value = set index); sets[n_sets][8] = the 256-bit byte sets.
 *
 * State image (TkGrammarState::export_image).  A parse stack is a list of positions still to be matched, top last.  The stacks of a state share
 * their bottom: `bottom` holds the longest common prefix of the non-empty stacks once, read-only; a stack is (base, n, priv[n]) = the first `base`
 * entries of `bottom` followed by its private entries.  A lane's own stacks have the same form, so a stack that pops below its private entries goes
 * on in the shared bottom (base shrinks).  The form is kept canonical — base as large as the entries allow — so equal stacks compare equal.
 *
 * The walk.  TkGrammarState::advance's recursion is a worklist inside the stack set itself: a stack whose top is a rule reference is taken out and
 * its alternatives are inserted, until every stack's top is a byte set or the stack is empty; insertion drops a stack the set already holds.  Caps:
 * TK_GW_MAX_STACKS stacks per set, TK_GW_MAX_PRIV private entries per stack, TK_GW_MAX_BOTTOM shared entries, TK_GW_MAX_STEPS rule expansions per
 * token.  A cap exceeded answers TK_GW_UNDECIDED, never a guess: left recursion overflows the private entries, an empty loop runs out of steps.
 * Measured for the tool-call grammar over every prefix of the golden documents: a state has at most 12 stacks of at most 4 private entries, and a
 * token walk needs 12 private entries at the most (the piece "[[[[" behind an open array: two return positions per nested array); 15 leaves room
 * for one more level (tests/test_grammar_mask_cpu.py holds the walk to zero undecided tokens there).
 *
 * Per-lane storage: two stack sets of TK_GW_MAX_STACKS * sizeof(TkGwStack) = 2 * 512 bytes.  On the device that is scratch memory (DESIGN.md §5
 * has the kernel's resource report and why it is not LDS).
 */
#ifndef TK_GRAMMAR_WALK_H
#define TK_GRAMMAR_WALK_H

#include <stdint.h>

#include "tk_exact_math.h" /* TK_HD */

#ifndef TK_GW_MAX_STACKS /* a stand-alone host program may try other caps */
#define TK_GW_MAX_STACKS 16
#define TK_GW_MAX_PRIV 15
#endif
#define TK_GW_MAX_BOTTOM 64
#define TK_GW_MAX_STEPS 2048
#define TK_GW_MAX_ELEMS 65535
#define TK_GW_LDS_WORDS 4096 /* k_grammar_mask stages a grammar image of at most this many 32-bit words (16 KiB) in LDS; a larger one is read from global memory */

enum { TK_GW_FORBIDDEN = 0, TK_GW_ALLOWED = 1, TK_GW_UNDECIDED = 2 };
enum { TK_GW_END = 0, TK_GW_ALT = 1, TK_GW_RULE = 2, TK_GW_SET = 3 };

struct TkGrammarImage {
    const uint32_t* rule_off; /* [n_rules + 1] */
    const uint32_t* elems;    /* [n_elems] type | value << 2 */
    const uint32_t* sets;     /* [n_sets][8] */
    int32_t n_rules, n_elems, n_sets, root;
};

struct TkGwStack {
    uint8_t base, n; /* bottom[0 .. base) then priv[0 .. n) */
    uint16_t priv[TK_GW_MAX_PRIV];
};

struct TkGrammarStateImage {
    int32_t mask_row; /* the row of the mask array this state's bits go to */
    int32_t grammar;  /* which grammar image of the launch's table the state belongs to */
    int32_t complete; /* some stack is empty: the end-of-sequence token is allowed */
    int32_t n_bottom, n_stacks;
    uint16_t bottom[TK_GW_MAX_BOTTOM];
    TkGwStack stacks[TK_GW_MAX_STACKS];
};

struct TkGwSet {
    int32_t n;
    TkGwStack s[TK_GW_MAX_STACKS];
};

TK_HD uint32_t tk_gw_type(const TkGrammarImage& g, uint32_t pos) { return g.elems[pos] & 3u; }
TK_HD uint32_t tk_gw_value(const TkGrammarImage& g, uint32_t pos) { return g.elems[pos] >> 2; }
/* an END or an ALT closes a sequence: nothing is left to match at such a position */
TK_HD bool tk_gw_open(const TkGrammarImage& g, uint32_t pos) { return tk_gw_type(g, pos) >= TK_GW_RULE; }

TK_HD bool tk_gw_empty(const TkGwStack& s) { return s.base == 0 && s.n == 0; }
TK_HD uint32_t tk_gw_top(const TkGwStack& s, const uint16_t* bottom) { return s.n ? s.priv[s.n - 1] : bottom[s.base - 1]; }
TK_HD void tk_gw_pop(TkGwStack* s) {
    if (s->n) --s->n;
    else --s->base;
}
/* false: the private entries are full */
TK_HD bool tk_gw_push(TkGwStack* s, uint32_t pos) {
    if (s->n >= TK_GW_MAX_PRIV) return false;
    s->priv[s->n++] = (uint16_t)pos;
    return true;
}
/* a private entry that repeats the shared bottom moves into it */
TK_HD void tk_gw_canon(TkGwStack* s, const uint16_t* bottom, int n_bottom) {
    while (s->n > 0 && s->base < n_bottom && s->priv[0] == bottom[s->base]) {
        for (int i = 1; i < s->n; ++i) s->priv[i - 1] = s->priv[i];
        --s->n;
        ++s->base;
    }
}
TK_HD bool tk_gw_same(const TkGwStack& a, const TkGwStack& b) {
    if (a.base != b.base || a.n != b.n) return false;
    for (int i = 0; i < a.n; ++i)
        if (a.priv[i] != b.priv[i]) return false;
    return true;
}
/* false: the set is full and does not hold the stack yet */
TK_HD bool tk_gw_insert(TkGwSet* set, TkGwStack s, const uint16_t* bottom, int n_bottom) {
    tk_gw_canon(&s, bottom, n_bottom);
    for (int i = 0; i < set->n; ++i)
        if (tk_gw_same(set->s[i], s)) return true;
    if (set->n >= TK_GW_MAX_STACKS) return false;
    set->s[set->n++] = s;
    return true;
}

/* TkGrammarState::advance over the whole set: afterwards every stack is empty or has a byte set on top.  false: a cap was exceeded */
TK_HD bool tk_gw_expand(const TkGrammarImage& g, TkGwSet* set, const uint16_t* bottom, int n_bottom, int* steps) {
    int i = 0;
    while (i < set->n) {
        TkGwStack st = set->s[i];
        if (tk_gw_empty(st)) { ++i; continue; }
        const uint32_t top = tk_gw_top(st, bottom);
        if (tk_gw_type(g, top) != TK_GW_RULE) { ++i; continue; }
        if (++*steps > TK_GW_MAX_STEPS) return false;
        set->s[i] = set->s[--set->n]; /* taken out; whatever moved into its place is looked at next */
        tk_gw_pop(&st);
        if (tk_gw_open(g, top + 1) && !tk_gw_push(&st, top + 1)) return false;
        uint32_t a = g.rule_off[tk_gw_value(g, top)];
        for (;;) { /* one stack per alternative of the rule */
            TkGwStack ns = st;
            if (tk_gw_open(g, a) && !tk_gw_push(&ns, a)) return false;
            if (!tk_gw_insert(set, ns, bottom, n_bottom)) return false;
            while (tk_gw_open(g, a)) ++a;
            if (tk_gw_type(g, a) == TK_GW_END) break;
            ++a;
        }
    }
    return true;
}

/* the bytes of one token against one state: TK_GW_ALLOWED, TK_GW_FORBIDDEN or TK_GW_UNDECIDED.  An empty piece is never allowed (TkTokenTrie) */
TK_HD int tk_grammar_token_walk(const TkGrammarImage& g, const TkGrammarStateImage& st, const uint16_t* bottom, const uint8_t* bytes, int n) {
    if (n <= 0) return TK_GW_FORBIDDEN;
    TkGwSet set[2];
    int cur = 0, steps = 0;
    set[0].n = st.n_stacks;
    for (int i = 0; i < st.n_stacks; ++i) set[0].s[i] = st.stacks[i];
    for (int k = 0; k < n; ++k) {
        const uint32_t b = bytes[k];
        TkGwSet& in = set[cur];
        TkGwSet& out = set[cur ^ 1];
        out.n = 0;
        for (int i = 0; i < in.n; ++i) {
            TkGwStack s = in.s[i];
            if (tk_gw_empty(s)) continue;
            const uint32_t top = tk_gw_top(s, bottom);
            if (tk_gw_type(g, top) != TK_GW_SET || !((g.sets[tk_gw_value(g, top) * 8 + (b >> 5)] >> (b & 31)) & 1u)) continue;
            tk_gw_pop(&s);
            if (tk_gw_open(g, top + 1) && !tk_gw_push(&s, top + 1)) return TK_GW_UNDECIDED;
            if (!tk_gw_insert(&out, s, bottom, st.n_bottom)) return TK_GW_UNDECIDED;
        }
        if (out.n == 0) return TK_GW_FORBIDDEN;
        if (!tk_gw_expand(g, &out, bottom, st.n_bottom, &steps)) return TK_GW_UNDECIDED;
        cur ^= 1;
    }
    return TK_GW_ALLOWED;
}

/* token t of one mask row, as lane t of k_grammar_mask decides it: the end-of-sequence token is allowed iff the state is complete, whatever its piece */
TK_HD int tk_grammar_mask_token(const TkGrammarImage& g, const TkGrammarStateImage& st, const uint16_t* bottom, const uint32_t* offsets, const uint8_t* pieces,
                                int32_t t, int32_t eos) {
    if (t == eos) return st.complete ? TK_GW_ALLOWED : TK_GW_FORBIDDEN;
    return tk_grammar_token_walk(g, st, bottom, pieces + offsets[t], (int)(offsets[t + 1] - offsets[t]));
}

/* one mask row on the host: the kernel's lanes in a loop.  Every word of the row is written whole; returns the number of undecided tokens (written 0) */
static inline int32_t tk_grammar_mask_row(const TkGrammarImage& g, const TkGrammarStateImage& st, const uint32_t* offsets, const uint8_t* pieces, int32_t vocab,
                                          int32_t eos, uint32_t* bits) {
    int32_t undecided = 0;
    for (int32_t w = 0; w < (vocab + 31) / 32; ++w) bits[w] = 0u;
    for (int32_t t = 0; t < vocab; ++t) {
        const int r = tk_grammar_mask_token(g, st, st.bottom, offsets, pieces, t, eos);
        if (r == TK_GW_ALLOWED) bits[t >> 5] |= 1u << (t & 31);
        undecided += r == TK_GW_UNDECIDED;
    }
    return undecided;
}

#endif
