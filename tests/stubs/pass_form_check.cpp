/* csrc/llm/tk_pass_form.h on the CPU: every entry of TkLlmSession described the way the session describes it, over the whole domain that
 * tests/test_pass_form_cpu.py compares with tests/pass_form_ref.py.  No GPU, no HIP call.
 *   pass_form_check forms   one line per case: entry nrows top caps adjust logprobs -> refused | attn rope head adjust logprobs key; verify_form
 *   pass_form_check plans   one line per case: launcher_kernel nrows top caps -> plan_at(fused) plan_at(not fused) plan_verify
 * caps is a number: 4 has_scores + 2 prefill_geometry + 1 long_geometry_at_nrows */
#include <stdio.h>
#include <string.h>

#include "tk_pass_form.h"

static const char* const kEntries[] = {"forward_head_distinct", "forward_head_repeated", "forward_no_head", "prefill", "decode", "verify-1", "verify0", "verify2", "verify4"};
static const int kRows[] = {1, 4, 5, 8, 9, 16, 256};
static const int kTops[] = {0, 127, 128, 255, 256, 511, 512, 767, 768};

/* false: the entry refuses */
static bool describe(int entry, int nrows, int top, const TkPassCaps& c, bool adjust, bool logprobs, TkPassForm* f) {
    switch (entry) {
    case 0: *f = tk_pass_form(true, true, nrows, top, c, adjust, logprobs); return true;   /* forward(): lm_head && distinct */
    case 1: *f = tk_pass_form(true, false, nrows, top, c, adjust, logprobs); return true;
    case 2: *f = tk_pass_form(false, false, nrows, top, c, adjust, logprobs); return true; /* forward(lm_head = false): adjust / logprobs are not looked at */
    case 3: *f = tk_pass_form(false, false, nrows, top, c); return true;                   /* a chunk of prefill() */
    case 4: *f = tk_pass_form(true, true, nrows, top, c); return true;                     /* a step of decode() */
    default: {
        int form = entry == 5 ? -1 : entry == 6 ? 0 : entry == 7 ? 2 : 4;
        if (form == -1) form = tk_verify_form(nrows, top, c);
        if (tk_verify_form_error(form, c)) return false;
        *f = tk_pass_form_verify(form);
        return true;
    }
    }
}

int main(int argc, char** argv) {
    const bool plans = argc > 1 && !strcmp(argv[1], "plans");
    if (argc < 2 || (!plans && strcmp(argv[1], "forms"))) { fprintf(stderr, "usage: pass_form_check forms|plans\n"); return 2; }
    printf("keys %d\n", TK_PASS_FORM_KEYS);
    for (int nrows : kRows)
        for (int top : kTops)
            for (int cb = 0; cb < 8; ++cb) {
                const TkPassCaps c{(cb & 4) != 0, (cb & 2) != 0, (cb & 1) != 0};
                if (plans) {
                    for (int k = 0; k < 3; ++k)
                        printf("%d %d %d %d -> %d %d %d\n", k, nrows, top, cb, tk_plan_kernel_at(k, true, nrows, top, c), tk_plan_kernel_at(k, false, nrows, top, c),
                               tk_plan_kernel_verify(k, nrows, top, c));
                    continue;
                }
                for (int e = 0; e < 9; ++e)
                    for (int al = 0; al < 4; ++al) {
                        TkPassForm f{};
                        printf("%s %d %d %d %d %d -> ", kEntries[e], nrows, top, cb, al >> 1, al & 1);
                        if (!describe(e, nrows, top, c, (al & 2) != 0, (al & 1) != 0, &f)) printf("refused");
                        else printf("%d %d %d %d %d %d", (int)f.attn, (int)f.rope_in_attention, (int)f.head, (int)f.adjust, (int)f.logprobs, tk_pass_form_key(f));
                        printf("; %d\n", tk_verify_form(nrows, top, c));
                    }
            }
    return 0;
}
