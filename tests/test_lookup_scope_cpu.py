"""CPU: lookup decoding beyond the greedy runner (csrc/llm/tk_lookup_scope.h).

1. The scheduler's verify requests WITH TABLES (csrc/llm/tk_llm_batcher.cpp) linked unchanged against the toy session (tests/stubs/llm_session_toy.cpp) in a
   stand-alone program of its own (tests/stubs/lookup_scope_soak.cpp): several threads submit verify requests whose rows each carry a mask, a sampling
   state, an adjustment and an n_top, in every combination of the four, beside plain, prompt and run-ahead traffic of other slots; every thread mirrors its
   sequence with the pure functions of namespace toy and compares every id and every record exactly.  The same program is built once more under the
   address and undefined-behaviour sanitizers and run as it is: a program with its own main, nothing preloaded.
2. The rules of tk_lookup_scope.h — scope, counter, window — through the library's host-only restatement check: tests/lookup_scope_ref.py against the
   header compiled into a small program (no GPU, no library)."""
import json
import os
import subprocess

import pytest

import lookup_scope_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "stubs")
CSRC = os.path.join(ROOT, "trackiellm_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
TIMEOUT = 120  # seconds; the program's own watchdog ends a stuck run after 10 s without a finished call


def build(out, *flags):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), "-I" + os.path.join(CSRC, "llm"),
                           "-I" + os.path.join(CSRC, "common"), "-I" + CSRC, os.path.join(STUBS, "lookup_scope_soak.cpp"), os.path.join(STUBS, "llm_session_toy.cpp"),
                           os.path.join(CSRC, "llm", "tk_llm_batcher.cpp"), "-o", out, "-lpthread"])
    return out


@pytest.fixture(scope="module")
def soak_bin(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("scope") / "lookup_scope_soak"))


@pytest.fixture(scope="module")
def soak_bin_sanitized(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("scope_san") / "lookup_scope_soak_asan"), "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")


def run(binary, *args):
    env = dict(os.environ)
    for k in ("TK_MI355X_BATCHER_TRACE", "TK_MI355X_BATCHER_DECODE_FIRST", "LD_PRELOAD"):
        env.pop(k, None)
    p = subprocess.run([binary] + [str(a) for a in args], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIMEOUT, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def check_soak(j, failing):
    print(json.dumps(j))
    assert j["mismatches"] == 0, j["notes"]
    assert j["breaches"] == 0, j["breach_list"]
    assert j["bad_errors"] == 0
    # the run reached what it is there to test: every combination of the four tables, every accepted count, the other traffic beside it
    assert len(j["by_combo"]) == 16 and all(v > 0 for v in j["by_combo"]), j["by_combo"]
    assert len(j["by_accepted"]) == 16 and all(v > 0 for v in j["by_accepted"]), j["by_accepted"]
    for key in ("tabled", "plain_verify", "steps", "prompts", "eos_cut", "verify_passes"):
        assert j[key] > 0, key
    assert j["widest"] > 16  # requests of several slots shared passes
    assert j["verify_passes"] < j["passes"]
    # a failing pass may hold run-ahead rows alone, whose owners went another way: then no request fails (the directed run fails a request for certain)
    assert j["failed_passes"] == 1 if failing else (j["failed_requests"] == 0 and j["failed_passes"] == 0)


@pytest.mark.parametrize("seed", [1, 2])
def test_tabled_verify_requests_beside_other_traffic(soak_bin, seed):
    check_soak(run(soak_bin, "soak", 9, seed, 600), False)


def test_a_failing_pass(soak_bin):
    """pass 30 fails in the middle of everything: its requests fail with the session's error, every later id and record is right again"""
    check_soak(run(soak_bin, "soak", 9, 1, 600, 30), True)


def test_entries_and_refusals(soak_bin):
    """a request without tables takes forward_verify, one with any table takes forward() in one pass; tables of the wrong length, n_top without records,
    records without n_top and values beyond their limits are refused before anything reaches the session"""
    j = run(soak_bin, "directed")
    assert j["failures"] == [] and j["mismatches"] == 0 and j["breaches"] == 0, j


def test_under_the_address_and_undefined_behaviour_sanitizers(soak_bin_sanitized):
    j = run(soak_bin_sanitized, "directed")
    assert j["failures"] == [] and j["mismatches"] == 0 and j["breaches"] == 0, j
    check_soak(run(soak_bin_sanitized, "soak", 9, 3, 400), False)
    check_soak(run(soak_bin_sanitized, "soak", 9, 1, 400, 30), True)


# ---- the rules of tk_lookup_scope.h against their restatement -----------------------------------------------------------------------------------

RULES_MAIN = r'''
#include <stdio.h>
#include <stdlib.h>
#include "tk_lookup_scope.h"
/* scope <flags> <sampled> <grammar> <adjusted> <logprobs> | window <last_n> <i> <n_acc> acc... drafts... | cut <nd> steps(0 refuse, 1 ok, 2 completes)... */
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (argv[1][0] == 's') { printf("%d\n", (int)tk_lookup_scope_allows((uint32_t)atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]))); return 0; }
    if (argv[1][0] == 'w') {
        const int last_n = atoi(argv[2]), i = atoi(argv[3]), n_acc = atoi(argv[4]);
        std::vector<int32_t> acc, dr, out((size_t)last_n + 1);
        for (int k = 0; k < n_acc; ++k) acc.push_back(atoi(argv[5 + k]));
        for (int k = 5 + n_acc; k < argc; ++k) dr.push_back(atoi(argv[k]));
        const int n = tk_lookup_row_window(acc.data(), n_acc, dr.data(), i, last_n, out.data());
        for (int k = 0; k < n; ++k) printf("%d ", out[(size_t)k]);
        printf("\n");
        return 0;
    }
    if (argv[1][0] == 'c') { /* a state is the number of drafts it has accepted; draft j's id is its behaviour */
        const int nd = atoi(argv[2]);
        std::vector<int32_t> dr;
        for (int k = 0; k < nd; ++k) dr.push_back(atoi(argv[3 + k]));
        struct St { int n = 0; bool done = false; };
        std::vector<St> states;
        const int kept = tk_lookup_grammar_cut(St(), dr.data(), nd, [](St* s, int32_t d) { if (d == 0) return false; s->n++; s->done = d == 2; return true; },
                                               [](const St& s) { return s.done; }, &states);
        printf("%d %zu", kept, states.size());
        for (const St& s : states) printf(" %d", s.n);
        printf("\n");
        return 0;
    }
    return 2;
}
'''


@pytest.fixture(scope="module")
def rules_bin(tmp_path_factory):
    d = tmp_path_factory.mktemp("scope_rules")
    src = d / "rules.cpp"
    src.write_text(RULES_MAIN)
    out = str(d / "rules")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(CSRC, "llm"), str(src), "-o", out])
    return out


def ask(rules_bin, *args):
    return subprocess.run([rules_bin] + [str(a) for a in args], stdout=subprocess.PIPE, timeout=TIMEOUT, text=True, check=True).stdout.split()


def test_scope_rule(rules_bin):
    for flags in range(16):
        for cond in range(16):
            c = [(cond >> b) & 1 for b in range(4)]
            assert ask(rules_bin, "scope", flags, *c) == [str(int(R.scope_allows(flags, *map(bool, c))))], (flags, c)


def test_window_rule(rules_bin):
    acc = [10, 11, 12, 13, 14]
    drafts = [20, 21, 22, 23]
    for last_n in (0, 1, 3, 5, 7, 64):
        for n_acc in (0, 2, 5):
            for i in range(len(drafts) + 1):
                got = [int(x) for x in ask(rules_bin, "window", last_n, i, n_acc, *acc[:n_acc], *drafts)]
                assert got == R.row_window(acc[:n_acc], drafts, i, last_n), (last_n, n_acc, i)


def test_grammar_cut_rule(rules_bin):
    for steps in ([], [1, 1, 1], [1, 0, 1], [0], [1, 2, 1], [2], [1, 1, 2]):
        kept, n_states, *ns = [int(x) for x in ask(rules_bin, "cut", len(steps), *steps)]
        want = R.cut_by(steps)
        assert kept == want and n_states == want + 1 and ns == list(range(want + 1)), steps


def test_the_restated_grammar_knows_the_tool_call_language():
    g = R.ToolCallGrammar
    for text in ['{}', '{ }', '{"tool_call": {"name": "a", "arguments": {}}}', '{"tool_call":{"name":"x\\n","arguments":{"k": [1, -2.5e3, true, null, "s", {}]}}}']:
        assert g.status(text.encode()) == "complete", text
        for cut in range(1, len(text)):
            assert g.status(text.encode()[:cut]) in ("partial", "complete"), (text, cut)
    for text in ['x', '{"tool_cal"', '{"tool_call": {"name": 1', '{}}', '{"tool_call": {"name": "a", "arguments": {"k": 01', '{"a"']:
        assert g.status(text.encode()) == "dead", text
    assert g.status(b'{') == "partial" and g.status(b'{"tool_call": {"name": "a", "arguments": {}}') == "partial"
