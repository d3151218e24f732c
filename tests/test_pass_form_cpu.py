"""CPU: the description of a pass (csrc/llm/tk_pass_form.h: the resolved attention, the key of the session's graph cache, the verify form, the kernel
numbers the plan entries report) in a stand-alone program (tests/stubs/pass_form_check.cpp) against tests/pass_form_ref.py, which restates what the
session did before the header existed — five mutable members, eight graph array families indexed by the unresolved members, the gating inside
enqueue_range() — over every entry x row count x top position x capability x adjust x logprobs of the domain below.

It cannot see that the session describes its passes the way the program does: tests/test_pass_forms_gpu.py counts the graphs a session records."""
import os
import subprocess

import pytest

import pass_form_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "stubs")
CSRC = os.path.join(ROOT, "trackiellm_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.fixture(scope="module")
def check_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pass_form") / "pass_form_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                           "-I" + os.path.join(CSRC, "llm"), "-I" + os.path.join(CSRC, "common"), "-I" + CSRC, os.path.join(STUBS, "pass_form_check.cpp"), "-o", out])
    return out


def caps_of(bits):
    return (bool(bits & 4), bool(bits & 2), bool(bits & 1))


@pytest.fixture(scope="module")
def forms(check_bin):
    """{case: None (refused) | (attn, rope, head, adjust, logprobs, key)}, {(nrows, top, caps): verify_form}, TK_PASS_FORM_KEYS"""
    lines = subprocess.run([check_bin, "forms"], stdout=subprocess.PIPE, check=True, text=True, timeout=60).stdout.splitlines()
    assert lines[0].startswith("keys ")
    out, vform = {}, {}
    for ln in lines[1:]:
        case, rest = ln.split(" -> ")
        got, vf = rest.split("; ")
        entry, nrows, top, cb, adjust, logprobs = case.split()
        key = (entry, int(nrows), int(top), caps_of(int(cb)), adjust == "1", logprobs == "1")
        assert key not in out
        out[key] = None if got == "refused" else tuple(int(v) for v in got.split())
        vform[(int(nrows), int(top), caps_of(int(cb)))] = int(vf)
    return out, vform, int(lines[0].split()[1])


def test_the_program_walks_the_whole_domain(forms):
    assert set(forms[0]) == set(ref.domain())
    assert len(forms[0]) == 9 * 7 * 9 * 8 * 4


def test_resolved_attention_and_refusals_are_the_parents(forms):
    for case, got in forms[0].items():
        want = ref.parent_pass(*case)
        assert (got is None) == (want is None), case
        if want is not None:
            assert got[0] == want["attn"], (case, got, want)


def test_equal_keys_iff_equal_launches(forms):
    """in both directions, over all pairs: a key stands for exactly one tuple of launches and the other way round"""
    key_of, launches_of = {}, {}
    for case, got in forms[0].items():
        if got is None:
            continue
        launches = ref.parent_pass(*case)["launches"]
        key = got[5]
        assert key_of.setdefault(launches, key) == key, (case, "one tuple of launches under two keys")
        assert launches_of.setdefault(key, launches) == launches, (case, "two tuples of launches under one key")
    assert len(key_of) == len(launches_of) > 1


def test_keys_are_dense_and_below_the_bound(forms):
    keys = {got[5] for got in forms[0].values() if got is not None}
    assert min(keys) >= 0 and max(keys) < forms[2]
    # every form these entries can describe is reached: without the head ROW and TILED with rope apart (rope in attention without the head is a
    # pipeline stage's); with it (rope in: ROW, LONG; rope apart: ROW, TILED) x adjust x logprobs, and RUN, which only verify passes take, plain
    assert len(keys) == 2 + 4 * 4 + 1


def test_a_pass_without_the_head_has_no_adjust_or_logprobs(forms):
    for case, got in forms[0].items():
        if got is not None and not got[2]:
            assert got[3] == 0 and got[4] == 0, case


def test_verify_forms_0_and_2_are_the_sampling_pass_with_repeated_sequences(forms):
    f = forms[0]
    for nrows in ref.NROWS:
        for caps in ref.CAPS:
            if caps[1]:
                assert f[("verify2", nrows, 128, caps, False, False)][5] == f[("forward_head_repeated", nrows, 128, caps, False, False)][5]
            assert f[("verify0", nrows, 0, caps, False, False)][5] == f[("forward_head_repeated", nrows, 0, caps, False, False)][5]


def test_verify_form_is_the_parents_everywhere(forms):
    for (nrows, top, caps), got in forms[1].items():
        assert got == ref.verify_form(nrows, top, caps), (nrows, top, caps)


def test_plan_entries_through_the_resolver(check_bin):
    lines = subprocess.run([check_bin, "plans"], stdout=subprocess.PIPE, check=True, text=True, timeout=60).stdout.splitlines()[1:]
    assert len(lines) == 3 * 7 * 9 * 8
    checked = 0
    for ln in lines:
        case, got = ln.split(" -> ")
        k, nrows, top, cb = (int(v) for v in case.split())
        caps = caps_of(cb)
        fused, plain, verify = (int(v) for v in got.split())
        if k != 2:  # the launcher plans k_attention_prefill for passes that rope apart only
            if ref.plan_caps_possible(nrows, caps, k):
                assert fused == ref.parent_plan_at(k, True, nrows, top, caps), ln
        if ref.plan_caps_possible(nrows, caps, k):
            assert plain == ref.parent_plan_at(k, False, nrows, top, caps), ln
            assert verify == ref.parent_plan_verify(k, nrows, top, caps), ln
            checked += 1
    assert checked > 500
