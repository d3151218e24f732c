"""CPU: the runner scheduler (csrc/llm/tk_llm_batcher.cpp: continuous batching, run-ahead rows, prompt prefix cache, context shifts, verify requests,
log-probability records, hold rules) linked UNCHANGED against a toy session (tests/stubs/llm_session_toy.cpp) in a stand-alone program
(tests/stubs/batcher_soak.cpp).  The toy's cache row is a chain hash of everything the row attended to, so any difference in what a row attended to —
a stale row, a row kept after a shift, a copy from the wrong slot, rows out of order — shows in a sampled id; every runner thread compares every id and
record with a private single-threaded mirror, exactly.  The toy also checks the rules a real session relies on (rows per pass, ascending positions,
never-written rows, the source / destination rule of a copy launch, kv_shift's range, optional tables given exactly when needed).

It cannot see arithmetic, graph replay or stream ordering inside the real session: those stay with tests/test_prefix_cache_gpu.py,
tests/test_context_shift_gpu.py, tests/test_lookup_gpu.py and tests/test_runner_mix_gpu.py.

The soak cases also assert that they reached what they claim to test: a soak that proves nothing fails."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "stubs")
CSRC = os.path.join(ROOT, "trackiellm_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
TIMEOUT = 120  # seconds; the program's own watchdog ends a stuck run after 10 s without a finished call

SCENARIOS = ["ahead_one", "no_ahead", "discard", "keep", "copy", "shift", "verify_record", "verify_waits", "many_copies", "src_dst", "shift_under_copy", "mixed_pass",
             "refusals",
             "failed_pass"]


@pytest.fixture(scope="module")
def soak_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("batcher") / "batcher_soak")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), "-I" + os.path.join(CSRC, "llm"),
                           "-I" + os.path.join(CSRC, "common"), "-I" + CSRC, os.path.join(STUBS, "batcher_soak.cpp"),
                           os.path.join(STUBS, "llm_session_toy.cpp"), os.path.join(CSRC, "llm", "tk_llm_batcher.cpp"), "-o", out, "-lpthread"])
    return out


def run(soak_bin, *args, decode_first=None):
    env = dict(os.environ)
    env.pop("TK_MI355X_BATCHER_TRACE", None)
    env.pop("TK_MI355X_BATCHER_DECODE_FIRST", None)
    if decode_first is not None:
        env["TK_MI355X_BATCHER_DECODE_FIRST"] = str(decode_first)
    p = subprocess.run([soak_bin] + [str(a) for a in args], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIMEOUT, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def check_soak(j, runners, failing):
    print(json.dumps(j))
    assert j["mismatches"] == 0, j["notes"]
    assert j["breaches"] == 0, j["breach_list"]
    assert j["accounting_errors"] == 0, j["accounting"]
    # the run reached what it is there to test
    for key in ("passes", "widest", "kept", "copied", "wasted", "shifts", "waiter_handovers", "done_handovers_with_record", "done_handovers_without_record",
                "verify_eos", "tool_feeds", "abandoned", "slot_changes", "cache_toggles", "penalties_over_empty_window"):
        assert j[key] > 0, key
    assert len(j["verify_by_accepted"]) == 16 and all(v > 0 for v in j["verify_by_accepted"]), j["verify_by_accepted"]
    if runners >= 64:
        assert j["widest"] == 256
    assert (j["failed_requests"] > 0 and j["failed_passes"] == 1) if failing else (j["failed_requests"] == 0 and j["failed_passes"] == 0)
    if not failing:
        assert j["rows"] + j["wasted"] == j["session_rows"]


@pytest.mark.parametrize("decode_first", [0, 1])
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("runners,calls", [(8, 1000), (64, 300)])
def test_soak(soak_bin, runners, calls, seed, decode_first):
    check_soak(run(soak_bin, "soak", runners, seed, calls, decode_first=decode_first), runners, False)


@pytest.mark.parametrize("decode_first", [0, 1])
def test_soak_with_a_failed_pass(soak_bin, decode_first):
    """pass 40 fails in the middle of everything: its requests and waiters fail with the session's error, every later id is right again"""
    check_soak(run(soak_bin, "soak", 8, 1, 1000, 40, decode_first=decode_first), 8, True)


def test_the_scenario_list_is_the_programs(soak_bin):
    p = subprocess.run([soak_bin, "list"], stdout=subprocess.PIPE, timeout=TIMEOUT, text=True)
    assert p.returncode == 0 and p.stdout.split() == SCENARIOS


@pytest.mark.parametrize("name", SCENARIOS)
def test_scenario(soak_bin, name):
    """one promise of tk_llm_batcher.h's header comment each, scripted in lock step (tests/stubs/batcher_soak.cpp, "directed scenarios")"""
    j = run(soak_bin, "scenario", name)
    print(json.dumps(j))
    assert j["failures"] == [], j["failures"]
    assert j["mismatches"] == 0, j["notes"]
    assert j["breaches"] == 0, j["breach_list"]
