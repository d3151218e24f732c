#!/usr/bin/env python3
"""ASR language detection: what "auto" costs a transcription, and that a configured language costs what it cost before — developer tool, needs an
MI355X.  32 utterances (1 s of noise each, the 30 s window is padded on the device) through tk_mi355x_asr_transcribe_tokens at the multilingual
tiny geometry (synthetic weights), 16 greedy steps, host clock around the call (it ends in a stream synchronisation).

    python tools/time_asr_lang.py [rounds] [calls per sample] [other library]

One process per library and round (two builds of the library cannot share a process), the rounds interleaved: other, this, other, this ...
`other library`: a libtrackie_mi355x.so built from another commit — it knows no detection, so only its configured-language time is taken.
A child prints one line per language setting; the parent prints the table and, per setting, median and spread over the rounds."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, STEPS = 32, 16


def child(calls, settings):
    import trackiellm_amd as tk
    hp = tk.WhisperHP(80, 1500, 384, 6, 4, 448, 384, 6, 4, 51865)
    asr = tk.Asr(hp=hp, seed=6, max_batch=B)
    rng = np.random.default_rng(1)
    pcm = np.clip(rng.normal(0, 3000, (B, 16000)), -32768, 32767).astype(np.int16)
    for lang in settings:
        assert asr.set_language(lang) == 0
        first = asr.transcribe_tokens(pcm, STEPS, want_aux=False)[0]       # warm-up: code objects, the engine's buffers
        asr.transcribe_tokens(pcm, STEPS, want_aux=False)
        t0 = time.perf_counter()
        for _ in range(calls):
            toks = asr.transcribe_tokens(pcm, STEPS, want_aux=False)[0]
        dt = (time.perf_counter() - t0) / calls
        assert np.array_equal(toks, first)
        print("SAMPLE %s %.4f %d" % (lang, 1e3 * dt, int(toks[0, 0])), flush=True)
    asr.close()


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    other = sys.argv[3] if len(sys.argv) > 3 else None
    builds = ([("other", other, ["en"])] if other else []) + [("this", None, ["en", "auto"])]
    samples = {}
    for r in range(rounds):
        for name, path, settings in builds:
            env = dict(os.environ)
            if path:
                env["TK_MI355X_LIB"] = os.path.abspath(path)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(calls), ",".join(settings)], env=env, check=True,
                                 stdout=subprocess.PIPE, text=True, timeout=300).stdout
            for line in out.splitlines():
                if line.startswith("SAMPLE "):
                    _, lang, ms, tok = line.split()
                    samples.setdefault((name, lang), []).append(float(ms))
                    print("round %d  %-5s language %-4s  %8.3f ms per call of %d utterances  (first token of row 0: %s)" % (r, name, lang, float(ms), B, tok), flush=True)
    print()
    for (name, lang), v in samples.items():
        v = np.array(v)
        print("%-5s language %-4s  median %8.3f ms  min %8.3f  max %8.3f  over %d rounds of %d calls" % (name, lang, np.median(v), v.min(), v.max(), v.size, calls))
    if ("this", "auto") in samples:
        d = np.array(samples[("this", "auto")]) - np.array(samples[("this", "en")])
        print("auto - configured, same process, per round (ms): %s   median %.4f" % (" ".join("%.4f" % x for x in d), np.median(d)))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), sys.argv[3].split(","))
    else:
        main()
