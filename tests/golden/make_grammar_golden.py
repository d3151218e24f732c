"""tool_call_grammar_samples.json — the reference's tool-call grammar (src/ai_models/grammars/tool_call.gbnf) on sample documents:
for every document, (bytes accepted, complete) as the library's GBNF engine answers when it is armed with that FILE.  The test then
checks that the built-in grammar text answers the same on every sample, without the reference tree.  Samples: the hand-picked
documents, 100 generated tool calls (tests/test_grammar_cpu.py: gen_call, seed 11) and a one-byte mutation of each longer one.
Run after building the library:  python tests/golden/make_grammar_golden.py <reference tree>/src/ai_models/grammars/tool_call.gbnf"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from test_grammar_cpu import check, gen_call  # noqa: E402


def samples():
    rng = random.Random(11)
    docs = ["{}", "{ }", '{"x":1}', '{"tool_call":{"name":5}}', "", "{", '{"tool_call":{"name":"a","arguments":{"k":01}}}']
    docs += ["{" + gen_call(rng, 0) + "}" for _ in range(100)]
    for d in list(docs):
        if len(d) > 4:
            docs.append(d[: rng.randrange(1, len(d))] + rng.choice(['"', "x", "}", " ", ":"]) + d[rng.randrange(1, len(d)):])
    return docs


if __name__ == "__main__":
    ref = open(sys.argv[1]).read()
    out = [{"doc": d, "accepted_bytes": n, "complete": c} for d in samples() for n, c in [check(d, ref)]]
    with open(os.path.join(HERE, "tool_call_grammar_samples.json"), "w") as f:  # one sample per line
        f.write('{"_comment": "answers of the GBNF engine armed with the reference\'s tool_call.gbnf; regenerate with tests/golden/make_grammar_golden.py",\n'
                ' "samples": [\n' + ",\n".join(json.dumps(s, ensure_ascii=False) for s in out) + "\n]}\n")
    print("wrote %d samples, %d complete" % (len(out), sum(s["complete"] for s in out)))
