#!/usr/bin/env python3
"""Compare two AMDGPU assembly files kernel by kernel: tools/compare_kernel_asm.py OLD.s NEW.s

The files come from the same source at two commits, compiled with the kernel flags of trackiellm_amd/csrc/Makefile plus
`--cuda-device-only -S`.  A kernel is the same when its instruction stream (comments, directives and blank lines stripped, the
function number taken out of local labels) and its kernel descriptor (the .amdhsa_ lines: registers, scratch, LDS) are the same.
Prints the names of the kernels that differ or exist on one side only, nothing else; exit status 1 if there are any."""
import re
import sys

LOCAL_LABEL = re.compile(r"\.L(BB|JTI|func_begin|func_end)\d+")


def kernels(path):
    """{name: (instruction lines, descriptor lines)}"""
    out, name, body, desc, in_desc = {}, None, [], {}, None
    for line in open(path):
        line = line.split(";")[0].strip()
        if not line:
            continue
        if line.startswith(".amdhsa_kernel "):
            in_desc = line.split()[1]
            desc[in_desc] = []
        elif line == ".end_amdhsa_kernel":
            in_desc = None
        elif in_desc:
            desc[in_desc].append(line)
        elif name is None:
            m = re.fullmatch(r"([A-Za-z_][\w$.]*):", line)
            if m and not line.startswith(".L"):
                name, body = m.group(1), []
        elif line.startswith(".Lfunc_end"):
            out[name], name = body, None
        elif not line.startswith(".") or line.endswith(":"):  # an instruction or a local label, not a directive
            body.append(LOCAL_LABEL.sub(r".L\1", line))
    return {k: (out.get(k), desc[k]) for k in desc}


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    differ = sorted(k for k in old.keys() | new.keys() if old.get(k) != new.get(k))
    for k in differ:
        print(k)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
