"""Writes tests/golden/edge_reference_answers.npz: what the COMPILED reference (oracle/_ref: its pre-processor and attribute classifiers built from their
own sources) answers on a subset of the cases of tests/edge_cases.py, with the sha256 of every input, so that the tests need no reference tree:
  - BOX_ATTRIBUTES: every box of every case whose rectangle lies inside the frame (the reference's door-state loop does not bounds-check, its colour loop
    does: boxes reaching outside are recorded for the colour alone) — the threshold colours, the ties and thin boxes, the density-threshold boxes;
  - PREPROCESS at scale 1/255 for the tightly packed RGB8 frames (the reference function takes no pitch, alpha or NHWC): planar outputs.
Run from the repository root after __graft_entry__.build(): python tests/golden/make_edge_golden.py"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import edge_cases as EC  # noqa: E402
import oracle_lib as O  # noqa: E402

NAMES = ["red", "yellow", "green", "cyan", "blue", "magenta", "black", "white", "gray"]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    out = {}
    for i, c in enumerate(EC.group("box_attributes")):
        W, H = c["in_w"], c["in_h"]
        frame, rects = c["a"].reshape(H, W, 3), c["b"].reshape(-1, 4)
        ans = np.full((len(rects), 2), 255, np.uint8)                       # 255: not recorded
        for k, (x, y, w, h) in enumerate(rects):
            inside = x >= 0 and y >= 0 and w > 0 and h > 0 and x + w <= W and y + h <= H
            if not inside and (w <= 0 or h <= 0 or abs(x) > 4 * W or abs(y) > 4 * H or w > 4 * W or h > 4 * H):
                continue
            # a box reaching outside: only a box one row tall is safe to hand to the reference (its door-state loop then runs no iteration); colour alone
            colour, door = O.ref_attributes(frame, (x, y, w, h)) if inside else (O.ref_attributes(frame, (x, y, w, h))[0] if h == 1 else None, None)
            if colour is not None:
                ans[k, 0] = NAMES.index(colour)
            if door is not None:
                ans[k, 1] = 1 if door == "closed" else 0
        out["box%d_sha" % i] = np.frombuffer(bytes.fromhex(sha(c["a"]) + sha(c["b"])), np.uint8)
        out["box%d" % i] = ans
    for i, c in enumerate(EC.group("preprocess")):
        if c["bpp"] != 3 or c["in_stride"] != 3 * c["in_w"] or not c["name"].endswith("scale 1/255"):
            continue
        frame = np.zeros((c["in_h"], c["in_w"], 3), np.uint8)
        frame.reshape(-1)[:len(c["a"])] = c["a"]
        y = O.ref_preprocess(frame, c["out_w"], c["out_h"], np.asarray(c["mean"], np.float32), np.asarray(c["std_dev"], np.float32))
        out["pre%d_sha" % i] = np.frombuffer(bytes.fromhex(sha(c["a"])), np.uint8)
        out["pre%d" % i] = y
    np.savez_compressed(os.path.join(HERE, "edge_reference_answers.npz"), **out)
    print("wrote edge_reference_answers.npz:", {k: v.shape for k, v in out.items() if not k.endswith("_sha")})


if __name__ == "__main__":
    main()
