#!/usr/bin/env python3
"""Writes tests/golden/surface_text.json: what the REFERENCE's ``misc.decode_sequence`` (REMOVE_BAD_ENDINGS 0 and 1, limit 0 and 3) and
``eval_utils.count_bad`` return for a handful of crafted id rows over a toy vocabulary -- the strings and flags that
``boficap_amd.surface.trim_host`` (and through it the kernel) must reproduce (tests/test_surface.py).

    python dev/make_surface_golden.py --reference <root of the reference checkout>

The two reference modules are loaded from ``<root>/captioning/utils`` by path, under a package name of their own (this repository has a
``captioning`` package too); nothing of them is copied.  The fixture holds data only: the rows, the vocabulary, the returned strings and flags.
"""
import argparse
import importlib
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VOCAB = {1: "a", 2: "the", 3: "on", 4: "man", 5: "dog", 6: "with", 7: "table", 8: "sitting", 9: "is", 10: "his", 11: "near", 12: "that", 13: "of", 14: "before"}
ROWS = [
    ([0, 0, 0, 0, 0, 0, 0, 0], "empty"),
    ([1, 0, 0, 0, 0, 0, 0, 0], "all bad, length 1"),
    ([1, 2, 1, 0, 0, 0, 0, 0], "all bad, length 3"),
    ([6, 10, 13, 12, 0, 0, 0, 0], "all bad, length 4, also above limit 3"),
    ([4, 1, 0, 0, 0, 0, 0, 0], "one trailing bad word"),
    ([4, 3, 1, 0, 0, 0, 0, 0], "two trailing bad words"),
    ([4, 1, 2, 6, 3, 1, 2, 0], "six trailing bad words"),
    ([4, 6, 10, 13, 0, 0, 0, 0], "three trailing bad words above limit 3"),
    ([4, 1, 5, 0, 0, 0, 0, 0], "a bad word in the middle only"),
    ([5, 6, 7, 13, 4, 0, 0, 0], "bad words in the middle only, above limit 3"),
    ([4, 8, 3, 2, 7, 6, 1, 5], "a full row without terminator that ends in a good word"),
    ([4, 8, 11, 7, 5, 6, 10, 13], "a full row without terminator that ends in bad words"),
    ([6, 10, 13, 12, 6, 10, 13, 12], "a full row of bad words"),
    ([0, 4, 5, 1, 0, 0, 0, 0], "a terminator at position 0"),
    ([4, 5, 0, 7, 1, 0, 0, 0], "a terminator in the middle, words after it"),
    ([5, 8, 6, 2, 4, 13, 0, 0], "an id <= 3 in the middle: limit 3 ends the caption on a bad word"),
    ([4, 9, 0, 0, 0, 0, 0, 0], "ends in a counted word that is not trimmed"),
    ([5, 11, 0, 0, 0, 0, 0, 0], "ends in another counted word that is not trimmed"),
    ([4, 10, 0, 0, 0, 0, 0, 0], "ends in a trimmed word that is not counted"),
    ([4, 14, 12, 0, 0, 0, 0, 0], "the trim uncovers a counted word"),
    ([4, 9, 12, 10, 0, 0, 0, 0], "the trim uncovers a counted word behind two"),
    ([4, 5, 7, 8, 0, 0, 0, 0], "no bad word at all"),
]


def load_reference(root):
    utils_dir = os.path.join(root, "captioning", "utils")
    pkg = types.ModuleType("reference_utils")
    pkg.__path__ = [utils_dir]
    sys.modules["reference_utils"] = pkg
    return importlib.import_module("reference_utils.misc"), importlib.import_module("reference_utils.eval_utils")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (holds captioning/utils/misc.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "surface_text.json"))
    args = ap.parse_args()
    misc, eval_utils = load_reference(args.reference)
    vocab = {str(k): w for k, w in VOCAB.items()}
    seq = torch.tensor([r for r, _ in ROWS], dtype=torch.long)
    cases = []
    for remove in (0, 1):
        for limit in (0, 3):
            os.environ["REMOVE_BAD_ENDINGS"] = str(remove)       # (how the reference's eval_split hands the option over, eval_utils.py:140)
            captions = misc.decode_sequence(vocab, seq, limit=limit)
            cases.append({"remove_bad_endings": remove, "limit": limit, "captions": captions, "bad": [int(eval_utils.count_bad(c)) for c in captions]})
    del os.environ["REMOVE_BAD_ENDINGS"]
    fixture = {"made_by": "dev/make_surface_golden.py: misc.decode_sequence and eval_utils.count_bad of the reference, both loaded and called, nothing restated",
               "vocab": vocab, "rows": [r for r, _ in ROWS], "what": [w for _, w in ROWS], "cases": cases}
    with open(args.out, "w") as f:
        json.dump(fixture, f, indent=1)
        f.write("\n")
    print(f"{args.out}: {len(ROWS)} rows x {len(cases)} cases")


if __name__ == "__main__":
    main()
