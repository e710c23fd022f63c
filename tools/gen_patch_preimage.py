#!/usr/bin/env python3
"""Writes tests/golden/reference_patch_preimage.json from an UNTOUCHED checkout of the reference: for every file
rust/reference-patch/sigma0-polymath-hip.patch touches, its line count and, per hunk, the sha256 of the reference's lines in
the range the hunk header names (or "absent" for a file the patch creates).  tests/test_abi.py holds the patch's own
pre-image against these hashes, so the check needs no reference checkout.

Run: python tools/gen_patch_preimage.py <reference checkout>      (after any change to the patch's context or removed lines)
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from helpers import patch_preimages  # noqa: E402

PATCH = os.path.join("rust", "reference-patch", "sigma0-polymath-hip.patch")
OUT = os.path.join(ROOT, "tests", "golden", "reference_patch_preimage.json")


def sha(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def main(ref):
    files = {}
    for path, hunks in patch_preimages(open(os.path.join(ROOT, PATCH)).read()).items():
        src = os.path.join(ref, path)
        if not os.path.exists(src):
            files[path] = {"absent": True}
            continue
        lines = open(src).read().split("\n")
        if lines and lines[-1] == "":
            lines.pop()
        files[path] = {"lines": len(lines),
                       "hunks": [{"start": s, "count": c, "sha256": sha(lines[s - 1:s - 1 + c])} for s, c, _ in hunks]}
    with open(OUT, "w") as f:
        json.dump({"patch": PATCH.replace(os.sep, "/"), "files": files}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
