#!/usr/bin/python3
"""What tests/test_binding.py::test_patches_apply_to_the_reference needs to know about the reference tree, recorded as data so
that the test runs without it: patches/*.patch are applied in order to a scratch copy of the files they touch, and before each
patch every hunk's target region (the old-side lines at the hunk's line number) is hashed (SHA-256 of the lines joined by
newlines).  Also recorded: how often the unpatched files hold each string the test asserts about (test_binding.PATCHED).
No line of the reference is stored.

Run: python tests/golden/make_patch_golden.py HALO2_PSE_CHECKOUT   (writes tests/golden/patches_reference.json)
"""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
from test_binding import PATCHED, patch_hunks  # noqa: E402


def sha(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def main(ref):
    patches = sorted(f for f in os.listdir(os.path.join(ROOT, "patches")) if f.endswith(".patch"))
    hunks = {p: patch_hunks(os.path.join(ROOT, "patches", p)) for p in patches}
    touched = sorted({h[0] for p in patches for h in hunks[p]})
    counts = {}
    for rel, strings in sorted(PATCHED.items()):
        lines = open(os.path.join(ref, rel)).read().split("\n")
        counts[rel] = {s: sum(ln.count(s) for ln in lines) for s in strings}
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for rel in touched:
            os.makedirs(os.path.dirname(os.path.join(tmp, rel)), exist_ok=True)
            shutil.copy(os.path.join(ref, rel), os.path.join(tmp, rel))
        for p in patches:
            for rel, start, n, pre, _ in hunks[p]:
                lines = open(os.path.join(tmp, rel)).read().split("\n")
                region = lines[start - 1:start - 1 + n]
                out.append({"patch": p, "file": rel, "old_start": start, "old_lines": n, "sha256": sha(region)})
                if region != pre:
                    print("%s: hunk at %s:%d does not match the reference" % (p, rel, start), file=sys.stderr)
            subprocess.run(["patch", "-p1", "--fuzz=0", "-i", os.path.join(ROOT, "patches", p)], cwd=tmp, check=True, capture_output=True)
    with open(os.path.join(HERE, "patches_reference.json"), "w") as f:
        json.dump({"hunks": out, "counts": counts}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
