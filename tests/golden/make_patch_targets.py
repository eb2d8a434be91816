"""Writes tests/golden/patch_targets.json: for every hunk of integration/rust/gpu-backend.patch, the sha256 of the lines
of the REFERENCE crate the hunk replaces (its checkout is given on the command line), and the length of each file.
tests/test_rust_shim_cpu.py hashes the hunk's own context + removed lines against it, so "the patch applies to the
reference" is checked without the reference's source.

    python tests/golden/make_patch_targets.py <checkout of ajalab/fm-index>
"""
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(ref):
    out, name = {}, None
    for ln in open(os.path.join(ROOT, "integration", "rust", "gpu-backend.patch")).read().splitlines():
        if ln.startswith("--- a/"):
            name = ln[6:].strip()
            src = open(os.path.join(ref, name)).read().splitlines()
            out[name] = {"lines": len(src), "hunks": []}
        m = re.match(r"@@ -(\d+),(\d+) \+\d+,\d+ @@", ln)
        if m and name:
            start, length = int(m.group(1)), int(m.group(2))
            old = "\n".join(src[start - 1:start - 1 + length])
            out[name]["hunks"].append({"start": start, "len": length, "sha256": hashlib.sha256(old.encode()).hexdigest()})
    with open(os.path.join(ROOT, "tests", "golden", "patch_targets.json"), "w") as f:
        json.dump({"_comment": "made by tests/golden/make_patch_targets.py from the reference crate", "files": out}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
