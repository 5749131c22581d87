"""Generates tests/golden/patch_preimages.json from a checkout of the reference (fabrizio-m/TyPLONK).

For every file that integration/rust/patches/*.patch touches it records the file's git blob id and line count, and for
every hunk the SHA-256 of the reference's lines that the hunk's context and removed lines must match.  Hashes only: no
line of the reference is stored.  tests/test_host.py checks the patches against this record, so the suite does not need
the reference tree itself.

    python tests/golden/gen_patch_preimages.py <reference-tree>      # rewrites the fixture
"""
import glob
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import patch_preimages  # noqa: E402


def lines_sha256(lines) -> str:
    return hashlib.sha256("".join(l + "\n" for l in lines).encode("utf-8")).hexdigest()


def main(ref: str) -> None:
    out = {}
    for patch in sorted(glob.glob(os.path.join(ROOT, "integration", "rust", "patches", "*.patch"))):
        rec = {}
        for path, d in patch_preimages(patch).items():
            with open(os.path.join(ref, path), "rb") as f:
                data = f.read()
            lines = data.decode("utf-8").split("\n")
            if lines[-1] == "":
                lines.pop()
            rec[path] = {"blob": hashlib.sha1(b"blob %d\0" % len(data) + data).hexdigest(), "lines": len(lines),
                         "hunks": [{"start": s, "length": n, "sha256": lines_sha256(lines[s - 1:s - 1 + n])} for s, n, _ in d["hunks"]]}
        out[os.path.basename(patch)] = rec
    with open(os.path.join(HERE, "patch_preimages.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
