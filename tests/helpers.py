"""Shared helpers for the tests: limb packing between Python ints and the C-ABI's arkworks form."""
from __future__ import annotations
import ctypes
import os
import re
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import bls12_381 as O  # noqa: E402


def fr_pack(vals) -> np.ndarray:
    """list of canonical ints -> (n,4) uint64 Montgomery limbs"""
    out = np.empty((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        out[i] = O.fr_to_mont_limbs(v)
    return out


def fr_unpack(arr) -> list[int]:
    arr = np.asarray(arr, dtype=np.uint64).reshape(-1, 4)
    return [O.fr_from_mont_limbs([int(x) for x in row]) for row in arr]


def g1_pack(points):
    """list of affine points (or None) -> ((n,12) uint64, (n,) uint8)"""
    xy = np.empty((len(points), 12), dtype=np.uint64)
    inf = np.zeros(len(points), dtype=np.uint8)
    for i, p in enumerate(points):
        limbs, f = O.g1_to_limbs(p)
        xy[i] = limbs
        inf[i] = f
    return xy, inf


def g1_unpack_one(xy, inf):
    return O.g1_from_limbs([int(x) for x in np.asarray(xy, dtype=np.uint64).reshape(12)], int(inf))


def u32p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def load_golden(name):
    import json
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


def hex_pt(p):
    return None if p is None else (int(p[0], 16), int(p[1], 16))


def patch_preimages(path):
    """a `git diff` patch -> {file: {"blob": abbreviated pre-image blob id, "hunks": [(start, length, lines)]}}: what each
    hunk expects to find in the file it patches (its context and removed lines, in order, from line `start` on)"""
    files, cur, old_rem, new_rem = {}, None, 0, 0
    with open(path, encoding="utf-8") as f:
        text = f.read()
    for line in text.split("\n")[:-1]:
        if old_rem or new_rem:                       # inside a hunk body
            tag, body = (line[:1] or " "), line[1:]
            if tag == "\\":                          # "\ No newline at end of file"
                continue
            if tag in " -":
                cur["hunks"][-1][2].append(body)
                old_rem -= 1
            if tag in " +":
                new_rem -= 1
            continue
        if line.startswith("diff --git "):
            cur = files.setdefault(line.split(" b/", 1)[1], {"blob": None, "hunks": []})
        elif line.startswith("index "):
            cur["blob"] = line.split()[1].split("..")[0]
        elif line.startswith("@@ "):
            m = re.match(r"@@ -(\d+)(?:,(\d+))? \+(\d+)(?:,(\d+))? @@", line)
            old_rem, new_rem = int(m.group(2) or 1), int(m.group(4) or 1)
            cur["hunks"].append((int(m.group(1)), old_rem, []))
    return files
