"""The big-integer statement of typlonk_srs_check and typlonk_srs_contribute (include/typlonk.h).

An SRS is a list of affine G1 points (None = the identity).  With the secret s KNOWN, g1[i+1] = [s] g1[i] needs no pairing:
the prefix test e(A_k, [s]G2) * e(-B_k, G2) = 1 of the library is, on the G1 side,
    sum_{i<k} rho^i ([s] g1[i] - g1[i+1]) = O,
which is what `prefix_holds` computes with the oracle's g1_mul.  `check` is the whole call on top of it: membership, point 0,
the whole-SRS fold and the bisection, with the folds counted as the library counts them."""
from __future__ import annotations

import hashlib
import struct

from oracle import bls12_381 as O

R = O.R
TAG = b"typlonk/srs/check/v1"
VALID, BAD_POINT, BAD_P0, BAD_RATIO = 0, 1, 2, 3
NOT_ON_CURVE, NOT_IN_SUBGROUP = 3, 4   # TYPLONK_POINT_*


def g2s_limbs(g2s):
    """[s]G2 as the C ABI's 24 limbs: x.c0 x.c1 y.c0 y.c1, six Montgomery limbs each"""
    (x0, x1), (y0, y1) = g2s
    return [limb for c in (x0, x1, y0, y1) for limb in O.fq_to_mont_limbs(c)]


def rho(seed: bytes, length: int, g2s) -> int:
    """Blake2b-512(tag || seed || u64 len || the 24 limbs of [s]G2), little-endian, mod r"""
    assert len(seed) == 32
    data = TAG + bytes(seed) + struct.pack("<Q", length) + b"".join(struct.pack("<Q", x) for x in g2s_limbs(g2s))
    return int.from_bytes(hashlib.blake2b(data, digest_size=64).digest(), "little") % R


def first_bad(points, s: int):
    """the lowest i with g1[i+1] != [s] g1[i], or None"""
    for i in range(len(points) - 1):
        if O.g1_mul(points[i], s) != points[i + 1]:
            return i
    return None


def prefix_holds(points, s: int, r: int, k: int) -> bool:
    """sum_{i<k} r^i ([s] g1[i] - g1[i+1]) = O"""
    acc, w = None, 1
    for i in range(k):
        d = O.g1_add(O.g1_mul(points[i], s), O.g1_neg(points[i + 1]))
        acc = O.g1_add(acc, O.g1_mul(d, w))
        w = w * r % R
    return acc is None


def membership(p):
    """0, or the class of a point that is not an element of the group"""
    if p is None:
        return 0
    if not (0 <= p[0] < O.P and 0 <= p[1] < O.P) or not O.g1_is_on_curve(p):
        return NOT_ON_CURVE
    # [r] P = [r - 1] P + P  (the oracle's g1_mul reduces its scalar mod r)
    return 0 if O.g1_add(O.g1_mul(p, R - 1), p) is None else NOT_IN_SUBGROUP


def check(points, s: int, seed: bytes, g2s) -> dict:
    """the report of typlonk_srs_check for an SRS whose [s]G2 is g2s = [s] G2"""
    rep = {"verdict": VALID, "point_class": 0, "index": 0, "bad_points": 0, "folds": 0}
    classes = [membership(p) for p in points]
    bad = [i for i, c in enumerate(classes) if c]
    if bad:
        return dict(rep, verdict=BAD_POINT, point_class=classes[bad[0]], index=bad[0], bad_points=len(bad))
    if points[0] != O.G1:
        return dict(rep, verdict=BAD_P0)
    n = len(points)
    if n == 1:
        return rep
    r = rho(seed, n, g2s)
    rep["folds"] = 1
    if prefix_holds(points, s, r, n - 1):
        return rep
    lo, hi = 0, n - 1
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        rep["folds"] += 1
        if prefix_holds(points, s, r, mid):
            lo = mid
        else:
            hi = mid
    return dict(rep, verdict=BAD_RATIO, index=hi - 1)


def contribute(points, t: int):
    """[t^i] g1[i]"""
    return [O.g1_mul(p, pow(t, i, R)) for i, p in enumerate(points)]


def cancelling_pair(s: int, r: int, j: int, k: int, a: int) -> int:
    """b such that g1[j] += [a] G and g1[k] += [b] G leave every prefix past max(j, k) + 1 of the test with weight r intact,
    1 <= j < k: the defects are (r s - 1) (a r^(j-1) + b r^(k-1)) G, so b = -a r^(j-k)"""
    assert 1 <= j < k
    return -a * pow(r, j - k, R) % R
