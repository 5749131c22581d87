"""Python statement of the wire format (include/typlonk.h): compressed G1 / G2 points in the ZCash / IETF BLS12-381 form and
the byte layouts of a compact proof and of a verifying key, over oracle/bls12_381.py and oracle/pairing.py.  Independent of the
native code.  Points are affine integer pairs (None = identity), scalars canonical integers; the proof and key dicts are those
of tests/compact_ref.py."""
from __future__ import annotations

import struct

from oracle import bls12_381 as O
from oracle import pairing as PR

P, R = O.P, O.R
HALF = (P - 1) // 2
OK, ENCODING, X_RANGE, NOT_ON_CURVE, NOT_IN_SUBGROUP, SCALAR_RANGE = 0, 1, 2, 3, 4, 5
G1_BYTES, G2_BYTES, PROOF_BYTES, VK_BYTES = 48, 96, 656, 628
COFACTOR = 0x396C8C005555E1568C00AAAB0000AAAB   # #E(Fq) = COFACTOR * R


def g1_mul_plain(pt, k: int):
    """[k] pt by double-and-add with NO reduction of k (O.g1_mul reduces mod r, which would make [r] P trivially O)"""
    acc = None
    for bit in bin(k)[2:]:
        acc = O.g1_add(acc, acc)
        if bit == "1":
            acc = O.g1_add(acc, pt)
    return acc


def g1_in_subgroup(pt) -> bool:
    return g1_mul_plain(pt, R) is None


def g2_mul_plain(q, k: int):
    acc = None
    for bit in bin(k)[2:]:
        acc = PR.g2_add(acc, acc)
        if bit == "1":
            acc = PR.g2_add(acc, q)
    return acc


def fq_sqrt(a: int):
    """a square root of a, or None (p = 3 mod 4)"""
    y = pow(a, (P + 1) // 4, P)
    return y if y * y % P == a % P else None


def g1_compress(pt) -> bytes:
    if pt is None:
        return bytes([0xC0]) + bytes(47)
    x, y = pt
    out = bytearray(x.to_bytes(48, "big"))
    out[0] |= 0x80 | (0x20 if y > HALF else 0)
    return bytes(out)


def g1_decompress(b: bytes, skip_subgroup: bool = False):
    """(status, point): the first failing check decides; a rejected encoding gives the identity"""
    assert len(b) == 48
    flags, x = b[0] >> 5, int.from_bytes(b, "big") & ((1 << 381) - 1)
    if not flags & 4:
        return ENCODING, None
    if flags & 2:
        return (ENCODING if (flags & 1) or x else OK), None
    if x >= P:
        return X_RANGE, None
    y = fq_sqrt((x * x * x + 4) % P)
    if y is None:
        return NOT_ON_CURVE, None
    if (y > HALF) != bool(flags & 1):
        y = P - y
    if not skip_subgroup and not g1_in_subgroup((x, y)):
        return NOT_IN_SUBGROUP, None
    return OK, (x, y)


# ---- Fq2 / G2 ----
def f2_sqrt(a):
    """a square root of a = (a0, a1) in Fq[u] / (u^2 + 1), or None: by exhaustion of the two candidates the norm gives"""
    a0, a1 = a[0] % P, a[1] % P
    if a1 == 0:
        s = fq_sqrt(a0)
        if s is not None:
            return (s, 0)
        s = fq_sqrt(-a0 % P)
        return None if s is None else (0, s)
    s = fq_sqrt((a0 * a0 + a1 * a1) % P)
    if s is None:
        return None
    inv2 = pow(2, -1, P)
    for t in ((a0 + s) * inv2 % P, (a0 - s) * inv2 % P):
        x0 = fq_sqrt(t)
        if x0:
            x1 = a1 * pow(2 * x0, -1, P) % P
            if PR.f2_mul((x0, x1), (x0, x1)) == (a0, a1):
                return (x0, x1)
    return None


def g2_y_is_high(y) -> bool:
    return y[1] > HALF if y[1] else y[0] > HALF


def g2_compress(q) -> bytes:
    (x0, x1), y = q
    out = bytearray(x1.to_bytes(48, "big") + x0.to_bytes(48, "big"))
    out[0] |= 0x80 | (0x20 if g2_y_is_high(y) else 0)
    return bytes(out)


def g2_decompress(b: bytes, skip_subgroup: bool = False):
    """(status, point); an infinite point is refused (a key's [s]G2 is finite)"""
    assert len(b) == 96
    flags = b[0] >> 5
    if not flags & 4 or flags & 2:
        return ENCODING, None
    x1 = int.from_bytes(b[:48], "big") & ((1 << 381) - 1)
    x0 = int.from_bytes(b[48:], "big")
    if x0 >= P or x1 >= P:
        return X_RANGE, None
    x = (x0, x1)
    y = f2_sqrt(PR.f2_add(PR.f2_mul(PR.f2_mul(x, x), x), PR.B2))
    if y is None:
        return NOT_ON_CURVE, None
    if g2_y_is_high(y) != bool(flags & 1):
        y = PR.f2_neg(y)
    if not skip_subgroup and g2_mul_plain((x, y), R) is not None:
        return NOT_IN_SUBGROUP, None
    return OK, (x, y)


# ---- the two layouts ----
def fr_bytes(x: int) -> bytes:
    assert 0 <= x < R
    return x.to_bytes(32, "little")


def proof_points(pf):
    return list(pf["commit"]) + [pf["z_commit"]] + list(pf["t_commit"]) + list(pf["witness"])


def proof_to_bytes(pf) -> bytes:
    out = b"".join(g1_compress(p) for p in proof_points(pf)) + b"".join(fr_bytes(e) for e in pf["evals"])
    assert len(out) == PROOF_BYTES
    return out


def proof_from_bytes(b: bytes, skip_subgroup: bool = False):
    """(status, proof): status 0, or class | field << 8 of the first bad field in wire order"""
    assert len(b) == PROOF_BYTES
    status, pts, evals = 0, [], []
    for i in range(9):
        st, p = g1_decompress(b[48 * i:48 * i + 48], skip_subgroup)
        if st and not status:
            status = st | i << 8
        pts.append(p)
    for i in range(7):
        e = int.from_bytes(b[432 + 32 * i:464 + 32 * i], "little")
        if e >= R and not status:
            status = SCALAR_RANGE | (9 + i) << 8
        evals.append(e)
    if status:
        return status, None
    return 0, {"commit": pts[:3], "z_commit": pts[3], "t_commit": pts[4:7], "witness": pts[7:], "evals": evals}


def vk_to_bytes(vk) -> bytes:
    out = (struct.pack("<I", vk["log_n"]) + b"".join(fr_bytes(k) for k in vk["cosets"]) +
           b"".join(g1_compress(c) for c in vk["commitments"]) + g1_compress(vk["srs0"]) + g2_compress(vk["g2s"]))
    assert len(out) == VK_BYTES
    return out


def vk_from_bytes(b: bytes, skip_subgroup: bool = False):
    """(status, vk); fields: 0..2 the cosets, 3..11 the G1 points, 12 [s]G2.  log_n is not judged here."""
    assert len(b) == VK_BYTES
    status = 0
    cosets = [int.from_bytes(b[4 + 32 * i:36 + 32 * i], "little") for i in range(3)]
    for i, k in enumerate(cosets):
        if k >= R and not status:
            status = SCALAR_RANGE | i << 8
    pts = []
    for i in range(9):
        st, p = g1_decompress(b[100 + 48 * i:148 + 48 * i], skip_subgroup)
        if st and not status:
            status = st | (3 + i) << 8
        pts.append(p)
    st, g2s = g2_decompress(b[532:], skip_subgroup)
    if st and not status:
        status = st | 12 << 8
    if status:
        return status, None
    return 0, {"log_n": struct.unpack("<I", b[:4])[0], "cosets": cosets, "commitments": pts[:8], "srs0": pts[8], "g2s": g2s}


# ---- inputs for the tests ----
def curve_point_at(x: int):
    """the curve point (x, y) with the smaller y, or None"""
    y = fq_sqrt((x * x * x + 4) % P)
    return None if y is None else (x, min(y, P - y))


def cofactor_point(x: int):
    """[r] (x, y): a point whose order divides the cofactor (the identity only for points of G)"""
    p = curve_point_at(x)
    return None if p is None else g1_mul_plain(p, R)


def smallest_non_residue_x() -> int:
    x = 0
    while fq_sqrt((x * x * x + 4) % P) is not None:
        x += 1
    return x
