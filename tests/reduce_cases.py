"""Bucket arrays for the MSM's reduction kernels (msm_reduce.hip) and what they must reduce to, for
tests/test_gpu_reduce.py (device, through tests/cpp/libdevice_reduce.so) and tests/test_reduce_cases.py (the reference
itself, on the CPU).

Every bucket is B_k = e_k G for a small signed integer e_k, taken from a pool of a few dozen points made with Python
integers: each point under several Z scalings (lifted toward the XYZZ invariants), its negative, and the identity in both
encodings.  A bucket array is an index array into the pool, so 2^19 buckets cost one numpy gather, and every sum of
buckets is known as an integer: a bit plane is (sum of e_k over the rows / columns whose weight has the bit) G, a set
sum is (sum of ((k >> v) + 1) e_k) G -- one short scalar multiplication each."""
from __future__ import annotations

import random

import numpy as np

import arith_cases as C
from oracle import bls12_381 as O

RC_NB = 16                      # planes per (set, kind) in the kernels' output (launch.hpp)
N_POINTS, N_Z = 24, 3           # pool: points e G and -e G, each under N_Z scalings (one of them Z = 1)


# ---- the shape and the weights, restated from launch.hpp's description ---------------------------------------------------
def shape_of(c: int, nsets: int = 1, top_v: int = 0) -> dict:
    """the grid of a c-bit window's 2^(c-1) buckets as msm_host.hip derives it"""
    c1 = c - 1
    cl = (c1 + 1) // 2
    ch = c1 - cl
    return {"nsets": nsets, "c1": c1, "ch": ch, "cl": cl, "lhc": min(3, ch), "llc": min(3, cl), "top_v": top_v}


def shape_words(sh: dict) -> np.ndarray:
    return np.array([sh[k] for k in ("nsets", "c1", "ch", "cl", "lhc", "llc", "top_v")], dtype=np.uint32)


def set_v(sh: dict, s: int) -> int:
    """virtual-copy bits of a set: top_v for the last one"""
    return sh["top_v"] if s + 1 == sh["nsets"] else 0


def plane_counts(sh: dict, s: int) -> tuple[int, int, int]:
    """(row planes, column planes, the rows' common shift)"""
    v, cl, ch = set_v(sh, s), sh["cl"], sh["ch"]
    if v <= cl:
        return ch, cl - v + 1, cl - v
    return max(ch - (v - cl), 0) + 1, 0, 0


def row_weights(sh: dict, s: int) -> np.ndarray:
    v, cl = set_v(sh, s), sh["cl"]
    hi = np.arange(1 << sh["ch"], dtype=np.int64)
    return hi if v <= cl else (hi >> (v - cl)) + 1


def col_weights(sh: dict, s: int) -> np.ndarray:
    v, cl = set_v(sh, s), sh["cl"]
    lo = np.arange(1 << cl, dtype=np.int64)
    return (lo >> v) + 1 if v <= cl else np.zeros_like(lo)


# ---- the pool ----------------------------------------------------------------------------------------------------------------
def _pack48(coords) -> list[int]:
    """XYZZ integers (< 2^384) -> the 4 x 12 words of the HBM form"""
    return [w for v in coords for w in C.limbs(v, 12, 32)]


class Pool:
    """words[i]: 48 packed words of pool entry i; e[i]: its scalar; of[(j, sign)]: the entries holding sign * e_j G"""

    def __init__(self, seed: int = 0x5EED0C):
        rnd = random.Random(seed)
        es = sorted(rnd.sample(range(1, 1 << 16), N_POINTS - 3)) + [1, 2, 3]
        words, e, self.of = [], [], {}
        for j, ej in enumerate(es):
            q = O.g1_mul(O.G1, ej)
            for sign, pt in ((1, q), (-1, O.g1_neg(q))):
                ids = []
                for k in range(N_Z):
                    ids.append(len(e))
                    words.append(_pack48(C.xyzz_of(pt, rnd, top=k == 1, z=1 if k == 0 else None)))
                    e.append(sign * ej)
                self.of[(j, sign)] = np.array(ids)
        self.identity = np.array([len(e), len(e) + 1])
        for top in (False, True):
            words.append(_pack48(C.xyzz_of(None, rnd, top)))
            e.append(0)
        self.words = np.array(words, dtype=np.uint32)
        self.e = np.array(e, dtype=np.int64)
        self.points = len(es)

    def buckets(self, idx: np.ndarray) -> np.ndarray:
        return np.ascontiguousarray(self.words[idx])


_POOL: list[Pool] = []


def pool() -> Pool:
    if not _POOL:
        _POOL.append(Pool())
    return _POOL[0]


# ---- bucket fills ------------------------------------------------------------------------------------------------------------
FILLS = ("random", "same_point", "one_first", "one_last", "one_middle", "alternating", "adjacent", "identity")


def fill(sh: dict, name: str, seed: int = 0) -> np.ndarray:
    """pool indices of the nsets << c1 buckets"""
    pl = pool()
    rng = np.random.default_rng([seed, sh["c1"], sh["nsets"], sh["top_v"], FILLS.index(name)])
    bsz, nb = 1 << sh["c1"], sh["nsets"] << sh["c1"]
    pick = lambda j, sign, n: pl.of[(j, sign)][rng.integers(0, N_Z, n)]   # noqa: E731 -- one point, a random Z per bucket
    if name == "random":
        return rng.integers(0, len(pl.e), nb)
    if name == "same_point":
        return pick(5, 1, nb)
    if name == "identity":
        return pl.identity[rng.integers(0, 2, nb)]
    if name.startswith("one_"):
        # one non-empty bucket per set pins w(k) exactly; the middle index has bits in the row AND the column part
        idx = pl.identity[rng.integers(0, 2, nb)]
        k = {"one_first": 0, "one_last": bsz - 1, "one_middle": (bsz * 5) // 8 + (1 << sh["cl"]) // 2 + 1}[name]
        for s in range(sh["nsets"]):
            idx[s * bsz + k] = pick(7 + s, 1, 1)[0]
        return idx
    if name == "alternating":
        idx = pick(3, 1, nb)
        idx[1::2] = pick(3, -1, nb // 2)
        return idx
    if name == "adjacent":
        # buckets 2k and 2k + 1 the same point under different Z for a quarter of the k
        idx = rng.integers(0, len(pl.e), nb)
        ks = np.nonzero(rng.integers(0, 4, nb // 2) == 0)[0]
        j = rng.integers(0, pl.points, len(ks))
        z0 = rng.integers(0, N_Z, len(ks))
        z1 = (z0 + rng.integers(1, N_Z, len(ks))) % N_Z
        ids = np.stack([pl.of[(p, 1)] for p in range(pl.points)])   # [point][scaling]
        idx[2 * ks], idx[2 * ks + 1] = ids[j, z0], ids[j, z1]
        return idx
    raise KeyError(name)


# ---- the reference ---------------------------------------------------------------------------------------------------------
def ref_planes(sh: dict, idx: np.ndarray) -> dict:
    """{(set, kind, bit): integer scalar of the plane}: kind 0 the rows whose weight has the bit (without the common
    shift), kind 1 the columns"""
    e = pool().e[idx]
    out = {}
    for s in range(sh["nsets"]):
        grid = e[s << sh["c1"]:(s + 1) << sh["c1"]].reshape(1 << sh["ch"], 1 << sh["cl"])
        nbr, nbc, _ = plane_counts(sh, s)
        for kind, sums, w, nbits in ((0, grid.sum(axis=1), row_weights(sh, s), nbr), (1, grid.sum(axis=0), col_weights(sh, s), nbc)):
            for b in range(nbits):
                out[(s, kind, b)] = int(sums[(w >> b) & 1 == 1].sum())
    return out


def ref_set_sums(sh: dict, idx: np.ndarray) -> list[int]:
    """per set sum_k ((k >> v) + 1) e_k, straight from the bucket weights (no rows, no columns)"""
    e = pool().e[idx]
    k = np.arange(1 << sh["c1"], dtype=np.int64)
    return [int((((k >> set_v(sh, s)) + 1) * e[s << sh["c1"]:(s + 1) << sh["c1"]]).sum()) for s in range(sh["nsets"])]


def recombine(sh: dict, planes: dict) -> list[int]:
    """what the planes stand for: per set sum_b 2^(b + shift) row_b + sum_b 2^b col_b"""
    out = []
    for s in range(sh["nsets"]):
        nbr, nbc, shift = plane_counts(sh, s)
        out.append(sum(planes[(s, 0, b)] << (b + shift) for b in range(nbr)) + sum(planes[(s, 1, b)] << b for b in range(nbc)))
    return out


_MUL_CACHE: dict = {}


def point_of(scalar: int):
    """scalar * G for a signed integer"""
    if scalar not in _MUL_CACHE:
        q = O.g1_mul(O.G1, abs(scalar) % O.R)
        _MUL_CACHE[scalar] = O.g1_neg(q) if scalar < 0 and q is not None else q
    return _MUL_CACHE[scalar]


def unpack48(words) -> tuple:
    return tuple(C.val(words[12 * j:12 * j + 12], 32) for j in range(4))
