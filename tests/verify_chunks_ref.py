"""The big-integer statement of typlonk_verify_chunks (include/typlonk.h): KZG multi-proofs checked a batch of cells per call.

n = 2^log_n, l = 2^log_l, r = n / l, w = O.domain_root(log_n), a_k = w^(k l).  A cell is (c, k, E, pi): an index into the
commitments, a coset index, the l evaluations E[t] = f(w^(k + r t)) and a proof.  Everything here works on SCALARS, as
open_chunks_ref does: a point [a]G is stood for by a, and with the secret s KNOWN the pairing product of a fold

    e(sum rho_i pi_i, [s^l]G2) * e(-(sum_c w_c C_c + sum rho_i a_(k_i) pi_i - [A(s)]G), G2) = 1

is  s^l sum rho_i pi_i - (sum_c w_c C_c + sum rho_i a_(k_i) pi_i - A(s)) = 0  mod r  (`fold_holds`).  rho_i = rho^i, i the
cell's position in the call; w_c = sum_{c_i = c} rho_i; A = sum_i rho_i I_i, I_i the interpolant of E_i on coset k_i, taken through
O.ntt (an inverse transform on the coset w^k) so that l = 1024 stays quick.  All sums run over the live cells of [lo, hi).
`check` is the whole call on top of it: one fold, then the bisection over the live cells, the folds counted as the library counts
them."""
from __future__ import annotations

import hashlib
import struct

from oracle import bls12_381 as O

R = O.R
TAG = b"typlonk/chunks/verify/v1"
OK, BAD_EVAL, BAD_POINT, BAD_COMMITMENT, BAD_PROOF = 0, 1, 2, 3, 4   # TYPLONK_CELL_*


def g2_limbs(q):
    """a G2 point as the C ABI's 24 limbs: x.c0 x.c1 y.c0 y.c1, six Montgomery limbs each"""
    (x0, x1), (y0, y1) = q
    return [limb for c in (x0, x1, y0, y1) for limb in O.fq_to_mont_limbs(c)]


def rho(seed: bytes, log_n: int, log_l: int, N: int, M: int, g2sl) -> int:
    """Blake2b-512(tag || seed || u64 log_n || u64 log_l || u64 N || u64 M || the 24 limbs of [s^l]G2), little-endian, mod r"""
    assert len(seed) == 32
    data = TAG + bytes(seed) + struct.pack("<QQQQ", log_n, log_l, N, M) + b"".join(struct.pack("<Q", x) for x in g2_limbs(g2sl))
    return int.from_bytes(hashlib.blake2b(data, digest_size=64).digest(), "little") % R


def coset_constant(k: int, log_n: int, log_l: int) -> int:
    return pow(O.domain_root(log_n), k << log_l, R)


def interpolant(ys, k: int, log_n: int, log_l: int):
    """the l coefficients of I_k from ys[t] = f(w^(k + r t)): the inverse transform of size l on the coset w^k"""
    assert len(ys) == 1 << log_l
    return O.ntt(ys, log_l, inverse=True, coset=pow(O.domain_root(log_n), k, R))


def weights(N: int, rho_: int, lo: int, hi: int, live=None):
    """rho^i for the live cells of [lo, hi), zero elsewhere"""
    out, w = [], 1
    for i in range(N):
        out.append(w if lo <= i < hi and (live is None or live[i]) else 0)
        w = w * rho_ % R
    return out


def commitment_weights(cells, w, M: int):
    """w_c = the sum of the weights of the cells that name commitment c"""
    out = [0] * M
    for (c, _, _, _), wi in zip(cells, w):
        out[c] = (out[c] + wi) % R
    return out


def fold_coefficients(cells, w, log_n: int, log_l: int):
    """A = sum_i w_i I_i, l coefficients"""
    acc = [0] * (1 << log_l)
    for (_, k, ys, _), wi in zip(cells, w):
        if wi:
            acc = [(a + wi * c) % R for a, c in zip(acc, interpolant(ys, k, log_n, log_l))]
    return acc


def fold_holds(cells, commitments, s: int, rho_: int, log_n: int, log_l: int, lo: int = 0, hi: int | None = None, live=None) -> bool:
    """the folded equation in the exponent; commitments and the cells' proofs are scalars"""
    hi = len(cells) if hi is None else hi
    w = weights(len(cells), rho_, lo, hi, live)
    lhs = sum(wi * pi for (_, _, _, pi), wi in zip(cells, w)) % R
    rhs = sum(wc * cm for wc, cm in zip(commitment_weights(cells, w, len(commitments)), commitments))
    rhs += sum(wi * coset_constant(k, log_n, log_l) % R * pi for (_, k, _, pi), wi in zip(cells, w))
    rhs -= O.poly_eval(fold_coefficients(cells, w, log_n, log_l), s)
    return (lhs * pow(s, 1 << log_l, R) - rhs) % R == 0


def cell_holds(cell, commitments, s: int, log_n: int, log_l: int) -> bool:
    """one cell's own equation: C - I(s) + a_k pi = s^l pi"""
    c, k, ys, pi = cell
    i_s = O.poly_eval(interpolant(ys, k, log_n, log_l), s)
    return (commitments[c] - i_s + coset_constant(k, log_n, log_l) * pi - pow(s, 1 << log_l, R) * pi) % R == 0


def check(cells, commitments, s: int, rho_: int, log_n: int, log_l: int, dead=None):
    """(status per cell, folds): `dead` maps a cell's position to the status that keeps it from the fold"""
    N = len(cells)
    dead = dead or {}
    status = [dead.get(i, OK) for i in range(N)]
    live = [st == OK for st in status]
    folds = 0

    def decide(lo, hi):
        nonlocal folds
        n_live = sum(live[lo:hi])
        if not n_live:
            return
        folds += 1
        if fold_holds(cells, commitments, s, rho_, log_n, log_l, lo, hi, live):
            return
        if n_live == 1:
            status[next(i for i in range(lo, hi) if live[i])] = BAD_PROOF
            return
        seen, mid = 0, lo
        while mid < hi:
            if live[mid] and seen == n_live // 2:
                break
            seen += live[mid]
            mid += 1
        decide(lo, mid)
        decide(mid, hi)

    decide(0, N)
    return status, folds
