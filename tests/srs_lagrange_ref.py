"""The big-integer statement of typlonk_srs_g1_ntt (include/typlonk.h): the Lagrange form of an SRS and back.

An SRS is a list of affine G1 points (None = the identity).  Over the domain {w^i}, i < n = 2^log_n, w = O.domain_root(log_n):

    TO_LAGRANGE    out[i] = [1/n] sum_j [w^(-ij)] g1[j]
    FROM_LAGRANGE  out[j] =       sum_i [w^(ij)]  g1[i]

Three references, by what is known about the points:
  * g1[j] = [s^j] G with s KNOWN: out[i] = [L_i(s)] G with the closed form L_i(s) = (s^n - 1) w^i / (n (s - w^i)) -- 0/0 when s
    is an n-th root of unity, where the inverse transform of the powers of s stands in (`lagrange_scalars`);
  * g1[j] = [k_j] G for known k_j: out = [intt(k)_i] G (`scalars_to_lagrange`);
  * any points at all: the double sum itself by the oracle's group law (`g1_ntt`), n^2 scalar multiplications."""
from __future__ import annotations

from oracle import bls12_381 as O

R = O.R
TO_LAGRANGE, FROM_LAGRANGE = 0, 1


def scalars_to_lagrange(k, log_n: int):
    """the scalars of the Lagrange points of [k_j] G: the inverse transform of k"""
    assert len(k) == 1 << log_n
    return O.ntt([x % R for x in k], log_n, inverse=True)


def lagrange_scalars(s: int, log_n: int):
    """L_i(s), i < 2^log_n"""
    n = 1 << log_n
    s %= R
    zh = (pow(s, n, R) - 1) % R
    if zh == 0:                                   # s is in the domain: the closed form is 0/0
        return scalars_to_lagrange([pow(s, j, R) for j in range(n)], log_n)
    w, n_inv = O.domain_root(log_n), pow(n, -1, R)
    out, wi = [], 1
    for _ in range(n):
        out.append(zh * wi % R * n_inv % R * pow((s - wi) % R, -1, R) % R)
        wi = wi * w % R
    return out


def lagrange_points(s: int, log_n: int, only=None):
    """[L_i(s)] G for every i < 2^log_n, or for the indices in `only`"""
    ls = lagrange_scalars(s, log_n)
    return [O.g1_mul(O.G1, ls[i]) for i in (range(len(ls)) if only is None else only)]


def g1_ntt(points, log_n: int, direction: int):
    """the transform of the first 2^log_n points by the explicit double sum: for ANY points, n^2 scalar multiplications"""
    n = 1 << log_n
    w = O.domain_root(log_n)
    if direction == TO_LAGRANGE:
        w = pow(w, -1, R)
    out = []
    for i in range(n):
        acc = None
        for j in range(n):
            acc = O.g1_add(acc, O.g1_mul(points[j], pow(w, i * j, R)))
        out.append(O.g1_mul(acc, pow(n, -1, R)) if direction == TO_LAGRANGE else acc)
    return out
