"""The big-integer statement of typlonk_srs_open_all_table / typlonk_open_all_* (include/typlonk.h): the KZG openings of a
polynomial f at every point w^k of its domain, k < n = 2^log_n, w = O.domain_root(log_n).

With S_m the SRS points and f_0 .. f_(n-1) the coefficients (zero-padded), the opening at w^k is

    pi_k = sum_{i<n} [w^(ik)] h_i,     h_i = sum_{m=0}^{n-2-i} f_(m+i+1) S_m  (i <= n - 2),  h_(n-1) = O

Everything here works on SCALARS: a point [a]G is stood for by a.  Three references, by what is known about the points:
  * S_m = [s^m] G with s KNOWN: the scalar of pi_k is q_k(s), q_k = (f - f(w^k)) / (X - w^k) by synthetic division -- valid
    also when s lies in the domain, where the closed quotient (f(s) - f(w^k)) / (s - w^k) is 0/0 (`openings_known_secret`);
  * S_m = [k_m] G for known k_m, any at all: the double sum itself (`openings_of_point_scalars`);
  * the same by the circular route of size 2n the library takes, step by step (`openings_circular`)."""
from __future__ import annotations

from oracle import bls12_381 as O

R = O.R


def _padded(f, log_n: int):
    n = 1 << log_n
    assert 1 <= len(f) <= n
    return [x % R for x in f] + [0] * (n - len(f))


def evaluations(f, log_n: int):
    """f(w^k), k < n"""
    return O.ntt(_padded(f, log_n), log_n)


def openings_known_secret(f, s: int, log_n: int):
    """q_k(s) for every k: n synthetic divisions"""
    f = _padded(f, log_n)
    w = O.domain_root(log_n)
    out, z = [], 1
    for _ in range(1 << log_n):
        q, _y = O.poly_div_linear(f, z)
        out.append(O.poly_eval(q, s) if q else 0)
        z = z * w % R
    return out


def h_of_point_scalars(f, ks, log_n: int):
    """the scalars of h_0 .. h_(n-1) for S_m = [ks[m]] G (ks may be longer than the n - 1 that are read)"""
    n = 1 << log_n
    f = _padded(f, log_n)
    assert len(ks) >= n - 1
    return [sum(f[m + i + 1] * ks[m] for m in range(n - 1 - i)) % R for i in range(n)]


def openings_of_point_scalars(f, ks, log_n: int):
    """the scalars of pi_k for S_m = [ks[m]] G: the forward transform of h"""
    return O.ntt(h_of_point_scalars(f, ks, log_n), log_n)


def circular_operands(f, ks, log_n: int):
    """(S^, c): the 2n-element operands of the circular product"""
    n = 1 << log_n
    f = _padded(f, log_n)
    s_hat = [ks[n - 2 - i] % R for i in range(n - 1)] + [0] * (n + 1)
    c = [f[n - 1]] + [0] * n + f[:n - 1]
    assert len(s_hat) == len(c) == 2 * n
    return s_hat, c


def openings_circular(f, ks, log_n: int):
    """(the scalars of pi_k, h^): table y = DFT_2n(S^); v = NTT_2n(c) / 2n; u = v * y; h^ = DFT_2n^-1(u) without scaling;
    pi = DFT_n(h^[:n]).  h^ is returned whole: h^[n-1] must be 0 and h^[:n] the h of the double sum."""
    n = 1 << log_n
    s_hat, c = circular_operands(f, ks, log_n)
    y = O.ntt(s_hat, log_n + 1)
    inv2n = pow(2 * n, -1, R)
    v = [x * inv2n % R for x in O.ntt(c, log_n + 1)]
    u = [a * b % R for a, b in zip(v, y)]
    w_inv = pow(O.domain_root(log_n + 1), -1, R)
    h_hat = O.dft_naive(u, w_inv)
    return O.ntt(h_hat[:n], log_n), h_hat


def points(scalars):
    """[a] G for every scalar (None = the identity)"""
    return [O.g1_mul(O.G1, a % R) for a in scalars]
