"""The big-integer statement of typlonk_srs_open_chunks_table / typlonk_open_chunks_* (include/typlonk.h): the KZG multi-proofs of
a polynomial f on every coset of its domain.  n = 2^log_n, l = 2^log_l, r = n / l >= 2, w = O.domain_root(log_n); coset k < r is
{w^(k + r t) : t < l}, the roots of X^l - a_k with a_k = w^(k l).

With S_m the SRS points and f_0 .. f_(n-1) the coefficients (zero-padded),

    f = q_k (X^l - a_k) + I_k,  deg I_k < l          pi_k = [q_k(s)] G = sum_{i<r} [w^(l i k)] h_i
    h_i = sum_{m=0}^{n-1-(i+1)l} f_(m+(i+1)l) S_m  (i <= r - 2),  h_(r-1) = O

Everything here works on SCALARS: a point [a]G is stood for by a.  Three references, by what is known about the points:
  * S_m = [s^m] G with s KNOWN: the scalar of pi_k is q_k(s), q_k by schoolbook division by X^l - a_k (`openings_known_secret`);
  * S_m = [k_m] G for known k_m, any at all: the double sum itself (`openings_of_point_scalars`);
  * the same by the circular route of size 2r over the l decimated sequences that the library takes, step by step, with the
    table in the library's layout (`openings_circular`).
And the evaluations in the library's chunk-major order, and the coefficients of I_k from the l evaluations on coset k."""
from __future__ import annotations

from oracle import bls12_381 as O

R = O.R


def shape(log_n: int, log_l: int):
    """(n, l, r); the generator of the size-r domain is w^l"""
    assert 0 <= log_l < log_n
    n, l = 1 << log_n, 1 << log_l
    assert O.domain_root(log_n - log_l) == pow(O.domain_root(log_n), l, R)
    return n, l, n // l


def _padded(f, log_n: int):
    n = 1 << log_n
    assert 1 <= len(f) <= n
    return [x % R for x in f] + [0] * (n - len(f))


def coset_constants(log_n: int, log_l: int):
    """a_k = w^(k l), k < r"""
    n, l, r = shape(log_n, log_l)
    w = O.domain_root(log_n)
    return [pow(w, k * l, R) for k in range(r)]


def evaluations(f, log_n: int, log_l: int):
    """chunk-major: out[k l + t] = f(w^(k + r t))"""
    n, l, r = shape(log_n, log_l)
    ev = O.ntt(_padded(f, log_n), log_n)
    return [ev[k + r * t] for k in range(r) for t in range(l)]


def divide(f, l: int, a: int):
    """(q, I): f = q (X^l - a) + I with deg I < l, schoolbook from the top coefficient down"""
    work = [x % R for x in f]
    q = [0] * max(len(work) - l, 0)
    for i in range(len(work) - 1, l - 1, -1):
        q[i - l] = work[i]
        work[i - l] = (work[i - l] + a * work[i]) % R
    return q, work[:l]


def openings_known_secret(f, s: int, log_n: int, log_l: int):
    """q_k(s) for every k < r: r divisions by X^l - a_k"""
    n, l, r = shape(log_n, log_l)
    f = _padded(f, log_n)
    return [O.poly_eval(q, s) if q else 0 for q in (divide(f, l, a)[0] for a in coset_constants(log_n, log_l))]


def h_of_point_scalars(f, ks, log_n: int, log_l: int):
    """the scalars of h_0 .. h_(r-1) for S_m = [ks[m]] G (ks may be longer than the n - l that are read)"""
    n, l, r = shape(log_n, log_l)
    f = _padded(f, log_n)
    assert len(ks) >= n - l
    return [sum(f[m + (i + 1) * l] * ks[m] for m in range(n - (i + 1) * l)) % R for i in range(r)]


def openings_of_point_scalars(f, ks, log_n: int, log_l: int):
    """the scalars of pi_k for S_m = [ks[m]] G: the forward transform of h over the size-r domain"""
    return O.ntt(h_of_point_scalars(f, ks, log_n, log_l), log_n - log_l)


def table(ks, log_n: int, log_l: int):
    """the 2n scalars of the table: block j < l is DFT_2r(S^(j)_(r-2), ..., S^(j)_0, 0 x (r + 1)), S^(j)_a = ks[a l + j], and
    y^(j)_i lies at j 2r + i"""
    n, l, r = shape(log_n, log_l)
    out = []
    for j in range(l):
        out += O.ntt([ks[(r - 2 - i) * l + j] % R for i in range(r - 1)] + [0] * (r + 1), log_n - log_l + 1)
    assert len(out) == 2 * n
    return out


def coefficient_vectors(f, log_n: int, log_l: int):
    """c^(j) = (f^(j)_(r-1), 0 x r, f^(j)_0, ..., f^(j)_(r-2)), f^(j)_a = f_(a l + j): l vectors of 2r"""
    n, l, r = shape(log_n, log_l)
    f = _padded(f, log_n)
    return [[f[(r - 1) * l + j]] + [0] * r + [f[a * l + j] for a in range(r - 1)] for j in range(l)]


def openings_circular(f, ks, log_n: int, log_l: int):
    """(the scalars of pi_k, h^): v^(j) = NTT_2r(c^(j)) / 2r; u_i = sum_j v^(j)_i y^(j)_i; h^ = DFT_2r^-1(u) without scaling;
    pi = DFT_r(h^[:r]).  h^ is returned whole: h^[r-1] must be 0 and h^[:r] the h of the double sum."""
    n, l, r = shape(log_n, log_l)
    y = table(ks, log_n, log_l)
    inv2r = pow(2 * r, -1, R)
    v = [[x * inv2r % R for x in O.ntt(c, log_n - log_l + 1)] for c in coefficient_vectors(f, log_n, log_l)]
    u = [sum(v[j][i] * y[j * 2 * r + i] for j in range(l)) % R for i in range(2 * r)]
    w_inv = pow(O.domain_root(log_n - log_l + 1), -1, R)
    h_hat = O.dft_naive(u, w_inv)
    return O.ntt(h_hat[:r], log_n - log_l), h_hat


def interpolant(ys, k: int, log_n: int, log_l: int):
    """the l coefficients of I_k from ys[t] = f(w^(k + r t)):  c_t = w^(-k t) (1/l) sum_u ys[u] mu^(-t u),  mu = w^r"""
    n, l, r = shape(log_n, log_l)
    assert len(ys) == l
    w = O.domain_root(log_n)
    mu_inv = pow(pow(w, r, R), -1, R)
    w_inv_k = pow(pow(w, k, R), -1, R)
    l_inv = pow(l, -1, R)
    return [pow(w_inv_k, t, R) * l_inv % R * sum(ys[u] * pow(mu_inv, t * u, R) for u in range(l)) % R for t in range(l)]


def points(scalars):
    """[a] G for every scalar (None = the identity)"""
    return [O.g1_mul(O.G1, a % R) for a in scalars]
