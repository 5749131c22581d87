"""The big-integer statement of typlonk_recover_chunks (include/typlonk.h): polynomials from K of the r cosets of their domain.
n = 2^log_n, l = 2^log_l, r = n / l, w = O.domain_root(log_n), a_k = w^(k l); coset k < r is {w^(k + r t) : t < l} and a cell holds
the l evaluations on one coset in that order.  cosets: K distinct indices in any order; cells[i][t] = f(w^(cosets[i] + r t)).

`recover` is the library's recipe, step by step: with M the cosets that are not named, Z'(Y) = prod_{j in M} (Y - a_j) and
Z(X) = Z'(X^l),
    1. Zd[k] = Z'(a_k) -- Z on every point of coset k -- and Zc[i] = Z'(g^l a_i), Z at g w^i' for i' = i mod r; g = 7
    2. V[k + r t] = cells[i][t] Zd[cosets[i]], zero on the missing cosets: h Z on the whole domain
    3. P = iNTT_n(V) = h Z exactly, because deg < K l + (r - K) l = n
    4. coset NTT_n of P (shift g), times 1 / Zc[i mod r], coset iNTT_n (shift g): the n coefficients of h, zero from K l on
    5. `verdict`: consistent with the degree bound m iff coefficients [m, K l) are zero
`lagrange` is the independent statement the recipe is tested against: the one polynomial of degree < K l through the K l points,
by the Lagrange formula over plain polynomial products, with no transform, no vanishing polynomial and no coset in it."""
from __future__ import annotations

from oracle import bls12_381 as O

R = O.R
COSET_G = 7
OK, BAD_EVAL, INCONSISTENT = 0, 1, 2
NO_EXCESS = (1 << 64) - 1


def shape(log_n: int, log_l: int):
    assert 0 <= log_l < log_n
    n, l = 1 << log_n, 1 << log_l
    return n, l, n // l


def points(cosets, log_n: int, log_l: int):
    """the K l points of the cells, cell by cell"""
    n, l, r = shape(log_n, log_l)
    w = O.domain_root(log_n)
    return [pow(w, k + r * t, R) for k in cosets for t in range(l)]


def cells_of(f, cosets, log_n: int, log_l: int):
    """the cells of the polynomial f (any length) on the named cosets, by Horner at every point"""
    n, l, r = shape(log_n, log_l)
    xs = points(cosets, log_n, log_l)
    return [[O.poly_eval(list(f), xs[i * l + t]) for t in range(l)] for i in range(len(cosets))]


def vanishing(cosets, log_n: int, log_l: int):
    """(missing cosets ascending, Zd (r), Zc (r))"""
    n, l, r = shape(log_n, log_l)
    assert len(set(cosets)) == len(cosets) >= 1 and all(0 <= k < r for k in cosets)
    w = O.domain_root(log_n)
    a = [pow(w, k * l, R) for k in range(r)]
    missing = [k for k in range(r) if k not in set(cosets)]
    gl = pow(COSET_G, l, R)

    def z_prime(y):
        acc = 1
        for j in missing:
            acc = acc * (y - a[j]) % R
        return acc

    return missing, [z_prime(a[k]) for k in range(r)], [z_prime(gl * a[i] % R) for i in range(r)]


def recover(cells, cosets, log_n: int, log_l: int):
    """the n coefficients of h, the polynomial of degree < K l through the cells (coefficients [K l, n) come out zero)"""
    n, l, r = shape(log_n, log_l)
    assert len(cells) == len(cosets) and all(len(c) == l for c in cells)
    _, zd, zc = vanishing(cosets, log_n, log_l)
    v = [0] * n
    for i, k in enumerate(cosets):
        for t in range(l):
            v[k + r * t] = cells[i][t] * zd[k] % R
    p = O.ntt(v, log_n, inverse=True)
    e = O.ntt(p, log_n, coset=COSET_G)
    e = [x * pow(zc[i % r], -1, R) % R for i, x in enumerate(e)]
    return O.ntt(e, log_n, inverse=True, coset=COSET_G)


def verdict(h, m: int, kl: int):
    """(status, first_excess) of the coefficients h under the degree bound m"""
    for j in range(m, kl):
        if h[j] % R:
            return INCONSISTENT, j
    return OK, NO_EXCESS


def recover_chunks(cells, cosets, m: int, log_n: int, log_l: int):
    """what the call returns for one polynomial: (status, first_excess, m coefficients, n evaluations chunk-major), zeros when
    the status is not OK"""
    n, l, r = shape(log_n, log_l)
    kl = len(cosets) * l
    assert 1 <= m <= kl
    h = recover(cells, cosets, log_n, log_l)
    status, first = verdict(h, m, kl)
    if status != OK:
        return status, first, [0] * m, [0] * n
    ev = O.ntt(h[:m] + [0] * (n - m), log_n)
    return status, first, h[:m], [ev[k + r * t] for k in range(r) for t in range(l)]


def lagrange(xs, ys):
    """the coefficients (len(xs) of them) of the polynomial of degree < len(xs) with value ys[i] at xs[i]: sum_i ys[i] N_i / N_i(xs[i]),
    N_i = prod_{j != i} (X - xs[j]) = N / (X - xs[i]) by synthetic division of the full product N"""
    k = len(xs)
    assert len(ys) == k and len(set(xs)) == k
    full = [1]
    for x in xs:                                   # N <- N (X - x)
        full = [((full[i - 1] if i else 0) - x * (full[i] if i < len(full) else 0)) % R for i in range(len(full) + 1)]
    out = [0] * k
    for x, y in zip(xs, ys):
        q = [0] * k                                # N / (X - x), from the top coefficient down
        carry = 0
        for i in range(k, 0, -1):
            carry = (full[i] + carry * x) % R
            q[i - 1] = carry
        scale = y * pow(O.poly_eval(q, x), -1, R) % R
        for i in range(k):
            out[i] = (out[i] + scale * q[i]) % R
    return out
