"""tests/recover_chunks_ref.py, the big-integer recipe of typlonk_recover_chunks, against an independent reference -- plain Lagrange
interpolation through the K l points, with no transform and no vanishing polynomial in it -- at every (log_n, log_l) with
log_n <= 5, with minimal K (K l = m, no redundancy), K = r / 2, r - 1 and r, random known sets in a shuffled order; and its two
invariants: coefficients [K l, n) are zero for ARBITRARY cell values, and a polynomial is consistent with a degree bound m iff
coefficients [m, K l) are zero -- the cells of a polynomial of degree < m are, the same cells with one value changed are not,
and the first excess coefficient of a constructed h is reported where it was put."""
import random

import pytest

import open_chunks_ref as CR
import recover_chunks_ref as RR
from helpers import O

R = O.R
SHAPES = [(log_n, log_l) for log_n in range(1, 6) for log_l in range(log_n)]


def _known_sets(rng, r):
    """K = 1, r / 2, r - 1, r (where distinct), random sets in a shuffled order"""
    out = []
    for k in sorted({1, max(r // 2, 1), max(r - 1, 1), r}):
        s = rng.sample(range(r), k)
        out.append(s)
    return out


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_the_recipe_is_lagrange_interpolation(log_n, log_l):
    n, l, r = RR.shape(log_n, log_l)
    rng = random.Random(1000 * log_n + log_l)
    for cosets in _known_sets(rng, r):
        kl = len(cosets) * l
        cells = [[rng.randrange(R) for _ in range(l)] for _ in cosets]          # arbitrary values
        h = RR.recover(cells, cosets, log_n, log_l)
        assert h[kl:] == [0] * (n - kl), (cosets, "coefficients [K l, n) are zero for arbitrary values")
        want = RR.lagrange(RR.points(cosets, log_n, log_l), [y for c in cells for y in c])
        assert h[:kl] == want, cosets
        assert RR.cells_of(h[:kl], cosets, log_n, log_l) == cells


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_consistent_iff_the_excess_coefficients_are_zero(log_n, log_l):
    n, l, r = RR.shape(log_n, log_l)
    rng = random.Random(2000 * log_n + log_l)
    for cosets in _known_sets(rng, r):
        kl = len(cosets) * l
        for m in sorted({1, l, max(kl - 1, 1), kl}):
            if m > kl:
                continue
            f = [rng.randrange(R) for _ in range(m)]
            cells = RR.cells_of(f, cosets, log_n, log_l)
            status, first, coeffs, evals = RR.recover_chunks(cells, cosets, m, log_n, log_l)
            assert (status, first, coeffs) == (RR.OK, RR.NO_EXCESS, f), (cosets, m)
            assert evals == CR.evaluations(f, log_n, log_l)
            # a nonzero coefficient put at j in [m, K l): inconsistent, and j is named
            for j in sorted({m, (m + kl) // 2, kl - 1}):
                if not m <= j < kl:
                    continue
                g = f + [0] * (kl - m)
                g[j] = rng.randrange(1, R)
                bad = RR.cells_of(g, cosets, log_n, log_l)
                assert RR.recover_chunks(bad, cosets, m, log_n, log_l) == (RR.INCONSISTENT, j, [0] * m, [0] * n), (cosets, m, j)
                assert RR.recover_chunks(bad, cosets, kl, log_n, log_l)[:3] == (RR.OK, RR.NO_EXCESS, g)   # m = K l: an interpolation
            # one evaluation changed under redundancy: some excess coefficient is not zero (h - f vanishes on K l - 1 points
            # and not on the last, so its degree is exactly K l - 1 >= m)
            if m < kl:
                i, t = rng.randrange(len(cosets)), rng.randrange(l)
                cells[i][t] = (cells[i][t] + 1) % R
                status, first, coeffs, _ = RR.recover_chunks(cells, cosets, m, log_n, log_l)
                assert status == RR.INCONSISTENT and m <= first < kl and coeffs == [0] * m


def test_the_vanishing_values():
    """Zd is zero exactly on the missing cosets and is Z on every point of a coset; Zc is Z on the shifted domain, period r, and
    never zero; the odd cosets missing: Z' = Y^(r/2) + 1"""
    log_n, log_l = 5, 2
    n, l, r = RR.shape(log_n, log_l)
    w = O.domain_root(log_n)
    cosets = [6, 1, 3]
    missing, zd, zc = RR.vanishing(cosets, log_n, log_l)
    assert missing == [0, 2, 4, 5, 7]
    z = [1]
    for j in missing:                               # Z(X) = prod (X^l - a_j), as a polynomial
        a = pow(w, j * l, R)
        nz = [0] * (len(z) + l)
        for i, c in enumerate(z):
            nz[i + l] = (nz[i + l] + c) % R
            nz[i] = (nz[i] - a * c) % R
        z = nz
    for k in range(r):
        assert (zd[k] == 0) == (k in missing)
        for t in range(l):
            assert O.poly_eval(z, pow(w, k + r * t, R)) == zd[k]
    for i in range(n):
        assert O.poly_eval(z, RR.COSET_G * pow(w, i, R) % R) == zc[i % r] != 0
    _, zd, zc = RR.vanishing(list(range(0, r, 2)), log_n, log_l)
    a = [pow(w, k * l, R) for k in range(r)]
    assert zd == [(pow(a[k], r // 2, R) + 1) % R for k in range(r)]
    assert zc == [(pow(pow(RR.COSET_G, l, R) * a[k], r // 2, R) + 1) % R for k in range(r)]
