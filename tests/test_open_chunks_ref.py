"""tests/open_chunks_ref.py against itself, tests/open_all_ref.py and the oracle (no GPU): the three statements of a polynomial's
multi-proofs over the cosets of its domain agree for every (log_n, log_l) up to log_n = 6, the circular route's h^ is h with the
identity at r - 1, l = 1 is the single-point statement, the interpolant from a coset's evaluations is the division's remainder,
and the verifier's equation holds on scalars.  And the boundary: the built library exports the three entry points, the header
declares them and states the formulas, a null context is refused."""
import os
import re

import numpy as np
import pytest

import open_all_ref as FK1
import open_chunks_ref as FK
from helpers import O, ROOT

R = O.R
SHAPES = [(log_n, log_l) for log_n in range(1, 7) for log_l in range(log_n)]


def _rand(rng, k):
    return [int.from_bytes(rng.bytes(32), "little") % R for _ in range(k)]


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_the_three_references_agree(log_n, log_l):
    n, l, r = FK.shape(log_n, log_l)
    rng = np.random.default_rng(0xC40 + 16 * log_n + log_l)
    s = _rand(rng, 1)[0]
    powers = [pow(s, m, R) for m in range(n + 3)]
    for m in (n, n // 2 + 1):
        f = _rand(rng, m)
        want = FK.openings_known_secret(f, s, log_n, log_l)
        assert len(want) == r
        assert FK.openings_of_point_scalars(f, powers, log_n, log_l) == want
        got, h_hat = FK.openings_circular(f, powers, log_n, log_l)
        assert got == want
        assert len(h_hat) == 2 * r and h_hat[r - 1] == 0 and h_hat[:r] == FK.h_of_point_scalars(f, powers, log_n, log_l)
        # the verifier's equation on scalars: f(s) - I_k(s) + a_k q_k(s) = q_k(s) s^l
        fs, sl = O.poly_eval(f, s), pow(s, l, R)
        for k, a in enumerate(FK.coset_constants(log_n, log_l)):
            rem = FK.divide(f + [0] * (n - m), l, a)[1]
            assert (fs - O.poly_eval(rem, s) + a * want[k] - want[k] * sl) % R == 0
    # arbitrary point scalars, exactly the n - l that are read: the double sum and the circular route
    ks, f = _rand(rng, n - l), _rand(rng, n)
    got, h_hat = FK.openings_circular(f, ks, log_n, log_l)
    assert got == FK.openings_of_point_scalars(f, ks, log_n, log_l) and h_hat[r - 1] == 0


@pytest.mark.parametrize("log_n", range(1, 7))
def test_one_point_per_coset_is_open_all(log_n):
    n = 1 << log_n
    rng = np.random.default_rng(0xC41 + log_n)
    ks, f = _rand(rng, n + 3), _rand(rng, n // 2 + 1)
    assert FK.openings_of_point_scalars(f, ks, log_n, 0) == FK1.openings_of_point_scalars(f, ks, log_n)
    assert FK.openings_known_secret(f, ks[0], log_n, 0) == FK1.openings_known_secret(f, ks[0], log_n)
    got, h_hat = FK.openings_circular(f, ks, log_n, 0)
    got1, h_hat1 = FK1.openings_circular(f, ks, log_n)
    assert got == got1 and h_hat == h_hat1
    assert FK.table(ks, log_n, 0) == O.ntt(FK1.circular_operands(f, ks, log_n)[0], log_n + 1)
    assert FK.coefficient_vectors(f, log_n, 0) == [FK1.circular_operands(f, ks, log_n)[1]]
    assert FK.evaluations(f, log_n, 0) == FK1.evaluations(f, log_n)


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_evaluations_and_the_interpolant(log_n, log_l):
    """chunk-major: the l values of coset k are contiguous and are f at w^(k + r t); the interpolant through them is the
    remainder of the division by X^l - a_k"""
    n, l, r = FK.shape(log_n, log_l)
    f = _rand(np.random.default_rng(0xC42 + 16 * log_n + log_l), n // 2 + 1)
    ev = FK.evaluations(f, log_n, log_l)
    w = O.domain_root(log_n)
    assert len(ev) == n
    for k, a in enumerate(FK.coset_constants(log_n, log_l)):
        ys = ev[k * l:(k + 1) * l]
        assert ys == [O.poly_eval(f, pow(w, k + r * t, R)) for t in range(l)]
        assert all(pow(pow(w, k + r * t, R), l, R) == a for t in range(l))       # the coset is the roots of X^l - a_k
        assert FK.interpolant(ys, k, log_n, log_l) == FK.divide(f + [0] * (n - len(f)), l, a)[1]


def test_the_library_exports_open_chunks_and_the_header_states_it(built):
    import typlonk_amd
    from typlonk_amd.capi import SYMBOLS, Context

    lib = typlonk_amd.load_library()
    for name in ("typlonk_srs_open_chunks_table", "typlonk_open_chunks_dev", "typlonk_open_chunks_host"):
        assert name in SYMBOLS and getattr(lib, name) is not None
    header = open(os.path.join(ROOT, "include", "typlonk.h")).read()
    assert re.search(r"int typlonk_srs_open_chunks_table\(typlonk_ctx\* ctx, uint32_t srs_id, uint32_t log_n, uint32_t log_l, uint32_t\* table_id\);", header)
    assert re.search(r"int typlonk_open_chunks_dev\(typlonk_ctx\* ctx, uint32_t table_id, const typlonk_buf\* const\* polys, const size_t\* offsets, size_t m,\s*"
                     r"size_t count, uint64_t\* proofs_xy /\* count\*r\*12 \*/, uint8_t\* proofs_inf /\* count\*r \*/,\s*"
                     r"uint64_t\* evals /\* count\*n\*4, chunk-major, or NULL \*/\);", header)
    assert re.search(r"int typlonk_open_chunks_host\(typlonk_ctx\* ctx, uint32_t table_id, const uint64_t\* const\* coeffs, size_t m, size_t count,\s*"
                     r"uint64_t\* proofs_xy, uint8_t\* proofs_inf, uint64_t\* evals\);", header)
    # the formulas
    flat = " ".join(header.split())
    for text in ("f = q_k (X^l - a_k) + I_k", "pi_k = [q_k(s)] G = sum_{i<r} [w^(l i k)] h_i",
                 "h_i = sum_{m=0}^{n-1-(i+1)l} f_(m+(i+1)l) S_m (i <= r - 2), h_(r-1) = O",
                 "y^(j) = DFT_2r(S^(j)_(r-2), ..., S^(j)_0, O x (r+1))", "u_i = sum_{j<l} [v^(j)_i] y^(j)_i",
                 "e(C - [I_k(s)]G + [a_k] pi_k, G2) = e(pi_k, [s^l]G2)", "f_p(w^(k + r t))", "y^(j)_i at record j 2r + i"):
        assert text in flat.replace(" * ", " "), text
    assert callable(Context.srs_open_chunks_table) and callable(Context.open_chunks)
    # without a context the calls are refused before they touch a device
    assert lib.typlonk_srs_open_chunks_table(None, 1, 3, 1, None) == -1
    assert lib.typlonk_open_chunks_dev(None, 1, None, None, 1, 1, None, None, None) == -1
    assert lib.typlonk_open_chunks_host(None, 1, None, 1, 1, None, None, None) == -1
