"""tests/open_all_ref.py against itself and the oracle (no GPU): the three statements of a polynomial's openings over its whole
domain agree, the circular route's h^ is h with the identity at n - 1, and every reference opening passes the restatement of
the reference's KzgScheme::verify.  And the boundary: the built library exports the three entry points, the header declares
them, a null context is refused."""
import os
import re

import numpy as np
import pytest

import open_all_ref as FK
from helpers import O, ROOT
from oracle import pairing as OP

R = O.R


def _rand(rng, k):
    return [int.from_bytes(rng.bytes(32), "little") % R for _ in range(k)]


@pytest.mark.parametrize("log_n", [1, 2, 3, 4])
def test_the_three_references_agree(log_n):
    n = 1 << log_n
    rng = np.random.default_rng(0xF20 + log_n)
    s = _rand(rng, 1)[0]
    powers = [pow(s, m, R) for m in range(n + 3)]
    for f in (_rand(rng, n), _rand(rng, n // 2 + 1), _rand(rng, 1), [0] * (n - 1) + [7]):
        want = FK.openings_known_secret(f, s, log_n)
        assert FK.openings_of_point_scalars(f, powers, log_n) == want
        got, h_hat = FK.openings_circular(f, powers, log_n)
        assert got == want
        assert h_hat[n - 1] == 0 and h_hat[:n] == FK.h_of_point_scalars(f, powers, log_n)
        # the closed quotient, where it is no 0/0
        ys = FK.evaluations(f, log_n)
        fs, w = O.poly_eval(f, s), O.domain_root(log_n)
        assert want == [(fs - ys[k]) * pow((s - pow(w, k, R)) % R, -1, R) % R for k in range(n)]
    # arbitrary point scalars: the double sum and the circular route
    ks, f = _rand(rng, n + 1), _rand(rng, n)
    got, h_hat = FK.openings_circular(f, ks, log_n)
    assert got == FK.openings_of_point_scalars(f, ks, log_n) and h_hat[n - 1] == 0


def test_a_secret_in_the_domain_takes_the_division():
    log_n, n = 3, 8
    s = pow(O.domain_root(log_n), 5, R)
    f = _rand(np.random.default_rng(0xD0), n)
    powers = [pow(s, m, R) for m in range(n)]
    want = FK.openings_known_secret(f, s, log_n)
    assert FK.openings_of_point_scalars(f, powers, log_n) == want
    assert FK.openings_circular(f, powers, log_n)[0] == want


def test_every_reference_opening_verifies():
    """log_n = 3: [q_k(s)] G with f(w^k) passes KzgScheme::verify against [f(s)] G for every k; y + 1 does not"""
    log_n, n = 3, 8
    rng = np.random.default_rng(0x7E51)
    s = _rand(rng, 1)[0]
    f = _rand(rng, n)
    g2, g2s = OP.srs_g2(s)
    commitment = O.g1_mul(O.G1, O.poly_eval(f, s))
    proofs = FK.points(FK.openings_known_secret(f, s, log_n))
    ys = FK.evaluations(f, log_n)
    w = O.domain_root(log_n)
    for k in range(n):
        assert OP.kzg_verify(commitment, (proofs[k], ys[k]), pow(w, k, R), g2, g2s), k
    assert not OP.kzg_verify(commitment, (proofs[3], (ys[3] + 1) % R), pow(w, 3, R), g2, g2s)


def test_the_library_exports_open_all_and_the_header_declares_it(built):
    import typlonk_amd
    from typlonk_amd.capi import SYMBOLS, Context

    lib = typlonk_amd.load_library()
    for name in ("typlonk_srs_open_all_table", "typlonk_open_all_dev", "typlonk_open_all_host"):
        assert name in SYMBOLS and getattr(lib, name) is not None
    header = open(os.path.join(ROOT, "include", "typlonk.h")).read()
    assert re.search(r"int typlonk_srs_open_all_table\(typlonk_ctx\* ctx, uint32_t srs_id, uint32_t log_n, uint32_t\* table_id\);", header)
    assert re.search(r"int typlonk_open_all_dev\s*\(typlonk_ctx\* ctx, uint32_t table_id, const typlonk_buf\* poly, size_t offset, size_t m,\s*"
                     r"uint64_t\* proofs_xy /\* n\*12 \*/, uint8_t\* proofs_inf /\* n \*/, uint64_t\* evals /\* n\*4 or NULL \*/\);", header)
    assert re.search(r"int typlonk_open_all_host\(typlonk_ctx\* ctx, uint32_t table_id, const uint64_t\* coeffs, size_t m,\s*"
                     r"uint64_t\* proofs_xy, uint8_t\* proofs_inf, uint64_t\* evals\);", header)
    assert callable(Context.srs_open_all_table) and callable(Context.open_all)
    # without a context the calls are refused before they touch a device
    assert lib.typlonk_srs_open_all_table(None, 1, 3, None) == -1
    assert lib.typlonk_open_all_dev(None, 1, None, 0, 1, None, None, None) == -1
    assert lib.typlonk_open_all_host(None, 1, None, 1, None, None, None) == -1
