"""tests/srs_lagrange_ref.py against itself and the oracle (no GPU): the closed form of L_i(s) is the inverse transform of
the powers of s, a combination of the Lagrange scalars with a column of evaluations is the interpolated polynomial at s, and
the double sum in the group agrees with both.  And the boundary: the built library exports typlonk_srs_g1_ntt, the header
declares it."""
import os
import re

import numpy as np
import pytest

import srs_lagrange_ref as LR
from helpers import O, ROOT

R = O.R


@pytest.mark.parametrize("log_n", [0, 1, 3, 5])
def test_closed_form_is_the_inverse_transform_of_the_powers(log_n):
    n = 1 << log_n
    rng = np.random.default_rng(0x1A6 + log_n)
    s = int.from_bytes(rng.bytes(32), "little") % R
    ls = LR.lagrange_scalars(s, log_n)
    assert ls == LR.scalars_to_lagrange([pow(s, j, R) for j in range(n)], log_n)
    evals = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(n)]
    assert sum(e * l for e, l in zip(evals, ls)) % R == O.poly_eval(O.interpolate(evals, log_n), s)


def test_a_secret_in_the_domain_takes_the_transform():
    w = O.domain_root(4)
    assert LR.lagrange_scalars(pow(w, 5, R), 4) == [1 if i == 5 else 0 for i in range(16)]
    assert LR.lagrange_scalars(1, 3) == [1] + [0] * 7
    assert LR.lagrange_scalars(0, 3) == [pow(8, -1, R)] * 8


def test_the_double_sum_in_the_group():
    ks = [5, 0, R - 2, 0x1234567890ABCDEF]
    pts = [O.g1_mul(O.G1, k) for k in ks]
    lag = LR.g1_ntt(pts, 2, LR.TO_LAGRANGE)
    assert lag == [O.g1_mul(O.G1, k) for k in LR.scalars_to_lagrange(ks, 2)]
    assert LR.g1_ntt(lag, 2, LR.FROM_LAGRANGE) == pts


def test_the_library_exports_the_transform_and_the_header_declares_it(built):
    import typlonk_amd
    from typlonk_amd.capi import SYMBOLS, Context

    lib = typlonk_amd.load_library()
    assert "typlonk_srs_g1_ntt" in SYMBOLS and getattr(lib, "typlonk_srs_g1_ntt") is not None
    header = open(os.path.join(ROOT, "include", "typlonk.h")).read()
    assert re.search(r"int typlonk_srs_g1_ntt\(typlonk_ctx\* ctx, uint32_t srs_id, uint32_t log_n, uint32_t direction, "
                     r"uint32_t\* new_srs_id\);", header)
    assert re.search(r"#define TYPLONK_SRS_TO_LAGRANGE\s+0\b", header) and re.search(r"#define TYPLONK_SRS_FROM_LAGRANGE\s+1\b", header)
    assert callable(Context.srs_lagrange) and callable(Context.srs_from_lagrange)
    # without a context the call is refused before it touches a device
    assert lib.typlonk_srs_g1_ntt(None, 1, 0, 0, None) == -1
