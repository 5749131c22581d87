"""tests/verify_chunks_ref.py, the big-integer statement of typlonk_verify_chunks, on small shapes -- and the one piece of the
feature that needs no GPU: typlonk_verify_chunks_challenge against hashlib.

The cells are the honest openings of tests/open_chunks_ref.py for a known s: A is the weighted sum of FK.interpolant's
coefficients (the l^2 sum, where the reference itself goes through O.ntt); the honest cells satisfy the fold for every
sub-range; each tampering the GPU tests use breaks it, and the bisection of `check` names exactly the tampered cells."""
import numpy as np
import pytest

import open_chunks_ref as FK
import verify_chunks_ref as VR
from helpers import O
from oracle import pairing as PR

R = O.R
SHAPES = [(4, 2), (6, 3)]
SEEDS = [bytes(32), bytes(range(32)), bytes([0xFF] * 32)]


def _rand(rng, k):
    return [int.from_bytes(rng.bytes(32), "little") % R for _ in range(k)]


def honest(log_n, log_l, polys, seed):
    """(cells, commitment scalars, s): every cell of `polys` random polynomials, cell (p, k) at position p r + k"""
    n, l, r = FK.shape(log_n, log_l)
    rng = np.random.default_rng(seed)
    s = _rand(rng, 1)[0]
    fs = [_rand(rng, n) for _ in range(polys)]
    cells = []
    for p, f in enumerate(fs):
        ev = FK.evaluations(f, log_n, log_l)
        pis = FK.openings_known_secret(f, s, log_n, log_l)
        cells += [(p, k, ev[k * l:(k + 1) * l], pis[k]) for k in range(r)]
    return cells, [O.poly_eval(f, s) for f in fs], s


def tamper(cells, i, how, log_n, log_l, M):
    """the four tamperings of the GPU tests, on a copy"""
    n, l, r = FK.shape(log_n, log_l)
    c, k, ys, pi = cells[i]
    out = list(cells)
    if how == "eval":
        out[i] = (c, k, ys[:-1] + [(ys[-1] + 1) % R], pi)
    elif how == "proof":
        out[i] = (c, k, ys, (pi + 1) % R)
    elif how == "coset":
        out[i] = (c, (k + 1) % r, ys, pi)
    else:
        assert how == "commitment"
        out[i] = ((c + 1) % M, k, ys, pi)
    return out


TAMPERINGS = ["eval", "proof", "coset", "commitment"]


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_fold_coefficients_are_the_weighted_interpolants(log_n, log_l):
    n, l, r = FK.shape(log_n, log_l)
    cells, _, _ = honest(log_n, log_l, 2, 0xA11 + log_n)
    for c, k, ys, _ in cells:                                   # the transform on the coset is the l^2 sum
        assert VR.interpolant(ys, k, log_n, log_l) == FK.interpolant(ys, k, log_n, log_l)
    rho = 0x1234567 * 0x89ABCDEF % R
    live = [i % 5 != 3 for i in range(len(cells))]
    for lo, hi in [(0, len(cells)), (3, 11), (r - 1, r + 2)]:
        w = VR.weights(len(cells), rho, lo, hi, live)
        want = [0] * l
        for i, (c, k, ys, _) in enumerate(cells):
            if lo <= i < hi and live[i]:
                want = [(a + pow(rho, i, R) * b) % R for a, b in zip(want, FK.interpolant(ys, k, log_n, log_l))]
        assert VR.fold_coefficients(cells, w, log_n, log_l) == want


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_honest_cells_satisfy_every_sub_range(log_n, log_l):
    cells, commitments, s = honest(log_n, log_l, 2, 0xB22 + log_n)
    N = len(cells)
    assert all(VR.cell_holds(c, commitments, s, log_n, log_l) for c in cells)
    rho = VR.rho(SEEDS[1], log_n, log_l, N, 2, PR.srs_g2(pow(s, 1 << log_l, R))[1])
    step = 1 if N <= 8 else 3
    for lo in range(0, N, step):
        for hi in range(lo + 1, N + 1, step):
            assert VR.fold_holds(cells, commitments, s, rho, log_n, log_l, lo, hi), (lo, hi)
    assert VR.check(cells, commitments, s, rho, log_n, log_l) == ([VR.OK] * N, 1)


@pytest.mark.parametrize("log_n,log_l", SHAPES)
@pytest.mark.parametrize("how", TAMPERINGS)
def test_each_tampering_breaks_the_fold(log_n, log_l, how):
    cells, commitments, s = honest(log_n, log_l, 2, 0xC33 + log_n)
    N = len(cells)
    rho = VR.rho(SEEDS[2], log_n, log_l, N, 2, PR.srs_g2(pow(s, 1 << log_l, R))[1])
    at = N // 2 + 1
    bad = tamper(cells, at, how, log_n, log_l, 2)
    assert not VR.cell_holds(bad[at], commitments, s, log_n, log_l)
    assert not VR.fold_holds(bad, commitments, s, rho, log_n, log_l)
    assert not VR.fold_holds(bad, commitments, s, rho, log_n, log_l, at, at + 1)
    assert VR.fold_holds(bad, commitments, s, rho, log_n, log_l, 0, at) and VR.fold_holds(bad, commitments, s, rho, log_n, log_l, at + 1, N)
    status, folds = VR.check(bad, commitments, s, rho, log_n, log_l)
    assert status == [VR.BAD_PROOF if i == at else VR.OK for i in range(N)]
    assert folds <= 2 * (N - 1).bit_length() + 1
    # a cell kept from the fold is not judged by it
    status, folds = VR.check(bad, commitments, s, rho, log_n, log_l, dead={at: VR.BAD_POINT})
    assert status == [VR.BAD_POINT if i == at else VR.OK for i in range(N)] and folds == 1


def test_three_tamperings_at_once():
    log_n, log_l = 6, 3
    cells, commitments, s = honest(log_n, log_l, 3, 0xD44)
    N = len(cells)
    rho = VR.rho(SEEDS[0], log_n, log_l, N, 3, PR.srs_g2(pow(s, 1 << log_l, R))[1])
    at = {1: "eval", 9: "coset", N - 1: "proof"}
    bad = cells
    for i, how in at.items():
        bad = tamper(bad, i, how, log_n, log_l, 3)
    status, folds = VR.check(bad, commitments, s, rho, log_n, log_l)
    assert status == [VR.BAD_PROOF if i in at else VR.OK for i in range(N)]
    assert folds <= 2 * 3 * (N - 1).bit_length() + 1


def test_rho_reads_every_input():
    g2sl = PR.srs_g2(5)[1]
    base = VR.rho(SEEDS[1], 13, 6, 128, 2, g2sl)
    others = [VR.rho(SEEDS[0], 13, 6, 128, 2, g2sl), VR.rho(SEEDS[1], 12, 6, 128, 2, g2sl), VR.rho(SEEDS[1], 13, 5, 128, 2, g2sl),
              VR.rho(SEEDS[1], 13, 6, 129, 2, g2sl), VR.rho(SEEDS[1], 13, 6, 128, 3, g2sl), VR.rho(SEEDS[1], 13, 6, 128, 2, PR.srs_g2(6)[1])]
    assert len({base, *others}) == 7 and all(0 <= x < R for x in [base, *others])


def test_native_challenge_equals_the_python_statement(built):
    """typlonk_verify_chunks_challenge (host-only) == rho, three seeds x two shapes"""
    from typlonk_amd.capi import verify_chunks_challenge

    g2sl = PR.srs_g2(0xABCDEF)[1]
    limbs = np.array(VR.g2_limbs(g2sl), dtype=np.uint64)
    for seed in SEEDS:
        for log_n, log_l, N, M in [(4, 2, 4, 1), (20, 6, (1 << 14) + 3, 128)]:
            got = verify_chunks_challenge(seed, log_n, log_l, N, M, limbs)
            assert O.fr_from_mont_limbs([int(x) for x in got]) == VR.rho(seed, log_n, log_l, N, M, g2sl), (seed, log_n)
