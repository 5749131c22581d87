"""tests/verify_chunks_ref.py, the big-integer statement of typlonk_verify_chunks, on small shapes -- and the one piece of the
feature that needs no GPU: typlonk_verify_chunks_challenge against hashlib.

The cells are the honest openings of tests/open_chunks_ref.py for a known s: A is the weighted sum of FK.interpolant's
coefficients (the l^2 sum, where the reference itself goes through O.ntt); the honest cells satisfy the fold for every
sub-range; each tampering the GPU tests use breaks it, and the bisection of `check` names exactly the tampered cells.

What tests/test_gpu_verify_chunks_wide.py leans on, at (10, 3) and (8, 0) -- r = 128 and 256 cosets --: `check` accepts the cells
made of tests/g1_wide_ref.py's closed forms, `cell_holds` rejects a coset moved in bit 5 and in its top bit, and `check` blames
exactly the cells of a commitment that was replaced."""
import numpy as np
import pytest

import g1_wide_ref as W
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


WIDE = [(10, 3), (8, 0)]
_wide = {}


def wide(log_n, log_l):
    """(cells, commitment scalars, s) of two random polynomials from g1_wide_ref's closed forms, cell (p, k) at position p r + k;
    made once a shape"""
    if (log_n, log_l) not in _wide:
        n, l, r = FK.shape(log_n, log_l)
        rng = np.random.default_rng(0x71DE + 64 * log_n + log_l)
        s = _rand(rng, 1)[0]
        cells, commitments = [], []
        for p in range(2):
            f = _rand(rng, n)
            ys = W.unpack(W.chunk_major(W.domain_evaluations(f, log_n), log_n, log_l))
            pis = W.open_chunks_scalars(f, s, log_n, log_l)
            cells += [(p, k, ys[k * l:(k + 1) * l], pis[k]) for k in range(r)]
            commitments.append(W.horner(f, s))
        _wide[(log_n, log_l)] = (cells, commitments, s)
    cells, commitments, s = _wide[(log_n, log_l)]
    return list(cells), list(commitments), s


@pytest.mark.parametrize("log_n,log_l", WIDE)
def test_cells_of_the_closed_forms_are_accepted(log_n, log_l):
    cells, commitments, s = wide(log_n, log_l)
    N = len(cells)
    assert all(VR.cell_holds(c, commitments, s, log_n, log_l) for c in cells)
    order = list(np.random.default_rng(0x0DE).permutation(N))
    assert VR.check([cells[i] for i in order], commitments, s, 0xABCDEF0123, log_n, log_l) == ([VR.OK] * N, 1)


@pytest.mark.parametrize("log_n,log_l", WIDE)
def test_a_coset_moved_in_one_high_bit_is_rejected(log_n, log_l):
    cells, commitments, s = wide(log_n, log_l)
    n, l, r = FK.shape(log_n, log_l)
    for i in (0, 31, 32, r // 2, r - 1, r + 45, 2 * r - 1):
        c, k, ys, pi = cells[i]
        for bit in (32, r // 2):
            assert not VR.cell_holds((c, k ^ bit, ys, pi), commitments, s, log_n, log_l), (i, bit)
    at = r + 33
    c, k, ys, pi = cells[at]
    for bit in (32, r // 2):
        bad = list(cells)
        bad[at] = (c, k ^ bit, ys, pi)
        status, folds = VR.check(bad, commitments, s, 0x5EED, log_n, log_l)
        assert status == [VR.BAD_PROOF if i == at else VR.OK for i in range(len(cells))]
        assert 1 < folds <= 2 * (len(cells) - 1).bit_length() + 1


@pytest.mark.parametrize("log_n,log_l", WIDE)
def test_a_wrong_commitment_blames_exactly_its_cells(log_n, log_l):
    """64 cells, commitment 1's in runs of 8 among commitment 0's: C_1 + G where C_1 belongs fails them all and no other"""
    cells, commitments, s = wide(log_n, log_l)
    n, l, r = FK.shape(log_n, log_l)
    sub = [cells[p * r + 4 * j + t] for j in range(0, 32, 8) for p in (0, 1) for t in range(8)]
    status, folds = VR.check(sub, [commitments[0], (commitments[1] + 1) % R], s, 0xC0FFEE, log_n, log_l)
    assert status == [VR.BAD_PROOF if c[0] == 1 else VR.OK for c in sub] and status.count(VR.BAD_PROOF) == 32
    assert folds <= 2 * 32 * 6 + 1
    assert VR.check(sub, commitments, s, 0xC0FFEE, log_n, log_l) == ([VR.OK] * 64, 1)


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
