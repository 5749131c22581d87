"""tests/srs_check_ref.py, the big-integer statement of typlonk_srs_check / typlonk_srs_contribute, on small SRS -- and the one
piece of the feature that needs no GPU: typlonk_srs_check_challenge against hashlib."""
import numpy as np
import pytest

import srs_check_ref as SR
from helpers import O
from oracle import pairing as PR

R = O.R
S = 0x5EC2E7D00D51
SEEDS = [bytes(32), bytes(range(32)), bytes([0xff] * 32)]
LEN = 9


@pytest.fixture(scope="module")
def srs():
    return O.srs_from_secret_fast(S, LEN)


@pytest.fixture(scope="module")
def g2s():
    return PR.srs_g2(S)[1]


def test_rho_is_the_stated_hash(g2s):
    import hashlib
    import struct

    limbs = SR.g2s_limbs(g2s)
    assert len(limbs) == 24 and limbs[:6] == O.fq_to_mont_limbs(g2s[0][0]) and limbs[18:] == O.fq_to_mont_limbs(g2s[1][1])
    data = b"typlonk/srs/check/v1" + SEEDS[1] + struct.pack("<Q", 130) + np.array(limbs, dtype="<u8").tobytes()
    assert SR.rho(SEEDS[1], 130, g2s) == int.from_bytes(hashlib.blake2b(data, digest_size=64).digest(), "little") % R
    # every input matters
    base = SR.rho(SEEDS[1], 130, g2s)
    assert len({base, SR.rho(SEEDS[0], 130, g2s), SR.rho(SEEDS[1], 131, g2s), SR.rho(SEEDS[1], 130, PR.srs_g2(S + 1)[1])}) == 4


def test_native_challenge_equals_the_python_statement(built, g2s):
    """typlonk_srs_check_challenge (host-only) == rho, three seeds x two lengths"""
    from typlonk_amd.capi import srs_check_challenge

    limbs = np.array(SR.g2s_limbs(g2s), dtype=np.uint64)
    for seed in SEEDS:
        for length in (2, (1 << 20) + 3):
            got = srs_check_challenge(seed, length, limbs)
            assert O.fr_from_mont_limbs([int(x) for x in got]) == SR.rho(seed, length, g2s), (seed, length)


def test_valid_srs(srs, g2s):
    assert SR.first_bad(srs, S) is None
    for seed in SEEDS[:2]:
        assert SR.check(srs, S, seed, g2s) == {"verdict": SR.VALID, "point_class": 0, "index": 0, "bad_points": 0, "folds": 1}
    assert SR.check(srs[:1], S, SEEDS[0], g2s)["folds"] == 0


@pytest.mark.parametrize("j", [1, 4, LEN - 1])
def test_one_bad_link(srs, g2s, j):
    bad = list(srs)
    bad[j] = O.g1_add(bad[j], O.G1)
    assert SR.first_bad(bad, S) == j - 1
    rep = SR.check(bad, S, SEEDS[1], g2s)
    assert (rep["verdict"], rep["index"]) == (SR.BAD_RATIO, j - 1) and rep["folds"] <= 1 + 4   # ceil(log2 9) = 4


def test_what_an_unweighted_sum_misses(srs, g2s):
    swapped = list(srs)
    swapped[2], swapped[6] = swapped[6], swapped[2]
    d = O.g1_mul(O.G1, 77)
    pair = list(srs)
    pair[3], pair[7] = O.g1_add(pair[3], d), O.g1_add(pair[7], O.g1_neg(d))
    for bad, at in ((swapped, 1), (pair, 2)):
        rep = SR.check(bad, S, SEEDS[2], g2s)
        assert (rep["verdict"], rep["index"]) == (SR.BAD_RATIO, at)
    # the compensating pair with ALL weights 1: its four defects -D, [s] D, D, -[s] D sum to the identity
    assert SR.prefix_holds(pair, S, 1, LEN - 1) and not SR.prefix_holds(pair, S, SR.rho(SEEDS[2], LEN, g2s), LEN - 1)


def test_known_seed_lets_defects_cancel(srs, g2s):
    """why the seed must be unknown to whoever made the points"""
    r = SR.rho(SEEDS[1], LEN, g2s)
    j, k, a = 2, 5, 12345
    b = SR.cancelling_pair(S, r, j, k, a)
    bad = list(srs)
    bad[j] = O.g1_add(bad[j], O.g1_mul(O.G1, a))
    bad[k] = O.g1_add(bad[k], O.g1_mul(O.G1, b))
    assert SR.first_bad(bad, S) == j - 1
    assert SR.check(bad, S, SEEDS[1], g2s)["verdict"] == SR.VALID
    rep = SR.check(bad, S, SEEDS[0], g2s)
    assert (rep["verdict"], rep["index"]) == (SR.BAD_RATIO, j - 1)


def test_membership_and_p0(srs, g2s):
    bad = list(srs)
    bad[5] = (0, 2)                                   # order 3
    bad[7] = (bad[7][0], (bad[7][1] + 1) % O.P)        # off the curve
    assert SR.check(bad, S, SEEDS[0], g2s) == {"verdict": SR.BAD_POINT, "point_class": SR.NOT_IN_SUBGROUP, "index": 5,
                                               "bad_points": 2, "folds": 0}
    ident = list(srs)
    ident[4] = None
    rep = SR.check(ident, S, SEEDS[0], g2s)
    assert (rep["verdict"], rep["index"], rep["bad_points"]) == (SR.BAD_RATIO, 3, 0)
    doubled = [O.g1_mul(p, 2) for p in srs]           # consistent, but point 0 is 2G
    assert SR.first_bad(doubled, S) is None
    assert SR.check(doubled, S, SEEDS[0], g2s)["verdict"] == SR.BAD_P0
    # the wrong G2 element: every link is off by (s' - s), the first one included
    rep = SR.check(srs, S + 1, SEEDS[0], PR.srs_g2(S + 1)[1])
    assert (rep["verdict"], rep["index"]) == (SR.BAD_RATIO, 0)


def test_contribution(srs):
    t = 0x7A0_C0FFEE
    new = SR.contribute(srs, t)
    assert new == O.srs_from_secret_fast(S * t % R, LEN)
    assert SR.contribute(srs, 1) == srs
    neg = SR.contribute(srs, R - 1)
    assert all(neg[i] == (srs[i] if i % 2 == 0 else O.g1_neg(srs[i])) for i in range(LEN))
    odd = [None, (0, 2)]
    assert SR.contribute(odd, 5) == [None, O.g1_mul((0, 2), 5 % 3)]
