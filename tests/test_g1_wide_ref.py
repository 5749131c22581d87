"""tests/g1_wide_ref.py without a GPU: the O(n log n) closed forms equal the quadratic big-integer references they stand in for
at every shape those reach in reasonable time, and `combination_check` accepts records made by the C oracle and rejects each
way a record can be wrong -- wrong group element (altered, swapped, negated, set to the identity) or right element in wrong
words (a coordinate plus p, the identity flag on a point's record)."""
import numpy as np
import pytest

import g1_wide_ref as W
import open_all_ref as FA
import open_chunks_ref as FK
from helpers import O, fr_pack
from oracle import coracle as CO

R, P = O.R, O.P


def _rand(rng, k):
    return [int.from_bytes(rng.bytes(32), "little") % R for _ in range(k)]


# ---- limbs and scalars ------------------------------------------------------------------------------------------------------
def test_pack_is_fr_pack():
    vals = _rand(np.random.default_rng(0x9AC), 9) + [0, 1, R - 1]
    assert (W.pack(vals) == fr_pack(vals)).all() and W.pack(vals).dtype == np.uint64
    assert W.unpack(W.pack(vals)) == vals


def test_batch_inverse_and_powers():
    xs = _rand(np.random.default_rng(0xB17), 33)
    assert W.batch_inverse(xs) == [pow(x, -1, R) for x in xs]
    assert W.powers(xs[0], 70) == [pow(xs[0], j, R) for j in range(70)]
    with pytest.raises(AssertionError):
        W.batch_inverse([3, 0, 5])


# ---- the closed forms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", range(7))
def test_lagrange_closed_form(log_n):
    """L_i(s) is the inverse transform of the powers of s"""
    n = 1 << log_n
    s = _rand(np.random.default_rng(0x1A7 + log_n), 1)[0]
    assert W.lagrange_scalars(s, log_n) == O.ntt(W.powers(s, n), log_n, inverse=True)


def test_closed_forms_refuse_a_secret_in_the_domain():
    s = pow(O.domain_root(4), 5, R)
    for call in (lambda: W.lagrange_scalars(s, 4), lambda: W.open_all_scalars([1, 2, 3], s, 4),
                 lambda: W.open_chunks_scalars([1, 2, 3], s, 4, 2)):
        with pytest.raises(AssertionError):
            call()


@pytest.mark.parametrize("log_n", range(1, 7))
def test_open_all_closed_form(log_n):
    """q_k(s) by synthetic division, at m = n and at m < n"""
    n = 1 << log_n
    rng = np.random.default_rng(0xF21 + log_n)
    s = _rand(rng, 1)[0]
    for m in sorted({n, max(n - 3, 1), n // 2 + 1}):
        f = _rand(rng, m)
        assert W.open_all_scalars(f, s, log_n) == FA.openings_known_secret(f, s, log_n), m
        assert W.unpack(W.domain_evaluations(f, log_n)) == FA.evaluations(f, log_n), m


@pytest.mark.parametrize("log_n,log_l", [(a, b) for a in range(1, 7) for b in range(a)])
def test_open_chunks_closed_form(log_n, log_l):
    """q_k(s) by schoolbook division by X^l - a_k, at m = n and at m < n; the chunk-major order of the evaluations"""
    n, l, r = FK.shape(log_n, log_l)
    rng = np.random.default_rng(0xC21 + 16 * log_n + log_l)
    s = _rand(rng, 1)[0]
    for m in sorted({n, max(n - 3, 1), n // 2 + 1}):
        f = _rand(rng, m)
        assert W.open_chunks_scalars(f, s, log_n, log_l) == FK.openings_known_secret(f, s, log_n, log_l), m
        ev = W.domain_evaluations(f, log_n)
        want = FK.evaluations(f, log_n, log_l)
        assert W.unpack(W.chunk_major(ev, log_n, log_l)) == want, m
        assert W.chunk_major(W.unpack(ev), log_n, log_l) == want, m
    if log_l == 0:
        assert W.open_chunks_scalars(f, s, log_n, 0) == W.open_all_scalars(f, s, log_n)


# ---- the sample -------------------------------------------------------------------------------------------------------------
def test_sample_indices():
    for n in (1, 2, 5, 64, 200, 1 << 14, 1 << 16):
        got = W.sample_indices(n, 7)
        assert got == sorted(set(got)) and all(0 <= i < n for i in got)
        assert len(got) == min(64, n)
        top = 1 << (n - 1).bit_length() - 1 if n > 1 else 1           # the largest power of two below n
        for i in (0, 1, 2, n - 3, n - 2, n - 1, 63, 64, 65, top - 1, top, top + 1):
            assert i in got or not 0 <= i < n, (n, i)
        assert got == W.sample_indices(n, 7)
    assert W.sample_indices(1 << 14, 7) != W.sample_indices(1 << 14, 8)


# ---- the checker ------------------------------------------------------------------------------------------------------------
N = 200
SEED = 0x51D


@pytest.fixture(scope="module")
def records():
    """[e_i] G from the C oracle for N full-width scalars, one of them 0 (an identity that belongs there)"""
    e = _rand(np.random.default_rng(0xEC0), N)
    e[7] = 0
    xy = np.zeros((N, 12), dtype=np.uint64)
    inf = np.zeros(N, dtype=np.uint8)
    for i, v in enumerate(e):
        xy[i], inf[i] = CO.g1_mul_generator(W.pack([v])[0])
    assert inf[7] == 1 and inf.sum() == 1
    xy.setflags(write=False)
    inf.setflags(write=False)
    return xy, inf, e


def _unsampled():
    """two indices the 64-record sample does not hold: only the combination can catch them"""
    held = set(W.sample_indices(N, SEED))
    out = [i for i in range(20, N - 20) if i not in held and i + 1 not in held]
    assert out
    return out[0], out[0] + 1


def _coord(words):
    return sum(int(v) << (64 * k) for k, v in enumerate(words))


def _words(v):
    return [(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(6)]


def test_the_checker_accepts_the_oracles_records(records):
    xy, inf, e = records
    W.combination_check(xy, inf, e, SEED)
    W.combination_check(xy[:1], inf[:1], e[:1], SEED)
    W.combination_check(xy[5:9], inf[5:9], e[5:9], SEED + 1)          # the identity among them
    assert W.non_canonical(xy, inf) == []


@pytest.mark.parametrize("where", ["sampled", "unsampled"])
@pytest.mark.parametrize("change", ["altered", "swapped", "negated", "identity", "plus_p", "flagged"])
def test_the_checker_rejects(records, change, where):
    """each change at an index of the sample (the failure names it) and at one only the combination or the canonical-form check
    sees"""
    xy0, inf0, e = records
    xy, inf = xy0.copy(), inf0.copy()
    i, j = (64, 65) if where == "sampled" else _unsampled()
    assert (i in W.sample_indices(N, SEED)) == (where == "sampled")
    if change == "altered":                                            # its neighbour's record: a point of the group, the wrong one
        xy[i] = xy0[j]
    elif change == "swapped":
        xy[i], xy[j] = xy0[j], xy0[i]
    elif change == "negated":                                          # (p - y in Montgomery form is the negative's residue)
        xy[i, 6:] = _words(P - _coord(xy0[i, 6:]))
    elif change == "identity":
        xy[i], inf[i] = W.IDENTITY_XY, 1
    elif change == "plus_p":                                           # the same point, in words no canonical form has
        xy[i, :6] = _words(_coord(xy0[i, :6]) + P)
    elif change == "flagged":                                          # the flag alone, on a point's record
        inf[i] = 1
    with pytest.raises(AssertionError) as err:
        W.combination_check(xy, inf, e, SEED)
    text = str(err.value)
    if change in ("plus_p", "flagged"):
        assert "canonical" in text and f"index {i}" in text
        assert W.non_canonical(xy, inf) == [i]
    elif where == "sampled":
        assert f"record {i} " in text
    else:
        assert "outside the sample" in text


def test_the_checker_rejects_the_identitys_record_without_its_flag(records):
    xy0, inf0, e = records
    inf = inf0.copy()
    inf[7] = 0
    with pytest.raises(AssertionError, match="canonical"):
        W.combination_check(xy0, inf, e, SEED)
    inf[7] = 2                                                         # a flag that is neither 0 nor 1
    with pytest.raises(AssertionError, match="canonical"):
        W.combination_check(xy0, inf, e, SEED)


def test_the_checker_rejects_a_wrong_scalar(records):
    """the other side: right records, one reference scalar off by one"""
    xy, inf, e = records
    e = list(e)
    e[_unsampled()[0]] += 1
    with pytest.raises(AssertionError, match="outside the sample"):
        W.combination_check(xy, inf, e, SEED)
