"""tests/witness_check_ref.py pinned against oracle/plonk_oracle.py: at log_n 3 and 4 the checker says "satisfied" exactly when
the quotient's remainder is zero -- honest witnesses, and every single-cell corruption (log_n 3) or a spread of them (log_n 4)."""
import pytest

import witness_check_ref as W
from oracle import bls12_381 as O
from oracle import plonk_oracle as PO

R = O.R
CHALLENGES = (0x1234567, 0x89ABCDE, 0xF00DF00D)   # alpha, beta, gamma
ZETA = 0x5EED5EED


def _rem(log_n, cols, q, perm, pi):
    n = 1 << log_n
    pi_evals = list(pi) + [0] * (n - len(pi))
    return PO.prove(log_n, cols, q, perm, pi_evals, CHALLENGES, ZETA, commit=lambda coeffs: None)["rem"]


def _circuits():
    yield "chain3", 3, W.chain_with_pi(3)[1:], ()
    yield "chain3_pi", 3, W.chain_with_pi(3, (5, 0, 9))[1:], (5, 0, 9)
    log_n, cols, q, perm = PO.pythagorean_circuit([3, 4, 5])
    yield "readme", log_n, (cols, q, perm), ()
    yield "chain4", 4, W.chain_with_pi(4, (7,))[1:], (7,)


@pytest.mark.parametrize("name,log_n,tables,pi", list(_circuits()), ids=[c[0] for c in _circuits()])
def test_checker_agrees_with_the_quotient_remainder(name, log_n, tables, pi):
    cols, q, perm = tables
    n = 1 << log_n
    assert W.check(q, perm, cols, pi) == ([], []) and _rem(log_n, cols, q, perm, pi) == []
    cells = range(3 * n) if log_n == 3 else range(0, 3 * n, 5)
    seen = set()
    for x in cells:
        bad = [list(c) for c in cols]
        bad[x // n][x % n] = (bad[x // n][x % n] + 1) % R
        ok = W.satisfied(q, perm, bad, pi)
        assert ok == (_rem(log_n, bad, q, perm, pi) == []), (name, x)
        seen.add(ok)
    assert seen == {True, False}        # blinding rows and unconstrained cells stay satisfied, gate cells do not
    # a wrong public value
    if pi:
        wrong = (pi[0] + 1,) + tuple(pi[1:])
        assert not W.satisfied(q, perm, cols, wrong) and _rem(log_n, cols, q, perm, wrong) != []


def test_checker_lists_rows_and_cells_in_ascending_order_and_reads_residues():
    n, cols, q, perm = W.chain_with_pi(4)
    bad = [list(c) for c in cols]
    bad[2][5] += 1                      # c_5: gate row 5, and the cycle (c_5 a_6 b_6)
    gate, copy = W.check(q, perm, bad)
    assert gate == [5] and copy == [(n + 6, 2 * n + 5), (2 * n + 5, 6)]       # b_6 -> c_5 and c_5 -> a_6; a_6 -> b_6 still holds
    shifted = [[v + R for v in c] for c in cols]       # v + r is v
    assert W.check(q, perm, shifted) == ([], [])


# ---- random circuits and the raw-word view ---------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,pi_len", [(4, 16), (9, 37), (13, 1)])
def test_random_circuits_are_honest_and_their_cycles_mixed(log_n, pi_len):
    n, cols, q, perm, pi = W.random_circuit(log_n, 40 + log_n, pi_len)
    assert n == 1 << log_n and len(pi) == pi_len and sorted(perm) == list(range(3 * n))
    assert W.check(q, perm, cols, pi) == ([], [])
    assert all(0 <= v < R for name in W.SELECTORS for v in q[name]) and all(len(q[name]) == n for name in W.SELECTORS)
    lengths = [len(c) for c in W.cycles_of(perm)]
    assert 1 in lengths and 2 in lengths and max(lengths) >= min(3 * n // 4, 200)
    assert any(len({x // n for x in c}) == 3 for c in W.cycles_of(perm))           # cycles cross the columns
    if log_n >= 9:
        # full-range selectors: no column is small, sparse or 0 / 1
        assert all(min(q[name]) > 0 and max(q[name]) >> 250 for name in W.SELECTORS)
    # another seed, another circuit; the same seed, the same one
    assert W.random_circuit(log_n, 40 + log_n, pi_len) == (n, cols, q, perm, pi)
    assert W.random_circuit(log_n, 41 + log_n, pi_len)[3] != perm
    with pytest.raises(ValueError):
        W.random_circuit(log_n, 1, n + 1)


@pytest.mark.parametrize("log_n", [4, 9])
def test_one_bumped_cell_fails_its_two_copy_pairs_or_none(log_n):
    n, cols, q, perm, pi = W.random_circuit(log_n, 50 + log_n, 3)
    pred = {y: x for x, y in enumerate(perm)}
    seen = set()
    for cyc in W.cycles_of(perm):
        x = cyc[len(cyc) // 2]
        bad = [list(c) for c in cols]
        bad[x // n][x % n] = (bad[x // n][x % n] + 1) % R
        gate, copy = W.check(q, perm, bad, pi)
        assert gate == [x % n]                                  # q_l, q_r, q_o are non-zero (full range): the row's gate fails too
        assert copy == ([] if len(cyc) == 1 else sorted({(pred[x], x), (x, perm[x])}))
        seen.add(min(len(cyc), 3))
    assert seen == {1, 2, 3}


def test_raw_words_agree_with_fr_pack_and_round_trip():
    import numpy as np
    from helpers import fr_pack, fr_unpack

    vals = [0, 1, R - 1, R, R + 5, 2**255, 0x123456789ABCDEF << 190] + O.random_frs(9, 20)
    assert np.array_equal(W.mont_words(vals), fr_pack([v % R for v in vals]))
    raw = [0, 1, R - 1, R, 2 * R + 1, 2**256 - 1, 2**255, (1 << 64) - 1, 1 << 64, 1 << 192]
    words = W.raw_words(raw)
    assert words.dtype == np.uint64 and words.shape == (len(raw), 4)
    assert [[int(w) for w in row] for row in words] == [[(x >> (64 * i)) & (2**64 - 1) for i in range(4)] for x in raw]
    assert W.words_raw(words).tolist() == raw
    assert W.residues_of(raw).tolist() == fr_unpack(words)       # the oracle's reading of the same words
    assert W.residues_of(W.raw_of(vals)).tolist() == [v % R for v in vals]


def test_the_raw_word_path_agrees_with_check_on_residues():
    n, cols, q, perm, pi = W.random_circuit(6, 66, 5)
    raw = [W.raw_of(c) for c in cols]
    raw_pi = W.raw_of(pi)
    assert W.check_raw(q, perm, raw, raw_pi) == ([], [])
    # v + r and v + 2r (where it fits the 256 bits) are v
    shifted = [c + R for c in raw]
    assert all(v < 1 << 256 for c in shifted for v in c)
    assert W.check_raw(q, perm, shifted, raw_pi + R) == ([], [])
    twice = [W._obj([v + 2 * R if v + 2 * R < 1 << 256 else v for v in c]) for c in raw]
    assert sum(int(v >= 2 * R) for c in twice for v in c) > n // 4          # 2^256 - 2r = 0.21 r: about a fifth of the cells
    assert W.check_raw(q, perm, twice, raw_pi) == ([], [])
    # a corruption of the raw word is the same corruption of the residue it stands for
    bad_raw = [c.copy() for c in shifted]
    bad_raw[1][7] += 1
    bad = [list(c) for c in cols]
    bad[1][7] = (bad[1][7] + W.MONT_INV) % R                     # raw + 1 stands for v + 2^-256
    exp = W.check(q, perm, bad, pi)
    assert exp[0] == [7] and W.check_raw(q, perm, bad_raw, raw_pi + R) == exp
