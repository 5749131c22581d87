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
