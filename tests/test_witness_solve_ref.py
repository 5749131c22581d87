"""tests/witness_solve_ref.py, the Python statement of typlonk_witness_solve, against the witness checker's
(tests/witness_check_ref.py): what it solves satisfies the circuit exactly where the contract says it must -- everywhere on an
honest witness, everywhere but the unequal tied pairs on a circuit that has them, and not at the undriven rows once the inputs
change, which solve does not enforce.  The README inputs [3, 4, 5] give the columns builder.rs would push.  The entries that
solve many witnesses of one circuit at once (solve_many here and in tests/witness_hints_ref.py) give what the one-witness
statements give, and the circuit H.hint_wall builds is the three wide levels it says.  No GPU."""
import pytest

import witness_check_ref as W
import witness_solve_ref as S
from oracle import frontend as F

R = W.R
WIDTHS = [3, 1, 9, 4, 12]


@pytest.mark.parametrize("log_n,pi_len", [(3, 0), (4, 1), (6, 64), (10, 0)])
def test_the_chain_is_solved_from_one_input(log_n, pi_len):
    n = 1 << log_n
    pi = S.public_values(n, pi_len, log_n)
    n, q, perm, assigned, cols = S.chain(log_n, pi)
    got = S.solve(q, perm, assigned, pi)
    assert got == cols and W.check(q, perm, got, pi) == ([], [])
    p = S.plan(q, perm)
    assert (p["driven_rows"], p["depth"], p["launches"]) == (n - 3, n - 3, 2)
    assert p["free_classes"] == 1 + 9 and p["schedule"] == [[0, n - 3, 0]]


@pytest.mark.parametrize("pi_len", [0, 1, 64])
def test_a_layered_circuit_fails_exactly_at_its_unequal_ties(pi_len):
    pi = S.public_values(64, pi_len, 5)
    c = S.layered(6, 1, WIDTHS, pi)
    n, q, perm, cols = c["n"], c["q"], c["perm"], c["cols"]
    assert S.solve(q, perm, c["assigned"], pi) == cols
    p = S.plan(q, perm)
    assert p["level"] == c["level"] and p["depth"] == len(WIDTHS)
    assert [p["level_off"][k + 1] - p["level_off"][k] for k in range(p["depth"])] == WIDTHS
    gate, copy = W.check(q, perm, cols, pi)
    assert gate == []
    # the copy constraints that fail run between cells of the classes that hold two different computed values, and each of
    # those classes fails somewhere
    assert copy and {x for pair in copy for x in pair} <= set(c["unequal"])
    classes = [set(cyc) for cyc in W.cycles_of(perm) if cyc[0] in c["unequal"]]
    assert len(classes) == 2 and all(any(x in cl for x, _ in copy) for cl in classes)
    # the non-driver's c cell keeps its own row's value; every other cell of the class has the driver's
    for cl in classes:
        drivers = sorted(x - 2 * n for x in cl if x >= 2 * n and q["q_o"][x - 2 * n])
        assert len(drivers) == 2
        own = [cols[2][j] for j in drivers]
        assert own[0] != own[1]
        assert all(cols[x // n][x % n] == own[0] for x in cl if x != 2 * n + drivers[1])
    # without unequal ties the whole witness is honest
    c = S.layered(6, 2, WIDTHS, pi, ties=(3, 0))
    assert c["unequal"] == [] and W.check(c["q"], c["perm"], c["cols"], pi) == ([], [])


def test_unassigned_free_classes_read_zero_and_blinding_cells_are_assigned():
    c = S.layered(6, 3, WIDTHS)
    n, cols = c["n"], c["cols"]
    for x, v in S.blinding_cells(n).items():
        assert cols[x // n][x % n] == v
    src, free = S.sources(c["q"], c["perm"])
    assigned_slots = {src[x] for x in c["assigned"]}
    zero = [x for x in range(3 * n) if src[x] & S.FREE and src[x] not in assigned_slots]
    assert zero and all(cols[x // n][x % n] == 0 for x in zero)
    assert any(x % n < n - 3 and x < 2 * n for x in zero)             # the input that is never assigned, at an operand cell


def test_undriven_rows_are_not_enforced_once_the_inputs_change():
    c = S.layered(6, 4, WIDTHS, ties=(2, 0))
    q, perm = c["q"], c["perm"]
    assert W.check(q, perm, c["cols"]) == ([], [])
    other = dict(c["assigned"])
    x = min(x for x in other if x % c["n"] < c["n"] - 3)
    other[x] = (other[x] + 1) % R
    cols = S.solve(q, perm, other)
    gate, copy = W.check(q, perm, cols)
    assert copy == [] and gate and set(gate) <= set(c["undriven"])    # every driven row and every copy constraint still holds


def test_the_readme_inputs_give_the_columns_the_builder_pushes():
    n, q, perm, cells, run = S.readme()
    assert n == 8
    adv = F.witness(run, [3, 4, 5])
    bl = S.blinding_cells(n)
    want = [list(col) + [0] * (n - 3 - len(col)) + [bl[i * n + n - 3 + k] for k in range(3)] for i, col in enumerate(adv)]
    got = S.solve(q, perm, {**dict(zip(cells, [3, 4, 5])), **bl})
    assert got == want and W.check(q, perm, got) == ([], [])
    # 9 + 16 != 36: the two computed values tied by assert_eq both stand, and the check names the copy constraint
    got = S.solve(q, perm, {**dict(zip(cells, [3, 4, 6])), **bl})
    assert got[2][:4] == [9, 16, 36, 25]
    assert W.check(q, perm, got) == ([], [(2 * n + 2, 2 * n + 3), (2 * n + 3, 2 * n + 2)])
    with pytest.raises(ValueError):
        S.solve(q, perm, {3: 9})                                       # a_3 is c_0's copy: computed, not assignable


def _other_inputs(assigned, n, k):
    return {x: (v * (k + 1) + k) % R if x % n < n - 3 else v for x, v in assigned.items()}


@pytest.mark.parametrize("log_n,widths,ties", [(4, [3, 2, 4], (1, 1)), (6, WIDTHS, (2, 2)), (9, [120, 257, 100, 32], (2, 2)),
                                               (9, [100, 257, 3, 120], (0, 3))])
def test_many_witnesses_of_one_circuit_are_solved_as_one_by_one(log_n, widths, ties):
    """solve_many shares the per-circuit work; every witness is what solve says, with and without public values"""
    n = 1 << log_n
    c = S.layered(log_n, 50 + log_n, widths, ties=ties)
    q, perm = c["q"], c["perm"]
    wits = [(c["assigned"], [])]
    for k, pl in enumerate((1, n, 0, n // 2, n)):
        wits.append((_other_inputs(c["assigned"], n, k + 1), S.public_values(n, pl, 90 + k)))
    got = S.solve_many(q, perm, wits)
    assert got[0] == c["cols"] and got == [S.solve(q, perm, a, pi) for a, pi in wits]
    assert len({str(cols) for cols in got}) == len(wits)               # no witness is another's
    n, q, perm, assigned, cols = S.chain(5, S.public_values(32, 32, 5))
    assert S.solve_many(q, perm, [(assigned, S.public_values(32, 32, 5)), (assigned, [])]) == [cols, S.solve(q, perm, assigned)]
    with pytest.raises(ValueError):
        S.solve_many(q, perm, [({2 * n: 1}, [])])                      # c_0 is computed


def test_many_hinted_witnesses_are_solved_as_one_by_one():
    import witness_hints_ref as H

    for L in (H.stacked(9, 8, [(60, 2), (200, 100), (60, 2)]), H.stacked(6, 9, [(5, 2), (6, 3), (20, 7), (5, 2)])):
        n, q, perm, hints = L["n"], L["q"], L["perm"], L["hints"]
        quiet = [j for j in range(n) if not q["q_o"][j]]
        wits = [(L["assigned"], [])] + [(_other_inputs(L["assigned"], n, k + 1), S.public_values(n, pl, 20 + k, zero_rows=quiet))
                                        for k, pl in enumerate((n, 1, n // 2))]
        got = H.solve_many(q, perm, hints, wits)
        assert got == [H.solve(q, perm, hints, a, pi) for a, pi in wits] and len({str(cols) for cols in got}) == len(wits)
        assert all(W.check(q, perm, cols, pi) == ([], []) for cols, (_, pi) in zip(got, wits))
    n, q, perm, hints, (cx, cy) = H.range_check(5, 8)
    wits = [({cx: x, cy: y}, []) for x, y in H.RANGE_PAIRS(8)]
    assert H.solve_many(q, perm, hints, wits) == [H.solve(q, perm, hints, a) for a, _ in wits]
    assert H.solve_many(q, perm, [], wits) == S.solve_many(q, perm, wits)
    with pytest.raises(ValueError):
        H.solve_many(q, perm, hints, [({1: 1}, [])])                   # a_1 is bit 0: hinted


def test_the_wall_of_hints_is_three_wide_levels():
    """H.hint_wall: 1000 rows, then 37 rows + 3041 hints of their outputs, then 300 rows over hint values; under the last set of
    inputs the source of one INV0 hint is 0; every set of inputs gives an honest witness"""
    import witness_hints_ref as H

    L = H.hint_wall(13, 3000)
    n, q, perm, hints = L["n"], L["q"], L["perm"], L["hints"]
    p = H.plan(q, perm, hints)
    assert p["schedule"] == [[0, 1, 1], [1, 1, 1], [2, 1, 1]]
    assert [p["level_off"][k + 1] - p["level_off"][k] for k in range(3)] == [1000, 37 + 3041, 300]
    assert set(p["hint_level"]) == {2} and [t[0] for t in hints[1000:1260]] == [H.INV0] * 130 + [H.BITS] * 130
    assert 100 < sum(t[0] == H.INV0 for t in hints[1260:]) < len(hints) - 1260 - 100
    wits = [(a, []) for a in L["assigned"]]
    got = H.solve_many(q, perm, hints, wits)
    assert got[1] == H.solve(q, perm, hints, L["assigned"][1])
    assert all(W.check(q, perm, cols) == ([], []) for cols in got)
    zero = hints[L["zero_hint"]]
    assert zero[:1] + zero[2:] == (H.INV0, 2 * n + L["zero_row"], 0, 0)
    assert [cols[2][L["zero_row"]] == 0 for cols in got] == [False, False, True]
    for cols in got:                                                   # every hinted cell holds the hint's value
        assert all(cols[0][t[1]] == H.hint_value(t[0], cols[2][t[2] - 2 * n], t[3], t[4]) for t in hints)


def test_cycles_are_refused_with_the_lowest_row_named():
    n = 8
    q = {name: [0] * n for name in W.SELECTORS}
    for j in (2, 5, 6):
        q["q_o"][j] = q["q_l"][j] = 1
    perm = list(range(3 * n))
    perm[2 * n + 2], perm[5] = 5, 2 * n + 2          # a_5 = c_2
    perm[2 * n + 5], perm[2] = 2, 2 * n + 5          # a_2 = c_5: rows 2 and 5 wait for each other
    perm[2 * n + 2], perm[5], perm[n + 6] = 5, n + 6, 2 * n + 2   # b_6 = c_2 too: row 6 depends on the cycle
    with pytest.raises(S.Unsolvable) as e:
        S.levels(q, perm)
    assert e.value.row == 2 and S.plan(q, perm) == {"status": 2, "bad": 2}
    q["q_o"][2] = q["q_o"][5] = 0                    # undriven rows wait for nothing: row 6 reads a free class
    assert S.levels(q, perm) == [0, 0, 0, 0, 0, 0, 1, 0]
    self_dep = list(range(3 * n))
    self_dep[2 * n + 6], self_dep[6] = 6, 2 * n + 6  # a_6 = c_6
    with pytest.raises(S.Unsolvable) as e:
        S.levels(q, self_dep)
    assert e.value.row == 6
