"""The general-selector circuits of tests/general_circuits.py on the CPU: every circuit and witness the GPU tests use is the case
they take it for (satisfied, all five selectors live on every row, q_l != q_r, a non-zero public value, a fixed point, a 2-cycle
and a cycle across the three columns), the broken witnesses break exactly one kind of constraint, and the Python provers and the
Python verifier work under cosets (1, k1, k2)."""
import pytest

import compact_ref as CR
import general_circuits as G
import witness_check_ref as W
from oracle import bls12_381 as O
from oracle import pairing as PR
from oracle import plonk_oracle as PO

R = O.R
SECRET = 0x5EC2E7D00D51
MIDS = {3: (1,), 4: (1, 5), 5: (1,), 6: (1,), 12: (2049,)}     # the pi_len of witness 1, per size


@pytest.mark.parametrize("log_n", sorted(G.SEEDS))
def test_circuits_and_witnesses_are_the_cases_the_tests_want(log_n):
    n, cols, q, perm = G.circuit(log_n)
    assert n == 1 << log_n and G.problems(n, cols, q, perm) == []
    sp = G.special_cells(perm, n)
    assert perm[sp["fixed"]] == sp["fixed"]
    x, y = sp["pair"]
    assert x != y and perm[x] == y and perm[y] == x
    assert {c // n for c in sp["spanning"]} == {0, 1, 2}
    for mid in MIDS[log_n]:
        lens = G.pi_lens(log_n, mid)
        assert lens == (0, mid, n, 0, n)
        for (wc, pi), pl in zip(G.witnesses(log_n, mid), lens):
            assert len(pi) == pl and G.problems(n, wc, q, perm, pi) == []
        assert G.witnesses(log_n, mid)[0] == (cols, [])


@pytest.mark.parametrize("log_n", [3, 5, 12])
def test_a_new_witness_under_n_public_values_changes_every_cycle(log_n):
    n, cols, q, perm = G.circuit(log_n)
    a, pa = G.witness(q, perm, cols, 1, n)
    b, pb = G.witness(q, perm, cols, 2, n)
    for wc, pi in ((a, pa), (b, pb)):
        assert W.satisfied(q, perm, wc, pi) and len(pi) == n
        assert all(wc[i] != cols[i] for i in range(3))
        # every cell changed, not one per column
        assert all(wc[i][j] != cols[i][j] for i in range(3) for j in range(n))
    assert all(a[i] != b[i] for i in range(3)) and pa != pb
    # the same seed gives the same witness; pi_len = 0 gives the circuit's own back
    assert G.witness(q, perm, cols, 1, n) == (a, pa)
    assert G.witness(q, perm, cols, 1, 0) == (cols, [])
    # in between: only cycles wholly in the first rows change, and the rows from pi_len on need no public value
    half, ph = G.witness(q, perm, cols, 3, n // 2)
    assert W.satisfied(q, perm, half, ph) and len(ph) == n // 2
    assert all(half[i][j] == cols[i][j] for i in range(3) for j in range(n // 2, n))


@pytest.mark.parametrize("log_n", [3, 4, 5, 12])
def test_broken_witnesses_break_one_kind_of_constraint(log_n):
    n, cols, q, perm = G.circuit(log_n)
    for wc, pi in G.witnesses(log_n, MIDS[log_n][0]):
        bad, row = G.break_gate_only(perm, wc)
        assert W.check(q, perm, bad, pi) == ([row], [])
    wc, pi = G.witnesses(log_n, MIDS[log_n][0])[2]
    bad, bad_pi, pairs = G.break_copy_only(q, perm, wc, pi)
    assert W.check(q, perm, bad, bad_pi) == ([], pairs) and len(pairs) == 2
    assert sum(x != y for x, y in zip(pi, bad_pi)) == 1


def test_python_provers_and_verifier_under_cosets_1_k1_k2():
    log_n = 3
    n, cols, q, perm = G.circuit(log_n)
    ks = G.large_cosets(log_n)
    assert ks[0] == 1 and all(k.bit_length() == 254 and k < R for k in ks[1:]) and G.cosets_are_disjoint(ks, n)
    assert not G.cosets_are_disjoint((1, O.domain_root(log_n), 5), n)
    srs = O.srs_from_secret_fast(SECRET, n + 3)
    wc, pi = G.witnesses(log_n)[2]
    circ = CR.setup(log_n, q, perm, srs, PR.srs_g2(SECRET)[1], cosets=ks)
    assert circ["vk"]["cosets"] == list(ks)
    pf = CR.prove(circ, wc, pi)
    assert pf["r_zeta"] == 0
    assert CR.verify_one(circ["vk"], pf, pi)
    assert not CR.verify_one(circ["vk"], pf, [(pi[0] + 1) % R] + pi[1:])
    # the same witness proved under the default cosets against that key: the permutation argument no longer closes
    assert CR.prove(circ, wc, pi, cosets=PO.COSETS)["r_zeta"] != 0
    # the reference shape
    ch, zeta = (0x1234567DEADBEEF, 0xABCDEF0123456789ABCDEF, 0x55AA55AA77), 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0
    ref = PO.prove(log_n, wc, q, perm, G.full_column(pi, n), ch, zeta, lambda c: O.kzg_commit(srs, c), cosets=ks)
    assert ref["rem"] == [] and ref["r_open"][1] == 0
    ids, sig = PO.compile_permutation(perm, n, log_n, ks)
    assert ids[0][1] == O.domain_root(log_n) and ids[2][0] == ks[2]
    assert PO.grand_product(wc, ids, sig, ch[1], ch[2], n, ks)[n] == 1
    # the defaults are the module constant
    assert PO.compile_permutation(perm, n, log_n) == PO.compile_permutation(perm, n, log_n, PO.COSETS)


def test_general_circuit_proves_and_a_changed_cell_does_not():
    """the Python compact prover on the 2^3 circuit: r(zeta) = 0 for each kind of witness, != 0 for the broken ones"""
    log_n = 3
    n, cols, q, perm = G.circuit(log_n)
    srs = O.srs_from_secret_fast(SECRET, n + 3)
    circ = CR.setup(log_n, q, perm, srs, PR.srs_g2(SECRET)[1])
    assert circ["vk"]["cosets"] == list(PO.COSETS)
    wc, pi = G.witnesses(log_n)[1]
    assert CR.prove(circ, wc, pi)["r_zeta"] == 0
    bad, _ = G.break_gate_only(perm, wc)
    assert CR.prove(circ, bad, pi)["r_zeta"] != 0
    wc, pi = G.witnesses(log_n)[2]
    bad, bad_pi, _ = G.break_copy_only(q, perm, wc, pi)
    assert CR.prove(circ, bad, bad_pi)["r_zeta"] != 0
