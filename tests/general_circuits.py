"""Circuits with general selectors for the prover and verifier tests (TEST INFRASTRUCTURE ONLY), built on
witness_check_ref.random_circuit: all five selectors uniform in [0, r) on every row, an arbitrary permutation, public values.
The squaring chain and the README circuit leave q_l, q_r and q_c zero (or q_l = q_r), so that a prover or verifier that swaps
two of them, or drops q_c, returns on those circuits what a correct one returns.  Here every gate term is live on every row.

A circuit is made with no public values of its own (q_c closes every gate row at PI = 0); witness() then makes further
witnesses of it, each under public values of its own on the first pi_len rows.  Cells are flat indices col * n + row."""
import functools
import random

import witness_check_ref as W

R = W.R

# log_n -> seed of the circuit the tests use: the first seed from 700 + log_n on for which problems() is empty for the circuit
# and for each of its witnesses() and, below 2^12, a cycle lies wholly in row 0 (so that pi_len = 1 changes the witness and its
# one public value is not zero)
SEEDS = {3: 719, 4: 706, 5: 711, 6: 754, 12: 712}
# the public-input lengths of the five witnesses of one circuit: one group of four with neighbours that differ in whether they
# have public values at all, and one proof alone in a second group (witness 3 is witness 0 again: a circuit with a fixed q_c has
# one witness under no public values)
WITNESS_SEEDS = (0, 11, 22, 0, 44)


def pi_lens(log_n, mid=1):
    n = 1 << log_n
    return (0, mid, n, 0, n)


@functools.lru_cache(maxsize=None)
def circuit(log_n, seed=None):
    """(n, cols, q, perm) of the circuit of SEEDS[log_n] (or of `seed`), made with no public values: cols is its own witness"""
    n, cols, q, perm, pi = W.random_circuit(log_n, SEEDS[log_n] if seed is None else seed, 0)
    assert pi == []
    return n, cols, q, perm


def special_cells(perm, n):
    """{"fixed": a cell that is its own successor, "pair": the two cells of a 2-cycle, "spanning": a cycle with cells in all
    three columns, "row0": a cycle that lies wholly in row 0}, each the lowest of its kind, None where there is none"""
    out = {"fixed": None, "pair": None, "spanning": None, "row0": None}
    for cyc in W.cycles_of(perm):
        if len(cyc) == 1 and out["fixed"] is None:
            out["fixed"] = cyc[0]
        if len(cyc) == 2 and out["pair"] is None:
            out["pair"] = (cyc[0], cyc[1])
        if {x // n for x in cyc} == {0, 1, 2} and out["spanning"] is None:
            out["spanning"] = cyc
        if all(x % n == 0 for x in cyc) and out["row0"] is None:
            out["row0"] = cyc
    return out


def problems(n, cols, q, perm, pi=(), pi_len=None):
    """what keeps (cols, q, perm, pi) from being a case the tests want, as a list of strings (empty: nothing does)"""
    out = []
    if not W.satisfied(q, perm, cols, pi):
        out.append("the witness does not satisfy the circuit")
    for j in range(n):
        if not all(q[name][j] % R for name in W.SELECTORS):
            out.append(f"a zero selector on row {j}")
        if (q["q_l"][j] - q["q_r"][j]) % R == 0:
            out.append(f"q_l = q_r on row {j}")
    if (len(pi) if pi_len is None else pi_len) > 0 and not any(v % R for v in pi):
        out.append("every public value is zero")
    sp = special_cells(perm, n)
    out += [f"no {kind} cycle" for kind in ("fixed", "pair", "spanning") if sp[kind] is None]
    return out


def witness(q, perm, cols, seed, pi_len):
    """Another witness of the circuit (q, perm), from the witness `cols` that satisfies it under no public values: every
    permutation cycle that lies wholly in rows < pi_len holds a fresh residue, the other cycles keep theirs, and
    pi_j = -(q_l a + q_r b - q_o c + q_m a b + q_c) on rows < pi_len.  With pi_len = n every cycle changes; with pi_len = 0 the
    witness is `cols` again.  Returns (cols, pi)."""
    n = len(cols[0])
    rng = random.Random(seed)
    flat = list(cols[0]) + list(cols[1]) + list(cols[2])
    for cyc in W.cycles_of(perm):
        if all(x % n < pi_len for x in cyc):
            v = rng.randrange(R)
            for x in cyc:
                flat[x] = v
    new = [flat[:n], flat[n:2 * n], flat[2 * n:]]
    return new, [public_value(q, new, j) for j in range(pi_len)]


def public_value(q, cols, j):
    """the public value that closes gate row j"""
    a, b, c = cols[0][j], cols[1][j], cols[2][j]
    return -(q["q_l"][j] * a + q["q_r"][j] * b - q["q_o"][j] * c + q["q_m"][j] * a * b + q["q_c"][j]) % R


@functools.lru_cache(maxsize=None)
def witnesses(log_n, mid=1):
    """the five witnesses [(cols, pi)] of circuit(log_n) under pi_lens(log_n, mid)"""
    _, cols, q, perm = circuit(log_n)
    return [witness(q, perm, cols, 1000 * log_n + s, pl) for s, pl in zip(WITNESS_SEEDS, pi_lens(log_n, mid))]


def full_column(pi, n):
    """the reference shape's public-input column: n evaluations"""
    return list(pi) + [0] * (n - len(pi))


# ---- broken witnesses ----------------------------------------------------------------------------------------------------
def break_gate_only(perm, cols):
    """the value of a fixed-point cell changed: its gate row fails, no copy constraint does.  Returns (cols, the row)."""
    n = len(cols[0])
    x = special_cells(perm, n)["fixed"]
    new = [list(c) for c in cols]
    new[x // n][x % n] = (new[x // n][x % n] + 1) % R
    return new, x % n


def break_copy_only(q, perm, cols, pi):
    """one cell of the 2-cycle changed and its row's public value recomputed (pi_len = n): no gate row fails, the two copy
    constraints of the pair do.  Returns (cols, pi, the failing (x, perm[x]) pairs)."""
    n = len(cols[0])
    assert len(pi) == n
    x, y = special_cells(perm, n)["pair"]
    new = [list(c) for c in cols]
    new[x // n][x % n] = (new[x // n][x % n] + 1) % R
    pi = list(pi)
    pi[x % n] = public_value(q, new, x % n)
    return new, pi, sorted([(x, y), (y, x)])


# ---- cosets (1, k1, k2) ----------------------------------------------------------------------------------------------------
def large_cosets(seed):
    """(1, k1, k2) with seeded 254-bit k1, k2 (every 254-bit value is below r): k_0 = 1 is the standard choice, and the one the
    batched quotient kernel treats on a path of its own"""
    rng = random.Random(seed)
    return (1, rng.getrandbits(253) | 1 << 253, rng.getrandbits(253) | 1 << 253)


def cosets_are_disjoint(cosets, n):
    return all(pow(cosets[i] * pow(cosets[j], -1, R) % R, n, R) != 1 for i in range(3) for j in range(3) if i != j)
