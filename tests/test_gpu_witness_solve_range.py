"""typlonk_witness_solve where tests/test_gpu_witness_solve.py and tests/test_gpu_witness_hints.py do not reach: more witnesses
than one launch group (rows and hints, narrow runs and wide launches); public values given as any word below 2^256 and a grid of
operands, selectors and quotients at the limits of the lazy arithmetic; a wide level of thousands of hints whose wavefronts hold
one kind of hint alone, both kinds, rows beside hints, and idle lanes; a loaded circuit whose permutation is recovered under
254-bit cosets, and the plan rebuilt from the installed hints after a call under other cosets.  Everything is integer equality
with the Python statements (tests/witness_solve_ref.py, tests/witness_hints_ref.py); every precondition that keeps a comparison
from passing vacuously is asserted on the CPU before anything goes to the device."""
import random

import numpy as np
import pytest

import witness_check_ref as W
import witness_hints_ref as H
import witness_solve_ref as S
from helpers import O
from oracle import plonk_oracle as PO
from test_gpu_witness_check_range import (_ALT_EVEN, _ALT_ODD, _LOW8, CELL_WORDS, SEL_WORDS, _cosets_are_disjoint, _large_cosets,
                                          _other_representatives)
from test_gpu_witness_solve import CLEAN, GARBAGE, L12_WIDTHS, Compiled, _expected, _limbs, _solve
from typlonk_amd import capi

pytestmark = pytest.mark.gpu

R = O.R
TOP = 1 << 256
ERR_INVALID_ARG = -1
MANY = 1030                                                     # above the 1024 witnesses of a launch group
GROUP = 1024


def _word_cols(want):
    """the canonical words of [three columns] per witness"""
    return [[W.mont_words(col) for col in cols] for cols in want]


def _differs(got, words):
    """the first (witness, column) whose words are not the expected ones, or None"""
    for k, (g, w) in enumerate(zip(got, words)):
        for i in range(3):
            if not np.array_equal(g[i], w[i]):
                return k, i
    return None


def _twice(ctx, c, wits, want, reports, raw_pi=False):
    """solve and check, then once more from the cached plan and the reused workspace: the words of `want` and `reports` both
    times"""
    words = _word_cols(want)
    for attempt in range(2):
        got, reps = _solve(ctx, c, wits, raw_pi=raw_pi)
        assert _differs(got, words) is None, attempt
        assert len(reps) == len(reports)
        bad = [k for k in range(len(reps)) if reps[k] != reports[k]]
        assert not bad, (attempt, bad[:8])


def _hinted(ctx, q, perm, hints, how="perm", cosets=PO.COSETS):
    c = Compiled(ctx, q, perm, how, cosets)
    try:
        ctx.circuit_set_hints(c.cid, c.cosets, hints)
    except BaseException:
        c.free()
        raise
    return c


def _past_the_group_differs(want, cells=None):
    """witnesses 1024 .. 1029 differ from witnesses 0 .. 5 and from each other, in every column (in the cells `cells` = [(column,
    row)] if given): an offset that forgets the group would show"""
    pick = (lambda cols: [cols[i][j] for i, j in cells]) if cells else None   # noqa: E731
    views = [[pick(want[k])] if pick else want[k] for k in list(range(6)) + list(range(GROUP, GROUP + 6))]
    return all(x != y for a in range(12) for b in range(a + 1, 12) for x, y in zip(views[a], views[b]))


# ---- 1. past one launch group ---------------------------------------------------------------------------------------------------
def many_chains(log_n=4):
    """the squaring chain at 2^4 rows: witness k starts from 2 + k, has blinding cells of its own and pi_len = 0, 1, n in turn"""
    n = 1 << log_n
    _, q, perm, _, _ = S.chain(log_n)
    wits, want = [], []
    for k in range(MANY):
        pi = S.public_values(n, (0, 1, n)[k % 3], 9000 + k)
        _, _, _, assigned, cols = S.chain(log_n, pi, x0=2 + k)
        for i, x in enumerate(sorted(S.blinding_cells(n))):
            assigned[x] = cols[x // n][x % n] = 70000 + 16 * k + i
        wits.append((assigned, pi))
        want.append(cols)
    return q, perm, wits, want


def test_chain_witnesses_past_one_launch_group(ctx):
    """narrow runs: blockIdx.x is the witness.  Witness 1024 + k has its own input, blinding cells and public values"""
    q, perm, wits, want = many_chains()
    assert _past_the_group_differs(want)
    assert [len(pi) for _, pi in wits[GROUP:]] == [len(pi) for _, pi in wits[1:7]] != [len(pi) for _, pi in wits[:6]]
    assert all(W.check(q, perm, want[k], wits[k][1]) == ([], []) for k in list(range(6)) + list(range(GROUP, MANY)))
    assert want[0] == S.solve(q, perm, *wits[0]) and want[MANY - 1] == S.solve(q, perm, *wits[MANY - 1])
    c = Compiled(ctx, q, perm)
    try:
        assert ctx.witness_solve_plan(c.cid, c.cosets)["launches"] == 2
        _twice(ctx, c, wits, want, [CLEAN] * MANY)
    finally:
        c.free()


def many_hinted(which):
    """H.range_check(5, 8) or H.nonzero(3) under 1030 inputs: (q, perm, hints, wits, want, the hinted cells as (column, row))"""
    rng = random.Random(1030)
    if which == "range":
        n, q, perm, hints, (cx, cy) = H.range_check(5, 8)
        wits = [({cx: k % 251, cy: rng.randrange(R) if k % 7 == 3 else k // 251}, []) for k in range(MANY)]
    else:
        n, q, perm, hints, (cx,) = H.nonzero(3)
        wits = [({cx: 0 if k % 97 == 7 or k == GROUP + 3 else k + 1}, []) for k in range(MANY)]
    want = H.solve_many(q, perm, hints, wits)
    return q, perm, hints, wits, want, [(t[1] // n, t[1] % n) for t in hints]


@pytest.mark.parametrize("which", ["range", "nonzero"])
def test_hinted_witnesses_past_one_launch_group(ctx, which):
    """BITS and INV0 values in the hint table across the group border (a.htab = d_htab + first * n_hints)"""
    q, perm, hints, wits, want, hinted_cells = many_hinted(which)
    assert _past_the_group_differs(want, hinted_cells)
    assert want[GROUP + 3] == H.solve(q, perm, hints, *wits[GROUP + 3])
    reports = [_expected(q, perm, cols, []) for cols in want]
    assert sum(r == CLEAN for r in reports) > MANY // 2 and sum(r != CLEAN for r in reports) >= 10
    if which == "nonzero":                                       # INV0 of 0 on either side of the border
        assert wits[7][0][0] == 0 and wits[GROUP + 3][0][0] == 0 and want[7][1][0] == 0 and want[GROUP + 3][1][0] == 0
    c = _hinted(ctx, q, perm, hints)
    try:
        _twice(ctx, c, wits, want, reports)
    finally:
        c.free()


WIDE_WIDTHS = [120, 257, 100, 32]                               # all 509 rows that are no blinding rows: none is undriven
WIDE_SHAPE = [(60, 2), (200, 100), (60, 2)]


def _inputs_of(assigned, n, k):
    """the inputs of witness k: every assigned cell but the blinding cells moved by k"""
    return {x: (v + k) % R if x % n < n - 3 else v for x, v in assigned.items()}


def many_layered():
    """a layered circuit at 2^9 rows whose second level is a wide launch of 257 rows, under 1030 inputs; pi_len = 0, 1, n in turn"""
    L = S.layered(9, 1030, WIDE_WIDTHS)
    n, q, perm = L["n"], L["q"], L["perm"]
    wits = [(_inputs_of(L["assigned"], n, k), S.public_values(n, (0, 1, n)[k % 3], 5000 + k)) for k in range(MANY)]
    return L, wits, S.solve_many(q, perm, wits)


def test_layered_witnesses_past_one_launch_group(ctx):
    """a wide launch: blockIdx.y is the witness"""
    L, wits, want = many_layered()
    q, perm = L["q"], L["perm"]
    assert S.plan(q, perm)["schedule"] == [[0, 1, 0], [1, 1, 1], [2, 2, 0]] and L["undriven"] == []
    assert want[0] == L["cols"] and want[GROUP + 1] == S.solve(q, perm, *wits[GROUP + 1])
    assert _past_the_group_differs(want)
    reports = [_expected(q, perm, cols, pi) for cols, (_, pi) in zip(want, wits)]
    assert all(r["gate_failures"] == 0 for r in reports)        # every row is driven
    c = Compiled(ctx, q, perm)
    try:
        _twice(ctx, c, wits, want, reports)
    finally:
        c.free()


def many_stacked():
    """H.stacked at 2^9 rows with a wide level of 200 rows + 100 hints, under 1030 inputs; every third witness has public values"""
    L = H.stacked(9, 1031, WIDE_SHAPE)
    n, q, perm, hints = L["n"], L["q"], L["perm"], L["hints"]
    undriven = [j for j in range(n) if not q["q_o"][j]]          # their selectors are all zero: no public value there
    wits = [(_inputs_of(L["assigned"], n, k), S.public_values(n, (0, 1, n)[k % 3], 6000 + k, zero_rows=undriven)) for k in range(MANY)]
    return L, wits, H.solve_many(q, perm, hints, wits)


def test_stacked_witnesses_past_one_launch_group(ctx):
    """the hinted wide launch and the hinted fill: the hint table of witness blockIdx.y of the second group"""
    L, wits, want = many_stacked()
    q, perm, hints = L["q"], L["perm"], L["hints"]
    assert H.plan(q, perm, hints)["schedule"] == [[0, 1, 0], [1, 1, 1], [2, 1, 0]]
    assert want[GROUP + 2] == H.solve(q, perm, hints, *wits[GROUP + 2])
    assert _past_the_group_differs(want) and _past_the_group_differs(want, [(t[1] // L["n"], t[1] % L["n"]) for t in hints])
    assert all(_expected(q, perm, want[k], wits[k][1]) == CLEAN for k in list(range(0, MANY, 50)) + list(range(GROUP, MANY)))
    c = _hinted(ctx, q, perm, hints)
    try:
        _twice(ctx, c, wits, want, [CLEAN] * MANY)               # every driven row holds, an empty row asks nothing
    finally:
        c.free()


# ---- 2. full-range public values and extreme operands ---------------------------------------------------------------------------
RANDOM_WIDTHS = {4: [3, 2, 4], 9: [100, 257, 3, 120], 12: L12_WIDTHS}


def raw_pi_case(log_n):
    """a layered circuit with a public value on every gate row; the values as raw words, a third of them another word of the same
    residue.  Two witnesses: all n public values, and the first n / 2 + 1 of them."""
    n = 1 << log_n
    pi = S.public_values(n, n, 40 + log_n)
    L = S.layered(log_n, 40 + log_n, RANDOM_WIDTHS[log_n], pi, ties=(1, 1))
    raw = _other_representatives(W.raw_of(pi), np.random.default_rng(50 + log_n))
    return L, raw, [raw, raw[:n // 2 + 1]]


@pytest.mark.parametrize("log_n", [4, 9, 12])
def test_public_values_as_any_word_below_2_256(ctx, log_n):
    L, raw, raws = raw_pi_case(log_n)
    n, q, perm = L["n"], L["q"], L["perm"]
    assert (raw >= R).sum() > n // 4 and raw.max() < TOP and (log_n < 9 or (raw >= 2 * R).sum() > n // 50)
    assert all(raw[j] % R != 0 for j in range(n - 3))            # a public value on every gate row
    residues = [W.residues_of(r).tolist() for r in raws]
    assert residues[0] == L["pi"]
    want = [S.solve(q, perm, L["assigned"], pi) for pi in residues]
    assert want[0] == L["cols"] and want[1] != want[0]
    reports = [_expected(q, perm, cols, pi) for cols, pi in zip(want, residues)]
    # the circuit's own witness is clean up to its unequal ties
    assert reports[0]["gate_failures"] == 0 and 0 < reports[0]["copy_failures"]
    assert {x for pair in reports[0]["copy_cells"] for x in pair} <= set(L["unequal"])
    c = Compiled(ctx, q, perm)
    try:
        _twice(ctx, c, [(L["assigned"], r) for r in raws], want, reports, raw_pi=True)
    finally:
        c.free()


A_WORDS = [0, 1, 2, R - 2, R - 1, 2**254, 2**240 - 1, _LOW8, _ALT_EVEN % R, _ALT_ODD]
QO_WORDS = [1, 2, R - 1, R - 2, 2**254, None]                   # None: a fresh random word
TOP_LIMB = R >> 240                                             # the largest top limb of a canonical word
# the special rows: (a and b word, selector word, q_o word, PI word, what q_c is chosen for)
SPECIAL = [(R - 1, R - 1, 1, TOP - 1, None), (R - 1, R - 1, R - 1, TOP - 1, None), (_LOW8, _LOW8, R - 1, TOP - 1, None),
           (_ALT_ODD, R - 1, R - 2, _ALT_EVEN, None), (R - 2, 2**254, 2**254, TOP - 2, None), (R - 1, _LOW8, 2, 2 * R + 1, None),
           (R - 1, R - 1, 1, TOP - 1, "zero"), (R - 1, R - 1, R - 1, TOP - 1, "zero"), (_LOW8, R - 2, 2**254, 2 * R - 1, "zero"),
           (1, 0, 2, 0, "zero"),
           (R - 1, R - 1, 1, TOP - 1, "residue r - 1"), (R - 1, R - 1, R - 1, TOP - 1, "residue r - 1"), (2, 1, R - 2, R, "residue r - 1"),
           (R - 1, R - 1, 1, TOP - 1, "word r - 1"), (R - 1, R - 1, R - 1, TOP - 1, "word r - 1"), (_ALT_ODD, _LOW8, 2, TOP - 1, "word r - 1"),
           (R - 1, R - 1, R - 1, TOP - 1, "top limb"), (0, 0, 1, 0, "top limb"), (R - 1, R - 1, R - 1, TOP - 1, "low limbs")]
TARGET_WORDS = {"zero": 0, "word r - 1": R - 1, "top limb": TOP_LIMB << 240, "low limbs": _LOW8}
N_GRID = 512
UNDRIVEN = [j for j in range(N_GRID) if j % 61 == 50]            # 50, 111, .. 477: eight rows with q_o = 0


def extremes_case():
    """n = 2^9 rows under the identity permutation: every a and b cell is a free class of its own and is assigned, so a driven
    row computes from the words the test chooses.  (a, b) run through A_WORDS x A_WORDS, q_l, q_r, q_m, q_c through SEL_WORDS
    at other strides, q_o through QO_WORDS, the public values (one on every row) through CELL_WORDS; the words are what the
    device reads, so the residues are those words * 2^-256.  The last rows are SPECIAL: the largest of everything at once, and
    q_c chosen for a numerator of 0, for the quotient r - 1 (as a residue and as a word) and for words with a full top limb or
    full low limbs.  The rows UNDRIVEN have q_o = 0: of their c cells two are assigned, one is left to read 0, five are left
    for hints.  Returns a dict: q, perm, assigned, raw_pi, pi (residues), special ({row: kind}), free_c (the five cells)."""
    n, ns = N_GRID, len(SEL_WORDS)
    rng = random.Random(31)
    assert all(0 <= w < R for w in A_WORDS) and len(set(A_WORDS)) == len(A_WORDS)
    a = [A_WORDS[j % 10] for j in range(n)]
    b = [A_WORDS[j // 10 % 10] for j in range(n)]
    sel = [[SEL_WORDS[(3 * j + j // 10) % ns] for j in range(n)], [SEL_WORDS[j // 3 % ns] for j in range(n)],
           [SEL_WORDS[(5 * j + j // 16) % ns] for j in range(n)], [SEL_WORDS[(7 * j + j // 64) % ns] for j in range(n)]]   # q_l q_r q_m q_c
    qo = [QO_WORDS[(j + j // 6) % len(QO_WORDS)] for j in range(n)]
    raw_pi = [CELL_WORDS[(3 * j + 1) % len(CELL_WORDS)] for j in range(n)]
    first = n - len(SPECIAL)
    assert first > max(UNDRIVEN)
    for i, (cw, sw, ow, pw, _) in enumerate(SPECIAL):
        j = first + i
        a[j] = b[j] = cw
        for s in sel:
            s[j] = sw
        qo[j], raw_pi[j] = ow, pw
    for j in UNDRIVEN:
        qo[j] = 0
    sel = [[rng.randrange(R) if w is None else w for w in s] for s in sel]
    qo = [rng.randrange(1, R) if w is None else w for w in qo]
    res = lambda words: W.residues_of(W._obj(words)).tolist()   # noqa: E731
    ar, br, pi = res(a), res(b), res(raw_pi)
    ql, qr, qm, qc = (res(s) for s in sel)
    qor = res(qo)
    special = {}
    for i, (_, _, _, _, kind) in enumerate(SPECIAL):
        j = first + i
        special[j] = kind
        if kind is None:
            continue
        target = R - 1 if kind == "residue r - 1" else TARGET_WORDS[kind] * W.MONT_INV % R
        qc[j] = (qor[j] * target - (ql[j] * ar[j] + qr[j] * br[j] + qm[j] * ar[j] * br[j] + pi[j])) % R
    q = dict(zip(W.SELECTORS, (ql, qr, qor, qm, qc)))
    assigned = {j: ar[j] for j in range(n)}
    assigned.update({n + j: br[j] for j in range(n)})
    assigned.update({2 * n + UNDRIVEN[0]: R - 1, 2 * n + UNDRIVEN[1]: W.residues_of(W._obj([_LOW8]))[0]})
    return {"n": n, "q": q, "perm": list(range(3 * n)), "assigned": assigned, "raw_pi": raw_pi, "pi": pi, "special": special,
            "free_c": [2 * n + j for j in UNDRIVEN[3:]]}


def extremes_expected(E):
    """the columns by big integers, row by row (the permutation is the identity: S.solve must say the same), with what the
    comparison needs to be worth something asserted"""
    n, q, pi, assigned = E["n"], E["q"], E["pi"], E["assigned"]
    a, b = [assigned[j] for j in range(n)], [assigned[n + j] for j in range(n)]
    c = [0] * n
    for j in range(n):
        if q["q_o"][j]:
            num = q["q_l"][j] * a[j] + q["q_r"][j] * b[j] + q["q_m"][j] * a[j] * b[j] + q["q_c"][j] + pi[j]
            c[j] = num * pow(q["q_o"][j], -1, R) % R
        else:
            c[j] = assigned.get(2 * n + j, 0)
    want = [a, b, c]
    assert want == S.solve(q, E["perm"], assigned, pi)
    words = W.raw_of(c).tolist()
    rows = lambda kind: [j for j, k in E["special"].items() if k == kind]   # noqa: E731
    assert len(rows("zero")) == 4 and all(c[j] == 0 for j in rows("zero"))
    assert len(rows("residue r - 1")) == 3 and all(c[j] == R - 1 for j in rows("residue r - 1"))
    for kind, w in TARGET_WORDS.items():
        assert rows(kind) and all(words[j] == w for j in rows(kind)), kind
    assert 0 in words and R - 1 in words and sum(w >> 240 == TOP_LIMB for w in words) >= 4
    driven = [j for j in range(n) if q["q_o"][j]]
    assert len(driven) == n - len(UNDRIVEN) > S.NARROW              # one wide level
    assert len({(W.raw_of([a[j]])[0], W.raw_of([b[j]])[0]) for j in driven}) >= 100     # every pair of A_WORDS x A_WORDS
    assert sum(w >= R for w in E["raw_pi"]) > n // 4 and max(E["raw_pi"]) == TOP - 1
    return want


def extremes_hints(E, want):
    """an INV0 and a BITS hint of a c cell that holds r - 1 and of one that holds 0, and a BITS hint of the word r - 1; each writes
    the c cell of an undriven row"""
    n = E["n"]
    at = lambda kind, i=0: 2 * n + [j for j, k in E["special"].items() if k == kind][i]   # noqa: E731
    top, zero, word = at("residue r - 1"), at("zero", 1), at("word r - 1", 2)
    assert want[2][top - 2 * n] == R - 1 and want[2][zero - 2 * n] == 0
    d = E["free_c"]
    return [(H.INV0, d[0], top, 0, 0), (H.BITS, d[1], top, 191, 64), (H.INV0, d[2], zero, 0, 0), (H.BITS, d[3], zero, 0, 64),
            (H.BITS, d[4], word, 250, 64)]


def test_a_grid_of_extreme_operands_selectors_and_public_words(ctx):
    E = extremes_case()
    n, q, perm, assigned = E["n"], E["q"], E["perm"], E["assigned"]
    want = extremes_expected(E)
    hints = extremes_hints(E, want)
    hinted = H.solve(q, perm, hints, assigned, E["pi"])
    cell = lambda cols, x: cols[x // n][x % n]   # noqa: E731
    assert [cell(hinted, t[1]) for t in hints] == [R - 1, (R - 1) >> 191, 0, 0, cell(hinted, hints[4][2]) >> 250]
    assert all(cell(want, t[1]) == 0 for t in hints) and cell(hinted, hints[4][1]) != 0
    assert all(cell(hinted, x) == cell(want, x) for x in range(3 * n) if x not in {t[1] for t in hints})
    assert H.plan(q, perm, hints)["schedule"] == [[0, 1, 1], [1, 1, 0]]
    wits = [(assigned, E["raw_pi"])]
    c = Compiled(ctx, q, perm)
    try:
        assert ctx.witness_solve_plan(c.cid, c.cosets) == {"driven_rows": n - len(UNDRIVEN), "free_classes": 2 * n + len(UNDRIVEN),
                                                           "depth": 1, "launches": 2}
        _twice(ctx, c, wits, [want], [_expected(q, perm, want, E["pi"])], raw_pi=True)
        # the same rows through the kernels of a circuit with hints, and hints that read the extremes
        ctx.circuit_set_hints(c.cid, c.cosets, hints)
        _twice(ctx, c, wits, [hinted], [_expected(q, perm, hinted, E["pi"])], raw_pi=True)
    finally:
        c.free()


# ---- 3. a wide level of thousands of hints --------------------------------------------------------------------------------------
def wall_case():
    L = H.hint_wall(13, 3000)
    n, q = L["n"], L["q"]
    quiet = [j for j in range(n) if not q["q_o"][j]] + [L["zero_row"]]
    pis = [[], S.public_values(n, n // 2, 3001, zero_rows=quiet), S.public_values(n, n, 3002, zero_rows=quiet)]
    return L, list(zip(L["assigned"], pis))


def wavefront_kinds(ref, hints, level):
    """what each wavefront of a wide level's launch holds: a set over "row", "inv0", "bits", "idle" per 64 lanes of its workgroups"""
    lo, hi = ref["level_off"][level], ref["level_off"][level + 1]
    entries = ref["order"][lo:hi] + [None] * (-(hi - lo) % S.NARROW)
    kind = lambda e: "idle" if e is None else ("row" if not H.is_hint(e) else ("inv0" if hints[e & ~H.HINT][0] == H.INV0 else "bits"))   # noqa: E731
    return [frozenset(kind(e) for e in entries[i:i + 64]) for i in range(0, len(entries), 64)]


def test_a_wide_level_of_three_thousand_hints(ctx):
    L, wits = wall_case()
    n, q, perm, hints = L["n"], L["q"], L["perm"], L["hints"]
    ref = H.plan(q, perm, hints)
    assert ref["schedule"] == [[0, 1, 1], [1, 1, 1], [2, 1, 1]] and ref["launches"] == 4
    width = ref["level_off"][2] - ref["level_off"][1]
    assert width == 37 + len(hints) and len(hints) >= 3000 and width % S.NARROW and width % 64
    waves = wavefront_kinds(ref, hints, 1)
    for held in ({"inv0"}, {"bits"}, {"inv0", "bits"}, {"row", "bits"}, {"idle"}):
        assert frozenset(held) in waves, held
    assert any("idle" in w and len(w) > 1 for w in waves)       # the last wavefront that has entries is partly idle
    assert {(t[3], t[4]) for t in hints if t[0] == H.BITS} == set(H.BIT_WINDOWS)
    first = ref["order"][ref["level_off"][0]:ref["level_off"][1]]
    assert len(first) == 1000 and {t[2] - 2 * n for t in hints[:1000]} == set(first)       # every output feeds a BITS hint
    want = H.solve_many(q, perm, hints, wits)
    assert want[2] == H.solve(q, perm, hints, *wits[2])
    assert all(_expected(q, perm, cols, pi) == CLEAN for cols, (_, pi) in zip(want, wits))
    zero = hints[L["zero_hint"]]
    assert zero[0] == H.INV0 and zero[2] == 2 * n + L["zero_row"]
    assert [cols[2][L["zero_row"]] == 0 for cols in want] == [False, False, True]
    assert [cols[0][zero[1]] == 0 for cols in want] == [False, False, True]
    readers = ref["order"][ref["level_off"][2]:ref["level_off"][3]]
    assert len(readers) == 300 and all(H.is_hint(ref["src"][j]) and H.is_hint(ref["src"][n + j]) for j in readers)
    c = _hinted(ctx, q, perm, hints)
    try:
        assert ctx.witness_solve_plan(c.cid, c.cosets) == {k: ref[k] for k in ("driven_rows", "free_classes", "depth", "launches")}
        _twice(ctx, c, wits, want, [CLEAN] * 3)
    finally:
        c.free()


# ---- 4. other cosets and the rebuild --------------------------------------------------------------------------------------------
COSET_WIDTHS = {5: [3, 1, 9, 4, 8], 12: L12_WIDTHS}
COSET_SHAPES = {5: [(5, 2), (6, 3), (5, 2)], 12: [(63, 2), (300, 200), (63, 2), (63, 2)]}


def _fill(ctx, n):
    outs = [ctx.alloc(n) for _ in range(3)]
    fill = np.full((n, 4), GARBAGE, dtype=np.uint64)
    for b in outs:
        b.upload(fill)
    return outs, fill


@pytest.mark.parametrize("log_n", [5, 12])
def test_a_loaded_circuit_under_254_bit_cosets(ctx, log_n):
    n = 1 << log_n
    cosets = _large_cosets(100 + log_n)
    assert all(k >> 253 == 1 for k in cosets[1:]) and _cosets_are_disjoint(cosets, n)
    pi = S.public_values(n, n // 2, 100 + log_n)
    L = S.layered(log_n, 100 + log_n, COSET_WIDTHS[log_n], pi)
    q, perm = L["q"], L["perm"]
    ref = S.plan(q, perm)
    c = Compiled(ctx, q, perm, "load", cosets)
    try:
        assert ctx.witness_solve_plan(c.cid, c.cosets) == {k: ref[k] for k in ("driven_rows", "free_classes", "depth", "launches")}
        _twice(ctx, c, [(L["assigned"], pi)], [L["cols"]], [_expected(q, perm, L["cols"], pi)])
    finally:
        c.free()


@pytest.mark.parametrize("log_n", [5, 12])
def test_hints_under_254_bit_cosets_and_the_rebuild_after_other_cosets(ctx, log_n):
    """a loaded circuit with hints: solved under its 254-bit cosets; refused under (1, 2, 3)-style cosets as the check refuses it
    (the ids are others: sigma is no permutation), the outputs untouched; solved again under its own cosets from a plan that
    is rebuilt from the installed hints"""
    n = 1 << log_n
    cosets = _large_cosets(200 + log_n)
    assert all(k >> 253 == 1 for k in cosets[1:]) and _cosets_are_disjoint(cosets, n) and tuple(cosets) != tuple(PO.COSETS)
    L = H.stacked(log_n, 200 + log_n, COSET_SHAPES[log_n])
    q, perm, hints, assigned = L["q"], L["perm"], L["hints"], L["assigned"]
    wits = [(assigned, [])]
    want = H.solve(q, perm, hints, assigned)
    bare = S.solve(q, perm, assigned)
    dst = [t[1] for t in hints]
    assert sum(want[x // n][x % n] != 0 for x in dst) > len(dst) // 2 and all(bare[x // n][x % n] == 0 for x in dst)
    small = [_limbs(k) for k in PO.COSETS]
    cells = sorted(assigned)
    values = W.mont_words([assigned[x] for x in cells])[None]
    c = _hinted(ctx, q, perm, hints, "load", cosets)
    outs, fill = _fill(ctx, n)
    try:
        assert ctx.witness_solve_plan(c.cid, c.cosets) == H.info(q, perm, hints)
        _twice(ctx, c, wits, [want], [CLEAN])
        with pytest.raises(capi.TyplonkError) as checked:
            ctx.witness_check(c.cid, [outs], None, None, small)
        assert checked.value.code == ERR_INVALID_ARG and "defects" in str(checked.value)
        with pytest.raises(capi.TyplonkError) as solved:
            ctx.witness_solve(c.cid, small, cells, values, [outs])
        assert solved.value.code == checked.value.code and str(solved.value) == str(checked.value)
        with pytest.raises(capi.TyplonkError) as planned:
            ctx.witness_solve_plan(c.cid, small)
        assert planned.value.code == checked.value.code
        assert all(np.array_equal(b.download(), fill) for b in outs)
        # the right cosets again: the hints are still in force
        ctx.witness_solve(c.cid, c.cosets, cells, values, [outs])
        assert _differs([[b.download() for b in outs]], _word_cols([want])) is None
        assert ctx.witness_solve_plan(c.cid, c.cosets) == H.info(q, perm, hints)
        _twice(ctx, c, wits, [want], [CLEAN])
    finally:
        for b in outs:
            b.free()
        c.free()
