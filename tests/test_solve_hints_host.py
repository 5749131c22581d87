"""solve_plan with hints (csrc/solve_plan.hpp), every decision of a solve under typlonk_circuit_set_hints, without a GPU: the
header as the host compiles it on its own (tests/cpp/solve_hints_host; tests/cpp/solve_hints_host_san is the same program under
the address and undefined-behaviour sanitizers) against the Python statement (tests/witness_hints_ref.py): src, the levels of
rows and hints, the level lists (rows first, then hints) and the schedule are equal word for word, a level's width counts rows
and hints, every refusal names the lowest offending hint and every kind of cycle is refused.  The Python statement itself is
held against witness_check_ref.check on the circuits the GPU tests solve."""
import json
import os
import subprocess

import pytest

import witness_check_ref as W
import witness_hints_ref as H
import witness_solve_ref as S
from helpers import ROOT

R = H.R


def _text(q, perm, hints, narrow=H.NARROW, cut=H.RUN_CUT):
    n = len(q["q_o"])
    return (f"{n} {narrow} {cut} {len(hints)}\n" + " ".join(map(str, perm)) + "\n" + " ".join(str(int(d)) for d in S.driven_rows(q)) + "\n"
            + "".join(" ".join(map(str, h)) + "\n" for h in hints))


def _plans(cases, exe="solve_hints_host"):
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", exe)], input="".join(_text(*c) for c in cases), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(cases)
    return out


STACK_SHAPE = [(63, 2), (63, 2), (63, 2), (200, 100), (63, 2), (63, 2)]


def _cases():
    out = []
    for log_n, k in ((4, 4), (5, 8), (6, 16)):
        _, q, perm, hints, _ = H.range_check(log_n, k)
        out.append((q, perm, hints))
    for log_n in (3, 6):
        _, q, perm, hints, _ = H.nonzero(log_n)
        out.append((q, perm, hints))
    _, q, perm, hints, _ = H.hint_chain(4)
    out.append((q, perm, hints))
    _, q, perm, hints, _ = H.bit_windows(4)
    out.append((q, perm, hints))
    c = H.stacked(10, 5, STACK_SHAPE)                         # 63 rows + 2 hints; 200 rows + 100 hints: wide
    out += [(c["q"], c["perm"], c["hints"]), (c["q"], c["perm"], c["hints"], 64, 2), (c["q"], c["perm"], c["hints"], 65, 1)]
    c = H.stacked(10, 6, [(200, 56), (3, 1), (199, 58), (4, 0)])   # 256 entries: narrow; 257: wide
    out.append((c["q"], c["perm"], c["hints"]))
    # no hints: the plan of the overload without them
    L = S.layered(6, 9, [3, 1, 9, 4, 12])
    out.append((L["q"], L["perm"], []))
    return out


@pytest.fixture(scope="module")
def cases():
    return _cases()


@pytest.fixture(scope="module")
def plans(built, cases):
    return _plans(cases)


def test_every_field_equals_the_python_statement(cases, plans):
    for case, got in zip(cases, plans):
        assert got["status"] == 0
        assert got == H.plan(*case), (len(case[1]) // 3, case[3:])


def test_without_hints_the_plan_is_the_unhinted_one(cases, plans):
    q, perm, hints = cases[-1]
    assert hints == []
    want = S.plan(q, perm)
    got = dict(plans[-1])
    assert got.pop("hint_level") == [] and got.pop("other") == 0
    assert got == want


def test_levels_order_and_widths(cases, plans):
    for case, p in zip(cases, plans):
        q, perm, hints = case[:3]
        narrow, cut = case[3:] if len(case) > 3 else (H.NARROW, H.RUN_CUT)
        n, driven, src, level, hl = len(perm) // 3, S.driven_rows(q), p["src"], p["level"], p["hint_level"]
        lev = lambda s: (hl[s & ~H.HINT] if H.is_hint(s) else 0) if s & H.FREE else level[s]   # noqa: E731
        for j in range(n):
            assert (level[j] > 0) == driven[j]
            if driven[j]:
                assert level[j] == 1 + max(lev(src[j]), lev(src[n + j])) and src[2 * n + j] == j
        for h, t in enumerate(hints):
            assert hl[h] == 1 + lev(src[t[2]]) and src[t[1]] == H.HINT | h
        assert p["driven_rows"] == sum(driven) and len(p["order"]) == sum(driven) + len(hints)
        # within a level: the rows ascending, then the hints ascending
        for l in range(p["depth"]):
            es = p["order"][p["level_off"][l]:p["level_off"][l + 1]]
            rows, hs = [e for e in es if not H.is_hint(e)], [e & ~H.HINT for e in es if H.is_hint(e)]
            assert es == rows + [H.HINT | h for h in hs] and rows == sorted(rows) and hs == sorted(hs)
            assert all(level[j] == l + 1 for j in rows) and all(hl[h] == l + 1 for h in hs)
        at = 0
        for first, levels, wide in p["schedule"]:
            assert first == at
            widths = [p["level_off"][l + 1] - p["level_off"][l] for l in range(first, first + levels)]
            assert (levels == 1 and widths[0] > narrow) if wide else (levels <= cut and max(widths) <= narrow)
            at += levels
        assert at == p["depth"] and p["launches"] == len(p["schedule"]) + 1
        # free classes: hinted ones are counted, and the unhinted ones keep their slot numbers
        plain, free = S.sources(q, perm)
        assert p["free_classes"] == free
        assert all(src[x] == plain[x] or H.is_hint(src[x]) for x in range(3 * n))


def test_a_levels_width_counts_rows_and_hints(cases, plans):
    by = {(len(c[1]) // 3, len(c[2])) + tuple(c[3:]): p for c, p in zip(cases, plans)}
    n_hints = sum(h for _, h in STACK_SHAPE)
    widths = lambda p: [b - a for a, b in zip(p["level_off"], p["level_off"][1:])]   # noqa: E731
    p = by[(1024, n_hints)]
    assert widths(p) == [65, 65, 65, 300, 65, 65] and p["schedule"] == [[0, 3, 0], [3, 1, 1], [4, 2, 0]]
    # 63 rows + 2 hints against a limit of 64 entries: wide, though the rows alone would fit
    assert by[(1024, n_hints, 64, 2)]["schedule"] == [[k, 1, 1] for k in range(6)]
    assert by[(1024, n_hints, 65, 1)]["schedule"] == [[0, 1, 0], [1, 1, 0], [2, 1, 0], [3, 1, 1], [4, 1, 0], [5, 1, 0]]
    p = by[(1024, 56 + 1 + 58)]
    assert widths(p) == [256, 4, 257, 4] and p["schedule"] == [[0, 2, 0], [2, 1, 1], [3, 1, 0]]
    for log_n, k in ((4, 4), (5, 8), (6, 16)):
        p = by[(1 << log_n, k)]
        assert p["depth"] == k + 1 and widths(p) == [1, k] + [1] * (k - 1) and p["launches"] == 2


def _refusals():
    """(name, q, perm, hints, status, bad, other)"""
    n, q, perm, hints, _ = H.range_check(4, 4)
    src, _ = S.sources(q, perm)
    driven_cell = 2 * n + 5                               # the c cell of a recomposition row
    rep = lambda i, t: hints[:i] + [t] + hints[i + 1:]   # noqa: E731
    out = [
        ("an unknown kind", q, perm, rep(2, (3, 3, 2 * n, 0, 1)), H.HINT_KIND, 2, 0),
        ("kind 0", q, perm, rep(1, (0, 2, 2 * n, 0, 1)), H.HINT_KIND, 1, 0),
        ("dst >= 3n", q, perm, rep(3, (H.BITS, 3 * n, 2 * n, 0, 1)), H.HINT_CELL, 3, 0),
        ("src >= 3n", q, perm, rep(0, (H.BITS, 1, 3 * n, 0, 1)), H.HINT_CELL, 0, 0),
        ("width 0", q, perm, rep(1, (H.BITS, 2, 2 * n, 1, 0)), H.HINT_RANGE, 1, 0),
        ("width 65", q, perm, rep(1, (H.BITS, 2, 2 * n, 1, 65)), H.HINT_RANGE, 1, 0),
        ("shift 255", q, perm, rep(2, (H.BITS, 3, 2 * n, 255, 1)), H.HINT_RANGE, 2, 0),
        ("dst in a driven class", q, perm, rep(2, (H.BITS, driven_cell, 2 * n, 2, 1)), H.HINT_DRIVEN, 2, 0),
        ("dst the c cell of row 0", q, perm, rep(2, (H.INV0, 2 * n, 0, 0, 0)), H.HINT_DRIVEN, 2, 0),
        ("two hints into one class", q, perm, rep(3, (H.BITS, n + 2, 2 * n, 3, 1)), H.HINT_CLASH, 3, 1),
        ("the lowest offender of two", q, perm, [hints[0], (H.BITS, 3 * n, 0, 0, 1), hints[2], (9, 0, 0, 0, 0)], H.HINT_CELL, 1, 0),
    ]
    assert not src[driven_cell] & S.FREE
    # cycles
    n, q, perm, hints, _ = H.nonzero(3)
    out += [
        ("src in dst's own class", q, perm, [(H.INV0, 5, 5, 0, 0)], H.HINT_CYCLE, 0, 0),
        ("src in dst's own class, which a row reads", q, perm, [(H.INV0, n, n, 0, 0)], H.CYCLE, 0, 0),
        ("two hints reading each other", q, perm, [(H.INV0, 5, 6, 0, 0), (H.INV0, n, 0, 0, 0), (H.BITS, 6, 5, 0, 8)], H.HINT_CYCLE, 0, 0),
        ("a hint reading a hint that reads a cycle", q, perm, [(H.INV0, n, 0, 0, 0), (H.INV0, 5, 6, 0, 0), (H.BITS, 6, 5, 0, 8), (H.BITS, 7, 6, 0, 8)],
         H.HINT_CYCLE, 1, 0),
        ("a hint reading a row that reads the hint", q, perm, [(H.INV0, n, 2 * n, 0, 0)], H.CYCLE, 0, 0),
    ]
    # a cycle among the rows alone, with a healthy hint beside it
    q2 = {name: [0] * 8 for name in W.SELECTORS}
    for j in (2, 5, 6):
        q2["q_o"][j] = 1
    two = list(range(24))
    two[16 + 5], two[2] = 2, 16 + 5
    two[16 + 2], two[5], two[8 + 6] = 5, 8 + 6, 16 + 2
    out.append(("a cycle among the rows", q2, two, [(H.INV0, 0, 1, 0, 0)], H.CYCLE, 2, 0))
    return out


def test_every_refusal_names_the_lowest_offender(built):
    ref = _refusals()
    got = _plans([(q, perm, hints) for _, q, perm, hints, _, _, _ in ref])
    for (name, q, perm, hints, status, bad, other), g in zip(ref, got):
        assert g == {"status": status, "bad": bad, "other": other}, name
        assert H.plan(q, perm, hints) == g, name


def test_the_sanitized_build_gives_the_same_plans(built, cases, plans):
    ref = _refusals()
    extra = [(q, perm, hints) for _, q, perm, hints, _, _, _ in ref]
    got = _plans(cases + extra, exe="solve_hints_host_san")
    assert got[:len(cases)] == plans
    assert [(g["status"], g["bad"]) for g in got[len(cases):]] == [(r[4], r[5]) for r in ref]


def test_host_program_refuses_input_cut_short(built):
    exe = os.path.join(ROOT, "tests", "cpp", "solve_hints_host")
    _, q, perm, hints, _ = H.nonzero(3)
    text = _text(q, perm, hints)
    assert subprocess.run([exe], input=text[:-4], capture_output=True, text=True, timeout=60).returncode == 2
    r = subprocess.run([exe], input="", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == ""


# ---- the Python statement against the Python checker ---------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,k", [(4, 4), (5, 8), (6, 16)])
def test_range_check_is_clean_exactly_below_2_k(log_n, k):
    n, q, perm, hints, (cx, cy) = H.range_check(log_n, k)
    assert H.plan(q, perm, hints)["depth"] == k + 1
    for x, y in H.RANGE_PAIRS(k):
        cols = H.solve(q, perm, hints, {cx: x, cy: y})
        gate, copy = W.check(q, perm, cols)
        if (x + y) % R < 1 << k:
            assert (gate, copy) == ([], []), (x, y)
        else:
            assert gate == [] and sorted(c[0] for c in copy) == [2 * n, 2 * n + 2 * k - 1], (x, y)


def test_nonzero_names_its_one_row_at_zero():
    for log_n in (3, 4, 5, 6):
        n, q, perm, hints, (cx,) = H.nonzero(log_n)
        for x in (1, 2, R - 1):
            assert W.check(q, perm, H.solve(q, perm, hints, {cx: x})) == ([], [])
        assert W.check(q, perm, H.solve(q, perm, hints, {cx: 0})) == ([1], [])


def test_the_statement_on_the_other_circuits():
    n, q, perm, hints, (cx,) = H.hint_chain(4)
    x = 0x1234567
    inv = pow(x, -1, R)
    cols = H.solve(q, perm, hints, {cx: x})
    assert cols[1][0] == inv and cols[0][1] == (inv >> 3) & ((1 << 40) - 1) and cols[2][2] == (cols[1][0] + cols[0][1]) % R
    n, q, perm, hints, (cx,) = H.bit_windows(4)
    v = (1 << 254) + 12345
    cols = H.solve(q, perm, hints, {cx: v})
    assert [cols[0][1 + i] for i in range(len(hints))] == [(v >> s) & ((1 << w) - 1) for s, w in H.BIT_WINDOWS]
    assert cols[0][1 + H.BIT_WINDOWS.index((250, 64))] == 16 and cols[0][1 + H.BIT_WINDOWS.index((254, 1))] == 1
    c = H.stacked(10, 5, STACK_SHAPE)
    cols = H.solve(c["q"], c["perm"], c["hints"], c["assigned"])
    assert W.check(c["q"], c["perm"], cols)[1] == []                 # every class holds one value
    assert cols[0][c["hints"][0][1]] == 0                            # INV0 of the unassigned input
