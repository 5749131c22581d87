"""typlonk_circuit_set_hints on the GPU: a solve under inverse and bit hints gives the columns of the Python statement
(tests/witness_hints_ref.py) word for word, and typlonk_witness_check on the solved buffers reports what the Python checker
reports on those columns.  The range check and the non-zero test, every window of BITS across the 30-, 32- and 64-bit
boundaries, a hint that reads a hint, narrow levels whose rows and hints straddle a wavefront, a wide level of rows and hints,
many witnesses per call, install / remove / reinstall, the three ways a circuit reaches the device, every refusal (each leaves the
installed hints in force), and solve -> check -> prove -> verify."""
import ctypes as C
import random

import numpy as np
import pytest

import witness_check_ref as W
import witness_hints_ref as H
import witness_solve_ref as S
from helpers import O, fr_pack
from test_gpu_witness_solve import CLEAN, COSETS, GARBAGE, Compiled, _expected, _limbs, _same, _solve
from typlonk_amd import capi

pytestmark = pytest.mark.gpu

R = O.R
ERR_INVALID_ARG, ERR_UNSATISFIED = -1, -8


def _hinted(ctx, q, perm, hints, how="perm"):
    c = Compiled(ctx, q, perm, how)
    try:
        ctx.circuit_set_hints(c.cid, COSETS, hints)
    except BaseException:
        c.free()
        raise
    return c


def _run(ctx, c, q, perm, hints, wits):
    """solve and check the witnesses [(assigned, pi)] in one call: the words and the reports are the Python statement's.
    Returns (the expected columns, the reports)."""
    want = [H.solve(q, perm, hints, a, pi) for a, pi in wits]
    got, reports = _solve(ctx, c, wits)
    for k, (g, w) in enumerate(zip(got, want)):
        assert _same(g, w), k
        assert reports[k] == _expected(q, perm, w, wits[k][1]), k
    return want, reports


@pytest.mark.parametrize("log_n,k", [(4, 4), (5, 8), (6, 16)])
def test_range_check(ctx, log_n, k):
    n, q, perm, hints, (cx, cy) = H.range_check(log_n, k)
    c = _hinted(ctx, q, perm, hints)
    try:
        info = ctx.witness_solve_plan(c.cid, COSETS)
        assert info == H.info(q, perm, hints) and info["depth"] == k + 1 and info["driven_rows"] == k
        pairs = H.RANGE_PAIRS(k)
        _, reports = _run(ctx, c, q, perm, hints, [({cx: x, cy: y}, []) for x, y in pairs])
        for (x, y), rep in zip(pairs, reports):
            if (x + y) % R < 1 << k:
                assert rep == CLEAN, (x, y)
            else:
                assert rep["gate_failures"] == 0 and sorted(p[0] for p in rep["copy_cells"]) == [2 * n, 2 * n + 2 * k - 1], (x, y)
    finally:
        c.free()


@pytest.mark.parametrize("log_n", [3, 4, 5, 6])
def test_nonzero(ctx, log_n):
    n, q, perm, hints, (cx,) = H.nonzero(log_n)
    c = _hinted(ctx, q, perm, hints)
    try:
        want, reports = _run(ctx, c, q, perm, hints, [({cx: x}, []) for x in (1, 2, R - 1, 0)])
        assert reports[:3] == [CLEAN] * 3
        assert reports[3] == {"gate_failures": 1, "copy_failures": 0, "gate_rows": [1], "copy_cells": []}   # solve papers over nothing
        assert want[2][1][0] == R - 1 and want[3][1][0] == 0
    finally:
        c.free()


def test_bits_across_every_limb_and_word_boundary(ctx):
    n, q, perm, hints, (cx,) = H.bit_windows(4)
    values = [0, 1, R - 1, (1 << 254) + 12345, random.Random(41).randrange(R)]
    c = _hinted(ctx, q, perm, hints)
    try:
        want, reports = _run(ctx, c, q, perm, hints, [({cx: v}, []) for v in values])
        assert reports == [CLEAN] * len(values)
        for v, cols in zip(values, want):
            assert [cols[0][1 + i] for i in range(len(hints))] == [(v >> s) & ((1 << w) - 1) for s, w in H.BIT_WINDOWS]
    finally:
        c.free()


def test_a_hint_reads_a_hint(ctx):
    n, q, perm, hints, (cx,) = H.hint_chain(4)
    c = _hinted(ctx, q, perm, hints)
    try:
        assert ctx.witness_solve_plan(c.cid, COSETS) == {"driven_rows": 1, "free_classes": H.info(q, perm, hints)["free_classes"], "depth": 3,
                                                         "launches": 2}
        _, reports = _run(ctx, c, q, perm, hints, [({cx: x}, []) for x in (0x1234567, 0, R - 1, 1)])
        assert reports == [CLEAN] * 4
    finally:
        c.free()


STACK_SHAPE = [(63, 2), (63, 2), (63, 2), (200, 100), (63, 2), (63, 2)]


def test_rows_and_hints_share_narrow_and_wide_levels_at_2_10(ctx):
    """levels of 63 rows + 2 hints: the entries straddle a wavefront, the second wavefront holds one row and two hints; a wide
    level of 200 rows + 100 hints, read by the run that follows it.  Three witnesses; the first hint, an INV0, reads an input that
    is never assigned."""
    L = H.stacked(10, 5, STACK_SHAPE)
    q, perm, hints = L["q"], L["perm"], L["hints"]
    ref = H.plan(q, perm, hints)
    assert ref["schedule"] == [[0, 3, 0], [3, 1, 1], [4, 2, 0]]
    undriven = [j for j in range(L["n"]) if not q["q_o"][j]]                  # their selectors are all zero: no public value there
    wits = [(L["assigned"], [])]
    for k in (1, 2):
        wits.append(({x: (v * (k + 1) + k) % R for x, v in L["assigned"].items()}, S.public_values(L["n"], L["n"] // 2, 70 + k, zero_rows=undriven)))
    c = _hinted(ctx, q, perm, hints)
    try:
        assert ctx.witness_solve_plan(c.cid, COSETS) == {k: ref[k] for k in ("driven_rows", "free_classes", "depth", "launches")}
        want, reports = _run(ctx, c, q, perm, hints, wits)
        assert reports == [CLEAN] * 3
        assert want[0][0][hints[0][1]] == 0
    finally:
        c.free()


def test_seventy_range_checks_at_2_5(ctx):
    n, q, perm, hints, (cx, cy) = H.range_check(5, 8)
    rng = random.Random(70)
    wits = [({cx: rng.randrange(256), cy: rng.randrange(256) if k % 2 else rng.randrange(R)}, []) for k in range(70)]
    c = _hinted(ctx, q, perm, hints)
    try:
        _, reports = _run(ctx, c, q, perm, hints, wits)
        assert [r == CLEAN for r in reports] == [(a[cx] + a[cy]) % R < 256 for a, _ in wits]
    finally:
        c.free()


def test_install_remove_reinstall_and_the_three_ways_to_the_device(ctx):
    n, q, perm, hints, (cx, cy) = H.range_check(5, 8)
    wits = [({cx: 100, cy: 55}, []), ({cx: 200, cy: 56}, [])]
    plain = Compiled(ctx, q, perm)
    c = Compiled(ctx, q, perm)
    try:
        bare_info = ctx.witness_solve_plan(plain.cid, COSETS)
        bare, _ = _solve(ctx, plain, wits)
        assert all(_same(g, S.solve(q, perm, a)) for g, (a, _) in zip(bare, wits))
        for _ in range(2):
            ctx.circuit_set_hints(c.cid, COSETS, hints)
            assert ctx.witness_solve_plan(c.cid, COSETS) == H.info(q, perm, hints)
            _run(ctx, c, q, perm, hints, wits)
            ctx.circuit_set_hints(c.cid, COSETS, [])
            assert ctx.witness_solve_plan(c.cid, COSETS) == bare_info
            got, _ = _solve(ctx, c, wits)
            assert all(np.array_equal(x, y) for g, b in zip(got, bare) for x, y in zip(g, b))
        # a set replaces the whole set
        ctx.circuit_set_hints(c.cid, COSETS, hints)
        ctx.circuit_set_hints(c.cid, COSETS, hints[:3])
        _run(ctx, c, q, perm, hints[:3], wits)
    finally:
        c.free()
        plain.free()
    for how in ("perm", "pairs", "load"):
        c = _hinted(ctx, q, perm, hints, how)
        try:
            got, reports = _solve(ctx, c, wits)
            assert all(_same(g, H.solve(q, perm, hints, a)) for g, (a, _) in zip(got, wits)), how
            assert [r["gate_failures"] for r in reports] == [0, 0] and [r["copy_failures"] for r in reports] == [0, 2], how
        finally:
            c.free()


def test_refusals_leave_the_installed_hints_in_force(ctx):
    n, q, perm, hints, (cx, cy) = H.range_check(4, 4)
    installed = hints[:2]                                                   # what stays in force throughout
    wits = [({cx: 3, cy: 5}, [])]
    lib, ks = ctx.lib, capi._cosets_arg(COSETS)
    rep = lambda i, t: hints[:i] + [t] + hints[i + 1:]   # noqa: E731
    driven_cell = 2 * n + 5
    cases = [
        ("an unknown kind", rep(2, (3, 3, 2 * n, 0, 1)), "hints[2]"),
        ("dst >= 3n", rep(3, (H.BITS, 3 * n, 2 * n, 0, 1)), "hints[3]"),
        ("src >= 3n", rep(0, (H.BITS, 1, 3 * n, 0, 1)), "hints[0]"),
        ("width 0", rep(1, (H.BITS, 2, 2 * n, 1, 0)), "hints[1]"),
        ("width 65", rep(1, (H.BITS, 2, 2 * n, 1, 65)), "hints[1]"),
        ("shift 255", rep(2, (H.BITS, 3, 2 * n, 255, 1)), "hints[2]"),
        ("dst in a driven class", rep(2, (H.BITS, driven_cell, 2 * n, 2, 1)), "hints[2]"),
        ("two hints into one class", rep(3, (H.BITS, n + 2, 2 * n, 3, 1)), "hints[3]"),
        ("the lowest offender", [hints[0], (H.BITS, 3 * n, 0, 0, 1), hints[2], (9, 0, 0, 0, 0)], "hints[1]"),
        ("src in dst's own class", installed + [(H.INV0, 12, 12, 0, 0)], "hints[2]"),
        ("two hints reading each other", installed + [(H.INV0, 12, 13, 0, 0), (H.BITS, 13, 12, 0, 8)], "hints[2]"),
        ("a hint reading a row that reads the hint", [(H.BITS, 1, 2 * n + 5, 0, 1)] + hints[1:], "row 5"),
    ]
    c = _hinted(ctx, q, perm, installed)
    outs = [ctx.alloc(n) for _ in range(3)]
    try:
        kept = ctx.witness_solve_plan(c.cid, COSETS)
        assert kept == H.info(q, perm, installed)

        def still_in_force():
            assert ctx.witness_solve_plan(c.cid, COSETS) == kept
            _run(ctx, c, q, perm, installed, wits)

        for name, bad, text in cases:
            assert H.plan(q, perm, bad)["status"] != 0, name
            with pytest.raises(capi.TyplonkError) as e:
                ctx.circuit_set_hints(c.cid, COSETS, bad)
            assert e.value.code == ERR_INVALID_ARG and text in str(e.value), (name, str(e.value))
            still_in_force()
        arr = (capi.Hint * 1)(capi.Hint(H.INV0, 12, 0, 0, 0))
        assert lib.typlonk_circuit_set_hints(ctx.h, c.cid, C.byref(ks), None, 1) == ERR_INVALID_ARG
        assert lib.typlonk_circuit_set_hints(ctx.h, c.cid, None, arr, 1) == ERR_INVALID_ARG
        assert lib.typlonk_circuit_set_hints(ctx.h, 0xFFFF, C.byref(ks), arr, 1) == ERR_INVALID_ARG
        assert lib.typlonk_circuit_set_hints(None, c.cid, C.byref(ks), arr, 1) == ERR_INVALID_ARG
        still_in_force()
        # at solve: a cell of a hinted class is refused and the outputs stay as they were
        fill = np.full((n, 4), GARBAGE, dtype=np.uint64)
        for b in outs:
            b.upload(fill)
        for cells in ([cx, 1], [n + 2, cy]):                                 # the a cell of bit 0's row, the b cell of bit 1's
            with pytest.raises(capi.TyplonkError) as e:
                ctx.witness_solve(c.cid, COSETS, cells, fr_pack([1, 1])[None], [outs])
            i = 0 if cells[0] != cx else 1
            assert e.value.code == ERR_INVALID_ARG and f"cells[{i}] lies in a hinted class: its value is computed" in str(e.value)
            assert all(np.array_equal(b.download(), fill) for b in outs)
        # bit 2 is not hinted in the installed set: its class is free again and may be assigned
        ctx.witness_solve(c.cid, COSETS, [cx, cy, 3], fr_pack([3, 5, 1])[None], [outs])
        assert _same([b.download() for b in outs], H.solve(q, perm, installed, {cx: 3, cy: 5, 3: 1}))
    finally:
        for b in outs:
            b.free()
        c.free()
    # a malformed circuit is refused as the solve refuses it
    from test_gpu_witness_check import Loaded, _scaled_roots, _sel_arrays

    m, _, q3, perm3 = W.chain_with_pi(3)
    seven = _scaled_roots(ctx, 3, [7])[0]
    bad = Loaded(ctx, 3, _sel_arrays(q3, m), perm3, patch={m + 2: seven[2]})
    try:
        with pytest.raises(capi.TyplonkError) as e:
            ctx.circuit_set_hints(bad.cid, COSETS, [(H.INV0, m - 1, 0, 0, 0)])
        assert e.value.code == ERR_INVALID_ARG and "defects" in str(e.value)
    finally:
        bad.free()


@pytest.mark.parametrize("log_n,k", [(5, 8), (6, 16)])
def test_solve_check_prove_verify(ctx, log_n, k):
    from test_gpu_compact import SECRET, _g2s

    n, q, perm, hints, (cx, cy) = H.range_check(log_n, k)
    cells = sorted([cx, cy] + list(S.blinding_cells(n)))
    c = _hinted(ctx, q, perm, hints)
    sid = ctx.srs_generate(_limbs(SECRET), n + 3)
    outs = [ctx.alloc(n) for _ in range(3)]
    try:
        vk = ctx.circuit_vk(sid, c.cid, COSETS, _g2s())
        good = {**S.blinding_cells(n), cx: (1 << k) - 9, cy: 8}
        ctx.witness_solve(c.cid, COSETS, cells, fr_pack([good[x] for x in cells])[None], [outs])
        assert _same([b.download() for b in outs], H.solve(q, perm, hints, good))
        assert ctx.witness_check(c.cid, [outs], None, None, COSETS) == [CLEAN]
        proof = ctx.prove_compact(sid, c.cid, outs, None, 0, COSETS)
        assert ctx.verify_compact(vk, [proof]).tolist() == [True]
        over = {**good, cy: 9}                                          # x + y = 2^k
        ctx.witness_solve(c.cid, COSETS, cells, fr_pack([over[x] for x in cells])[None], [outs])
        rep = ctx.witness_check(c.cid, [outs], None, None, COSETS)[0]
        assert rep["gate_failures"] == 0 and rep["copy_failures"] == 2
        with pytest.raises(capi.TyplonkError) as e:
            ctx.prove_compact(sid, c.cid, outs, None, 0, COSETS)
        assert e.value.code == ERR_UNSATISFIED
    finally:
        for b in outs:
            b.free()
        ctx.srs_free(sid)
        c.free()
