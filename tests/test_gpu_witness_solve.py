"""typlonk_witness_solve_plan / typlonk_witness_solve on the GPU: the columns equal the Python statement of the contract
(tests/witness_solve_ref.py) word for word, and typlonk_witness_check on the solved buffers reports what the Python checker
reports on the reference's columns.  Chains (one narrow run of n - 3 levels; at 2^17 two runs, across the 65,536-level cut),
layered circuits whose narrow runs and wide launches alternate, several witnesses per call, public values, unassigned free
classes, tied pairs, the three ways a circuit reaches the device, every refusal, and solve -> check -> prove -> verify.

The number of launches of a call cannot be observed from outside: what is held here is that the plan the library reports
(driven rows, free classes, depth, launches) is the Python statement's, whose schedule tests/test_solve_plan_host.py holds
against the very header the library queues its launches from, and that a second call returns the same words."""
import ctypes as C

import numpy as np
import pytest

import witness_check_ref as W
import witness_solve_ref as S
from helpers import O, fr_pack
from oracle import plonk_oracle as PO
from typlonk_amd import capi

pytestmark = pytest.mark.gpu

R = O.R
ERR_INVALID_ARG, ERR_LENGTH, ERR_RANGE, ERR_UNSATISFIED = -1, -2, -7, -8
CLEAN = {"gate_failures": 0, "copy_failures": 0, "gate_rows": [], "copy_cells": []}
GARBAGE = 0xA5A5A5A5A5A5A5A5


def _limbs(v):
    return np.array(O.fr_to_mont_limbs(v % R), dtype=np.uint64)


COSETS = [_limbs(k) for k in PO.COSETS]


def _selector_bufs(ctx, q):
    bufs = []
    for name in W.SELECTORS:
        b = ctx.alloc(len(q[name]))
        b.upload(W.mont_words(q[name]))
        bufs.append(b)
    return bufs


class Compiled:
    """a circuit on the device through typlonk_circuit_compile (how="perm"), typlonk_circuit_compile_pairs ("pairs") or
    typlonk_circuit_load ("load": the permutation is recovered from the sigma values), under the cosets `cosets` (integers);
    .cosets = their limbs, which _solve passes on"""

    def __init__(self, ctx, q, perm, how="perm", cosets=PO.COSETS):
        self.ctx, self.n = ctx, len(perm) // 3
        log_n = self.n.bit_length() - 1
        self.loaded = None
        self.cosets = [_limbs(k) for k in cosets]
        if how == "load":
            from test_gpu_witness_check import Loaded, _sel_arrays

            self.loaded = Loaded(ctx, log_n, _sel_arrays(q, self.n), perm, cosets)
            self.cid = self.loaded.cid
            return
        sel = _selector_bufs(ctx, q)
        try:
            if how == "pairs":
                self.cid, _ = ctx.circuit_compile_pairs(log_n, sel, [(x, y) for x, y in enumerate(perm) if x != y] or np.zeros((0, 2)),
                                                        self.cosets)
            else:
                self.cid = ctx.circuit_compile(log_n, sel, perm, self.cosets)
        finally:
            for b in sel:
                b.free()

    def free(self):
        self.ctx.circuit_free(self.cid)


def _solve(ctx, c, wits, garbage=3, raw_pi=False):
    """wits = [(assigned {cell: value}, pi)] over one set of cells -> (the solved columns as (n, 4) word arrays per witness, the
    check's reports on the very buffers).  The public values are residues, uploaded as their canonical words; with raw_pi they
    are raw values below 2^256 and go up as they are (a word w stands for w * 2^-256 mod r), with the largest words behind
    them.  Solve and check run under c.cosets."""
    n, cosets = c.n, c.cosets
    cells = sorted(wits[0][0])
    values = np.stack([fr_pack([a[x] % R for x in cells]) if cells else np.zeros((0, 4), dtype=np.uint64) for a, _ in wits])
    fill = np.full((n, 4), GARBAGE, dtype=np.uint64)
    outs, pibs = [], []
    try:
        for _, pi in wits:
            bs = [ctx.alloc(n) for _ in range(3)]
            for b in bs:
                b.upload(fill)
            outs.append(bs)
            pb = None
            if len(pi):
                pb = ctx.alloc(len(pi) + garbage)
                if raw_pi:
                    pb.upload(W.raw_words(list(pi) + [(1 << 256) - 1 - i for i in range(garbage)]))
                else:
                    pb.upload(W.mont_words(list(pi) + [0xBAD] * garbage))
            pibs.append(pb)
        lens = [len(pi) for _, pi in wits]
        ctx.witness_solve(c.cid, cosets, cells, values, outs, pibs, lens)
        got = [[b.download() for b in bs] for bs in outs]
        reports = ctx.witness_check(c.cid, outs, pibs, lens, cosets, cap=8)
        return got, reports
    finally:
        for b in [b for bs in outs for b in bs] + [b for b in pibs if b is not None]:
            b.free()


def _words(cols):
    return [W.mont_words(col) for col in cols]


def _same(got, cols):
    return all(np.array_equal(g, w) for g, w in zip(got, _words(cols)))


def _expected(q, perm, cols, pi, cap=8):
    gate, copy = W.check(q, perm, cols, pi)
    return {"gate_failures": len(gate), "copy_failures": len(copy), "gate_rows": gate[:cap], "copy_cells": copy[:cap]}


# ---- chains --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [3, 4, 5, 6, 10])
def test_the_chain_is_one_narrow_run(ctx, log_n):
    n, q, perm, assigned, cols = S.chain(log_n)
    c = Compiled(ctx, q, perm)
    try:
        info = ctx.witness_solve_plan(c.cid, COSETS)
        assert info == {"driven_rows": n - 3, "free_classes": 10, "depth": n - 3, "launches": 2}
        got, reports = _solve(ctx, c, [(assigned, [])])
        assert _same(got[0], cols) and reports == [CLEAN]
    finally:
        c.free()


def test_the_chain_at_2_17_crosses_the_run_cut(ctx):
    n, q, perm, assigned, cols = S.chain(17, S.public_values(1 << 17, 70000, 17))
    pi = S.public_values(n, 70000, 17)
    c = Compiled(ctx, q, perm)
    try:
        info = ctx.witness_solve_plan(c.cid, COSETS)
        assert info["depth"] == n - 3 > S.RUN_CUT and info["launches"] == 3        # 65,536 levels, the other 65,533, the fill
        got, reports = _solve(ctx, c, [(assigned, pi)])
        assert _same(got[0], cols) and reports == [CLEAN]
    finally:
        c.free()


def test_five_chain_witnesses_with_their_own_public_values(ctx):
    """count = 5 at 2^6, pi_len in {0, 1, n}; the call is repeated: the same words from the cached plan"""
    n = 64
    _, q, perm, _, _ = S.chain(6)
    wits, want = [], []
    for k, pl in enumerate((0, 1, n, 0, n)):
        pi = S.public_values(n, pl, 60 + k)
        _, _, _, assigned, cols = S.chain(6, pi, x0=3 + k)
        assigned[n - 2] = 1000 + k                                # a blinding cell of its own
        cols[0][n - 2] = 1000 + k
        wits.append((assigned, pi))
        want.append(cols)
    c = Compiled(ctx, q, perm)
    try:
        info = ctx.witness_solve_plan(c.cid, COSETS)
        for _ in range(2):
            got, reports = _solve(ctx, c, wits)
            assert all(_same(g, w) for g, w in zip(got, want)) and reports == [CLEAN] * 5
            assert ctx.witness_solve_plan(c.cid, COSETS) == info
    finally:
        c.free()


def test_seventy_witnesses_at_2_5(ctx):
    n = 32
    _, q, perm, _, _ = S.chain(5)
    wits, want = [], []
    for k in range(70):
        pi = S.public_values(n, (0, 1, n)[k % 3], 500 + k)
        _, _, _, assigned, cols = S.chain(5, pi, x0=2 + k)
        wits.append((assigned, pi))
        want.append(cols)
    c = Compiled(ctx, q, perm)
    try:
        got, reports = _solve(ctx, c, wits)
        assert all(_same(g, w) for g, w in zip(got, want)) and reports == [CLEAN] * 70
    finally:
        c.free()


# ---- layered circuits ----------------------------------------------------------------------------------------------------------
L12_WIDTHS = [255, 1, 1500, 256, 1, 257, 255, 1500]


@pytest.fixture(scope="module")
def layered12():
    return S.layered(12, 7, L12_WIDTHS)


def test_layered_2_12_alternates_narrow_runs_and_wide_launches(ctx, layered12):
    """widths 255, 1 | 1500 | 256, 1 | 257 | 255 | 1500: three runs, three wide launches, the fill.  Five witnesses: the
    circuit's own (honest but for its unequal ties), then other inputs under pi_len = 1, n, 0, n.  The last input is never
    assigned and reads 0; the blinding cells are assigned."""
    L = layered12
    n, q, perm = L["n"], L["q"], L["perm"]
    ref = S.plan(q, perm)
    assert ref["schedule"] == [[0, 2, 0], [2, 1, 1], [3, 2, 0], [5, 1, 1], [6, 1, 0], [7, 1, 1]]
    wits = [(L["assigned"], [])]
    for k, pl in enumerate((1, n, 0, n)):
        other = {x: (v + k + 1) % R if x % n < n - 3 else v for x, v in L["assigned"].items()}
        wits.append((other, S.public_values(n, pl, 120 + k)))
    want = [L["cols"]] + [S.solve(q, perm, a, pi) for a, pi in wits[1:]]
    c = Compiled(ctx, q, perm)
    try:
        info = ctx.witness_solve_plan(c.cid, COSETS)
        assert info == {k: ref[k] for k in ("driven_rows", "free_classes", "depth", "launches")} and info["launches"] == 7
        got, reports = _solve(ctx, c, wits)
        for k in range(5):
            assert _same(got[k], want[k]), k
            assert reports[k] == _expected(q, perm, want[k], wits[k][1]), k
        # the circuit's own witness: no gate fails, and the copy constraints that fail are those of the unequal ties
        assert reports[0]["gate_failures"] == 0 and reports[0]["copy_failures"] > 0
        assert {x for pair in reports[0]["copy_cells"] for x in pair} <= set(L["unequal"])
        # the unassigned input reads 0 at an operand cell of a gate row
        src, _ = S.sources(q, perm)
        slots = {src[x] for x in L["assigned"]}
        zero = [x for x in range(2 * n) if src[x] & S.FREE and src[x] not in slots and x % n < n - 3]
        assert zero and all(not got[0][x // n][x % n].any() for x in zero)
    finally:
        c.free()


def test_layered_2_13_with_a_level_of_6000_rows(ctx):
    L = S.layered(13, 13, [100, 6000, 50, 8], S.public_values(1 << 13, 1 << 13, 13))
    q, perm, pi = L["q"], L["perm"], L["pi"]
    c = Compiled(ctx, q, perm)
    try:
        assert ctx.witness_solve_plan(c.cid, COSETS)["launches"] == 4                # a run, the wide level, a run, the fill
        got, reports = _solve(ctx, c, [(L["assigned"], pi)])
        assert _same(got[0], L["cols"]) and reports == [_expected(q, perm, L["cols"], pi)]
        assert reports[0]["gate_failures"] == 0
    finally:
        c.free()


@pytest.mark.parametrize("ties", [(3, 0), (0, 3)])
def test_tied_pairs_equal_and_unequal(ctx, ties):
    L = S.layered(6, 21, [3, 1, 9, 4, 12], ties=ties)
    q, perm = L["q"], L["perm"]
    c = Compiled(ctx, q, perm)
    try:
        got, reports = _solve(ctx, c, [(L["assigned"], [])])
        assert _same(got[0], L["cols"]) and reports == [_expected(q, perm, L["cols"], [], 8)]
        if ties[1] == 0:
            assert reports == [CLEAN]
        else:
            full = ctx.witness_check_host(c.cid, [got[0]], None, COSETS, cap=3 * L["n"])[0]
            assert full["gate_failures"] == 0 and {x for pair in full["copy_cells"] for x in pair} <= set(L["unequal"])
            failing = {x for x, _ in full["copy_cells"]}
            classes = [set(cyc) for cyc in W.cycles_of(perm) if cyc[0] in L["unequal"]]
            assert len(classes) == 3 and all(cl & failing for cl in classes)
    finally:
        c.free()


def _canonical(perm):
    """the permutation typlonk_circuit_compile_pairs makes of perm's classes: every class ascending, its highest cell back to
    its lowest"""
    out = list(perm)
    for cyc in W.cycles_of(perm):
        cells = sorted(cyc)
        for u, v in zip(cells, cells[1:] + cells[:1]):
            out[u] = v
    return out


def test_the_same_words_however_the_circuit_was_made(ctx):
    """compiled from the permutation, from its classes as pairs (the library then keeps the canonical permutation of the same
    classes: the check lists a failing cell with another successor) and loaded as sigma polynomials (the permutation is
    recovered): the same columns word for word"""
    L = S.layered(6, 22, [3, 1, 9, 4, 12], S.public_values(64, 64, 22))
    for how in ("perm", "pairs", "load"):
        c = Compiled(ctx, L["q"], L["perm"], how)
        try:
            got, reports = _solve(ctx, c, [(L["assigned"], L["pi"])])
            assert _same(got[0], L["cols"]), how
            kept = _canonical(L["perm"]) if how == "pairs" else L["perm"]
            assert reports == [_expected(L["q"], kept, L["cols"], L["pi"])], how
        finally:
            c.free()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(ctx):
    L = S.layered(6, 23, [3, 1, 9, 4, 12])
    n, q, perm = L["n"], L["q"], L["perm"]
    c = Compiled(ctx, q, perm)
    lib, ks = ctx.lib, capi._cosets_arg(COSETS)
    cells = sorted(L["assigned"])
    src, _ = S.sources(q, perm)
    driven_cell = next(x for x in range(3 * n) if not src[x] & S.FREE)
    mate = next(x for x in range(3 * n) if x not in L["assigned"] and any(src[x] == src[y] for y in cells))   # of an input's class
    last = len(cells) - 1                                                       # a blinding cell: a class of its own
    outs = [ctx.alloc(n) for _ in range(3)]
    short, pib, big = ctx.alloc(n - 1), ctx.alloc(4), ctx.alloc(n + 1)
    try:
        fill = np.full((n, 4), GARBAGE, dtype=np.uint64)
        for b in outs:
            b.upload(fill)
        pib.upload(fr_pack([1, 2, 3, 4]))
        vals = np.ascontiguousarray(fr_pack([L["assigned"][x] for x in cells]))
        u32 = lambda xs: (C.c_uint32 * len(xs))(*xs)   # noqa: E731
        one = lambda v: (C.c_size_t * 1)(v)   # noqa: E731
        handles = lambda bs: (C.c_void_p * 3)(*[b.handle.value if b is not None else None for b in bs])   # noqa: E731
        w = handles(outs)

        def call(h=ctx.h, cid=c.cid, ks=C.byref(ks), cl=u32(cells), k=len(cells), v=capi._u64p(vals), pip=None, lens=None, count=1, w=w):
            return lib.typlonk_witness_solve(h, cid, ks, cl, k, v, pip, lens, count, w)

        def with_cell(i, x):
            cl = list(cells)
            cl[i] = x
            return u32(cl)

        bad_val = vals.copy()
        bad_val[2] = [0xFFFFFFFFFFFFFFFF] * 4                                   # >= r
        pi1 = (C.c_void_p * 1)(pib.handle.value)
        cases = [
            ("null context", call(h=None), ERR_INVALID_ARG, None),
            ("null cosets", call(ks=None), ERR_INVALID_ARG, None),
            ("null outputs", call(w=None), ERR_INVALID_ARG, None),
            ("null cells", call(cl=None), ERR_INVALID_ARG, None),
            ("null values", call(v=None), ERR_INVALID_ARG, None),
            ("unknown circuit", call(cid=0xFFFF), ERR_INVALID_ARG, None),
            ("a null output column", call(w=handles([outs[0], None, outs[2]])), ERR_INVALID_ARG, None),
            ("pi_len without pi", call(lens=one(2)), ERR_INVALID_ARG, None),
            ("pi_len with a null entry", call(pip=(C.c_void_p * 1)(None), lens=one(2)), ERR_INVALID_ARG, None),
            ("a cell >= 3n", call(cl=with_cell(4, 3 * n)), ERR_INVALID_ARG, "cells[4]"),
            ("a cell in a driven class", call(cl=with_cell(1, driven_cell)), ERR_INVALID_ARG, "cells[1]"),
            ("two cells of one class", call(cl=with_cell(last, mate)), ERR_INVALID_ARG, f"cells[{last}]"),
            ("a value >= r", call(v=capi._u64p(bad_val)), ERR_INVALID_ARG, "cells[2]"),
            ("a short output", call(w=handles([outs[0], short, outs[2]])), ERR_RANGE, None),
            ("a short pi buffer", call(pip=pi1, lens=one(5)), ERR_RANGE, None),
            ("pi_len > n", call(pip=(C.c_void_p * 1)(big.handle.value), lens=one(n + 1)), ERR_LENGTH, None),
        ]
        # (every call above has run already; typlonk_last_error is read for the ones that name an index by calling again)
        for name, rc, want, _ in cases:
            assert rc == want, (name, rc)
        for i, x, text in ((4, 3 * n, "cells[4]"), (1, driven_cell, "cells[1]"), (last, mate, f"cells[{last}]")):
            assert call(cl=with_cell(i, x)) == ERR_INVALID_ARG and text in lib.typlonk_last_error(ctx.h).decode()
        assert call(v=capi._u64p(bad_val)) == ERR_INVALID_ARG and "cells[2]" in lib.typlonk_last_error(ctx.h).decode()
        info = capi.SolveInfo()
        assert lib.typlonk_witness_solve_plan(ctx.h, 0xFFFF, C.byref(ks), C.byref(info)) == ERR_INVALID_ARG
        assert lib.typlonk_witness_solve_plan(ctx.h, c.cid, None, C.byref(info)) == ERR_INVALID_ARG
        assert lib.typlonk_witness_solve_plan(ctx.h, c.cid, C.byref(ks), None) == ERR_INVALID_ARG
        assert all(np.array_equal(b.download(), fill) for b in outs)
        # count = 0 is a no-op, and the same arguments are accepted once they are right
        assert call(count=0) == 0 and all(np.array_equal(b.download(), fill) for b in outs)
        assert call() == 0 and _same([b.download() for b in outs], L["cols"])
    finally:
        for b in outs + [short, pib, big]:
            b.free()
        c.free()


def test_unsolvable_and_malformed_circuits_are_refused(ctx):
    n = 8
    q = {name: [0] * n for name in W.SELECTORS}
    for j in (2, 5, 6):
        q["q_o"][j] = q["q_l"][j] = 1
    perm = list(range(3 * n))
    perm[2 * n + 5], perm[2] = 2, 2 * n + 5                              # a_2 = c_5
    perm[2 * n + 2], perm[5], perm[n + 6] = 5, n + 6, 2 * n + 2          # a_5 = b_6 = c_2
    outs = [ctx.alloc(n) for _ in range(3)]
    fill = np.full((n, 4), GARBAGE, dtype=np.uint64)
    for b in outs:
        b.upload(fill)
    c = Compiled(ctx, q, perm)
    try:
        for attempt in range(2):                                         # nothing half-built is cached
            with pytest.raises(capi.TyplonkError) as e:
                ctx.witness_solve(c.cid, COSETS, [], np.zeros((1, 0, 4), dtype=np.uint64), [outs])
            assert e.value.code == ERR_INVALID_ARG and "row 2" in str(e.value)
        with pytest.raises(capi.TyplonkError) as e:
            ctx.witness_solve_plan(c.cid, COSETS)
        assert e.value.code == ERR_INVALID_ARG and "row 2" in str(e.value)
    finally:
        c.free()
    # a loaded circuit whose sigma is no permutation of the cells: refused as the check refuses it
    from test_gpu_witness_check import Loaded, _scaled_roots, _sel_arrays

    n, _, q, perm = W.chain_with_pi(3)
    seven = _scaled_roots(ctx, 3, [7])[0]
    bad = Loaded(ctx, 3, _sel_arrays(q, n), perm, patch={n + 2: seven[2]})
    try:
        with pytest.raises(capi.TyplonkError) as e:
            ctx.witness_solve(bad.cid, COSETS, [], np.zeros((1, 0, 4), dtype=np.uint64), [outs])
        assert e.value.code == ERR_INVALID_ARG and "defects" in str(e.value)
        assert all(np.array_equal(b.download(), fill) for b in outs)
    finally:
        bad.free()
        for b in outs:
            b.free()


# ---- end to end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [5, 6])
def test_solve_check_prove_verify(ctx, log_n):
    from test_gpu_compact import SECRET, _g2s

    n = 1 << log_n
    pi = S.public_values(n, n // 2, log_n)
    L = S.layered(log_n, 30 + log_n, [3, 2, 5, 4], pi, ties=(1, 0))
    q, perm = L["q"], L["perm"]
    assert W.check(q, perm, L["cols"], pi) == ([], [])
    cells = sorted(L["assigned"])
    c = Compiled(ctx, q, perm)
    sid = ctx.srs_generate(_limbs(SECRET), n + 3)
    outs = [ctx.alloc(n) for _ in range(3)]
    pib = ctx.alloc(len(pi))
    pib.upload(W.mont_words(pi))
    try:
        vk = ctx.circuit_vk(sid, c.cid, COSETS, _g2s())
        ctx.witness_solve(c.cid, COSETS, cells, fr_pack([L["assigned"][x] for x in cells])[None], [outs], [pib], [len(pi)])
        assert ctx.witness_check(c.cid, [outs], [pib], [len(pi)], COSETS) == [CLEAN]
        proof = ctx.prove_compact(sid, c.cid, outs, pib, len(pi), COSETS)
        assert ctx.verify_compact(vk, [proof], [W.mont_words(pi)]).tolist() == [True]
        # one changed input under the same public values: solve still fills every driven row, the undriven rows no longer close
        x = min(x for x in cells if x % n < n - 3)
        other = dict(L["assigned"])
        other[x] = (other[x] + 1) % R
        ctx.witness_solve(c.cid, COSETS, cells, fr_pack([other[x] for x in cells])[None], [outs], [pib], [len(pi)])
        rep = ctx.witness_check(c.cid, [outs], [pib], [len(pi)], COSETS, cap=n)[0]
        want = S.solve(q, perm, other, pi)
        assert rep == _expected(q, perm, want, pi, n)
        assert rep["gate_failures"] > 0 and rep["copy_failures"] == 0 and set(rep["gate_rows"]) <= set(L["undriven"])
        with pytest.raises(capi.TyplonkError) as e:
            ctx.prove_compact(sid, c.cid, outs, pib, len(pi), COSETS)
        assert e.value.code == ERR_UNSATISFIED
    finally:
        for b in outs + [pib]:
            b.free()
        ctx.srs_free(sid)
        c.free()
