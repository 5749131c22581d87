"""typlonk_permutation_from_pairs and typlonk_circuit_compile_pairs / _host on the GPU against perm_pairs_ref: the canonical
permutation word for word and the class count, for every partition of six cells, random lists, adversarial shapes at 2^12 and
2^16 rows and the row ties at 2^20; a circuit compiled from pairs against its twin compiled through typlonk_circuit_compile
from the reference's canonical permutation; every refusal.  Nothing here is compared within a tolerance."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import general_circuits as G
import perm_pairs_ref as P
import witness_check_ref as W
from helpers import O
from oracle import plonk_oracle as PO
from perm_pairs_cases import ADVERSARIAL, ONE_CLASS, adversarial
from test_gpu_circuit_compile import _compile, _sel_words, circuit_of
from test_gpu_prove_batch import _g2s_limbs, same
from test_gpu_prove_batch_compact import _bytes, _free, _upload
from test_gpu_witness_check import _expected, _limbs
from typlonk_amd import capi

pytestmark = pytest.mark.gpu

SECRET = 2
ERR_INVALID_ARG, ERR_LENGTH, ERR_DOMAIN, ERR_RANGE = -1, -2, -3, -7
U32P = C.POINTER(C.c_uint32)


def check(ctx, log_n, pairs, want=None):
    """the library's (perm, classes) of `pairs` equals the reference's (or `want`); returns it"""
    cells = 3 << log_n
    arr = P.pairs_array(pairs)
    if want is None:
        want = P.canonical(cells, arr.tolist())
    perm, classes = ctx.permutation_from_pairs(log_n, arr)
    assert perm.dtype == np.uint32 and perm.shape == (cells,)
    assert classes == want[1] and np.array_equal(perm, want[0])
    return perm, classes


# ---- six cells: every partition -------------------------------------------------------------------------------------------
def set_partitions(items):
    if not items:
        yield []
        return
    first, rest = items[0], items[1:]
    for part in set_partitions(rest):
        yield [[first]] + part
        for i in range(len(part)):
            yield part[:i] + [[first] + part[i]] + part[i + 1:]


def test_every_partition_of_six_cells(ctx):
    rng = random.Random(1906)
    parts = list(set_partitions(list(range(6))))
    assert len(parts) == 203
    for part in parts:
        pairs = []
        for block in part:            # a random spanning tree of the block, each edge in a random orientation
            order = list(block)
            rng.shuffle(order)
            for i in range(1, len(order)):
                e = (order[i], order[rng.randrange(i)])
                pairs.append(e if rng.random() < 0.5 else e[::-1])
        pairs += [rng.choice(pairs) for _ in range(len(pairs) // 2 + 1)] if pairs else []
        pairs += [(x, x) for x in rng.sample(range(6), 2)]
        rng.shuffle(pairs)
        want = list(range(6))
        for block in part:
            b = sorted(block)
            for i, x in enumerate(b):
                want[x] = b[(i + 1) % len(b)]
        perm, classes = check(ctx, 1, pairs)
        assert perm.tolist() == want and classes == len(part), part


# ---- random lists ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [3, 4, 5, 6, 7])
def test_random_lists_and_their_rearrangements(ctx, log_n):
    n, cells = 1 << log_n, 3 << log_n
    rng = random.Random(1910 + log_n)
    for count in (1, n, 3 * n, 10 * n):
        fresh = count - count // 5                       # a fifth of the list repeats earlier pairs
        pairs = [(rng.randrange(cells), rng.randrange(cells)) for _ in range(fresh)]
        pairs += [rng.choice(pairs) for _ in range(count - fresh)]
        for i in rng.sample(range(count), count // 8):   # self-pairs mixed in
            pairs[i] = (pairs[i][0], pairs[i][0])
        rng.shuffle(pairs)
        perm, classes = check(ctx, log_n, pairs)
        again, classes2 = check(ctx, log_n, [(b, a) for a, b in reversed(pairs)])
        assert again.tobytes() == perm.tobytes() and classes2 == classes


# ---- adversarial shapes ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(shape, log_n):
    cells = 3 << log_n
    if shape in ONE_CLASS:
        return (np.arange(1, cells + 1, dtype=np.uint32) % cells).astype(np.uint32), 1
    return P.canonical(cells, adversarial(shape, cells).tolist())


@pytest.mark.parametrize("shape", ADVERSARIAL)
@pytest.mark.parametrize("log_n", [12, 16])
def test_adversarial_shapes(ctx, log_n, shape):
    """12,288 cells: three tiles of the sort, two passes; 196,608 cells: 48 tiles, an 18-bit key in three passes, hundreds of
    workgroups hooking into one class"""
    cells = 3 << log_n
    want = reference(shape, log_n)
    if shape == "strided_hypercube" and log_n == 16:
        assert want[1] == 3281
    if shape == "low_digit_classes":
        assert want[1] == 256
    check(ctx, log_n, adversarial(shape, cells), want)


def test_one_class_reference_is_the_references():
    """the closed form the one-class shapes are held against is what perm_pairs_ref gives"""
    cells = 3 << 12
    for shape in ("path_shuffled", "star_top"):
        perm, classes = P.canonical(cells, adversarial(shape, cells).tolist())
        want = reference(shape, 12)
        assert classes == want[1] and np.array_equal(perm, want[0])


def test_row_ties_at_2_20(ctx):
    """(j, j + n), (j + n, j + 2n) for every row j: n classes of three, a 22-bit key, the whole-chip grid"""
    from conftest import need_resources

    need_resources(host_gib=1, hbm_gib=1)
    log_n = 20
    n = 1 << log_n
    j = np.arange(n, dtype=np.uint32)
    pairs = np.concatenate([np.stack([j, j + n], axis=1), np.stack([j + n, j + 2 * n], axis=1)])
    want = ((np.arange(3 * n, dtype=np.uint64) + n) % (3 * n)).astype(np.uint32)
    check(ctx, log_n, pairs, (want, n))


# ---- compile from pairs ---------------------------------------------------------------------------------------------------
def _compile_pairs(ctx, log_n, sel, pairs, cosets):
    bufs = []
    try:
        for ev in sel:
            b = ctx.alloc(len(ev))
            bufs.append(b)
            b.upload(np.ascontiguousarray(ev))
        return ctx.circuit_compile_pairs(log_n, bufs, pairs, cosets)
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("log_n,ones", [(1, False), (4, False), (4, True), (7, False), (12, False)])
def test_compiled_from_pairs_equals_compiled_from_the_canonical_permutation(ctx, log_n, ones):
    n, cols, q, perm = circuit_of(log_n)
    ks = G.large_cosets(log_n) if ones else PO.COSETS
    assert G.cosets_are_disjoint(ks, n)
    cosets = [_limbs(k) for k in ks]
    pairs = [(x, y) for x, y in enumerate(perm) if x != y]
    cperm_arr, want_classes = P.canonical(3 * n, pairs)
    cperm = cperm_arr.tolist()
    assert sorted(map(sorted, W.cycles_of(cperm))) == sorted(map(sorted, W.cycles_of(perm))) and W.satisfied(q, cperm, cols)
    sel = _sel_words(q)
    cid, classes = _compile_pairs(ctx, log_n, sel, pairs, cosets)
    twin = _compile(ctx, log_n, sel, cperm, cosets)
    host, host_classes = ctx.circuit_compile_pairs_host(log_n, sel, pairs, cosets)
    sid = ctx.srs_generate(_limbs(SECRET), n + 3)
    bufs, pibs = _upload(ctx, n, [([W.mont_words(col) for col in cols], [])])
    try:
        assert classes == host_classes == want_classes
        exp = ctx.circuit_commitments(sid, twin)
        for other in (cid, host):
            got = ctx.circuit_commitments(sid, other)
            assert all((got[i][0] == exp[i][0]).all() and got[i][1] == exp[i][1] for i in range(8))
        g2s = _g2s_limbs(SECRET)
        vk, vk_twin = (capi.vk_to_bytes(ctx.circuit_vk(sid, c, cosets, g2s)) for c in (cid, twin))
        assert vk == vk_twin
        a, b = (ctx.prove_native(sid, c, bufs[0], None, cosets) for c in (cid, twin))
        assert same(a, b)
        ca, cb = (ctx.prove_compact(sid, c, bufs[0], None, 0, cosets) for c in (cid, twin))
        assert _bytes(ca) == _bytes(cb)
        assert ctx.verify_compact(ctx.circuit_vk(sid, cid, cosets, g2s), [ca], pi=[None]).tolist() == [True]
        for c in (cid, host):
            got, defects = ctx.circuit_permutation(c, n, cosets)
            assert got.tolist() == cperm and defects == 0
        clean = {"gate_failures": 0, "copy_failures": 0, "gate_rows": [], "copy_cells": []}
        assert ctx.witness_check(cid, bufs, None, None, cosets, cap=16) == [clean]
    finally:
        _free(bufs, pibs)
    try:
        # one cell of a 2-cycle changed under public values on every row: the pair's two copy constraints alone
        full_cols, full_pi = G.witness(q, cperm, cols, 5100 + log_n, n)
        bad, bad_pi, cells = G.break_copy_only(q, cperm, full_cols, full_pi)
        assert W.check(q, cperm, bad, bad_pi) == ([], cells)
        bufs, pibs = _upload(ctx, n, [([W.mont_words(col) for col in bad], bad_pi)])
        try:
            assert ctx.witness_check(cid, bufs, pibs, [len(bad_pi)], cosets, cap=16) == [_expected(q, cperm, bad, bad_pi, 16)]
        finally:
            _free(bufs, pibs)
    finally:
        for c in (cid, twin, host):
            ctx.circuit_free(c)
        ctx.srs_free(sid)


def test_no_pairs_is_compile_with_a_null_perm(ctx):
    log_n = 4
    n, cols, q, perm = circuit_of(log_n)
    sel = _sel_words(q)
    cosets = [_limbs(k) for k in PO.COSETS]
    sid = ctx.srs_generate(_limbs(SECRET), n + 3)
    a, classes = _compile_pairs(ctx, log_n, sel, np.zeros((0, 2), dtype=np.uint32), cosets)
    b = _compile(ctx, log_n, sel, None, cosets)
    try:
        assert classes == 3 * n
        x, y = ctx.circuit_commitments(sid, a), ctx.circuit_commitments(sid, b)
        assert all((x[i][0] == y[i][0]).all() and x[i][1] == y[i][1] for i in range(8))
        got, defects = ctx.circuit_permutation(a, n, cosets)
        assert got.tolist() == list(range(3 * n)) and defects == 0
        perm0, classes0 = ctx.permutation_from_pairs(log_n, np.zeros((0, 2), dtype=np.uint32))
        assert perm0.tolist() == list(range(3 * n)) and classes0 == 3 * n
    finally:
        ctx.circuit_free(a)
        ctx.circuit_free(b)
        ctx.srs_free(sid)


# ---- refusals -------------------------------------------------------------------------------------------------------------
class RawPairs:
    """the three entry points through ctypes, outputs pre-filled"""

    FILL = 0xA5A5A5A5

    def __init__(self, ctx, log_n, q):
        self.ctx, self.log_n, self.n = ctx, log_n, 1 << log_n
        self.words = [np.ascontiguousarray(w) for w in _sel_words(q)]
        self.bufs = [ctx.alloc(self.n) for _ in range(5)]
        for b, w in zip(self.bufs, self.words):
            b.upload(w)
        self.ks = capi._cosets_arg([_limbs(k) for k in PO.COSETS])

    def free(self):
        for b in self.bufs:
            b.free()

    @staticmethod
    def _ptr(pairs):
        if pairs is None:
            return None, None
        keep = np.ascontiguousarray(pairs, dtype=np.uint32)
        return keep, keep.ctypes.data_as(U32P)

    def perm(self, pairs, count, log_n=None):
        """(rc, perm untouched?, classes, last error)"""
        ctx, log_n = self.ctx, self.log_n if log_n is None else log_n
        keep, pp = self._ptr(pairs)
        out = np.full(3 * self.n, self.FILL, dtype=np.uint32)
        classes = C.c_uint64(self.FILL)
        rc = ctx.lib.typlonk_permutation_from_pairs(ctx.h, pp, count, log_n, out.ctypes.data_as(U32P), C.byref(classes))
        return rc, bool((out == self.FILL).all()), classes.value, ctx.lib.typlonk_last_error(ctx.h).decode()

    def compile(self, pairs, count, log_n=None, bufs=None, host=False, rows=None):
        """(rc, circuit id, classes, last error)"""
        ctx, log_n = self.ctx, self.log_n if log_n is None else log_n
        keep, pp = self._ptr(pairs)
        cid, classes = C.c_uint32(self.FILL), C.c_uint64(self.FILL)
        if host:
            sel = (C.POINTER(C.c_uint64) * 5)(*[capi._u64p(w) for w in self.words])
            rc = ctx.lib.typlonk_circuit_compile_pairs_host(ctx.h, sel, self.n if rows is None else rows, pp, count, C.byref(self.ks),
                                                            log_n, C.byref(cid), C.byref(classes))
        else:
            sel = (C.c_void_p * 5)(*[b.handle.value for b in (bufs or self.bufs)])
            rc = ctx.lib.typlonk_circuit_compile_pairs(ctx.h, sel, pp, count, C.byref(self.ks), log_n, C.byref(cid), C.byref(classes))
        return rc, cid.value, classes.value, ctx.lib.typlonk_last_error(ctx.h).decode()


def test_refusals_leave_everything_alone(ctx):
    log_n = 5
    n, cols, q, perm = circuit_of(log_n)
    cells = 3 * n
    raw = RawPairs(ctx, log_n, q)
    FILL = raw.FILL
    short = ctx.alloc(n - 1)
    good = [(x, y) for x, y in enumerate(perm) if x != y]
    count = len(good)
    assert count >= 9
    want = P.canonical(cells, good)
    try:
        def works():
            check(ctx, log_n, good, want)
            rc, cid, classes, _ = raw.compile(good, count)
            assert rc == 0 and classes == want[1] and cid != FILL
            got, d = ctx.circuit_permutation(cid, n, [_limbs(k) for k in PO.COSETS])
            assert np.array_equal(got, want[0]) and d == 0
            ctx.circuit_free(cid)
            return cid

        first = works()
        # a cell that is not below 3n, in the first, a middle and the last pair, on either side
        for bad_cell in (cells, 0xFFFFFFFF):
            for at in (0, count // 2, count - 1):
                for side in (0, 1):
                    bad = [list(p) for p in good]
                    bad[at][side] = bad_cell
                    msg = f"1 pairs name a cell that is not below 3n = {cells}, the lowest is pair {at} with cell {bad_cell}"
                    rc, untouched, classes, err = raw.perm(bad, count)
                    assert (rc, untouched, classes) == (ERR_INVALID_ARG, True, FILL) and msg in err, err
                    for host in (False, True):
                        rc, cid, classes, err = raw.compile(bad, count, host=host)
                        assert (rc, cid, classes) == (ERR_INVALID_ARG, FILL, FILL) and msg in err, err
                    works()           # straight afterwards, on the same context
        # two bad pairs: the lower one is named
        bad = [list(p) for p in good]
        bad[count - 2][1], bad[3][0] = cells + 7, cells
        rc, untouched, classes, err = raw.perm(bad, count)
        assert (rc, untouched, classes) == (ERR_INVALID_ARG, True, FILL)
        assert "2 pairs name" in err and f"the lowest is pair 3 with cell {cells}" in err, err
        # what is refused before a pair is read
        assert raw.perm(None, 3)[:3] == (ERR_INVALID_ARG, True, FILL)
        assert raw.compile(None, 3)[:3] == (ERR_INVALID_ARG, FILL, FILL)
        two = [(0, 1)]
        assert raw.perm(two, 1 << 32)[:3] == (ERR_LENGTH, True, FILL)       # 2^32 pairs "in" a two-entry array: never read
        for host in (False, True):
            assert raw.compile(two, 1 << 32, host=host)[:3] == (ERR_LENGTH, FILL, FILL)
        for bad_log in (0, capi_max_log_n() + 1):
            assert raw.perm(good, count, log_n=bad_log)[:3] == (ERR_DOMAIN, True, FILL)
            for host in (False, True):
                assert raw.compile(good, count, log_n=bad_log, host=host)[:3] == (ERR_DOMAIN, FILL, FILL)
        # the compile's own: a short selector buffer; rows != n
        assert raw.compile(good, count, bufs=raw.bufs[:3] + [short] + raw.bufs[4:])[:3] == (ERR_RANGE, FILL, FILL)
        for rows in (n - 1, 2 * n, 0):
            assert raw.compile(good, count, host=True, rows=rows)[:3] == (ERR_LENGTH, FILL, FILL), rows
        # no id was handed out in between
        assert works() == first + 13
        # the Python layer: shapes that are no (count, 2)
        for shape in ([1, 2, 3], [[1, 2, 3]], [[[1, 2]]], 7):
            with pytest.raises(ValueError):
                ctx.permutation_from_pairs(log_n, shape)
            with pytest.raises(ValueError):
                ctx.circuit_compile_pairs(log_n, raw.bufs, shape)
        with pytest.raises(capi.TyplonkError) as e:
            ctx.permutation_from_pairs(log_n, [(0, cells)])
        assert e.value.code == ERR_INVALID_ARG and "pair 0 with cell" in str(e.value)
    finally:
        short.free()
        raw.free()


def capi_max_log_n():
    """TYPLONK_MAX_PROVER_LOG_N as the header states it"""
    import os
    import re

    from helpers import ROOT

    return int(re.search(r"#define TYPLONK_MAX_PROVER_LOG_N (\d+)", open(os.path.join(ROOT, "include", "typlonk.h")).read()).group(1))


# ---- the C++ mirror ---------------------------------------------------------------------------------------------------------
def test_compile_from_pairs_through_the_cpp_mirror(built):
    from test_host_mirror import _run

    out = _run("test_circuit_pairs_host")
    for t in ("commitments ok", "proofs ok", "check ok", "refusal ok", "all ok"):
        assert t in out
    lines = {k: v.split() for k, _, v in (line.partition(":") for line in out.splitlines()) if _}
    flat = [int(v) for v in lines["pairs"]]
    pairs = list(zip(flat[::2], flat[1::2]))
    perm, classes = P.canonical(24, pairs)
    assert [int(v) for v in lines["perm"]] == perm.tolist() and int(lines["classes"][0]) == classes
    assert 0 < len(pairs) and classes < 24
