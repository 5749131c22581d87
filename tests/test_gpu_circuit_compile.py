"""typlonk_circuit_compile / _host on the GPU: a circuit compiled from selector evaluations and the permutation itself against its
twin, the same circuit loaded the long way round (test_gpu_witness_check.Loaded: w^j as the forward transform of X, k_i w^j by
typlonk_lincomb, the sigma rows spliced on the host by the Python permutation, eight inverse transforms, typlonk_circuit_load --
a path that never runs sigma_from_perm_kernel): equal commitments, equal proofs in both shapes, the same verdicts and reports; the lint of the
permutation and of the cosets; what is cached.  Python integers state every permutation, witness and expected report."""
import ctypes as C

import numpy as np
import pytest

import general_circuits as G
import witness_check_ref as W
from helpers import O
from oracle import plonk_oracle as PO
from test_gpu_prove_batch import _g2s_limbs, same
from test_gpu_prove_batch_compact import _bytes, _free, _upload
from test_gpu_witness_check import Loaded, _expected, _limbs
from typlonk_amd import capi

pytestmark = pytest.mark.gpu

R = O.R
SECRET = 2
ERR_INVALID_ARG, ERR_LENGTH, ERR_DOMAIN, ERR_RANGE = -1, -2, -3, -7
# the circuits of the sizes general_circuits.SEEDS lacks: witness_check_ref.random_circuit(log_n, seed)
OWN_SEEDS = {1: 901, 7: 907}


def circuit_of(log_n):
    """(n, cols, q, perm): general_circuits.circuit where it has the size, else random_circuit under OWN_SEEDS"""
    if log_n in G.SEEDS:
        return G.circuit(log_n)
    n, cols, q, perm, pi = W.random_circuit(log_n, OWN_SEEDS[log_n], 0)
    assert pi == [] and W.satisfied(q, perm, cols)
    return n, cols, q, perm


def _sel_words(q):
    return [W.mont_words(q[name]) for name in W.SELECTORS]


def _compile(ctx, log_n, sel, perm, cosets):
    bufs = []
    try:
        for ev in sel:
            b = ctx.alloc(len(ev))
            bufs.append(b)
            b.upload(np.ascontiguousarray(ev))
        return ctx.circuit_compile(log_n, bufs, perm, cosets)
    finally:
        for b in bufs:
            b.free()


class Pair:
    """a circuit compiled from (q, perm) and its twin loaded through typlonk_circuit_load, over one SRS of secret 2"""

    def __init__(self, ctx, log_n, ks):
        self.ctx, self.log_n, self.ks = ctx, log_n, tuple(ks)
        self.n, self.cols, self.q, self.perm = circuit_of(log_n)
        assert G.cosets_are_disjoint(self.ks, self.n)
        sel = _sel_words(self.q)
        self.twin = Loaded(ctx, log_n, sel, self.perm, self.ks)
        self.cosets = self.twin.cosets
        self.cid = _compile(ctx, log_n, sel, self.perm, self.cosets)
        self.sid = ctx.srs_generate(_limbs(SECRET), self.n + 3)

    def free(self):
        self.ctx.circuit_free(self.cid)
        self.twin.free()
        self.ctx.srs_free(self.sid)


@pytest.fixture(scope="module")
def pairs(ctx):
    made = {}

    def get(log_n, ones=False):
        if (log_n, ones) not in made:
            made[log_n, ones] = Pair(ctx, log_n, G.large_cosets(log_n) if ones else PO.COSETS)
        return made[log_n, ones]

    yield get
    for p in made.values():
        p.free()


TWIN_CASES = [(1, False), (3, False), (4, False), (4, True), (5, False), (6, False), (7, False), (12, False)]


@pytest.mark.parametrize("log_n,ones", TWIN_CASES)
def test_compiled_circuit_equals_its_loaded_twin(ctx, pairs, log_n, ones):
    """3n cells: 6 (one partial block), 24 .. 192, 384 (two 256-thread blocks, the last partial), 12288 (both table halves
    2^6); (4, True): cosets (1, k1, k2)"""
    p = pairs(log_n, ones)
    n = p.n
    assert p.ks[0] == (1 if ones else 2)
    # the eight commitments
    got, exp = ctx.circuit_commitments(p.sid, p.cid), ctx.circuit_commitments(p.sid, p.twin.cid)
    assert len(got) == len(exp) == 8
    for i in range(8):
        assert (got[i][0] == exp[i][0]).all() and got[i][1] == exp[i][1], i
    # both provers, every field, challenges included
    words = [W.mont_words(col) for col in p.cols]
    bufs, pibs = _upload(ctx, n, [(words, [])])
    try:
        a, b = (ctx.prove_native(p.sid, cid, bufs[0], None, p.cosets) for cid in (p.cid, p.twin.cid))
        assert same(a, b) and not np.asarray(a["evals"][5]).any()
        ca, cb = (ctx.prove_compact(p.sid, cid, bufs[0], None, 0, p.cosets) for cid in (p.cid, p.twin.cid))
        assert _bytes(ca) == _bytes(cb)
        vk = ctx.circuit_vk(p.sid, p.twin.cid, p.cosets, _g2s_limbs(SECRET))
        assert ctx.verify_compact(vk, [ca], pi=[None]).tolist() == [True]
        # the permutation the circuit keeps
        perm, defects = ctx.circuit_permutation(p.cid, n, p.cosets)
        assert perm.tolist() == p.perm and defects == 0
        # the witness check: honest
        clean = {"gate_failures": 0, "copy_failures": 0, "gate_rows": [], "copy_cells": []}
        for cid in (p.cid, p.twin.cid):
            assert ctx.witness_check(cid, bufs, None, None, p.cosets, cap=16) == [clean]
    finally:
        _free(bufs, pibs)
    # ... a cell of a fixed point changed: its gate row alone
    bad, row = G.break_gate_only(p.perm, p.cols)
    broken = [(bad, [], ([row], []))]
    # ... one cell of a 2-cycle changed under public values on every row: the pair's two copy constraints alone
    full_cols, full_pi = G.witness(p.q, p.perm, p.cols, 5000 + log_n, n)
    bad, bad_pi, cells = G.break_copy_only(p.q, p.perm, full_cols, full_pi)
    broken.append((bad, bad_pi, ([], cells)))
    for cols, pi, want in broken:
        assert W.check(p.q, p.perm, cols, pi) == want
        bufs, pibs = _upload(ctx, n, [([W.mont_words(col) for col in cols], pi)])
        try:
            reps = [ctx.witness_check(cid, bufs, pibs, [len(pi)], p.cosets, cap=16) for cid in (p.cid, p.twin.cid)]
        finally:
            _free(bufs, pibs)
        assert reps[0] == reps[1] == [_expected(p.q, p.perm, cols, pi, 16)]


def test_host_form_equals_the_buffer_form(ctx, pairs):
    p = pairs(5)
    cid = ctx.circuit_compile_host(5, _sel_words(p.q), p.perm, p.cosets)
    try:
        got, exp = ctx.circuit_commitments(p.sid, cid), ctx.circuit_commitments(p.sid, p.cid)
        assert all((got[i][0] == exp[i][0]).all() and got[i][1] == exp[i][1] for i in range(8))
        perm, defects = ctx.circuit_permutation(cid, p.n, p.cosets)
        assert perm.tolist() == p.perm and defects == 0
    finally:
        ctx.circuit_free(cid)


def test_null_perm_is_the_identity(ctx, pairs):
    """and the default cosets of the Python layer are (2, 3, 4)"""
    p = pairs(4)
    sel = _sel_words(p.q)
    ids = [_compile(ctx, 4, sel, None, None), _compile(ctx, 4, sel, list(range(3 * p.n)), p.cosets)]
    try:
        a, b = (ctx.circuit_commitments(p.sid, cid) for cid in ids)
        assert all((a[i][0] == b[i][0]).all() and a[i][1] == b[i][1] for i in range(8))
        c = ctx.circuit_commitments(p.sid, p.cid)
        assert all((a[i][0] == c[i][0]).all() for i in range(5)) and not any((a[i][0] == c[i][0]).all() for i in range(5, 8))
        for cid in ids:
            perm, defects = ctx.circuit_permutation(cid, p.n, p.cosets)
            assert perm.tolist() == list(range(3 * p.n)) and defects == 0
    finally:
        for cid in ids:
            ctx.circuit_free(cid)


def test_squaring_chain_at_2_16_from_its_permutation(ctx):
    """structural: the chain's permutation written with numpy (a_0 <-> b_0; c_j -> a_{j+1} -> b_{j+1} -> c_j for j <= g - 2),
    its selector evaluations from SquaringChain; 3n > 2^16 cells, table halves 2^8"""
    from typlonk_amd.circuits import SquaringChain

    log_n = 16
    chain = SquaringChain(ctx, log_n, keep_host=True)
    n, g = chain.n, chain.gates
    perm = np.arange(3 * n, dtype=np.uint32)
    j = np.arange(g - 1, dtype=np.uint32)
    perm[0], perm[n] = n, 0
    perm[2 * n + j] = j + 1
    perm[j + 1] = n + j + 1
    perm[n + j + 1] = 2 * n + j
    assert np.array_equal(np.sort(perm), np.arange(3 * n))
    sid = ctx.srs_generate(_limbs(SECRET), n + 3)
    cid = _compile(ctx, log_n, chain.host_inputs()["selectors"], perm, chain.cosets)
    try:
        got, exp = ctx.circuit_commitments(sid, cid), ctx.circuit_commitments(sid, chain.circuit)
        assert all((got[i][0] == exp[i][0]).all() and got[i][1] == exp[i][1] for i in range(8))
        a, b = (ctx.prove_compact(sid, c, chain.wire_evals, None, 0, chain.cosets) for c in (cid, chain.circuit))
        assert _bytes(a) == _bytes(b)
    finally:
        ctx.circuit_free(cid)
        ctx.srs_free(sid)
        chain.free()


# ---- lint ----------------------------------------------------------------------------------------------------------------------
class Raw:
    """typlonk_circuit_compile / _host called through ctypes, outputs pre-filled: (rc, circuit id, defects, last error)"""

    def __init__(self, ctx, log_n, q):
        self.ctx, self.n = ctx, 1 << log_n
        self.words = [np.ascontiguousarray(w) for w in _sel_words(q)]
        self.bufs = [ctx.alloc(self.n) for _ in range(5)]
        for b, w in zip(self.bufs, self.words):
            b.upload(w)

    def free(self):
        for b in self.bufs:
            b.free()

    def call(self, log_n, perm, cosets, bufs=None, host=False, rows=None):
        ctx = self.ctx
        cid, defects = C.c_uint32(0xA5A5), C.c_uint64(0xA5A5)
        pp = np.ascontiguousarray(perm, dtype=np.uint32)
        ks = capi._cosets_arg(cosets)
        if host:
            sel = (C.POINTER(C.c_uint64) * 5)(*[capi._u64p(w) for w in self.words])
            rc = ctx.lib.typlonk_circuit_compile_host(ctx.h, sel, self.n if rows is None else rows, pp.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                      C.byref(ks), log_n, C.byref(cid), C.byref(defects))
        else:
            sel = (C.c_void_p * 5)(*[b.handle.value for b in (bufs or self.bufs)])
            rc = ctx.lib.typlonk_circuit_compile(ctx.h, sel, pp.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(ks), log_n,
                                                 C.byref(cid), C.byref(defects))
        return rc, cid.value, defects.value, ctx.lib.typlonk_last_error(ctx.h).decode()


def _raw_limbs(x):
    return np.array([(x >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)


def test_lint_refuses_and_leaves_the_context_alone(ctx, pairs):
    log_n = 5
    p = pairs(log_n)
    n, perm = p.n, p.perm
    raw = Raw(ctx, log_n, p.q)
    short = ctx.alloc(n - 1)
    w = O.domain_root(log_n)
    try:
        def works():
            rc, cid, defects, _ = raw.call(log_n, perm, p.cosets)
            assert rc == 0 and defects == 0 and cid != 0xA5A5
            got, d = ctx.circuit_permutation(cid, n, p.cosets)
            assert got.tolist() == perm and d == 0
            ctx.circuit_free(cid)
            return cid

        first = works()
        # one entry that is no cell: the cell without an image, and its orphaned target
        x = n + 2
        for none in (3 * n, 0xFFFFFFFF):
            bad = list(perm)
            bad[x] = none
            rc, cid, defects, err = raw.call(log_n, bad, p.cosets)
            assert (rc, cid, defects) == (ERR_INVALID_ARG, 0xA5A5, 2) and f"cell {min(x, perm[x])})" in err, err
        # two cells with one image: that image, and the second cell's old target
        a, b = 7, 2 * n + 1
        bad = list(perm)
        bad[b] = perm[a]
        assert perm[a] != perm[b]
        for host in (False, True):
            rc, cid, defects, err = raw.call(log_n, bad, p.cosets, host=host)
            assert (rc, cid, defects) == (ERR_INVALID_ARG, 0xA5A5, 2) and f"cell {min(perm[a], perm[b])})" in err, err
        # cosets: (2, 2 w, 4) meet, a zero, a value that is not below r -- the lint does not run, *defects stays
        r_words = _raw_limbs(R)
        for what, ks in (("not disjoint", [_limbs(2), _limbs(2 * w), _limbs(4)]),
                         ("zero", [_limbs(2), _limbs(0), _limbs(4)]),
                         ("not canonical", [_limbs(2), _limbs(3), r_words])):
            for host in (False, True):
                assert raw.call(log_n, perm, ks, host=host)[:3] == (ERR_INVALID_ARG, 0xA5A5, 0xA5A5), what
        assert pow(2 * w * pow(2, -1, R) % R, n, R) == 1
        # a short selector buffer; rows != n; log_n outside 1..24
        assert raw.call(log_n, perm, p.cosets, bufs=raw.bufs[:3] + [short] + raw.bufs[4:])[:3] == (ERR_RANGE, 0xA5A5, 0xA5A5)
        for rows in (n - 1, 2 * n, 0):
            assert raw.call(log_n, perm, p.cosets, host=True, rows=rows)[:3] == (ERR_LENGTH, 0xA5A5, 0xA5A5), rows
        for bad_log in (0, 25):
            for host in (False, True):
                assert raw.call(bad_log, perm, p.cosets, host=host)[:3] == (ERR_DOMAIN, 0xA5A5, 0xA5A5), bad_log
        # no id was handed out in between, and a correct compile still works
        assert works() == first + 1
        # the Python layer raises with the count and the cell
        with pytest.raises(capi.TyplonkError) as e:
            ctx.circuit_compile(log_n, raw.bufs, bad, p.cosets)
        assert e.value.code == ERR_INVALID_ARG and "2 defects" in str(e.value) and f"cell {min(perm[a], perm[b])})" in str(e.value)
    finally:
        short.free()
        raw.free()


def test_the_compiled_permutation_is_cached_for_its_cosets(ctx, pairs):
    """What can be seen of the cache without a hook into the launches: the compiled 2^12 circuit answers
    typlonk_circuit_permutation and typlonk_witness_check under its own cosets at once; other cosets recover the map from the
    sigma values (whose ids are not theirs: defects); the original cosets then recover the same permutation again."""
    p = pairs(12)
    n = p.n
    words = [W.mont_words(col) for col in p.cols]
    bufs, pibs = _upload(ctx, n, [(words, [])])
    clean = {"gate_failures": 0, "copy_failures": 0, "gate_rows": [], "copy_cells": []}
    cid = _compile(ctx, 12, _sel_words(p.q), p.perm, p.cosets)
    try:
        assert ctx.witness_check(cid, bufs, None, None, p.cosets, cap=4) == [clean]      # the first call on the circuit
        got, defects = ctx.circuit_permutation(cid, n, p.cosets)
        assert got.tolist() == p.perm and defects == 0
        other = [_limbs(k) for k in (5, 6, 7)]
        got, defects = ctx.circuit_permutation(cid, n, other)
        assert defects != 0 and got.tolist() != p.perm
        got, defects = ctx.circuit_permutation(cid, n, p.cosets)
        assert got.tolist() == p.perm and defects == 0
        assert ctx.witness_check(cid, bufs, None, None, p.cosets, cap=4) == [clean]
    finally:
        ctx.circuit_free(cid)
        _free(bufs, pibs)


def test_compile_through_the_cpp_mirror(built):
    from test_host_mirror import _run

    out = _run("test_circuit_compile_host")
    for t in ("commitments ok", "proofs ok", "check ok", "identity ok", "lint ok", "all ok"):
        assert t in out
