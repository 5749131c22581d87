"""typlonk_circuit_permutation / typlonk_witness_check / _host on the GPU: the permutation recovered from the sigma columns
equals the one the circuit was built from; malformed sigma columns are counted and refused; honest witnesses have no failure;
every corruption gives exactly the counts and the lists of the Python checker (tests/witness_check_ref.py); the verdict agrees
with the prover's; every refusal leaves the outputs alone.  Circuits reach the device as evaluations that are interpolated
there (typlonk_ntt_fr_dev), then typlonk_circuit_load."""
import ctypes as C

import numpy as np
import pytest

import witness_check_ref as W
from helpers import O, fr_pack
from oracle import frontend as F
from oracle import plonk_oracle as PO
from typlonk_amd import capi

pytestmark = pytest.mark.gpu

R = O.R
NONE = capi.CELL_NONE
ERR_INVALID_ARG, ERR_LENGTH, ERR_RANGE = -1, -2, -7


def _limbs(v):
    return np.array(O.fr_to_mont_limbs(v % R), dtype=np.uint64)


def _raw_limbs(x):
    """the integer x < 2^256 as four words, as it is (no reduction)"""
    return np.array([(x >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)


def _scaled_roots(ctx, log_n, ks):
    """k * w^j for j < n and each k: (n, 4) limb arrays made on the device (the transform of X, scaled)"""
    n = 1 << log_n
    xpoly = np.zeros((n, 4), dtype=np.uint64)
    xpoly[1] = _limbs(1)
    roots, out = ctx.alloc(n), []
    roots.upload(xpoly)
    ctx.ntt_dev(roots, log_n)
    for k in ks:
        b = ctx.alloc(n)
        ctx.lincomb_dev([roots], [_limbs(k)], n, b)
        out.append(b.download())
        b.free()
    roots.free()
    return out


class Loaded:
    """a circuit on the device: selector evaluations (five (n, 4) limb arrays) and sigma = the ids of perm's targets, with
    `patch` = {cell: limbs} written over single sigma evaluations"""

    def __init__(self, ctx, log_n, sel_evals, perm, cosets=PO.COSETS, patch=None):
        self.ctx, self.log_n, self.n = ctx, log_n, 1 << log_n
        n = self.n
        ids = np.concatenate(_scaled_roots(ctx, log_n, cosets))
        sig = ids[np.asarray(perm, dtype=np.int64)]
        for x, limbs in (patch or {}).items():
            sig[x] = limbs
        bufs = []
        for ev in list(sel_evals) + [sig[i * n:(i + 1) * n] for i in range(3)]:
            b = ctx.alloc(n)
            b.upload(np.ascontiguousarray(ev))
            ctx.ntt_dev(b, log_n, inverse=True)
            bufs.append(b)
        self.cid = ctx.circuit_load(log_n, bufs[:5], bufs[5:])
        for b in bufs:
            b.free()
        self.cosets = [_limbs(k) for k in cosets]

    def free(self):
        self.ctx.circuit_free(self.cid)


def _sel_arrays(q, n):
    return [fr_pack([v % R for v in q[name]]) for name in W.SELECTORS]


def _zero_selectors(n):
    return [np.zeros((n, 4), dtype=np.uint64)] * 5


def _program(log_n, index, with_eq=True):
    """the index-th generated program (oracle/frontend.py) that compiles to 2^log_n rows: (q, perm, unpadded witness columns)"""
    ops, found = {3: 5, 4: 12, 5: 26, 6: 56}[log_n], 0
    for seed in range(1, 200):
        prog = F.random_program(seed, 3, ops)
        if not with_eq:
            prog = [p for p in prog if p[0] != "eq"]
        try:
            rows, _, sel, perm = F.compile_circuit(F.run_program(prog), 3)
        except ValueError:
            continue
        if rows != 1 << log_n:
            continue
        if found == index:
            q = {name: [row[k] for row in sel] for k, name in enumerate(W.SELECTORS)}
            return q, perm, F.witness(F.run_program(prog), [3, 4, 5])
        found += 1
    raise AssertionError("no such program")


def _padded(adv, n, seed):
    """witness columns padded with zeros to n - 3 rows, then three random blinding rows (proof.rs:43-49)"""
    rng = np.random.default_rng(seed)
    return [list(col) + [0] * (n - 3 - len(col)) + [int(v) for v in rng.integers(1, 1 << 62, size=3)] for col in adv]


def _upload(ctx, wits, garbage=5):
    """wits = [(three columns as (n, 4) limb arrays, list of public values)] -> device columns, and pi buffers longer than
    pi_len with garbage behind the values"""
    bufs, pibs = [], []
    for cols, pi in wits:
        bs = [ctx.alloc(len(c)) for c in cols]
        for b, c in zip(bs, cols):
            b.upload(np.ascontiguousarray(c))
        bufs.append(bs)
        pb = None
        if pi:
            pb = ctx.alloc(len(pi) + garbage)
            pb.upload(fr_pack(list(pi) + [0xBAD] * garbage))
        pibs.append(pb)
    return bufs, pibs


def _free(bufs, pibs):
    for b in [b for bs in bufs for b in bs] + [b for b in pibs if b is not None]:
        b.free()


def _check(ctx, c, wits, cap=16):
    """the device form on integer witnesses [(cols, pi)]"""
    bufs, pibs = _upload(ctx, [([fr_pack([v % R for v in col]) for col in cols], pi) for cols, pi in wits])
    try:
        return ctx.witness_check(c.cid, bufs, pibs, [len(pi) for _, pi in wits], c.cosets, cap=cap)
    finally:
        _free(bufs, pibs)


def _expected(q, perm, cols, pi, cap):
    gate, copy = W.check(q, perm, cols, pi)
    return {"gate_failures": len(gate), "copy_failures": len(copy), "gate_rows": gate[:cap], "copy_cells": copy[:cap]}


# ---- recovery ----------------------------------------------------------------------------------------------------------------------
def test_recovery_of_the_identity_at_log_n_1(ctx):
    c = Loaded(ctx, 1, _zero_selectors(2), list(range(6)))
    try:
        perm, defects = ctx.circuit_permutation(c.cid, 2, c.cosets)
        assert perm.tolist() == list(range(6)) and defects == 0
    finally:
        c.free()


@pytest.mark.parametrize("log_n", [3, 4, 5, 6])
@pytest.mark.parametrize("index", [0, 1, 2])
def test_recovery_on_generated_circuits(ctx, log_n, index):
    q, perm, _ = _program(log_n, index)
    n = 1 << log_n
    c = Loaded(ctx, log_n, _sel_arrays(q, n), perm)
    try:
        got, defects = ctx.circuit_permutation(c.cid, n, c.cosets)
        assert got.tolist() == perm and defects == 0
    finally:
        c.free()


def test_recovery_over_many_blocks_at_log_n_12(ctx):
    n, _, q, perm = PO.squaring_chain(12)
    one, zero = _limbs(1), np.zeros(4, dtype=np.uint64)
    sel = [np.array([one if v else zero for v in q[name]]) for name in W.SELECTORS]
    c = Loaded(ctx, 12, sel, perm)
    try:
        got, defects = ctx.circuit_permutation(c.cid, n, c.cosets)
        assert got.tolist() == perm and defects == 0
    finally:
        c.free()


def test_recovery_of_a_random_pairing_at_log_n_16(ctx):
    """3n > 2^16 cells: an index cut to 16 bits anywhere would show"""
    n = 1 << 16
    order = np.random.default_rng(16).permutation(3 * n)
    perm = np.empty(3 * n, dtype=np.int64)
    perm[order[0::2]], perm[order[1::2]] = order[1::2], order[0::2]
    c = Loaded(ctx, 16, _zero_selectors(n), perm)
    try:
        got, defects = ctx.circuit_permutation(c.cid, n, c.cosets)
        assert np.array_equal(got.astype(np.int64), perm) and defects == 0
    finally:
        c.free()


def test_other_cosets_rebuild_the_cached_map(ctx):
    q, perm, _ = _program(5, 0)
    c = Loaded(ctx, 5, _sel_arrays(q, 32), perm, cosets=(5, 6, 7))
    try:
        _, defects = ctx.circuit_permutation(c.cid, 32, [_limbs(k) for k in PO.COSETS])
        assert defects != 0                                    # the ids of (5, 6, 7) are not those of (2, 3, 4)
        got, defects = ctx.circuit_permutation(c.cid, 32, c.cosets)
        assert got.tolist() == perm and defects == 0
        got, defects = ctx.circuit_permutation(c.cid, 32, c.cosets)     # from the cache
        assert got.tolist() == perm and defects == 0
    finally:
        c.free()


# ---- lint ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [3, 12])
def test_a_sigma_value_that_is_no_cell_id(ctx, log_n):
    """(7 / k)^n != 1 for k in {2, 3, 4} at every log_n <= 24: 7 w^j is the id of no cell"""
    n, cols, q, perm = W.chain_with_pi(log_n)
    assert all(pow(7 * pow(k, -1, R) % R, n, R) != 1 for k in PO.COSETS)
    x = n + 2                                                   # cell b_2
    seven = _scaled_roots(ctx, log_n, [7])[0]
    c = Loaded(ctx, log_n, _sel_arrays(q, n), perm, patch={x: seven[x % n]})
    try:
        got, defects = ctx.circuit_permutation(c.cid, n, c.cosets)
        exp = list(perm)
        exp[x] = NONE
        assert got.tolist() == exp and defects == 2             # the cell without an image, and its orphaned target
        with pytest.raises(capi.TyplonkError) as e:
            _check(ctx, c, [(cols, [])])
        assert e.value.code == ERR_INVALID_ARG and f"cell {min(x, perm[x])}" in str(e.value)
    finally:
        c.free()


def test_two_cells_with_one_target(ctx):
    n, cols, q, perm = W.chain_with_pi(4)
    two = _scaled_roots(ctx, 4, [2])[0]
    c = Loaded(ctx, 4, _sel_arrays(q, n), perm, patch={n + 9: two[3]})       # b_9 -> a_3, which a cell of its cycle maps to already
    try:
        got, defects = ctx.circuit_permutation(c.cid, n, c.cosets)
        assert got[n + 9] == 3 and defects == 2                 # a_3 is the image of two cells, b_9's old target of none
        with pytest.raises(capi.TyplonkError) as e:
            _check(ctx, c, [(cols, [])])
        assert e.value.code == ERR_INVALID_ARG
    finally:
        c.free()


# ---- honest witnesses ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [1, 3, 6, 12])
def test_honest_chain_witnesses_have_no_failure(ctx, log_n):
    n = 1 << log_n
    lens = (0,) if log_n == 1 else (0, 1, n)
    wits = []
    for k, pl in enumerate(lens):
        rng = np.random.default_rng(100 * log_n + k)
        pi = [int(v) for v in rng.integers(1, 1 << 60, size=min(pl, max(n - 3, 0)))] + [0] * (pl - min(pl, max(n - 3, 0)))
        bl = [[int(v) for v in rng.integers(1, 1 << 62, size=3)] for _ in range(3)]
        if log_n == 1:
            q, perm = {name: [0, 0] for name in W.SELECTORS}, list(range(6))
            cols = [[int(v) for v in rng.integers(1, 1 << 62, size=2)] for _ in range(3)]
        else:
            _, cols, q, perm = W.chain_with_pi(log_n, pi, blinders=bl)
        assert W.check(q, perm, cols, pi) == ([], [])
        wits.append((cols, pi))
    c = Loaded(ctx, log_n, _sel_arrays(q, n), perm)
    try:
        for rep in _check(ctx, c, wits):
            assert rep == {"gate_failures": 0, "copy_failures": 0, "gate_rows": [], "copy_cells": []}
    finally:
        c.free()


@pytest.mark.parametrize("log_n", [3, 4, 5, 6])
def test_generated_circuits_against_the_python_checker(ctx, log_n):
    """additions and multiplications over reused variables: honest without the assert_eq steps, and whatever the checker says
    with them (the inputs 3, 4, 5 need not meet a generated equality)"""
    n = 1 << log_n
    for with_eq in (False, True):
        q, perm, adv = _program(log_n, 1, with_eq)
        cols = _padded(adv, n, log_n)
        exp = _expected(q, perm, cols, [], 16)
        if not with_eq:
            assert exp["gate_failures"] == exp["copy_failures"] == 0
        c = Loaded(ctx, log_n, _sel_arrays(q, n), perm)
        try:
            assert _check(ctx, c, [(cols, [])]) == [exp]
        finally:
            c.free()


# ---- corruptions -------------------------------------------------------------------------------------------------------------------
def _corruptions(n, cols, pi):
    """(name, cols, pi) variants of an honest chain witness"""
    def bump(col, row):
        out = [list(c) for c in cols]
        out[col][row] = (out[col][row] + 1) % R
        return out

    yield "wire_a", bump(0, 2), pi
    yield "wire_c", bump(2, n - 5), pi
    yield "blinding_row", bump(1, n - 2), pi
    yield "wrong_public_value", cols, [pi[0] + 1] + list(pi[1:])
    yield "two_cells", [list(c) for c in bump(0, 1)[:2]] + [bump(2, 3)[2]], pi


@pytest.mark.parametrize("log_n", [3, 6])
def test_corruptions_against_the_python_checker(ctx, log_n):
    n, cols, q, perm = W.chain_with_pi(log_n, [11, 12])
    c = Loaded(ctx, log_n, _sel_arrays(q, n), perm)
    try:
        for name, bad, pi in _corruptions(n, cols, [11, 12]):
            exp = _expected(q, perm, bad, pi, 16)
            assert (exp["gate_failures"] + exp["copy_failures"] == 0) == (name == "blinding_row"), name
            assert _check(ctx, c, [(bad, pi)]) == [exp], name
    finally:
        c.free()


def test_a_cell_holding_v_plus_r_equals_v(ctx):
    n, cols, q, perm = W.chain_with_pi(4)
    c = Loaded(ctx, 4, _sel_arrays(q, n), perm)
    try:
        packed = [fr_pack(col) for col in cols]
        for col, row in ((0, 3), (2, 2), (1, 4)):                # cells of gates and of copy cycles
            v = sum(int(w) << (64 * i) for i, w in enumerate(packed[col][row]))
            assert v + R < 1 << 256
            packed[col][row] = _raw_limbs(v + R)
        bufs, pibs = _upload(ctx, [(packed, [])])
        try:
            rep = ctx.witness_check(c.cid, bufs, None, None, c.cosets)
        finally:
            _free(bufs, pibs)
        assert rep == [{"gate_failures": 0, "copy_failures": 0, "gate_rows": [], "copy_cells": []}]
    finally:
        c.free()


def test_many_failures_over_many_blocks_are_listed_lowest_first(ctx):
    """2^12 rows, every third row corrupted, cap = 16: the counts are totals, the lists the 16 lowest in ascending order"""
    n, cols, q, perm = W.chain_with_pi(12, x0=5)
    bad = [list(col) for col in cols]
    for j in range(0, n - 3, 3):
        bad[2][j] = (bad[2][j] + 1) % R
    exp = _expected(q, perm, bad, [], 16)
    assert exp["gate_failures"] == len(range(0, n - 3, 3)) and exp["copy_failures"] > 2000
    assert n < exp["copy_cells"][-1][0] < 2 * n                  # b_{j+1} -> c_j fails before c_j -> a_{j+1}: all 16 in column 1
    c = Loaded(ctx, 12, _sel_arrays(q, n), perm)
    try:
        assert _check(ctx, c, [(bad, [])], cap=16) == [exp]
        # cap = 0 with null lists: the counts alone
        assert _check(ctx, c, [(bad, [])], cap=0) == [dict(exp, gate_rows=[], copy_cells=[])]
        # a cap beyond every count lists everything, columns 1 and 2 included
        full = _expected(q, perm, bad, [], 3 * n)
        assert _check(ctx, c, [(bad, [])], cap=3 * n) == [full]
    finally:
        c.free()


def test_five_witnesses_with_different_corruptions_in_one_call(ctx):
    n, cols, q, perm = W.chain_with_pi(6, [11, 12])
    variants = list(_corruptions(n, cols, [11, 12]))
    wits = [(bad, pi) for _, bad, pi in variants]
    exp = [_expected(q, perm, bad, pi, 4) for bad, pi in wits]
    assert len(wits) == 5 and len({str(e) for e in exp}) == 5
    c = Loaded(ctx, 6, _sel_arrays(q, n), perm)
    try:
        assert _check(ctx, c, wits, cap=4) == exp
        # the host form: the same reports
        host = ctx.witness_check_host(c.cid, [[fr_pack(col) for col in bad] for bad, _ in wits],
                                      [fr_pack(pi) for _, pi in wits], c.cosets, cap=4)
        assert host == exp
        assert ctx.witness_check_host(c.cid, [[fr_pack(col) for col in cols]], None, c.cosets) == [_expected(q, perm, cols, [], 16)]
    finally:
        c.free()


# ---- agreement with the prover -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [3, 4, 5, 6])
def test_the_verdict_is_the_provers(ctx, log_n):
    from test_gpu_compact import Chain
    from test_gpu_prove_batch_compact import single

    c = Chain(ctx, log_n)
    try:
        n = c.n
        pi = [21, 22]
        wits = [(c.columns(1), []), (c.columns(2, pi), pi)]
        for col, row in ((0, 1), (2, n - 4), (1, n - 1)):         # a gate cell, the last gate's output, a blinding row
            cols = c.columns(3, pi)
            cols[col][row] = _limbs(7 + col)
            wits.append((cols, pi))
        wits.append((c.columns(4, pi), [21, 23]))                 # a wrong public value
        bufs, pibs = _upload(ctx, wits)
        try:
            lens = [len(p) for _, p in wits]
            reps = ctx.witness_check(c.cid, bufs, pibs, lens, c.cosets)
            proved = [single(ctx, c, bufs[k], pibs[k], lens[k])[0] == 0 for k in range(len(wits))]
        finally:
            _free(bufs, pibs)
        clean = [r["gate_failures"] == 0 and r["copy_failures"] == 0 for r in reps]
        assert clean == proved == [True, True, False, False, True, False]
    finally:
        c.free()


def _proof_bytes(d):
    parts = []
    for key in ("commit", "t_commit", "witness"):
        for xy, inf in d[key]:
            parts += [np.asarray(xy, dtype=np.uint64).tobytes(), bytes([int(inf)])]
    parts += [np.asarray(d["z_commit"][0], dtype=np.uint64).tobytes(), bytes([int(d["z_commit"][1])])]
    return b"".join(parts + [np.asarray(e, dtype=np.uint64).tobytes() for e in d["evals"]])


@pytest.mark.parametrize("log_n", [6, 12])
def test_a_check_between_the_rounds_of_an_open_prover(ctx, log_n):
    """allowed while a round-by-round prover is open: the first check on the circuit (recovery, selector transforms) after
    round 1 and another after round 2 leave the proof as it is without them, bit for bit"""
    from test_gpu_compact import Chain

    c = Chain(ctx, log_n)
    bufs = [ctx.alloc(c.n) for _ in range(3)]
    try:
        for b, col in zip(bufs, c.columns(1)):
            b.upload(col)
        ch12, ch34 = (_limbs(0x1111), _limbs(0x2222)), (_limbs(0x3333), _limbs(0x4444))
        plain = ctx.prove(c.sid, c.cid, bufs, None, c.cosets, lambda pts: ch12, lambda pts: ch34)
        seen = []

        def checked(challenges):
            def squeeze(pts):
                seen.extend(ctx.witness_check(c.cid, [bufs], None, None, c.cosets))
                return challenges
            return squeeze

        busy = ctx.prove(c.sid, c.cid, bufs, None, c.cosets, checked(ch12), checked(ch34))
        assert seen == [{"gate_failures": 0, "copy_failures": 0, "gate_rows": [], "copy_cells": []}] * 2
        assert _proof_bytes(busy) == _proof_bytes(plain) and not np.asarray(busy["evals"][5]).any()
    finally:
        for b in bufs:
            b.free()
        c.free()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(ctx):
    n, cols, q, perm = W.chain_with_pi(4)
    c = Loaded(ctx, 4, _sel_arrays(q, n), perm)
    bufs, pibs = _upload(ctx, [(([fr_pack(col) for col in cols]), [1, 2])])
    short = ctx.alloc(n - 1)
    lib, ks = ctx.lib, capi._cosets_arg(c.cosets)
    try:
        reports = (capi.WitnessReport * 1)()
        gate, copy = (C.c_uint32 * 4)(*[0xA5] * 4), (C.c_uint32 * 8)(*[0xA5] * 8)
        C.memset(reports, 0xA5, C.sizeof(reports))
        before = (bytes(reports), bytes(gate), bytes(copy))
        w = (C.c_void_p * 3)(*[b.handle.value for b in bufs[0]])
        pip = (C.c_void_p * 1)(pibs[0].handle.value)
        one = lambda v: (C.c_size_t * 1)(v)   # noqa: E731

        def call(cid=c.cid, w=w, pip=pip, lens=one(2), count=1, ks=C.byref(ks), cap=4, reports=reports, gate=gate, copy=copy):
            return lib.typlonk_witness_check(ctx.h, cid, w, pip, lens, count, ks, cap, reports, gate, copy)

        w_null = (C.c_void_p * 3)(bufs[0][0].handle.value, None, bufs[0][2].handle.value)
        w_short = (C.c_void_p * 3)(bufs[0][0].handle.value, short.handle.value, bufs[0][2].handle.value)
        cases = [
            ("unknown circuit", call(cid=0xFFFF), ERR_INVALID_ARG),
            ("null columns", call(w=None), ERR_INVALID_ARG),
            ("null cosets", call(ks=None), ERR_INVALID_ARG),
            ("null reports", call(reports=None), ERR_INVALID_ARG),
            ("null lists with a cap", call(gate=None), ERR_INVALID_ARG),
            ("null copy list with a cap", call(copy=None), ERR_INVALID_ARG),
            ("a null column", call(w=w_null), ERR_INVALID_ARG),
            ("pi_len without pi", call(pip=None), ERR_INVALID_ARG),
            ("pi_len with a null entry", call(pip=(C.c_void_p * 1)(None)), ERR_INVALID_ARG),
            ("a short column", call(w=w_short), ERR_RANGE),
            ("a short pi buffer", call(lens=one(2 + 5 + 1)), ERR_RANGE),
        ]
        big = ctx.alloc(n + 1)
        cases.append(("pi_len > n", call(pip=(C.c_void_p * 1)(big.handle.value), lens=one(n + 1)), ERR_LENGTH))
        big.free()
        for name, rc, want in cases:
            assert rc == want, (name, rc)
        assert lib.typlonk_witness_check(None, c.cid, w, pip, one(2), 1, C.byref(ks), 4, reports, gate, copy) == ERR_INVALID_ARG
        # the host form: rows != n, and its own null checks
        host = [np.ascontiguousarray(fr_pack(col)) for col in cols]
        hw = (C.POINTER(C.c_uint64) * 3)(*[capi._u64p(a) for a in host])
        hcall = lambda rows, hw=hw: lib.typlonk_witness_check_host(ctx.h, c.cid, hw, rows, None, None, 1, C.byref(ks), 4, reports,  # noqa: E731
                                                                   gate, copy)
        assert hcall(n - 1) == ERR_LENGTH and hcall(2 * n) == ERR_LENGTH
        assert hcall(n, hw=(C.POINTER(C.c_uint64) * 3)(capi._u64p(host[0]), None, capi._u64p(host[2]))) == ERR_INVALID_ARG
        assert (bytes(reports), bytes(gate), bytes(copy)) == before
        # typlonk_circuit_permutation: unknown circuit, null cosets, null defects
        d = C.c_uint64(0xA5)
        assert lib.typlonk_circuit_permutation(ctx.h, 0xFFFF, C.byref(ks), None, C.byref(d)) == ERR_INVALID_ARG
        assert lib.typlonk_circuit_permutation(ctx.h, c.cid, None, None, C.byref(d)) == ERR_INVALID_ARG
        assert lib.typlonk_circuit_permutation(ctx.h, c.cid, C.byref(ks), None, None) == ERR_INVALID_ARG
        assert d.value == 0xA5
        # count = 0 is a no-op, and the same arguments are accepted once they are right
        assert call(count=0) == 0 and (bytes(reports), bytes(gate), bytes(copy)) == before
        assert call() == 0 and reports[0].gate_failures == 2 and reports[0].gate_listed == 2 and list(gate)[:2] == [0, 1]
        # (the witness was made for pi = []: rows 0 and 1 fail under the public values 1, 2)
    finally:
        short.free()
        _free(bufs, pibs)
        c.free()
