"""typlonk_witness_check / _host / typlonk_circuit_permutation where tests/test_gpu_witness_check.py does not reach: full-range
selectors over full-width, non-canonical cell words (random circuits and a grid of extreme limb patterns); circuits of 2^15 and
2^17 rows, where a thread of witness_scan_kernel owns more than one block count (or none); more witnesses than one launch
group, in both forms; recovery under 254-bit cosets.  Everything is integer equality with tests/witness_check_ref.py, which
reads the same raw words the device is given (a word w < 2^256 stands for w * 2^-256 mod r)."""
import random

import numpy as np
import pytest

import witness_check_ref as W
from oracle import plonk_oracle as PO
from test_gpu_witness_check import Loaded, _limbs

pytestmark = pytest.mark.gpu

R = W.R
TOP = 1 << 256
CLEAN = {"gate_failures": 0, "copy_failures": 0, "gate_rows": [], "copy_cells": []}
GARBAGE = 3                                                     # entries behind the public values in a device buffer


def _report(exp, cap):
    gate, copy = exp
    return {"gate_failures": len(gate), "copy_failures": len(copy), "gate_rows": gate[:cap], "copy_cells": copy[:cap]}


def _large_cosets(seed):
    """(1, k1, k2) with seeded 254-bit k1, k2 (every 254-bit value is below r)"""
    rng = random.Random(seed)
    return (1, rng.getrandbits(253) | 1 << 253, rng.getrandbits(253) | 1 << 253)


def _cosets_are_disjoint(cosets, n):
    return all(pow(cosets[i] * pow(cosets[j], -1, R) % R, n, R) != 1 for i in range(3) for j in range(3) if i != j)


def _load(ctx, log_n, q, perm, cosets=PO.COSETS):
    return Loaded(ctx, log_n, [W.mont_words(q[name]) for name in W.SELECTORS], perm, cosets)


def _pi_buffer(ctx, words):
    """the public values with GARBAGE entries behind them (the check must stop at pi_len)"""
    pb = ctx.alloc(len(words) + GARBAGE)
    pb.upload(np.concatenate([words, W.raw_words([TOP - 1 - i for i in range(GARBAGE)])]))
    return pb


def _check_raw_on_device(ctx, c, wits, cap):
    """the device form on [(3n raw values, raw public values)]"""
    n, bufs, pibs = c.n, [], []
    try:
        for raw, raw_pi in wits:
            bs = [ctx.alloc(n) for _ in range(3)]
            bufs.append(bs)
            for i, b in enumerate(bs):
                b.upload(W.raw_words(raw[i * n:(i + 1) * n]))
            pibs.append(_pi_buffer(ctx, W.raw_words(raw_pi)) if len(raw_pi) else None)
        return ctx.witness_check(c.cid, bufs, pibs, [len(p) for _, p in wits], c.cosets, cap=cap)
    finally:
        for b in [b for bs in bufs for b in bs] + [b for b in pibs if b is not None]:
            b.free()


def _expected_raw(q, perm, raw, raw_pi, n):
    return W.check_raw(q, perm, [raw[i * n:(i + 1) * n] for i in range(3)], raw_pi)


# ---- 2. full-range gate and copy arithmetic -------------------------------------------------------------------------------------
def _other_representatives(raw, rng):
    """a seeded third of the canonical raw values replaced by another word of the same residue: v + r, and for every other one
    of them v + 2r where that is below 2^256"""
    raw = raw.copy()
    for i, x in enumerate(np.flatnonzero(rng.random(len(raw)) < 1 / 3)):
        v = raw[x] + R
        raw[x] = v + R if i % 2 and v + R < TOP else v
    return raw


def _corrupted(raw, rng, count):
    """`count` seeded cells with their words moved by +1, -1 and a large offset in turn (mod 2^256)"""
    bad = raw.copy()
    offsets = (1, -1, int(rng.integers(1, 1 << 62)) << 190)
    for i, x in enumerate(rng.choice(len(raw), size=count, replace=False)):
        bad[x] = (bad[x] + offsets[i % 3]) % TOP
    return bad


def random_case(log_n, pi_len, seed):
    """a random circuit, its honest witness as raw words (a third of them non-canonical) and a corrupted one"""
    n, cols, q, perm, pi = W.random_circuit(log_n, seed, min(pi_len, 1 << log_n))
    rng = np.random.default_rng(seed)
    raw = _other_representatives(np.concatenate([W.raw_of(c) for c in cols]), rng)
    raw_pi = _other_representatives(W.raw_of(pi), rng)
    assert (raw >= R).sum() > n // 2 and raw.max() < TOP and (log_n < 9 or (raw >= 2 * R).sum() > n // 50)
    bad = _corrupted(raw, rng, max(3, n // 50))
    return n, q, perm, raw, raw_pi, bad


@pytest.mark.parametrize("pi_len", [0, 1, 37])
@pytest.mark.parametrize("log_n", [4, 9, 13])
def test_random_full_range_circuits_on_non_canonical_words(ctx, log_n, pi_len):
    """(2^4 rows take at most 16 public values: there 37 stands for "one on every row")"""
    n, q, perm, raw, raw_pi, bad = random_case(log_n, pi_len, 1000 * log_n + pi_len)
    assert _expected_raw(q, perm, raw, raw_pi, n) == ([], [])
    exp = _expected_raw(q, perm, bad, raw_pi, n)
    if log_n >= 9:                                              # the comparison below is not vacuous
        assert len(exp[0]) >= 3 and {x // n for x, _ in exp[1]} == {0, 1, 2}
    c = _load(ctx, log_n, q, perm)
    try:
        assert _check_raw_on_device(ctx, c, [(raw, raw_pi)], 16) == [CLEAN]
        assert _check_raw_on_device(ctx, c, [(bad, raw_pi)], 3 * n) == [_report(exp, 3 * n)]
        assert _check_raw_on_device(ctx, c, [(bad, raw_pi), (raw, raw_pi)], 5) == [_report(exp, 5), CLEAN]
    finally:
        c.free()


_ALT_EVEN = sum(0x3FFFFFFF << (30 * i) for i in range(0, 9, 2)) % TOP       # limbs 0, 2, 4, 6 full, limb 8 = 0xffff
_ALT_ODD = sum(0x3FFFFFFF << (30 * i) for i in range(1, 9, 2))              # limbs 1, 3, 5, 7 full
_LOW8 = 0x73ED * 2**240 - 1                                     # the largest value below r whose low eight limbs are full
CELL_WORDS = [0, 1, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, 2**254, 2**255 - 1, 2**255, TOP - 2, TOP - 1, _ALT_EVEN,
              _ALT_ODD] + [2**240 * k + s for k in (1, 0x73ED, 0x73EE, 0xFFFF) for s in (-1, 1)]
SEL_WORDS = [0, 1, R - 1, R - 2, 2**254, 2**240 - 1, _LOW8, None]           # None: a fresh random word
# word pairs that differ by 1, by r - 1 or by r + 1: never one residue
FAIL_PAIRS = [(0, 1), (R, R + 1), (2 * R, 2 * R + 1), (R - 1, R), (2 * R - 1, 2 * R), (TOP - 2, TOP - 1), (2**255 - 1, 2**255),
              (0, R - 1), (1, R), (R + 1, 2 * R), (0, R + 1), (R - 1, 2 * R), (R, 2 * R + 1)]
EXTREMES_PI_LEN = 32


def extremes_case():
    """n = 2^9 rows over CELL_WORDS x CELL_WORDS for (a, b), c and the four selectors running through their sets at other
    strides, the last rows the largest of everything at once; q_c makes the even rows hold and the odd rows miss by one.
    Rows 0, 1 mod 4 give the cells of cycles that hold several words of one residue, rows 2 mod 4 those of 2-cycles over
    FAIL_PAIRS, the rest stay fixed points.  Returns (n, q, perm, sel raw words, 3n raw, raw_pi, the failing copy pairs)."""
    n, nc, ns = 512, len(CELL_WORDS), len(SEL_WORDS)
    assert all(0 <= w < TOP for w in CELL_WORDS) and len(set(CELL_WORDS)) == nc
    assert all(w is None or 0 <= w < R for w in SEL_WORDS) and _LOW8 + 1 + (R & (2**240 - 1)) == R
    rng = random.Random(29)
    cell = [[CELL_WORDS[j % nc] for j in range(n)], [CELL_WORDS[j // nc % nc] for j in range(n)],
            [CELL_WORDS[(7 * j + 3) % nc] for j in range(n)]]
    sel = [[SEL_WORDS[j // 8**k % ns] if k < 3 else SEL_WORDS[(3 * j + j // nc) % ns] for j in range(n)] for k in range(4)]
    worst = [(TOP - 1, R - 1), (TOP - 1, _LOW8), (_ALT_EVEN, R - 1), (_ALT_ODD, _LOW8), (TOP - 2, R - 2), (2 * R + 1, 2**254)]
    for i, (cw, sw) in enumerate(worst):
        for j in (n - 2 * len(worst) + 2 * i, n - 2 * len(worst) + 2 * i + 1):     # an even row and an odd one
            for col in cell:
                col[j] = cw
            for s in sel:
                s[j] = sw
    sel = [[rng.randrange(R) if w is None else w for w in s] for s in sel]
    raw = W._obj([w for col in cell for w in col])
    raw_pi = W._obj([CELL_WORDS[(3 * j + 1) % nc] for j in range(EXTREMES_PI_LEN)])
    a, b, c = (W.residues_of(col) for col in cell)
    ql, qr, qo, qm = (W.residues_of(s) for s in sel)
    pub = W._obj(W.residues_of(raw_pi).tolist() + [0] * (n - EXTREMES_PI_LEN))
    odd = W._obj([j & 1 for j in range(n)])
    qc = (odd - (ql * a + qr * b - qo * c + qm * a * b + pub)) % R
    q = {name: v.tolist() for name, v in zip(W.SELECTORS, (ql, qr, qo, qm, qc))}
    sel_raw = [W._obj(s) for s in sel] + [W.raw_of(qc)]
    # the permutation
    perm, used = list(range(3 * n)), set()
    where = {}                                                  # word -> its cells in the rows of each pool
    for x in range(3 * n):
        where.setdefault((int(raw[x]), x % n % 4), []).append(x)
    same = 0
    for words in ((0, R, 2 * R), (1, R + 1, 2 * R + 1), (R - 1, 2 * R - 1)):
        lists = [where[w, 0] + where[w, 1] for w in words]
        cells = [lst[i] for i in range(max(map(len, lists))) for lst in lists if i < len(lst)]     # the words in turn
        at, length = 0, 2
        while at + length <= len(cells):
            cyc = cells[at:at + length]
            for x, y in zip(cyc, cyc[1:] + cyc[:1]):
                perm[x] = y
                same += raw[x] != raw[y]
            at, length = at + length, 2 + (length - 1) % 4      # lengths 2, 3, 4, 5, 2, ..
    assert same > 100                                           # copy constraints between different words of one residue
    failing = []
    for wa, wb in FAIL_PAIRS:
        xs, ys = ([x for x in where[w, 2] if x not in used] for w in (wa, wb))
        assert xs and ys
        for x, y in list(zip(xs, reversed(ys)))[:3]:                # low cells with high ones: all three columns
            perm[x], perm[y] = y, x
            used.update((x, y))
            failing += [(x, y), (y, x)]
    assert sorted(perm) == list(range(3 * n))
    return n, q, perm, sel_raw, raw, raw_pi, sorted(failing)


def test_a_grid_of_extreme_words_and_selectors(ctx):
    n, q, perm, sel_raw, raw, raw_pi, failing = extremes_case()
    exp = _expected_raw(q, perm, raw, raw_pi, n)
    assert exp == (list(range(1, n, 2)), failing) and len(failing) >= 4 * len(FAIL_PAIRS)
    assert {x // n for x, _ in failing} == {0, 1, 2}
    c = Loaded(ctx, 9, [W.raw_words(s) for s in sel_raw], perm)
    try:
        assert _check_raw_on_device(ctx, c, [(raw, raw_pi)], 3 * n) == [_report(exp, 3 * n)]
    finally:
        c.free()


# ---- 3. past one scan piece ------------------------------------------------------------------------------------------------------
def corruption_rows(n):
    """the rows next to block and piece borders, every 1000th row outside the clean stretch 7001..12999, and five rows of
    one mask word"""
    rows = {0, 255, 256, 257, 511, 512, 513, n // 2 - 1, n // 2, n - 257, n - 256, n - 1} | set(range(4160, 4165))
    return sorted(rows | {j for j in range(1000, n, 1000) if not 7000 < j < 13000})


class Big:
    """a random circuit of 2^log_n rows with a public value on every row, loaded on the device, its honest witness in device
    buffers, and corrupted variants of it (built on first use, kept until the module is done)"""

    def __init__(self, ctx, log_n, cosets):
        self.ctx, self.log_n, self.cosets_int = ctx, log_n, cosets
        n, cols, self.q, self.perm, pi = W.random_circuit(log_n, 300 + log_n, 1 << log_n)
        self.n = n
        self.raw = [W.raw_of(c) for c in cols]
        self.raw_pi = W.raw_of(pi)
        self.words = [W.raw_words(r) for r in self.raw]
        self.pi_words = W.raw_words(self.raw_pi)
        self.c = _load(ctx, log_n, self.q, self.perm, cosets)
        self.bufs = [self._column(w) for w in self.words]
        self.pib = _pi_buffer(ctx, self.pi_words)
        self.extra, self.made = [], {}

    def _column(self, words):
        b = self.ctx.alloc(self.n)
        b.upload(words)
        return b

    def _changes(self, name):
        """{(column or "pi", row): offset} of a variant"""
        n = self.n
        if name == "honest":
            return {}
        if name == "spread":
            return {(0 if j % 3 == 2 else 2, j): (1, -1, 1 << 200)[i % 3] for i, j in enumerate(corruption_rows(n))}
        if name == "row_0":
            return {("pi", 0): 1}
        if name == "last_row":
            return {("pi", n - 1): 1}
        if name == "other":
            return {(1, 300): 1, (1, 301): -1, (1, n - 2): 5, ("pi", 5): 1, (0, n // 2 + 255): 1, (0, n // 2 + 256): 1}
        raise KeyError(name)

    def variant(self, name):
        """{"raw", "raw_pi", "words", "pi_words", "bufs", "pib", "exp"}: the columns a variant does not touch are the honest
        ones (the same arrays, the same device buffers)"""
        if name not in self.made:
            raw, raw_pi = list(self.raw), self.raw_pi
            words, pi_words, bufs, pib = list(self.words), self.pi_words, list(self.bufs), self.pib
            changes = self._changes(name)
            for col in sorted({col for col, _ in changes}, key=str):
                v = (raw_pi if col == "pi" else raw[col]).copy()
                for (c2, row), off in changes.items():
                    if c2 == col:
                        v[row] = (v[row] + off) % TOP
                if col == "pi":
                    raw_pi, pi_words = v, W.raw_words(v)
                    pib = _pi_buffer(self.ctx, pi_words)
                    self.extra.append(pib)
                else:
                    raw[col], words[col] = v, W.raw_words(v)
                    bufs[col] = self._column(words[col])
                    self.extra.append(bufs[col])
            exp = W.check_raw(self.q, self.perm, raw, raw_pi)
            self.made[name] = {"raw": raw, "raw_pi": raw_pi, "words": words, "pi_words": pi_words, "bufs": bufs, "pib": pib, "exp": exp}
        return self.made[name]

    def check(self, names, cap):
        vs = [self.variant(name) for name in names]
        return self.ctx.witness_check(self.c.cid, [v["bufs"] for v in vs], [v["pib"] for v in vs], [self.n] * len(vs), self.c.cosets,
                                      cap=cap)

    def free(self):
        for b in self.bufs + [self.pib] + self.extra:
            b.free()
        self.c.free()


@pytest.fixture(scope="module")
def big15(ctx):
    b = Big(ctx, 15, PO.COSETS)
    yield b
    b.free()


@pytest.fixture(scope="module")
def big17(ctx):
    cosets = _large_cosets(17)
    assert _cosets_are_disjoint(cosets, 1 << 17)
    b = Big(ctx, 17, cosets)
    yield b
    b.free()


@pytest.fixture(params=[15, 17])
def big(request):
    return request.getfixturevalue(f"big{request.param}")


def scan_pieces(n, failures):
    """witness_scan_kernel's cut of the block counts, for the gate rows or the cells that fail: (entries per thread, the number
    of non-empty blocks in each thread's piece, the threads that own nothing)"""
    gate_scan = not failures or not isinstance(failures[0], tuple)
    length = n // 256 if gate_scan else 3 * n // 256
    blocks = {(f if gate_scan else f[0]) // 256 for f in failures}
    per = -(-length // 256)
    counts = [sum(b in blocks for b in range(t * per, min(t * per + per, length))) for t in range(256) if t * per < length]
    return per, counts, 256 - len(counts)


def cap_inside_a_mask_word(gate):
    """a cap that lists the first two of at least three failing rows of one 64-row word"""
    for i, j in enumerate(gate):
        if i + 2 < len(gate) and gate[i + 2] // 64 == j // 64:
            return i + 2
    raise AssertionError("no mask word with three failures")


def test_honest_witnesses_past_one_scan_piece(big):
    assert big.variant("honest")["exp"] == ([], [])
    assert big.check(["honest"], 16) == [CLEAN]


def test_failures_at_block_and_piece_borders(big):
    n = big.n
    gate, copy = exp = big.variant("spread")["exp"]
    rows = corruption_rows(n)
    assert gate == rows and not any(7000 < j < 13000 for j in gate) and {x // n for x, _ in copy} == {0, 1, 2}
    assert copy[-1][0] == 3 * n - 1                             # the last cell of all
    gate_per, gate_counts, gate_idle = scan_pieces(n, gate)
    cell_per, cell_counts, cell_idle = scan_pieces(n, copy)
    if big.log_n == 15:
        assert (gate_per, gate_idle, cell_per, cell_idle) == (1, 128, 2, 64)
    else:
        assert (gate_per, gate_idle, cell_per, cell_idle) == (2, 0, 6, 0)
        assert max(gate_counts) >= 2 and 0 in gate_counts and any(j // 256 >= 256 for j in gate)
    assert max(cell_counts) >= 2 and 0 in cell_counts
    inside = cap_inside_a_mask_word(gate)
    assert gate[inside - 1] // 64 == gate[inside] // 64 and inside not in (0, 16) and inside < len(gate)
    for cap in (0, 16, inside, 3 * n):
        assert big.check(["spread"], cap) == [_report(exp, cap)], cap


@pytest.mark.parametrize("name", ["row_0", "last_row"])
def test_a_single_failing_row_at_either_end(big, name):
    exp = big.variant(name)["exp"]
    assert exp == ([0 if name == "row_0" else big.n - 1], [])
    assert big.check([name], 16) == [_report(exp, 16)]
    assert big.check([name], 0) == [_report(exp, 0)]


def test_two_witnesses_with_different_corruptions_in_one_call(big15):
    exp = [big15.variant(name)["exp"] for name in ("spread", "other")]
    assert exp[0] != exp[1] and len(exp[1][0]) == 6 and exp[1][1]
    for cap in (16, 3 * big15.n):
        assert big15.check(["spread", "other"], cap) == [_report(e, cap) for e in exp]
        assert big15.check(["other", "honest", "spread"], cap) == [_report(exp[1], cap), CLEAN, _report(exp[0], cap)]


# ---- 4. more witnesses than one launch group --------------------------------------------------------------------------------
MANY = 1030                                                     # above the 1024 witnesses of a launch group


def many_small_witnesses():
    """2^3 rows: witness k adds 1 + k // 24 to the word of cell k mod 24.  Returns (q, perm, honest word columns, pi words,
    [(column, its corrupted words)], [expected (gate, copy)])"""
    n, cols, q, perm, pi = W.random_circuit(3, 33, 2)
    raw, raw_pi = [W.raw_of(c) for c in cols], W.raw_of(pi)
    changed, exp = [], []
    for k in range(MANY):
        col, row = k % 24 // n, k % 24 % n
        bad = list(raw)
        bad[col] = raw[col].copy()
        bad[col][row] += 1 + k // 24
        changed.append((col, W.raw_words(bad[col])))
        exp.append(W.check_raw(q, perm, bad, raw_pi))
    assert all(e[0] == [k % 24 % n] for k, e in enumerate(exp)) and all(a != b for a, b in zip(exp, exp[1:]))
    assert exp[1024] != exp[0] and exp[1029] != exp[5] and sum(bool(e[1]) for e in exp) > MANY // 2
    return q, perm, [W.raw_words(r) for r in raw], W.raw_words(raw_pi), changed, exp


def test_more_witnesses_than_one_launch_group(ctx):
    q, perm, honest, pi_words, changed, exp = many_small_witnesses()
    c = _load(ctx, 3, q, perm)
    bufs = []
    try:
        for words in honest + [w for _, w in changed]:
            bufs.append(ctx.alloc(8))
            bufs[-1].upload(words)
        pib = _pi_buffer(ctx, pi_words)
        bufs.append(pib)
        wires = [[bufs[3 + k] if i == col else bufs[i] for i in range(3)] for k, (col, _) in enumerate(changed)]
        got = ctx.witness_check(c.cid, wires, [pib] * MANY, [2] * MANY, c.cosets, cap=4)
        assert got == [_report(e, 4) for e in exp]
        # the host form
        host = [[w if i == col else honest[i] for i in range(3)] for col, w in changed]
        got = ctx.witness_check_host(c.cid, host, [pi_words] * MANY, c.cosets, cap=4)
        assert got == [_report(e, 4) for e in exp]
    finally:
        for b in bufs:
            b.free()
        c.free()


def test_host_witnesses_in_groups_cut_by_the_staging_buffer(big17):
    """33 witnesses of 2^17 rows: 4 n 32 bytes of staged columns each bring a launch group down to about 31 witnesses.  The
    honest ones are one set of host arrays; 0, 30 and 32 are corrupted, each in its own way."""
    names = ["honest"] * 33
    names[0], names[30], names[32] = "spread", "row_0", "last_row"
    vs = [big17.variant(name) for name in names]
    assert big17.n * 4 * 32 * 33 > 512 << 20
    got = big17.ctx.witness_check_host(big17.c.cid, [v["words"] for v in vs], [v["pi_words"] for v in vs], big17.c.cosets, cap=16)
    assert got == [_report(v["exp"], 16) for v in vs]
    assert [g != CLEAN for g in got] == [name != "honest" for name in names]


# ---- 5. recovery under large cosets -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [5, 12])
def test_recovery_and_check_under_254_bit_cosets(ctx, log_n):
    cosets = _large_cosets(log_n)
    assert all(k >> 253 == 1 for k in cosets[1:]) and _cosets_are_disjoint(cosets, 1 << log_n)
    n, q, perm, raw, raw_pi, bad = random_case(log_n, 3, 77 + log_n)
    exp = _expected_raw(q, perm, bad, raw_pi, n)
    assert exp[0] and exp[1]
    c = _load(ctx, log_n, q, perm, cosets)
    try:
        got, defects = ctx.circuit_permutation(c.cid, n, c.cosets)
        assert got.tolist() == perm and defects == 0
        assert _check_raw_on_device(ctx, c, [(raw, raw_pi), (bad, raw_pi)], 3 * n) == [CLEAN, _report(exp, 3 * n)]
        # the ids of (1, k1, k2) are not those of (2, 3, 4)
        assert ctx.circuit_permutation(c.cid, n, [_limbs(k) for k in PO.COSETS])[1] != 0
    finally:
        c.free()


def test_recovery_at_2_17_rows_under_254_bit_cosets(big17):
    got, defects = big17.ctx.circuit_permutation(big17.c.cid, big17.n, big17.c.cosets)
    assert defects == 0 and np.array_equal(got.astype(np.int64), np.asarray(big17.perm, dtype=np.int64))
