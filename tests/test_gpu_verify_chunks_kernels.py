"""The kernels of typlonk_verify_chunks -- verify_chunks.hip compiled as the library compiles it, behind the test-only harness
tests/cpp/libdevice_verify_chunks.so -- with their launchers called directly, against tests/verify_chunks_ref.py word for word.

chunks_weights_kernel, chunks_fold_kernel, chunks_fold_sum_kernel: the weights of a fold over [lo, hi), w_c and the l coefficients
of A, for l in {1, 2, 8, 64, 128, 1024} (a wavefront per cell up to 64, the workgroup above, one, two and four coefficients a
thread), N in {1, 2, one strip + 1, three strips with a ragged last one} for two named strip sizes and the plan's own -- every
strip size gives the same words, a sum of field elements being a canonical residue --, sub-ranges inside one strip and across
strips with dead cells inside, cosets 0 and r - 1, one cell twice, all-zero evaluations and evaluations of r - 1, every cell
under one commitment and a commitment no cell names.  chunks_cosets_kernel past the r = 8 of those cases: r = 32 and 64, and
log_n = 24 at l = 1, 8, 64, 1024 with coset indices 0, 1, 31, 32, 33, 2^16 - 1, 2^16, r/2, r - 1 and random ones -- w^(-k_i) and
rho_i w^(l k_i) from Python's pow --, and pairs of cells that differ in one bit of k_i alone (bit 5, the top bit, one between).
chunks_weights_kernel past four commitments: M = 1000 over N = 700 cells in no order (one commitment of 300 cells, 300 of one or
two, runs of unnamed ones, ranges that cut the big one and that miss it), M = 65536 over N = 5, and M = N = 1.
chunks_membership_kernel: one flag per record, and the failing records
cleared, on the generator, an identity, the order-3 point (0, 2) and an off-curve record, over more than one wavefront."""
import ctypes

import numpy as np
import pytest

import arith_cases as AC
import verify_chunks_ref as VR
from helpers import O, ROOT, fr_pack, fr_unpack

pytestmark = pytest.mark.gpu

R = O.R
U32P = ctypes.POINTER(ctypes.c_uint32)
U8P = ctypes.POINTER(ctypes.c_uint8)
U64P = ctypes.POINTER(ctypes.c_uint64)
PT_WORDS = 32
LOG_LS = [0, 1, 3, 6, 7, 10]
LOG_R = 3
STRIPS = [5, 8]                      # no multiple of the four cells a workgroup takes at once at l <= 64, and one
NOT_ON_CURVE, NOT_IN_SUBGROUP = 3, 4


@pytest.fixture(scope="module")
def lib(built):
    import os

    try:    # PyTorch's bundled HIP runtime must be loaded before the system one the harness links (typlonk_amd.capi.load_library says
        import torch  # noqa: F401  why), or the tests that use torch later in the same process find no device
    except ImportError:
        pass
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpp", "libdevice_verify_chunks.so"))
    lib.dvc_fold.restype = ctypes.c_int
    lib.dvc_fold.argtypes = [U32P, U32P, U32P, U8P, U32P, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32,
                             U32P, U32P, ctypes.c_uint64, U32P, U32P, U32P, U32P, U32P, U64P, U32P]
    lib.dvc_membership.restype = ctypes.c_int
    lib.dvc_membership.argtypes = [U32P, ctypes.c_uint64, ctypes.c_uint32, U8P, U32P]
    return lib


def _words(vals) -> np.ndarray:
    """canonical ints -> (k, 8) uint32: the Montgomery limbs as the kernels' 32-bit words"""
    return np.ascontiguousarray(fr_pack(list(vals))).view(np.uint32).reshape(-1, 8)


def _p(a, t=U32P):
    return a.ctypes.data_as(t)


def _rand(rng, k):
    return [int.from_bytes(rng.bytes(32), "little") % R for _ in range(k)]


class Case:
    """N cells of l evaluations over M commitments, their device inputs, and the reference's outputs for any range"""

    def __init__(self, log_l, N, M, seed, one_commitment=False, log_r=LOG_R, cosets=None, commits=None, same_evals=()):
        """cosets, commits: the cells' k_i and c_i, named by the caller (N of each) instead of drawn; same_evals: pairs (i, j),
        cell j gets cell i's evaluations"""
        self.log_l, self.log_n, self.N, self.M = log_l, log_l + log_r, N, M
        l, r = 1 << log_l, 1 << log_r
        assert cosets is None or (len(cosets) == N and all(0 <= k < r for k in cosets))
        assert commits is None or (len(commits) == N and all(0 <= c < M for c in commits))
        rng = np.random.default_rng(seed)
        self.rho = _rand(rng, 1)[0]
        cells = []
        for i in range(N):
            ys = _rand(rng, l)
            if i == 2:
                ys = [0] * l                                   # all-zero evaluations
            if i == 3:
                ys = [R - 1] * l                               # full-range values
            if cosets is not None:
                k = cosets[i]
            else:
                k = (0, r - 1)[i] if i < 2 and N > 2 else int(rng.integers(0, r))
            if commits is not None:
                c = commits[i]
            else:
                c = 0 if one_commitment else int(rng.integers(0, M - 1)) if M > 1 else 0    # commitment M - 1: no cell names it
            cells.append((c, k, ys, 0))
        if N >= 6 and cosets is None and commits is None:
            cells[5] = cells[4]                                # the same cell twice
        for i, j in same_evals:
            cells[j] = (cells[j][0], cells[j][1], cells[i][2], 0)
        self.cells = cells
        w = O.domain_root(self.log_n)
        mu_inv = pow(O.domain_root(log_l), -1, R)
        self.pw = _words(pow(self.rho, i, R) for i in range(N))
        self.commit = np.array([c[0] for c in cells], dtype=np.uint32)
        self.coset = np.array([c[1] for c in cells], dtype=np.uint32)
        self.evals = _words(y for c in cells for y in c[2])
        self.consts = _words([pow(w, l, R), pow(w, -1, R), pow(l, -1, R)])
        self.tw = _words(pow(mu_inv, j, R) for j in range(max(l // 2, 1)))
        self.twist = _words(pow(w, -c[1], R) for c in cells)

    def run(self, lib, lo, hi, live, strip):
        N, M, l = self.N, self.M, 1 << self.log_l
        lv = np.array(live, dtype=np.uint8)
        out = {k: np.full((n, 8), 0x11111111, dtype=np.uint32) for k, n in (("s_pi", N + M), ("s_all", N + M), ("scale", N), ("twist", N), ("coef", l))}
        blocks = np.zeros(1, dtype=np.uint64)
        guard = np.zeros(1, dtype=np.uint32)
        rc = lib.dvc_fold(_p(self.pw), _p(self.commit), _p(self.coset), _p(lv, U8P), _p(self.evals), N, M, lo, hi, self.log_l, _p(self.consts),
                          _p(self.tw), strip, _p(out["s_pi"]), _p(out["s_all"]), _p(out["scale"]), _p(out["twist"]), _p(out["coef"]),
                          _p(blocks, U64P), _p(guard))
        assert rc == 0, rc
        assert guard[0] == 1, "a launcher wrote behind one of its outputs"
        return out, int(blocks[0])

    def expected(self, lo, hi, live):
        l = 1 << self.log_l
        w = VR.weights(self.N, self.rho, lo, hi, live)
        a = [VR.coset_constant(c[1], self.log_n, self.log_l) for c in self.cells]
        return {"s_pi": _words(w + [0] * self.M),
                "s_all": _words([wi * ai % R for wi, ai in zip(w, a)] + VR.commitment_weights(self.cells, w, self.M)),
                "scale": _words(wi * pow(l, -1, R) % R for wi in w),
                "twist": self.twist,
                "coef": _words(VR.fold_coefficients(self.cells, w, self.log_n, self.log_l))}


def _compare(got, want, what):
    for k in want:
        assert (got[k] == want[k]).all(), (what, k, np.argwhere((got[k] != want[k]).any(axis=1)).ravel()[:8])


@pytest.mark.parametrize("log_l", LOG_LS)
def test_fold_and_weights_match_the_reference_for_every_strip(lib, log_l):
    """all cells live, the whole range: N = 1, 2, one strip + 1 and three strips with a ragged last one, for both named strips and
    the plan's own; the named strips cut the cells into the expected number of partial vectors"""
    for N in sorted({1, 2} | {s + 1 for s in STRIPS} | {2 * s + 3 for s in STRIPS}):
        case = Case(log_l, N, 3, 0x5E0 + 64 * log_l + N)
        live = [1] * N
        want = case.expected(0, N, live)
        for strip in [0] + STRIPS:
            got, blocks = case.run(lib, 0, N, live, strip)
            _compare(got, want, (N, strip))
            if strip:
                assert blocks == -(-N // strip)


@pytest.mark.parametrize("log_l", [3, 6, 7])
def test_sub_ranges_and_dead_cells(lib, log_l):
    """[lo, hi) inside one strip, across strips, a single cell, the last cell; dead cells inside and at the ends of the range: the
    weights outside are zero, the dead cells add nothing"""
    N, strip = 19, 5
    case = Case(log_l, N, 4, 0xDEAD + log_l)
    live = [0 if i in (2, 7, 8, 18) else 1 for i in range(N)]
    for lo, hi in [(0, N), (1, 4), (3, 14), (6, 10), (7, 9), (18, 19), (17, 19), (11, 12)]:
        want = case.expected(lo, hi, live)
        for s in (strip, 8, 0):
            got, _ = case.run(lib, lo, hi, live, s)
            _compare(got, want, (lo, hi, s))
    none = case.expected(7, 9, live)                           # no live cell in the range: everything is zero
    assert not none["coef"].any() and not none["s_all"].any()


@pytest.mark.parametrize("log_l", [0, 6])
def test_every_cell_under_one_commitment_and_one_unnamed(lib, log_l):
    """w_0 is the sum of every live weight of the range -- more cells than the 256 threads of the workgroup that sums them, so
    that every thread strides -- and the commitments no cell names get zero"""
    N, M = 600, 3
    case = Case(log_l, N, M, 0x0C0 + log_l, one_commitment=True)
    live = [0 if i % 7 == 3 else 1 for i in range(N)]
    for lo, hi in [(0, N), (255, 513)]:
        got, _ = case.run(lib, lo, hi, live, 0)
        want = case.expected(lo, hi, live)
        _compare(got, want, (lo, hi))
        w = VR.weights(N, case.rho, lo, hi, live)
        assert (got["s_all"][N] == _words([sum(w) % R])[0]).all() and not got["s_all"][N + 1:].any()


# ---- cosets past 32: every bit of k_i counts ------------------------------------------------------------------------------------
# (log_l, log_r): log_n = 24, the widest domain the call admits, at l = 1, 8, 64, 1024 -- k_i up to 2^24 - 1 --, and r = 32 and
# 64, the first sizes past the r = 8 of every case above
COSET_SHAPES = [(0, 24), (3, 21), (6, 18), (10, 14), (3, 5), (3, 6)]


def _ints(words) -> list[int]:
    """(k, 8) uint32 Montgomery words -> canonical ints"""
    return fr_unpack(np.ascontiguousarray(words).view(np.uint64).reshape(-1, 4))


def _cosets(log_r, seed):
    """0, 1, 31, 32, 33, 2^16 - 1, 2^16, r/2 and r - 1 where they are below r, and seeded random ones to make twelve"""
    r = 1 << log_r
    ks = [k for k in (0, 1, 31, 32, 33, (1 << 16) - 1, 1 << 16, r // 2, r - 1) if k < r]
    rng = np.random.default_rng(seed)
    return ks + [int(rng.integers(0, r)) for _ in range(12 - len(ks))]


@pytest.mark.parametrize("log_l,log_r", COSET_SHAPES)
def test_cosets_across_the_admitted_range(lib, log_l, log_r):
    """twist[i] = w^(-k_i), s_all[i] = rho_i w^(l k_i) and the fold's coefficients, for coset indices that use every bit up to
    log_r - 1, under the plan's own strip and a named one; the whole range, and a sub-range with dead cells"""
    r, l = 1 << log_r, 1 << log_l
    ks = _cosets(log_r, 0xC05E7 + 64 * log_l + log_r)
    N = len(ks)
    assert N == 12 and max(ks) == r - 1 and (log_r < 17 or (1 << 16) in ks)
    case = Case(log_l, N, 3, 0xC05 + 64 * log_l + log_r, log_r=log_r, cosets=ks)
    w = O.domain_root(log_l + log_r)
    assert pow(w, 1 << (log_l + log_r - 1), R) == R - 1                      # w has order n exactly: w^k differ for k < n
    for lo, hi, live in [(0, N, [1] * N), (1, N - 1, [0 if i in (4, 9) else 1 for i in range(N)])]:
        want = case.expected(lo, hi, live)
        rho_i = VR.weights(N, case.rho, lo, hi, live)
        for strip in (0, 5):
            got, _ = case.run(lib, lo, hi, live, strip)
            assert _ints(got["twist"]) == [pow(w, -k, R) for k in ks], (lo, hi, strip)
            assert _ints(got["s_all"][:N]) == [x * pow(w, l * k, R) % R for x, k in zip(rho_i, ks)], (lo, hi, strip)
            _compare(got, want, (lo, hi, strip))


@pytest.mark.parametrize("log_l,log_r", COSET_SHAPES)
def test_cosets_that_differ_in_one_high_bit(lib, log_l, log_r):
    """cells 2j and 2j + 1 carry the same evaluations under the same commitment and the cosets k and k XOR 2^b, for b = 5,
    b = log_r - 1 and one bit between: their twists and their a_k = s_all / s_pi differ, and each is the reference's"""
    r = 1 << log_r
    bits = sorted({5, (5 + log_r - 1) // 2, log_r - 1} & set(range(log_r)))
    assert bits[-1] == log_r - 1 and (5 in bits or log_r == 5)              # (r = 32 has no bit 5: its top bit is 4)
    rng = np.random.default_rng(0xB17 + 64 * log_l + log_r)
    ks = []
    for b in bits:
        k = int(rng.integers(0, r))
        ks += [k, k ^ (1 << b)]
    N = len(ks)
    case = Case(log_l, N, 2, 0xB175 + 64 * log_l + log_r, log_r=log_r, cosets=ks, commits=[0] * N,
                same_evals=[(2 * j, 2 * j + 1) for j in range(N // 2)])
    live = [1] * N
    got, _ = case.run(lib, 0, N, live, 0)
    _compare(got, case.expected(0, N, live), (log_l, log_r))
    rho_i, a = _ints(got["s_pi"][:N]), _ints(got["s_all"][:N])
    a = [x * pow(y, -1, R) % R for x, y in zip(a, rho_i)]
    assert a == [VR.coset_constant(k, log_l + log_r, log_l) for k in ks]
    for j, b in enumerate(bits):
        assert case.cells[2 * j][2] == case.cells[2 * j + 1][2]
        assert (got["twist"][2 * j] != got["twist"][2 * j + 1]).any(), b
        assert a[2 * j] != a[2 * j + 1], b


# ---- many commitments ------------------------------------------------------------------------------------------------------------
def _thousand_commitments(seed):
    """(commits of 700 cells over M = 1000, the named commitments): commitment 7 holds 300 cells, 200 commitments hold one and 100
    hold two; commitment 0 and 400 .. 519 are among the unnamed.  The first 100 cells name none of commitment 7's, the other 600
    are commitment 7's and the rest in a seeded order: nothing is sorted by commitment."""
    rng = np.random.default_rng(seed)
    pool = [c for c in range(1, 1000) if c != 7 and not 400 <= c < 520]
    named = [int(c) for c in rng.choice(pool, size=300, replace=False)]
    if 999 not in named:
        named[0] = 999                                                       # the last workgroup of the launch has a cell
    others = named + named[:100]
    rng.shuffle(others)
    tail = [7] * 300 + others[100:]
    rng.shuffle(tail)
    return others[:100] + tail, set(named) | {7}


@pytest.mark.parametrize("log_l", [0, 6])
def test_a_thousand_commitments(lib, log_l):
    """M = 1000 outnumbers N = 700.  w_c for a commitment of 300 cells (every thread of its workgroup strides), of one and of two
    cells, and for runs of commitments no cell names; over the whole call, a range that cuts commitment 7's cells in two and one
    that holds none of them, with dead cells everywhere: an unnamed commitment and one whose cells all lie outside the range or
    are dead get zero"""
    N, M = 700, 1000
    commits, named = _thousand_commitments(0x7C0 + log_l)
    assert len(commits) == N and commits.count(7) == 300 and 7 not in commits[:100] and commits != sorted(commits)
    assert 0 not in named and not named & set(range(400, 520)) and len(named) == 301 and max(named) == 999
    assert sum(commits.count(c) == 1 for c in named) == 200 and sum(commits.count(c) == 2 for c in named) == 100
    assert sum(1 for c in named if c > 255) > 100
    case = Case(log_l, N, M, 0x3E8 + log_l, commits=commits)
    live = [0 if i % 7 == 3 else 1 for i in range(N)]
    sevens = [i for i, c in enumerate(commits) if c == 7]
    for lo, hi in [(0, N), (sevens[150], N), (3, 100)]:
        got, _ = case.run(lib, lo, hi, live, 0)
        _compare(got, case.expected(lo, hi, live), (lo, hi))
        reached = {commits[i] for i in range(lo, hi) if live[i]}
        assert (7 in reached) == (hi > 100) and len(reached) < M
        for c in range(M):
            assert got["s_all"][N + c].any() == (c in reached), (lo, hi, c)   # (a sum of distinct powers of rho is not zero)
        assert not got["s_pi"][N:].any()
    inside = [i for i in sevens if i >= sevens[150] and live[i]]
    assert 0 < len(inside) < sum(live[i] for i in sevens)                     # the second range does cut commitment 7's cells


def test_more_commitments_than_a_launch_has_cells(lib):
    """M = 65536, the most the harness admits, and N = 5 cells that name commitments 0, 1, 32767 and 65535: one workgroup of
    cells and 65536 of commitments"""
    N, M = 5, 1 << 16
    commits = [65535, 1, 0, 32767, 1]
    for log_l in (0, 6):
        case = Case(log_l, N, M, 0xFFFF + log_l, commits=commits)
        for lo, hi, live in [(0, N, [1] * N), (1, 5, [1, 1, 1, 0, 1])]:
            got, _ = case.run(lib, lo, hi, live, 0)
            _compare(got, case.expected(lo, hi, live), (log_l, lo, hi))
            reached = {commits[i] for i in range(lo, hi) if live[i]}
            assert set(np.nonzero(got["s_all"][N:].any(axis=1))[0].tolist()) == reached


def test_one_cell_one_commitment(lib):
    for log_l in (0, 6):
        case = Case(log_l, 1, 1, 0x111 + log_l)
        got, _ = case.run(lib, 0, 1, [1], 0)
        _compare(got, case.expected(0, 1, [1]), log_l)
        assert (got["s_all"][1] == got["s_pi"][0]).all()                      # w_0 = rho^0


def _record(pt) -> list[int]:
    """a point (affine integers or None) as the PT_WORDS words of an SRS record: x, y canonical in Montgomery form, 12 words each"""
    if pt is None:
        return [0] * PT_WORDS
    return AC.limbs(AC.mont(pt[0]), 12, 32) + AC.limbs(AC.mont(pt[1]), 12, 32) + [0] * 8


@pytest.mark.parametrize("clear", [0, 1])
def test_membership_flags(lib, clear):
    g5 = O.g1_mul(O.G1, 5)
    order3 = (0, 2)
    off = (O.GX, (O.GY + 1) % O.P)
    assert O.g1_is_on_curve(order3) and not O.g1_is_on_curve(off)
    pts = [O.G1, None, order3, off] + [g5] * 66
    pts[63], pts[64], pts[69] = off, order3, None             # the last lane of a wavefront, the first of the next, the last record
    want = [NOT_IN_SUBGROUP if p == order3 else NOT_ON_CURVE if p == off else 0 for p in pts]
    recs = np.array([_record(p) for p in pts], dtype=np.uint32)
    before = recs.copy()
    flags = np.full(len(pts), 0x77, dtype=np.uint8)
    guard = np.zeros(1, dtype=np.uint32)
    assert lib.dvc_membership(_p(recs), len(pts), clear, _p(flags, U8P), _p(guard)) == 0
    assert guard[0] == 1
    assert flags.tolist() == want
    for i, f in enumerate(want):
        if f and clear:
            assert not recs[i].any(), i                        # a failing record became the identity
        else:
            assert (recs[i] == before[i]).all(), i
