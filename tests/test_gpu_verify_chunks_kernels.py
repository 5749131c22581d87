"""The kernels of typlonk_verify_chunks -- verify_chunks.hip compiled as the library compiles it, behind the test-only harness
tests/cpp/libdevice_verify_chunks.so -- with their launchers called directly, against tests/verify_chunks_ref.py word for word.

chunks_weights_kernel, chunks_fold_kernel, chunks_fold_sum_kernel: the weights of a fold over [lo, hi), w_c and the l coefficients
of A, for l in {1, 2, 8, 64, 128, 1024} (a wavefront per cell up to 64, the workgroup above, one, two and four coefficients a
thread), N in {1, 2, one strip + 1, three strips with a ragged last one} for two named strip sizes and the plan's own -- every
strip size gives the same words, a sum of field elements being a canonical residue --, sub-ranges inside one strip and across
strips with dead cells inside, cosets 0 and r - 1, one cell twice, all-zero evaluations and evaluations of r - 1, every cell
under one commitment and a commitment no cell names.  chunks_membership_kernel: one flag per record, and the failing records
cleared, on the generator, an identity, the order-3 point (0, 2) and an off-curve record, over more than one wavefront."""
import ctypes

import numpy as np
import pytest

import arith_cases as AC
import verify_chunks_ref as VR
from helpers import O, ROOT, fr_pack

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

    def __init__(self, log_l, N, M, seed, one_commitment=False):
        self.log_l, self.log_n, self.N, self.M = log_l, log_l + LOG_R, N, M
        l, r = 1 << log_l, 1 << LOG_R
        rng = np.random.default_rng(seed)
        self.rho = _rand(rng, 1)[0]
        cells = []
        for i in range(N):
            ys = _rand(rng, l)
            if i == 2:
                ys = [0] * l                                   # all-zero evaluations
            if i == 3:
                ys = [R - 1] * l                               # full-range values
            k = (0, r - 1)[i] if i < 2 and N > 2 else int(rng.integers(0, r))
            c = 0 if one_commitment else int(rng.integers(0, M - 1)) if M > 1 else 0    # commitment M - 1: no cell names it
            cells.append((c, k, ys, 0))
        if N >= 6:
            cells[5] = cells[4]                                # the same cell twice
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
