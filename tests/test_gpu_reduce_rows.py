"""The row form of the bucket reduction on the device (tests/cpp/libdevice_reduce_rows.so over csrc/fq30_rows.hpp and
msm_reduce.hip as the library compiles it).

(a) g1_add_rows, one XYZZ addition per wavefront, on the point pairs of tests/test_fq30_rows_host.py -- random pairs, the
    identity on either side and both, P + P, P + (-P), one point in two representations -- 64 pairs in one launch, against
    g1_add on the same words as affine points, and against the integers.
(b) The bit planes summed one addition per wavefront against the same planes summed one thread per point
    (msm_rc2_planes_kernel, the four-launch form before the row kernels) on the same bucket arrays, plane by plane as affine
    points, and both against the integers (tests/reduce_cases.py).  Shapes: the smallest the kernels take; ch != cl; two sets
    with virtual copies in the top one; the benchmark's 2^19 buckets.  Fills: random points; all identity but one bucket; all
    identity but one row of equal points, so that every column sum is that point and every level of a column plane doubles.
(c) Whole MSMs under TYPLONK_MSM_REDUCE=rc4 against the CPU bucket method: 2^10 terms plain, 2^14 terms with c = 15 tables.
Equality of group elements, no tolerances."""
import ctypes
import os

import numpy as np
import pytest

import arith_cases as C
import reduce_cases as RC
import test_fq30_rows_host as H
from helpers import O, ROOT

pytestmark = pytest.mark.gpu

U32P = ctypes.POINTER(ctypes.c_uint32)
ROWS, LANES = 0, 1


@pytest.fixture(scope="module")
def lib(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpp", "libdevice_reduce_rows.so"))
    lib.drr_reduce.restype = ctypes.c_int
    lib.drr_reduce.argtypes = [ctypes.c_int, U32P, U32P, U32P]
    lib.drr_add_pairs.restype = ctypes.c_int
    lib.drr_add_pairs.argtypes = [U32P, U32P, ctypes.c_uint32, U32P, U32P, U32P]
    return lib


# ---- (a) ---------------------------------------------------------------------------------------------------------------------
def _words(limbs52):
    """52 loose limbs (X, Y, ZZ, ZZZ) -> the 48 packed words of the stored point"""
    out = []
    for c in range(4):
        v = H.val(limbs52[13 * c:13 * c + 13])
        out += [(v >> (32 * j)) & 0xFFFFFFFF for j in range(12)]
    return out


def test_g1_add_rows_on_the_device_equals_g1_add_and_the_integers(lib):
    pairs = H.point_pairs()
    assert len(pairs) == 64
    a = np.array([_words(la) for _, _, la, _ in pairs], dtype=np.uint32)
    b = np.array([_words(lb) for _, _, _, lb in pairs], dtype=np.uint32)
    rows = np.full((64, 48), 0xFFFFFFFF, dtype=np.uint32)
    lane = np.full((64, 48), 0xFFFFFFFF, dtype=np.uint32)
    slow = np.full(64, 0xFFFFFFFF, dtype=np.uint32)
    rc = lib.drr_add_pairs(a.ctypes.data_as(U32P), b.ctypes.data_as(U32P), 64, rows.ctypes.data_as(U32P), lane.ctypes.data_as(U32P),
                           slow.ctypes.data_as(U32P))
    assert rc == 0, f"HIP error {rc}"
    for i, (ka, kb, _, _) in enumerate(pairs):
        r, l = RC.unpack48(rows[i]), RC.unpack48(lane[i])
        H.check_sum(ka, kb, *r)                                       # the affine sum, within the stored invariants
        assert C.xyzz_point(r) == C.xyzz_point(l), (ka, kb)           # ... and what g1_add gives on the same words
        assert slow[i] == (1 if ka == 0 or kb == 0 or ka == kb or ka == -kb else 0), (ka, kb)


# ---- (b) ---------------------------------------------------------------------------------------------------------------------
SHAPES = [
    dict(nsets=1, c1=12, ch=6, cl=6, lhc=3, llc=3, top_v=0),
    dict(nsets=1, c1=13, ch=6, cl=7, lhc=3, llc=3, top_v=0),
    dict(nsets=2, c1=12, ch=6, cl=6, lhc=3, llc=3, top_v=5),
    dict(nsets=1, c1=19, ch=9, cl=10, lhc=3, llc=3, top_v=0),
]
FILLS = ("random", "one_middle", "equal_row")


def _fill(sh, name):
    if name != "equal_row":
        return RC.fill(sh, name)
    pl = RC.pool()
    idx = RC.fill(sh, "identity")
    for s in range(sh["nsets"]):
        row = (1 << sh["ch"]) * 5 // 8 + 1                            # bits in several row planes
        first = (s << sh["c1"]) + (row << sh["cl"])
        idx[first:first + (1 << sh["cl"])] = pl.of[(5, 1)][0]         # one point, one representation, in every column
    return idx


def _planes(lib, form, sh, buckets):
    planes = np.full((sh["nsets"] * 2 * RC.RC_NB, 48), 0xFFFFFFFF, dtype=np.uint32)
    words = RC.shape_words(sh)
    rc = lib.drr_reduce(form, words.ctypes.data_as(U32P), buckets.ctypes.data_as(U32P), planes.ctypes.data_as(U32P))
    assert rc == 0, f"HIP error {rc}"
    return planes


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("sh", SHAPES, ids=lambda s: "-".join(str(s[k]) for k in ("nsets", "c1", "ch", "cl", "top_v")))
def test_planes_one_addition_per_wavefront_equal_one_thread_per_point(lib, sh, fill):
    idx = _fill(sh, fill)
    buckets = RC.pool().buckets(idx)
    rows, lanes = _planes(lib, ROWS, sh, buckets), _planes(lib, LANES, sh, buckets)
    want = RC.ref_planes(sh, idx)
    fails = []
    for (s, kind, b), scalar in want.items():
        at = (s * 2 + kind) * RC.RC_NB + b
        r, l = RC.unpack48(rows[at]), RC.unpack48(lanes[at])
        try:
            assert C._xyzz_ok(r), "XYZZ invariants X < 5.1p, Y < 3.2p, ZZ, ZZZ < 1.1p"
            assert C.xyzz_point(r) == C.xyzz_point(l), "differs from the one-thread-per-point plane"
            assert C.xyzz_point(r) == RC.point_of(scalar), "differs from the integers"
        except AssertionError as e:
            fails.append(f"set {s} {'column' if kind else 'row'} plane {b}: {e}")
    assert not fails, f"{len(fails)} of {len(want)} planes wrong, first: " + "; ".join(fails[:4])
    # planes the shape does not have stay as the harness zeroed them
    live = {(s * 2 + kind) * RC.RC_NB + b for (s, kind, b) in want}
    for at in range(len(rows)):
        if at not in live:
            assert not rows[at].any()


def test_harness_refuses_shapes_the_row_kernels_do_not_take(lib):
    buckets = np.zeros((1 << 12, 48), dtype=np.uint32)
    planes = np.zeros((2 * RC.RC_NB, 48), dtype=np.uint32)
    for form, sh in ((ROWS, dict(SHAPES[0], c1=10, ch=5, cl=5)), (2, SHAPES[0]), (ROWS, dict(SHAPES[0], c1=11)),
                     (ROWS, dict(SHAPES[0], nsets=0))):
        words = RC.shape_words(sh)
        assert lib.drr_reduce(form, words.ctypes.data_as(U32P), buckets.ctypes.data_as(U32P), planes.ctypes.data_as(U32P)) == 1


# ---- (c) ---------------------------------------------------------------------------------------------------------------------
def _limbs(v):
    return np.array(O.fr_to_mont_limbs(v % O.R), dtype=np.uint64)


@pytest.mark.parametrize("log_m,table_c", [(10, 0), (14, 15)])
def test_whole_msm_under_rc4_equals_the_cpu_bucket_method(built, log_m, table_c, monkeypatch):
    import typlonk_amd
    from oracle import coracle as CO

    monkeypatch.setenv("TYPLONK_MSM_REDUCE", "rc4")
    c2 = typlonk_amd.Context(0)
    try:
        m = 1 << log_m
        h = c2.srs_generate(_limbs(0x0123456789ABCDEF0123456789ABCDEF), m)
        xy, inf = c2.srs_download(h)
        if table_c:
            c2.srs_precompute(h, table_c)
        rng = np.random.default_rng(log_m)
        sc = rng.integers(0, 1 << 63, size=(m, 4), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(m, 4), dtype=np.uint64)
        sc[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)                     # < 2^254 < r: any limb pattern is a valid Montgomery residue
        exp, einf, _, _ = CO.msm_pippenger(sc, xy, inf, c=11)
        got, ginf = c2.msm(h, sc)
        assert (got == exp).all() and ginf == einf
    finally:
        c2.close()
