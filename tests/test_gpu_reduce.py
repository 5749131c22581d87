"""The MSM's bucket reduction -- msm_reduce.hip compiled as the library compiles it, behind the test-only harness
tests/cpp/libdevice_reduce.so -- on bucket arrays chosen here instead of the sums of distinct SRS points a whole MSM
produces: every bucket a known multiple of G (tests/reduce_cases.py), so every bit plane and every set sum is one scalar
multiplication with Python integers.  Shapes: the smallest c that reaches each code path of the two- and four-launch forms;
fills: random, one point everywhere, a single bucket per set (first, last, middle: pins w(k)), P / -P alternating, the same
point in two representations on adjacent buckets, all identity.  Equality of group elements, no tolerances."""
import ctypes
import os

import numpy as np
import pytest

import arith_cases as C
import reduce_cases as RC
from helpers import ROOT

pytestmark = pytest.mark.gpu

U32P = ctypes.POINTER(ctypes.c_uint32)
RC2, RC4 = 0, 1          # launch_msm_rc2_reduce / launch_msm_rc_reduce


@pytest.fixture(scope="module")
def lib(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpp", "libdevice_reduce.so"))
    lib.dr_reduce.restype = ctypes.c_int
    lib.dr_reduce.argtypes = [ctypes.c_int, U32P, U32P, U32P, U32P]
    assert lib.dr_rc_nb() == RC.RC_NB
    return lib


def _reduce(lib, form, sh, idx, combine):
    buckets = RC.pool().buckets(idx)
    planes = np.full((sh["nsets"] * 2 * RC.RC_NB, 48), 0xFFFFFFFF, dtype=np.uint32)
    sets = np.full((sh["nsets"], 48), 0xFFFFFFFF, dtype=np.uint32)
    words = RC.shape_words(sh)
    rc = lib.dr_reduce(form, words.ctypes.data_as(U32P), buckets.ctypes.data_as(U32P), planes.ctypes.data_as(U32P),
                       sets.ctypes.data_as(U32P) if combine else None)
    assert rc == 0, f"HIP error {rc}"
    return planes, sets


def _point(words, what):
    c = RC.unpack48(words)
    assert C._xyzz_ok(c), f"{what}: XYZZ invariants X < 5.1p, Y < 3.2p, ZZ, ZZZ < 1.1p"
    return C.xyzz_point(c)


def _check_planes(sh, idx, planes):
    want = RC.ref_planes(sh, idx)
    fails = []
    for (s, kind, b), scalar in want.items():
        try:
            got = _point(planes[(s * 2 + kind) * RC.RC_NB + b], "plane")
            assert got == RC.point_of(scalar), "point"
        except AssertionError as e:
            fails.append(f"set {s} {'column' if kind else 'row'} plane {b}: {e}")
    assert not fails, f"{len(fails)} of {len(want)} planes wrong, first: " + "; ".join(fails[:4])


# (c, form): c = 8 the msm_rc_bits / msm_rc_final tail; 13 the smallest two-launch shape (sr = sc = 0) and the planes kernel
# with one partial per item; 14 an asymmetric split; 17 the shard shape; 18 several buckets per lane in the first launch
# (sr, sc > 0); 20 the four-launch form of the benchmark's MSM
TABLE_SHAPES = [(8, RC4), (13, RC2), (13, RC4), (14, RC2), (14, RC4), (17, RC2), (17, RC4), (18, RC2)]


@pytest.mark.parametrize("fill", RC.FILLS)
@pytest.mark.parametrize("c,form", TABLE_SHAPES)
def test_one_shared_set(lib, c, form, fill):
    sh = RC.shape_of(c)
    idx = RC.fill(sh, fill)
    planes, _ = _reduce(lib, form, sh, idx, False)
    _check_planes(sh, idx, planes)


@pytest.mark.parametrize("fill", ["random", "adjacent"])
def test_one_shared_set_of_2_19_buckets(lib, fill):
    sh = RC.shape_of(20)
    idx = RC.fill(sh, fill)
    planes, _ = _reduce(lib, RC4, sh, idx, False)
    _check_planes(sh, idx, planes)


PLAIN = [(c, form, v) for c, form in ((8, RC4), (13, RC2), (13, RC4)) for v in (0, 1, RC.shape_of(c)["cl"], RC.shape_of(c)["cl"] + 2)]


@pytest.mark.parametrize("fill", RC.FILLS)
@pytest.mark.parametrize("c,form,top_v", PLAIN)
def test_three_sets_with_virtual_copies(lib, c, form, top_v, fill):
    """a plain MSM's shape: the last of three sets spreads its digits over 2^top_v virtual copies (top_v = cl + 2: the
    v > cl branch of rc_weight, rows only); the planes, then launch_msm_rc_combine's set sums sum_k ((k >> v) + 1) B_k"""
    sh = RC.shape_of(c, 3, top_v)
    idx = RC.fill(sh, fill)
    planes, sets = _reduce(lib, form, sh, idx, True)
    _check_planes(sh, idx, planes)
    want = RC.ref_set_sums(sh, idx)
    got = [_point(sets[s], f"set sum {s}") for s in range(3)]
    assert got == [RC.point_of(x) for x in want]


def test_harness_refuses_shapes_the_kernels_do_not_take(lib):
    """cl + ch != c1, the two-launch form below cl, ch = 6, more planes than RC_NB, a fold over more than one wavefront"""
    buckets = np.zeros((1 << 12, 48), dtype=np.uint32)
    planes = np.zeros((2 * RC.RC_NB, 48), dtype=np.uint32)
    bad = [(RC2, dict(RC.shape_of(8))), (RC4, dict(RC.shape_of(13), c1=11)), (2, RC.shape_of(13)),
           (RC4, dict(RC.shape_of(13), nsets=0)), (RC4, dict(RC.shape_of(13), llc=0, lhc=0, cl=12, ch=0)),
           (RC4, dict(RC.shape_of(13), lhc=7))]
    for form, sh in bad:
        words = RC.shape_words(sh)
        assert lib.dr_reduce(form, words.ctypes.data_as(U32P), buckets.ctypes.data_as(U32P), planes.ctypes.data_as(U32P), None) == 1
