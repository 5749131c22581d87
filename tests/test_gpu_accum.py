"""The MSM's bucket accumulation -- msm_accum.hip compiled as the library compiles it, behind the test-only harness
tests/cpp/libdevice_accum.so -- bucket by bucket, on sort outputs made in tests/accum_cases.py instead of whatever msm_plan() gives
a whole MSM: msm_accum_kernel, msm_accum_ml_kernel<2|4|8|16> in one and in two size classes at splits the launcher rounds, a
continuing chunk (init = 1) over stored buckets, and msm_heavy_kernel with 1, 2, 64 and 65 tasks per bucket, 1024-entry tasks and
more tasks than the launch has wavefronts.  Every bucket and every task partial is read back: within the stored-XYZZ bounds, equal
as a group element to (stored e + sum of +-e_i) G, and word for word the stored bucket where nothing was to be added.  Integers and
group equality throughout, no tolerances.  tests/test_accum_cases.py holds the cases to the paths they are there for."""
import ctypes
import os

import numpy as np
import pytest

import accum_cases as A
import reduce_cases as RC
from helpers import ROOT

pytestmark = pytest.mark.gpu

U32P = ctypes.POINTER(ctypes.c_uint32)
UNWRITTEN = 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib(built):
    try:    # PyTorch's bundled HIP runtime must be loaded before the system one the harness links (typlonk_amd.capi.load_library says
        import torch  # noqa: F401  why), or the tests that use torch later in the same process find no device
    except ImportError:
        pass
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpp", "libdevice_accum.so"))
    lib.da_accum.restype = ctypes.c_int
    lib.da_accum.argtypes = [U32P, ctypes.c_uint64, U32P, U32P, ctypes.c_uint64, U32P] + [ctypes.c_uint32] * 5 + [U32P] * 4 \
        + [ctypes.c_uint64] + [U32P] * 4
    return lib


def _p(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.uint32).ctypes.data_as(U32P)


def _call(lib, a, lanes, split, init, stored, points=None, npoints=None):
    """one da_accum call: (rc, buckets, partials, heavy records, guard bits); what the harness does not write stays UNWRITTEN"""
    points = A.pool().words if points is None else points
    nheavy, ntasks = (int(a["sched"][512]), int(a["sched"][513])) if a["sched"] is not None else (0, 0)
    buckets = np.full((a["nb"], 48), UNWRITTEN, dtype=np.uint32)
    partial = np.full((max(ntasks, 1), 48), UNWRITTEN, dtype=np.uint32)
    heavy = np.full((max(nheavy, 1), 4), UNWRITTEN, dtype=np.uint32)
    guards = np.full(1, UNWRITTEN, dtype=np.uint32)
    keep = [np.ascontiguousarray(x, dtype=np.uint32) if x is not None else None
            for x in (points, a["offsets"], a["sorted"], a["order"], stored, a["sched"], a["heavy"], a["tasks"])]
    ptr = [None if x is None else x.ctypes.data_as(U32P) for x in keep]
    rc = lib.da_accum(ptr[0], len(points) if npoints is None else npoints, ptr[1], ptr[2], a["total"], ptr[3], a["nb"], a["cap"], init,
                      lanes, split, ptr[4], ptr[5], ptr[6], ptr[7], a["max_tasks"], _p(buckets), _p(partial), _p(heavy), _p(guards))
    return rc, buckets, partial[:ntasks], heavy[:nheavy], int(guards[0])


def _run(lib, a, lanes, split, init, stored_idx=None, heavy_pass=False):
    """run the case and hold every bucket (and, with the heavy pass, every partial and counter) against the integers"""
    assert A.admit(a, len(A.pool().e), lanes, init, stored_idx)
    stored = RC.pool().buckets(stored_idx) if init else None
    run = a if heavy_pass else dict(a, sched=None, heavy=None, tasks=None, max_tasks=0)
    rc, buckets, partial, heavy, guards = _call(lib, run, lanes, split, init, stored)
    assert rc == 0, f"HIP error {rc}"
    want, untouched = A.expected(a, RC.pool().e[stored_idx] if init else None, heavy_pass)
    bad = A.wrong_points(buckets, want, a["counts"], untouched if init else None, stored)
    assert not bad, f"{len(bad)} of {a['nb']} buckets wrong, first: " + "; ".join(bad[:4])
    assert guards == 3, f"written past the buckets or the partials: intact mask {guards:#x}"
    if heavy_pass:
        assert np.array_equal(heavy[:, :3], a["heavy"][:, :3]), "the heavy records changed"
        late = np.flatnonzero(heavy[:, 3] != a["heavy"][:, 2])
        assert late.size == 0, f"{late.size} done counters differ from their task counts, first records {late[:4].tolist()}"
        bad = A.wrong_points(partial, A.task_sums(a))
        assert not bad, f"{len(bad)} of {partial.shape[0]} task partials wrong, first: " + "; ".join(bad[:4])


@pytest.mark.parametrize("order", ["falling", "scrambled"])
def test_one_thread_per_bucket(lib, order):
    """msm_accum_kernel: counts 0, 1, 2, 31, 32 under cap 32, P P / P -P / -P -P 2P as neighbours, identity bases, a bucket that ends
    as the identity, one above cap (stored as the identity: the heavy pass would fill it)"""
    _run(lib, A.thread_case(order), 1, 0, 0)


@pytest.mark.parametrize("split", ["all", "half", "rounded", "none"])
@pytest.mark.parametrize("lanes", A.LANES)
def test_lanes_and_split(lib, lanes, split):
    """msm_accum_ml_kernel<lanes>: counts around every lane count, 300 buckets (no multiple of a workgroup's), one expected table for
    one class, two classes at half the slots, a split the launcher rounds down and one it rounds to 0; equal and opposite points
    at every power-of-two distance, so that a lane's own addition, the pair step and a later step each settle some"""
    a = A.lanes_case()
    _run(lib, a, lanes, A.splits(a["nb"], lanes)[split], 0)


@pytest.mark.parametrize("lanes", [1, 4, 16])
def test_continuing_chunk(lib, lanes):
    """init = 1 over stored buckets under several Z scalings and both identity encodings, the schedule scrambled, two size classes:
    P stored under P and under -P, empty and above-cap buckets word for word as stored, nothing written past the last bucket"""
    a = A.lanes_case("scrambled")
    _run(lib, a, lanes, a["nb"] // 2, 1, A.stored_for(a, 5))


@pytest.mark.parametrize("lanes,init", [(1, 0), (1, 1), (4, 1)])
def test_heavy_buckets(lib, lanes, init):
    """msm_heavy_kernel behind the accumulation, cap 32: 1, 1, 2, 64, 65 tasks of 256 entries, 64 and 65 of 1024, tasks of one entry,
    2082 tasks on 2048 wavefronts; every done counter at its k, every partial its own sum, the bucket the sum of them all on top of
    the identity (init = 0) or of the stored bucket (init = 1) the accumulation left alone"""
    a = A.heavy_case()
    _run(lib, a, lanes, a["nb"] // 2, init, A.stored_for(a, 6) if init else None, heavy_pass=True)


def test_harness_refuses_what_could_leave_an_array(lib):
    """every malformed input of tests/accum_cases.malformed() comes back as hipErrorInvalidValue with no output word written"""
    a = A.small_case()
    stored = RC.pool().buckets(A.stored_for(a, 7))
    rc, buckets, *_ = _call(lib, a, 4, 2, 1, stored)
    assert rc == 0 and (buckets != UNWRITTEN).any(), "the well-formed case itself"
    for what, b, kw in A.malformed(a, len(A.pool().e)):
        rc, buckets, partial, heavy, guards = _call(lib, b, kw.get("lanes", 4), 2, kw.get("init", 1), None if kw.get("no_stored") else stored,
                                                    npoints=kw.get("npoints"))
        assert rc == A.INVALID, f"{what}: {rc}"
        assert (buckets == UNWRITTEN).all() and (partial == UNWRITTEN).all() and (heavy == UNWRITTEN).all() and guards == UNWRITTEN, what
