"""The MSM's bucket sorts -- msm_sort.hip compiled as the library compiles it, behind the test-only harness
tests/cpp/libdevice_sort.so -- judged by everything they hand to the accumulation instead of by the MSM's point: counts, offsets,
the entries of every bucket, the size-ordered schedule, the heavy-bucket and task lists with their counters, and the byte sizes
msm_plan() gives each buffer (every buffer ends in a guard band).  The harness plans the MSM itself and runs one chunk's sort as
msm_queue does: the segmented sort in the chunk's planned shape, or (force_atomic, plain inputs) the atomic counting sort that the
plan keeps for single chunks of more than 2^23 terms.  The reference is tests/msm_sort_ref.py, held against big integers by
tests/test_msm_sort_ref.py, which also pins the path every case below takes.  Integers throughout: every comparison is exact."""
import ctypes
import os

import numpy as np
import pytest

import msm_sort_ref as SR
from helpers import ROOT

pytestmark = pytest.mark.gpu

U32P = ctypes.POINTER(ctypes.c_uint32)
INVALID = 1   # hipErrorInvalidValue


@pytest.fixture(scope="module")
def lib(built):
    try:    # PyTorch's bundled HIP runtime must be loaded before the system one the harness links (typlonk_amd.capi.load_library says
        import torch  # noqa: F401  why), or the tests that use torch later in the same process find no device
    except ImportError:
        pass
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpp", "libdevice_sort.so"))
    plan_args = [ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_uint32]
    lib.ds_plan.restype = ctypes.c_int
    lib.ds_plan.argtypes = plan_args + [U32P]
    lib.ds_sort.restype = ctypes.c_int
    lib.ds_sort.argtypes = [U32P] + plan_args + [ctypes.c_int] + [U32P] * 8
    assert lib.ds_info_words() == SR.INFO_WORDS
    return lib


def _p(a):
    return a.ctypes.data_as(U32P)


def _plan(lib, case):
    info = np.zeros(SR.INFO_WORDS, dtype=np.uint32)
    rc = lib.ds_plan(case["m"], case["mode"], case["len"], case["table_c"], case["chunks"], case["staged"], case["k"], _p(info))
    assert rc == 0, f"the harness refuses the case: {rc}"
    return info


def _sort(lib, case, words, plan):
    """one chunk's sort on the device: what the harness copies back, unwritten words 0xFFFFFFFF"""
    nb, total, mt = int(plan[SR.I_NB]), int(plan[SR.I_W]) * int(plan[SR.I_MK]), int(plan[SR.I_MAX_TASKS])
    info = np.zeros(SR.INFO_WORDS, dtype=np.uint32)
    out = {name: np.full(n, 0xFFFFFFFF, dtype=np.uint32) for name, n in
           (("counts", nb), ("offsets", nb + 1), ("sorted", total), ("order", nb), ("sched", 514), ("heavy", 4 * mt), ("tasks", 3 * mt))}
    rc = lib.ds_sort(_p(words), case["m"], case["mode"], case["len"], case["table_c"], case["chunks"], case["staged"], case["k"],
                     case["atomic"], _p(info), *[_p(out[n]) for n in ("counts", "offsets", "sorted", "order", "sched", "heavy", "tasks")])
    assert rc == 0, f"HIP error {rc}"
    out["heavy"] = out["heavy"].reshape(-1, 4)
    out["tasks"] = out["tasks"].reshape(-1, 3)
    out["guards"] = int(info[SR.I_GUARDS])
    return info, out


PARAMS = [pytest.param(case, kind, id=f"{case['name']}-{kind}") for case in SR.CASES for kind in case["kinds"]]


@pytest.mark.parametrize("case,kind", PARAMS)
def test_sort_hands_on_what_the_reference_says(lib, case, kind):
    """the six conditions of the reference's verify(): counts and offsets; every bucket's multiset of entries; order a permutation
    with min(count, 255) not rising; the heavy buckets, their tasks and both counters; the atomic sort's size histogram; every
    guard band intact"""
    plan = _plan(lib, case)
    c, W, top_v, nb, cap = (int(plan[i]) for i in (SR.I_C, SR.I_W, SR.I_DIGIT_V, SR.I_NB, SR.I_CAP))
    tables, centred, off, mk = bool(plan[SR.I_TABLES]), bool(plan[SR.I_CENTRED]), int(plan[SR.I_OFF]), int(plan[SR.I_MK])
    shape = plan[SR.I_SHAPE:SR.I_SHAPE + 14]
    # the reference takes from the plan only what the issue of an MSM fixes; W and top_v follow from c here as well
    assert W == SR.windows(c, centred) and top_v == (0 if tables else SR.plain_top_v(c, W)) and nb == (1 if tables else W) << (c - 1)
    assert tables == bool(case["table_c"]) and (not tables or (c == case["table_c"] and int(shape[SR.S_TLEN]) == case["len"]))
    assert int(plan[SR.I_NCH]) == case["expect"]["nch"] and 0 < mk <= case["m"]
    ks = SR.scalars(kind, case["m"], c)
    info, got = _sort(lib, case, SR.montgomery_words(ks), plan)
    assert (info[:SR.I_STAGED] == plan[:SR.I_STAGED]).all() and (info[SR.I_NCH:SR.I_ATOMIC] == plan[SR.I_NCH:SR.I_ATOMIC]).all()
    assert int(info[SR.I_ATOMIC]) == case["atomic"]
    if not case["atomic"]:
        assert int(plan[SR.I_SEGSORT]) == 1 and int(shape[SR.S_PRIO]) == case["expect"]["prio"] and int(shape[SR.S_NSEG]) <= 8192
        assert int(info[SR.I_STAGED]) == case["staged"], "the level-1 scatter the case is there for"
    ref = SR.reference(ks[off:off + mk], c, W, top_v, centred, case["len"] if tables else 0, nb, cap)
    if kind == "zero":
        assert int(ref["offsets"][nb]) == 0
    if case["name"] in ("plain-65537", "atomic-65537") and kind == "equal":
        assert (ref["counts"][ref["heavy"]] == 65537).all() and ref["heavy"].size == W       # the 1024-entry tasks
    bad = SR.verify(ref, got, bool(case["atomic"]), lib.ds_guard_buffers())
    assert not bad, "\n".join(bad)


def test_harness_refuses_what_the_plan_refuses(lib):
    """a chunk the plan does not have, more terms than the SRS has points, a window typlonk_srs_precompute refuses, 2^31 entries
    (32-bit entry indices), a mode that is neither stand-alone nor queued, and the atomic sort for a table-mode plan"""
    words = np.zeros((4, 8), dtype=np.uint32)
    info = np.zeros(SR.INFO_WORDS, dtype=np.uint32)
    out = np.zeros(16, dtype=np.uint32)
    #      m, mode, len, table_c, chunks, staged, k, force_atomic
    bad = [(4, 2, 4, 0, 0, 1, 1, 0), (5, 2, 4, 0, 0, 1, 0, 0), (0, 2, 4, 0, 0, 1, 0, 0), (4097, 2, SR.TABLE_LEN, 13, 0, 1, 0, 0),
           (1 << 27, 2, 1 << 27, 0, 0, 1, 0, 0), (4, 3, 4, 0, 0, 1, 0, 0), (8193, 0, 8193, 0, 2, 1, 2, 0),
           (4097, 2, SR.TABLE_LEN, 20, 0, 1, 0, 1)]
    for a in bad:
        assert lib.ds_sort(_p(words), *a, _p(info), *[_p(out)] * 7) == INVALID, a
        if not a[7]:
            assert lib.ds_plan(*a[:7], _p(info)) == INVALID, a
