"""The host build of the paired Fq30 products (fq30_mul_pair, fq30_sqr_pair, fq30_mul2_add) against Python integers,
through tests/cpp/libfq30_pair_host.so.  Cases and checks: tests/fq30_pair_cases.py; the device build of the same
functions: tests/test_gpu_fq30_pair.py."""
import ctypes
import os

import numpy as np
import pytest

import fq30_pair_cases as FP
from helpers import ROOT

U32P = ctypes.POINTER(ctypes.c_uint32)


@pytest.fixture(scope="module")
def host(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpp", "libfq30_pair_host.so"))
    lib.fp_host.restype = ctypes.c_int
    lib.fp_host.argtypes = [ctypes.c_int] + [U32P] * 6 + [ctypes.c_int]
    return lambda op, *arrs: lib.fp_host(op, *[a.ctypes.data_as(U32P) for a in arrs[:6]], arrs[6])


@pytest.mark.parametrize("op", [FP.OP_MUL_PAIR, FP.OP_SQR_PAIR, FP.OP_MUL2_ADD], ids=["mul_pair", "sqr_pair", "mul2_add"])
def test_fq30_pair_host(host, op):
    FP.run_and_check(host, op)


def test_fq30_pair_cases_differ():
    """the two chains of a call see different operands (the pairing is not a product computed twice)"""
    for op in (FP.OP_MUL_PAIR, FP.OP_SQR_PAIR):
        cs = FP.cases(op)
        assert sum(1 for a, b, c, d in cs if (a, b) != (c, d)) > len(cs) * 0.9
    assert np.array_equal(FP._arr([FP.C.FQ_R - 1])[0], np.full(13, FP.C.M30, dtype=np.uint32))
