"""The device build of the paired Fq30 products (fq30_mul_pair, fq30_sqr_pair, fq30_mul2_add: the interleaved column
chains of typlonk_amd/csrc/fq30_pair.hpp) against Python integers, through the test-only harness
tests/cpp/libdevice_pair.so.  Same cases and checks as the host test (tests/fq30_pair_cases.py)."""
import ctypes
import os

import pytest

import fq30_pair_cases as FP
from helpers import ROOT

pytestmark = pytest.mark.gpu

U32P = ctypes.POINTER(ctypes.c_uint32)


@pytest.fixture(scope="module")
def device(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpp", "libdevice_pair.so"))
    lib.fp_device.restype = ctypes.c_int
    lib.fp_device.argtypes = [ctypes.c_int] + [U32P] * 6 + [ctypes.c_int]
    return lambda op, *arrs: lib.fp_device(op, *[a.ctypes.data_as(U32P) for a in arrs[:6]], arrs[6])


@pytest.mark.parametrize("op", [FP.OP_MUL_PAIR, FP.OP_SQR_PAIR, FP.OP_MUL2_ADD], ids=["mul_pair", "sqr_pair", "mul2_add"])
def test_fq30_pair_device(device, op):
    FP.run_and_check(device, op)
