"""The shipped device arithmetic -- ff.hpp's Fr, fq30.hpp, fr30.hpp, fr_inv.hpp, g1.hpp and the wavefront butterflies of
msm_common.hpp, compiled for gfx950 exactly as the library's units compile them -- on chosen inputs, through the test-only harness tests/cpp/libdevice_arith.so.  Every
result is checked against Python integers: its residue, its limb form, and the value bound the function's comment
promises.  Case lists and checks: tests/arith_cases.py (their preconditions are asserted on the CPU too,
tests/test_arith_cases.py).  tests/test_host.py covers the host branches of the same headers."""
import ctypes
import os

import numpy as np
import pytest

import arith_cases as C
from helpers import ROOT

pytestmark = pytest.mark.gpu

I32P = ctypes.POINTER(ctypes.c_int32)
U32P = ctypes.POINTER(ctypes.c_uint32)


@pytest.fixture(scope="module")
def lib(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpp", "libdevice_arith.so"))
    for fn, n in (("da_fr", 6), ("da_fq30", 8), ("da_fr30", 6), ("da_g1", 7)):
        getattr(lib, fn).restype = ctypes.c_int
        getattr(lib, fn).argtypes = [ctypes.c_int] + [U32P] * (n - 3) + [I32P, ctypes.c_int]
    lib.da_wave.restype = ctypes.c_int
    lib.da_wave.argtypes = [ctypes.c_int, ctypes.c_int, U32P, U32P, I32P, ctypes.c_int]
    return lib


def _arr(rows, width: int, bits: int = 30) -> np.ndarray:
    """rows of ints (values, split into `bits`-bit limbs) or of limb lists -> (n, width) uint32"""
    out = np.zeros((len(rows), width), dtype=np.uint32)
    for i, r in enumerate(rows):
        ls = r if isinstance(r, (list, tuple)) else C.limbs(r, (r.bit_length() + bits - 1) // bits or 1, bits)
        out[i, :len(ls)] = ls
    return out


def _call(fn, code: int, ins: list[np.ndarray], width: int, n: int):
    out = np.zeros((n, width), dtype=np.uint32)
    aux = np.full(n, -7, dtype=np.int32)
    args = [np.ascontiguousarray(a) for a in ins]
    rc = fn(code, *[a.ctypes.data_as(U32P) for a in args], out.ctypes.data_as(U32P), aux.ctypes.data_as(I32P), n)
    assert rc == 0, f"HIP error {rc}"
    assert (aux != -7).all() and (aux != -1).all(), "harness did not run every case"
    return out, aux


def _preconditions(name, pre, cases):
    n = C.distinct(cases)
    assert n >= C.min_distinct(name), f"{name}: only {n} distinct cases"
    bad = [i for i, c in enumerate(cases) if not pre(*c)]
    assert not bad, f"{name}: cases {bad[:5]} break the function's precondition (the case list is wrong, not the kernel)"


def _report(name, failures, n):
    assert not failures, f"{name}: {len(failures)} of {n} cases wrong, first: " + "; ".join(failures[:4])


@pytest.mark.parametrize("name", list(C.FR_OPS))
def test_fr(lib, name):
    code, make, pre, want = C.FR_OPS[name]
    cases = make()
    _preconditions(name, pre, cases)
    n = len(cases)
    a = _arr([c[0] for c in cases], 8, 32)
    b = _arr([c[1] if len(c) > 1 else 0 for c in cases], 8, 32)
    out, aux = _call(lib.da_fr, code, [a, b], 8, n)
    fails = []
    for i, c in enumerate(cases):
        got = C.val(out[i], 32)
        if got != want(*c):
            fails.append(f"#{i} {[hex(x) for x in c]} -> {hex(got)}, want {hex(want(*c))}")
        elif name == "fr_inv_divsteps" and not 0 <= aux[i] <= 25:
            fails.append(f"#{i}: {aux[i]} rounds > FR_DIVSTEP_ROUNDS")
    _report(name, fails, n)


@pytest.mark.parametrize("name", list(C.FQ_OPS))
def test_fq30(lib, name):
    code, make, pre = C.FQ_OPS[name]
    cases = make()
    _preconditions(name, pre, cases)
    n = len(cases)
    bits_in = 32 if name in C.FQ_WORDS_IN else 30
    ins = [_arr([c[k] if k < len(c) else 0 for c in cases], 13, bits_in) for k in range(4)]
    out, aux = _call(lib.da_fq30, code, ins, 13, n)
    fails = []
    for i, c in enumerate(cases):
        try:
            if name in C.FQ_WORDS_OUT:
                assert not out[i, 12], "word 12 written"
                got = C.val(out[i, :12], 32)
            else:
                assert (out[i] <= C.M30).all(), "limbs not normalised (< 2^30)"
                got = C.val(out[i])
            C.fq_check(name, c, got, int(aux[i]))
        except AssertionError as e:
            fails.append(f"#{i} {[hex(x) for x in c]}: {e}")
    _report(name, fails, n)


@pytest.mark.parametrize("name", list(C.FR30_OPS))
def test_fr30(lib, name):
    code, make, pre = C.FR30_OPS[name]
    cases = make()
    _preconditions(name, pre, cases)
    n = len(cases)
    ins = [_arr([c[k] if k < len(c) else [0] * 9 for c in cases], 9) for k in range(2)]
    out, _ = _call(lib.da_fr30, code, ins, 9, n)
    fails = []
    for i, c in enumerate(cases):
        try:
            C.fr30_check(name, c, [int(x) for x in out[i]])
        except AssertionError as e:
            fails.append(f"#{i} {[[hex(x) for x in a] for a in c]} -> {[hex(x) for x in out[i]]}: {e}")
    _report(name, fails, n)


@pytest.mark.parametrize("name", list(C.G1_OPS))
def test_g1(lib, name):
    cases = C.g1_cases(name)
    _preconditions(name, lambda a, b, f: C.g1_pre(name, a, b, f), cases)
    n = len(cases)
    pack = lambda coords: [limb for v in coords for limb in C.limbs(v, 13)]  # noqa: E731
    a = _arr([pack(c[0]) for c in cases], 52)
    b = _arr([pack(c[1]) for c in cases], 52)
    f = _arr([[int(c[2])] for c in cases], 1)
    out, _ = _call(lib.da_g1, C.G1_OPS[name], [a, b, f], 52, n)
    fails = []
    for i, (ca, cb, fl) in enumerate(cases):
        try:
            assert (out[i] <= C.M30).all(), "limbs not normalised (< 2^30)"
            C.g1_check(name, ca, cb, int(fl), [C.val(out[i, 13 * k:13 * k + 13]) for k in range(4)])
        except AssertionError as e:
            fails.append(f"#{i}: {e}")
    _report(name, fails, n)


@pytest.mark.parametrize("name,param", [(name, param) for name in C.WAVE_OPS for param in C.WAVE_PARAMS[name]])
def test_wave(lib, name, param):
    """butterfly_add / butterfly_add4 / butterfly_reduce (msm_common.hpp) on whole wavefronts of chosen points, every lane's
    result read back: the sum as a group element, the XYZZ invariants, ZZ^3 = ZZZ^2, and identical words on the lanes the
    next four-lane step reads as one operand -- in the formula's path and in every exceptional one (equal points in two
    representations or in the same words, opposite points, the identity in either encoding on one or both sides; on every
    pair of a wave, and on one pair of an otherwise ordinary wave)."""
    cases = [(label, wave) for label, p, wave in C.wave_cases(name) if p == param]
    bad = [label for label, wave in cases if not C.wave_pre(name, param, wave)]
    assert not bad, f"{name}: waves {bad[:5]} break the precondition (the case list is wrong, not the kernel)"
    n = len(cases) * C.WAVE
    pack = lambda coords: [limb for v in coords for limb in C.limbs(v, 13)]  # noqa: E731
    a = _arr([pack(c) for _, wave in cases for c in wave], 52)
    out = np.zeros((n, 52), dtype=np.uint32)
    aux = np.full(n, -7, dtype=np.int32)
    rc = lib.da_wave(C.WAVE_OPS[name], param, a.ctypes.data_as(U32P), out.ctypes.data_as(U32P), aux.ctypes.data_as(I32P), n)
    assert rc == 0, f"HIP error {rc}"
    assert (aux == 0).all(), "harness did not run every lane"
    fails = []
    for k, (label, wave) in enumerate(cases):
        rows = out[k * C.WAVE:(k + 1) * C.WAVE]
        try:
            assert (rows <= C.M30).all(), "limbs not normalised (< 2^30)"
            C.wave_check(name, param, wave, [tuple(C.val(r[13 * j:13 * j + 13]) for j in range(4)) for r in rows])
        except AssertionError as e:
            fails.append(f"{label}: {e}")
    _report(f"{name}({param})", fails, len(cases))


def test_wave_refuses_what_the_butterflies_do_not_take(lib):
    """a mask or lane count outside the wavefront (or not a power of two) and a partial wavefront never reach the device"""
    buf = np.zeros((C.WAVE, 52), dtype=np.uint32)
    aux = np.zeros(C.WAVE, dtype=np.int32)
    args = (buf.ctypes.data_as(U32P), buf.ctypes.data_as(U32P), aux.ctypes.data_as(I32P))
    for op, param, n in ((0, 64, 64), (0, 3, 64), (0, 0, 64), (1, 1, 64), (1, 64, 64), (2, 128, 64), (2, 0, 64), (0, 1, 63)):
        assert lib.da_wave(op, param, *args, n) == 1


@pytest.mark.parametrize("name,limit", [("fq30_inv_divsteps", 37), ("fr_inv_divsteps", 25)])
def test_inversion_wave_exit(lib, name, limit):
    """the divsteps loop leaves when no lane of the wave has g != 0: a wave of zeros runs no round at all, a wave of
    Montgomery ones (the same input in every lane) a few, and the mixed waves stay within the Bernstein-Yang bound.
    Deliberately pins the shipped wave-uniform exit (__any): every lane of a wave must report the same count.  A build
    that lets lanes leave on their own, or runs a fixed count (-DFQ30_INV_FIXED_ROUNDS, not what the library ships), fails
    here although its arithmetic is right -- test_fq30 / test_fr check the arithmetic."""
    if name == "fq30_inv_divsteps":
        code, make, _ = C.FQ_OPS[name]
        cases = make()
        ins = [_arr([c[0] for c in cases], 13)] + [np.zeros((len(cases), 13), dtype=np.uint32)] * 3
        _, aux = _call(lib.da_fq30, code, ins, 13, len(cases))
    else:
        code, make, _, _ = C.FR_OPS[name]
        cases = make()
        ins = [_arr([c[0] for c in cases], 8, 32), np.zeros((len(cases), 8), dtype=np.uint32)]
        _, aux = _call(lib.da_fr, code, ins, 8, len(cases))
    w = C.WAVE
    assert (aux[:w] == 0).all(), "a wave of zeros ran divsteps rounds"
    easy = aux[w:2 * w]
    assert (easy == easy[0]).all() and 0 < easy[0] < limit, "a uniform wave of ones"
    assert aux.max() <= limit
    for k in range(len(aux) // w):                   # wave-uniform exit: every lane of a wave reports the same count
        assert len(set(aux[k * w:(k + 1) * w])) == 1, f"wave {k} lanes left the loop at different rounds"
