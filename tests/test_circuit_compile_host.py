"""typlonk_circuit_compile without a GPU: the library loads and refuses a null context, and sigma_cell (csrc/sigma_cell.hpp),
the per-cell body of sigma_from_perm_kernel, as the host compiles it (tests/cpp/libsigma_cell_host.so, tables built on the
host as get_pow2l builds them) against Python integers: sigma[x] = k_col(perm[x]) * w^row(perm[x]) * 2^256 mod r, words equal.
The device build of the same body: tests/test_gpu_circuit_compile.py."""
import ctypes as C
import os

import numpy as np
import pytest

import general_circuits as G
import witness_check_ref as W
from helpers import ROOT, O

R = O.R
U32P = C.POINTER(C.c_uint32)
COSET_TRIPLES = {"2_3_4": lambda log_n: (2, 3, 4), "1_k1_k2": G.large_cosets}
SEED = 900   # + log_n: the circuits of witness_check_ref.random_circuit this file uses


def test_library_loads_without_a_device_and_refuses_a_null_context(built):
    import typlonk_amd
    from typlonk_amd.capi import ERR_INVALID_ARG, SYMBOLS

    lib = typlonk_amd.load_library()
    assert "typlonk_circuit_compile" in SYMBOLS and "typlonk_circuit_compile_host" in SYMBOLS
    cid, defects = C.c_uint32(0xA5), C.c_uint64(0xA5)
    assert lib.typlonk_circuit_compile(None, None, None, None, 5, C.byref(cid), C.byref(defects)) == ERR_INVALID_ARG
    assert lib.typlonk_circuit_compile_host(None, None, 32, None, None, 5, C.byref(cid), C.byref(defects)) == ERR_INVALID_ARG
    assert cid.value == 0xA5 and defects.value == 0xA5


@pytest.fixture(scope="module")
def shim(built):
    lib = C.CDLL(os.path.join(ROOT, "tests", "cpp", "libsigma_cell_host.so"))
    lib.sigma_cells_host.restype = C.c_int
    lib.sigma_cells_host.argtypes = [C.c_uint32, U32P, U32P, U32P, U32P, C.POINTER(C.c_ubyte)]

    def run(log_n, cosets, perm):
        n3 = 3 << log_n
        root = np.ascontiguousarray(W.mont_words([O.domain_root(log_n)])).view(np.uint32)
        ks = np.ascontiguousarray(W.mont_words(list(cosets))).view(np.uint32)
        p = np.ascontiguousarray(perm, dtype=np.uint32)
        out = np.full((n3, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        cell = np.zeros(n3, dtype=np.uint8)
        h = lib.sigma_cells_host(log_n, root.ctypes.data_as(U32P), ks.ctypes.data_as(U32P), p.ctypes.data_as(U32P),
                                 out.view(np.uint32).ctypes.data_as(U32P), cell.ctypes.data_as(C.POINTER(C.c_ubyte)))
        return h, out, cell

    return run


def expected_sigma(log_n, cosets, perm):
    """the Montgomery words of k_col(y) * w^row(y) for y = perm[x], as Python integers make them"""
    n, w = 1 << log_n, O.domain_root(log_n)
    pw = [1]
    for _ in range(n - 1):
        pw.append(pw[-1] * w % R)
    return W.mont_words([cosets[y >> log_n] * pw[y & (n - 1)] % R for y in perm])


@pytest.mark.parametrize("log_n", [1, 2, 3, 5, 6, 7])
@pytest.mark.parametrize("triple", sorted(COSET_TRIPLES))
def test_sigma_cell_on_the_host_equals_python_integers(shim, log_n, triple):
    """odd and even table splits (h = 1, 1, 2, 3, 3, 4 of log_n = 1, 2, 3, 5, 6, 7: halves of unequal size at every odd
    log_n), a random permutation and the identity"""
    n = 1 << log_n
    cosets = COSET_TRIPLES[triple](log_n)
    assert G.cosets_are_disjoint(cosets, n)
    perms = {"random": W.random_circuit(log_n, SEED + log_n)[3], "identity": list(range(3 * n))}
    assert sorted(perms["random"]) == perms["identity"] and perms["random"] != perms["identity"]
    for name, perm in perms.items():
        h, got, cell = shim(log_n, cosets, perm)
        assert h == (log_n + 1) // 2
        assert cell.all(), name
        assert np.array_equal(got, expected_sigma(log_n, cosets, perm)), name


def test_sigma_cell_refuses_what_is_no_cell(shim):
    """an entry that is not below 3n: reported, and its output left alone"""
    log_n, n = 3, 8
    perm = list(range(3 * n))
    perm[5], perm[17] = 3 * n, 0xFFFFFFFF
    _, got, cell = shim(log_n, (2, 3, 4), perm)
    assert [x for x in range(3 * n) if not cell[x]] == [5, 17]
    assert (got[[5, 17]] == 0xA5A5A5A5A5A5A5A5).all()
    keep = [x for x in range(3 * n) if x not in (5, 17)]
    assert np.array_equal(got[keep], expected_sigma(log_n, (2, 3, 4), [perm[x] for x in keep]))
