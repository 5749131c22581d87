"""The union-find of typlonk_permutation_from_pairs without a GPU: the library loads and refuses a null context, and the find, hook
and pointer-jumping bodies of csrc/perm_pairs.hpp as the host compiles them (tests/cpp/perm_pairs_host, a program of its own:
relaxed __atomic builtins, the hooks on 1 thread and on 16) against perm_pairs_ref on the adversarial pair lists of
tests/test_gpu_perm_pairs.py at 2^12 rows: the labels are equal word for word, whatever the interleaving.
The device build of the same bodies: tests/test_gpu_perm_pairs.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import perm_pairs_ref as P
from helpers import ROOT
from perm_pairs_cases import ADVERSARIAL, adversarial

LOG_N = 12
CELLS = 3 << LOG_N


def test_library_loads_without_a_device_and_refuses_a_null_context(built):
    import typlonk_amd
    from typlonk_amd.capi import ERR_INVALID_ARG, SYMBOLS

    lib = typlonk_amd.load_library()
    for s in ("typlonk_permutation_from_pairs", "typlonk_circuit_compile_pairs", "typlonk_circuit_compile_pairs_host"):
        assert s in SYMBOLS
    cid, classes = C.c_uint32(0xA5), C.c_uint64(0xA5)
    assert lib.typlonk_permutation_from_pairs(None, None, 0, 5, None, C.byref(classes)) == ERR_INVALID_ARG
    assert lib.typlonk_circuit_compile_pairs(None, None, None, 0, None, 5, C.byref(cid), C.byref(classes)) == ERR_INVALID_ARG
    assert lib.typlonk_circuit_compile_pairs_host(None, None, 32, None, 0, None, 5, C.byref(cid), C.byref(classes)) == ERR_INVALID_ARG
    assert cid.value == 0xA5 and classes.value == 0xA5


def run_host(log_n, pairs):
    """(exit status, the label arrays of the 1-thread and of the 16-thread run)"""
    text = "\n".join(f"{a} {b}" for a, b in np.asarray(pairs, dtype=np.uint64).reshape(-1, 2).tolist())
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "perm_pairs_host"), str(log_n)], input=text, capture_output=True,
                       text=True, timeout=120)
    return r.returncode, [np.array(line.split(), dtype=np.uint32) for line in r.stdout.splitlines()]


@pytest.mark.parametrize("shape", ADVERSARIAL)
def test_host_union_find_equals_the_reference(built, shape):
    pairs = adversarial(shape, CELLS)
    want = P.labels(CELLS, pairs.tolist())
    rc, got = run_host(LOG_N, pairs)
    assert rc == 0 and len(got) == 2
    for labels in got:     # 1 thread, 16 threads
        assert np.array_equal(labels, want)


def test_host_program_small_and_refusals(built):
    rc, got = run_host(1, [])
    assert rc == 0 and all(g.tolist() == list(range(6)) for g in got)
    rc, got = run_host(1, [(5, 2), (2, 2), (4, 5), (1, 0)])
    assert rc == 0 and all(g.tolist() == [0, 0, 2, 3, 2, 2] for g in got)
    assert run_host(1, [(0, 6)])[0] == 2      # a cell outside the table
