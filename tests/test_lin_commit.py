"""The verifiers' one statement of the linearisation commitment (csrc/lin_commit.hpp, through the host shim): the sum of its
eleven scalars times their bases equals oracle/pairing.linearisation_commitment.  The identity needs no valid proof, so the
evaluations and challenges are arbitrary residues; the commitments are those of test_verify_fold's circuit and first proof."""
import ctypes
import os
import random

import numpy as np
import pytest

from helpers import O, ROOT, u32p
from oracle import pairing as PR
from oracle import plonk_oracle as PO
from test_verify_fold import LOG_N, _setup

R = O.R


@pytest.fixture(scope="module")
def shim(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpp", "libff_host_shim.so"))
    lib.shim_lin_commit_scalars.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    lib.shim_lin_commit_scalars.restype = None
    return lib


def _scalars(shim, values, n):
    arr = np.array([limb for v in values for limb in O.fr_to_mont_limbs(v % R)], dtype=np.uint64)
    out = np.zeros(4 * 11, dtype=np.uint64)
    shim.shim_lin_commit_scalars(u32p(arr), n, u32p(out))
    return [O.fr_from_mont_limbs([int(x) for x in out[4 * i:4 * i + 4]]) for i in range(11)]


# the Python function takes PI(zeta) with the sign the scalar function is given: the prover's sign reaches it as -PI(zeta)
@pytest.mark.parametrize("case", ["pi_zero", "pi_reference_sign", "pi_prover_sign", "zeta_one"])
def test_scalars_times_bases_equal_the_oracles_commitment(shim, case):
    s = _setup()
    pf = s["proofs"][0]
    n = s["n"]
    rnd = random.Random({"pi_zero": 1, "pi_reference_sign": 2, "pi_prover_sign": 3, "zeta_one": 4}[case])
    a, b, c, zw, s1, s2, alpha, beta, gamma = (rnd.randrange(R) for _ in range(9))
    zeta = 1 if case == "zeta_one" else rnd.randrange(2, R)
    pi = rnd.randrange(1, R)
    pi_signed = {"pi_zero": 0, "pi_reference_sign": pi, "pi_prover_sign": -pi % R, "zeta_one": pi}[case]
    got = _scalars(shim, [a, b, c, zw, s1, s2, alpha, beta, gamma, zeta, pow(zeta, n, R), *PO.COSETS, pi_signed], n)
    # q_l q_r q_o q_m q_c, sigma_3, P0, Z, t_lo t_mid t_hi
    bases = s["fixed"] + [s["sigma_c"][2], s["srs"][0], pf["z_commit"]] + pf["t_commit"]
    assert len(bases) == len(got) == 11
    total = None
    for base, k in zip(bases, got):
        term = O.g1_mul(base, k)
        total = term if total is None else O.g1_add(total, term)
    want = PR.linearisation_commitment(LOG_N, s["fixed"], s["sigma_c"], [s1, s2, 0], PO.COSETS, [a, b, c], pf["z_commit"],
                                       (0, zw), zeta, pf["t_commit"], (alpha, beta, gamma), pi_signed)
    assert s["srs"][0] == O.G1   # the oracle puts the constant on G
    assert total == want
