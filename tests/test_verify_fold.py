"""The batched verifier's algebra on the CPU (tests/verify_ref.py): for oracle-made proofs the folded decision with bisection
equals oracle/pairing.plonk_verify proof by proof, under each tampering, and the fold's weights are a function of the batch
bytes alone.  Pins what typlonk_verify computes independently of the device code (Python pairings: a handful of proofs)."""
import functools

import pytest

import verify_ref as V
from oracle import bls12_381 as O
from oracle import pairing as PR
from oracle import plonk_oracle as PO

R = O.R
SECRET = 0xC0FFEE1234
LOG_N = 3


@functools.lru_cache(maxsize=None)
def _setup():
    n, _, q_evals, perm = PO.squaring_chain(LOG_N)
    srs = O.srs_from_secret_fast(SECRET, n + 3)
    commit = lambda coeffs: O.kzg_commit(srs, coeffs)   # noqa: E731
    _, sig = PO.compile_permutation(perm, n, LOG_N)
    sigma_polys = [O.interpolate(s, LOG_N) for s in sig]
    fixed = [commit(O.interpolate(q_evals[k], LOG_N)) for k in ("q_l", "q_r", "q_o", "q_m", "q_c")]
    sigma_c = [commit(p) for p in sigma_polys]
    g2, g2s = PR.srs_g2(SECRET)
    proofs, chals = [], []
    for k in range(3):
        _, cols, _, _ = PO.squaring_chain(LOG_N, x0=3 + k, blinders=[[(31 * k + 7 * i + j + 5) % R for j in range(3)] for i in range(3)])
        ch = (0xA11A + 977 * k, 0xBE7A + 13 * k, 0x6A77A + 5 * k)   # alpha, beta, gamma
        zeta = 0x2E7A0000 + 1009 * k
        pf = PO.prove(LOG_N, cols, q_evals, perm, [0] * n, ch, zeta, commit)
        assert pf["r_open"][1] == 0
        proofs.append(pf)
        chals.append((ch, zeta))
    return {"n": n, "srs": srs, "fixed": fixed, "sigma_polys": sigma_polys, "sigma_c": sigma_c, "g2": g2, "g2s": g2s,
            "proofs": proofs, "chals": chals}


def _checks(s, pf, ch, zeta):
    sigma_evals = [O.poly_eval(p, zeta) for p in s["sigma_polys"]]
    advice = [op[1] for op in pf["open"]]
    r_c = PR.linearisation_commitment(LOG_N, s["fixed"], s["sigma_c"], sigma_evals, PO.COSETS, advice, pf["z_commit"],
                                      (pf["z_open"][1], pf["zw_open"][1]), zeta, pf["t_commit"], ch, 0)
    return V.kzg_checks(pf, zeta, LOG_N, r_c)


def _batch(s, proofs, stats=None):
    zetas = [z for _, z in s["chals"]]
    data = V.batch_bytes(s["n"], 0, s["g2s"], s["srs"][0], s["fixed"] + s["sigma_c"], proofs, zetas, [0] * len(proofs))
    rho = V.fold_rho(data)
    checks = [_checks(s, pf, ch, z) for pf, (ch, z) in zip(proofs, s["chals"])]
    live = [pf["r_open"][1] == 0 for pf in proofs]      # the host check r(zeta) = 0 keeps a proof out of the fold
    return V.batch_verify(checks, live, rho, s["g2s"], stats)


def _oracle(s, pf, k):
    ch, zeta = s["chals"][k]
    return PR.plonk_verify(LOG_N, pf, s["fixed"], s["sigma_polys"], s["sigma_c"], PO.COSETS, [0] * s["n"], ch, zeta, s["g2"],
                           s["g2s"])


def _tamper(pf, kind):
    g = O.G1
    if kind == "eval_a":
        return dict(pf, open=[(pf["open"][0][0], (pf["open"][0][1] + 1) % R)] + pf["open"][1:])
    if kind == "commit_b":
        return dict(pf, commit=[pf["commit"][0], O.g1_add(pf["commit"][1], g), pf["commit"][2]])
    if kind == "witness_zw":
        return dict(pf, zw_open=(O.g1_add(pf["zw_open"][0], g), pf["zw_open"][1]))
    if kind == "t_hi":
        return dict(pf, t_commit=pf["t_commit"][:2] + [O.g1_add(pf["t_commit"][2], g)])
    if kind == "r_nonzero":
        return dict(pf, r_open=(pf["r_open"][0], 1))
    raise ValueError(kind)


def test_all_valid_batch_is_one_fold_and_matches_the_oracle():
    s = _setup()
    stats = {}
    assert _batch(s, s["proofs"], stats) == [True, True, True]
    assert stats["folds"] == 1
    assert _oracle(s, s["proofs"][0], 0)


@pytest.mark.parametrize("kind", ["eval_a", "commit_b", "witness_zw", "t_hi", "r_nonzero"])
def test_tampered_proof_alone_is_rejected_as_the_oracle_rejects_it(kind):
    s = _setup()
    bad = _tamper(s["proofs"][1], kind)
    assert not _oracle(s, bad, 1)
    stats = {}
    assert _batch(s, [s["proofs"][0], bad, s["proofs"][2]], stats) == [True, False, True]
    # bisection: 1 fold of all, then halves [0] and [1, 2], then [1] and [2] (r_nonzero never enters the fold: 1)
    assert stats["folds"] == (1 if kind == "r_nonzero" else 5)


def test_two_bad_proofs():
    s = _setup()
    batch = [_tamper(s["proofs"][0], "eval_a"), s["proofs"][1], _tamper(s["proofs"][2], "commit_b")]
    assert _batch(s, batch) == [False, True, False]


def test_weights_are_a_function_of_the_batch_bytes():
    import hashlib

    s = _setup()
    zetas = [z for _, z in s["chals"]]
    args = (s["n"], 0, s["g2s"], s["srs"][0], s["fixed"] + s["sigma_c"], s["proofs"], zetas, [0, 0, 0])
    data = V.batch_bytes(*args)
    # 16 + 192 + 9 x 97 bytes of header, 13 x 97 + 8 x 32 per proof
    assert len(data) == 16 + 192 + 9 * 97 + 3 * (13 * 97 + 8 * 32)
    rho = V.fold_rho(data)
    assert rho == V.fold_rho(V.batch_bytes(*args)) == int.from_bytes(hashlib.blake2b(data, digest_size=64).digest(), "little") % R
    assert 0 < rho < R
    # any change of the batch moves rho: an evaluation, a point, the flags, the PI value, the order of the proofs
    assert V.fold_rho(V.batch_bytes(*args[:5], [_tamper(s["proofs"][0], "eval_a")] + s["proofs"][1:], zetas, [0, 0, 0])) != rho
    assert V.fold_rho(V.batch_bytes(*args[:5], [_tamper(s["proofs"][0], "t_hi")] + s["proofs"][1:], zetas, [0, 0, 0])) != rho
    assert V.fold_rho(V.batch_bytes(s["n"], 1, *args[2:])) != rho
    assert V.fold_rho(V.batch_bytes(*args[:7], [0, 5, 0])) != rho
    assert V.fold_rho(V.batch_bytes(*args[:5], s["proofs"][::-1], zetas[::-1], [0, 0, 0])) != rho
