"""The compact proof shape on the CPU (tests/compact_ref.py): honest proofs verify, every single-field tampering is rejected,
the native transcript (typlonk_compact_challenges) equals the Python one, and the forgery the reference shape admits -- a
quotient chosen after zeta -- is caught by the compact transcript, which binds t before zeta is drawn."""
import functools

import numpy as np
import pytest

import compact_ref as CR
import verify_ref as V
from oracle import bls12_381 as O
from oracle import pairing as PR
from oracle import plonk_oracle as PO

R = O.R
SECRET = 0xC0FFEE1234
LOG_N = 3


def chain_columns(log_n, pi=(), x0=3, seed=0):
    """the squaring chain's witness with public inputs: x_{j+1} = x_j^2 + pi_j (the gate a b - c + PI = 0), blinders by seed"""
    n = 1 << log_n
    g = n - 3
    xs = [x0 % R]
    for j in range(g):
        xs.append((xs[-1] * xs[-1] + (pi[j] if j < len(pi) else 0)) % R)
    bl = [[(977 * seed + 7 * i + j + 5) % R for j in range(3)] for i in range(3)]
    return [xs[:g] + bl[0], xs[:g] + bl[1], xs[1:g + 1] + bl[2]]


@functools.lru_cache(maxsize=None)
def circuit(log_n=LOG_N):
    n, _, q_evals, perm = PO.squaring_chain(log_n)
    srs = O.srs_from_secret_fast(SECRET, n + 3)
    _, g2s = PR.srs_g2(SECRET)
    c = CR.setup(log_n, q_evals, perm, srs, g2s)
    c["q_evals"] = q_evals
    return c


@functools.lru_cache(maxsize=None)
def honest(pi=(), seed=0):
    c = circuit()
    pf = CR.prove(c, chain_columns(LOG_N, pi, seed=seed), list(pi))
    assert pf["r_zeta"] == 0
    return pf


def test_honest_proofs_are_accepted_with_and_without_public_inputs():
    c = circuit()
    vk = c["vk"]
    for pi in ((), (5,), (5, 0, 9, 0, 0, 0, 0, 0)):
        pf = honest(pi)
        assert CR.verify_one(vk, pf, list(pi)), pi
    stats = {}
    batch = [honest(), honest((5,)), honest(seed=1)]
    assert CR.verify_batch(vk, batch, [[], [5], []], stats) == [True, True, True]
    assert stats["folds"] == 1
    # the public values are part of the statement: the same proof under other public inputs does not verify
    assert not CR.verify_one(vk, honest((5,)), [])


def _tampered(pf):
    """(name, proof, pi) with exactly one field changed"""
    out = []

    def with_point(key, i):
        d = dict(pf)
        if i is None:
            d[key] = O.g1_add(d[key], O.G1)
        else:
            lst = list(d[key])
            lst[i] = O.g1_add(lst[i], O.G1)
            d[key] = lst
        return d

    for i in range(3):
        out.append((f"commit{i}", with_point("commit", i)))
    out.append(("z_commit", with_point("z_commit", None)))
    for i in range(3):
        out.append((f"t{i}", with_point("t_commit", i)))
    for i in range(2):
        out.append((f"witness{i}", with_point("witness", i)))
    for i in range(7):
        ev = list(pf["evals"])
        ev[i] = (ev[i] + 1) % R
        out.append((f"eval{i}", dict(pf, evals=ev)))
    return out


def test_every_single_field_tampering_is_rejected():
    c = circuit()
    vk = c["vk"]
    pi = [5, 7]
    pf = honest(tuple(pi))
    cases = [(name, d, pi) for name, d in _tampered(pf)]
    cases.append(("pi value", pf, [5, 8]))
    cases.append(("pi_len + 1", pf, pi + [0]))
    assert len(cases) == 18
    for name, d, p in cases:
        assert CR.verify_batch(vk, [d], [p]) == [False], name
    # in a batch: exactly the tampered proof is rejected
    stats = {}
    good = honest(seed=1)
    bad = _tampered(honest(seed=2))[8][1]                   # W_zeta_w
    assert CR.verify_batch(vk, [good, bad, honest()], [[], [], []], stats) == [True, False, True]
    assert stats["folds"] <= 2 * 2 + 1


def test_native_transcript_equals_the_python_statement(built):
    """typlonk_compact_challenges (host-only) on the Python prover's proof: the five challenges it drew"""
    from helpers import fr_pack, fr_unpack, g1_pack
    from typlonk_amd import capi

    c = circuit()
    vk = c["vk"]
    for pi in ((), (5, 7), (5, 0, 9, 0, 0, 0, 0, 0)):
        pf = honest(pi)
        cxy, cinf = g1_pack(vk["commitments"])
        s0 = g1_pack([vk["srs0"]])
        nvk = capi.vk_from(LOG_N, fr_pack(vk["cosets"]), [(cxy[i], cinf[i]) for i in range(8)], (s0[0][0], s0[1][0]),
                           CR.g2s_limbs(vk["g2s"]))
        pts = lambda ps: [(x, f) for x, f in zip(*g1_pack(ps))]   # noqa: E731
        d = {"commit": pts(pf["commit"]), "z_commit": pts([pf["z_commit"]])[0], "t_commit": pts(pf["t_commit"]),
             "witness": pts(pf["witness"]), "evals": list(fr_pack(pf["evals"]))}
        got = capi.compact_challenges(nvk, d, fr_pack(list(pi)) if pi else None)
        exp = CR.challenges(vk, pf, list(pi))
        assert fr_unpack(np.array(got)) == list(exp), pi
        assert [pf["challenges"][k] for k in capi.COMPACT_CHALLENGES] == list(exp)
    with pytest.raises(capi.TyplonkError) as e:
        capi.compact_challenges(nvk, d, np.zeros(((1 << LOG_N) + 1, 4), dtype=np.uint64))
    assert e.value.code == capi.ERR_LENGTH


def test_the_reference_shapes_forgery_passes_there_and_fails_here():
    """A witness that satisfies nothing.  In the reference shape zeta does not depend on t, so t = N(zeta) / Z_H(zeta) makes
    r(zeta) = 0 and every opening honest: the per-proof check accepts.  The compact prover that tries the same (t from the
    zeta it can predict) is rejected, because zeta is drawn after [t]."""
    c = circuit()
    n = 1 << LOG_N
    cols = [[(1000 + 31 * i + 7 * j) % R for j in range(n)] for i in range(3)]
    ch, zeta = (0xA11A, 0xBE7A, 0x6A77A), 0x2E7A0001
    ref = CR.forged_reference_proof(LOG_N, cols, c["q_evals"], c["perm"], c["srs"], ch, zeta)
    assert ref["r_open"][1] == 0
    g2, g2s = PR.srs_g2(SECRET)
    cm = c["vk"]["commitments"]
    sigma_evals = [O.poly_eval(s, zeta) for s in c["sigma"]]
    r_c = PR.linearisation_commitment(LOG_N, cm[:5], cm[5:], sigma_evals, PO.COSETS, [op[1] for op in ref["open"]],
                                      ref["z_commit"], (ref["z_open"][1], ref["zw_open"][1]), zeta, ref["t_commit"], ch, 0)
    assert V.folded_check([V.kzg_checks(ref, zeta, LOG_N, r_c)], 0x5EED, [0], g2s)
    assert PR.plonk_verify(LOG_N, ref, cm[:5], c["sigma"], cm[5:], PO.COSETS, [0] * n, ch, zeta, g2, g2s)
    # the same in the compact shape
    forged = CR.prove(c, cols, [], forge=True)
    assert forged["r_zeta"] != 0
    assert not CR.verify_one(c["vk"], forged, [])
    assert CR.verify_batch(c["vk"], [forged], [[]]) == [False]
    # and an honest compact proof of that witness carries r(zeta) != 0 and does not verify either
    plain = CR.prove(c, cols, [])
    assert plain["r_zeta"] != 0
    assert not CR.verify_one(c["vk"], plain, [])
