"""Python restatement of the batched verifier's algebra (typlonk_verify, typlonk_amd/csrc/verify.hip), independent of the
device code: the six KZG checks of every proof folded with weights rho^(6k + j + 1) into one pairing product, bisection on
failure, and rho drawn from the batch bytes.  Proofs are the dicts oracle/plonk_oracle.prove returns (affine points as
integers, None = identity), with the challenges and zeta given.

A KZG check e(W, [s]G2 - z G2) = e(C - y G, G2) is e(W, [s]G2) = e(C - y G + z W, G2), so with weights rho_j:
    e(sum rho_j W_j, [s]G2) * e(-sum rho_j (C_j + z_j W_j) + (sum rho_j y_j) G, G2) = 1."""
from __future__ import annotations

import hashlib
import struct

from oracle import bls12_381 as O
from oracle import pairing as PR

R = O.R


def _u64s(vals) -> bytes:
    return b"".join(struct.pack("<Q", int(v)) for v in vals)


def _point(p) -> bytes:
    limbs, inf = O.g1_to_limbs(p)
    return _u64s(limbs) + bytes([inf])


def _fr(x: int) -> bytes:
    return _u64s(O.fr_to_mont_limbs(x % R))


def proof_points(pf):
    """the 13 points in the hashed order: [a] [b] [c] [Z] [t_lo] [t_mid] [t_hi], the witnesses a b c Z Zw r"""
    w = [op[0] for op in pf["open"]] + [pf["z_open"][0], pf["zw_open"][0], pf["r_open"][0]]
    return list(pf["commit"]) + [pf["z_commit"]] + list(pf["t_commit"]) + w


def proof_evals(pf):
    return [op[1] for op in pf["open"]] + [pf["z_open"][1], pf["zw_open"][1], pf["r_open"][1]]


def batch_bytes(n, flags, g2s, srs0, circuit_commitments, proofs, zetas, pi_evals) -> bytes:
    """what typlonk_verify hashes: n, flags (u64 each), [s]G2 as 24 Montgomery limbs (x.c0 x.c1 y.c0 y.c1), SRS point 0,
    the eight circuit commitments, then per proof its 13 points, 6 evaluations, zeta and PI(zeta) (0 for a proof the
    host checks rejected).  A point is 12 limbs + its infinity byte; every limb little-endian."""
    (x0, x1), (y0, y1) = g2s
    out = _u64s([n, flags]) + _u64s([lb for c in (x0, x1, y0, y1) for lb in O.fq_to_mont_limbs(c)]) + _point(srs0)
    out += b"".join(_point(p) for p in circuit_commitments)
    for pf, z, pe in zip(proofs, zetas, pi_evals):
        out += b"".join(_point(p) for p in proof_points(pf))
        out += b"".join(_fr(e) for e in proof_evals(pf)) + _fr(z) + _fr(pe)
    return out


def fold_rho(data: bytes) -> int:
    """Blake2b-512 of the batch bytes read as a little-endian integer, mod r"""
    return int.from_bytes(hashlib.blake2b(data, digest_size=64).digest(), "little") % R


def kzg_checks(pf, zeta, log_n, r_commitment):
    """the six (C, W, z, y) of plonk::proof::verify (proof.rs:247-272 and the r check), in the weight order j = 0..5"""
    w = O.domain_root(log_n)
    ck = [(pf["commit"][i], pf["open"][i][0], zeta, pf["open"][i][1]) for i in range(3)]
    ck.append((pf["z_commit"], pf["z_open"][0], zeta, pf["z_open"][1]))
    ck.append((pf["z_commit"], pf["zw_open"][0], zeta * w % R, pf["zw_open"][1]))
    ck.append((r_commitment, pf["r_open"][0], zeta, pf["r_open"][1]))
    return ck


def folded_check(checks_by_proof, rho, members, g2s) -> bool:
    """one pairing product over the checks of the proofs in `members` (indices into checks_by_proof)"""
    a = None
    b = None
    ysum = 0
    for k in members:
        for j, (c, w, z, y) in enumerate(checks_by_proof[k]):
            rj = pow(rho, 6 * k + j + 1, R)
            a = O.g1_add(a, O.g1_mul(w, rj))
            b = O.g1_add(b, O.g1_mul(O.g1_add(c, O.g1_mul(w, z)), rj))
            ysum = (ysum + rj * y) % R
    b = O.g1_add(O.g1_neg(b), O.g1_mul(O.G1, ysum))
    f = PR.f12_mul(PR.miller_loop(a, g2s), PR.miller_loop(b, PR.G2))
    return PR.f12_conj(PR.f12_pow(f, PR.FINAL_EXP)) == PR.f12_one()


def batch_verify(checks_by_proof, live, rho, g2s, stats=None):
    """verdicts of every proof: the live ones folded, the fold bisected over the live proofs when it fails"""
    ok = [False] * len(checks_by_proof)

    def decide(members):
        if not members:
            return
        if stats is not None:
            stats["folds"] = stats.get("folds", 0) + 1
        if folded_check(checks_by_proof, rho, members, g2s):
            for k in members:
                ok[k] = True
            return
        if len(members) == 1:
            return
        h = len(members) // 2
        decide(members[:h])
        decide(members[h:])

    decide([k for k in range(len(checks_by_proof)) if live[k]])
    return ok


def bisection_folds(live, bad) -> int:
    """how many folds the verifiers' bisection makes (csrc/verify.hip, FoldBisect::decide), replayed without any arithmetic:
    a range with no live proof is skipped; otherwise one fold, which passes iff no bad live proof is in the range; a failed
    fold over more than one live proof splits the range so that its first floor(live / 2) live proofs go left"""
    def decide(lo, hi):
        members = [k for k in range(lo, hi) if live[k]]
        if not members:
            return 0
        if len(members) == 1 or not any(bad[k] for k in members):
            return 1
        mid = members[len(members) // 2]
        return 1 + decide(lo, mid) + decide(mid, hi)

    return decide(0, len(live))
