"""Python statement of the compact proof shape (include/typlonk.h, typlonk_prove_compact / typlonk_verify_compact), independent
of the native code: the statement digest and transcript, a prover built from oracle/plonk_oracle.py (quotient_polynomial,
linearisation_poly, batched_opening) and a verifier over oracle/pairing.py -- the two KZG checks of one proof, and the fold of
a batch with its bisection.  Points are affine integer pairs (None = identity), scalars canonical integers.  Small domains
only (schoolbook products, Python pairings)."""
from __future__ import annotations

import hashlib
import struct

from oracle import bls12_381 as O
from oracle import pairing as PR
from oracle import plonk_oracle as PO

R = O.R
TAG = b"typlonk/compact/v1"
FOLD_TAG = b"typlonk/compact/fold/v1"


# ---- encodings -------------------------------------------------------------------------------------------------------
def fr_bytes(x: int) -> bytes:
    return (x % R).to_bytes(32, "little")


def point_bytes(p) -> bytes:
    """serialize_unchecked of a G1 affine point: x, y as 48 little-endian bytes, the infinity flag 0x40 in the last byte"""
    x, y, flag = (0, 1, 0x40) if p is None else (p[0], p[1], 0)
    out = bytearray(x.to_bytes(48, "little") + y.to_bytes(48, "little"))
    out[-1] |= flag
    return bytes(out)


def H(data: bytes) -> int:
    return int.from_bytes(hashlib.blake2b(data, digest_size=64).digest(), "little") % R


def vk_bytes(vk) -> bytes:
    """u32 log_n || k_0 k_1 k_2 || [q_l] [q_r] [q_o] [q_m] [q_c] [sigma_1] [sigma_2] [sigma_3] || P0"""
    return (struct.pack("<I", vk["log_n"]) + b"".join(fr_bytes(k) for k in vk["cosets"]) +
            b"".join(point_bytes(c) for c in vk["commitments"]) + point_bytes(vk["srs0"]))


def statement_digest(vk, pi) -> bytes:
    return hashlib.blake2b(TAG + vk_bytes(vk) + struct.pack("<Q", len(pi)) + b"".join(fr_bytes(x) for x in pi),
                           digest_size=64).digest()


class Transcript:
    def __init__(self, d0: bytes):
        self.t = bytes(d0)

    def points(self, *ps):
        self.t += b"".join(point_bytes(p) for p in ps)

    def scalars(self, *xs):
        self.t += b"".join(fr_bytes(x) for x in xs)

    def squeeze(self, label: bytes) -> int:
        return H(self.t + label)


def challenges(vk, proof, pi):
    """beta, gamma, alpha, zeta, v of a proof dict"""
    tr = Transcript(statement_digest(vk, pi))
    tr.points(*proof["commit"])
    beta, gamma = tr.squeeze(b"b"), tr.squeeze(b"g")
    tr.points(proof["z_commit"])
    alpha = tr.squeeze(b"a")
    tr.points(*proof["t_commit"])
    zeta = tr.squeeze(b"z")
    tr.scalars(*proof["evals"])
    return beta, gamma, alpha, zeta, tr.squeeze(b"v")


# ---- the circuit and its verifying key ---------------------------------------------------------------------------------
def setup(log_n, q_evals, perm, srs, g2s, cosets=None):
    """the circuit polynomials and the verifying key: vk = log_n, cosets (default PO.COSETS), the eight commitments,
    P0 = srs[0], [s]G2"""
    cosets = PO.COSETS if cosets is None else cosets
    n = 1 << log_n
    _, sig = PO.compile_permutation(perm, n, log_n, cosets)
    q = {k: O.interpolate(v, log_n) for k, v in q_evals.items()}
    sigma = [O.interpolate(s, log_n) for s in sig]
    commit = lambda c: O.kzg_commit(srs, c)   # noqa: E731
    comms = [commit(q[k]) for k in ("q_l", "q_r", "q_o", "q_m", "q_c")] + [commit(s) for s in sigma]
    vk = {"log_n": log_n, "cosets": list(cosets), "commitments": comms, "srs0": srs[0], "g2s": g2s}
    return {"q": q, "sigma": sigma, "perm": perm, "srs": srs, "vk": vk, "log_n": log_n}


# ---- the prover -----------------------------------------------------------------------------------------------------------
def prove(circ, cols, pi, forge=False, cosets=None):
    """A compact proof for witness columns `cols` (n evaluations each) and public values `pi` (pi_len <= n values).
    forge=True: a prover holding a witness that satisfies nothing tries the reference shape's forgery -- t = the constant
    N(zeta*) / Z_H(zeta*) for the zeta* it can predict before committing to t -- which the compact transcript defeats.
    cosets: the key's own by default (what setup() was given, PO.COSETS unless it was told otherwise)."""
    cosets = circ["vk"]["cosets"] if cosets is None else cosets
    log_n, srs, q, sigma = circ["log_n"], circ["srs"], circ["q"], circ["sigma"]
    n = 1 << log_n
    w = O.domain_root(log_n)
    commit = lambda c: O.kzg_commit(srs, c)   # noqa: E731
    ids, sig = PO.compile_permutation(circ["perm"], n, log_n, cosets)
    wires = [O.interpolate(c, log_n) for c in cols]
    pi_poly = O.interpolate(list(pi) + [0] * (n - len(pi)), log_n)
    tr = Transcript(statement_digest(circ["vk"], pi))
    cm = [commit(p) for p in wires]
    tr.points(*cm)
    beta, gamma = tr.squeeze(b"b"), tr.squeeze(b"g")
    acc = PO.grand_product(cols, ids, sig, beta, gamma, n)
    z = O.interpolate(acc[:n], log_n)
    zw = O.interpolate(acc[1:n] + acc[:1], log_n)
    z_c = commit(z)
    tr.points(z_c)
    alpha = tr.squeeze(b"a")
    if forge:
        zeta_guess = tr.squeeze(b"z")   # what the reference's transcript would give: t is not hashed there
        t_slices = forged_quotient(log_n, q, sigma, wires, z, pi_poly, (alpha, beta, gamma), zeta_guess, cosets)
    else:
        (t, _), _ = PO.quotient_polynomial(log_n, wires, z, zw, q, sigma, alpha, beta, gamma, pi_poly, cosets)
        t_slices = PO.slices(t, n)
    t_c = [commit(s) for s in t_slices]
    tr.points(*t_c)
    zeta = tr.squeeze(b"z")
    adv = [O.poly_eval(p, zeta) for p in wires]
    evals = adv + [O.poly_eval(z, zeta), O.poly_eval(z, zeta * w % R), O.poly_eval(sigma[0], zeta), O.poly_eval(sigma[1], zeta)]
    tr.scalars(*evals)
    v = tr.squeeze(b"v")
    r = PO.linearisation_poly(log_n, q, sigma, cosets, adv, evals[4], z, (alpha, beta, gamma), zeta, t_slices,
                              O.poly_eval(pi_poly, zeta))
    w_z, _ = PO.batched_opening([wires[0], wires[1], wires[2], z, r, sigma[0], sigma[1]], v, zeta, commit)
    w_zw = commit(O.poly_div_linear(z, zeta * w % R)[0])
    return {"commit": cm, "z_commit": z_c, "t_commit": t_c, "witness": [w_z, w_zw], "evals": evals,
            "challenges": {"beta": beta, "gamma": gamma, "alpha": alpha, "zeta": zeta, "v": v},
            "r_zeta": O.poly_eval(r, zeta)}


def forged_quotient(log_n, q, sigma, wires, z, pi_poly, ch, zeta, cosets=None):
    """the three slices of the constant t = N(zeta) / Z_H(zeta): r(zeta) = N(zeta) - Z_H(zeta) t(zeta) = 0 at this zeta"""
    cosets = PO.COSETS if cosets is None else cosets
    n = 1 << log_n
    w = O.domain_root(log_n)
    adv = [O.poly_eval(p, zeta) for p in wires]
    r0 = PO.linearisation_poly(log_n, q, sigma, cosets, adv, O.poly_eval(z, zeta * w % R), z, ch, zeta, [[], [], []],
                               O.poly_eval(pi_poly, zeta))
    t0 = O.poly_eval(r0, zeta) * pow((pow(zeta, n, R) - 1) % R, -1, R) % R
    return [[t0], [], []]


def forged_reference_proof(log_n, cols, q_evals, perm, srs, ch, zeta):
    """the reference shape's forgery (oracle/plonk_oracle.prove's dict): every opening honest, t = N(zeta) / Z_H(zeta)"""
    n = 1 << log_n
    w = O.domain_root(log_n)
    commit = lambda c: O.kzg_commit(srs, c)   # noqa: E731
    alpha, beta, gamma = ch
    ids, sig = PO.compile_permutation(perm, n, log_n)
    wires = [O.interpolate(c, log_n) for c in cols]
    acc = PO.grand_product(cols, ids, sig, beta, gamma, n)
    z = O.interpolate(acc[:n], log_n)
    q = {k: O.interpolate(v, log_n) for k, v in q_evals.items()}
    sigma = [O.interpolate(s, log_n) for s in sig]
    t_slices = forged_quotient(log_n, q, sigma, wires, z, [], ch, zeta)

    def open_(p, x):
        qq, y = O.poly_div_linear(p, x)
        return commit(qq), y

    openings = [open_(p, zeta) for p in wires]
    zw_open = open_(z, zeta * w % R)
    r = PO.linearisation_poly(log_n, q, sigma, PO.COSETS, [o[1] for o in openings], zw_open[1], z, ch, zeta, t_slices, 0)
    return {"commit": [commit(p) for p in wires], "open": openings, "z_commit": commit(z), "z_open": open_(z, zeta),
            "zw_open": zw_open, "t_commit": [commit(s) for s in t_slices], "r_open": open_(r, zeta)}


# ---- the verifier ---------------------------------------------------------------------------------------------------------
def _in_field(x) -> bool:
    return isinstance(x, int) and 0 <= x < R


def host_checks(vk, proof, pi):
    """None when the proof is rejected before any pairing, else (challenges, PI(zeta))"""
    pts = list(proof["commit"]) + [proof["z_commit"]] + list(proof["t_commit"]) + list(proof["witness"])
    if len(pts) != 9 or not all(O.g1_is_on_curve(p) for p in pts):
        return None
    if len(proof["evals"]) != 7 or not all(_in_field(e) for e in proof["evals"]):
        return None
    ch = challenges(vk, proof, pi)
    n = 1 << vk["log_n"]
    if pow(ch[3], n, R) == 1:
        return None
    pi_eval = O.poly_eval(O.interpolate(list(pi) + [0] * (n - len(pi)), vk["log_n"]), ch[3])
    return ch, pi_eval


def kzg_checks(vk, proof, ch, pi_eval):
    """[(C, W, z, y)] of the two checks: F at zeta and Z at zeta w"""
    beta, gamma, alpha, zeta, v = ch
    log_n = vk["log_n"]
    a, b, c, z_ev, zw_ev, s1, s2 = proof["evals"]
    cm = vk["commitments"]
    # [r] with the prover's sign of PI(zeta) (PR.linearisation_commitment subtracts its public_eval)
    r_c = PR.linearisation_commitment(log_n, cm[:5], cm[5:], [s1, s2], vk["cosets"], [a, b, c], proof["z_commit"],
                                      [z_ev, zw_ev], zeta, proof["t_commit"], (alpha, beta, gamma), (-pi_eval) % R)
    bases = list(proof["commit"]) + [proof["z_commit"], r_c, cm[5], cm[6]]
    f_c = PR.g1_lincomb([(p, pow(v, i, R)) for i, p in enumerate(bases)])
    y_f = (a + v * b + v * v * c + pow(v, 3, R) * z_ev + pow(v, 5, R) * s1 + pow(v, 6, R) * s2) % R
    w = O.domain_root(log_n)
    return [(f_c, proof["witness"][0], zeta, y_f), (proof["z_commit"], proof["witness"][1], zeta * w % R, zw_ev)]


def verify_one(vk, proof, pi) -> bool:
    """the two KZG checks of one proof, each its own pairing equation"""
    hc = host_checks(vk, proof, pi)
    if hc is None:
        return False
    g2 = PR.G2
    return all(PR.kzg_verify(c, (wt, y), z, g2, vk["g2s"]) for c, wt, z, y in kzg_checks(vk, proof, *hc))


def g2s_limbs(g2s):
    (x0, x1), (y0, y1) = g2s
    return [limb for c in (x0, x1, y0, y1) for limb in O.fq_to_mont_limbs(c)]


def fold_rho(vk, proofs, pi_evals) -> int:
    data = FOLD_TAG + vk_bytes(vk) + b"".join(struct.pack("<Q", x) for x in g2s_limbs(vk["g2s"]))
    for pf in proofs:
        data += b"".join(point_bytes(p) for p in list(pf["commit"]) + [pf["z_commit"]] + list(pf["t_commit"]) + list(pf["witness"]))
        data += b"".join(fr_bytes(e) for e in pf["evals"])
    return H(data + b"".join(fr_bytes(e) for e in pi_evals))


def folded_check(checks, rho, members, g2s) -> bool:
    a, b, ysum = None, None, 0
    for k in members:
        for j, (c, w, z, y) in enumerate(checks[k]):
            rj = pow(rho, 2 * k + j + 1, R)
            a = O.g1_add(a, O.g1_mul(w, rj))
            b = O.g1_add(b, O.g1_mul(O.g1_add(c, O.g1_mul(w, z)), rj))
            ysum = (ysum + rj * y) % R
    b = O.g1_add(O.g1_neg(b), O.g1_mul(O.G1, ysum))
    f = PR.f12_mul(PR.miller_loop(a, g2s), PR.miller_loop(b, PR.G2))
    return PR.f12_conj(PR.f12_pow(f, PR.FINAL_EXP)) == PR.f12_one()


def verify_batch(vk, proofs, pis, stats=None):
    """typlonk_verify_compact's decision: host checks, one fold of the live proofs, bisection when it fails"""
    hcs = [host_checks(vk, pf, pi) for pf, pi in zip(proofs, pis)]
    pi_evals = [hc[1] if hc else 0 for hc in hcs]
    rho = fold_rho(vk, proofs, pi_evals)
    checks = [kzg_checks(vk, pf, *hc) if hc else None for pf, hc in zip(proofs, hcs)]
    ok = [False] * len(proofs)

    def decide(members):
        if not members:
            return
        if stats is not None:
            stats["folds"] = stats.get("folds", 0) + 1
        if folded_check(checks, rho, members, vk["g2s"]):
            for k in members:
                ok[k] = True
            return
        if len(members) == 1:
            return
        h = len(members) // 2
        decide(members[:h])
        decide(members[h:])

    decide([k for k in range(len(proofs)) if hcs[k] is not None])
    return ok
