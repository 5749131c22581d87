"""References for typlonk_srs_g1_ntt, typlonk_open_all_* and typlonk_open_chunks_* at domains past what a quadratic big-integer
reference and one Python scalar multiplication per record can reach (tests/srs_lagrange_ref.py, open_all_ref.py,
open_chunks_ref.py stop at 2^7).  Two parts.

1. Closed forms ON SCALARS in O(n log n), for the SRS [s^m] G with a known s outside the domain.  n = 2^log_n, l = 2^log_l,
   r = n / l, w = O.domain_root(log_n):

       Lagrange      L_i(s) = w^i (s^n - 1) / (n (s - w^i))
       open_all      q_k(s) = (f(s) - f(w^k)) / (s - w^k)
       open_chunks   q_k(s) = (f(s) - I_k(s)) / (s^l - a_k),   a_k = w^(k l),   I_k(s) = sum_t c_t (s w^-k)^t,
                     c = the size-l inverse transform of the l evaluations f(w^(k + r t)), t < l, on coset k

   (f = q_k (X^l - a_k) + I_k with deg I_k < l, and I_k(w^k mu^t) = sum_u (c'_u w^(k u)) mu^(t u) for mu = w^r, so the inverse
   transform of the coset's evaluations is c_u = c'_u w^(k u).)  Powers are running products, every vector of denominators is
   inverted by one batch inversion, the evaluations f(w^k) come from the C oracle's NTT on limb arrays.  Python integers in and
   out.

2. `combination_check`: a whole vector of device records P_k against reference scalars e_k by ONE MSM of the C oracle.  With
   seeded, full-width, non-zero rho_k drawn independently of the records,

       sum_k [rho_k] P_k  ==  [sum_k rho_k e_k mod r] G

   holds when every P_k = [e_k] G and, for any other records of the group, with probability about 2^-254 over rho.  Equal group
   elements have equal words only in canonical form, so every coordinate must be below p and the identity flag must go with
   the identity's record -- x = 0, y = 1 in this ABI (arkworks' GroupAffine::zero; (0, 1) is not on the curve, so no other
   point has it) -- and with no other.  A sample of 64 records is also compared word for word and flag for flag with
   [e_k] G from the C oracle, so that a failure names an index."""
from __future__ import annotations

import numpy as np

from oracle import bls12_381 as O
from oracle import coracle as CO

R, P = O.R, O.P
_MONT_INV = pow(O.FR_MONT_R, -1, R)
IDENTITY_XY = np.array(O.g1_to_limbs(None)[0], dtype=np.uint64)
SAMPLE = 64


# ---- limbs ------------------------------------------------------------------------------------------------------------------
def pack(vals) -> np.ndarray:
    """canonical ints -> (k, 4) uint64 Montgomery limbs (helpers.fr_pack, through bytes: 2^17 elements in a tenth of a second)"""
    raw = b"".join((v % R * O.FR_MONT_R % R).to_bytes(32, "little") for v in vals)
    return np.frombuffer(raw, dtype="<u8").reshape(-1, 4).astype(np.uint64)


def unpack(arr) -> list[int]:
    raw = np.ascontiguousarray(arr, dtype="<u8").tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") * _MONT_INV % R for i in range(0, len(raw), 32)]


# ---- scalars ----------------------------------------------------------------------------------------------------------------
def powers(x: int, count: int):
    """x^0 .. x^(count-1) by a running product"""
    out, acc = [], 1
    for _ in range(count):
        out.append(acc)
        acc = acc * x % R
    return out


def batch_inverse(xs):
    """1/x for every x, none of them zero, by one inversion"""
    prefix, acc = [], 1
    for x in xs:
        assert x % R, "batch_inverse: a zero"
        prefix.append(acc)
        acc = acc * x % R
    inv = pow(acc, -1, R)
    out = [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        out[i] = prefix[i] * inv % R
        inv = inv * xs[i] % R
    return out


def horner(coeffs, x: int) -> int:
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def padded(f, log_n: int):
    n = 1 << log_n
    assert 1 <= len(f) <= n
    return [x % R for x in f] + [0] * (n - len(f))


# ---- evaluations ------------------------------------------------------------------------------------------------------------
def domain_evaluations(f, log_n: int) -> np.ndarray:
    """f(w^k), k < n, as (n, 4) limbs: the C oracle's transform of the zero-padded coefficients"""
    return CO.ntt(pack(padded(f, log_n)), log_n)


def chunk_major(evals, log_n: int, log_l: int):
    """natural order -> the order typlonk_open_chunks_* writes: out[k l + t] = evals[k + r t].  An (n, 4) limb array or a list."""
    n, l = 1 << log_n, 1 << log_l
    r = n // l
    if isinstance(evals, np.ndarray):
        assert evals.shape == (n, 4)
        return np.ascontiguousarray(evals.reshape(l, r, 4).transpose(1, 0, 2)).reshape(n, 4)
    assert len(evals) == n
    return [evals[k + r * t] for k in range(r) for t in range(l)]


# ---- the closed forms -------------------------------------------------------------------------------------------------------
def lagrange_scalars(s: int, log_n: int):
    """L_i(s), i < n, for s outside the domain"""
    n = 1 << log_n
    s %= R
    zh = (pow(s, n, R) - 1) % R
    assert zh, "s lies in the domain: the closed form is 0/0"
    wi = powers(O.domain_root(log_n), n)
    inv = batch_inverse([n * (s - x) % R for x in wi])
    return [x * zh % R * d % R for x, d in zip(wi, inv)]


def open_all_scalars(f, s: int, log_n: int):
    """q_k(s), k < n, for s outside the domain"""
    n = 1 << log_n
    s %= R
    assert pow(s, n, R) != 1, "s lies in the domain: the closed form is 0/0"
    f = padded(f, log_n)
    ys = unpack(domain_evaluations(f, log_n))
    fs = horner(f, s)
    inv = batch_inverse([(s - x) % R for x in powers(O.domain_root(log_n), n)])
    return [(fs - y) * d % R for y, d in zip(ys, inv)]


def open_chunks_scalars(f, s: int, log_n: int, log_l: int):
    """q_k(s), k < r, for s^l different from every a_k"""
    assert 0 <= log_l < log_n
    n, l = 1 << log_n, 1 << log_l
    r = n // l
    s %= R
    w = O.domain_root(log_n)
    assert O.domain_root(log_l) == pow(w, r, R)                      # the size-l transform runs over mu = w^r
    f = padded(f, log_n)
    ys = chunk_major(domain_evaluations(f, log_n), log_n, log_l)
    if l > 1:
        ys = np.concatenate([CO.ntt(ys[k * l:(k + 1) * l], log_l, inverse=True) for k in range(r)])
    c = unpack(ys)
    fs, sl = horner(f, s), pow(s, l, R)
    a = powers(pow(w, l, R), r)
    assert all(sl != x for x in a), "s^l is a coset constant: the closed form is 0/0"
    inv = batch_inverse([(sl - x) % R for x in a])
    w_inv_k = powers(pow(w, -1, R), r)
    return [(fs - horner(c[k * l:(k + 1) * l], s * w_inv_k[k] % R)) * inv[k] % R for k in range(r)]


# ---- the checker ------------------------------------------------------------------------------------------------------------
def sample_indices(n: int, seed: int):
    """0, 1, 2, the last three, every power of two with its two neighbours, and seeded random indices to fill up to 64"""
    want = {0, 1, 2, n - 3, n - 2, n - 1}
    p = 1
    while p < n:
        want |= {p - 1, p, p + 1}
        p *= 2
    want = {i for i in want if 0 <= i < n}
    rng = np.random.default_rng([seed, 0x5A3B1E])
    while len(want) < min(SAMPLE, n):
        want.add(int(rng.integers(n)))
    return sorted(want)


def non_canonical(xy, inf):
    """the indices of the records that are not in canonical form: a coordinate of p or more, a flag other than 0 or 1, the
    identity flag on another record than the identity's, or the identity's record without the flag"""
    raw = np.ascontiguousarray(xy, dtype="<u8").tobytes()
    big = {i // 96 for i in range(0, len(raw), 48) if int.from_bytes(raw[i:i + 48], "little") >= P}
    is_identity = (xy == IDENTITY_XY).all(axis=1)
    flags = {int(i) for i in np.nonzero((inf > 1) | ((inf == 1) != is_identity))[0]}
    return sorted(big | flags)


def _window(n: int) -> int:
    """the bucket MSM's window for n terms: about log2(n) - 2 bits, within what the C oracle takes"""
    return max(2, min(13, n.bit_length() - 3))


def combination_check(xy, inf, scalars, seed: int):
    """records (k, 12) with flags (k,) are [scalars[i]] G for every i, or an AssertionError that names what differs: the first
    non-canonical record, else the first sampled index whose words differ, else only that the combination does"""
    xy = np.ascontiguousarray(xy, dtype=np.uint64).reshape(-1, 12)
    inf = np.ascontiguousarray(inf, dtype=np.uint8).reshape(-1)
    n = len(scalars)
    assert xy.shape[0] == n and inf.shape[0] == n and n >= 1, (xy.shape, inf.shape, n)
    bad = non_canonical(xy, inf)
    assert not bad, f"{len(bad)} records are not in canonical form, the first at index {bad[0]}"
    differing = []
    for i in sample_indices(n, seed):
        wxy, winf = CO.g1_mul_generator(pack([scalars[i]])[0])
        if not (xy[i] == wxy).all() or int(inf[i]) != winf:
            differing.append(i)
    assert not differing, f"record {differing[0]} is not [e_{differing[0]}] G ({len(differing)} of the sampled records differ)"
    rng = np.random.default_rng([seed, 0xC0B1])
    rho = [int.from_bytes(rng.bytes(32), "little") % (R - 1) + 1 for _ in range(n)]
    got_xy, got_inf, _, _ = CO.msm_pippenger(pack(rho), xy, inf, c=_window(n))
    want_xy, want_inf = CO.g1_mul_generator(pack([sum(a * b for a, b in zip(rho, scalars)) % R])[0])
    assert (got_xy == want_xy).all() and got_inf == want_inf, \
        "sum [rho_k] P_k != [sum rho_k e_k] G: a record outside the sample is wrong (every sampled one is right)"
