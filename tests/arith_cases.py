"""Case lists of tests/test_gpu_arith.py: operands of every device arithmetic primitive in its raw internal form, the
precondition each function's comment states, and the check of a result -- residue, limb form and the documented value
bound -- against Python integers (modular arithmetic and oracle/bls12_381.py's group law, never the limb algorithm).

Operand forms (what the harness tests/cpp/device_arith.hip takes):
  Fr     one int < 2^256, the 8 x 32-bit words of arkworks' Montgomery form (x * 2^256 mod r, read as a plain integer)
  Fq30   one int < 2^390, 13 normalised 30-bit limbs (x * 2^390 mod p, possibly lifted by multiples of p)
  Fr30   a list of 9 limbs, each < 2^32 (lazy forms carry limbs above 2^30)
  G1     tuples of Fq30 ints: XYZZ (X, Y, ZZ, ZZZ), Jacobian (X, Y, Z), affine (x, y)
  wave   64 XYZZ tuples, one per lane of a wavefront (the cross-lane additions of msm_common.hpp)

Every list is deterministic (fixed seeds) and starts with whole 64-lane waves of one kind (all zero, all easy) before the
mixed ones, so that the wave-uniform early exit of the divsteps inversions and the exceptional branches of the group law
run both uniformly and divergently."""
from __future__ import annotations

import math
import random

from oracle import bls12_381 as O

P, R = O.P, O.R
WAVE = 64
M30 = (1 << 30) - 1
FQ_R = 1 << 390          # Fq30's Montgomery radix
FR30_R = 1 << 270        # Fr30's Montgomery radix (fr30_mul)
FR_R = 1 << 256          # Fr's (arkworks) Montgomery radix
N8 = 0x73EDA75           # limb 8 of 2^12 r (fr30_bias)
LAZY = (1 << 30) + 3     # the largest limb 0..7 of a lazy Fr30 value
N_RAND = 2048            # random cases per field primitive
N_RAND_G1 = 384          # random cases per group-law primitive


def limbs(x: int, n: int, bits: int = 30) -> list[int]:
    assert 0 <= x < 1 << (bits * n), "value does not fit the limbs"
    return [(x >> (bits * i)) & ((1 << bits) - 1) for i in range(n)]


def val(ls, bits: int = 30) -> int:
    return sum(int(v) << (bits * i) for i, v in enumerate(ls))


def _rand(seed: int, limit: int, n: int = N_RAND) -> list[int]:
    """n values in [0, limit) from ONE generator seeded once"""
    rnd = random.Random(seed)
    return [rnd.randrange(limit) for _ in range(n)]


def distinct(cases: list) -> int:
    return len(set(map(repr, cases)))


def min_distinct(name: str) -> int:
    """the fewest DISTINCT cases an op's list may hold (repeats, such as the uniform waves, do not count)"""
    return 1 if name == "fr30_const_one" else 250 if name.startswith("g1_") else 2000


def fill_wave(cases: list, filler) -> list:
    """pad to a whole number of waves with `filler` cases, so that the next block starts on a fresh wave"""
    return cases + [filler] * (-len(cases) % WAVE)


def _edges(m: int, word_bits: int, words: int) -> list[int]:
    e = {0, 1, 2, m - 1, m - 2, (m - 1) // 2, (m + 1) // 2, M30, 1 << 30, (1 << 32) - 1, 1 << 32}
    for k in range(1, words):
        e |= {1 << (word_bits * k), (1 << (word_bits * k)) - 1, 1 << (30 * k), (1 << (30 * k)) - 1}
    top = m.bit_length()
    e |= {(1 << (top - 1)) - 1, 1 << (top - 1)}
    return sorted(x for x in e if 0 <= x < m)


# ---- Fr (ff.hpp, arkworks words) ---------------------------------------------------------------------------------------
# all-ones words below r: r - 1 = [1 word of 0, then r's words], and values with the low words all ones under r's top word
FR_EDGE = sorted(set(_edges(R, 32, 8) + [R - (1 << 32), ((R >> 224) - 1 << 224) | ((1 << 224) - 1), (1 << 254) - 1,
                                           ((R >> 32) << 32) - 1, FR_R % R, (FR_R * FR_R) % R]))


def _fr_pairs(seed: int) -> list[tuple[int, int]]:
    rnd = random.Random(seed)
    cases = [(a, b) for a in FR_EDGE for b in FR_EDGE]
    return cases + [(rnd.randrange(R), rnd.randrange(R)) for _ in range(N_RAND)]


def _fr_inv_cases(seed: int) -> list[tuple[int]]:
    rnd = random.Random(seed)
    cases = [(0,)] * WAVE + [(FR_R % R,)] * WAVE          # a wave of zeros, a wave of Montgomery ones
    cases += fill_wave([(x,) for x in FR_EDGE], (0,))
    return cases + [(rnd.randrange(R),) for _ in range(N_RAND)]


FR_OPS = {
    # name: (op code, case builder, precondition, the canonical result).  Every output is canonical (< r).
    "fe_add": (0, lambda: _fr_pairs(11), lambda a, b: a < R and b < R, lambda a, b: (a + b) % R),
    "fe_sub": (1, lambda: _fr_pairs(12), lambda a, b: a < R and b < R, lambda a, b: (a - b) % R),
    "fe_neg": (2, lambda: [(a,) for a, _ in _fr_pairs(13)], lambda a: a < R, lambda a: (-a) % R),
    "fe_mul": (3, lambda: _fr_pairs(14), lambda a, b: a < R and b < R, lambda a, b: a * b * pow(FR_R, -1, R) % R),
    "fe_sqr": (4, lambda: [(a,) for a, _ in _fr_pairs(15)], lambda a: a < R, lambda a: a * a * pow(FR_R, -1, R) % R),
    # x < 2r; the harness hands it straight to the carry chain
    "fe_reduce_once": (5, lambda: [(x,) for x in FR_EDGE + [R, R + 1, 2 * R - 1, 2 * R - 2, R + (1 << 32)]]
                       + [(x,) for x in _rand(16, 2 * R)], lambda a: a < 2 * R, lambda a: a % R),
    # scalars of an MSM (msm_digits_kernel, msm_canon) come straight from the caller: any 256-bit word pattern
    "fe_from_mont": (6, lambda: [(x,) for x in FR_EDGE + [R, 2 * R, FR_R - 1, FR_R - 2, FR_R - R]]
                     + [(x,) for x in _rand(17, FR_R)], lambda a: a < FR_R,
                     lambda a: a * pow(FR_R, -1, R) % R),
    "fr_inv_divsteps": (7, lambda: _fr_inv_cases(18), lambda a: a < R,
                        lambda a: 0 if a == 0 else pow(a, -1, R) * FR_R * FR_R % R),
}


# ---- Fq30 (fq30.hpp) ---------------------------------------------------------------------------------------------------
FQ_EDGE = sorted(set(_edges(P, 30, 13) + [FQ_R % P, (FQ_R * FQ_R) % P, (1 << 380) - 1]))
ALL_ONES_390 = FQ_R - 1


def _lifts(x: int, limit: int) -> list[int]:
    """x + k p below `limit` for k = 0..7 and the largest such k"""
    if x >= limit:
        return []
    kmax = (limit - 1 - x) // P
    return [x + k * P for k in sorted(set(range(min(kmax, 7) + 1)) | {kmax})]


def _below(rnd, limit: int) -> int:
    return rnd.randrange(limit)


def _fq_mul_cases(seed: int, sqr: bool) -> list[tuple]:
    rnd = random.Random(seed)
    ops = [x for e in FQ_EDGE[::3] for x in _lifts(e, 8 * P)[::3]] + [8 * P - 1, ALL_ONES_390, ALL_ONES_390 - 1, (1 << 389) - 1]
    # limbs of all ones in every other / every third limb: the fused columns 10..14 near their maxima
    ops += [val([M30 if i % 2 == 0 else 0 for i in range(13)]), val([M30 if i % 3 else 0 for i in range(13)])]
    if sqr:
        cases = [(a,) for a in ops]
        cases += [(_below(rnd, 8 * P),) for _ in range(N_RAND)]
        cases += [(FQ_R - 1 - rnd.randrange(1 << 300),) for _ in range(256)]      # near all ones
        return cases
    cases = [(a, b) for a in ops for b in ops[::2]]
    cases += [(_below(rnd, 8 * P), _below(rnd, 8 * P)) for _ in range(N_RAND)]
    cases += [(FQ_R - 1 - rnd.randrange(1 << 300), FQ_R - 1 - rnd.randrange(1 << 300)) for _ in range(256)]
    return cases


def _fq_mul2_cases(seed: int) -> list[tuple]:
    rnd = random.Random(seed)
    h = math.isqrt((FQ_R * FQ_R - 1) // 2)                 # 2 h^2 < 2^780: both products at the top
    cases = [(ALL_ONES_390, ALL_ONES_390, 0, 0), (0, 0, ALL_ONES_390, ALL_ONES_390), (h, h, h, h), (h, h - 1, h, h + 1),
             (8 * P - 1, 8 * P - 1, 8 * P - 1, 8 * P - 1), (0, 0, 0, 0), (1, 1, 1, 1), (P, P, P, P)]
    # the group law's form: r*t + (4p - y)*w, y <= 4p
    for _ in range(N_RAND):
        y = rnd.randrange(4 * P + 1)
        cases.append((rnd.randrange(8 * P), rnd.randrange(8 * P), 4 * P - y, rnd.randrange(8 * P)))
    return cases


def _fq_pairs(seed: int, amax: int, bmax: int, extra=()) -> list[tuple]:
    rnd = random.Random(seed)
    cases = list(extra)
    ea = [x for x in FQ_EDGE if x < amax] + [amax - 1]
    eb = [x for x in FQ_EDGE if x < bmax] + [bmax - 1]
    cases += [(a, b) for a in ea[::2] for b in eb[::2]]
    return cases + [(rnd.randrange(amax), rnd.randrange(bmax)) for _ in range(N_RAND)]


def _fq_singles(seed: int, amax: int, extra=()) -> list[tuple]:
    rnd = random.Random(seed)
    ea = sorted({x for e in FQ_EDGE for x in _lifts(e, amax)} | {amax - 1} | set(extra))
    return [(a,) for a in ea] + [(rnd.randrange(amax),) for _ in range(N_RAND)]


def _fq_sub_cases(seed: int, k: int) -> list[tuple]:
    rnd = random.Random(seed)
    amax = FQ_R - k * P                                     # a + K p < 2^390
    cases = [(0, k * P), (amax - 1, 0), (amax - 1, k * P), (0, 0), (P, k * P), (amax - 1, k * P - 1)]
    cases += _fq_pairs(seed, 8 * P, k * P + 1)
    cases += [(rnd.randrange(amax), rnd.randrange(k * P + 1)) for _ in range(N_RAND // 2)]
    return cases


def _fq_sub2_cases(seed: int) -> list[tuple]:
    rnd = random.Random(seed)
    amax = FQ_R - 4 * P
    cases = [(0, 4 * P, 0), (0, 0, 4 * P), (0, 2 * P, 2 * P), (amax - 1, 0, 0), (amax - 1, 4 * P - 1, 1), (0, 0, 0)]
    for _ in range(N_RAND):
        b = rnd.randrange(4 * P + 1)
        cases.append((rnd.randrange(amax if rnd.random() < 0.3 else 8 * P), b, rnd.randrange(4 * P + 1 - b)))
    return cases


def _fq_inv_cases(seed: int, amax: int) -> list[tuple]:
    rnd = random.Random(seed)
    cases = [(0,)] * WAVE + [(FQ_R % P,)] * WAVE + [(1,)] * WAVE         # zero wave, two waves of easy inversions
    cases += [(P * (i % (amax // P)),) for i in range(WAVE)]               # zero mod p, lifted
    cases += fill_wave([x for e in FQ_EDGE for x in [(y,) for y in _lifts(e, amax)]], (0,))
    cases += [((0,) if i % 7 == 0 else (rnd.randrange(amax),)) for i in range(5 * N_RAND // 4)]   # zeros mixed in
    return cases


def _is_zero_mod_cases() -> list[tuple]:
    pl = limbs(P, 13)
    cases = [(0,), (P,), (P - 1,), (P + 1,), (1,), (2 * P - 1,), (FQ_R % P,)]
    for i in range(13):                                     # p with one limb off by one: the limb-wise compare
        for d in (-1, 1):
            v = pl[i] + d
            if 0 <= v <= M30:
                cases.append((val(pl[:i] + [v] + pl[i + 1:]),))
        cases.append((1 << (30 * i),))
    rnd = random.Random(31)
    return cases + [((P if rnd.random() < 0.25 else 0) + (0 if rnd.random() < 0.25 else rnd.randrange(P)),) for _ in range(3 * N_RAND // 2)]


def _inv_fq(a: int) -> int:
    return 0 if a % P == 0 else pow(a, -1, P) * FQ_R * FQ_R % P


FQ_OPS = {
    # name: (op code, case builder, precondition); fq_check holds the expected values and bounds
    "fq30_mul": (0, lambda: _fq_mul_cases(41, False), lambda a, b: a * b < FQ_R * FQ_R),
    "fq30_sqr": (1, lambda: _fq_mul_cases(42, True), lambda a: a * a < FQ_R * FQ_R),
    "fq30_mul2_add": (2, lambda: _fq_mul2_cases(43), lambda a, b, c, d: a * b + c * d < FQ_R * FQ_R),
    "fq30_add_lazy": (3, lambda: _fq_pairs(44, 1 << 389, 1 << 389, [(FQ_R - 1, 0), (0, FQ_R - 1), (1 << 389, (1 << 389) - 1)]),
                      lambda a, b: a + b < FQ_R),
    "fq30_mulk_lazy<2>": (4, lambda: _fq_singles(45, 8 * P, [(FQ_R - 1) // 2]), lambda a: 2 * a < FQ_R),
    "fq30_mulk_lazy<3>": (5, lambda: _fq_singles(46, 8 * P, [(FQ_R - 1) // 3]), lambda a: 3 * a < FQ_R),
    **{f"fq30_sub_lazy<{k}>": (4 + k, (lambda k=k: _fq_sub_cases(46 + k, k)), (lambda a, b, k=k: b <= k * P and a + k * P < FQ_R))
       for k in (2, 3, 4, 5, 6)},
    "fq30_sub2_lazy<4>": (11, lambda: _fq_sub2_cases(53), lambda a, b, c: b + c <= 4 * P and a + 4 * P < FQ_R),
    "fq30_neg_lazy<1>": (12, lambda: _fq_singles(54, P + 1), lambda a: a <= P),
    "fq30_neg_lazy<4>": (13, lambda: _fq_singles(55, 4 * P + 1), lambda a: a <= 4 * P),
    **{f"fq30_cond_sub<{k}>": (c, (lambda k=k: _fq_singles(55 + k, FQ_R, [k * P - 1, k * P, k * P + 1, FQ_R - 1])),
                               lambda a: a < FQ_R) for c, k in ((14, 1), (15, 2), (16, 4))},
    "fq30_canon": (17, lambda: _fq_singles(60, 8 * P), lambda a: a < 8 * P),
    "fq30_is_zero_mod": (18, _is_zero_mod_cases, lambda a: a < 2 * P),
    "fq30_is_zero_exact": (19, lambda: [(1 << (30 * i),) for i in range(13)] + _fq_singles(61, FQ_R), lambda a: a < FQ_R),
    "fq30_pack": (20, lambda: _fq_singles(62, 1 << 384, [8 * P - 1]), lambda a: a < 1 << 384),
    "fq30_unpack": (21, lambda: _fq_singles(63, 1 << 384), lambda a: a < 1 << 384),
    "fq30_from_ark": (22, lambda: _fq_singles(64, P), lambda a: a < P),
    "fq30_to_ark": (23, lambda: _fq_singles(65, 8 * P), lambda a: a < 8 * P),
    "fq30_inv": (24, lambda: _fq_inv_cases(66, 8 * P), lambda a: a < 8 * P),
    "fq30_inv_divsteps": (25, lambda: _fq_inv_cases(67, 8 * P), lambda a: a < 8 * P),
    "fq30_inv_fermat": (26, lambda: _fq_inv_cases(68, 2 * P), lambda a: a < 2 * P),
}
FQ_WORDS_IN = {"fq30_unpack", "fq30_from_ark"}     # operand passed as 12 x 32-bit words
FQ_WORDS_OUT = {"fq30_pack", "fq30_to_ark"}        # result read as 12 x 32-bit words


FQ_MUL_MAX = (FQ_R - P) * FQ_R     # the largest product (or sum of two) whose reduction p + T / 2^390 fits 390 bits
_PINV = pow(P, -1, FQ_R)


def redc(t: int) -> int:
    """Montgomery's reduction by 2^390 as a plain integer: (T + m p) / 2^390 with m = -T p^-1 mod 2^390"""
    return (t + (-t * _PINV) % FQ_R * P) >> 390


def fq_check(name: str, args: tuple, out: int, aux: int) -> None:
    """out: the result as an integer (limbs already checked < 2^30 where promised); aux: predicate / round count"""
    if name in ("fq30_mul", "fq30_sqr", "fq30_mul2_add"):
        t = args[0] * args[1] if name == "fq30_mul" else args[0] ** 2 if name == "fq30_sqr" else args[0] * args[1] + args[2] * args[3]
        # every column fits for T < 2^780, so the result is REDC(T) = (T + m p) / 2^390 exactly, m = -T p^-1 mod 2^390 --
        # kept to 390 bits: above FQ_MUL_MAX the value p + T / 2^390 no longer fits 13 limbs and its top bit is lost.
        # Those cases (outside the contract, fq30.hpp) check only that the columns survive, not that the result is usable.
        assert out == redc(t) % FQ_R, "REDC(T) = (T + m p) / 2^390"
        if t < FQ_MUL_MAX:
            assert out % P == t * pow(FQ_R, -1, P) % P, "residue"
            assert out * FQ_R < P * FQ_R + t, "value bound p + T / 2^390"
    elif name == "fq30_add_lazy":
        assert out == args[0] + args[1]
    elif name.startswith("fq30_mulk_lazy"):
        assert out == int(name[-2]) * args[0]
    elif name.startswith("fq30_sub_lazy"):
        assert out == args[0] - args[1] + int(name[-2]) * P
    elif name == "fq30_sub2_lazy<4>":
        assert out == args[0] - args[1] - args[2] + 4 * P
    elif name.startswith("fq30_neg_lazy"):
        assert out == int(name[-2]) * P - args[0]
    elif name.startswith("fq30_cond_sub"):
        kp = int(name[-2]) * P
        assert out == (args[0] - kp if args[0] >= kp else args[0])
    elif name == "fq30_canon":
        assert out == args[0] % P
    elif name == "fq30_is_zero_mod":
        assert aux == (1 if args[0] % P == 0 else 0)
    elif name == "fq30_is_zero_exact":
        assert aux == (1 if args[0] == 0 else 0)
    elif name in ("fq30_pack", "fq30_unpack"):
        assert out == args[0]
    elif name == "fq30_from_ark":
        assert out == args[0] * (1 << 6) % P, "x 2^384 -> x 2^390, canonical"
    elif name == "fq30_to_ark":
        assert out == args[0] * pow(1 << 6, -1, P) % P, "x 2^390 -> x 2^384, canonical"
    elif name.startswith("fq30_inv"):
        assert out % P == _inv_fq(args[0]), "residue (a R)^-1 R^2"
        assert out * 100 < 101 * P, "value bound 1.01 p"
        if name == "fq30_inv_divsteps":
            assert 0 <= aux <= 37, "round count above FQ30_DIVSTEP_ROUNDS"
    else:
        raise KeyError(name)


# ---- Fr30 (fr30.hpp) ---------------------------------------------------------------------------------------------------
def fr30_exact(x: int) -> list[int]:
    return limbs(x, 9)


def fr30_lazy_max() -> list[int]:
    return [LAZY] * 8 + [(1 << 29) - 1]


def _fr30_lazy(rnd, top: int = (1 << 29) - 1) -> list[int]:
    """a lazy value: limbs 0..7 <= 2^30 + 3 mixing the extremes and random limbs, limb 8 <= top"""
    return [rnd.choice((0, LAZY, LAZY - 1, M30, rnd.randrange(LAZY + 1))) for _ in range(8)] + [rnd.randrange(top + 1)]


def _fr30_mul_cases() -> list[tuple]:
    rnd = random.Random(71)
    tw = [0, 1, R - 1, R, R + 1, 2 * R - 1, FR30_R % R, (FR30_R * FR30_R) % R, M30, 1 << 240]
    lazy = [fr30_lazy_max(), [LAZY] * 8 + [0], [0] * 8 + [(1 << 29) - 1], [M30] * 8 + [(1 << 29) - 1]]
    cases = [(a, fr30_exact(b)) for a in lazy for b in tw] + [(fr30_lazy_max(), fr30_lazy_max())]
    cases += [(fr30_exact(a), fr30_exact(b)) for a in tw for b in tw]
    for i in range(N_RAND):
        a = _fr30_lazy(rnd) if i % 2 else fr30_exact(rnd.randrange(2 * R))
        b = _fr30_lazy(rnd) if i % 8 == 1 else fr30_exact(rnd.randrange(2 * R))
        cases.append((a, b))
    return cases


def _fr30_reduce_cases() -> list[tuple]:
    """top limbs at the 0x73ee boundaries: the quotient estimate floor(x_8 / 0x73ee) is exact or one short"""
    rnd = random.Random(72)
    lows = ([0] * 8, [LAZY] * 8, [M30] * 8)
    tops = {(1 << 29) - 1, 0, 1}
    for k in list(range(1, 9)) + [(1 << 29) // 0x73EE - j for j in range(4)] + [rnd.randrange(1, (1 << 29) // 0x73EE) for _ in range(16)]:
        tops |= {k * 0x73EE - 1, k * 0x73EE, k * 0x73EE + 1, k * 0x73ED, k * 0x73ED - 1}
    cases = [(lo + [t],) for t in sorted(x for x in tops if 0 <= x < 1 << 29) for lo in lows]
    # values just below / at multiples of r, lifted into the lazy range
    for k in (1, 2, 3, 1000, (1 << 269) // R - 1):
        for d in (-1, 0, 1):
            cases.append((fr30_exact(k * R + d),))
    return cases + [(_fr30_lazy(rnd),) for _ in range(N_RAND)]


def _fr30_sub_cases() -> list[tuple]:
    rnd = random.Random(73)
    zero = [0] * 9
    cases = [
        (zero, [LAZY] * 8 + [N8 - 2]),                      # x = 0, the largest subtrahend the limb contract admits
        (zero, fr30_exact((N8 - 2) << 240)),
        (zero, fr30_exact(((N8 - 1) << 240) - 1)),          # the largest exact-limbed subtrahend for x = 0
        (fr30_exact(2 << 240), fr30_exact((1 << 12) * R - 1)),   # y = 2^12 r - 1 with x_8 = 2
        (fr30_lazy_max(), [LAZY] * 8 + [N8 - 2]),
        (fr30_lazy_max(), zero), (zero, zero), (fr30_lazy_max(), fr30_lazy_max()),
    ]
    for i in range(N_RAND):
        a = _fr30_lazy(rnd) if i % 2 else fr30_exact(rnd.randrange(2 * R))
        b = _fr30_lazy(rnd, N8 - 2) if i % 3 else fr30_exact(rnd.randrange(((N8 - 1) << 240)))
        cases.append((a, b))
    return cases


def _fr30_add_cases() -> list[tuple]:
    rnd = random.Random(74)
    cases = [(fr30_lazy_max(), fr30_lazy_max()), ([0] * 9, [0] * 9), ([M30] * 9, [M30] * 9)]
    return cases + [(_fr30_lazy(rnd, 1 << 28), _fr30_lazy(rnd, 1 << 28)) for _ in range(N_RAND)]


def _fr30_norm_cases() -> list[tuple]:
    rnd = random.Random(75)
    cases = [([(1 << 32) - 1] * 8 + [(1 << 32) - 4],), ([0] * 9,), ([1 << 30] * 9,), ([M30] * 9,)]
    return cases + [([rnd.randrange(1 << 32) for _ in range(8)] + [rnd.randrange((1 << 32) - 3)],) for _ in range(N_RAND)]


def _fr30_sub_qr_cases() -> list[tuple]:
    rnd = random.Random(76)
    cases = []
    for q in (0, 1, 2, 18089, (1 << 15) - 1):
        for x in (q * R, q * R + 1, q * R + R - 1, q * R + 2 * R - 1):
            if x < 1 << 270:
                cases.append((fr30_exact(x), [q] + [0] * 8))
    cases.append(([LAZY] * 8 + [0x73EE * 18089 + 0x73ED], [18089] + [0] * 8))
    for _ in range(N_RAND):
        q = rnd.randrange(1 << 15)
        cases.append((fr30_exact(q * R + rnd.randrange(3 * R)), [q] + [0] * 8))
    return cases


def _fr30_ok_lazy(a) -> bool:
    return all(0 <= x <= LAZY for x in a[:8]) and 0 <= a[8] < 1 << 29


FR30_OPS = {
    "fr30_mul": (0, _fr30_mul_cases,
                 lambda a, b: _fr30_ok_lazy(a) and _fr30_ok_lazy(b) and R + val(a) * val(b) // FR30_R < FR30_R),
    "fr30_unpack": (1, lambda: [([w] * 8,) for w in (0, 0xFFFFFFFF, 0x55555555)] + [(limbs(x, 8, 32),) for x in FR_EDGE]
                    + [(limbs(x, 8, 32),) for x in _rand(77, FR_R)], lambda a: len(a) == 8),
    "fr30_pack": (2, lambda: [(fr30_exact(x),) for x in FR_EDGE + [FR_R - 1, 2 * R - 1]]
                  + [(fr30_exact(x),) for x in _rand(78, FR_R)],
                  lambda a: all(x <= M30 for x in a) and val(a) < FR_R),
    "fr30_norm": (3, _fr30_norm_cases, lambda a: all(x < 1 << 32 for x in a) and a[8] + 3 < 1 << 32),
    "fr30_add": (4, _fr30_add_cases, lambda a, b: all(x + y < 1 << 32 for x, y in zip(a, b)) and a[8] + b[8] + 3 < 1 << 32),
    # limbs 0..7 of both <= 2^30 + 3 (fr30_bias: no limb goes negative or wraps), and y_8 <= x_8 + N8 - 2 (limb 8 of the
    # spread bias is N8 - 2: it lends 2^31 downwards) -- which every y < (N8 - 1) 2^240 < 2^12 r meets
    "fr30_sub": (5, _fr30_sub_cases,
                 lambda a, b: all(x <= LAZY and y <= LAZY for x, y in zip(a[:8], b[:8])) and b[8] <= a[8] + N8 - 2 and a[8] < 1 << 29),
    "fr30_to_canonical": (6, lambda: [(fr30_exact(x),) for x in FR_EDGE + [R, R + 1, 2 * R - 1]]
                          + [(fr30_exact(x),) for x in _rand(79, 2 * R)],
                          lambda a: all(x <= M30 for x in a) and val(a) < 2 * R),
    "fr30_sub_qr": (7, _fr30_sub_qr_cases, lambda a, q: q[0] < 1 << 15 and 0 <= val(a) - q[0] * R < 1 << 270),
    "fr30_reduce_lazy": (8, _fr30_reduce_cases, _fr30_ok_lazy),
    "fr30_const_one": (9, lambda: [([0] * 9,)] * WAVE, lambda a: True),
}
FR30_WORDS_OUT = {"fr30_pack", "fr30_to_canonical"}


def fr30_check(name: str, args: tuple, out: list[int]) -> None:
    """out: 9 limbs (8 words for FR30_WORDS_OUT)"""
    if name in FR30_WORDS_OUT:
        v = val(out[:8], 32)
        assert v == (val(args[0]) if name == "fr30_pack" else val(args[0]) % R)
        return
    v = val(out)
    if name == "fr30_norm" or name == "fr30_add" or name == "fr30_sub":
        assert all(x <= LAZY for x in out[:8]), "limbs 0..7 <= 2^30 + 3"
        want = val(args[0]) if name == "fr30_norm" else val(args[0]) + val(args[1]) if name == "fr30_add" \
            else val(args[0]) - val(args[1]) + (1 << 12) * R
        assert v == want, "value (exact)"
        return
    assert all(x <= M30 for x in out), "exact limbs (< 2^30)"
    if name == "fr30_mul":
        t = val(args[0]) * val(args[1])
        assert v % R == t * pow(FR30_R, -1, R) % R, "residue"
        assert v * FR30_R < R * FR30_R + t, "value bound r + a b / 2^270"
    elif name == "fr30_unpack":
        assert v == val(args[0], 32)
    elif name == "fr30_sub_qr":
        assert v == val(args[0]) - args[1][0] * R
    elif name == "fr30_reduce_lazy":
        assert v % R == val(args[0]) % R, "residue"
        assert v < 2 * R, "value bound 2r"
    elif name == "fr30_const_one":
        assert v == FR30_R % R
    else:
        raise KeyError(name)


# ---- G1 (g1.hpp) -------------------------------------------------------------------------------------------------------
# Invariants of a stored XYZZ point in units of p (g1.hpp): X < 5.1, Y < 3.2, ZZ, ZZZ < 1.1; affine operands < 1.1.
X_MAX, Y_MAX, Z_MAX = 51 * P // 10, 32 * P // 10, 11 * P // 10
RINV = pow(FQ_R, -1, P)


def mont(x: int) -> int:
    return x * FQ_R % P


def unmont(x: int) -> int:
    return x * RINV % P


def random_point(rnd):
    """a random point of E(Fp) (not necessarily in the prime-order subgroup: the formulas do not care)"""
    while True:
        x = rnd.randrange(P)
        y2 = (x * x * x + O.B_COEFF) % P
        y = pow(y2, (P + 1) // 4, P)
        if y * y % P == y2 and y:
            return (x, y if rnd.random() < 0.5 else P - y)


def _lift(v: int, limit: int, rnd, top: bool) -> int:
    """v + k p with the largest k (top) or a random k that keeps the value below `limit`"""
    kmax = (limit - 1 - v) // P
    return v + P * (kmax if top else rnd.randrange(kmax + 1))


def xyzz_of(pt, rnd, top: bool = False, z: int | None = None) -> tuple:
    """the point in XYZZ form with a random (or given) Z, raw Montgomery coordinates lifted toward the invariants"""
    if pt is None:
        return (mont(1), mont(1), 0, 0) if not top else (mont(1), mont(1), P, P)
    z = z or rnd.randrange(1, P)
    zz, zzz = z * z % P, z * z * z % P
    x, y = pt
    c = (mont(x * zz % P), mont(y * zzz % P), mont(zz), mont(zzz))
    return (_lift(c[0], X_MAX, rnd, top), _lift(c[1], Y_MAX, rnd, top), _lift(c[2], Z_MAX, rnd, top), _lift(c[3], Z_MAX, rnd, top))


def jac_of(pt, rnd, top: bool = False) -> tuple:
    if pt is None:
        return (mont(1), mont(1), P if top else 0)
    z = rnd.randrange(1, P)
    x, y = pt
    c = (mont(x * z * z % P), mont(y * z * z * z % P), mont(z))
    return (_lift(c[0], X_MAX, rnd, top), _lift(c[1], Y_MAX, rnd, top), _lift(c[2], Z_MAX, rnd, top))


def affine_of(pt, rnd=None, top: bool = False) -> tuple:
    if pt is None:
        return (0, 0)
    c = (mont(pt[0]), mont(pt[1]))
    return c if rnd is None else (_lift(c[0], Z_MAX, rnd, top), _lift(c[1], Z_MAX, rnd, top))


def xyzz_point(c):
    """the group element an XYZZ tuple stands for (None: the identity), checking ZZ^3 = ZZZ^2 on the way"""
    zz, zzz = unmont(c[2]), unmont(c[3])
    if zz == 0:
        return None
    assert zzz != 0 and pow(zz, 3, P) == zzz * zzz % P, "ZZ^3 != ZZZ^2"
    return (unmont(c[0]) * pow(zz, -1, P) % P, unmont(c[1]) * pow(zzz, -1, P) % P)


def jac_point(c):
    z = unmont(c[2])
    if z == 0:
        return None
    return (unmont(c[0]) * pow(z * z, -1, P) % P, unmont(c[1]) * pow(z * z * z, -1, P) % P)


def _g1_cases(name: str) -> list[tuple]:
    """(a, b, flag) per case: a = XYZZ / Jacobian coordinates, b = XYZZ / affine (or zinv), flag = neg / k"""
    rnd = random.Random(sum(map(ord, name)))
    pts = [random_point(rnd) for _ in range(N_RAND_G1)]
    cases = []
    if name in ("g1_madd", "g1_madd_xy"):
        # g1_madd takes a stored (canonical) affine point -- its neg_lazy<1> needs y <= p --, g1_madd_xy any x, y < 1.1p
        aff = (lambda q, top: affine_of(q)) if name == "g1_madd" else (lambda q, top: affine_of(q, rnd, top))
        # a wave of identity accumulators, then P + P, P + (-P), lifted operands, random pairs
        cases += [(xyzz_of(None, rnd, i % 2 == 1), affine_of(pts[i]), 0) for i in range(WAVE)]
        for i, q in enumerate(pts):
            kind = i % 6
            top = i % 4 == 0
            neg = name == "g1_madd" and i % 3 == 0
            same = q if not neg else O.g1_neg(q)                  # the point the accumulator must equal for P + P
            if kind == 0:
                cases.append((xyzz_of(same, rnd, top), aff(q, top), neg))                 # doubling
            elif kind == 1:
                cases.append((xyzz_of(O.g1_neg(same), rnd, top), aff(q, top), neg))      # sum is the identity
            elif kind == 2 and name == "g1_madd":
                cases.append((xyzz_of(pts[i - 1], rnd, top), (0, 0), neg))                # affine identity: no-op
            else:
                cases.append((xyzz_of(pts[i - 1], rnd, top), aff(q, top), neg))
    elif name == "g1_add":
        cases += [(xyzz_of(None, rnd), xyzz_of(None, rnd, True), 0)] * WAVE
        for i, q in enumerate(pts):
            kind, top = i % 6, i % 4 == 0
            a = {0: q, 1: q, 2: None, 3: pts[i - 1], 4: pts[i - 1], 5: pts[i - 1]}[kind]
            b = {0: q, 1: O.g1_neg(q), 2: q, 3: None, 4: q, 5: q}[kind]
            cases.append((xyzz_of(a, rnd, top), xyzz_of(b, rnd, not top), 0))
    elif name == "g1_dbl":
        cases += [(xyzz_of(None, rnd, i % 2 == 1), (0, 0), 0) for i in range(WAVE)]
        cases += [(xyzz_of(q, rnd, i % 2 == 0), (0, 0), 0) for i, q in enumerate(pts)]
    elif name == "g1_dbl_affine":
        cases += [((0, 0), affine_of(q, rnd, i % 2 == 0), 0) for i, q in enumerate(pts)]
    elif name == "g1_to_affine":
        cases += [(xyzz_of(None, rnd, i % 2 == 1), (0, 0), 0) for i in range(WAVE)]
        cases += [(xyzz_of(None if i % 9 == 0 else q, rnd, i % 2 == 0), (0, 0), 0) for i, q in enumerate(pts)]
    elif name in ("g1_jac_dbl", "g1_jac_to_xyzz"):
        cases += [(jac_of(None, rnd, i % 2 == 1), (0, 0), 0) for i in range(WAVE)]
        cases += [(jac_of(None if i % 9 == 0 else q, rnd, i % 2 == 0), (0, 0), 0) for i, q in enumerate(pts)]
    elif name == "g1_jac_to_affine_with":
        for i, q in enumerate(pts):
            j = jac_of(q, rnd, i % 2 == 0)
            zinv = mont(pow(unmont(j[2]), -1, P))
            cases.append((j, (_lift(zinv, Z_MAX, rnd, i % 4 == 0), 0), 0))
    elif name == "g1_mul_small":
        ks = [0, 1, 2, 3, 4, 5, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF]
        cases += [(xyzz_of(None, rnd, i % 2 == 1), (0, 0), ks[i % len(ks)]) for i in range(WAVE)]
        cases += [(xyzz_of(q, rnd, i % 2 == 0), (0, 0), ks[i] if i < len(ks) else rnd.randrange(1 << 32))
                  for i, q in enumerate(pts[:256])]
    else:
        raise KeyError(name)
    return cases


G1_OPS = {n: i for i, n in enumerate(["g1_madd", "g1_madd_xy", "g1_add", "g1_dbl", "g1_dbl_affine", "g1_to_affine", "g1_jac_dbl",
                                      "g1_jac_to_xyzz", "g1_jac_to_affine_with", "g1_mul_small"])}
G1_JAC_IN = {"g1_jac_dbl", "g1_jac_to_xyzz", "g1_jac_to_affine_with"}


def g1_cases(name: str) -> list[tuple]:
    return _g1_cases(name)


def _xyzz_ok(c) -> bool:
    return c[0] < X_MAX and c[1] < Y_MAX and c[2] < Z_MAX and c[3] < Z_MAX


def _aff_ok(c) -> bool:
    return c[0] < Z_MAX and c[1] < Z_MAX


def g1_pre(name: str, a, b, flag) -> bool:
    if name in G1_JAC_IN:
        ok = a[0] < X_MAX and a[1] < Y_MAX and a[2] < Z_MAX
        if name == "g1_jac_to_affine_with":
            ok = ok and a[2] % P != 0 and b[0] < Z_MAX and unmont(a[2]) * unmont(b[0]) % P == 1
        return ok
    if name in ("g1_madd", "g1_madd_xy"):
        ok = _xyzz_ok(a) and (_aff_ok(b) if name == "g1_madd_xy" else b[0] < P and b[1] < P)
        if name == "g1_madd_xy":
            ok = ok and b != (0, 0)                   # the affine operand must not be the identity (callers test first)
        return ok and (b == (0, 0) or O.g1_is_on_curve((unmont(b[0]), unmont(b[1])))) and _on_curve(xyzz_point(a))
    if name == "g1_add":
        return _xyzz_ok(a) and _xyzz_ok(b) and _on_curve(xyzz_point(a)) and _on_curve(xyzz_point(b))
    if name == "g1_dbl_affine":
        return _aff_ok(b) and O.g1_is_on_curve((unmont(b[0]), unmont(b[1])))
    return _xyzz_ok(a) and _on_curve(xyzz_point(a)) and 0 <= flag < 1 << 32


def _on_curve(pt) -> bool:
    return pt is None or O.g1_is_on_curve(pt)


def g1_expected(name: str, a, b, flag):
    if name in ("g1_madd", "g1_madd_xy"):
        q = None if b == (0, 0) else (unmont(b[0]), unmont(b[1]))
        if flag and name == "g1_madd":
            q = O.g1_neg(q)
        return O.g1_add(xyzz_point(a), q)
    if name == "g1_add":
        return O.g1_add(xyzz_point(a), xyzz_point(b))
    if name == "g1_dbl":
        p = xyzz_point(a)
        return O.g1_add(p, p)
    if name == "g1_dbl_affine":
        p = (unmont(b[0]), unmont(b[1]))
        return O.g1_add(p, p)
    if name == "g1_to_affine":
        return xyzz_point(a)
    if name == "g1_jac_dbl":
        p = jac_point(a)
        return O.g1_add(p, p)
    if name in ("g1_jac_to_xyzz", "g1_jac_to_affine_with"):
        return jac_point(a)
    if name == "g1_mul_small":
        p, acc = xyzz_point(a), None
        for bit in range(31, -1, -1):
            acc = O.g1_add(acc, acc)
            if (flag >> bit) & 1:
                acc = O.g1_add(acc, p)
        return acc
    raise KeyError(name)


def g1_check(name: str, a, b, flag, out: list[int]) -> None:
    """out: the four 13-limb coordinates (XYZZ), three (Jacobian) or two (affine) as integers"""
    want = g1_expected(name, a, b, flag)
    if name in ("g1_to_affine", "g1_jac_to_affine_with"):
        assert out[0] < P and out[1] < P, "affine output not canonical"
        assert (None if out[:2] == [0, 0] else (unmont(out[0]), unmont(out[1]))) == want, "point"
        return
    if name == "g1_jac_dbl":
        assert out[0] < X_MAX and out[1] < Y_MAX and out[2] < Z_MAX, "Jacobian invariants X < 5.1p, Y < 3.2p, Z < 1.1p"
        assert jac_point(out[:3]) == want, "point"
        return
    assert _xyzz_ok(out), "XYZZ invariants X < 5.1p, Y < 3.2p, ZZ, ZZZ < 1.1p"
    assert xyzz_point(out) == want, "point"


# ---- wavefront butterflies (msm_common.hpp) ----------------------------------------------------------------------------
# One case = (label, param, wave): 64 XYZZ tuples, lane by lane, for butterfly_add(v, mask), butterfly_add4(v, mask)
# (identical on lanes l and l ^ 1: its precondition) or butterfly_reduce(v, lanes).  Every kind of wave is built twice: with
# random lifts of the coordinates and with the largest lifts the XYZZ invariants admit (`top`).
WAVE_OPS = {"butterfly_add": 0, "butterfly_add4": 1, "butterfly_reduce": 2}
WAVE_PARAMS = {"butterfly_add": (1, 2, 4, 8, 16, 32), "butterfly_add4": (2, 4, 8, 16, 32), "butterfly_reduce": (1, 2, 4, 8, 16, 32, 64)}
_WAVE_POOL: list = []


def wave_pool() -> list:
    """random points of E(Fp), made once (a square root each)"""
    if not _WAVE_POOL:
        rnd = random.Random(0xB077E7F1)
        while len(_WAVE_POOL) < 3 * WAVE:
            q = random_point(rnd)
            if q not in _WAVE_POOL and O.g1_neg(q) not in _WAVE_POOL:
                _WAVE_POOL.append(q)
    return _WAVE_POOL


def _pair_units(rnd, units: int, pm: int, top: bool) -> list[tuple[str, list]]:
    """the waves of one butterfly step as `units` operands, unit u meeting unit u ^ pm (butterfly_add: a unit is a lane and
    pm the mask; butterfly_add4: a unit is the lane pair {2u, 2u + 1} and pm = mask / 2)"""
    pool = wave_pool()
    lower = [u for u in range(units) if not u & pm]

    def ordinary():
        return [xyzz_of(q, rnd, top) for q in rnd.sample(pool, units)]

    def inf(alt=False):
        return xyzz_of(None, rnd, top != alt)

    def with_z(q, z):
        return xyzz_of(q, rnd, top, z)

    out = [("random", ordinary())]
    out.append(("identity", [inf() for _ in range(units)]))
    if not top:   # both encodings of the identity in one wave, also as partners
        out.append(("identity, both encodings", [inf(rnd.random() < 0.5) for _ in range(units)]))
    w = ordinary()
    out.append(("identity below", [inf(u % 3 == 0) if not u & pm else w[u] for u in range(units)]))
    out.append(("identity above", [inf(u % 3 == 0) if u & pm else w[u] for u in range(units)]))
    out.append(("identity on a random subset", [inf(rnd.random() < 0.5) if rnd.random() < 0.4 else w[u] for u in range(units)]))
    w = ordinary()
    out.append(("same point, different Z", [xyzz_of(pool[min(u, u ^ pm)], rnd, top) for u in range(units)]))
    for u in lower:
        w[u ^ pm] = w[u]
    out.append(("same point, identical words", list(w)))
    out.append(("opposite points, different Z",
                [xyzz_of(pool[u] if not u & pm else O.g1_neg(pool[u ^ pm]), rnd, top) for u in range(units)]))
    # exactly one exceptional pair among ordinary ones: the wave-uniform branch runs for it alone
    for where, u in (("first", lower[0]), ("last", lower[-1]), ("middle", lower[len(lower) // 2])):
        for kind in ("equal", "opposite", "identity"):
            w = ordinary()
            a = xyzz_point(w[u])
            w[u ^ pm] = with_z(a, None) if kind == "equal" else with_z(O.g1_neg(a), None) if kind == "opposite" else inf()
            if kind == "identity" and where == "middle":
                w[u], w[u ^ pm] = w[u ^ pm], w[u]
            out.append((f"one {kind} pair, {where}", w))
    return out


def _reduce_waves(rnd, top: bool) -> list[tuple[str, list]]:
    pool = wave_pool()
    lane = lambda q: xyzz_of(q, rnd, top)   # noqa: E731
    inf = lambda: xyzz_of(None, rnd, top != (rnd.random() < 0.3))   # noqa: E731
    out = [("random", [lane(q) for q in rnd.sample(pool, WAVE)])]
    out.append(("identity", [inf() for _ in range(WAVE)]))
    w = [lane(q) for q in rnd.sample(pool, WAVE)]
    out.append(("identity on a random subset", [inf() if rnd.random() < 0.4 else w[i] for i in range(WAVE)]))
    out.append(("same point on lane pairs, different Z", [lane(pool[i // 2]) for i in range(WAVE)]))
    out.append(("opposite points on lane pairs", [lane(pool[i // 2] if i % 2 == 0 else O.g1_neg(pool[i // 2])) for i in range(WAVE)]))
    # the exception arises at the second step: P + Q meets Q + P in another representation; P + Q meets -(P + Q)
    out.append(("P Q Q P", [lane(pool[2 * (i // 4) + (1 if i % 4 in (1, 2) else 0)]) for i in range(WAVE)]))
    out.append(("P Q -P -Q", [lane(pool[2 * (i // 4) + i % 2] if i % 4 < 2 else O.g1_neg(pool[2 * (i // 4) + i % 2])) for i in range(WAVE)]))
    out.append(("one point, a Z per lane", [lane(pool[7]) for _ in range(WAVE)]))
    out.append(("one point, identical words", [lane(pool[8])] * WAVE))
    # 2A on lanes 0 and 1 in two representations, then a step that takes its operand from both lanes
    w = [lane(q) for q in rnd.sample(pool[16:], WAVE)]
    w[0], w[1], w[2], w[3] = lane(pool[9]), lane(pool[9]), lane(pool[10]), inf()
    out.append(("A A H identity, then random", w))
    return out


def wave_cases(name: str) -> list[tuple]:
    rnd = random.Random(sum(map(ord, name)))
    cases = []
    for param in WAVE_PARAMS[name]:
        for top in (False, True):
            tag = ", top lift" if top else ""
            if name == "butterfly_add":
                cases += [(label + tag, param, w) for label, w in _pair_units(rnd, WAVE, param, top)]
            elif name == "butterfly_add4":
                cases += [(label + tag, param, [u for u in w for _ in range(2)]) for label, w in _pair_units(rnd, WAVE // 2, param // 2, top)]
            else:
                cases += [(label + tag, param, w) for label, w in _reduce_waves(rnd, top)]
    return cases


def wave_min_distinct(name: str) -> int:
    """the fewest distinct waves an op's list may hold"""
    return {"butterfly_add": 200, "butterfly_add4": 170, "butterfly_reduce": 130}[name]


def wave_pre(name: str, param: int, wave) -> bool:
    ok = len(wave) == WAVE and param in WAVE_PARAMS[name] and all(_xyzz_ok(c) and _on_curve(xyzz_point(c)) for c in wave)
    if name == "butterfly_add4":
        ok = ok and all(wave[i] == wave[i ^ 1] for i in range(WAVE))
    return ok


def wave_expected(name: str, param: int, wave) -> list:
    """the group element every lane holds afterwards"""
    pts = [xyzz_point(c) for c in wave]
    if name != "butterfly_reduce":
        return [O.g1_add(pts[i], pts[i ^ param]) for i in range(WAVE)]
    sums = []
    for g in range(0, WAVE, param):
        acc = None
        for q in pts[g:g + param]:
            acc = O.g1_add(acc, q)
        sums += [acc] * param
    return sums


def wave_check(name: str, param: int, wave, out: list) -> None:
    """out: per lane the four coordinates as integers.  Every lane holds the sum (butterfly_reduce: of its group of `param`
    lanes, the first lane of a group being the one the kernels store) within the XYZZ invariants, and lanes l and l ^ 1 hold
    identical words wherever a four-lane step may follow: after butterfly_add (on the two lanes of a pair, whatever the
    mask), after butterfly_add4, and after butterfly_reduce over more than one lane."""
    want = wave_expected(name, param, wave)
    for i in range(WAVE):
        assert _xyzz_ok(out[i]), f"lane {i}: XYZZ invariants X < 5.1p, Y < 3.2p, ZZ, ZZZ < 1.1p"
        assert xyzz_point(out[i]) == want[i], f"lane {i}: point"
    partner = param if name == "butterfly_add" else 1
    if name != "butterfly_reduce" or param > 1:
        for i in range(WAVE):
            assert out[i] == out[i ^ partner], f"lanes {i} and {i ^ partner} hold different words"
