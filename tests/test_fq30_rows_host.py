"""csrc/fq30_rows.hpp -- Fq with one limb per lane of a 16-lane row, and g1_add_rows, one XYZZ addition per wavefront --
without a GPU: the header as the host compiles it over RowsHost, the array-of-64 wave (tests/cpp/fq30_rows_host, a program
with its own main and no HIP include), against Python integers.  The device build runs the same arithmetic text
(tests/test_gpu_reduce_rows.py).

Multiplication: the exact REDC value (a b + m p) / 2^390 with m = -a b / p mod 2^390, hence residue and value bound, and
limbs within the stated loose bound 2^30 + 3, on random inputs, 0, 1, p - 1, every limb at the loose maximum, and the largest
values the contract a b < (2^390 - p) 2^390 admits.  Lazy operations: exact integer results at their bounds.  The program
marks a line when the four rows disagree, when a lane above 12 is not zero or when a 64-bit accumulator wrapped."""
import os
import random
import subprocess

import pytest

from helpers import O, ROOT

P = O.P
R = 1 << 390
MASK = (1 << 30) - 1
LOOSE = (1 << 30) + 3
MONT = R % P
MONT_INV = pow(MONT, -1, P)


def limbs(v):
    assert 0 <= v < R
    return [(v >> (30 * i)) & MASK for i in range(13)]


def val(ls):
    return sum(x << (30 * i) for i, x in enumerate(ls))


def hexes(xs):
    return " ".join("%x" % x for x in xs)


def loosen(v, rng):
    """the same value in loose limbs where it has any: a limb <= 3 may take 2^30 from the limb above"""
    ls = limbs(v)
    for i in range(12):
        k = min(rng.randrange(2), ls[i + 1], (LOOSE - ls[i]) >> 30)
        ls[i] += k << 30
        ls[i + 1] -= k
    assert val(ls) == v and all(0 <= x <= LOOSE for x in ls)
    return ls


def loose_random(rng):
    """13 limbs drawn at and around the loose maximum (a value below 2^382: the top limb stays under 2^21)"""
    return [rng.choice((LOOSE, LOOSE - 1, 1 << 30, MASK, 0, 1, rng.randrange(LOOSE + 1))) for _ in range(12)] + [rng.randrange(1 << 21)]


def run(name, lines):
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", name)], input="\n".join(lines) + "\n", capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def parse(line):
    assert "!" not in line, "rows disagree, a lane above 12 is not zero, or an accumulator wrapped: " + line
    return [int(x, 16) for x in line.split()]


# ---- the cases: (command line, check(list of numbers)) -----------------------------------------------------------------------
def redc(a, b):
    m = (-(a * b) * pow(P, -1, R)) % R
    return (a * b + m * P) >> 390


def make_cases():
    rng = random.Random(0x726F7773)
    cases = []

    def mul_case(la, lb):
        a, b = val(la), val(lb)
        assert a * b < (R - P) * R

        def check(got):
            assert len(got) == 13 and all(0 <= x <= LOOSE for x in got)
            v = val(got)
            assert v == redc(a, b)                                   # the exact REDC value ...
            assert v % P == a * b * pow(R, -1, P) % P and v * R < P * R + a * b + R   # ... hence the residue and v < p + a b / 2^390
        cases.append(("mul " + hexes(la) + " " + hexes(lb), check))

    top = (R - P - 1)
    loose_max = [LOOSE] * 12 + [(8 * P) >> 360]                      # every limb at the loose maximum, the value below 2^390
    for _ in range(40):
        a, b = rng.randrange(8 * P), rng.randrange(8 * P)
        mul_case(limbs(a), limbs(b))
        mul_case(loosen(a, rng), loosen(b, rng))
        mul_case(loose_random(rng), loose_random(rng))
    for a in (0, 1, P - 1, P, MONT):
        for b in (0, 1, P - 1, rng.randrange(P)):
            mul_case(limbs(a), limbs(b))
    mul_case(loose_max, loose_max)
    mul_case(loose_max, limbs(P - 1))
    mul_case([MASK] * 13, limbs(top >> 1))                           # 2^390 - 1 times the largest partner the contract admits
    mul_case(limbs(top), [MASK] * 13)
    mul_case(limbs(R - 1), limbs(R - P - 1))                         # a b < (2^390 - p) 2^390 at its edge

    def lazy(cmd, ops, want):
        def check(got):
            assert len(got) == 13 and all(0 <= x <= LOOSE for x in got), cmd
            assert val(got) == want, cmd
        cases.append((cmd + " " + " ".join(hexes(o) for o in ops), check))

    lm = val(loose_max)
    for _ in range(10):
        a, b, c = rng.randrange(5 * P), rng.randrange(2 * P - (1 << 361)), rng.randrange(2 * P)
        ra, rb = loose_random(rng), loose_random(rng)
        lazy("add", (ra, rb), val(ra) + val(rb))
        lazy("sub 2", (ra, rb), val(ra) + 2 * P - val(rb))
        rc = loose_random(rng)
        lazy("sub2 4", (ra, rb, rc), val(ra) + 4 * P - val(rb) - val(rc))
        lazy("mulk 3", (ra,), 3 * val(ra))
        for la, lb in ((limbs(a), limbs(b)), (loosen(a, rng), loosen(b, rng))):
            lazy("add", (la, lb), a + b)
            lazy("sub 2", (la, lb), a + 2 * P - b)
            lazy("sub 4", (la, lb), a + 4 * P - b)
            lazy("sub 6", (la, lb), a + 6 * P - b)
            lazy("sub2 4", (la, lb, loosen(c, rng)), a + 4 * P - b - c)
            lazy("mulk 2", (la,), 2 * a)
            lazy("mulk 3", (la,), 3 * a)
            lazy("sel 1", (la, lb), a)
            lazy("sel 0", (la, lb), b)
    # at the bounds: loose maxima on both sides; the largest subtrahend K p - 2^361; a = 0 against it
    lazy("add", (loose_max, loose_max), 2 * lm)
    lazy("mulk 3", (loose_max,), 3 * lm)
    for k in (2, 4, 6):
        big = k * P - (1 << 361)
        lazy("sub %d" % k, (limbs(0), limbs(big)), k * P - big)
        lazy("sub %d" % k, (limbs(0), loosen(big, rng)), k * P - big)
        lazy("sub %d" % k, (loose_max, limbs(0)), lm + k * P)
        lazy("sub %d" % k, (limbs(0), limbs(0)), k * P)
    lazy("sub2 4", (limbs(0), loosen(2 * P, rng), loosen(2 * P - (1 << 361), rng)), 1 << 361)
    lazy("sub2 4", (loose_max, limbs(0), limbs(0)), lm + 4 * P)

    # zero test on values < 2p: 0, p, p +- 1, and p in loose limbs
    for v, want in ((0, 1), (P, 1), (P + 1, 0), (P - 1, 0), (1, 0), (2 * P - 1, 0), (P + (1 << 30), 0), (P ^ (1 << 200), 0)):
        for ls in (limbs(v), loosen(v, rng)):
            def check(got, want=want, v=v):
                assert got[0] == want, hex(v)
                assert got[1] == 1 or not want                       # the cheap test never misses a zero
            cases.append(("zero " + hexes(ls), check))

    # packed form: against fq30_unpack / fq30_pack (printed by the program) and against the integers
    for v in [0, 1, P - 1, (1 << 384) - 1, 8 * P - 1] + [rng.randrange(1 << 384) for _ in range(10)]:
        words = [(v >> (32 * j)) & 0xFFFFFFFF for j in range(12)]

        def check_load(got, v=v):
            assert got[:13] == got[13:] == limbs(v)
        cases.append(("load " + hexes(words), check_load))
        for ls in (limbs(v), loosen(v, rng)):
            def check_store(got, words=words):
                assert got[:12] == got[12:] == words
            cases.append(("store " + hexes(ls), check_store))
    return cases


@pytest.fixture(scope="module")
def cases():
    return make_cases()


def test_every_field_operation_matches_python_integers_within_the_loose_bound(built, cases):
    out = run("fq30_rows_host", [c for c, _ in cases])
    for (cmd, check), line in zip(cases, out):
        check(parse(line))


# ---- g1_add_rows -----------------------------------------------------------------------------------------------------------------
_mul = {}


def mul_g(k):
    if k not in _mul:
        pt = O.g1_mul(O.G1, abs(k) % O.R) if k else None
        _mul[k] = O.g1_neg(pt) if k < 0 and pt is not None else pt
    return _mul[k]


def stored(k, lam, lift, rng, ident_p=False):
    """k G as stored XYZZ limbs (52), coordinates lifted by lift[i] p within the stored invariants; k = 0: the identity"""
    if k == 0:
        vals = [MONT, MONT, P if ident_p else 0, P if ident_p else 0]
    else:
        x, y = mul_g(k)
        vals = [x * lam * lam % P * MONT % P, y * lam ** 3 % P * MONT % P, lam * lam % P * MONT % P, lam ** 3 % P * MONT % P]
        vals = [v + l * P for v, l in zip(vals, lift)]
    return [x for v in vals for x in loosen(v, rng)]


def point_pairs():
    """[(k_a, k_b, limbs of A, limbs of B)]: random pairs, identity on either side and both (either encoding), P + P,
    P + (-P), one point in two representations"""
    rng = random.Random(0x70616972)
    out = []

    def add(ka, kb, pa=False, pb=False):
        la = stored(ka, rng.randrange(2, P), (rng.randrange(5), rng.randrange(3), 0, 0), rng, pa)
        lb = stored(kb, rng.randrange(2, P), (rng.randrange(5), rng.randrange(3), 0, 0), rng, pb)
        out.append((ka, kb, la, lb))

    for _ in range(24):
        ka, kb = rng.randrange(1, 50), rng.randrange(51, 99)
        add(ka * rng.choice((1, -1)), kb * rng.choice((1, -1)))
    for pa in (False, True):
        for pb in (False, True):
            add(0, 7, pa)
            add(-9, 0, False, pb)
            add(0, 0, pa, pb)
    for k in (1, 5, -11, 23):
        add(k, k)                                                    # P + P: two representations of one point (two lambdas)
        add(k, -k)                                                   # P + (-P)
    while len(out) < 64:
        k = rng.randrange(1, 40)
        add(k, rng.choice((k, -k, k + 1, 0)))
    # the same words on both sides: P + P with equal representations
    out[-1] = (out[-1][0], out[-1][0], out[-1][2], list(out[-1][2]))
    return out[:64]


def check_sum(ka, kb, X, Y, ZZ, ZZZ):
    """(X, Y, ZZ, ZZZ) integers: (ka + kb) G as an affine point within the stored invariants"""
    assert 10 * X < 51 * P and 10 * Y < 32 * P and 10 * ZZ < 11 * P and 10 * ZZZ < 11 * P, (ka, kb)
    want = mul_g(ka + kb)
    if want is None:
        assert ZZ % P == 0, (ka, kb)
        return
    assert ZZ % P != 0, (ka, kb)
    zz, zzz = ZZ * MONT_INV % P, ZZZ * MONT_INV % P
    assert pow(zz, 3, P) == zzz * zzz % P, (ka, kb)
    assert (X * MONT_INV * pow(zz, -1, P) % P, Y * MONT_INV * pow(zzz, -1, P) % P) == want, (ka, kb)


@pytest.fixture(scope="module")
def pairs():
    return point_pairs()


def test_g1_add_rows_gives_the_affine_sum_on_ordinary_and_exceptional_pairs(built, pairs):
    out = run("fq30_rows_host", ["gadd " + hexes(la) + " " + hexes(lb) for _, _, la, lb in pairs])
    slow_seen = fast_seen = 0
    for (ka, kb, _, _), line in zip(pairs, out):
        got = parse(line)
        assert len(got) == 53 and all(0 <= x <= LOOSE for x in got[:52])
        check_sum(ka, kb, *(val(got[13 * i:13 * i + 13]) for i in range(4)))
        exceptional = ka == 0 or kb == 0 or ka == kb or ka == -kb
        assert got[52] == (1 if exceptional else 0), (ka, kb)         # the slow path where it must run and (2^-29) nowhere else
        slow_seen += got[52]
        fast_seen += 1 - got[52]
    assert slow_seen >= 20 and fast_seen >= 24


def test_the_same_commands_under_the_address_and_undefined_behaviour_sanitizers(built, cases, pairs):
    lines = [c for c, _ in cases] + ["gadd " + hexes(la) + " " + hexes(lb) for _, _, la, lb in pairs]
    assert run("fq30_rows_host_san", lines) == run("fq30_rows_host", lines)


def test_host_program_refuses_a_line_that_does_not_parse(built):
    exe = os.path.join(ROOT, "tests", "cpp", "fq30_rows_host")
    for text in ("mul 1 2 3\n", "frob 1\n", "zero " + "0 " * 12 + "xyz\n", "zero " + "0 " * 14 + "\n"):
        assert subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60).returncode == 2
    r = subprocess.run([exe], input="", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == ""
