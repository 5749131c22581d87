"""g1_madd_acc / g1_acc_finish (csrc/g1.hpp), the mixed addition of the MSM's accumulation loops with its identity and sign
bits carried beside the point, without a GPU: the header as the host compiles it (tests/cpp/madd_acc_host, a program with its
own main and no HIP include) against Python big integers (oracle/bls12_381.py).

A case is a start -- the empty accumulator or a stored XYZZ bucket, as a later chunk of an MSM loads it -- and 0, 1, 2, 3, 4 or 7
signed additions of multiples of G.  Each addend is a fresh multiple, the point the sum already holds (the doubling path), its
opposite (the sum becomes the identity, and later additions start again from it) or an SRS identity (0, 0).  After
g1_acc_finish the point must be the expected one as an AFFINE point (or the identity, ZZ = 0 mod p) and must keep the
invariants of a stored bucket: limbs below 2^30, X < 5.1 p, Y < 3.2 p, ZZ, ZZZ < 1.1 p.  The program also prints the flags word
after every addition, from which the test checks that the cases reached what they were built for: an equal point as the 1st,
2nd and 3rd addend with either sign and -- where an addition has come before -- either parity of the sign bit, an opposite
point followed by further additions, and an identity in every position.  The same cases run once more through the build
under the address and undefined-behaviour sanitizers (a plain executable)."""
import os
import random
import subprocess

import pytest

from helpers import O, ROOT

P = O.P
MONT = (1 << 390) % P                      # the kernels' Montgomery radix (fq30.hpp)
MONT_INV = pow(MONT, -1, P)
INF, FLIP = 1, 2
LENGTHS = (0, 1, 2, 3, 4, 7)

_mul_cache = {}


def mul_g(k):
    """k G as an affine point (None = identity), k any integer"""
    if k not in _mul_cache:
        pt = O.g1_mul(O.G1, abs(k) % O.R) if k else None
        _mul_cache[k] = O.g1_neg(pt) if k < 0 and pt is not None else pt
    return _mul_cache[k]


def to_mont(v):
    return v * MONT % P


def stored_bucket(k, lam, lift):
    """k G as the XYZZ words (lam^2 x, lam^3 y, lam^2, lam^3), each lifted by lift[i] p (within the stored invariants)"""
    x, y = mul_g(k)
    vals = [x * lam * lam % P, y * lam ** 3 % P, lam * lam % P, lam ** 3 % P]
    return [to_mont(v) + l * P for v, l in zip(vals, lift)]


def make_cases():
    """[(stored words or None, start multiple, [(kind, multiple, neg)])], kinds: 'pt', 'eq', 'opp', 'id'"""
    rng = random.Random(0x6D616464)
    cases = []
    starts = [(None, 0)]
    for k, lift in ((3, (0, 0, 0, 0)), (-5, (4, 2, 0, 0)), (7, (3, 1, 0, 0)), (2, (0, 2, 0, 0))):
        starts.append((stored_bucket(k, rng.randrange(2, P), lift), k))
    starts.append(([to_mont(1), to_mont(1), 0, 0], 0))          # a stored identity, ZZ = 0
    starts.append(([to_mont(5), to_mont(9), P, P], 0))          # ... and in its other encoding, ZZ = p

    def run(start, plan):
        """plan: kinds; resolves 'eq' / 'opp' against the running sum (a fresh point where the sum is the identity)"""
        words, total = start
        ops = []
        for kind in plan:
            if kind == "id":
                ops.append(("id", 0, rng.randrange(2)))
                continue
            if kind in ("eq", "opp") and total != 0:
                k = total if kind == "eq" else -total
            else:
                kind, k = "pt", rng.choice([1, 2, 3, 4, 5, 6, 9]) * rng.choice([1, -1])
                if k == total or k == -total:                    # keep 'pt' a fresh point
                    k += 11 if k > 0 else -11
            ops.append((kind, k, 1 if k < 0 else 0))
            total += k
        cases.append((words, start[1], ops))

    # directed: an equal / opposite point in positions 1..3 after every sign pattern of the additions before it
    for start in starts:
        for pos in (1, 2, 3):
            for special in ("eq", "opp"):
                for _ in range(6):
                    for tail in (0, 1, 4):
                        run(start, ["pt"] * (pos - 1) + [special] + ["pt"] * tail)
    # an identity in every position of every length, alone and next to the special points
    for start in starts:
        for n in LENGTHS:
            for pos in range(n):
                plan = [rng.choice(["pt", "pt", "eq", "opp"]) for _ in range(n)]
                plan[pos] = "id"
                run(start, plan)
    # random blends of every length
    for start in starts:
        for n in LENGTHS:
            for _ in range(4 if n else 1):
                run(start, [rng.choice(["pt", "pt", "pt", "eq", "opp", "id"]) for _ in range(n)])
    return cases


def case_text(case):
    words, _, ops = case
    out = ["1 " + " ".join("%x" % w for w in words) if words else "0", str(len(ops))]
    for _, k, neg in ops:
        if k == 0:
            out.append("0 0 %d" % neg)
        else:
            x, y = mul_g(abs(k))
            out.append("%x %x %d" % (to_mont(x), to_mont(y), neg))
    return " ".join(out)


@pytest.fixture(scope="module")
def cases():
    return make_cases()


@pytest.fixture(scope="module")
def text(cases):
    return "\n".join(case_text(c) for c in cases) + "\n"


def run_program(name, text):
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", name)], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = []
    for line in r.stdout.splitlines():
        flags, limbs = line.split("|")
        out.append(([int(f, 16) for f in flags.split()], [int(x, 16) for x in limbs.split()]))
    return out


@pytest.fixture(scope="module")
def results(built, cases, text):
    out = run_program("madd_acc_host", text)
    assert len(out) == len(cases)
    return out


def value(limbs):
    assert len(limbs) == 13 and all(0 <= v < (1 << 30) for v in limbs), limbs
    return sum(v << (30 * i) for i, v in enumerate(limbs))


def test_every_sum_is_the_expected_affine_point_within_the_stored_bounds(cases, results):
    for (words, k0, ops), (flags, limbs) in zip(cases, results):
        assert len(limbs) == 52 and len(flags) == len(ops) + 1
        X, Y, ZZ, ZZZ = (value(limbs[13 * i:13 * i + 13]) for i in range(4))
        # bounds in units of p, exactly: X < 5.1, Y < 3.2, ZZ, ZZZ < 1.1
        assert 10 * X < 51 * P and 10 * Y < 32 * P and 10 * ZZ < 11 * P and 10 * ZZZ < 11 * P, (k0, ops)
        want = mul_g(k0 + sum(k for _, k, _ in ops))
        if want is None:
            assert ZZ % P == 0 and flags[-1] & INF, (k0, ops)
            continue
        assert ZZ % P != 0 and not flags[-1] & INF, (k0, ops)
        zz, zzz = ZZ * MONT_INV % P, ZZZ * MONT_INV % P
        assert pow(zz, 3, P) == zzz * zzz % P, (k0, ops)
        got = (X * MONT_INV * pow(zz, -1, P) % P, Y * MONT_INV * pow(zzz, -1, P) % P)
        assert got == want, (k0, ops)


def test_the_sign_bit_is_clear_on_a_stored_start_and_toggles_on_every_full_addition(cases, results):
    for (words, k0, ops), (flags, _) in zip(cases, results):
        assert flags[0] == (INF if k0 == 0 else 0)
        total = k0
        for (kind, k, neg), before, after in zip(ops, flags, flags[1:]):
            if kind == "id":
                assert after == before
            elif total == 0:
                assert before & INF and after == (FLIP if neg else 0)      # the sum is the point itself, signed by the bit
            elif kind == "eq":
                assert after == 0                                          # a doubling is held with its true sign
            elif kind == "opp":
                assert after & INF
            else:
                assert after == before ^ FLIP
            total += k


def test_the_cases_reach_every_path_they_were_built_for(cases, results):
    seen = set()
    for (words, k0, ops), (flags, _) in zip(cases, results):
        total, adds = k0, 0
        for pos, ((kind, k, neg), before) in enumerate(zip(ops, flags), 1):
            if kind == "id":
                seen.add(("id", pos, len(ops)))
                continue
            if kind in ("eq", "opp") and total != 0:
                seen.add((kind, pos, neg, bool(before & FLIP)))
                if kind == "opp" and pos < len(ops) and any(o[0] != "id" for o in ops[pos:]):
                    seen.add("opp then more")
            total += k
            adds += 1
        seen.add(("len", len(ops), words is not None))
    for kind in ("eq", "opp"):
        for neg in (0, 1):
            assert (kind, 1, neg, False) in seen                     # the 1st addend meets a stored bucket: sign bit clear
            for pos in (2, 3):
                for flip in (False, True):
                    assert (kind, pos, neg, flip) in seen, (kind, pos, neg, flip)
    assert "opp then more" in seen
    for n in LENGTHS:
        assert ("len", n, False) in seen and ("len", n, True) in seen
        for pos in range(1, n + 1):
            assert ("id", pos, n) in seen


def test_the_same_cases_under_the_address_and_undefined_behaviour_sanitizers(built, cases, text, results):
    assert run_program("madd_acc_host_san", text) == results


def test_host_program_refuses_a_case_cut_short(built):
    exe = os.path.join(ROOT, "tests", "cpp", "madd_acc_host")
    assert subprocess.run([exe], input="0 1 5 7\n", capture_output=True, text=True, timeout=60).returncode == 2
    assert subprocess.run([exe], input="0 1 5 xyz 0\n", capture_output=True, text=True, timeout=60).returncode == 2
    r = subprocess.run([exe], input="", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == ""
