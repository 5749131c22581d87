"""CPU suite for the product's host side: the shared Fp/Fr/G1 arithmetic headers (through the
host shim), the host-only C-ABI helper, and that the HIP library loads and exports every symbol
include/typlonk.h declares.  No GPU compute is called."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

from helpers import O, ROOT, g1_pack, g1_unpack_one, u32p


@pytest.fixture(scope="module")
def shim(built):
    return ctypes.CDLL(os.path.join(ROOT, "tests", "cpp", "libff_host_shim.so"))


def _fr(x):
    return np.array(O.fr_to_mont_limbs(x), dtype=np.uint64)


def _fq(x):
    return np.array(O.fq_to_mont_limbs(x), dtype=np.uint64)


def _call(shim, fn, n, *args):
    o = np.zeros(n, dtype=np.uint64)
    getattr(shim, fn)(*[u32p(a) for a in args], u32p(o))
    return [int(v) for v in o]


def test_fr_arithmetic_vs_bigint(shim):
    rnd = random.Random(1)
    er = [0, 1, 2, O.R - 1, O.R - 2, (1 << 255) % O.R, (1 << 32) - 1, 1 << 32]
    for it in range(600):
        a = rnd.choice(er) if it < 64 else rnd.randrange(O.R)
        b = er[it % 8] if it < 64 else rnd.randrange(O.R)
        assert O.fr_from_mont_limbs(_call(shim, "shim_fr_mul", 4, _fr(a), _fr(b))) == a * b % O.R
        assert O.fr_from_mont_limbs(_call(shim, "shim_fr_add", 4, _fr(a), _fr(b))) == (a + b) % O.R
        assert O.fr_from_mont_limbs(_call(shim, "shim_fr_sub", 4, _fr(a), _fr(b))) == (a - b) % O.R
        x = _call(shim, "shim_fr_from_mont", 4, _fr(a))
        assert sum(v << (64 * i) for i, v in enumerate(x)) == a
    for a in [1, 2, 5, rnd.randrange(O.R)]:
        assert O.fr_from_mont_limbs(_call(shim, "shim_fr_inv", 4, _fr(a))) == pow(a, -1, O.R)


def test_fr_divsteps_inversion_vs_bigint(shim):
    """the device's Fr inversion (csrc/fr_inv.hpp: Bernstein-Yang divsteps on nine signed 30-bit limbs; the grand product's
    one inversion, permutation/src/proving.rs:18-24) compiled for the host: equal to Python's pow and to the Fermat ladder
    on edge values and 3000 random residues, 0 -> 0, inside the 25-round bound of Theorem 11.2"""
    rnd = random.Random(11)
    edge = [0, 1, 2, 3, O.R - 1, O.R - 2, (O.R + 1) // 2, (1 << 254) % O.R, (1 << 30) - 1, 1 << 30, (1 << 240) + 1,
            pow(1 << 256, -1, O.R), (1 << 256) % O.R]
    worst = 0
    for it in range(3000):
        a = edge[it] if it < len(edge) else rnd.randrange(O.R)
        o = np.zeros(4, dtype=np.uint64)
        rounds = shim.shim_fr_inv_divsteps(u32p(_fr(a)), u32p(o))
        got = O.fr_from_mont_limbs([int(v) for v in o])
        assert got == (pow(a, -1, O.R) if a else 0), hex(a)
        assert 0 <= rounds <= 25
        worst = max(worst, rounds)
        if it < 40:
            assert [int(v) for v in o] == _call(shim, "shim_fr_inv", 4, _fr(a))   # same words as a^(r-2)
    assert worst >= 15   # the loop really runs (a broken early exit would return the initial d = 0)


def _q(shim, fn, *args):
    """call a shim Fq function: numpy arrays are passed as u32 pointers, ints as ints"""
    o = np.zeros(6, dtype=np.uint64)
    getattr(shim, fn)(*[u32p(a) if isinstance(a, np.ndarray) else a for a in args], u32p(o))
    return O.fq_from_mont_limbs([int(v) for v in o])


def test_fq30_arithmetic_vs_bigint(shim):
    """13 x 30-bit lazily reduced Fq: every operation, with operands lifted by multiples of p up to
    the bounds the group law uses, against Python big ints (through the arkworks in/out conversions)"""
    rnd = random.Random(3)
    ep = [0, 1, 2, O.P - 1, O.P - 2, (1 << 380) % O.P, (1 << 30) - 1, 1 << 30, (1 << 360) - 1]
    for it in range(400):
        a = ep[it % 9] if it < 81 else rnd.randrange(O.P)
        b = ep[(it // 9) % 9] if it < 81 else rnd.randrange(O.P)
        c = rnd.randrange(O.P)
        la, lb = rnd.randrange(0, 7), rnd.randrange(0, 7)
        assert _q(shim, "shim_fq_roundtrip", _fq(a)) == a
        assert _q(shim, "shim_fq_mul", _fq(a), _fq(b), la, lb) == a * b % O.P
        assert _q(shim, "shim_fq_sqr", _fq(a), la) == a * a % O.P
        assert _q(shim, "shim_fq_add", _fq(a), _fq(b), la % 4, lb % 4) == (a + b) % O.P
        assert _q(shim, "shim_fq_sub", _fq(a), _fq(b), la, lb % 6) == (a - b) % O.P
        assert _q(shim, "shim_fq_sub2", _fq(a), _fq(b), _fq(c)) == (a - b - c) % O.P
        assert _q(shim, "shim_fq_mul3", _fq(a)) == 3 * a % O.P
        assert _q(shim, "shim_fq_neg", _fq(a)) == (-a) % O.P
        assert shim.shim_fq_is_zero_mod(u32p(_fq(a)), 0) == (1 if a == 0 else 0)
    assert shim.shim_fq_is_zero_mod(u32p(_fq(0)), 1) == 1       # the value p itself
    assert shim.shim_fq_is_zero_mod(u32p(_fq(1)), 1) == 0
    for a in [1, 2, 5, O.P - 1, (O.P + 1) // 2, 1 << 380] + [rnd.randrange(O.P) for _ in range(40)]:
        assert _q(shim, "shim_fq_inv", _fq(a)) == pow(a, -1, O.P)
        for la in (0, 1, 5):   # lazily reduced inputs; the host's Euclid inversion equals the device's Fermat ladder
            assert shim.shim_fq_inv_agree(u32p(_fq(a)), la) == 1
    assert _q(shim, "shim_fq_inv", _fq(0)) == 0
    # pack/unpack is the identity on any 384-bit word pattern
    for _ in range(50):
        w = np.array([rnd.getrandbits(64) for _ in range(6)], dtype=np.uint64)
        o = np.zeros(6, dtype=np.uint64)
        shim.shim_fq_pack_unpack(u32p(w), u32p(o))
        assert (o == w).all()


def test_fq30_divsteps_inversion_equals_fermat_and_euclid(shim):
    """the device's SIMT inversion (Bernstein-Yang divsteps on 13 signed 30-bit limbs, fq30.hpp) digit for digit against
    the Fermat ladder a^(p-2) and the host's binary Euclid: edge values, inputs lifted up to 8p, 200,000 random residues
    (every 500th also through the ladder), x * x^-1 = 1, and the round count stays inside the proven bound of 37"""
    rnd = random.Random(11)
    edges = [0, 1, 2, 3, O.P - 1, O.P - 2, (O.P + 1) // 2, (O.P - 1) // 2, 1 << 30, (1 << 30) - 1, 1 << 380, (1 << 380) - 1,
             (1 << 381) % O.P, pow(2, -1, O.P), pow(3, -1, O.P), O.P - (1 << 30)]
    for a in edges + [rnd.randrange(O.P) for _ in range(60)]:
        for la in (0, 1, 3, 7):                     # a + la * p < 8p
            r = shim.shim_fq_inv_divsteps_agree(u32p(_fq(a)), la)
            assert 0 <= r <= 37, (a, la, r)
    hist = np.zeros(38, dtype=np.uint32)
    shim.shim_fq_inv_divsteps_bulk.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    assert shim.shim_fq_inv_divsteps_bulk(0x5EED, 200_000, 500, hist.ctypes.data) == 0
    assert int(hist.sum()) == 200_000 and int(hist[37:].sum()) < 200_000
    used = np.nonzero(hist)[0]
    assert used.max() <= 37
    print("divstep rounds histogram:", {int(k): int(hist[k]) for k in used})


def _pt(p):
    if p is None:
        return np.zeros(12, dtype=np.uint64)
    return np.array(O.fq_to_mont_limbs(p[0]) + O.fq_to_mont_limbs(p[1]), dtype=np.uint64)


def _unpt(a):
    a = [int(x) for x in a]
    if not any(a):
        return None
    return (O.fq_from_mont_limbs(a[:6]), O.fq_from_mont_limbs(a[6:]))


def test_group_law_all_exceptional_cases(shim):
    """identity operands, P + P, P + (-P), with and without a non-trivial Z on the accumulator"""
    rnd = random.Random(2)
    pts = [None] + [O.g1_mul(O.G1, k) for k in [1, 2, 3, 5, O.R - 1, O.R - 2, 12345678901234567890]]
    for a in pts:
        for b in pts:
            for neg in (0, 1):
                for zs in (None, _fq(rnd.randrange(1, O.P))):
                    o = np.zeros(12, dtype=np.uint64)
                    shim.shim_g1_madd(u32p(_pt(a)), u32p(_pt(b)), neg, None if zs is None else u32p(zs), u32p(o))
                    exp = O.g1_add(a, O.g1_neg(b) if neg else b)
                    assert _unpt(o) == exp
                    if not neg:
                        z2 = _fq(rnd.randrange(1, O.P))
                        shim.shim_g1_add(u32p(_pt(a)), u32p(_pt(b)), None if zs is None else u32p(zs), u32p(z2), u32p(o))
                        assert _unpt(o) == exp
    for k in [0, 1, 2, 3, 65535, 65536, 0xFFFFFFFF]:
        o = np.zeros(12, dtype=np.uint64)
        shim.shim_g1_mul_small(u32p(_pt(pts[3])), k, u32p(o))
        assert _unpt(o) == O.g1_mul(pts[3], k)


def test_group_law_long_dependent_chain(shim):
    """200 dependent mixed adds (every third negated) + 40 doublings + one full add: the lazy
    reduction bounds must hold along the whole chain"""
    n, ndbl = 200, 40
    pts = O.srs_from_secret_fast(3, n)
    arr = np.concatenate([_pt(p) for p in pts])
    o = np.zeros(12, dtype=np.uint64)
    shim.shim_g1_chain(u32p(arr), n, ndbl, u32p(o))
    k = sum((-1 if i % 3 == 1 else 1) * pow(3, i, O.R) for i in range(n)) % O.R
    assert _unpt(o) == O.g1_mul(O.G1, k * pow(2, ndbl + 1, O.R) % O.R)


def test_host_finish_on_64_bit_words_against_the_oracle(shim):
    """g1_host64.hpp: what ends every MSM on the host (sum of the reduction's bit planes, Horner over powers of two,
    affine normalisation) runs on 6 x 64-bit Montgomery words and reads the device's packed XYZZ form -- lazily reduced
    13 x 30-bit limbs in 12 words, non-trivial Z.  Points built by the limb code and read back by the 64-bit code must
    sum to what the oracle says, through the doubling branch, a cancellation, long chains, and to the identity."""
    rnd = random.Random(64)
    for n, ndbl in ((2, 0), (3, 1), (40, 19), (200, 40)):
        pts = O.srs_from_secret_fast(5, n)
        arr = np.concatenate([_pt(p) for p in pts])
        for zs in (None, _fq(rnd.randrange(1, O.P))):
            o = np.zeros(12, dtype=np.uint64)
            ok = shim.shim_h64_chain(u32p(arr), n, ndbl, None if zs is None else u32p(zs), u32p(o))
            k = (2 + sum(pow(5, i, O.R) for i in range(2, n))) * pow(2, ndbl, O.R) % O.R   # 2 p_0 + 0 + p_2 + ...
            assert ok == 1 and _unpt(o) == O.g1_mul(O.G1, k), (n, ndbl)
    # p_0 + p_0 with p_0 = the point of order dividing... a sum that IS the identity: G + G, then (2G) + (-2G) needs n = 2 only
    g2 = O.g1_mul(O.G1, 2)
    arr = np.concatenate([_pt(O.g1_neg(O.G1)), _pt(g2)])   # 2 * (-G) + (2G + (-2G)) = -2G: not the identity; identity next
    o = np.zeros(12, dtype=np.uint64)
    assert shim.shim_h64_chain(u32p(arr), 2, 0, None, u32p(o)) == 1 and _unpt(o) == O.g1_neg(g2)
    arr = np.concatenate([_pt(None), _pt(g2)])             # inf + inf + (2G - 2G)
    assert shim.shim_h64_chain(u32p(arr), 2, 3, None, u32p(o)) == 0


def test_library_loads_and_exports_every_declared_symbol(built):
    import typlonk_amd
    from typlonk_amd.capi import SYMBOLS

    lib = typlonk_amd.load_library()
    header = open(os.path.join(ROOT, "include", "typlonk.h")).read()
    declared = set(re.findall(r"\b(typlonk_[a-z0-9_]+)\s*\(", header))
    assert declared == set(SYMBOLS), declared ^ set(SYMBOLS)
    for s in SYMBOLS:
        assert getattr(lib, s) is not None
    assert b"gfx950" in lib.typlonk_version()
    assert lib.typlonk_strerror(-2) == b"MSM length exceeds SRS length"
    # every error code of the header has its own text
    codes = {int(v) for v in re.findall(r"#define TYPLONK_ERR_[A-Z_]+ \((-\d+)\)", header)}
    assert codes == set(range(-9, 0))
    texts = {lib.typlonk_strerror(c) for c in codes}
    assert len(texts) == len(codes) and b"unknown error" not in texts
    assert b"r(zeta)" in lib.typlonk_strerror(-8)


def test_no_cpu_fallback_without_device(built):
    """the product path must fail loudly when there is no GPU (this suite runs without one)"""
    import torch
    import typlonk_amd
    from typlonk_amd.capi import ERR_NO_DEVICE, TyplonkError

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(TyplonkError) as e:
        typlonk_amd.Context(0)
    assert e.value.code == ERR_NO_DEVICE


def test_g1_sum_host_fold(built):
    """deterministic fold of per-rank partial sums (host-only entry point)"""
    import typlonk_amd

    pts = [O.g1_mul(O.G1, k) for k in (3, 5, 7)] + [None, O.g1_mul(O.G1, O.R - 15)]
    xy, inf = g1_pack(pts)
    out, oi = typlonk_amd.g1_sum_host(xy[:3], inf[:3])
    assert g1_unpack_one(out, oi) == O.g1_mul(O.G1, 15)
    out, oi = typlonk_amd.g1_sum_host(xy[:4], inf[:4])
    assert g1_unpack_one(out, oi) == O.g1_mul(O.G1, 15)
    out, oi = typlonk_amd.g1_sum_host(xy, inf)
    assert oi == 1 and g1_unpack_one(out, oi) is None
    assert not out[:6].any() and [int(x) for x in out[6:]] == O.fq_to_mont_limbs(1)
    dup = np.stack([xy[0], xy[0]])
    out, oi = typlonk_amd.g1_sum_host(dup, None)
    assert g1_unpack_one(out, oi) == O.g1_mul(O.G1, 6)   # P + P goes through the doubling branch


def test_fold_of_all_gathered_records_for_three_ranks(built):
    """typlonk_g1_fold_records_host -- what the library runs on the output of its ncclAllGather (and what a host with its
    own exchange can call): records are rank-major, `count` per rank, 12 limbs + flag word.  Three ranks x four points,
    identities and cancelling points included; a flagged record (bits 32.. of the flag word = a rank's error code) makes
    the fold fail with TYPLONK_ERR_COMM and name the rank.  The multi-rank index arithmetic cannot run under RCCL on a
    one-GPU box (one rank per device), so it is pinned here."""
    from typlonk_amd.capi import ERR_COMM, TyplonkError, g1_fold_records_host

    ks = [[3, 0, 10, 1], [5, 0, O.R - 10, 2], [7, 9, 0, O.R - 3]]     # rank r, point i -> k * G (0 = identity)
    world, count = 3, 4
    rec = np.zeros((world, count, 13), dtype=np.uint64)
    for r in range(world):
        for i in range(count):
            limbs, f = O.g1_to_limbs(O.g1_mul(O.G1, ks[r][i]) if ks[r][i] else None)
            rec[r, i, :12] = limbs
            rec[r, i, 12] = f
    got = g1_fold_records_host(rec, world, count)
    want = [sum(ks[r][i] for r in range(world)) % O.R for i in range(count)]
    for (xy, inf), k in zip(got, want):
        assert g1_unpack_one(xy, inf) == (O.g1_mul(O.G1, k) if k else None)
    assert got[2][1] == 1 and got[3][1] == 1                           # 10 - 10 + 0 and 1 + 2 - 3: the identity
    bad = rec.copy()
    bad[1, 2, 12] = np.uint64(1) | (np.uint64(6) << np.uint64(32))     # rank 1 reports error code -6
    with pytest.raises(TyplonkError) as e:
        g1_fold_records_host(bad, world, count)
    assert e.value.code == ERR_COMM and "rank 1" in str(e.value)


def test_product_never_imports_oracle():
    """the oracle is test infrastructure: nothing under typlonk_amd/ or include/ may import, link or
    load it"""
    pat = re.compile(r"(import\s+oracle|from\s+oracle|liboracle|coracle|bls12_381\.py|oracle/)")
    for top in ("typlonk_amd", "include"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".py", ".hpp", ".hip", ".h", ".cpp")):
                    src = open(os.path.join(dirpath, f)).read()
                    assert not pat.search(src), f"{f} references the oracle"


def test_shipped_library_has_no_test_hooks(built):
    """fault injection lives in the test build only (tests/cpp/hooks, -DTYPLONK_TEST_HOOKS): the shipped library must not
    read any TYPLONK_TEST_* switch from the environment; the hooked build must"""
    shipped = open(os.path.join(ROOT, "typlonk_amd", "libtyplonk_hip.so"), "rb").read()
    assert b"TYPLONK_TEST" not in shipped
    hooked = open(os.path.join(ROOT, "tests", "cpp", "hooks", "libtyplonk_hip.so"), "rb").read()
    assert b"TYPLONK_TEST_COMM_FAIL_STAGING" in hooked


# ---- Fiat-Shamir transcript (tests/transcript_ref.py, the harness's separate Python statement; unverifiable against Rust here, see its docstring) -------
def test_transcript_building_blocks():
    import struct

    import transcript_ref as T

    # ChaCha block function against RFC 7539 section 2.3.2 (20 rounds; the reference's StdRng runs 12)
    key = list(struct.unpack("<8I", bytes(range(32))))
    out = T.chacha_block(key, 0, rounds=20, state_tail=[1, 0x09000000, 0x4A000000, 0])
    assert out == [0xE4E7F110, 0x15593BD1, 0x1FDD0F50, 0xC47120A3, 0xC7F4D1C7, 0x0368C033, 0x9AAA2204, 0x4E6CD4C3,
                   0x466482D2, 0x09AA9F07, 0x05D7C214, 0xA2028BD9, 0xD19C12B5, 0xB94E16DE, 0xE883D0CB, 0x4E3C50A2]
    # serialize_unchecked: canonical little-endian x || y, infinity flag 0x40 on the last byte, identity = (0, 1)
    gx = 0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB
    gy = 0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1
    mont = lambda v: [(v * (1 << 384) % T.FQ_MODULUS >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(6)]   # noqa: E731
    b = T.serialize_unchecked_g1(mont(gx) + mont(gy), 0)
    assert b == gx.to_bytes(48, "little") + gy.to_bytes(48, "little")
    z = T.serialize_unchecked_g1([0] * 12, 1)
    assert z[:48] == bytes(48) and z[48] == 1 and z[-1] == 0x40 and z[49:95] == bytes(46)
    # challenges: deterministic, < r, different transcripts give different challenges, 4-limb C-ABI form
    a = T.challenge12([(mont(gx) + mont(gy), 0)] * 3)
    a2 = T.challenge12([(mont(gx) + mont(gy), 0)] * 3)
    c = T.challenge34([(mont(gx) + mont(gy), 0)] * 3 + [([0] * 12, 1)])
    val = lambda l: sum(int(x) << (64 * i) for i, x in enumerate(l))   # noqa: E731
    assert all((x == y).all() for x, y in zip(a, a2)) and len(a) == 2 and len(c) == 2
    assert all(val(x) < T.FR_MODULUS for x in a + c) and val(a[0]) != val(c[0]) and val(a[0]) != val(a[1])
    # seed expansion: 32 bytes, a function of the seed
    assert len(T.seed_from_u64(0)) == 32 and T.seed_from_u64(0) != T.seed_from_u64(1)


def test_native_transcript_equals_the_python_statement(built):
    """typlonk_transcript_challenges (csrc/transcript.hpp: Blake2b-512, PCG32 seed expansion, ChaCha12, Fr::rand,
    serialize_unchecked) against tests/transcript_ref.py (hashlib Blake2b + an independent ChaCha): two restatements
    of plonk/src/proof/challenges.rs:9-46 written separately must agree bit for bit -- 0..6 commitments (0, 96, ... 576
    bytes: below, at and across Blake2b's 128-byte blocks), the point at infinity included"""
    import random

    import transcript_ref as T
    from typlonk_amd.capi import transcript_challenges

    rnd = random.Random(77)
    pts = []
    for i in range(6):
        p = None if i == 3 else O.g1_mul(O.G1, rnd.randrange(1, O.R))
        limbs, f = O.g1_to_limbs(p)
        pts.append((np.array(limbs, dtype=np.uint64), f))
    for k in range(0, 7):
        for n in (1, 2, 5):
            a = transcript_challenges(pts[:k], n)
            b = T.ChallengeGenerator.with_digest(pts[:k]).generate_challenges(n)
            assert len(a) == len(b) == n and all((x == y).all() for x, y in zip(a, b)), (k, n)
            for x in a:   # a valid Montgomery residue: the limbs read as an integer are below r
                assert sum(int(v) << (64 * i) for i, v in enumerate(x)) < O.R


def test_transcript_generator_against_the_crates_published_vectors(built):
    """Known answers that come from OUTSIDE this repository, reproduced by both statements of the generator
    (tests/transcript_ref.py and csrc/transcript.hpp through the host shim):
      * ChaCha12, 256-bit zero key, zero counter/nonce: keystream block of draft-strombergson-chacha-test-vectors-01
        (TC1, 12 rounds) -- the block function at the round count rand 0.8's StdRng uses;
      * rand 0.8 `rngs::std::test_stdrng_construction`: StdRng::from_seed([1,0,0,0, 23,0,0,0, 200,1,0,0, 210,30,0,0,
        0...]).next_u64() == 10719222850664546238 -- pins the 64-bit block counter layout, the 12 rounds and the order
        in which two 32-bit words make a u64;
      * rand_chacha `test_chacha_construction` (ChaCha20Rng): seed words 0,0,1,0,2,0,3,0 -> next_u32() == 137206642.
    Not covered by any published vector known here: the PCG32 expansion of seed_from_u64 (only its constants are
    standard) and ark-ff's Fr::rand shaving -- those wait for tools/rust_vectors."""
    import ctypes
    import struct

    import transcript_ref as T

    tc1 = bytes.fromhex("9bf49a6a0755f953811fce125f2683d50429c3bb49e074147e0089a52eae155f"
                        "0564f879d27ae3c02ce82834acfa8c793a629f2ca0de6919610be82f411326be")
    assert b"".join(struct.pack("<I", w) for w in T.chacha_block([0] * 8, 0, rounds=12)) == tc1
    seed = bytes([1, 0, 0, 0, 23, 0, 0, 0, 200, 1, 0, 0, 210, 30, 0, 0] + [0] * 16)
    assert T.StdRng(seed).next_u64() == 10719222850664546238
    key20 = list(struct.unpack("<8I", bytes([0] * 8 + [1] + [0] * 7 + [2] + [0] * 7 + [3] + [0] * 7)))
    assert T.chacha_block(key20, 0, rounds=20)[0] == 137206642
    # the native generator
    shim = ctypes.CDLL(os.path.join(ROOT, "tests", "cpp", "libff_host_shim.so"))
    out = (ctypes.c_uint64 * 8)()
    shim.shim_stdrng_words((ctypes.c_uint32 * 8)(*[0] * 8), out, 8)
    assert b"".join(struct.pack("<Q", v) for v in out) == tc1
    shim.shim_stdrng_words((ctypes.c_uint32 * 8)(*struct.unpack("<8I", seed)), out, 1)
    assert out[0] == 10719222850664546238
    # the two statements agree on the seed expansion (no published vector): 8 seeds, all 8 key words
    for state in (0, 1, 2, 3, 4, 8, 16, (1 << 64) - 1):
        key = (ctypes.c_uint32 * 8)()
        shim.shim_seed_from_u64(ctypes.c_uint64(state), key)
        assert bytes(key) == T.seed_from_u64(state)


def test_public_header_is_plain_c99_and_cxx11(tmp_path):
    """include/typlonk.h is the drop-in boundary a Rust / C / C++ host binds: it must compile on its own
    as strict C99 and as C++11 -- no HIP, torch or C++-only constructs in the signatures"""
    import shutil
    import subprocess

    src = tmp_path / "h.c"
    src.write_text('#include "typlonk.h"\nint main(void) { return 0; }\n')
    inc = os.path.join(ROOT, "include")
    for cc, args in (("gcc", ["-std=c99", "-pedantic"]), ("g++", ["-std=c++11", "-x", "c++"])):
        if shutil.which(cc) is None:
            pytest.skip(cc + " not available")
        r = subprocess.run([cc, *args, "-Wall", "-Wextra", "-Werror", "-I", inc, "-fsyntax-only", str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_scale_table_reads_bench_lines(tmp_path):
    """tools/scale_table.py (arrival day of a multi-GPU box): measured speed-ups per mode next to the one-GPU projection, and a
    note when the exchange did not run over the library's own communicator"""
    import json
    import subprocess
    import sys

    d1 = {"n_gpus": 1, "ms_per_step": 2.6, "msm_batch": {"ms_per_msm": 2.4}, "prove_native_ms": 36.0, "rccl_world": 0}
    d8 = {"n_gpus": 8, "ms_per_step": 0.65, "msm_batch": {"ms_per_msm": 0.4}, "prove_sharded_native_ms": 10.0, "rccl_world": 8,
          "expected_from_1gpu": {"one_msm_plus_exchange_ms": 0.59, "batched_ms_per_msm": 0.417, "prove_on_shard_ms": 10.3,
                                 "speedup": {"one_msm": 4.4, "batched_msms": 5.9, "prove": 3.6}}}
    d2 = {"n_gpus": 2, "ms_per_step": 1.5, "msm_batch": {"ms_per_msm": 1.25}, "rccl_world": 0}
    paths = []
    for d in (d1, d8, d2):
        p = tmp_path / f"{d['n_gpus']}.json"
        p.write_text("log noise\n" + json.dumps(d) + "\n")
        paths.append(str(p))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scale_table.py"), *paths], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = {l.split()[0]: l for l in r.stdout.splitlines() if l[:3].strip().isdigit()}
    assert "4.00" in rows["8"] and "6.00" in rows["8"] and "3.60" in rows["8"] and "5.90" in rows["8"]    # measured and projected
    assert "1.73" in rows["2"] and "NOTE: N = [2]" in r.stdout


def test_bench_without_a_launcher_still_ends_with_one_contract_line(built):
    """`python bench.py --gpus 2` with no torch.distributed.run around it starts its own rank processes; without a GPU
    (this suite) the ranks fail loudly -- no CPU fallback -- and the parent still ends with ONE contract line that
    carries n_gpus = 2 and the error, and a non-zero exit code."""
    import json
    import subprocess
    import sys

    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_dist.py runs the real thing")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--log-n", "10", "--steps", "1",
                        "--warmup", "0"], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    out = [l for l in r.stdout.splitlines() if l.strip()]
    assert r.returncode != 0
    assert sum(l.startswith('{"metric"') for l in out) == 1 and out[-1].startswith('{"metric"')
    d = json.loads(out[-1])
    assert d["n_gpus"] == 2 and d["value"] is None and "No HIP GPUs" in d["error"]


def test_fold_of_eight_ranks_with_every_exceptional_column(built):
    """typlonk_g1_fold_records_host (the rank-order fold behind every *_sharded_* call: mixed additions of the ranks'
    affine records + ONE inversion for all points, round 5): nine points from eight ranks against the big-int oracle, with
    columns that hold identity records, the same point on two ranks (doubling), opposite points (the sum is the identity)
    and nothing but identities"""
    from helpers import g1_pack as pack
    from typlonk_amd.capi import g1_fold_records_host

    world, count = 8, 9
    pts = [O.g1_mul(O.G1, 1000 + 17 * i) for i in range(world * count)]
    pts[0] = None
    pts[count + 1] = pts[1]
    pts[2 * count + 2] = O.g1_neg(pts[2])
    for r in range(world):
        pts[r * count + 3] = None
    for r in (1, 3, 4, 5, 6, 7):
        pts[r * count + 2] = None                    # column 2: P on rank 0, -P on rank 2, identities elsewhere
    xy, inf = pack(pts)
    rec = np.zeros((world * count, 13), dtype=np.uint64)
    rec[:, :12] = xy
    rec[:, 12] = inf
    got = g1_fold_records_host(rec, world, count)
    for i in range(count):
        want = None
        for r in range(world):
            want = O.g1_add(want, pts[r * count + i])
        assert g1_unpack_one(*got[i]) == want, i
    assert got[3][1] == 1 and got[2][1] == 1        # all identities; P + (-P)


def test_missing_librccl_is_an_error_code_not_a_crash(built):
    """the loader of the RCCL exchange pointed at a library that does not exist (TYPLONK_RCCL_LIB): typlonk_comm_available
    says 0 and typlonk_comm_unique_id returns TYPLONK_ERR_COMM -- in a fresh process, because the loader resolves once.
    (Round 3 built the message from two dlerror() calls; the second returns NULL and the string constructor crashed.)"""
    import subprocess
    import sys

    code = (
        "import ctypes, sys; sys.path.insert(0, %r); import typlonk_amd\n"
        "lib = typlonk_amd.load_library()\n"
        "lib.typlonk_comm_available.restype = ctypes.c_int\n"
        "a = lib.typlonk_comm_available()\n"
        "buf = (ctypes.c_uint8 * 128)()\n"
        "rc = lib.typlonk_comm_unique_id(buf)\n"
        "print('RESULT', a, rc)\n" % ROOT)
    env = dict(os.environ, TYPLONK_RCCL_LIB="/nonexistent/librccl-not-here.so")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-1500:]
    assert "RESULT 0 -9" in r.stdout, r.stdout + r.stderr[-500:]


def test_rust_ffi_mirror_is_generated_from_the_header_and_complete(built):
    """integration/rust/kzg_hip/src/ffi.rs is what tools/gen_rust_ffi.py makes of include/typlonk.h (not stale), and every
    symbol the library exports appears in it as a `pub fn` -- the Rust side binds the whole boundary, not a sample."""
    import subprocess
    import sys

    from typlonk_amd.capi import SYMBOLS

    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ffi = open(os.path.join(ROOT, "integration", "rust", "kzg_hip", "src", "ffi.rs")).read()
    bound = set(re.findall(r"pub fn (typlonk_[a-z0-9_]+)\(", ffi))
    assert bound == set(SYMBOLS), bound ^ set(SYMBOLS)
    # the structs that cross the boundary by value keep the header's field order
    assert re.search(r"pub struct TyplonkProof \{\s*pub commit_xy: \[\[u64; 12\]; 3\],\s*pub commit_inf: \[u8; 3\],\s*pub z_xy", ffi)
    # and the safe layer only calls functions the mirror declares
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "kzg_hip", "src", "lib.rs")).read()
    assert set(re.findall(r"ffi::(typlonk_[a-z0-9_]+)\(", lib_rs)) <= bound


def test_rust_patches_apply_to_the_reference(tmp_path):
    """the two patches under integration/rust/patches apply cleanly to the reference's kzg / plonk crates.  The reference
    tree is pinned by tests/golden/patch_preimages.json (tests/golden/gen_patch_preimages.py: per touched file its git blob
    id and line count, per hunk the SHA-256 of the reference's lines there): every patch names that blob as its pre-image,
    every hunk's context and removed lines hash to the reference's lines at the hunk's position, and `git apply --check`
    accepts each patch against files of the reference's length that hold exactly those lines there."""
    import hashlib
    import subprocess

    from helpers import load_golden, patch_preimages

    pinned = load_golden("patch_preimages.json")
    for p in ("0001-kzg-msm-on-hip.patch", "0002-plonk-prove-on-hip.patch"):
        patch = os.path.join(ROOT, "integration", "rust", "patches", p)
        files = patch_preimages(patch)
        assert set(files) == set(pinned[p]), p
        tree = tmp_path / p
        for path, d in files.items():
            ref = pinned[p][path]
            assert ref["blob"].startswith(d["blob"]), f"{p}: {path} was cut against blob {d['blob']}, the reference holds {ref['blob']}"
            assert [(h["start"], h["length"]) for h in ref["hunks"]] == [(s, n) for s, n, _ in d["hunks"]], f"{p}: {path}"
            body = [f"@@ line {i + 1} of the reference's {path} @@" for i in range(ref["lines"])]
            for (start, length, lines), h in zip(d["hunks"], ref["hunks"]):
                assert len(lines) == length, f"{p}: {path} hunk at {start}"
                assert hashlib.sha256("".join(l + "\n" for l in lines).encode("utf-8")).hexdigest() == h["sha256"], \
                    f"{p}: {path} hunk at line {start} does not match the reference"
                body[start - 1:start - 1 + length] = lines
            (tree / path).parent.mkdir(parents=True, exist_ok=True)
            (tree / path).write_text("".join(l + "\n" for l in body), encoding="utf-8")
        subprocess.run(["git", "init", "-q", "."], cwd=tree, check=True)
        r = subprocess.run(["git", "apply", "--check", patch], cwd=tree, capture_output=True, text=True)
        assert r.returncode == 0, p + ": " + r.stderr
