"""The accumulation loops' mixed addition (g1_madd_acc / g1_acc_finish, csrc/g1.hpp: the sum's identity and sign bits travel
beside the point) inside whole MSMs, against big integers, at the smallest shapes that reach each kernel that uses it:
  2^10 terms, plain SRS        c = 10, 2 entries per bucket: msm_accum_kernel, one thread per bucket
  2^14 terms, c = 15 tables    17 entries per bucket, 4 and 2 lanes per bucket: msm_accum_ml_kernel; with 2^12 equal scalars
                               on top, whose buckets pass the cap: msm_heavy_kernel
  2^16 terms, c = 17 tables    15 entries per bucket, 2 lanes and 1
  2^13 terms in two chunks     (TYPLONK_MSM_CHUNKS=2: 4096 terms each, the smallest the plan cuts) a bucket continues from storage
Every SRS is [s^i]G from the device with a few bases replaced by small multiples of G and by identities, and the scalars of
those terms are chosen so that their first window's digit puts them into one bucket, the pattern of
test_equal_buckets_in_two_representations_side_by_side (bases G, G, 2G, 5G with scalars d, d, d + 1, d + 2, d = 129):
  * equal points (the doubling path) as the 2nd and 3rd entry of a bucket, of either sign: a scalar 2^c - d has the digit -d;
  * opposite points (G with d and with 2^c - d), alone in a bucket and with a third entry after them;
  * -G, -G, 2G: a doubling whose result the next entry cancels;
  * identities among them.
The expected point is (sum of scalar_i * multiple_i mod r) G, computed with Python integers (oracle/bls12_381.py)."""
import numpy as np
import pytest

from helpers import O, fr_pack, g1_pack, g1_unpack_one

pytestmark = pytest.mark.gpu

SECRET = 0x6D6164645F616363


def special_terms(c):
    """[(multiple of G or None for an identity base, scalar)]: groups that meet in one bucket of the first window"""
    neg = lambda d: (1 << c) - d     # noqa: E731 -- first digit -d, and a carry of 1 into the second window
    return [
        (1, 129), (1, 129), (2, 130), (5, 131),           # G + G beside a loaded 2G
        (1, 300), (1, 300), (2, 300),                     # a doubling as the 2nd entry, or as the 2nd and the 3rd
        (1, 77), (1, neg(77)), (5, 77),                   # G - G, in any order with 5G
        (3, 200), (3, neg(200)),                          # a bucket that ends as the identity
        (1, neg(50)), (1, neg(50)), (2, 50),              # -G - G = -2G, then + 2G
        (7, neg(61)), (7, neg(61)),                       # a doubling of a negated point that stays
        (None, 300), (None, 77), (None, 12345),           # identities, two of them in the buckets above
        (4, 91), (None, 91), (4, 91), (4, neg(91)),       # 4G, identity, 4G, -4G
        (6, 1),                                           # a bucket of one entry
    ]


def build_case(ctx, m, c):
    """an m-point SRS with the special bases spread over it, scalars, and the multiples the expectation needs"""
    rng = np.random.default_rng(m + c)
    sid0 = ctx.srs_generate(np.array(O.fr_to_mont_limbs(SECRET), dtype=np.uint64), m)
    xy, inf = ctx.srs_download(sid0)
    ctx.srs_free(sid0)
    xy, inf = np.ascontiguousarray(xy).copy(), np.ascontiguousarray(inf).copy()
    mult, acc = [], 1
    for _ in range(m):
        mult.append(acc)
        acc = acc * SECRET % O.R
    vals = [int.from_bytes(rng.bytes(32), "little") % O.R for _ in range(m)]
    terms = special_terms(c)
    # in order, at equal distances over the whole vector (so that both halves of a two-chunk run hold some of each group)
    where = [(j * m) // len(terms) + (j % 3) for j in range(len(terms))]
    assert len(set(where)) == len(terms) and max(where) < m
    pts = [None if b is None else O.g1_mul(O.G1, b) for b, _ in terms]
    sxy, sinf = g1_pack(pts)
    for i, (b, k), pxy, pinf in zip(where, terms, sxy, sinf):
        xy[i], inf[i] = pxy, pinf
        mult[i] = b or 0
        vals[i] = k
    return xy, inf, mult, vals


def expected(mult, vals):
    return O.g1_mul(O.G1, sum(k * b for k, b in zip(vals, mult)) % O.R)


def check(ctx, sid, mult, vals):
    out, oinf = ctx.msm(sid, fr_pack(vals))
    assert g1_unpack_one(out, oinf) == expected(mult, vals)


def test_plain_srs_2_10_terms_one_thread_per_bucket(ctx):
    xy, inf, mult, vals = build_case(ctx, 1 << 10, 10)
    sid = ctx.srs_load(xy, inf)
    check(ctx, sid, mult, vals)
    ctx.srs_free(sid)


def test_tables_c15_2_14_terms_multi_lane_and_a_heavy_bucket(ctx):
    """the multi-lane kernel; then 2^12 of the terms share one scalar, so the buckets of its digits pass the cap and go to the
    heavy-bucket tasks, 64 lanes striding over each: among those terms' bases 1024 copies of G, 256 of -G (equal and opposite
    points meet in a lane) and 128 identities"""
    m, c = 1 << 14, 15
    xy, inf, mult, vals = build_case(ctx, m, c)
    sid = ctx.srs_load(xy, inf)
    ctx.srs_precompute(sid, c)
    check(ctx, sid, mult, vals)
    ctx.srs_free(sid)
    # the heavy bucket: terms 8192 .. 12287 take one scalar
    rep = O.random_frs(0xACC, 1)[0]
    g = O.g1_mul(O.G1, 1)
    gxy, ginf = g1_pack([g, O.g1_neg(g), None])
    for i in range(8192, 8192 + 4096):
        vals[i] = rep
        r = i % 16
        if r < 4:
            xy[i], inf[i], mult[i] = gxy[0], ginf[0], 1              # 1024 copies of G ...
        elif r == 4:
            xy[i], inf[i], mult[i] = gxy[1], ginf[1], O.R - 1        # ... 256 of -G
        elif r == 5 and i % 32 == 5:
            xy[i], inf[i], mult[i] = gxy[2], ginf[2], 0              # ... 128 identities
    sid = ctx.srs_load(xy, inf)
    ctx.srs_precompute(sid, c)
    check(ctx, sid, mult, vals)
    ctx.srs_free(sid)


def test_tables_c17_2_16_terms(ctx):
    m, c = 1 << 16, 17
    xy, inf, mult, vals = build_case(ctx, m, c)
    sid = ctx.srs_load(xy, inf)
    ctx.srs_precompute(sid, c)
    check(ctx, sid, mult, vals)
    ctx.srs_free(sid)


def test_two_chunks_continue_a_bucket_from_storage_after_an_odd_number_of_additions(built, monkeypatch):
    """2^13 terms of a plain SRS (c = 13) in two chunks of 4096.  A bucket's first chunk leaves it after 1 or 3 additions --
    the sign bit set, so the stored Y is the negated one -- and the second chunk loads it and adds an equal point (G stored,
    + G), an opposite one (3G stored after three additions, - 3G, then more), and ordinary ones."""
    import typlonk_amd

    m, c = 1 << 13, 13
    neg = lambda d: (1 << c) - d     # noqa: E731
    monkeypatch.setenv("TYPLONK_MSM_CHUNKS", "2")
    c2 = typlonk_amd.Context(0)
    try:
        xy, inf, mult, vals = build_case(c2, m, c)
        first = [(1, 1500), (1, 1600), (1, 1600), (1, 1600), (2, 1700), (9, 1700), (8, neg(1700)), (5, 1800), (None, 1800), (5, 1900)]
        second = [(1, 1500), (3, neg(1600)), (4, 1600), (3, 1700), (6, neg(1700)), (5, neg(1800)), (7, 1800), (10, 1900), (None, 1500)]
        gxy, ginf = g1_pack([None if b is None else O.g1_mul(O.G1, b) for b, _ in first + second])
        slots = [100 + 7 * j for j in range(len(first))] + [4096 + 100 + 7 * j for j in range(len(second))]
        taken = {i for i, b in enumerate(mult) if b < 16}              # build_case's own special bases
        assert not taken & set(slots)
        for i, (b, k), pxy, pinf in zip(slots, first + second, gxy, ginf):
            xy[i], inf[i], mult[i], vals[i] = pxy, pinf, b or 0, k
        sid = c2.srs_load(xy, inf)
        check(c2, sid, mult, vals)
        c2.srs_free(sid)
    finally:
        c2.close()
