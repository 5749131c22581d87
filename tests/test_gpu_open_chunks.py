"""typlonk_srs_open_chunks_table / typlonk_open_chunks_* on the GPU: a polynomial's multi-proofs on every coset of its domain
against big integers (tests/open_chunks_ref.py) word for word and flag for flag over all r proofs and n evaluations, against
typlonk_open_all_* at one point per coset, through the verifier's pairing equation, in batches, on the degenerate polynomials and
secrets that drive the zero scalars, the identities and the exceptional additions through every pass, on arbitrary points, the
table's lifetime, the refusals and the C++ mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import open_chunks_ref as FK
from helpers import O, fr_pack, fr_unpack, g1_pack, g1_unpack_one

pytestmark = pytest.mark.gpu

R = O.R
ORDER3 = (0, 2)   # on y^2 = x^3 + 4, of order 3: not a multiple of G


def _limbs(v):
    return np.array(O.fr_to_mont_limbs(v % R), dtype=np.uint64)


def _rand(rng, k):
    return [int.from_bytes(rng.bytes(32), "little") % R for _ in range(k)]


def _same(got, want):
    return (got[0] == want[0]).all() and (got[1] == want[1]).all()


def _bad(got, want):
    return [i for i in range(len(want[1])) if not (got[0][i] == want[0][i]).all() or got[1][i] != want[1][i]]


def _open_both_ways(ctx, tab, fs, log_n, log_l):
    """open_chunks over host coefficients and over device buffers (at a non-zero offset) must agree word for word; returns the
    former"""
    n, l, r = FK.shape(log_n, log_l)
    m = len(fs[0])
    host = ctx.open_chunks(tab, [fr_pack(f) for f in fs])
    bufs = [ctx.alloc(m + 3) for _ in fs]
    try:
        for b, f in zip(bufs, fs):
            b.upload(fr_pack([5, 6, 7] + list(f)))
        dev = ctx.open_chunks(tab, bufs, m, offsets=[3] * len(fs))
    finally:
        for b in bufs:
            b.free()
    assert (host[0] == dev[0]).all() and (host[1] == dev[1]).all() and (host[2] == dev[2]).all()
    assert host[0].shape == (len(fs), r, 12) and host[1].shape == (len(fs), r) and host[2].shape == (len(fs), r, l, 4)
    return host


def _check(ctx, tab, f, scalars, log_n, log_l):
    """every proof is [scalars[k]] G and every evaluation f(w^(k + r t)) at k l + t, over all r proofs and n evaluations"""
    xy, inf, ev = _open_both_ways(ctx, tab, [f], log_n, log_l)
    want = g1_pack(FK.points(scalars))
    assert not _bad((xy[0], inf[0]), want), _bad((xy[0], inf[0]), want)
    assert (ev[0].reshape(-1, 4) == fr_pack(FK.evaluations(f, log_n, log_l))).all()
    return xy[0], inf[0], ev[0]


# ---- 1. the closed form, a known full-width s -------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,log_l", [(a, b) for a in range(1, 8) for b in range(a)])
def test_closed_form(ctx, log_n, log_l):
    """[q_k(s)] G for every coset and f at every point, by division by X^l - a_k.  Odd log_n: the source holds exactly the n - l
    points that are read."""
    n, l, r = FK.shape(log_n, log_l)
    rng = np.random.default_rng(0xC20 + 16 * log_n + log_l)
    s = _rand(rng, 1)[0]
    f = _rand(rng, n)
    length = n - l if log_n & 1 else n + 3
    sid = ctx.srs_generate(_limbs(s), length)
    tab = None
    try:
        before = ctx.srs_download(sid)
        tab = ctx.srs_open_chunks_table(sid, log_n, log_l)
        assert ctx.srs_len(tab) == 2 * n
        _check(ctx, tab, f, FK.openings_known_secret(f, s, log_n, log_l), log_n, log_l)
        assert ctx.srs_len(sid) == length and _same(ctx.srs_download(sid), before)   # the source entry is untouched
    finally:
        ctx.srs_free(sid)
        if tab is not None:
            ctx.srs_free(tab)


def test_the_table_is_the_reference_table(ctx):
    """the table's records in the layout the header states: y^(j)_i at record j 2r + i"""
    log_n, log_l = 4, 2
    n, l, r = FK.shape(log_n, log_l)
    ks = _rand(np.random.default_rng(0x7AB), n - l)
    sid = ctx.srs_load(*g1_pack(FK.points(ks)))
    tab = ctx.srs_open_chunks_table(sid, log_n, log_l)
    try:
        assert _same(ctx.srs_download(tab), g1_pack(FK.points(FK.table(ks, log_n, log_l))))
    finally:
        ctx.srs_free(sid)
        ctx.srs_free(tab)


# ---- 2. l = 1 against the code that exists ----------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [1, 4, 7])
def test_one_point_per_coset_is_open_all(ctx, log_n):
    """typlonk_open_all_* and typlonk_srs_open_all_table are now entry points over the code of typlonk_open_chunks_* at
    log_l = 0, so both sides of every comparison below run the same kernels: what it still checks is the entry points' wrapping
    (one polynomial, one offset, count = 1) and the refusal open_all alone makes.  The independent check of the one-point path
    is tests/test_gpu_open_all.py, against the Python oracle."""
    from typlonk_amd.capi import ERR_INVALID_ARG, TyplonkError

    n = 1 << log_n
    rng = np.random.default_rng(0x1A1 + log_n)
    s = _rand(rng, 1)[0]
    f = _rand(rng, n - 1 if log_n > 1 else n)
    sid = ctx.srs_generate(_limbs(s), n + 3)
    old = ctx.srs_open_all_table(sid, log_n)
    new = ctx.srs_open_chunks_table(sid, log_n, 0)
    wide = ctx.srs_open_chunks_table(sid, log_n, 2) if log_n > 2 else None
    try:
        assert _same(ctx.srs_download(new), ctx.srs_download(old))               # the same 2n records, word for word
        want = ctx.open_all(old, fr_pack(f))
        for tab in (old, new):                                                   # open_chunks takes a table of either constructor
            xy, inf, ev = ctx.open_chunks(tab, [fr_pack(f)])
            assert (xy[0] == want[0]).all() and (inf[0] == want[1]).all() and (ev[0, :, 0] == want[2]).all()
        got = ctx.open_all(new, fr_pack(f))                                      # and open_all the log_l = 0 table of the new one
        assert all((a == b).all() for a, b in zip(got, want))
        if wide is not None:
            with pytest.raises(TyplonkError) as e:
                ctx.open_all(wide, fr_pack(f))
            assert e.value.code == ERR_INVALID_ARG
    finally:
        for t in (sid, old, new, wide):
            if t is not None:
                ctx.srs_free(t)


# ---- 3. through pairings ----------------------------------------------------------------------------------------------------
def test_device_multiproofs_verify(ctx):
    """log_n = 4, l = 4: for every coset k, e(C - [I_k(s)]G + [a_k] pi_k, G2) = e(pi_k, [s^l]G2), with C and [I_k(s)]G device
    MSMs and I_k interpolated from the device's evaluations on the coset; a proof paired with its neighbour's coset fails"""
    from oracle import pairing as OP

    log_n, log_l = 4, 2
    n, l, r = FK.shape(log_n, log_l)
    rng = np.random.default_rng(0x7E53)
    s = _rand(rng, 1)[0]
    f = _rand(rng, n)
    sid = ctx.srs_generate(_limbs(s), n + 3)
    tab = ctx.srs_open_chunks_table(sid, log_n, log_l)
    try:
        xy, inf, ev = ctx.open_chunks(tab, [fr_pack(f)])
        commitment = g1_unpack_one(*ctx.msm(sid, fr_pack(f)))
        remainders = []
        for k in range(r):
            i_k = FK.interpolant(fr_unpack(ev[0, k]), k, log_n, log_l)
            remainders.append(g1_unpack_one(*ctx.msm(sid, fr_pack(i_k))))
    finally:
        ctx.srs_free(sid)
        ctx.srs_free(tab)
    g2, g2sl = OP.srs_g2(pow(s, l, R))
    proofs = [g1_unpack_one(xy[0, k], inf[0, k]) for k in range(r)]
    a = FK.coset_constants(log_n, log_l)

    def holds(k, proof):
        lhs = O.g1_add(O.g1_add(commitment, O.g1_neg(remainders[k])), O.g1_mul(proof, a[k]))
        return OP.pairing(lhs, g2) == OP.pairing(proof, g2sl)

    for k in range(r):
        assert holds(k, proofs[k]), k
    assert not holds(1, proofs[2])


# ---- 4. batches -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,log_l", [(6, 2), (5, 3)])
@pytest.mark.parametrize("count", [2, 3, 5])
def test_batches(ctx, log_n, log_l, count):
    """each polynomial of a batch equals its own count = 1 call, at m = n and at one m < n; the same polynomial twice in one batch,
    as host coefficients and as one device buffer named twice"""
    n, l, r = FK.shape(log_n, log_l)
    rng = np.random.default_rng(0xBA7 + 64 * log_n + count)
    s = _rand(rng, 1)[0]
    sid = ctx.srs_generate(_limbs(s), n + 3)
    tab = ctx.srs_open_chunks_table(sid, log_n, log_l)
    try:
        for m in (n, n // 2 + 3):
            fs = [_rand(rng, m) for _ in range(count)]
            fs[-1] = fs[0]                                                         # the same polynomial twice
            xy, inf, ev = _open_both_ways(ctx, tab, fs, log_n, log_l)
            for p, f in enumerate(fs):
                one = ctx.open_chunks(tab, [fr_pack(f)])
                assert (xy[p] == one[0][0]).all() and (inf[p] == one[1][0]).all() and (ev[p] == one[2][0]).all(), p
            assert not _bad((xy[1], inf[1]), g1_pack(FK.points(FK.openings_known_secret(fs[1], s, log_n, log_l))))
        buf = ctx.alloc(n)
        try:
            buf.upload(fr_pack(fs[0] + [0] * (n - len(fs[0]))))
            twice = ctx.open_chunks(tab, [buf] * count, len(fs[0]))
            assert all((twice[0][p] == xy[0]).all() and (twice[1][p] == inf[0]).all() and (twice[2][p] == ev[0]).all() for p in range(count))
        finally:
            buf.free()
    finally:
        ctx.srs_free(sid)
        ctx.srs_free(tab)


# ---- 5. degenerate inputs ---------------------------------------------------------------------------------------------------
DEGENERATE = [(4, 1), (6, 3), (6, 5)]


@pytest.mark.parametrize("log_n,log_l", DEGENERATE)
def test_degenerate_polynomials(ctx, log_n, log_l):
    n, l, r = FK.shape(log_n, log_l)
    rng = np.random.default_rng(0xDE7 + 16 * log_n + log_l)
    s = _rand(rng, 1)[0]
    sid = ctx.srs_generate(_limbs(s), n + 3)
    tab = ctx.srs_open_chunks_table(sid, log_n, log_l)
    try:
        # f = 0: every scalar of the pointwise pass is 0, every proof an identity
        xy, inf, ev = _check(ctx, tab, [0] * n, [0] * r, log_n, log_l)
        assert inf.all() and not ev.any()                     # (_check: the records are the identity's, word for word)
        # deg f < l: f is its own remainder on every coset, every proof an identity
        low = _rand(rng, l)
        for f in (low + [0] * (n - l), low, low[:1]):
            xy, inf, ev = _check(ctx, tab, f, [0] * r, log_n, log_l)
            assert inf.all()
        # f = X^(n-1): one nonzero coefficient, in c^(l-1)_0
        f = [0] * (n - 1) + [1]
        _check(ctx, tab, f, FK.openings_known_secret(f, s, log_n, log_l), log_n, log_l)
        # the zero padding
        for m in sorted({1, l, l + 1, n // 2 + 1, n - 1}):
            f = _rand(rng, m)
            _check(ctx, tab, f, FK.openings_known_secret(f, s, log_n, log_l), log_n, log_l)
    finally:
        ctx.srs_free(sid)
        ctx.srs_free(tab)


@pytest.mark.parametrize("log_n,log_l", DEGENERATE)
@pytest.mark.parametrize("secret", ["one", "zero", "in_domain"])
def test_degenerate_secrets(ctx, log_n, log_l, secret):
    """s = 1: every point is G, so the terms of a sum share one base and P = +-[w]Q in every stage.  s = 0: G, then identities.
    s = w^5: s^l = a_5 (mod r cosets), where a closed quotient would be 0/0; the reference divides."""
    n, l, r = FK.shape(log_n, log_l)
    s = {"one": 1, "zero": 0, "in_domain": pow(O.domain_root(log_n), 5, R)}[secret]
    f = _rand(np.random.default_rng(0x5ED + 16 * log_n + log_l), n)
    sid = ctx.srs_generate(_limbs(s), n + 3)
    tab = ctx.srs_open_chunks_table(sid, log_n, log_l)
    try:
        _check(ctx, tab, f, FK.openings_known_secret(f, s, log_n, log_l), log_n, log_l)
    finally:
        ctx.srs_free(sid)
        ctx.srs_free(tab)


@pytest.mark.parametrize("log_n,log_l", DEGENERATE)
def test_arbitrary_points(ctx, log_n, log_l):
    """[k_m] G for random k_m with an identity record and a repeated point, against the double sum.  Then the order-3 point (0, 2)
    in one record: no scalar of Fr acts on it, but every step is a homomorphism, so each proof moves by an element of the group
    (0, 2) generates."""
    n, l, r = FK.shape(log_n, log_l)
    rng = np.random.default_rng(0xA4D + 16 * log_n + log_l)
    ks = _rand(rng, n - l)
    ks[3] = 0            # the identity record
    ks[6] = ks[1]        # a repeated point
    f = _rand(rng, n)
    pts = [O.g1_mul(O.G1, k) for k in ks]
    assert pts[3] is None
    sid = ctx.srs_load(*g1_pack(pts))
    tab = ctx.srs_open_chunks_table(sid, log_n, log_l)
    try:
        _check(ctx, tab, f, FK.openings_of_point_scalars(f, ks, log_n, log_l), log_n, log_l)
    finally:
        ctx.srs_free(sid)
        ctx.srs_free(tab)
    ks[5] = 0
    pts[5] = ORDER3
    base = FK.points(FK.openings_of_point_scalars(f, ks, log_n, log_l))
    sid = ctx.srs_load(*g1_pack(pts))
    tab = ctx.srs_open_chunks_table(sid, log_n, log_l)
    try:
        xy, inf, ev = ctx.open_chunks(tab, [fr_pack(f)])
        assert (ev[0].reshape(-1, 4) == fr_pack(FK.evaluations(f, log_n, log_l))).all()
        orbit = [None, ORDER3, O.g1_neg(ORDER3)]
        for k in range(r):
            p = O.g1_from_limbs([int(v) for v in xy[0, k]], int(inf[0, k]))
            assert O.g1_add(p, O.g1_neg(base[k])) in orbit, k
    finally:
        ctx.srs_free(sid)
        ctx.srs_free(tab)


# ---- 6. lifetime and refusals -----------------------------------------------------------------------------------------------
def test_table_lifetime(ctx):
    """two polynomials on one table; the table outlives its source entry; srs_len = 2n; a freed table id is refused"""
    from typlonk_amd.capi import ERR_INVALID_ARG, TyplonkError

    log_n, log_l = 5, 2
    n, l, r = FK.shape(log_n, log_l)
    rng = np.random.default_rng(0x11FF)
    s = _rand(rng, 1)[0]
    f, g = _rand(rng, n), _rand(rng, n - 3)
    sid = ctx.srs_generate(_limbs(s), n + 3)
    tab = ctx.srs_open_chunks_table(sid, log_n, log_l)
    try:
        _check(ctx, tab, f, FK.openings_known_secret(f, s, log_n, log_l), log_n, log_l)
        ctx.srs_free(sid)
        sid = None
        assert ctx.srs_len(tab) == 2 * n
        _check(ctx, tab, g, FK.openings_known_secret(g, s, log_n, log_l), log_n, log_l)
        xy, inf = ctx.open_chunks(tab, [fr_pack(f)], evals=False)              # evals = NULL
        assert not _bad((xy[0], inf[0]), g1_pack(FK.points(FK.openings_known_secret(f, s, log_n, log_l))))
    finally:
        if sid is not None:
            ctx.srs_free(sid)
        ctx.srs_free(tab)
    with pytest.raises(TyplonkError) as e:
        ctx.open_chunks(tab, [fr_pack(f)])
    assert e.value.code == ERR_INVALID_ARG


def test_refusals(ctx):
    """every refusal the header lists but TYPLONK_ERR_OOM (no allocation a test can afford is refused), with the outputs filled
    with a pattern beforehand and found unchanged"""
    from typlonk_amd.capi import ERR_DOMAIN, ERR_INVALID_ARG, ERR_LENGTH, ERR_RANGE, _u8p, _u64p

    lib = ctx.lib
    log_n, log_l = 4, 2
    n, l, r = FK.shape(log_n, log_l)
    s = 0x5EC2E7D00D52
    sid = ctx.srs_generate(_limbs(s), n + 3)
    tab = ctx.srs_open_chunks_table(sid, log_n, log_l)

    def table_refused(handle, src, lg_n, lg_l, with_id=True):
        new = C.c_uint32(0xABABABAB)
        rc = lib.typlonk_srs_open_chunks_table(handle, src, lg_n, lg_l, C.byref(new) if with_id else None)
        assert new.value == 0xABABABAB, "a refused call wrote to its output"
        return rc

    f = fr_pack(_rand(np.random.default_rng(0x4F0), n))
    buf = ctx.alloc(n)
    buf.upload(f)
    COUNT = 2

    def open_refused(handle, t, m, dev=True, polys=True, entry=True, xy=True, inf=True, offset=0, count=COUNT, offsets=True):
        # (sized for one point per coset, the most any table of this domain writes)
        oxy = np.full((COUNT, n, 12), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        oinf = np.full((COUNT, n), 0x5A, dtype=np.uint8)
        oev = np.full((COUNT, n, 4), 0xC3C3C3C3C3C3C3C3, dtype=np.uint64)
        a = (_u64p(oxy) if xy else None, _u8p(oinf) if inf else None, _u64p(oev))
        if dev:
            hs = (C.c_void_p * COUNT)(buf.handle, buf.handle if entry else None)
            offs = (C.c_size_t * COUNT)(0, offset)
            rc = lib.typlonk_open_chunks_dev(handle, t, hs if polys else None, offs if offsets else None, m, count, *a)
        else:
            ps = (C.c_void_p * COUNT)(f.ctypes.data, f.ctypes.data if entry else None)
            rc = lib.typlonk_open_chunks_host(handle, t, ps if polys else None, m, count, *a)
        assert (oxy == 0xA5A5A5A5A5A5A5A5).all() and (oinf == 0x5A).all() and (oev == 0xC3C3C3C3C3C3C3C3).all(), "a refused call wrote to its outputs"
        return rc

    try:
        # ---- the table
        for lg in (0, 25, 26, 64, 0xFFFFFFFF):
            assert table_refused(ctx.h, sid, lg, 0) == ERR_DOMAIN                            # log_n outside 1..24
        for lg_l in (log_n, log_n + 1, 0xFFFFFFFF):
            assert table_refused(ctx.h, sid, log_n, lg_l) == ERR_DOMAIN                      # log_l >= log_n
        assert b"log_l" in lib.typlonk_last_error(ctx.h)
        assert table_refused(None, sid, log_n, log_l) == ERR_INVALID_ARG                     # a null context
        assert table_refused(ctx.h, sid, log_n, log_l, with_id=False) == ERR_INVALID_ARG     # a null output id
        assert table_refused(ctx.h, 999999, log_n, log_l) == ERR_INVALID_ARG                 # an unknown id
        shard = ctx.srs_generate(_limbs(s), n + 3)
        ctx.srs_set_shard(shard, 0, 2 * n + 6)
        assert table_refused(ctx.h, shard, log_n, log_l) == ERR_INVALID_ARG                  # a shard
        ctx.srs_free(shard)
        assert table_refused(ctx.h, sid, 5, 2) == ERR_INVALID_ARG                            # 19 < 28 points
        short = ctx.srs_generate(_limbs(s), n - l - 1)
        assert table_refused(ctx.h, short, log_n, log_l) == ERR_INVALID_ARG                  # one point short of n - l
        ctx.srs_free(short)
        assert table_refused(ctx.h, tab, 2, 1) == ERR_INVALID_ARG                            # a table as the source
        assert b"table" in lib.typlonk_last_error(ctx.h)
        # ---- the openings, both forms
        for dev in (True, False):
            assert open_refused(None, tab, n, dev) == ERR_INVALID_ARG                        # a null context
            assert open_refused(ctx.h, tab, n, dev, polys=False) == ERR_INVALID_ARG          # null polys / coeffs
            assert open_refused(ctx.h, tab, n, dev, entry=False) == ERR_INVALID_ARG          # a null entry of polys / coeffs
            assert open_refused(ctx.h, tab, n, dev, xy=False) == ERR_INVALID_ARG             # null proofs_xy
            assert open_refused(ctx.h, tab, n, dev, inf=False) == ERR_INVALID_ARG            # null proofs_inf
            assert open_refused(ctx.h, 999999, n, dev) == ERR_INVALID_ARG                    # an unknown id
            assert open_refused(ctx.h, sid, n, dev) == ERR_INVALID_ARG                       # an SRS that is no table
            assert open_refused(ctx.h, tab, 0, dev) == ERR_LENGTH                            # m = 0
            assert open_refused(ctx.h, tab, n + 1, dev) == ERR_LENGTH                        # m > n
            assert open_refused(ctx.h, tab, n, dev, count=0) == ERR_LENGTH                   # count = 0
            assert open_refused(ctx.h, tab, n, dev, count=(1 << 25) // (2 * r) + 1) == ERR_LENGTH   # count * 2r > 2^25 records
        assert open_refused(ctx.h, tab, n, offset=1) == ERR_RANGE                            # past the end of the second buffer
        assert open_refused(ctx.h, tab, 1, offset=n + 1) == ERR_RANGE
        # nothing was created or changed, and a good call still succeeds -- with offsets = NULL too
        assert ctx.srs_len(sid) == n + 3 and ctx.srs_len(tab) == 2 * n
        xy, inf, ev = _check(ctx, tab, fr_unpack(f), FK.openings_known_secret(fr_unpack(f), s, log_n, log_l), log_n, log_l)
        oxy = np.zeros((COUNT, r, 12), dtype=np.uint64)
        oinf = np.zeros((COUNT, r), dtype=np.uint8)
        hs = (C.c_void_p * COUNT)(buf.handle, buf.handle)
        assert lib.typlonk_open_chunks_dev(ctx.h, tab, hs, None, n, COUNT, _u64p(oxy), _u8p(oinf), None) == 0
        assert all((oxy[p] == xy).all() and (oinf[p] == inf).all() for p in range(COUNT))
    finally:
        buf.free()
        ctx.srs_free(sid)
        ctx.srs_free(tab)


# ---- 7. the C++ mirror ------------------------------------------------------------------------------------------------------
def test_mirror_open_chunks(built):
    """tests/cpp/test_open_chunks_host: kzg::Srs::open_chunks_table / KzgScheme::open_chunks of the C++ mirror"""
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "test_open_chunks_host")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for t in ("open_chunks ok", "refusals ok"):
        assert t in r.stdout
