"""typlonk_srs_open_all_table / typlonk_open_all_* on the GPU: a polynomial's openings at every point of its domain against big
integers (tests/open_all_ref.py) word for word and flag for flag over all n outputs, against typlonk_open_dev + an MSM (existing,
oracle-tested code), through the restatement of the reference's verifier, the degenerate polynomials and secrets that drive the
zero scalars, the identities and the exceptional additions through every pass, arbitrary points, the table's lifetime, the
refusals and the C++ mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import open_all_ref as FK
from helpers import O, fr_pack, fr_unpack, g1_pack

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


def _open_both_ways(ctx, tab, f, log_n):
    """open_all over host coefficients and over a device buffer (at an offset) must agree word for word; returns the former"""
    host = ctx.open_all(tab, fr_pack(f))
    buf = ctx.alloc(len(f) + 3)
    try:
        buf.upload(fr_pack([5, 6, 7] + list(f)))
        dev = ctx.open_all(tab, buf, len(f), offset=3)
    finally:
        buf.free()
    assert (host[0] == dev[0]).all() and (host[1] == dev[1]).all() and (host[2] == dev[2]).all()
    assert host[0].shape == (1 << log_n, 12) and host[2].shape == (1 << log_n, 4)
    return host


def _check(ctx, tab, f, scalars, log_n):
    """every proof is [scalars[k]] G and every evaluation f(w^k), over all n outputs"""
    xy, inf, ev = _open_both_ways(ctx, tab, f, log_n)
    want = g1_pack(FK.points(scalars))
    assert not _bad((xy, inf), want), _bad((xy, inf), want)
    assert (ev == fr_pack(FK.evaluations(f, log_n))).all()
    return xy, inf, ev


# ---- 1. the closed form, a known full-width s -------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", range(1, 8))
def test_closed_form(ctx, log_n):
    """[q_k(s)] G and f(w^k) for every k.  2n = 64 at log_n = 5 is exactly one wavefront of the pointwise pass, below it the spare
    lanes shadow; log_n = 7 puts a stage's butterflies in two wavefronts and the pointwise pass in four.  Odd log_n: the source
    holds exactly the n - 1 points that are read."""
    n = 1 << log_n
    rng = np.random.default_rng(0xF20 + log_n)
    s = _rand(rng, 1)[0]
    f = _rand(rng, n)
    length = n - 1 if log_n & 1 else n + 3
    sid = ctx.srs_generate(_limbs(s), length)
    tab = None
    try:
        before = ctx.srs_download(sid)
        tab = ctx.srs_open_all_table(sid, log_n)
        assert ctx.srs_len(tab) == 2 * n
        _, _, ev = _check(ctx, tab, f, FK.openings_known_secret(f, s, log_n), log_n)
        assert (ev == ctx.ntt(fr_pack(f), log_n)).all()
        assert ctx.srs_len(sid) == length and _same(ctx.srs_download(sid), before)   # the source entry is untouched
    finally:
        ctx.srs_free(sid)
        if tab is not None:
            ctx.srs_free(tab)


# ---- 2. against the code that exists ----------------------------------------------------------------------------------------
def test_against_open_dev_and_msm(ctx):
    """proof k and evaluation k are typlonk_open_dev at z = w^k followed by the MSM of the quotient over the source entry"""
    log_n, n = 7, 128
    rng = np.random.default_rng(0x0DE7)
    s = _rand(rng, 1)[0]
    f = _rand(rng, n)
    sid = ctx.srs_generate(_limbs(s), n + 3)
    tab = ctx.srs_open_all_table(sid, log_n)
    poly, q = ctx.alloc(n), ctx.alloc(n)
    try:
        poly.upload(fr_pack(f))
        xy, inf, ev = ctx.open_all(tab, poly)
        w = O.domain_root(log_n)
        for k in (0, 1, n // 2, n - 1):
            y = ctx.open_dev(poly, n, _limbs(pow(w, k, R)), q)
            pxy, pinf = ctx.msm_dev(sid, q, 0, n - 1)
            assert (pxy == xy[k]).all() and pinf == inf[k], k
            assert (y == ev[k]).all(), k
    finally:
        poly.free()
        q.free()
        ctx.srs_free(sid)
        ctx.srs_free(tab)


# ---- 3. through the reference's verifier ------------------------------------------------------------------------------------
def test_device_openings_verify(ctx):
    """log_n = 3: all eight device openings pass KzgScheme::verify (oracle/pairing.py) against the device commitment"""
    from helpers import g1_unpack_one
    from oracle import pairing as OP

    log_n, n = 3, 8
    rng = np.random.default_rng(0x7E52)
    s = _rand(rng, 1)[0]
    f = _rand(rng, n)
    sid = ctx.srs_generate(_limbs(s), n + 3)
    tab = ctx.srs_open_all_table(sid, log_n)
    try:
        xy, inf, ev = ctx.open_all(tab, fr_pack(f))
        cxy, cinf = ctx.msm(sid, fr_pack(f))
    finally:
        ctx.srs_free(sid)
        ctx.srs_free(tab)
    commitment = g1_unpack_one(cxy, cinf)
    g2, g2s = OP.srs_g2(s)
    ys = fr_unpack(ev)
    w = O.domain_root(log_n)
    for k in range(n):
        assert OP.kzg_verify(commitment, (g1_unpack_one(xy[k], inf[k]), ys[k]), pow(w, k, R), g2, g2s), k


# ---- 4. degenerate polynomials ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [4, 6])
def test_degenerate_polynomials(ctx, log_n):
    n = 1 << log_n
    rng = np.random.default_rng(0xDE6 + log_n)
    s = _rand(rng, 1)[0]
    f0 = _rand(rng, 1)[0]
    sid = ctx.srs_generate(_limbs(s), n + 3)
    tab = ctx.srs_open_all_table(sid, log_n)
    try:
        # f = 0: every ladder has k = 0, every proof is an identity
        xy, inf, ev = _check(ctx, tab, [0] * n, [0] * n, log_n)
        assert inf.all() and not ev.any()                     # (_check: the records are the identity's, word for word)
        # f = f_0 only, as n coefficients and as one: identities, every evaluation f_0
        for f in ([f0] + [0] * (n - 1), [f0]):
            xy, inf, ev = _check(ctx, tab, f, [0] * n, log_n)
            assert inf.all() and (ev == fr_pack([f0] * n)).all()
        # f = X^(n-1): only c_0 is nonzero
        f = [0] * (n - 1) + [1]
        _check(ctx, tab, f, FK.openings_known_secret(f, s, log_n), log_n)
        # the zero padding
        for m in (n // 2 + 1, n - 1):
            f = _rand(rng, m)
            _check(ctx, tab, f, FK.openings_known_secret(f, s, log_n), log_n)
    finally:
        ctx.srs_free(sid)
        ctx.srs_free(tab)


# ---- 5. degenerate secrets --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [4, 7])
@pytest.mark.parametrize("secret", ["one", "zero", "in_domain"])
def test_degenerate_secrets(ctx, log_n, secret):
    """s = 1: every point is G, so P = +-[w]Q in every stage.  s = 0: G, then identities.  s = w^5: the closed quotient is 0/0 at
    k = 5, the reference divides."""
    n = 1 << log_n
    s = {"one": 1, "zero": 0, "in_domain": pow(O.domain_root(log_n), 5, R)}[secret]
    f = _rand(np.random.default_rng(0x5EC + log_n), n)
    sid = ctx.srs_generate(_limbs(s), n + 3)
    tab = ctx.srs_open_all_table(sid, log_n)
    try:
        if secret == "zero":
            assert _same(ctx.srs_download(sid), g1_pack([O.G1] + [None] * (n + 2)))
        _check(ctx, tab, f, FK.openings_known_secret(f, s, log_n), log_n)
    finally:
        ctx.srs_free(sid)
        ctx.srs_free(tab)


# ---- 6. arbitrary points ----------------------------------------------------------------------------------------------------
def test_arbitrary_points(ctx):
    """[k_m] G for random k_m at log_n = 6 with an identity record and a repeated point, against the double sum.  Then the order-3
    point (0, 2) in one record: no scalar of Fr acts on it, but every step is a homomorphism, so each proof moves by an element of
    the group (0, 2) generates (tests/test_gpu_srs_lagrange.py, the same property of the transform)."""
    log_n, n = 6, 64
    rng = np.random.default_rng(0xA4C)
    ks = _rand(rng, n + 3)
    ks[9] = 0            # the identity record
    ks[40] = ks[17]      # a repeated point
    f = _rand(rng, n)
    pts = [O.g1_mul(O.G1, k) for k in ks]
    assert pts[9] is None
    sid = ctx.srs_load(*g1_pack(pts))
    tab = ctx.srs_open_all_table(sid, log_n)
    try:
        _check(ctx, tab, f, FK.openings_of_point_scalars(f, ks, log_n), log_n)
    finally:
        ctx.srs_free(sid)
        ctx.srs_free(tab)
    ks[23] = 0
    pts[23] = ORDER3
    base = FK.points(FK.openings_of_point_scalars(f, ks, log_n))
    sid = ctx.srs_load(*g1_pack(pts))
    tab = ctx.srs_open_all_table(sid, log_n)
    try:
        xy, inf, ev = ctx.open_all(tab, fr_pack(f))
        assert (ev == fr_pack(FK.evaluations(f, log_n))).all()
        orbit = [None, ORDER3, O.g1_neg(ORDER3)]
        for i in range(n):
            p = O.g1_from_limbs([int(v) for v in xy[i]], int(inf[i]))
            assert O.g1_add(p, O.g1_neg(base[i])) in orbit, i
    finally:
        ctx.srs_free(sid)
        ctx.srs_free(tab)


# ---- 7. lifetime ------------------------------------------------------------------------------------------------------------
def test_table_lifetime(ctx):
    """two polynomials on one table; the table outlives its source entry; srs_len = 2n; a freed table id is refused"""
    from typlonk_amd.capi import ERR_INVALID_ARG, TyplonkError

    log_n, n = 5, 32
    rng = np.random.default_rng(0x11FE)
    s = _rand(rng, 1)[0]
    f, g = _rand(rng, n), _rand(rng, n - 3)
    sid = ctx.srs_generate(_limbs(s), n + 3)
    tab = ctx.srs_open_all_table(sid, log_n)
    try:
        _check(ctx, tab, f, FK.openings_known_secret(f, s, log_n), log_n)
        ctx.srs_free(sid)
        sid = None
        assert ctx.srs_len(tab) == 2 * n
        _check(ctx, tab, g, FK.openings_known_secret(g, s, log_n), log_n)
        xy, inf = ctx.open_all(tab, fr_pack(f), evals=False)                 # evals = NULL
        assert not _bad((xy, inf), g1_pack(FK.points(FK.openings_known_secret(f, s, log_n))))
    finally:
        if sid is not None:
            ctx.srs_free(sid)
        ctx.srs_free(tab)
    with pytest.raises(TyplonkError) as e:
        ctx.open_all(tab, fr_pack(f))
    assert e.value.code == ERR_INVALID_ARG


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    """every refusal the header lists but TYPLONK_ERR_OOM (no allocation a test can afford is refused), with the outputs filled
    with a pattern beforehand and found unchanged"""
    from typlonk_amd.capi import ERR_DOMAIN, ERR_INVALID_ARG, ERR_LENGTH, ERR_RANGE, _u8p, _u64p

    lib = ctx.lib
    log_n, n = 4, 16
    s = 0x5EC2E7D00D51
    sid = ctx.srs_generate(_limbs(s), n + 3)
    tab = ctx.srs_open_all_table(sid, log_n)

    def table_refused(handle, src, lg, with_id=True):
        new = C.c_uint32(0xABABABAB)
        rc = lib.typlonk_srs_open_all_table(handle, src, lg, C.byref(new) if with_id else None)
        assert new.value == 0xABABABAB, "a refused call wrote to its output"
        return rc

    f = fr_pack(_rand(np.random.default_rng(0x4EF), n))
    buf = ctx.alloc(n)
    buf.upload(f)

    def open_refused(handle, t, m, dev=True, poly=True, xy=True, inf=True, offset=0):
        oxy = np.full((n, 12), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        oinf = np.full(n, 0x5A, dtype=np.uint8)
        oev = np.full((n, 4), 0xC3C3C3C3C3C3C3C3, dtype=np.uint64)
        a = (_u64p(oxy) if xy else None, _u8p(oinf) if inf else None, _u64p(oev))
        if dev:
            rc = lib.typlonk_open_all_dev(handle, t, buf.handle if poly else None, offset, m, *a)
        else:
            rc = lib.typlonk_open_all_host(handle, t, _u64p(f) if poly else None, m, *a)
        assert (oxy == 0xA5A5A5A5A5A5A5A5).all() and (oinf == 0x5A).all() and (oev == 0xC3C3C3C3C3C3C3C3).all(), "a refused call wrote to its outputs"
        return rc

    try:
        # ---- the table
        for lg in (0, 25, 26, 64, 0xFFFFFFFF):
            assert table_refused(ctx.h, sid, lg) == ERR_DOMAIN                               # log_n outside 1..24
        assert b"log_n" in lib.typlonk_last_error(ctx.h)
        assert table_refused(None, sid, log_n) == ERR_INVALID_ARG                            # a null context
        assert table_refused(ctx.h, sid, log_n, with_id=False) == ERR_INVALID_ARG            # a null output id
        assert table_refused(ctx.h, 999999, log_n) == ERR_INVALID_ARG                        # an unknown id
        shard = ctx.srs_generate(_limbs(s), n + 3)
        ctx.srs_set_shard(shard, 0, 2 * n + 6)
        assert table_refused(ctx.h, shard, log_n) == ERR_INVALID_ARG                         # a shard
        ctx.srs_free(shard)
        assert table_refused(ctx.h, sid, 5) == ERR_INVALID_ARG                               # 19 < 31 points
        short = ctx.srs_generate(_limbs(s), n - 2)
        assert table_refused(ctx.h, short, log_n) == ERR_INVALID_ARG                         # one point short of n - 1
        ctx.srs_free(short)
        assert table_refused(ctx.h, tab, 2) == ERR_INVALID_ARG                               # a table as the source
        assert b"table" in lib.typlonk_last_error(ctx.h)
        # ---- the openings, both forms
        for dev in (True, False):
            assert open_refused(None, tab, n, dev) == ERR_INVALID_ARG                        # a null context
            assert open_refused(ctx.h, tab, n, dev, poly=False) == ERR_INVALID_ARG           # null coefficients
            assert open_refused(ctx.h, tab, n, dev, xy=False) == ERR_INVALID_ARG             # null proofs_xy
            assert open_refused(ctx.h, tab, n, dev, inf=False) == ERR_INVALID_ARG            # null proofs_inf
            assert open_refused(ctx.h, 999999, n, dev) == ERR_INVALID_ARG                    # an unknown id
            assert open_refused(ctx.h, sid, n, dev) == ERR_INVALID_ARG                       # an SRS that is no table
            assert open_refused(ctx.h, tab, 0, dev) == ERR_LENGTH                            # m = 0
            assert open_refused(ctx.h, tab, n + 1, dev) == ERR_LENGTH                        # m > n
        assert open_refused(ctx.h, tab, n, offset=1) == ERR_RANGE                            # past the end of the buffer
        assert open_refused(ctx.h, tab, 1, offset=n + 1) == ERR_RANGE
        # nothing was created or changed, and a good call still succeeds
        assert ctx.srs_len(sid) == n + 3 and ctx.srs_len(tab) == 2 * n
        _check(ctx, tab, fr_unpack(f), FK.openings_known_secret(fr_unpack(f), s, log_n), log_n)
    finally:
        buf.free()
        ctx.srs_free(sid)
        ctx.srs_free(tab)


# ---- 9. the C++ mirror ------------------------------------------------------------------------------------------------------
def test_mirror_open_all(built):
    """tests/cpp/test_open_all_host: kzg::Srs::open_all_table / KzgScheme::open_all of the C++ mirror"""
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "test_open_all_host")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for t in ("open_all ok", "verify ok", "refusals ok"):
        assert t in r.stdout
