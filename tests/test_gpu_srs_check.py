"""typlonk_srs_check on the GPU: SRS entries made by typlonk_srs_generate, tampered through a download, the oracle's g1_add and
typlonk_srs_load, and judged against [s]G2 -- valid entries of every length class, single bad links, the errors an unweighted
sum misses, defects that cancel under a known seed (the weights pinned to the stated hash), the wrong G2 element, points that
are not group elements, and every refusal."""
import ctypes as C
import functools

import numpy as np
import pytest

import srs_check_ref as SR
from helpers import O, g1_pack, g1_unpack_one
from oracle import pairing as PR

pytestmark = pytest.mark.gpu

R = O.R
S = 0x5EC2E7D00D51
SEED_A, SEED_B = bytes(range(32)), bytes(range(100, 132))
BIG = (1 << 14) + 3   # above TYPLONK_TABLES_AUTO_MIN_LEN: typlonk_srs_precompute(0) builds tables


def _limbs(v):
    return np.array(O.fr_to_mont_limbs(v % R), dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _g2s_py(s=S):
    return PR.srs_g2(s)[1]


def _g2s(s=S):
    return np.array(SR.g2s_limbs(_g2s_py(s)), dtype=np.uint64)


def _ceil_log2(n):
    return (n - 1).bit_length()


class Entry:
    """a generated SRS, its points on the host, and tampered copies of it"""

    def __init__(self, ctx, length, s=S):
        self.ctx, self.len = ctx, length
        self.sid = ctx.srs_generate(_limbs(s), length)
        self.xy, self.inf = ctx.srs_download(self.sid)

    def point(self, i):
        return g1_unpack_one(self.xy[i], self.inf[i])

    def tampered(self, changes, precompute=False):
        """changes: {index: point (None = the identity through the inf flag) or raw (xy[12], inf)} -> a new sid"""
        xy, inf = self.xy.copy(), self.inf.copy()
        for i, p in changes.items():
            if isinstance(p, tuple) and len(p) == 2 and isinstance(p[0], np.ndarray):
                xy[i], inf[i] = p
            else:
                pxy, pinf = g1_pack([p])
                xy[i], inf[i] = pxy[0], pinf[0]
        sid = self.ctx.srs_load(xy, inf)
        if precompute:
            self.ctx.srs_precompute(sid)
        return sid

    def plus_g(self, j, k=1):
        return O.g1_add(self.point(j), O.g1_mul(O.G1, k))


@pytest.fixture(scope="module")
def e130(ctx):
    e = Entry(ctx, 130)
    yield e
    ctx.srs_free(e.sid)


@pytest.fixture(scope="module")
def ebig(ctx):
    e = Entry(ctx, BIG)
    yield e
    ctx.srs_free(e.sid)


def _check_free(ctx, sid, seed=SEED_A, g2s=None):
    try:
        return ctx.srs_check(sid, _g2s() if g2s is None else g2s, seed)
    finally:
        ctx.srs_free(sid)


VALID = {"verdict": SR.VALID, "point_class": 0, "index": 0, "bad_points": 0}


@pytest.mark.parametrize("length", [1, 2, 3, 67, 130])
def test_valid(ctx, length):
    sid = ctx.srs_generate(_limbs(S), length)
    try:
        for seed in (SEED_A, SEED_B):
            assert ctx.srs_check(sid, _g2s(), seed) == dict(VALID, folds=0 if length == 1 else 1), (length, seed)
    finally:
        ctx.srs_free(sid)


@pytest.mark.parametrize("precompute", [False, True])
def test_valid_above_the_table_threshold(ctx, precompute):
    sid = ctx.srs_generate(_limbs(S), BIG)
    try:
        if precompute:
            ctx.srs_precompute(sid)
        for seed in (SEED_A, SEED_B):
            assert ctx.srs_check(sid, _g2s(), seed) == dict(VALID, folds=1), seed
    finally:
        ctx.srs_free(sid)


@pytest.mark.parametrize("j", [1, 63, 64, 129])
def test_one_bad_link(ctx, e130, j):
    rep = _check_free(ctx, e130.tampered({j: e130.plus_g(j)}))
    assert (rep["verdict"], rep["index"], rep["bad_points"]) == (SR.BAD_RATIO, j - 1, 0), rep
    assert 2 <= rep["folds"] <= 1 + _ceil_log2(130), rep


@pytest.mark.parametrize("precompute", [False, True])
def test_one_bad_link_above_the_table_threshold(ctx, ebig, precompute):
    j = 9000
    rep = _check_free(ctx, ebig.tampered({j: ebig.plus_g(j)}, precompute=precompute))
    assert (rep["verdict"], rep["index"]) == (SR.BAD_RATIO, j - 1), rep
    assert 2 <= rep["folds"] <= 1 + _ceil_log2(BIG), rep


def test_errors_an_unweighted_sum_misses(ctx, e130):
    j, k = 17, 99
    swapped = e130.tampered({j: e130.point(k), k: e130.point(j)})
    rep = _check_free(ctx, swapped, SEED_B)
    assert (rep["verdict"], rep["index"]) == (SR.BAD_RATIO, j - 1), rep
    d = O.g1_mul(O.G1, 0xD1FF)
    pair = e130.tampered({j: O.g1_add(e130.point(j), d), k: O.g1_add(e130.point(k), O.g1_neg(d))})
    rep = _check_free(ctx, pair, SEED_B)
    assert (rep["verdict"], rep["index"]) == (SR.BAD_RATIO, j - 1), rep


def test_weights_are_the_powers_of_the_stated_hash(ctx, e130):
    """With s and the seed known, two defects are made to cancel under rho^i: VALID under that seed, BAD_RATIO at j - 1 under
    any other -- which is why the seed must be unknown to whoever made the points, and what fails for any implementation
    whose weights are not exactly the rho^i of the stated hash."""
    j, k, a = 5, 70, 0xABCDEF
    r = SR.rho(SEED_A, 130, _g2s_py())
    b = SR.cancelling_pair(S, r, j, k, a)
    sid = e130.tampered({j: e130.plus_g(j, a), k: e130.plus_g(k, b)})
    try:
        assert ctx.srs_check(sid, _g2s(), SEED_A) == dict(VALID, folds=1)
        rep = ctx.srs_check(sid, _g2s(), SEED_B)
        assert (rep["verdict"], rep["index"]) == (SR.BAD_RATIO, j - 1), rep
    finally:
        ctx.srs_free(sid)


def test_wrong_g2_and_wrong_p0(ctx, e130):
    rep = ctx.srs_check(e130.sid, _g2s(S + 1), SEED_A)
    assert (rep["verdict"], rep["index"]) == (SR.BAD_RATIO, 0), rep
    assert rep["folds"] <= 1 + _ceil_log2(130)
    # [2 s^i] G: a consistent progression from the wrong point
    xy, inf = g1_pack([O.g1_mul(O.G1, 2 * pow(S, i, R)) for i in range(4)])
    rep = _check_free(ctx, ctx.srs_load(xy, inf))
    assert rep == {"verdict": SR.BAD_P0, "point_class": 0, "index": 0, "bad_points": 0, "folds": 0}


def test_membership(ctx, e130):
    off = e130.xy[70].copy()
    off[6] ^= np.uint64(1)   # y + 1 (as a Montgomery residue): off the curve
    rep = _check_free(ctx, e130.tampered({5: (0, 2), 70: (off, 0)}))
    assert rep == {"verdict": SR.BAD_POINT, "point_class": SR.NOT_IN_SUBGROUP, "index": 5, "bad_points": 2, "folds": 0}
    rep = _check_free(ctx, e130.tampered({70: (off, 0)}))
    assert (rep["verdict"], rep["point_class"], rep["index"], rep["bad_points"]) == (SR.BAD_POINT, SR.NOT_ON_CURVE, 70, 1)
    rep = _check_free(ctx, e130.tampered({4: None}))
    assert (rep["verdict"], rep["index"], rep["bad_points"]) == (SR.BAD_RATIO, 3, 0), rep


def test_a_coordinate_above_p_is_reduced_by_the_load(ctx):
    """typlonk_srs_load validates nothing but writes canonical records: G with x + p and y + p as its limbs IS G, word for
    word, to the check and to a download -- no record with a coordinate >= p reaches the membership pass"""
    good = [O.fq_to_mont_limbs(O.GX), O.fq_to_mont_limbs(O.GY)]
    lifted = []
    for limbs in good:
        v = sum(w << (64 * i) for i, w in enumerate(limbs)) + O.P
        assert v < 1 << 384
        lifted += [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(6)]
    sid = ctx.srs_load(np.array([lifted], dtype=np.uint64), np.zeros(1, dtype=np.uint8))
    try:
        assert ctx.srs_check(sid, _g2s(), SEED_A) == dict(VALID, folds=0)
        xy, inf = ctx.srs_download(sid)
        assert xy[0].tolist() == good[0] + good[1] and not inf[0]
    finally:
        ctx.srs_free(sid)


def test_a_shard_is_refused_with_a_communicator_too(built):
    """a one-rank communicator (the real librccl) on a context of the test's own: the shard is still refused, by the check
    and by the contribution, and the outputs are left as they were"""
    import typlonk_amd
    from typlonk_amd import capi
    from typlonk_amd.capi import ERR_INVALID_ARG, _u8p, _u64p, comm_available, comm_unique_id

    if not comm_available():
        pytest.fail("librccl cannot be loaded: the refusal on a context with a communicator cannot run")
    c = typlonk_amd.Context(0)
    try:
        g2s = _g2s()
        seed = np.frombuffer(SEED_A, dtype=np.uint8).copy()
        whole = c.srs_generate(_limbs(S), 16)
        shard = c.srs_generate(_limbs(S), 16)
        c.srs_set_shard(shard, 0, 32)
        c.comm_init(comm_unique_id(), 0, 1)
        try:
            fill = bytes([0xAB]) * C.sizeof(capi.SrsReport)
            rep = capi.SrsReport.from_buffer_copy(fill)
            assert c.lib.typlonk_srs_check(c.h, shard, _u64p(g2s), _u8p(seed), C.byref(rep)) == ERR_INVALID_ARG
            assert bytes(rep) == fill, "a refused call wrote to the report"
            new = C.c_uint32(0xABABABAB)
            out = np.full(24, 0xABABABABABABABAB, dtype=np.uint64)
            t = _limbs(12345)
            assert c.lib.typlonk_srs_contribute(c.h, shard, _u64p(t), _u64p(g2s), C.byref(new), _u64p(out)) == ERR_INVALID_ARG
            assert new.value == 0xABABABAB and (out == 0xABABABABABABABAB).all()
            # a whole entry on the same context is checked as on any other: the call is never a collective
            assert c.srs_check(whole, g2s, SEED_A) == dict(VALID, folds=1)
        finally:
            c.comm_destroy()
    finally:
        c.close()


def test_refusals(ctx, e130):
    from typlonk_amd import capi
    from typlonk_amd.capi import ERR_INVALID_ARG, ERR_LENGTH, _u8p, _u64p

    lib = ctx.lib
    g2s = _g2s()
    seed = np.frombuffer(SEED_A, dtype=np.uint8).copy()
    fill = bytes([0xAB]) * C.sizeof(capi.SrsReport)

    def refused(sid, g, s, with_report=True):
        rep = capi.SrsReport.from_buffer_copy(fill)
        rc = lib.typlonk_srs_check(ctx.h, sid, None if g is None else _u64p(g), None if s is None else _u8p(s),
                                   C.byref(rep) if with_report else None)
        assert bytes(rep) == fill, "a refused call wrote to the report"
        return rc

    assert refused(e130.sid, None, seed) == ERR_INVALID_ARG
    assert refused(e130.sid, g2s, None) == ERR_INVALID_ARG
    assert refused(e130.sid, g2s, seed, with_report=False) == ERR_INVALID_ARG
    assert lib.typlonk_srs_check(None, e130.sid, _u64p(g2s), _u8p(seed), None) == ERR_INVALID_ARG
    assert refused(999999, g2s, seed) == ERR_INVALID_ARG
    bad_g2 = g2s.copy()
    bad_g2[12] ^= np.uint64(1)
    assert refused(e130.sid, bad_g2, seed) == ERR_INVALID_ARG
    shard = ctx.srs_generate(_limbs(S), 16)
    ctx.srs_set_shard(shard, 0, 32)
    assert refused(shard, g2s, seed) == ERR_INVALID_ARG
    ctx.srs_free(shard)
    empty = ctx.srs_generate(_limbs(S), 0)
    assert refused(empty, g2s, seed) == ERR_LENGTH
    ctx.srs_free(empty)
    with pytest.raises(ValueError):
        ctx.srs_check(e130.sid, g2s, b"short")
    rho = np.zeros(4, dtype=np.uint64)
    assert lib.typlonk_srs_check_challenge(None, 130, _u64p(g2s), _u64p(rho)) == ERR_INVALID_ARG
    # after the refusals the entry still checks
    assert ctx.srs_check(e130.sid, g2s, SEED_A) == dict(VALID, folds=1)
