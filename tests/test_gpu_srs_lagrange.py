"""typlonk_srs_g1_ntt on the GPU: the Lagrange form of an SRS against big integers (tests/srs_lagrange_ref.py) word for word,
the degenerate secrets that drive every exceptional addition through every stage, arbitrary points, commitments from
evaluations against iNTT + MSM (existing, oracle-tested code), the round trip, the prover's own commitments, the C++ mirror
and the refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import srs_lagrange_ref as LR
from helpers import O, fr_pack, g1_pack

pytestmark = pytest.mark.gpu

R = O.R
S = 0x5EC2E7D00D51
ORDER3 = (0, 2)   # on y^2 = x^3 + 4, of order 3: not a multiple of G


def _limbs(v):
    return np.array(O.fr_to_mont_limbs(v % R), dtype=np.uint64)


def _same(got, want):
    return (got[0] == want[0]).all() and (got[1] == want[1]).all()


def _lagrange_of(ctx, sid, log_n, points):
    """the Lagrange entry of `sid` must download as `points`, word for word and flag for flag"""
    lag = ctx.srs_lagrange(sid, log_n)
    try:
        assert ctx.srs_len(lag) == 1 << log_n
        got = ctx.srs_download(lag)
    finally:
        ctx.srs_free(lag)
    want = g1_pack(points)
    bad = [i for i in range(len(points)) if not (got[0][i] == want[0][i]).all() or got[1][i] != want[1][i]]
    assert not bad, bad
    return got


# ---- 1. the closed form, a known full-width s ------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", range(8))
def test_closed_form(ctx, log_n):
    """[L_i(s)] G point for point; log_n = 0 gives G itself, log_n = 7 puts a stage's butterflies in more than one wavefront"""
    n = 1 << log_n
    s = int.from_bytes(np.random.default_rng(0x1A6 + log_n).bytes(32), "little") % R
    sid = ctx.srs_generate(_limbs(s), n + 3)
    try:
        before = ctx.srs_download(sid)
        want = LR.lagrange_points(s, log_n)
        assert log_n or want == [O.G1]
        _lagrange_of(ctx, sid, log_n, want)
        assert ctx.srs_len(sid) == n + 3 and _same(ctx.srs_download(sid), before)   # the source entry is untouched
    finally:
        ctx.srs_free(sid)


# ---- 2. degenerate secrets: every exceptional addition ----------------------------------------------------------------------
def test_secret_in_the_domain(ctx):
    """s = w^5 at log_n = 4: L_i(s) is 1 at i = 5 and 0 elsewhere, so every other sum must cancel to the identity"""
    s = pow(O.domain_root(4), 5, R)
    sid = ctx.srs_generate(_limbs(s), 19)
    try:
        got = _lagrange_of(ctx, sid, 4, [O.G1 if i == 5 else None for i in range(16)])
        assert got[1].tolist() == [0 if i == 5 else 1 for i in range(16)]
    finally:
        ctx.srs_free(sid)


@pytest.mark.parametrize("log_n", [1, 4, 7])
def test_secret_one(ctx, log_n):
    """s = 1: every point is G, so P = [w]Q or P = -[w]Q wherever w = +-1; index 0 is G, the rest the identity"""
    n = 1 << log_n
    sid = ctx.srs_generate(_limbs(1), n + 3)
    try:
        assert _same(ctx.srs_download(sid), g1_pack([O.G1] * (n + 3)))
        _lagrange_of(ctx, sid, log_n, [O.G1] + [None] * (n - 1))
    finally:
        ctx.srs_free(sid)


@pytest.mark.parametrize("log_n", [1, 4, 7])
def test_secret_zero(ctx, log_n):
    """s = 0: G, then identities -- identity operands in every stage; every output is [1/n] G"""
    n = 1 << log_n
    sid = ctx.srs_generate(_limbs(0), n + 3)
    try:
        assert _same(ctx.srs_download(sid), g1_pack([O.G1] + [None] * (n + 2)))
        _lagrange_of(ctx, sid, log_n, [O.g1_mul(O.G1, pow(n, -1, R))] * n)
    finally:
        ctx.srs_free(sid)


# ---- 3. arbitrary points ---------------------------------------------------------------------------------------------------
def test_arbitrary_points(ctx):
    """[k_j] G for random k_j at log_n = 6 with an identity record and a repeated point: [intt(k)_i] G.  Then the same entry with
    the order-3 point (0, 2) in place of one record: no scalar of Fr acts on that point, so what it adds to each output is not
    fixed by the formula -- but every step is a homomorphism, so each output moves by an element of the group (0, 2) generates
    (the written-out case below pins the values)."""
    rng = np.random.default_rng(0xA4B)
    ks = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(64)]
    ks[9] = 0            # the identity record
    ks[40] = ks[17]      # a repeated point
    pts = [O.g1_mul(O.G1, k) for k in ks]
    assert pts[9] is None
    xy, inf = g1_pack(pts + [O.G1] * 3)                     # three more points than the domain: ignored
    sid = ctx.srs_load(xy, inf)
    want = [O.g1_mul(O.G1, k) for k in LR.scalars_to_lagrange(ks, 6)]
    try:
        _lagrange_of(ctx, sid, 6, want)
    finally:
        ctx.srs_free(sid)
    ks[23] = 0
    pts[23] = ORDER3
    base = [O.g1_mul(O.G1, k) for k in LR.scalars_to_lagrange(ks, 6)]
    xy, inf = g1_pack(pts)
    sid = ctx.srs_load(xy, inf)
    lag = ctx.srs_lagrange(sid, 6)
    try:
        got = ctx.srs_download(lag)
        orbit = [None, ORDER3, O.g1_neg(ORDER3)]
        for i in range(64):
            p = O.g1_from_limbs([int(v) for v in got[0][i]], int(got[1][i]))
            assert O.g1_add(p, O.g1_neg(base[i])) in orbit, i
    finally:
        ctx.srs_free(sid)
        ctx.srs_free(lag)


@pytest.mark.parametrize("direction", [LR.TO_LAGRANGE, LR.FROM_LAGRANGE])
def test_small_order_point_written_out(ctx, direction):
    """log_n = 2 over ((0, 2), [a]G, (0, 2), identity): P = Q in the first stage's sum (a doubling), P = -(-Q) in its difference
    (the identity), and an identity operand.  Outside the group of order r a scalar acts as its canonical integer and -1 as
    negation, which is how the sums are written out here: with v = w_4^(+-1) and c = 1/4 (TO_LAGRANGE; 1 the other way)
        out[0] = [c]((x0 + x2) + (x1 + x3))      out[1] = [c]((x0 - x2) + [v](x1 - x3))
        out[2] = [c]((x0 + x2) - (x1 + x3))      out[3] = [c]((x0 - x2) - [v](x1 - x3))"""
    a = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100A5A5 % R
    x = [ORDER3, O.g1_mul(O.G1, a), ORDER3, None]
    xy, inf = g1_pack(x)
    sid = ctx.srs_load(xy, inf)
    add, neg, mul = O.g1_add, O.g1_neg, O.g1_mul
    v = O.domain_root(2)
    c = 1
    if direction == LR.TO_LAGRANGE:
        v, c = pow(v, -1, R), pow(4, -1, R)
    e, o = add(x[0], x[2]), add(x[0], neg(x[2]))
    assert e == neg(ORDER3) and o is None
    f, g = add(x[1], x[3]), mul(add(x[1], neg(x[3])), v)
    want = [mul(add(e, f), c), mul(add(o, g), c), mul(add(e, neg(f)), c), mul(add(o, neg(g)), c)]
    new = ctx.srs_lagrange(sid, 2) if direction == LR.TO_LAGRANGE else ctx.srs_from_lagrange(sid, 2)
    try:
        assert _same(ctx.srs_download(new), g1_pack(want))
    finally:
        ctx.srs_free(sid)
        ctx.srs_free(new)


# ---- 4. a commitment from evaluations ---------------------------------------------------------------------------------------
def test_commitment_from_evaluations(ctx):
    """msm(lagrange, evals) == msm(srs, intt(evals)) at n = 2^14, on the plain path and over tables; the points at wavefront
    and workgroup edges against the closed form"""
    log_n, n = 14, 1 << 14
    sid = ctx.srs_generate(_limbs(S), n + 3)
    lag = ctx.srs_lagrange(sid, log_n)
    try:
        assert ctx.srs_len(lag) == n
        rng = np.random.default_rng(0xE7A1)
        evals = fr_pack([int.from_bytes(rng.bytes(32), "little") % R for _ in range(n)])
        want = ctx.msm(sid, ctx.ntt(evals, log_n, inverse=True))
        got = ctx.msm(lag, evals)
        assert (got[0] == want[0]).all() and got[1] == want[1] == 0
        ctx.srs_precompute(lag)                              # n = TYPLONK_TABLES_AUTO_MIN_LEN: tables are built
        got = ctx.msm(lag, evals)
        assert (got[0] == want[0]).all() and got[1] == want[1]
        edges = [0, 1, 63, 64, n - 1]
        exp = g1_pack(LR.lagrange_points(S, log_n, only=edges))
        for k, i in enumerate(edges):
            xy, inf = ctx.srs_download(lag, i, 1)
            assert (xy[0] == exp[0][k]).all() and inf[0] == exp[1][k], i
    finally:
        ctx.srs_free(sid)
        ctx.srs_free(lag)


# ---- 5. the round trip -------------------------------------------------------------------------------------------------------
def test_round_trip(ctx):
    """from_lagrange(lagrange(x, 10), 10) == the first 1024 points of x, for a generated SRS and for one with an identity inside"""
    sid = ctx.srs_generate(_limbs(S), 1027)
    xy, inf = ctx.srs_download(sid)
    holed_xy, holed_inf = xy.copy(), inf.copy()
    holed_xy[517], holed_inf[517] = g1_pack([None])[0][0], 1
    holed = ctx.srs_load(holed_xy, holed_inf)
    try:
        for src, (wxy, winf) in ((sid, (xy, inf)), (holed, (holed_xy, holed_inf))):
            lag = ctx.srs_lagrange(src, 10)
            back = ctx.srs_from_lagrange(lag, 10)
            try:
                assert ctx.srs_len(lag) == ctx.srs_len(back) == 1024
                assert _same(ctx.srs_download(back), (wxy[:1024], winf[:1024]))
                assert not _same(ctx.srs_download(lag), (wxy[:1024], winf[:1024]))
            finally:
                ctx.srs_free(lag)
                ctx.srs_free(back)
    finally:
        ctx.srs_free(sid)
        ctx.srs_free(holed)


# ---- 6. the prover's own commitments ----------------------------------------------------------------------------------------
def test_the_provers_commitments(ctx):
    """the wire commitments of a compact proof are the MSMs of the wire columns over the Lagrange entry (the blinding rows are
    rows of the column), and typlonk_circuit_commitments the MSMs of the selector and sigma evaluations"""
    from oracle import plonk_oracle as PO
    from test_gpu_compact import PyCircuit

    c = PyCircuit(ctx, 3)
    lag = ctx.srs_lagrange(c.sid, 3)
    try:
        cols = c.columns([], seed=0)
        proof = c.prove([], seed=0)
        for col, (xy, inf) in zip(cols, proof["commit"]):
            got = ctx.msm(lag, fr_pack(col))
            assert (got[0] == xy).all() and got[1] == inf
        _, _, q_evals, perm = PO.squaring_chain(3)
        _, sig = PO.compile_permutation(perm, c.n, 3, PO.COSETS)
        evals = [q_evals[k] for k in ("q_l", "q_r", "q_o", "q_m", "q_c")] + list(sig)
        for ev, (xy, inf) in zip(evals, ctx.circuit_commitments(c.sid, c.cid)):
            got = ctx.msm(lag, fr_pack(ev))
            assert (got[0] == xy).all() and got[1] == inf
    finally:
        ctx.srs_free(lag)
        c.free()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    from typlonk_amd.capi import ERR_INVALID_ARG

    lib = ctx.lib
    sid = ctx.srs_generate(_limbs(S), 19)

    def refused(handle, s, log_n, direction, with_id=True):
        new = C.c_uint32(0xABABABAB)
        rc = lib.typlonk_srs_g1_ntt(handle, s, log_n, direction, C.byref(new) if with_id else None)
        assert new.value == 0xABABABAB, "a refused call wrote to its output"
        return rc

    try:
        before = ctx.srs_len(sid)
        assert refused(None, sid, 4, LR.TO_LAGRANGE) == ERR_INVALID_ARG                     # a null context
        assert refused(ctx.h, sid, 4, LR.TO_LAGRANGE, with_id=False) == ERR_INVALID_ARG     # a null output id
        assert refused(ctx.h, 999999, 4, LR.TO_LAGRANGE) == ERR_INVALID_ARG                 # an unknown id
        shard = ctx.srs_generate(_limbs(S), 19)
        ctx.srs_set_shard(shard, 0, 38)
        assert refused(ctx.h, shard, 4, LR.TO_LAGRANGE) == ERR_INVALID_ARG                  # a shard
        ctx.srs_free(shard)
        for direction in (2, 0xFFFFFFFF):
            assert refused(ctx.h, sid, 4, direction) == ERR_INVALID_ARG                     # neither direction
        for direction in (LR.TO_LAGRANGE, LR.FROM_LAGRANGE):
            assert refused(ctx.h, sid, 5, direction) == ERR_INVALID_ARG                     # 32 > 19 points
            assert refused(ctx.h, sid, 26, direction) == ERR_INVALID_ARG                    # past the SRS length cap
            assert refused(ctx.h, sid, 64, direction) == ERR_INVALID_ARG
        assert b"log_n" in lib.typlonk_last_error(ctx.h)
        # nothing was created or changed, and a good call still succeeds
        assert ctx.srs_len(sid) == before
        lag = ctx.srs_lagrange(sid, 4)
        assert _same(ctx.srs_download(lag), g1_pack(LR.lagrange_points(S, 4)))
        ctx.srs_free(lag)
    finally:
        ctx.srs_free(sid)


# ---- 8. the C++ mirror -----------------------------------------------------------------------------------------------------------
def test_mirror_lagrange_and_commit_evaluations(built):
    """tests/cpp/test_srs_lagrange_host: kzg::Srs::lagrange / from_lagrange / KzgScheme::commit_evaluations of the C++ mirror"""
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "test_srs_lagrange_host")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for t in ("lagrange ok", "from_lagrange ok", "commit_evaluations ok", "refusals ok"):
        assert t in r.stdout
