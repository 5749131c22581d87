"""typlonk_srs_contribute on the GPU: [t^i] P_i against big integers, against typlonk_srs_generate(s t) -- existing,
oracle-tested code -- word for word, the edge scalars 1 and r - 1, the exceptional additions (a point of order 3, the
identity), a compact proof on the contributed SRS, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import srs_check_ref as SR
from helpers import O, fr_pack, g1_pack, g1_unpack_one
from oracle import pairing as PR

pytestmark = pytest.mark.gpu

R = O.R
S = 0x5EC2E7D00D51
T = 0x2F7A11C0FFEE5EED2F7A11C0FFEE5EED2F7A11C0FFEE5EED2F7A11C0FFEE5EED % R   # a full-width scalar
SEED = bytes(range(7, 39))
BIG = (1 << 14) + 3


def _limbs(v):
    return np.array(O.fr_to_mont_limbs(v % R), dtype=np.uint64)


def _g2s(s=S):
    return np.array(SR.g2s_limbs(PR.srs_g2(s)[1]), dtype=np.uint64)


def _points(ctx, sid):
    xy, inf = ctx.srs_download(sid)
    return [g1_unpack_one(xy[i], inf[i]) for i in range(len(inf))]


def test_against_big_integers(ctx):
    rng = np.random.default_rng(0x5125)
    s = int.from_bytes(rng.bytes(32), "little") % R
    t = int.from_bytes(rng.bytes(32), "little") % R
    sid = ctx.srs_generate(_limbs(s), 67)
    new, g2o = ctx.srs_contribute(sid, _limbs(t), _g2s(s))
    try:
        old = _points(ctx, sid)
        assert old == O.srs_from_secret_fast(s, 67)             # the old entry is untouched
        got_xy, got_inf = ctx.srs_download(new)
        exp_xy, exp_inf = g1_pack(SR.contribute(old, t))
        assert (got_xy == exp_xy).all() and (got_inf == exp_inf).all()
        assert g2o.tolist() == SR.g2s_limbs(PR.g2_mul(PR.srs_g2(s)[1], t))
    finally:
        ctx.srs_free(sid)
        ctx.srs_free(new)


def test_against_the_generator(ctx):
    """contribute(generate(s), t) == generate(s t), word for word, past many wavefronts and from an entry with tables"""
    sid = ctx.srs_generate(_limbs(S), BIG)
    ctx.srs_precompute(sid)                                     # table 0 is what the contribution reads
    ref = ctx.srs_generate(_limbs(S * T % R), BIG)
    new, g2o = ctx.srs_contribute(sid, _limbs(T), _g2s())
    try:
        assert ctx.srs_len(new) == BIG
        a, b = ctx.srs_download(new), ctx.srs_download(ref)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
        assert g2o.tolist() == SR.g2s_limbs(PR.g2_mul(PR.srs_g2(S)[1], T))
        assert g2o.tolist() == _g2s(S * T % R).tolist()
        rep = ctx.srs_check(new, g2o, SEED)
        assert (rep["verdict"], rep["folds"]) == (SR.VALID, 1), rep
        rep = ctx.srs_check(new, _g2s(), SEED)
        assert (rep["verdict"], rep["index"]) == (SR.BAD_RATIO, 0), rep
    finally:
        for x in (sid, ref, new):
            ctx.srs_free(x)


def test_edge_scalars(ctx):
    sid = ctx.srs_generate(_limbs(S), 130)
    xy, inf = ctx.srs_download(sid)
    one, g2o = ctx.srs_contribute(sid, _limbs(1), _g2s())
    top, g2n = ctx.srs_contribute(sid, _limbs(R - 1), _g2s())
    try:
        a = ctx.srs_download(one)
        assert (a[0] == xy).all() and (a[1] == inf).all() and g2o.tolist() == _g2s().tolist()
        # t = r - 1 = -1: odd indices negated (y -> p - y), even indices unchanged
        exp = xy.copy()
        for i in range(1, 130, 2):
            exp[i, 6:] = O.fq_to_mont_limbs(O.P - O.fq_from_mont_limbs([int(v) for v in xy[i, 6:]]))
        b = ctx.srs_download(top)
        assert (b[0] == exp).all() and not b[1].any()
        assert g2n.tolist() == SR.g2s_limbs(PR.g2_neg(PR.srs_g2(S)[1]))
    finally:
        for x in (sid, one, top):
            ctx.srs_free(x)


def test_exceptional_additions(ctx):
    """a point of order 3 meets g1_madd's equal and opposite branches at every step; the identity stays the identity"""
    pts = O.srs_from_secret_fast(S, 9)
    pts[5], pts[6] = (0, 2), None
    xy, inf = g1_pack(pts)
    sid = ctx.srs_load(xy, inf)
    try:
        for want in (0, 1, 2):   # one t per value of (t^5 mod r) mod 3: the identity, the point, its negative
            t = next(T + d for d in range(64) if pow(T + d, 5, R) % 3 == want)
            new, _ = ctx.srs_contribute(sid, _limbs(t), _g2s())
            got = _points(ctx, new)
            ctx.srs_free(new)
            assert got[5] == O.g1_mul((0, 2), want) and got[6] is None, t
            assert got[:5] == SR.contribute(pts[:5], t)
    finally:
        ctx.srs_free(sid)


def test_a_compact_proof_on_the_contributed_srs(ctx):
    from test_gpu_compact import PyCircuit, _g2s as compact_g2s

    c = PyCircuit(ctx, 3)
    new, g2o = ctx.srs_contribute(c.sid, _limbs(T), compact_g2s())
    try:
        vk = ctx.circuit_vk(new, c.cid, c.cosets, g2o)
        cols = [fr_pack(col) for col in c.columns([], seed=0)]
        proof = ctx.prove_compact_host(new, c.cid, cols, None, c.cosets)
        assert ctx.verify_compact(vk, [proof]).tolist() == [True]
        stale = ctx.circuit_vk(new, c.cid, c.cosets, compact_g2s())      # the old [s]G2 with the new points
        assert ctx.verify_compact(stale, [proof]).tolist() == [False]
        # the check may run while a round-by-round prover is open: it touches none of its arena
        bufs = [ctx.alloc(c.n) for _ in range(3)]
        for b, col in zip(bufs, cols):
            b.upload(col)
        w = (C.c_void_p * 3)(*[b.handle.value for b in bufs])
        pr = C.c_void_p()
        cxy, cinf = ((C.c_uint64 * 12) * 3)(), (C.c_uint8 * 3)()
        assert ctx.lib.typlonk_prover_round1(ctx.h, new, c.cid, w, None, C.byref(pr), C.byref(cxy), C.byref(cinf)) == 0
        try:
            assert ctx.srs_check(new, g2o, SEED)["verdict"] == SR.VALID
        finally:
            ctx.lib.typlonk_prover_free(pr)
            for b in bufs:
                b.free()
    finally:
        ctx.srs_free(new)
        c.free()


def test_mirror_check_and_contribute(built):
    """tests/cpp/test_srs_check_host: kzg::Srs::check / Srs::contribute of the C++ mirror"""
    import os
    import subprocess

    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "test_srs_check_host")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for t in ("check ok", "contribute ok", "verdicts ok", "refusals ok"):
        assert t in r.stdout


def test_refusals(ctx):
    from typlonk_amd.capi import ERR_INVALID_ARG, _u64p

    lib = ctx.lib
    sid = ctx.srs_generate(_limbs(S), 5)
    g2s = _g2s()
    t = _limbs(T)

    def refused(s, tl, g, with_id=True, with_out=True):
        new = C.c_uint32(0xABABABAB)
        out = np.full(24, 0xABABABABABABABAB, dtype=np.uint64)
        rc = lib.typlonk_srs_contribute(ctx.h, s, None if tl is None else _u64p(tl), None if g is None else _u64p(g),
                                        C.byref(new) if with_id else None, _u64p(out) if with_out else None)
        assert new.value == 0xABABABAB and (out == 0xABABABABABABABAB).all(), "a refused call wrote to its outputs"
        return rc

    try:
        before = ctx.srs_len(sid)
        assert refused(sid, None, g2s) == ERR_INVALID_ARG
        assert refused(sid, t, None) == ERR_INVALID_ARG
        assert refused(sid, t, g2s, with_id=False) == ERR_INVALID_ARG
        assert refused(sid, t, g2s, with_out=False) == ERR_INVALID_ARG
        assert refused(999999, t, g2s) == ERR_INVALID_ARG
        assert refused(sid, np.zeros(4, dtype=np.uint64), g2s) == ERR_INVALID_ARG                       # t = 0
        assert refused(sid, np.array([0xffffffff00000001, 0x53bda402fffe5bfe, 0x3339d80809a1d805, 0x73eda753299d7d48],
                                     dtype=np.uint64), g2s) == ERR_INVALID_ARG                           # t = r: not canonical
        assert refused(sid, np.full(4, 0xffffffffffffffff, dtype=np.uint64), g2s) == ERR_INVALID_ARG
        bad_g2 = g2s.copy()
        bad_g2[12] ^= np.uint64(1)
        assert refused(sid, t, bad_g2) == ERR_INVALID_ARG
        shard = ctx.srs_generate(_limbs(S), 5)
        ctx.srs_set_shard(shard, 0, 10)
        assert refused(shard, t, g2s) == ERR_INVALID_ARG
        ctx.srs_free(shard)
        # nothing was created, and the entry still contributes
        assert ctx.srs_len(sid) == before
        new, _ = ctx.srs_contribute(sid, t, g2s)
        assert _points(ctx, new) == SR.contribute(O.srs_from_secret_fast(S, 5), T)
        ctx.srs_free(new)
    finally:
        ctx.srs_free(sid)
