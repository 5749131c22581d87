"""The compact proof shape on the GPU: typlonk_prove_compact / _host against the Python statement (tests/compact_ref.py) bit for
bit, against the round API driven by the compact proof's own challenges, and typlonk_verify_compact -- batches, tampering,
long public-input columns, a fresh context holding nothing but the verifying key -- and every refusal."""
import ctypes as C
import functools

import numpy as np
import pytest

import compact_ref as CR
from helpers import O, fr_pack, fr_unpack, g1_pack, g1_unpack_one
from oracle import pairing as PR
from oracle import plonk_oracle as PO

pytestmark = pytest.mark.gpu

R = O.R
SECRET = 0x5EC2E7D00D51


def _limbs(v):
    return np.array(O.fr_to_mont_limbs(v % R), dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _g2s():
    return np.array(CR.g2s_limbs(PR.srs_g2(SECRET)[1]), dtype=np.uint64)


def _pt(p):
    return g1_unpack_one(p[0], p[1])


def _to_python(d):
    """a compact_dict -> compact_ref's proof form (affine integer points, canonical integers)"""
    return {"commit": [_pt(p) for p in d["commit"]], "z_commit": _pt(d["z_commit"]), "t_commit": [_pt(p) for p in d["t_commit"]],
            "witness": [_pt(p) for p in d["witness"]], "evals": fr_unpack(np.array(d["evals"]))}


def _tamper_point(d, key, i=None):
    """replace one point by itself + G (still on the curve)"""
    d = dict(d)
    if i is None:
        xy, f = g1_pack([O.g1_add(_pt(d[key]), O.G1)])
        d[key] = (xy[0], int(f[0]))
    else:
        lst = list(d[key])
        xy, f = g1_pack([O.g1_add(_pt(lst[i]), O.G1)])
        lst[i] = (xy[0], int(f[0]))
        d[key] = lst
    return d


def _tampered(d):
    out = []
    for key, cnt in (("commit", 3), ("t_commit", 3), ("witness", 2)):
        for i in range(cnt):
            out.append((f"{key}{i}", _tamper_point(d, key, i)))
    out.append(("z_commit", _tamper_point(d, "z_commit")))
    for i in range(7):
        ev = list(d["evals"])
        ev[i] = _limbs(fr_unpack(ev[i])[0] + 1)
        out.append((f"eval{i}", dict(d, evals=ev)))
    w = list(d["witness"])
    xy = w[1][0].copy()
    xy[6] ^= np.uint64(1)                               # y + 1: off the curve
    w[1] = (xy, 0)
    out.append(("off_curve", dict(d, witness=w)))
    ev = list(d["evals"])
    ev[2] = np.array([~np.uint64(0)] * 4, dtype=np.uint64)   # not a canonical residue
    out.append(("non_canonical", dict(d, evals=ev)))
    return out


# ---- the Python circuit on the device: bit-exact comparison --------------------------------------------------------------
class PyCircuit:
    """compact_ref's squaring chain, its tables loaded on the device"""

    def __init__(self, ctx, log_n):
        n, _, q_evals, perm = PO.squaring_chain(log_n)
        self.ctx, self.log_n, self.n = ctx, log_n, n
        srs = O.srs_from_secret_fast(SECRET, n + 3)
        self.ref = CR.setup(log_n, q_evals, perm, srs, PR.srs_g2(SECRET)[1])
        bufs = []
        for poly in [self.ref["q"][k] for k in ("q_l", "q_r", "q_o", "q_m", "q_c")] + self.ref["sigma"]:
            b = ctx.alloc(n)
            b.upload(fr_pack(list(poly) + [0] * (n - len(poly))))
            bufs.append(b)
        self.cid = ctx.circuit_load(log_n, bufs[:5], bufs[5:])
        for b in bufs:
            b.free()
        self.sid = ctx.srs_generate(_limbs(SECRET), n + 3)
        self.cosets = [_limbs(k) for k in PO.COSETS]
        self.vk = ctx.circuit_vk(self.sid, self.cid, self.cosets, _g2s())

    def columns(self, pi, seed=0):
        from test_compact_ref import chain_columns

        return chain_columns(self.log_n, pi, seed=seed)

    def prove(self, pi, seed=0, host=False):
        cols = self.columns(pi, seed)
        if host:
            return self.ctx.prove_compact_host(self.sid, self.cid, [fr_pack(c) for c in cols],
                                               fr_pack(pi) if pi else None, self.cosets)
        bufs = [self.ctx.alloc(self.n) for _ in range(3)]
        for b, c in zip(bufs, cols):
            b.upload(fr_pack(c))
        pib = None
        if pi:
            pib = self.ctx.alloc(len(pi) + 5)                   # longer than pi_len: only pi_len rows are read
            pib.upload(fr_pack(list(pi) + [0xBAD] * 5))
        try:
            return self.ctx.prove_compact(self.sid, self.cid, bufs, pib, len(pi), self.cosets)
        finally:
            for b in bufs + ([pib] if pib else []):
                b.free()

    def free(self):
        self.ctx.circuit_free(self.cid)
        self.ctx.srs_free(self.sid)


def _pi_values(n, length, seed):
    """`length` public values; rows n - 3 .. (the blinding rows, no gate) are zero"""
    rng = np.random.default_rng(seed)
    vals = [int(v) for v in rng.integers(1, 1 << 60, size=min(length, n - 3))]
    return vals + [0] * (length - len(vals))


@pytest.mark.parametrize("log_n,pi_lens", [(3, (0, 1, 8)), (4, (0,)), (5, (0, 1, 32)), (6, (0, 1))])
def test_whole_proof_equals_the_python_prover(ctx, log_n, pi_lens):
    c = PyCircuit(ctx, log_n)
    try:
        vk_py = c.ref["vk"]
        assert [_pt((c.vk.commit_xy[i], c.vk.commit_inf[i])) for i in range(8)] == vk_py["commitments"]
        assert _pt((c.vk.srs0_xy, c.vk.srs0_inf)) == vk_py["srs0"]
        for pl in pi_lens:
            pi = _pi_values(c.n, pl, 100 + pl)
            got = c.prove(pi, seed=pl)
            exp = CR.prove(c.ref, c.columns(pi, seed=pl), pi)
            assert exp["r_zeta"] == 0
            assert _to_python(got) == {k: exp[k] for k in ("commit", "z_commit", "t_commit", "witness", "evals")}, (log_n, pl)
            assert {k: fr_unpack(v)[0] for k, v in got["challenges"].items()} == exp["challenges"]
            assert got["challenges"]["v"].tolist() == CR_native_challenges(c.vk, got, pi)[4].tolist()
            # the device verifier and the Python one agree, on the proof and on a tampered copy
            bad = _tamper_point(got, "witness", 0)
            pis = [fr_pack(pi) if pi else None] * 2
            assert ctx.verify_compact(c.vk, [got, bad], pi=pis).tolist() == [True, False]
            assert CR.verify_batch(vk_py, [_to_python(got), _to_python(bad)], [pi, pi]) == [True, False]
    finally:
        c.free()


def CR_native_challenges(vk, d, pi):
    from typlonk_amd.capi import compact_challenges

    return compact_challenges(vk, d, fr_pack(pi) if pi else None)


# ---- the typlonk_amd squaring chain: round-API cross-checks, batches ----------------------------------------------------------
class Chain:
    def __init__(self, ctx, log_n):
        from typlonk_amd.circuits import SquaringChain

        self.ctx, self.log_n, self.n = ctx, log_n, 1 << log_n
        self.chain = SquaringChain(ctx, log_n, keep_host=True)
        self.cid, self.cosets = self.chain.circuit, self.chain.cosets
        self.host = self.chain.host_inputs()
        self.sid = ctx.srs_generate(_limbs(SECRET), self.n + 3)
        self.vk = ctx.circuit_vk(self.sid, self.cid, self.cosets, _g2s())

    def columns(self, variant=0, pi=None):
        n = self.n
        cols = [c.copy() for c in self.host["wires"]]
        if pi is not None:
            x = 3
            xs = [x]
            for j in range(n - 3):
                x = (x * x + (pi[j] if j < len(pi) else 0)) % R
                xs.append(x)
            cols[0][:n - 3] = fr_pack(xs[:n - 3])
            cols[1][:n - 3] = cols[0][:n - 3]
            cols[2][:n - 3] = fr_pack(xs[1:n - 2])
        if variant:
            for i in range(3):
                cols[i][n - 3:] = fr_pack([(variant * 1000003 + 17 * i + k) % R for k in range(3)])
        return cols

    def prove(self, variant=0, pi=None, host=False):
        cols = self.columns(variant, pi)
        pic = fr_pack(pi) if pi else None
        if host:
            return self.ctx.prove_compact_host(self.sid, self.cid, cols, pic, self.cosets)
        bufs = [self.ctx.alloc(self.n) for _ in range(3)]
        for b, c in zip(bufs, cols):
            b.upload(c)
        pib = None
        if pic is not None:
            pib = self.ctx.alloc(len(pi))
            pib.upload(pic)
        try:
            return self.ctx.prove_compact(self.sid, self.cid, bufs, pib, None, self.cosets)
        finally:
            for b in bufs + ([pib] if pib else []):
                b.free()

    def free(self):
        self.chain.free()
        self.ctx.srs_free(self.sid)


def _cross_check(ctx, c, d):
    """the round API driven by the compact proof's challenges gives its commitments, evaluations and witnesses"""
    ch = d["challenges"]
    bufs = [ctx.alloc(c.n) for _ in range(3)]
    for b, col in zip(bufs, c.columns()):
        b.upload(col)
    rounds = ctx.prove(c.sid, c.cid, bufs, None, c.cosets, challenge12=lambda pts: (ch["beta"], ch["gamma"]),
                       challenge34=lambda pts: (ch["alpha"], ch["zeta"]), challenge_v=lambda evals: ch["v"])
    for b in bufs:
        b.free()
    same = lambda p, q: (np.asarray(p[0]) == np.asarray(q[0])).all() and int(p[1]) == int(q[1])   # noqa: E731
    assert all(same(p, q) for p, q in zip(rounds["commit"], d["commit"]))                         # round1
    assert same(rounds["z_commit"], d["z_commit"])                                                # round2(beta, gamma)
    assert all((rounds["evals"][i] == d["evals"][i]).all() for i in range(5))                     # round3_evals(alpha, zeta)
    assert not rounds["evals"][5].any()                                                           # r(zeta) = 0
    assert all(same(p, q) for p, q in zip(rounds["t_commit"], d["t_commit"]))                     # round4_batched(v)
    assert same(rounds["witness"][1], d["witness"][1])
    # sigma_i(zeta) and W_zeta = w[0] + v^5 [q_s1] + v^6 [q_s2]
    sig = []
    for ev in c.host["sigma"][:2]:
        b = ctx.alloc(c.n)
        b.upload(ev)
        ctx.ntt_dev(b, c.log_n, inverse=True)
        sig.append(b)
    se = ctx.poly_eval_dev(sig, c.n, np.array([ch["zeta"]]))
    assert (se[0, 0] == d["evals"][5]).all() and (se[1, 0] == d["evals"][6]).all()
    v = fr_unpack(ch["v"])[0]
    acc = _pt(rounds["witness"][0])
    for i, b in enumerate(sig):
        q = ctx.alloc(c.n)
        y = ctx.open_dev(b, c.n, ch["zeta"], q_out=q)
        assert (y == d["evals"][5 + i]).all()
        acc = O.g1_add(acc, O.g1_mul(g1_unpack_one(*ctx.msm_dev(c.sid, q, 0, c.n - 1)), pow(v, 5 + i, R)))
        q.free()
        b.free()
    assert acc == _pt(d["witness"][0])


@pytest.mark.parametrize("log_n", [12, 16])
def test_round_api_cross_check(ctx, log_n):
    c = Chain(ctx, log_n)
    try:
        d = c.prove()
        _cross_check(ctx, c, d)
        assert ctx.verify_compact(c.vk, [d]).tolist() == [True]
    finally:
        c.free()


def test_round_api_cross_check_and_verify_at_2_20(built):
    from conftest import need_resources

    import typlonk_amd

    need_resources(host_gib=8, hbm_gib=12)
    ctx = typlonk_amd.Context(0)
    try:
        c = Chain(ctx, 20)
        d = c.prove()
        _cross_check(ctx, c, d)
        d2 = c.prove(2)
        assert ctx.verify_compact(c.vk, [d, d2]).tolist() == [True, True]
        bad = dict(d2, evals=d2["evals"][:4] + [_limbs(fr_unpack(d2["evals"][4])[0] + 1)] + d2["evals"][5:])
        assert ctx.verify_compact(c.vk, [d, bad]).tolist() == [True, False]
        c.free()
    finally:
        ctx.close()


@pytest.mark.slow
def test_verify_at_2_22(built):
    from conftest import need_resources

    import typlonk_amd

    need_resources(host_gib=16, hbm_gib=24)
    ctx = typlonk_amd.Context(0)
    try:
        c = Chain(ctx, 22)
        d = c.prove()
        assert ctx.verify_compact(c.vk, [d]).tolist() == [True]
        assert ctx.verify_compact(c.vk, [_tamper_point(d, "t_commit", 1)]).tolist() == [False]
        c.free()
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def chain12(ctx):
    c = Chain(ctx, 12)
    c.proofs = [c.prove(v) for v in range(64)]
    yield c
    c.free()


def test_device_form_equals_host_form(chain12):
    c = chain12
    for pi in (None, _pi_values(c.n, 5, 1), _pi_values(c.n, 3000, 2)):
        a = c.prove(4, pi=pi)
        b = c.prove(4, pi=pi, host=True)
        assert all((np.asarray(x[0]) == np.asarray(y[0])).all() and x[1] == y[1]
                   for key in ("commit", "t_commit", "witness") for x, y in zip(a[key], b[key]))
        assert (a["z_commit"][0] == b["z_commit"][0]).all()
        assert all((x == y).all() for x, y in zip(a["evals"], b["evals"]))
        assert all((a["challenges"][k] == b["challenges"][k]).all() for k in a["challenges"])
    # same witness, different statement: pi_len is hashed (a trailing zero changes the challenges)
    pi = _pi_values(c.n, 5, 1)
    assert not (c.prove(4, pi=pi)["challenges"]["zeta"] == c.prove(4, pi=pi + [0])["challenges"]["zeta"]).all()


def test_batches_are_accepted(ctx, chain12):
    c = chain12
    for k in (1, 2, 17, 64):
        assert ctx.verify_compact(c.vk, c.proofs[:k]).all(), k
    assert ctx.verify_compact(c.vk, []).shape == (0,)
    # short and long public-input columns (host barycentric up to 2048 values, the device above)
    for length in (8, 2048, 2049, 4096):
        pi = _pi_values(c.n, length, length)
        d = c.prove(1, pi=pi)
        col = fr_pack(pi)
        assert ctx.verify_compact(c.vk, [d, c.proofs[3]], pi=[col, None]).tolist() == [True, True], length
        assert ctx.verify_compact(c.vk, [d], pi=[None]).tolist() == [False], length
        assert ctx.verify_compact(c.vk, [d], pi=[col[:-1]]).tolist() == [False], length
    # a long column in a batch of 17
    pi = _pi_values(c.n, 3000, 7)
    d = c.prove(2, pi=pi)
    pis = [None] * 16 + [fr_pack(pi)]
    assert ctx.verify_compact(c.vk, c.proofs[:16] + [d], pi=pis).all()


def test_mixed_batch_rejects_exactly_the_tampered_proofs(ctx, chain12):
    c = chain12
    cases = _tampered(c.proofs[5])
    for name, bad in cases:
        batch = c.proofs[:5] + [bad] + c.proofs[6:17]
        assert ctx.verify_compact(c.vk, batch).tolist() == [k != 5 for k in range(17)], name
    batch = list(c.proofs)
    bad_idx = (1, 30, 63)
    batch[1] = _tamper_point(c.proofs[1], "witness", 0)
    batch[30] = dict(c.proofs[30], evals=[_limbs(7)] + c.proofs[30]["evals"][1:])
    batch[63] = _tamper_point(c.proofs[63], "t_commit", 2)
    ctx.set_profiling(1)
    try:
        got = ctx.verify_compact(c.vk, batch)
        prof = dict(ctx.profile())
    finally:
        ctx.set_profiling(0)
    assert got.tolist() == [k not in bad_idx for k in range(64)]
    assert 1 < prof["verify_folds"] <= 2 * 3 * 6 + 1
    assert "verify_eval" not in prof and {"verify_host", "verify_msm", "verify_pairing"} <= set(prof)


def test_bisection_schedule_is_the_replayed_one(ctx, chain12):
    """three rejected proofs and one that never enters the fold (a non-canonical evaluation), 16 proofs: the verdicts, and
    exactly the folds of verify_ref.bisection_folds -- four levels of splitting"""
    import verify_ref as V

    c = chain12
    batch = list(c.proofs[:16])
    batch[1] = _tamper_point(c.proofs[1], "witness", 0)
    batch[9] = dict(c.proofs[9], evals=[_limbs(7)] + c.proofs[9]["evals"][1:])
    batch[15] = _tamper_point(c.proofs[15], "t_commit", 2)
    batch[4] = dict(_tampered(c.proofs[4]))["non_canonical"]
    ctx.set_profiling(1)
    try:
        got = ctx.verify_compact(c.vk, batch)
        prof = dict(ctx.profile())
    finally:
        ctx.set_profiling(0)
    assert got.tolist() == [k not in (1, 4, 9, 15) for k in range(16)]
    want = V.bisection_folds([k != 4 for k in range(16)], [k in (1, 9, 15) for k in range(16)])
    print("verify_folds", prof["verify_folds"], "replayed", want)
    assert prof["verify_folds"] == want


def test_fresh_context_needs_only_the_vk(built, chain12):
    """a context with no SRS and no circuit: the vk travels as bytes"""
    import typlonk_amd
    from typlonk_amd.capi import Vk

    c = chain12
    vk = Vk.from_buffer_copy(bytes(c.vk))
    fresh = typlonk_amd.Context(0)
    try:
        assert fresh.verify_compact(vk, c.proofs[:3]).tolist() == [True] * 3
        assert fresh.verify_compact(vk, [c.proofs[0], _tamper_point(c.proofs[1], "z_commit")]).tolist() == [True, False]
        pi = _pi_values(c.n, 2100, 3)
        d = c.prove(3, pi=pi)
        fresh.set_profiling(1)
        assert fresh.verify_compact(vk, [d], pi=[fr_pack(pi)]).tolist() == [True]
        assert "verify_eval" in dict(fresh.profile())
        fresh.set_profiling(0)
    finally:
        fresh.close()


def test_unsatisfied_witness(ctx, chain12):
    from typlonk_amd.capi import ERR_UNSATISFIED, TyplonkError

    c = chain12
    cols = c.columns(5)
    cols[2][7] = _limbs(12345)                             # a gate row that no longer holds
    bufs = [ctx.alloc(c.n) for _ in range(3)]
    for b, col in zip(bufs, cols):
        b.upload(col)
    with pytest.raises(TyplonkError) as e:
        ctx.prove_compact(c.sid, c.cid, bufs, None, 0, c.cosets)
    for b in bufs:
        b.free()
    assert e.value.code == ERR_UNSATISFIED
    d = e.value.proof
    assert all(x[0].any() for x in d["commit"] + d["t_commit"] + d["witness"]) and d["challenges"]["v"].any()
    assert ctx.verify_compact(c.vk, [d, c.proofs[0]]).tolist() == [False, True]
    with pytest.raises(TyplonkError) as e:
        ctx.prove_compact_host(c.sid, c.cid, cols, None, c.cosets)
    assert e.value.code == ERR_UNSATISFIED


def test_refusals(ctx, chain12):
    from typlonk_amd import capi
    from typlonk_amd.capi import ERR_INVALID_ARG, ERR_LENGTH, ERR_RANGE, TyplonkError, _u8p

    c = chain12

    def code(fn):
        with pytest.raises(TyplonkError) as e:
            fn()
        return e.value.code

    cols = c.columns()
    bufs = [ctx.alloc(c.n) for _ in range(3)]
    for b, col in zip(bufs, cols):
        b.upload(col)
    pib = ctx.alloc(c.n + 1)
    pib.upload(np.zeros((c.n + 1, 4), dtype=np.uint64))
    try:
        # prover: pi_len > n, a short pi buffer, a short SRS, a sharded SRS, a round-by-round prover open, rows != n
        assert code(lambda: ctx.prove_compact(c.sid, c.cid, bufs, pib, c.n + 1, c.cosets)) == ERR_LENGTH
        assert code(lambda: ctx.prove_compact(c.sid, c.cid, bufs, pib, c.n + 2, c.cosets)) == ERR_LENGTH
        short_pi = ctx.alloc(4)
        assert code(lambda: ctx.prove_compact(c.sid, c.cid, bufs, short_pi, 5, c.cosets)) == ERR_RANGE
        short_pi.free()
        assert code(lambda: ctx.prove_compact_host(c.sid, c.cid, cols, np.zeros((c.n + 1, 4), dtype=np.uint64),
                                                   c.cosets)) == ERR_LENGTH
        short = ctx.srs_generate(_limbs(SECRET), c.n - 1)
        assert code(lambda: ctx.prove_compact(short, c.cid, bufs, None, 0, c.cosets)) == ERR_LENGTH
        ctx.srs_free(short)
        shard = ctx.srs_generate(_limbs(SECRET), c.n + 3)
        ctx.srs_set_shard(shard, 0, 2 * c.n)
        assert code(lambda: ctx.prove_compact(shard, c.cid, bufs, None, 0, c.cosets)) == ERR_INVALID_ARG
        assert code(lambda: ctx.circuit_vk(shard, c.cid, c.cosets, _g2s())) == ERR_INVALID_ARG
        ctx.srs_free(shard)
        assert code(lambda: ctx.prove_compact_host(c.sid, c.cid, [x[:-1] for x in cols], None, c.cosets)) == ERR_LENGTH
        assert code(lambda: ctx.prove_compact_host(c.sid, c.cid, [np.vstack([x, x[:1]]) for x in cols], None,
                                                   c.cosets)) == ERR_LENGTH
        with pytest.raises(ValueError):
            ctx.prove_compact_host(c.sid, c.cid, [cols[0], cols[1], cols[2][:-1]], None, c.cosets)
        assert code(lambda: ctx.prove_compact(c.sid, 99999, bufs, None, 0, c.cosets)) == ERR_INVALID_ARG
        lib = ctx.lib
        w = (C.c_void_p * 3)(*[b.handle.value for b in bufs])
        pr = C.c_void_p()
        cxy = ((C.c_uint64 * 12) * 3)()
        cinf = (C.c_uint8 * 3)()
        assert lib.typlonk_prover_round1(ctx.h, c.sid, c.cid, w, None, C.byref(pr), C.byref(cxy), C.byref(cinf)) == 0
        try:
            assert code(lambda: ctx.prove_compact(c.sid, c.cid, bufs, None, 0, c.cosets)) == ERR_INVALID_ARG
            assert code(lambda: ctx.prove_compact_host(c.sid, c.cid, cols, None, c.cosets)) == ERR_INVALID_ARG
        finally:
            lib.typlonk_prover_free(pr)
        pf = capi.ProofCompact()
        assert lib.typlonk_prove_compact(ctx.h, c.sid, c.cid, None, None, 0, C.byref(capi._cosets_arg(c.cosets)),
                                         C.byref(pf)) == ERR_INVALID_ARG
        assert lib.typlonk_prove_compact(ctx.h, c.sid, c.cid, w, None, 3, C.byref(capi._cosets_arg(c.cosets)),
                                         C.byref(pf)) == ERR_INVALID_ARG
        # after the refusals the context still proves the same proof
        d = ctx.prove_compact(c.sid, c.cid, bufs, None, 0, c.cosets)
        assert (d["witness"][0][0] == c.proofs[0]["witness"][0][0]).all()
    finally:
        for b in bufs + [pib]:
            b.free()
    # vk: g2s off the twist; verifier: a vk point off the curve, a bad g2s, log_n out of range, pi_len > n, null arguments
    bad_g2 = _g2s().copy()
    bad_g2[12] ^= np.uint64(1)
    assert code(lambda: ctx.circuit_vk(c.sid, c.cid, c.cosets, bad_g2)) == ERR_INVALID_ARG
    p = c.proofs[:1]
    for field, idx in (("commit_xy", 2), ("srs0_xy", None), ("g2s_xy", None)):
        vk = capi.Vk.from_buffer_copy(bytes(c.vk))
        arr = getattr(vk, field)
        if idx is None:
            arr[6 if field == "srs0_xy" else 12] ^= 1
        else:
            arr[idx][6] ^= 1
            vk.commit_inf[idx] = 0
        assert code(lambda: ctx.verify_compact(vk, p)) == ERR_INVALID_ARG, field
    vk = capi.Vk.from_buffer_copy(bytes(c.vk))
    vk.log_n = 25
    assert code(lambda: ctx.verify_compact(vk, p)) == capi.ERR_DOMAIN
    assert code(lambda: ctx.verify_compact(c.vk, p, pi=[np.zeros((c.n + 1, 4), dtype=np.uint64)])) == ERR_LENGTH
    ok = np.zeros(1, dtype=np.uint8)
    assert ctx.lib.typlonk_verify_compact(ctx.h, None, None, 1, None, None, _u8p(ok)) == ERR_INVALID_ARG
    assert ctx.lib.typlonk_verify_compact(ctx.h, None, None, 0, None, None, None) == 0
    assert ctx.lib.typlonk_circuit_vk(ctx.h, c.sid, c.cid, None, None, None) == ERR_INVALID_ARG


def test_mirror_prove_compact_and_verify_compact(built):
    """tests/cpp/test_compact_host: CompiledCircuit::prove_compact / verifying_key and plonk::verify_compact, the last one in a
    fresh context holding only the vk"""
    import os
    import subprocess

    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "test_compact_host")
    r = subprocess.run([exe, "6"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "compact mirror ok" in r.stdout
