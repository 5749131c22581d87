"""typlonk_prove_batch / typlonk_prove_batch_host: many witnesses of one circuit per call.  Every proof of a batch must be bit
for bit what typlonk_prove returns for the same witness (commitments, openings, evaluations, challenges), across wave
boundaries, with public inputs, with an unsatisfied witness among satisfied ones, and it must verify with typlonk_verify."""
import ctypes as C

import numpy as np
import pytest

from helpers import O, fr_pack

pytestmark = pytest.mark.gpu

R = O.R
SECRET = 0x5EC2E7D00D51


def _limbs(v):
    return np.array(O.fr_to_mont_limbs(v % R), dtype=np.uint64)


def _g2s_limbs(secret):
    from oracle import pairing as PR

    (x0, x1), (y0, y1) = PR.srs_g2(secret)[1]
    return np.array([limb for c in (x0, x1, y0, y1) for limb in O.fq_to_mont_limbs(c)], dtype=np.uint64)


class Circuit:
    """the squaring chain of typlonk_amd.circuits (x_{j+1} = x_j^2 + pi_j) with witnesses of other seeds, blinders and
    public-input columns"""

    def __init__(self, ctx, log_n, srs_points=None):
        from typlonk_amd.circuits import SquaringChain

        self.ctx, self.log_n, self.n = ctx, log_n, 1 << log_n
        self.chain = SquaringChain(ctx, log_n, keep_host=True)
        self.cid, self.cosets = self.chain.circuit, self.chain.cosets
        self.sid = ctx.srs_generate(_limbs(SECRET), srs_points or self.n + 3)

    def witness(self, k, pi=False, broken=False):
        """host columns (and the public-input column or None) of witness k: chain seed 3 + k, blinders of k; pi: a non-zero
        public-input column; broken: one gate violated"""
        n, g = self.n, self.n - 3
        pis = [int(v) for v in np.random.default_rng(1000 + k).integers(1, 1 << 60, size=g)] if pi else [0] * g
        x = 3 + k
        xs = [x]
        for j in range(g):
            x = (x * x + pis[j]) % R
            xs.append(x)
        bl = [[(k * 1000003 + 17 * i + r + 1) % R for r in range(3)] for i in range(3)]
        cols = [xs[:g] + bl[0], xs[:g] + bl[1], xs[1:g + 1] + bl[2]]
        if broken:
            cols[2][g // 2] = (cols[2][g // 2] + 1) % R
        return [fr_pack(c) for c in cols], (fr_pack(pis + [0] * 3) if pi else None)

    def upload(self, wits):
        bufs, pibs = [], []
        for cols, pi in wits:
            bs = [self.ctx.alloc(self.n) for _ in range(3)]
            for b, c in zip(bs, cols):
                b.upload(c)
            bufs.append(bs)
            pb = None
            if pi is not None:
                pb = self.ctx.alloc(self.n)
                pb.upload(pi)
            pibs.append(pb)
        return bufs, pibs

    def free(self):
        self.chain.free()
        self.ctx.srs_free(self.sid)


def _free(bufs, pibs):
    for bs in bufs:
        for b in bs:
            b.free()
    for b in pibs:
        if b is not None:
            b.free()


def single(ctx, sid, cid, bufs, pib, cosets):
    """typlonk_prove on one witness: (return code, the filled proof) -- also for an unsatisfied witness"""
    from typlonk_amd.capi import Proof

    w = (C.c_void_p * 3)(*[b.handle.value for b in bufs])
    ks = ((C.c_uint64 * 4) * 3)()
    for i in range(3):
        for j, limb in enumerate(np.asarray(cosets[i], dtype=np.uint64).reshape(4)):
            ks[i][j] = int(limb)
    pr = Proof()
    rc = ctx.lib.typlonk_prove(ctx.h, sid, cid, w, pib.handle if pib is not None else None, C.byref(ks), C.byref(pr))
    return rc, ctx._proof_dict(pr)


def same(a, b):
    for key in ("commit", "t_commit", "witness"):
        if any(not (x[0] == y[0]).all() or x[1] != y[1] for x, y in zip(a[key], b[key])):
            return False
    if not (a["z_commit"][0] == b["z_commit"][0]).all() or a["z_commit"][1] != b["z_commit"][1]:
        return False
    if any(not (x == y).all() for x, y in zip(a["evals"], b["evals"])):
        return False
    return all((a["challenges"][k] == b["challenges"][k]).all() for k in ("beta", "gamma", "alpha", "zeta"))


def _check_against_singles(ctx, c, wits, statuses_expected=None):
    from typlonk_amd.capi import OK

    bufs, pibs = c.upload(wits)
    try:
        proofs, st = ctx.prove_batch(c.sid, c.cid, bufs, pibs, c.cosets)
        assert len(proofs) == len(wits)
        for k in range(len(wits)):
            rc, ref = single(ctx, c.sid, c.cid, bufs[k], pibs[k], c.cosets)
            assert st[k] == rc, (k, st[k], rc)
            assert same(proofs[k], ref), k
        if statuses_expected is not None:
            assert st == statuses_expected
        else:
            assert st == [OK] * len(wits)
        return proofs, st
    finally:
        _free(bufs, pibs)


@pytest.mark.parametrize("log_n", [3, 6, 10, 16])
@pytest.mark.parametrize("count", [1, 2, 5])
def test_batch_equals_single_proofs(ctx, log_n, count):
    c = Circuit(ctx, log_n)
    try:
        wits = [c.witness(k, pi=(k % 2 == 1)) for k in range(count)]
        _check_against_singles(ctx, c, wits)
    finally:
        c.free()


def test_batch_across_a_wave_boundary(ctx):
    """70 proofs at 2^4: a wave of 64 and one of 6"""
    c = Circuit(ctx, 4)
    try:
        wits = [c.witness(k, pi=(k % 3 == 0)) for k in range(70)]
        _check_against_singles(ctx, c, wits)
    finally:
        c.free()


def test_host_and_device_forms_agree(ctx):
    c = Circuit(ctx, 8)
    try:
        wits = [c.witness(k, pi=(k == 1)) for k in range(3)]
        bufs, pibs = c.upload(wits)
        try:
            dev, st_dev = ctx.prove_batch(c.sid, c.cid, bufs, pibs, c.cosets)
        finally:
            _free(bufs, pibs)
        host, st_host = ctx.prove_batch_host(c.sid, c.cid, [w[0] for w in wits], [w[1] for w in wits], c.cosets)
        assert st_dev == st_host == [0, 0, 0]
        assert all(same(a, b) for a, b in zip(dev, host))
        # a NULL public-input array is the zero column of every proof
        plain = [c.witness(k) for k in range(2)]
        host2, st2 = ctx.prove_batch_host(c.sid, c.cid, [w[0] for w in plain], None, c.cosets)
        host3, st3 = ctx.prove_batch_host(c.sid, c.cid, [w[0] for w in plain], [None, None], c.cosets)
        assert st2 == st3 == [0, 0] and all(same(a, b) for a, b in zip(host2, host3))
    finally:
        c.free()


@pytest.mark.parametrize("pos", [0, 2])
def test_unsatisfied_witness_only_affects_its_proof(ctx, pos):
    from typlonk_amd.capi import ERR_UNSATISFIED, OK

    c = Circuit(ctx, 6)
    try:
        wits = [c.witness(k, pi=(k == 1), broken=(k == pos)) for k in range(4)]
        exp = [ERR_UNSATISFIED if k == pos else OK for k in range(4)]
        _check_against_singles(ctx, c, wits, exp)
    finally:
        c.free()


def test_batch_proofs_verify(ctx):
    from typlonk_amd.capi import ERR_UNSATISFIED

    c = Circuit(ctx, 10)
    try:
        wits = [c.witness(k, pi=(k in (1, 4)), broken=(k == 3)) for k in range(6)]
        bufs, pibs = c.upload(wits)
        try:
            proofs, st = ctx.prove_batch(c.sid, c.cid, bufs, pibs, c.cosets)
        finally:
            _free(bufs, pibs)
        assert st == [0, 0, 0, ERR_UNSATISFIED, 0, 0]
        ok = ctx.verify(c.sid, c.cid, _g2s_limbs(SECRET), c.cosets, proofs, pi=[w[1] for w in wits], pi_as_prover=True)
        assert ok.tolist() == [True, True, True, False, True, True]
    finally:
        c.free()


def test_prove_batch_arguments(ctx):
    from typlonk_amd.capi import ERR_INVALID_ARG, ERR_LENGTH, Proof, TyplonkError

    c = Circuit(ctx, 5)
    lib = ctx.lib
    wits = [c.witness(k) for k in range(2)]
    bufs, pibs = c.upload(wits)
    ks = ((C.c_uint64 * 4) * 3)()
    for i in range(3):
        for j, limb in enumerate(np.asarray(c.cosets[i], dtype=np.uint64).reshape(4)):
            ks[i][j] = int(limb)
    w = (C.c_void_p * 6)(*[b.handle.value for bs in bufs for b in bs])
    out = (Proof * 2)()
    st = (C.c_int * 2)()

    def still_proves():
        rc, _ = single(ctx, c.sid, c.cid, bufs[0], None, c.cosets)
        assert rc == 0

    def code(fn):
        with pytest.raises(TyplonkError) as e:
            fn()
        return e.value.code

    try:
        assert ctx.prove_batch(c.sid, c.cid, [], None, c.cosets) == ([], [])
        assert lib.typlonk_prove_batch(ctx.h, c.sid, c.cid, None, None, 0, None, None, None) == 0
        assert lib.typlonk_prove_batch(ctx.h, c.sid, c.cid, w, None, 2, C.byref(ks), None, st) == ERR_INVALID_ARG
        still_proves()
        assert lib.typlonk_prove_batch(ctx.h, c.sid, c.cid, w, None, 2, C.byref(ks), out, None) == ERR_INVALID_ARG
        assert lib.typlonk_prove_batch(ctx.h, c.sid, c.cid, None, None, 2, C.byref(ks), out, st) == ERR_INVALID_ARG
        holey = (C.c_void_p * 6)(*[b.handle.value for bs in bufs for b in bs])
        holey[4] = None
        assert lib.typlonk_prove_batch(ctx.h, c.sid, c.cid, holey, None, 2, C.byref(ks), out, st) == ERR_INVALID_ARG
        hp = (C.POINTER(C.c_uint64) * 6)()
        assert lib.typlonk_prove_batch_host(ctx.h, c.sid, c.cid, hp, None, 2, C.byref(ks), out, st) == ERR_INVALID_ARG
        assert lib.typlonk_prove_batch(None, c.sid, c.cid, w, None, 2, C.byref(ks), out, st) == ERR_INVALID_ARG
        still_proves()
        assert code(lambda: ctx.prove_batch(c.sid, 99999, bufs, pibs, c.cosets)) == ERR_INVALID_ARG
        assert code(lambda: ctx.prove_batch(99999, c.cid, bufs, pibs, c.cosets)) == ERR_INVALID_ARG
        still_proves()
        short = ctx.srs_generate(_limbs(SECRET), c.n - 1)
        assert code(lambda: ctx.prove_batch(short, c.cid, bufs, pibs, c.cosets)) == ERR_LENGTH
        ctx.srs_free(short)
        still_proves()
        shard = ctx.srs_generate(_limbs(SECRET), c.n + 3)
        ctx.srs_set_shard(shard, 0, 2 * c.n)
        assert code(lambda: ctx.prove_batch(shard, c.cid, bufs, pibs, c.cosets)) == ERR_INVALID_ARG
        ctx.srs_free(shard)
        still_proves()
        # a round-by-round prover left open refuses the batch; once freed, both forms work again
        pr = C.c_void_p()
        cxy = ((C.c_uint64 * 12) * 3)()
        cinf = (C.c_uint8 * 3)()
        w3 = (C.c_void_p * 3)(*[b.handle.value for b in bufs[0]])
        assert lib.typlonk_prover_round1(ctx.h, c.sid, c.cid, w3, None, C.byref(pr), C.byref(cxy), C.byref(cinf)) == 0
        try:
            assert code(lambda: ctx.prove_batch(c.sid, c.cid, bufs, pibs, c.cosets)) == ERR_INVALID_ARG
        finally:
            lib.typlonk_prover_free(pr)
        still_proves()
        proofs, stt = ctx.prove_batch(c.sid, c.cid, bufs, pibs, c.cosets)
        assert stt == [0, 0]
        _, ref = single(ctx, c.sid, c.cid, bufs[1], None, c.cosets)
        assert same(proofs[1], ref)
    finally:
        _free(bufs, pibs)
        c.free()


@pytest.mark.slow
def test_batch_at_2_20_equals_single_proofs(built):
    """two proofs of 2^20 rows: one wave of two at full size"""
    from conftest import need_resources

    import typlonk_amd

    need_resources(host_gib=8, hbm_gib=24)
    ctx = typlonk_amd.Context(0)
    try:
        c = Circuit(ctx, 20)
        try:
            host = c.chain.host_inputs()["wires"]
            wits = []
            for k in range(2):
                cols = [col.copy() for col in host]
                for i in range(3):
                    cols[i][c.n - 3:] = fr_pack([(k * 7919 + 31 * i + r + 5) % R for r in range(3)])
                wits.append((cols, None))
            _check_against_singles(ctx, c, wits)
        finally:
            c.free()
    finally:
        ctx.close()


def test_mirror_prove_batch(built):
    """tests/cpp/test_prove_batch_host: plonk::CompiledCircuit::prove_batch (typlonk_prove_batch_host) equals the mirror's
    prove_native on each witness, statuses included"""
    import os
    import subprocess

    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "test_prove_batch_host")
    r = subprocess.run([exe, "6"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "prove_batch agrees with prove ok" in r.stdout
