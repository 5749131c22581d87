"""typlonk_prove_batch_compact / typlonk_prove_batch_compact_host: many witnesses of one circuit per call in the compact proof
shape.  Every proof of a batch must be byte for byte what typlonk_prove_compact returns for the same witness and statement
(the 9 points, the 7 evaluations, the five challenges) -- with mixed pi_len inside one batch, across wave boundaries, with an
unsatisfied witness among satisfied ones --, must equal the Python prover of tests/compact_ref.py, and must verify through
typlonk_verify_compact in a context that holds nothing but the verifying key.  Every comparison is exact equality."""
import ctypes as C

import numpy as np
import pytest

import compact_ref as CR
from helpers import fr_pack, fr_unpack
from test_gpu_compact import Chain, PyCircuit, _limbs, _pi_values, _tamper_point, _to_python

pytestmark = pytest.mark.gpu

GARBAGE = 5     # rows behind the pi_len values of a device pi buffer: they must not be read


def _pi_lens(log_n):
    """the mixed public-input lengths of a batch: 0, 1 and n where n is small; 0, 1 and 3000 (the verifier's > 2048 path) at 2^16"""
    return (0, 1, 3000) if log_n >= 16 else (0, 1, 1 << log_n)


def _bytes(d):
    """every field of a compact_dict as one byte string"""
    parts = []
    for key in ("commit", "t_commit", "witness"):
        for xy, inf in d[key]:
            parts += [np.asarray(xy, dtype=np.uint64).tobytes(), bytes([int(inf)])]
    parts += [np.asarray(d["z_commit"][0], dtype=np.uint64).tobytes(), bytes([int(d["z_commit"][1])])]
    parts += [np.asarray(e, dtype=np.uint64).tobytes() for e in d["evals"]]
    parts += [np.asarray(d["challenges"][k], dtype=np.uint64).tobytes() for k in ("beta", "gamma", "alpha", "zeta", "v")]
    return b"".join(parts)


def _upload(ctx, n, wits):
    """wits = [(three host columns, list of public values)]: device columns, and pi buffers longer than pi_len with garbage
    behind the values"""
    bufs, pibs = [], []
    for cols, pi in wits:
        bs = [ctx.alloc(n) for _ in range(3)]
        for b, c in zip(bs, cols):
            b.upload(c)
        bufs.append(bs)
        pb = None
        if pi:
            pb = ctx.alloc(len(pi) + GARBAGE)
            pb.upload(fr_pack(list(pi) + [0xBAD] * GARBAGE))
        pibs.append(pb)
    return bufs, pibs


def _free(bufs, pibs):
    for b in [b for bs in bufs for b in bs] + [b for b in pibs if b is not None]:
        b.free()


def single(ctx, c, bufs, pib, pi_len):
    """typlonk_prove_compact on one witness: (return code, the filled proof) -- also for an unsatisfied witness"""
    from typlonk_amd import capi

    w = (C.c_void_p * 3)(*[b.handle.value for b in bufs])
    pr = capi.ProofCompact()
    rc = ctx.lib.typlonk_prove_compact(ctx.h, c.sid, c.cid, w, pib.handle if pib is not None else None, pi_len,
                                       C.byref(capi._cosets_arg(c.cosets)), C.byref(pr))
    return rc, capi.compact_dict(pr)


def _check_against_singles(ctx, c, wits, statuses_expected=None):
    """the batch of `wits` on the device against typlonk_prove_compact of each; returns (proofs, statuses)"""
    bufs, pibs = _upload(ctx, c.n, wits)
    lens = [len(pi) for _, pi in wits]
    try:
        proofs, st = ctx.prove_batch_compact(c.sid, c.cid, bufs, pibs, lens, c.cosets)
        assert len(proofs) == len(st) == len(wits)
        for k in range(len(wits)):
            rc, ref = single(ctx, c, bufs[k], pibs[k], lens[k])
            assert st[k] == rc, (k, st[k], rc)
            assert _bytes(proofs[k]) == _bytes(ref), k
        assert st == (statuses_expected if statuses_expected is not None else [0] * len(wits))
        return proofs, st
    finally:
        _free(bufs, pibs)


def _wits(c, count, lens, first=0, broken=()):
    """witness k: the chain under its own public values (pi_len cycling through `lens`) with blinders of variant k + 1"""
    out = []
    for k in range(first, first + count):
        pl = lens[k % len(lens)]
        pi = _pi_values(c.n, pl, 100 * c.log_n + k) if pl else []
        cols = c.columns(k + 1, pi if pi else None)
        if k in broken:
            cols[2][(c.n - 3) // 2] = _limbs(fr_unpack(cols[2][(c.n - 3) // 2])[0] + 1)     # a gate row that no longer holds
        out.append((cols, pi))
    return out


def _pis(wits):
    return [fr_pack(pi) if pi else None for _, pi in wits]


# ---- 1: equals single compact proofs -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [3, 6, 10, 16])
@pytest.mark.parametrize("count", [1, 2, 5])
def test_batch_equals_single_compact_proofs(ctx, log_n, count):
    c = Chain(ctx, log_n)
    try:
        lens = _pi_lens(log_n)
        # (count = 1 and 2 start the cycle at another length each, so that every length leads a batch somewhere)
        wits = _wits(c, count, lens, first=count)
        proofs, _ = _check_against_singles(ctx, c, wits)
        assert ctx.verify_compact(c.vk, proofs, pi=_pis(wits)).all()
    finally:
        c.free()


# ---- 2: equals the Python prover -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [3, 4, 5, 6])
def test_batch_equals_the_python_prover(ctx, log_n):
    c = PyCircuit(ctx, log_n)
    try:
        pis = [_pi_values(c.n, pl, 100 + pl) if pl else [] for pl in (0, 1, c.n)]
        wits = [([fr_pack(col) for col in c.columns(pi, seed=k)], pi) for k, pi in enumerate(pis)]
        bufs, pibs = _upload(ctx, c.n, wits)
        try:
            proofs, st = ctx.prove_batch_compact(c.sid, c.cid, bufs, pibs, [len(pi) for pi in pis], c.cosets)
        finally:
            _free(bufs, pibs)
        assert st == [0, 0, 0]
        for k, pi in enumerate(pis):
            exp = CR.prove(c.ref, c.columns(pi, seed=k), pi)
            assert exp["r_zeta"] == 0
            assert _to_python(proofs[k]) == {key: exp[key] for key in ("commit", "z_commit", "t_commit", "witness", "evals")}, k
            assert {key: fr_unpack(v)[0] for key, v in proofs[k]["challenges"].items()} == exp["challenges"], k
    finally:
        c.free()


# ---- 3: across a wave boundary ---------------------------------------------------------------------------------------------------
def test_batch_across_a_wave_boundary(ctx):
    """70 proofs at 2^4: a wave of 64 and one of 6, pi_len cycling through 0, 1 and n"""
    c = Chain(ctx, 4)
    try:
        wits = _wits(c, 70, (0, 1, c.n))
        proofs, _ = _check_against_singles(ctx, c, wits)
        assert ctx.verify_compact(c.vk, proofs, pi=_pis(wits)).all()
    finally:
        c.free()


# ---- 4: host form = device form ----------------------------------------------------------------------------------------------------
def test_host_and_device_forms_agree(ctx):
    c = Chain(ctx, 8)
    try:
        wits = _wits(c, 4, (0, 1, c.n))
        bufs, pibs = _upload(ctx, c.n, wits)
        try:
            dev, st_dev = ctx.prove_batch_compact(c.sid, c.cid, bufs, pibs, [len(pi) for _, pi in wits], c.cosets)
        finally:
            _free(bufs, pibs)
        host, st_host = ctx.prove_batch_compact_host(c.sid, c.cid, [w[0] for w in wits], _pis(wits), c.cosets)
        assert st_dev == st_host == [0] * 4
        assert [_bytes(d) for d in dev] == [_bytes(d) for d in host]
        # the host form of one witness is typlonk_prove_compact_host's proof
        one = ctx.prove_compact_host(c.sid, c.cid, wits[1][0], fr_pack(wits[1][1]), c.cosets)
        assert _bytes(host[1]) == _bytes(one)
        # NULL pi / pi_len arrays: no proof has public values
        plain = [(c.columns(k + 1), []) for k in range(2)]
        h2, st2 = ctx.prove_batch_compact_host(c.sid, c.cid, [w[0] for w in plain], None, c.cosets)
        h3, st3 = ctx.prove_batch_compact_host(c.sid, c.cid, [w[0] for w in plain], [None, None], c.cosets)
        assert st2 == st3 == [0, 0] and [_bytes(d) for d in h2] == [_bytes(d) for d in h3]
        bufs, pibs = _upload(ctx, c.n, plain)
        try:
            d2, st4 = ctx.prove_batch_compact(c.sid, c.cid, bufs, None, None, c.cosets)
        finally:
            _free(bufs, pibs)
        assert st4 == [0, 0] and [_bytes(d) for d in d2] == [_bytes(d) for d in h2]
    finally:
        c.free()


# ---- 5: an unsatisfied witness -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos", [0, 2])
def test_unsatisfied_witness_only_affects_its_proof(ctx, pos):
    from typlonk_amd.capi import ERR_UNSATISFIED, OK

    c = Chain(ctx, 6)
    try:
        exp = [ERR_UNSATISFIED if k == pos else OK for k in range(5)]
        good = _wits(c, 5, (0, 1, c.n))
        wits = _wits(c, 5, (0, 1, c.n), broken=(pos,))
        proofs, _ = _check_against_singles(ctx, c, wits, exp)       # its proof is what typlonk_prove_compact fills for it
        all_good, _ = _check_against_singles(ctx, c, good)
        assert [_bytes(proofs[k]) == _bytes(all_good[k]) for k in range(5)] == [k != pos for k in range(5)]   # the others: unchanged
        assert ctx.verify_compact(c.vk, proofs, pi=_pis(wits)).tolist() == [k != pos for k in range(5)]
    finally:
        c.free()


# ---- 6: verifies with only a vk ----------------------------------------------------------------------------------------------------
def test_fresh_context_verifies_the_batch_with_only_the_vk(built, ctx):
    import typlonk_amd
    from typlonk_amd.capi import Vk

    c = Chain(ctx, 10)
    try:
        wits = _wits(c, 6, (0, 1, c.n))
        proofs, _ = _check_against_singles(ctx, c, wits)
        vk = Vk.from_buffer_copy(bytes(c.vk))
    finally:
        c.free()
    fresh = typlonk_amd.Context(0)
    try:
        pis = _pis(wits)
        assert fresh.verify_compact(vk, proofs, pi=pis).tolist() == [True] * 6
        mixed = list(proofs)
        mixed[1] = _tamper_point(proofs[1], "witness", 0)
        mixed[4] = dict(proofs[4], evals=proofs[4]["evals"][:5] + [_limbs(fr_unpack(proofs[4]["evals"][5])[0] + 1)]
                        + proofs[4]["evals"][6:])
        assert fresh.verify_compact(vk, mixed, pi=pis).tolist() == [k not in (1, 4) for k in range(6)]
        other = list(pis)
        other[0] = fr_pack([1])                                  # proof 0 under another statement
        assert fresh.verify_compact(vk, proofs, pi=other).tolist() == [k != 0 for k in range(6)]
    finally:
        fresh.close()


# ---- 7: every refusal, and the context stays usable ---------------------------------------------------------------------------------
def test_refusals(ctx):
    """every refusal of include/typlonk.h except TYPLONK_ERR_DOMAIN (log_n > 24: typlonk_circuit_load accepts no such circuit to
    try it with)"""
    from typlonk_amd import capi
    from typlonk_amd.capi import ERR_INVALID_ARG, ERR_LENGTH, ERR_RANGE, ProofCompact, TyplonkError

    c = Chain(ctx, 5)
    lib = ctx.lib
    n = c.n
    wits = _wits(c, 2, (0, 1))
    bufs, pibs = _upload(ctx, n, wits)
    hosts = [w[0] for w in wits]
    ks = capi._cosets_arg(c.cosets)
    w = (C.c_void_p * 6)(*[b.handle.value for bs in bufs for b in bs])
    pip = (C.c_void_p * 2)(None, pibs[1].handle.value)
    lens = (C.c_size_t * 2)(0, 1)
    out = (ProofCompact * 2)()
    st = (C.c_int * 2)()

    def good_batch():
        proofs, stt = ctx.prove_batch_compact(c.sid, c.cid, bufs, pibs, [0, 1], c.cosets)
        assert stt == [0, 0]
        return [_bytes(p) for p in proofs]

    def code(fn):
        with pytest.raises(TyplonkError) as e:
            fn()
        return e.value.code

    def raw(wp=w, pp=pip, lp=lens, count=2, kp=C.byref(ks), op=out, sp=st, h=None, sid=None, cid=None):
        return lib.typlonk_prove_batch_compact(ctx.h if h is None else h, c.sid if sid is None else sid,
                                               c.cid if cid is None else cid, wp, pp, lp, count, kp, op, sp)

    try:
        want = good_batch()
        # count == 0 is a no-op, whatever else is null
        assert ctx.prove_batch_compact(c.sid, c.cid, [], None, None, c.cosets) == ([], [])
        assert lib.typlonk_prove_batch_compact(ctx.h, c.sid, c.cid, None, None, None, 0, None, None, None) == 0
        assert lib.typlonk_prove_batch_compact_host(ctx.h, c.sid, c.cid, None, n, None, None, 0, None, None, None) == 0
        # null arguments
        assert raw(op=None) == ERR_INVALID_ARG
        assert raw(sp=None) == ERR_INVALID_ARG
        assert raw(kp=None) == ERR_INVALID_ARG
        assert raw(wp=None) == ERR_INVALID_ARG
        assert lib.typlonk_prove_batch_compact(None, c.sid, c.cid, w, pip, lens, 2, C.byref(ks), out, st) == ERR_INVALID_ARG
        assert good_batch() == want
        # unknown circuit / SRS
        assert code(lambda: ctx.prove_batch_compact(c.sid, 99999, bufs, pibs, [0, 1], c.cosets)) == ERR_INVALID_ARG
        assert code(lambda: ctx.prove_batch_compact(99999, c.cid, bufs, pibs, [0, 1], c.cosets)) == ERR_INVALID_ARG
        # a null wire column, device and host form
        holey = (C.c_void_p * 6)(*[b.handle.value for bs in bufs for b in bs])
        holey[4] = None
        assert raw(wp=holey) == ERR_INVALID_ARG
        hp = (C.POINTER(C.c_uint64) * 6)()
        assert lib.typlonk_prove_batch_compact_host(ctx.h, c.sid, c.cid, hp, n, None, None, 2, C.byref(ks), out, st) == ERR_INVALID_ARG
        # pi_len[k] != 0 with a null pi array / a null pi[k]
        assert raw(pp=None) == ERR_INVALID_ARG
        assert raw(pp=(C.c_void_p * 2)(pibs[1].handle.value, None)) == ERR_INVALID_ARG
        assert raw(pp=None, lp=None) == 0                                        # (NULL pi_len = all 0: accepted)
        assert good_batch() == want
        # a wire buffer shorter than n, a pi buffer shorter than pi_len[k]
        short_col = ctx.alloc(n - 1)
        try:
            assert code(lambda: ctx.prove_batch_compact(c.sid, c.cid, [bufs[0], [bufs[1][0], short_col, bufs[1][2]]], pibs,
                                                        [0, 1], c.cosets)) == ERR_RANGE
        finally:
            short_col.free()
        assert code(lambda: ctx.prove_batch_compact(c.sid, c.cid, bufs, pibs, [0, 1 + GARBAGE + 1], c.cosets)) == ERR_RANGE
        # pi_len[k] > n, an SRS shorter than n, host rows != n
        big = ctx.alloc(n + 2)
        try:
            assert code(lambda: ctx.prove_batch_compact(c.sid, c.cid, bufs, [None, big], [0, n + 1], c.cosets)) == ERR_LENGTH
        finally:
            big.free()
        assert code(lambda: ctx.prove_batch_compact_host(c.sid, c.cid, hosts, [None, np.zeros((n + 1, 4), dtype=np.uint64)],
                                                         c.cosets)) == ERR_LENGTH
        short = ctx.srs_generate(_limbs(0x5EC2E7D00D51), n - 1)
        assert code(lambda: ctx.prove_batch_compact(short, c.cid, bufs, pibs, [0, 1], c.cosets)) == ERR_LENGTH
        ctx.srs_free(short)
        assert code(lambda: ctx.prove_batch_compact_host(c.sid, c.cid, [[x[:-1] for x in cols] for cols in hosts], None,
                                                         c.cosets)) == ERR_LENGTH
        assert code(lambda: ctx.prove_batch_compact_host(c.sid, c.cid, [[np.vstack([x, x[:1]]) for x in cols] for cols in hosts],
                                                         None, c.cosets)) == ERR_LENGTH
        with pytest.raises(ValueError):
            ctx.prove_batch_compact_host(c.sid, c.cid, [hosts[0], [hosts[1][0], hosts[1][1], hosts[1][2][:-1]]], None, c.cosets)
        assert good_batch() == want
        # a sharded SRS (a folding communicator is a shard on a context with a communicator: the same condition)
        shard = ctx.srs_generate(_limbs(0x5EC2E7D00D51), n + 3)
        ctx.srs_set_shard(shard, 0, 2 * n)
        assert code(lambda: ctx.prove_batch_compact(shard, c.cid, bufs, pibs, [0, 1], c.cosets)) == ERR_INVALID_ARG
        ctx.srs_free(shard)
        # a round-by-round prover open on the context refuses both forms; once freed, they work again
        pr = C.c_void_p()
        cxy = ((C.c_uint64 * 12) * 3)()
        cinf = (C.c_uint8 * 3)()
        w3 = (C.c_void_p * 3)(*[b.handle.value for b in bufs[0]])
        assert lib.typlonk_prover_round1(ctx.h, c.sid, c.cid, w3, None, C.byref(pr), C.byref(cxy), C.byref(cinf)) == 0
        try:
            assert code(lambda: ctx.prove_batch_compact(c.sid, c.cid, bufs, pibs, [0, 1], c.cosets)) == ERR_INVALID_ARG
            assert code(lambda: ctx.prove_batch_compact_host(c.sid, c.cid, hosts, _pis(wits), c.cosets)) == ERR_INVALID_ARG
        finally:
            lib.typlonk_prover_free(pr)
        assert good_batch() == want
        host, sth = ctx.prove_batch_compact_host(c.sid, c.cid, hosts, _pis(wits), c.cosets)
        assert sth == [0, 0] and [_bytes(p) for p in host] == want
    finally:
        _free(bufs, pibs)
        c.free()


# ---- 8: existing callers untouched ---------------------------------------------------------------------------------------------------
def test_existing_entry_points_are_unchanged_after_a_compact_batch(ctx):
    """the arena and the tables are shared: prove_batch (reference shape) and prove_compact return after a compact batch what
    they returned before it"""
    from test_gpu_prove_batch import same

    c = Chain(ctx, 8)
    try:
        wits = _wits(c, 5, (0, 1, c.n))
        bufs, pibs = _upload(ctx, c.n, wits)
        full = []                                               # the reference shape's full public-input columns
        for _, pi in wits:
            b = None
            if pi:
                b = ctx.alloc(c.n)
                b.upload(fr_pack(list(pi) + [0] * (c.n - len(pi))))
            full.append(b)
        try:
            lens = [len(pi) for _, pi in wits]
            ref_before, st_before = ctx.prove_batch(c.sid, c.cid, bufs, full, c.cosets)
            one_before = [single(ctx, c, bufs[k], pibs[k], lens[k]) for k in range(5)]
            batch, st = ctx.prove_batch_compact(c.sid, c.cid, bufs, pibs, lens, c.cosets)
            ref_after, st_after = ctx.prove_batch(c.sid, c.cid, bufs, full, c.cosets)
            one_after = [single(ctx, c, bufs[k], pibs[k], lens[k]) for k in range(5)]
            again, st2 = ctx.prove_batch_compact(c.sid, c.cid, bufs, pibs, lens, c.cosets)
        finally:
            _free(bufs, pibs + full)
        assert st_before == st_after == st == st2 == [0] * 5
        assert all(same(a, b) for a, b in zip(ref_before, ref_after))
        assert [(rc, _bytes(d)) for rc, d in one_before] == [(rc, _bytes(d)) for rc, d in one_after]
        assert [_bytes(d) for d in batch] == [_bytes(d) for d in again] == [_bytes(d) for _, d in one_before]
    finally:
        c.free()


# ---- 9: 2^20 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.slow
def test_batch_at_2_20_equals_single_compact_proofs(built):
    """five proofs of 2^20 rows: a wave of four and a wave of one"""
    from conftest import need_resources

    import typlonk_amd

    need_resources(host_gib=8, hbm_gib=24)
    ctx = typlonk_amd.Context(0)
    try:
        c = Chain(ctx, 20)
        try:
            wits = [(c.columns(k + 1), []) for k in range(5)]
            _check_against_singles(ctx, c, wits)
        finally:
            c.free()
    finally:
        ctx.close()


# ---- 10: the C++ mirror --------------------------------------------------------------------------------------------------------------
def test_mirror_prove_batch_compact(built):
    """tests/cpp/test_prove_batch_compact_host: plonk::CompiledCircuit::prove_batch_compact (typlonk_prove_batch_compact_host)
    equals the mirror's prove_compact on each witness, statuses included, and verifies in a context holding only the vk"""
    import os
    import subprocess

    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "test_prove_batch_compact_host")
    r = subprocess.run([exe, "6"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "prove_batch_compact agrees with prove_compact ok" in r.stdout
