"""The wire format on the GPU: the decode / encode kernels of csrc/point_codec.hip against the Python statement
(tests/point_codec_ref.py) and against the library's own host path word for word; a compressed SRS round trip; compact proofs
as bytes through typlonk_verify_compact_bytes; every refusal.  Malformed input is data the kernel rejects: nothing here reads
or writes out of bounds."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import point_codec_ref as W
from helpers import O, fr_pack, g1_pack, g1_unpack_one
from test_gpu_compact import Chain, _limbs
from test_gpu_prove_batch_compact import _free, _pis, _upload, _wits

pytestmark = pytest.mark.gpu

P, R = O.P, O.R
INF = bytes([0xC0]) + bytes(47)


def _x_bytes(x, flags=0x80):
    b = bytearray(x.to_bytes(48, "big"))
    b[0] |= flags
    return bytes(b)


@functools.lru_cache(maxsize=None)
def _cofactor_points(count=16):
    """[r] P' for the first `count` curve points P' = (x, .) from x = 0 up that lie outside G: order dividing the cofactor"""
    out, x = [], 0
    while len(out) < count:
        p = W.curve_point_at(x)
        x += 1
        if p is None:
            continue
        q = W.g1_mul_plain(p, R)
        if q is not None:
            out.append((p, q))
    return out


@functools.lru_cache(maxsize=None)
def _seeded_set():
    """(blobs, classes): >= 2000 distinct valid points and >= 64 distinct inputs of every reject class"""
    rng = np.random.default_rng(20261)
    valid, pt = [], O.g1_mul(O.G1, 0xA5A5A5A5)
    step = O.g1_mul(O.G1, int(rng.integers(1, 1 << 62)))
    for i in range(1008):
        pt = O.g1_add(pt, step)
        valid += [pt, O.g1_neg(pt)]
    valid += [O.G1, O.g1_neg(O.G1), None]
    cases = [(W.g1_compress(p), 0) for p in valid]
    # encoding: the compression bit clear; infinity with stray bits
    for p in valid[:40]:
        b = W.g1_compress(p)
        cases.append((bytes([b[0] & 0x7F]) + b[1:], W.ENCODING))
    for i in range(40):
        b = bytearray(INF)
        b[int(rng.integers(0, 48))] |= 1 << int(rng.integers(0, 6))     # (bits 6, 7 of byte 0 stay as they are)
        cases.append((bytes(b), W.ENCODING))
    cases.append((bytes([0xE0]) + bytes(47), W.ENCODING))
    # x >= p
    top = (1 << 381) - 1 - P
    for i in range(70):
        d = i if i < 8 else int(rng.integers(0, 1 << 62)) * int(rng.integers(1, 1 << 62)) % top
        cases.append((_x_bytes(P + d, 0xA0 if i & 1 else 0x80), W.X_RANGE))
    cases.append((_x_bytes(P + top), W.X_RANGE))
    # x^3 + 4 not a square
    found = 0
    while found < 70:
        x = int.from_bytes(rng.bytes(48), "big") % P
        if W.curve_point_at(x) is None:
            cases.append((_x_bytes(x, 0xA0 if found & 1 else 0x80), W.NOT_ON_CURVE))
            found += 1
    cases.append((_x_bytes(1), W.NOT_ON_CURVE))
    # on the curve, outside the subgroup: curve points at small x, their cofactor-order multiples, G-multiples + those
    for i, (p, q) in enumerate(_cofactor_points()):
        for o in (p, q, O.g1_add(O.g1_mul(O.G1, 1000 + i), q), O.g1_add(valid[i], p)):
            cases += [(W.g1_compress(o), W.NOT_IN_SUBGROUP), (W.g1_compress(O.g1_neg(o)), W.NOT_IN_SUBGROUP)]
    order = rng.permutation(len(cases))
    return [cases[i][0] for i in order], [cases[i][1] for i in order]


def test_kernel_decode_equals_the_python_statement(ctx):
    blobs, classes = _seeded_set()
    by_class = {c: {b for b, k in zip(blobs, classes) if k == c} for c in range(5)}
    assert len(by_class[0]) >= 2000 and all(len(by_class[c]) >= 64 for c in (1, 2, 3, 4)), {c: len(s) for c, s in by_class.items()}
    xy, inf, st = ctx.g1_decompress(b"".join(blobs))
    checked = 0
    for i, (b, cls) in enumerate(zip(blobs, classes)):
        est, ept = W.g1_decompress(b)
        assert est == cls, (i, est, cls)
        assert (int(st[i]), g1_unpack_one(xy[i], inf[i])) == (est, ept), (i, b.hex())
        checked += 1
    assert checked == len(blobs)
    # the skip flag skips the last check only
    xy2, inf2, st2 = ctx.g1_decompress(b"".join(blobs), skip_subgroup=True)
    for i, (b, cls) in enumerate(zip(blobs, classes)):
        if cls == W.NOT_IN_SUBGROUP:
            assert (int(st2[i]), g1_unpack_one(xy2[i], inf2[i])) == W.g1_decompress(b, True) and st2[i] == 0
        else:
            assert st2[i] == st[i] and (xy2[i] == xy[i]).all() and inf2[i] == inf[i]
    # the kernel's compression of what it decoded is the input again
    from typlonk_amd import capi

    good = [i for i, c in enumerate(classes) if c == 0]
    assert capi.g1_compress(xy[good], inf[good]) == b"".join(blobs[i] for i in good)


def test_kernel_equals_the_host_path_word_for_word(ctx):
    """>= 4096 inputs of all classes: device-made valid encodings, and mutations of them"""
    from typlonk_amd import capi

    rng = np.random.default_rng(77)
    sid = ctx.srs_generate(_limbs(0x1234567), 3000)
    try:
        valid = ctx.srs_download_compressed(sid)
    finally:
        ctx.srs_free(sid)
    blobs = [valid[48 * i:48 * i + 48] for i in range(3000)]
    seeded, _ = _seeded_set()
    blobs += seeded[:400]
    for i in range(1200):
        b = bytearray(blobs[i])
        kind = i % 6
        if kind == 0:
            b[0] &= 0x7F
        elif kind == 1:
            b[0] |= 0x40
        elif kind == 2:
            b[0] ^= 0x20                                                 # the other root: still valid
        elif kind == 3:
            b = bytearray(_x_bytes(P + int(rng.integers(0, 1 << 40))))
        else:
            b = bytearray(_x_bytes(int.from_bytes(rng.bytes(48), "big") % P, 0xA0 if i & 8 else 0x80))   # off the curve, or off G
        blobs.append(bytes(b))
    assert len(set(blobs)) >= 4096
    data = b"".join(blobs)
    for skip in (False, True):
        dxy, dinf, dst = ctx.g1_decompress(data, skip_subgroup=skip)
        hxy, hinf, hst = capi.g1_decompress(data, skip_subgroup=skip)
        assert dxy.shape == (len(blobs), 12)
        assert (dst == hst).all() and (dinf == hinf).all() and (dxy == hxy).all()
        if not skip:
            assert set(int(s) for s in dst) == {0, 1, 2, 3, 4}


def _rand_scalars(n, seed):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    s[:, 3] >>= np.uint64(2)                                             # < 2^253 < r: a valid residue
    return s


def _srs_round_trip(ctx, n, secret=2):
    sid = ctx.srs_generate(_limbs(secret), n)
    sid2 = None
    try:
        data = ctx.srs_download_compressed(sid)
        assert len(data) == 48 * n
        sid2 = ctx.srs_load_compressed(data)
        assert ctx.srs_len(sid2) == n
        a, b = ctx.srs_download(sid), ctx.srs_download(sid2)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and not a[1].any()
        sc = _rand_scalars(n, n)
        r1, r2 = ctx.msm(sid, sc), ctx.msm(sid2, sc)
        assert (r1[0] == r2[0]).all() and r1[1] == r2[1] == 0
        assert ctx.srs_download_compressed(sid2, 5, 7) == data[48 * 5:48 * 12]
        return data, a
    finally:
        ctx.srs_free(sid)
        if sid2 is not None:
            ctx.srs_free(sid2)


def test_srs_round_trip_and_rejects(ctx):
    from typlonk_amd import capi

    n = (1 << 16) + 3
    data, (xy, inf) = _srs_round_trip(ctx, n)
    # the first points are G, 2G, 4G: the kernel's compression is the Python one
    assert data[:144] == b"".join(W.g1_compress(O.g1_mul(O.G1, k)) for k in (1, 2, 4))
    sc = _rand_scalars(n, 5)
    # an identity inside
    j = 40000
    with_inf = data[:48 * j] + INF + data[48 * j + 48:]
    sid = ctx.srs_load_compressed(with_inf)
    exy, einf = xy.copy(), inf.copy()
    exy[j], einf[j] = g1_pack([None])[0][0], 1
    ref = ctx.srs_load(exy, einf)
    try:
        got = ctx.srs_download(sid)
        assert (got[0] == exy).all() and (got[1] == einf).all()
        assert ctx.srs_download_compressed(sid) == with_inf
        r1, r2 = ctx.msm(sid, sc), ctx.msm(ref, sc)
        assert (r1[0] == r2[0]).all() and r1[1] == r2[1]
    finally:
        ctx.srs_free(sid)
        ctx.srs_free(ref)
    # a cofactor-order point at index i: no SRS, the lowest bad index, its class in the error text
    q = _cofactor_points()[1][1]
    for i, also in ((12345, None), (n - 1, None), (777, 60000)):
        bad = bytearray(data)
        bad[48 * i:48 * i + 48] = W.g1_compress(q)
        if also is not None:
            bad[48 * also:48 * also + 48] = _x_bytes(P)                  # a later bad point does not change first_bad
        probe = ctx.srs_generate(_limbs(3), 1)                           # the id the refused load would have got is the next one
        ctx.srs_free(probe)
        with pytest.raises(capi.TyplonkError) as e:
            ctx.srs_load_compressed(bytes(bad))
        assert e.value.code == capi.ERR_INVALID_ARG and e.value.first_bad == i
        assert "subgroup" in str(e.value)
        for guess in (probe + 1, probe + 2):
            with pytest.raises(capi.TyplonkError):
                ctx.srs_len(guess)
        if also is None:
            sid = ctx.srs_load_compressed(bytes(bad), skip_subgroup=True)    # with the skip flag it loads
            try:
                got = ctx.srs_download(sid, i, 1)
                assert g1_unpack_one(got[0][0], got[1][0]) == q
            finally:
                ctx.srs_free(sid)
    bad = bytearray(data)
    bad[48 * 9:48 * 10] = _x_bytes(1)
    with pytest.raises(capi.TyplonkError) as e:
        ctx.srs_load_compressed(bytes(bad), skip_subgroup=True)
    assert e.value.first_bad == 9 and "curve" in str(e.value)


@pytest.mark.slow
def test_srs_round_trip_at_2_20(ctx):
    from conftest import need_resources

    need_resources(host_gib=2, hbm_gib=2)
    _srs_round_trip(ctx, 1 << 20, secret=0xC0FFEE)


# ---- proofs ----
def _batch(ctx, c, count):
    lens = (0, 1, 3000) if c.log_n >= 16 else (0, 1, c.n)
    wits = _wits(c, count, lens)
    bufs, pibs = _upload(ctx, c.n, wits)
    try:
        proofs, st = ctx.prove_batch_compact(c.sid, c.cid, bufs, pibs, [len(pi) for _, pi in wits], c.cosets)
    finally:
        _free(bufs, pibs)
    assert st == [0] * count
    return proofs, _pis(wits)


@pytest.mark.parametrize("log_n,count", [(6, 8), (16, 64)])
def test_verify_compact_bytes(ctx, log_n, count):
    import typlonk_amd
    from typlonk_amd import capi

    c = Chain(ctx, log_n)
    try:
        proofs, pis = _batch(ctx, c, count)
        vk = c.vk
    finally:
        c.free()
    data = b"".join(capi.proof_to_bytes(p) for p in proofs)
    assert len(data) == 656 * count
    assert ctx.verify_compact(vk, proofs, pi=pis).all()
    assert ctx.verify_compact_bytes(vk, data, pi=pis).tolist() == [True] * count
    # device decode = host decode = the structs
    dev, dst = ctx.proofs_from_bytes(data)
    host, hst = capi.proofs_from_bytes(data)
    assert not dst.any() and not hst.any()
    for d, h, p in zip(dev, host, proofs):
        assert bytes(capi.compact_struct(d)) == bytes(capi.compact_struct(h))
        for key in ("commit", "t_commit", "witness"):
            assert all((a[0] == b[0]).all() and a[1] == b[1] for a, b in zip(d[key], p[key]))
        assert (d["z_commit"][0] == p["z_commit"][0]).all() and (np.array(d["evals"]) == np.array(p["evals"])).all()
        assert capi.proof_to_bytes(d) == capi.proof_to_bytes(p)
    # one proof spoiled at a time: exactly its ok is 0
    q = W.g1_compress(_cofactor_points()[2][1])
    k1, k2, k3, k4 = 1, count // 2, count - 1, 3
    spoil = {
        "sign": (k1, 48 * 7, None, (0, 0)),                              # W_z with the other root: decodes, fails
        "cofactor": (k2, 48 * 4, q, (W.NOT_IN_SUBGROUP, 4)),             # t_lo
        "eval": (k3, 432 + 32 * 4, R.to_bytes(32, "little"), (W.SCALAR_RANGE, 13)),
        "x_range": (k4, 48 * 2, _x_bytes(P + 1), (W.X_RANGE, 2)),        # [c]
    }
    for name, (k, off, repl, status) in spoil.items():
        b = bytearray(data)
        at = 656 * k + off
        if repl is None:
            b[at] ^= 0x20
        else:
            b[at:at + len(repl)] = repl
        ok = ctx.verify_compact_bytes(vk, bytes(b), pi=pis)
        assert ok.tolist() == [i != k for i in range(count)], name
        _, st = ctx.proofs_from_bytes(bytes(b))
        assert [capi.decode_status(int(s)) for s in st] == [status if i == k else (0, 0) for i in range(count)], name
    # all four at once
    b = bytearray(data)
    for name, (k, off, repl, status) in spoil.items():
        at = 656 * k + off
        if repl is None:
            b[at] ^= 0x20
        else:
            b[at:at + len(repl)] = repl
    bad = {k1, k2, k3, k4}
    assert ctx.verify_compact_bytes(vk, bytes(b), pi=pis).tolist() == [i not in bad for i in range(count)]
    # with the skip flag the cofactor-order point decodes -- and the proof still fails
    assert not ctx.verify_compact_bytes(vk, bytes(b), pi=pis, skip_subgroup=True)[k2]
    # a fresh context holding only the key that went through its bytes
    vkb = capi.vk_to_bytes(vk)
    assert len(vkb) == 628
    vk2 = capi.vk_from_bytes(vkb)
    assert capi.vk_to_bytes(vk2) == vkb and list(vk2.g2s_xy) == list(vk.g2s_xy) and vk2.log_n == vk.log_n
    assert all(list(vk2.commit_xy[i]) == list(vk.commit_xy[i]) for i in range(8)) and list(vk2.srs0_xy) == list(vk.srs0_xy)
    fresh = typlonk_amd.Context(0)
    try:
        assert fresh.verify_compact_bytes(vk2, data, pi=pis).all()
        assert fresh.verify_compact_bytes(vk2, bytes(b), pi=pis).tolist() == [i not in bad for i in range(count)]
    finally:
        fresh.close()


def test_refusals(ctx):
    from typlonk_amd import capi

    lib = ctx.lib
    u8 = (C.c_uint8 * 656)()
    sid = C.c_uint32()
    # null arguments
    assert lib.typlonk_g1_decompress(ctx.h, None, 1, 0, None, None, None) == capi.ERR_INVALID_ARG
    assert lib.typlonk_srs_load_compressed(ctx.h, None, 48, 0, C.byref(sid), None) == capi.ERR_INVALID_ARG
    assert lib.typlonk_srs_load_compressed(ctx.h, u8, 48, 0, None, None) == capi.ERR_INVALID_ARG
    assert lib.typlonk_srs_load_compressed(None, u8, 48, 0, C.byref(sid), None) == capi.ERR_INVALID_ARG
    assert lib.typlonk_srs_load_compressed(ctx.h, u8, 47, 0, C.byref(sid), None) == capi.ERR_LENGTH
    assert lib.typlonk_srs_download_compressed(ctx.h, 999999, 0, 1, u8) == capi.ERR_INVALID_ARG
    assert lib.typlonk_srs_download_compressed(None, 1, 0, 1, u8) == capi.ERR_INVALID_ARG
    assert lib.typlonk_proof_compact_from_bytes(ctx.h, None, 1, 0, None, None) == capi.ERR_INVALID_ARG
    assert lib.typlonk_verify_compact_bytes(ctx.h, None, None, 1, None, None, 0, None) == capi.ERR_INVALID_ARG
    assert lib.typlonk_verify_compact_bytes(None, None, None, 1, None, None, 0, None) == capi.ERR_INVALID_ARG
    # count = 0: a no-op
    assert lib.typlonk_g1_decompress(ctx.h, None, 0, 0, None, None, None) == 0
    assert lib.typlonk_proof_compact_from_bytes(ctx.h, None, 0, 0, None, None) == 0
    assert lib.typlonk_verify_compact_bytes(ctx.h, None, None, 0, None, None, 0, None) == 0
    assert ctx.g1_decompress(b"")[0].shape == (0, 12)
    empty = ctx.srs_load_compressed(b"")
    assert ctx.srs_len(empty) == 0 and ctx.srs_download_compressed(empty) == b""
    ctx.srs_free(empty)
    small = ctx.srs_load_compressed(W.g1_compress(O.G1) * 3)
    try:
        with pytest.raises(capi.TyplonkError) as e:
            ctx.srs_download_compressed(small, 2, 2)
        assert e.value.code == capi.ERR_RANGE
        assert ctx.srs_download_compressed(small, 3, 0) == b""
    finally:
        ctx.srs_free(small)
    # wrong lengths in the Python layer
    for call in (lambda: ctx.g1_decompress(bytes(49)), lambda: ctx.proofs_from_bytes(bytes(655)),
                 lambda: ctx.verify_compact_bytes(capi.Vk(), bytes(657)), lambda: capi.vk_from_bytes(bytes(627)),
                 lambda: ctx.verify_compact_bytes(capi.Vk(), bytes(656), pi=[None, None])):
        with pytest.raises(ValueError):
            call()
    # a key with a bad log_n: as bytes, and as a struct handed to the verifier
    c = Chain(ctx, 4)
    try:
        proofs, pis = _batch(ctx, c, 2)
        vk = c.vk
    finally:
        c.free()
    data = b"".join(capi.proof_to_bytes(p) for p in proofs)
    vkb = capi.vk_to_bytes(vk)
    with pytest.raises(capi.TyplonkError) as e:
        capi.vk_from_bytes((25).to_bytes(4, "little") + vkb[4:])
    assert e.value.code == capi.ERR_DOMAIN
    bad_vk = capi.Vk.from_buffer_copy(bytes(vk))
    bad_vk.log_n = 0
    for blob in (data, bytes(656)):                                      # also when no proof decodes
        with pytest.raises(capi.TyplonkError) as e:
            ctx.verify_compact_bytes(bad_vk, blob)
        assert e.value.code == capi.ERR_DOMAIN
    # a key the verifier refuses is refused whichever proofs decode -- all, some or none -- and with the verifier's code
    off = capi.Vk.from_buffer_copy(bytes(vk))
    off.commit_xy[2][6] ^= 1
    off.commit_inf[2] = 0
    g2bad = capi.Vk.from_buffer_copy(bytes(vk))
    g2bad.g2s_xy[12] ^= 1
    for blob in (data, bytes(656) + data[656:], bytes(2 * 656)):
        for k in (off, g2bad):
            with pytest.raises(capi.TyplonkError) as e:
                ctx.verify_compact_bytes(k, blob)
            assert e.value.code == capi.ERR_INVALID_ARG
            with pytest.raises(capi.TyplonkError) as e:
                ctx.verify_compact(k, proofs)
            assert e.value.code == capi.ERR_INVALID_ARG
    # a public-input column longer than n: also when it belongs to a proof that does not decode
    for blob in (data, bytes(656) + data[656:]):
        with pytest.raises(capi.TyplonkError) as e:
            ctx.verify_compact_bytes(vk, blob, pi=[np.zeros((c.n + 1, 4), dtype=np.uint64), None])
        assert e.value.code == capi.ERR_LENGTH
    assert ctx.verify_compact_bytes(vk, data, pi=pis).all()              # the context is fine after the refusals
    assert ctx.verify_compact_bytes(vk, bytes(656) + data[656:], pi=pis).tolist() == [False, True]


def test_mirror_wire_format(built):
    """tests/cpp/test_wire_host: plonk::proof_to_bytes / proofs_from_bytes / vk_to_bytes / vk_from_bytes / verify_compact_bytes"""
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "test_wire_host")
    r = subprocess.run([exe, "6"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wire format round trip ok" in r.stdout
