"""The wire format on the CPU: the library's host path (ctx = NULL) of the compressed-point codec and the byte forms of compact
proofs and verifying keys, against the Python statement (tests/point_codec_ref.py), the published ZCash / IETF anchors and
the Python prover and verifier of tests/compact_ref.py."""
import functools

import numpy as np
import pytest

import compact_ref as CR
import point_codec_ref as W
from helpers import O, fr_pack, fr_unpack, g1_pack, g1_unpack_one
from oracle import pairing as PR

P, R = O.P, O.R

G1_HEX = "97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb"
INF = bytes([0xC0]) + bytes(47)


@pytest.fixture(scope="module")
def capi(built):
    from typlonk_amd import capi as c

    c.load_library()
    return c


def _decode(capi, blobs, skip=False):
    """[(status, point)] of the native host path"""
    xy, inf, st = capi.g1_decompress(b"".join(blobs), skip_subgroup=skip)
    return [(int(st[i]), g1_unpack_one(xy[i], inf[i])) for i in range(len(blobs))], xy, inf


def _x_bytes(x, flags=0x80):
    b = bytearray(x.to_bytes(48, "big"))
    b[0] |= flags
    return bytes(b)


@functools.lru_cache(maxsize=None)
def cofactor_points():
    """points of order dividing the cofactor, not the identity: [r] P' for curve points P' outside G"""
    out = []
    for x in (0, 4, 5, 6, 8):
        p = W.curve_point_at(x)
        assert p is not None and O.g1_is_on_curve(p) and not W.g1_in_subgroup(p), x
        q = W.g1_mul_plain(p, R)
        assert q is not None and O.g1_is_on_curve(q) and W.g1_mul_plain(q, W.COFACTOR) is None
        out += [p, q]
    return out


def test_published_anchors(capi):
    assert W.g1_compress(O.G1).hex() == G1_HEX and (O.GX | 1 << 383).to_bytes(48, "big").hex() == G1_HEX
    assert O.GY <= W.HALF                                 # the generator's sign bit is clear: the top byte is 0x97 = 0x80 | 0x17
    xy, inf = g1_pack([O.G1, None])
    assert capi.g1_compress(xy, inf) == bytes.fromhex(G1_HEX) + INF
    assert capi.g1_compress(xy[:1]) == bytes.fromhex(G1_HEX)
    g2 = W.g2_compress(PR.G2)
    assert g2.hex().startswith("93e02b6052719f60")
    assert g2[:48] == (PR.G2[0][1] | 1 << 383).to_bytes(48, "big") and g2[48:] == PR.G2[0][0].to_bytes(48, "big")
    assert W.g2_decompress(g2) == (0, PR.G2)
    assert W.g2_decompress(W.g2_compress(PR.g2_neg(PR.G2))) == (0, PR.g2_neg(PR.G2))
    # 80 00 .. 00 is the order-3 point (0, 2), not infinity
    got, _, _ = _decode(capi, [_x_bytes(0), _x_bytes(0, 0xA0), INF], skip=True)
    assert got == [(0, (0, 2)), (0, (0, P - 2)), (0, None)]
    assert W.g1_mul_plain((0, 2), 3) is None


def test_native_decode_equals_the_python_one_on_valid_points(capi):
    pts = [O.g1_mul(O.G1, k) for k in (1, 2, 3, 5, 7, 0xDEADBEEF, R - 1, R - 2, 2 ** 200 + 9)]
    pts += [O.g1_neg(p) for p in pts] + [None]
    assert {p[1] > W.HALF for p in pts if p} == {True, False}       # both sign bits
    blobs = [W.g1_compress(p) for p in pts]
    got, xy, inf = _decode(capi, blobs)
    assert got == [(0, p) for p in pts] == [W.g1_decompress(b) for b in blobs]
    # compress(decompress(b)) == b, and the C-ABI identity is (0, 1, inf)
    assert capi.g1_compress(xy, inf) == b"".join(blobs)
    exy, einf = g1_pack(pts)
    assert xy.tolist() == exy.tolist() and inf.tolist() == einf.tolist()
    # (0, +-2) decode only without the subgroup check
    small = [_x_bytes(0), _x_bytes(0, 0xA0)]
    assert [s for s, _ in _decode(capi, small)[0]] == [W.NOT_IN_SUBGROUP] * 2
    assert _decode(capi, small, skip=True)[0] == [W.g1_decompress(b, True) for b in small] == [(0, (0, 2)), (0, (0, P - 2))]


def test_every_reject_class(capi):
    g = bytearray.fromhex(G1_HEX)
    cases = []                                           # (bytes, class)
    cases.append((bytes([g[0] & 0x7F]) + bytes(g[1:]), W.ENCODING))              # compression bit clear
    cases.append((bytes(48), W.ENCODING))
    cases.append((bytes([0xE0]) + bytes(47), W.ENCODING))                        # infinity with the sign bit
    cases.append((bytes([0xC0]) + bytes(46) + b"\x01", W.ENCODING))              # infinity with a stray low bit
    cases.append((bytes([0xC1]) + bytes(47), W.ENCODING))
    cases.append((bytes([0x40]) + bytes(47), W.ENCODING))                        # infinity without the compression bit
    for d in (0, 1, 2, 1000, (1 << 381) - 1 - P):
        cases.append((_x_bytes(P + d), W.X_RANGE))
        cases.append((_x_bytes(P + d, 0xA0), W.X_RANGE))
    xn = W.smallest_non_residue_x()
    assert xn == 1 and W.curve_point_at(xn) is None      # 1 + 4 = 5 is not a square mod p
    cases.append((_x_bytes(xn), W.NOT_ON_CURVE))
    cases.append((_x_bytes(xn, 0xA0), W.NOT_ON_CURVE))
    cases.append((_x_bytes(P - 1), W.NOT_ON_CURVE if W.curve_point_at(P - 1) is None else W.NOT_IN_SUBGROUP))
    outside = list(cofactor_points())
    outside += [O.g1_add(O.g1_mul(O.G1, 12345 + i), q) for i, q in enumerate(cofactor_points())]   # G-multiple + cofactor-order
    for q in outside:
        assert O.g1_is_on_curve(q) and not W.g1_in_subgroup(q)
        cases += [(W.g1_compress(q), W.NOT_IN_SUBGROUP), (W.g1_compress(O.g1_neg(q)), W.NOT_IN_SUBGROUP)]
    blobs = [b for b, _ in cases]
    got, xy, inf = _decode(capi, blobs)
    assert [s for s, _ in got] == [c for _, c in cases] == [W.g1_decompress(b)[0] for b in blobs]
    # a rejected slot holds the C-ABI identity
    ixy, iinf = g1_pack([None])
    assert all(xy[i].tolist() == ixy[0].tolist() and inf[i] == 1 for i in range(len(blobs)))
    # with SKIP_SUBGROUP the last class -- and only it -- decodes
    got, _, _ = _decode(capi, blobs, skip=True)
    for (st, pt), (b, cls) in zip(got, cases):
        assert (st, pt) == W.g1_decompress(b, True)
        assert st == (0 if cls == W.NOT_IN_SUBGROUP else cls)
    assert len({b for b, c in cases if c == W.NOT_IN_SUBGROUP}) >= 30


def test_compress_refuses_what_has_no_encoding(capi):
    xy, _ = g1_pack([O.G1])
    bad = xy.copy()
    bad[0, :6] = np.array(_p_limbs(), dtype=np.uint64)           # x = p: not a canonical residue
    with pytest.raises(capi.TyplonkError) as e:
        capi.g1_compress(bad)
    assert e.value.code == capi.ERR_INVALID_ARG
    # a refused call leaves the output as it was, also when the bad point is not the first
    two = np.vstack([xy, bad])
    out = np.full(96, 0xAA, dtype=np.uint8)
    lib0 = capi.load_library()
    assert lib0.typlonk_g1_compress(capi._u64p(two), None, 2, capi._u8p(out)) == capi.ERR_INVALID_ARG
    assert (out == 0xAA).all()
    assert capi.g1_compress(np.zeros((0, 12), dtype=np.uint64)) == b""
    xy0, inf0, st0 = capi.g1_decompress(b"")
    assert xy0.shape == (0, 12) and inf0.size == 0 and st0.size == 0
    with pytest.raises(ValueError):
        capi.g1_decompress(bytes(47))
    with pytest.raises(ValueError):
        capi.g1_compress(xy, inf=np.zeros(2, dtype=np.uint8))
    lib = capi.load_library()
    assert lib.typlonk_g1_compress(None, None, 1, None) == capi.ERR_INVALID_ARG
    assert lib.typlonk_g1_decompress(None, None, 1, 0, None, None, None) == capi.ERR_INVALID_ARG
    assert lib.typlonk_proof_compact_to_bytes(None, None) == capi.ERR_INVALID_ARG
    assert lib.typlonk_vk_to_bytes(None, None) == capi.ERR_INVALID_ARG
    assert lib.typlonk_vk_from_bytes(None, 0, None, None) == capi.ERR_INVALID_ARG
    assert lib.typlonk_proof_compact_from_bytes(None, None, 1, 0, None, None) == capi.ERR_INVALID_ARG
    assert lib.typlonk_proof_compact_from_bytes(None, None, 0, 0, None, None) == 0      # count = 0: a no-op
    assert lib.typlonk_verify_compact_bytes(None, None, None, 0, None, None, 0, None) == capi.ERR_INVALID_ARG


def _p_limbs():
    return [(P >> (64 * i)) & (2 ** 64 - 1) for i in range(6)]


# ---- proofs and keys ----
@functools.lru_cache(maxsize=None)
def _circuit_and_proofs():
    from test_compact_ref import circuit, honest

    return circuit(), [(honest(), []), (honest((5,)), [5])]


def _proof_struct(capi, pf):
    pt = lambda p: (g1_pack([p])[0][0], int(g1_pack([p])[1][0]))   # noqa: E731
    return capi.compact_struct({"commit": [pt(p) for p in pf["commit"]], "z_commit": pt(pf["z_commit"]),
                                "t_commit": [pt(p) for p in pf["t_commit"]], "witness": [pt(p) for p in pf["witness"]],
                                "evals": list(fr_pack(pf["evals"]))})


def _vk_struct(capi, vk):
    pt = lambda p: (g1_pack([p])[0][0], int(g1_pack([p])[1][0]))   # noqa: E731
    return capi.vk_from(vk["log_n"], fr_pack(vk["cosets"]), [pt(c) for c in vk["commitments"]], pt(vk["srs0"]),
                        np.array(CR.g2s_limbs(vk["g2s"]), dtype=np.uint64))


def _to_python(d):
    pt = lambda p: g1_unpack_one(p[0], p[1])   # noqa: E731
    return {"commit": [pt(p) for p in d["commit"]], "z_commit": pt(d["z_commit"]), "t_commit": [pt(p) for p in d["t_commit"]],
            "witness": [pt(p) for p in d["witness"]], "evals": fr_unpack(np.array(d["evals"]))}


def _vk_python(vk):
    pt = lambda xy, f: g1_unpack_one(xy, f)   # noqa: E731
    g = [O.fq_from_mont_limbs([int(v) for v in vk.g2s_xy[6 * i:6 * i + 6]]) for i in range(4)]
    return {"log_n": vk.log_n, "cosets": fr_unpack(np.array([list(vk.cosets[i]) for i in range(3)], dtype=np.uint64)),
            "commitments": [pt(vk.commit_xy[i], vk.commit_inf[i]) for i in range(8)], "srs0": pt(vk.srs0_xy, vk.srs0_inf),
            "g2s": ((g[0], g[1]), (g[2], g[3]))}


def test_proof_bytes_are_the_python_layout_and_decode_to_a_proof_the_python_verifier_accepts(capi):
    c, proofs = _circuit_and_proofs()
    blob = b""
    for pf, pi in proofs:
        b = capi.proof_to_bytes(_proof_struct(capi, pf))
        assert len(b) == 656 and b == W.proof_to_bytes(pf)
        blob += b
    back, st = capi.proofs_from_bytes(blob)
    assert st.tolist() == [0, 0]
    for d, (pf, pi) in zip(back, proofs):
        assert _to_python(d) == {k: pf[k] for k in ("commit", "z_commit", "t_commit", "witness", "evals")} == W.proof_from_bytes(
            W.proof_to_bytes(pf))[1]
        assert all(not d["challenges"][k].any() for k in capi.COMPACT_CHALLENGES)   # not sent: the verifier recomputes them
        assert CR.verify_one(c["vk"], _to_python(d), pi)
        assert capi.proof_to_bytes(d) == W.proof_to_bytes(pf)                        # to_bytes(from_bytes(b)) == b


def test_key_bytes_are_the_python_layout_and_round_trip(capi):
    c, _ = _circuit_and_proofs()
    vk = c["vk"]
    s = _vk_struct(capi, vk)
    b = capi.vk_to_bytes(s)
    assert len(b) == 628 and b == W.vk_to_bytes(vk)
    back = capi.vk_from_bytes(b)
    assert _vk_python(back) == vk == W.vk_from_bytes(b)[1]
    assert capi.vk_to_bytes(back) == b
    # log_n outside 1..24
    for log_n in (0, 25, 1 << 31):
        with pytest.raises(capi.TyplonkError) as e:
            capi.vk_from_bytes(log_n.to_bytes(4, "little") + b[4:])
        assert e.value.code == capi.ERR_DOMAIN
    s2 = _vk_struct(capi, dict(vk, log_n=25))
    with pytest.raises(capi.TyplonkError) as e:
        capi.vk_to_bytes(s2)
    assert e.value.code == capi.ERR_DOMAIN
    with pytest.raises(ValueError):
        capi.vk_from_bytes(b[:-1])


def test_native_g2_encoder_gives_the_published_generator_encoding(capi):
    """a key whose [s]G2 is the G2 generator itself (s = 1): the last 96 bytes of typlonk_vk_to_bytes are the published
    compressed generator, and typlonk_vk_from_bytes brings back its coordinates"""
    c, _ = _circuit_and_proofs()
    b = capi.vk_to_bytes(_vk_struct(capi, dict(c["vk"], g2s=PR.G2)))
    g2 = b[532:]
    assert len(g2) == 96 and g2.hex().startswith("93e02b6052719f60")
    assert g2[:48] == (PR.G2[0][1] | 1 << 383).to_bytes(48, "big") and g2[48:] == PR.G2[0][0].to_bytes(48, "big")
    assert _vk_python(capi.vk_from_bytes(b))["g2s"] == PR.G2
    # the other root sets the sign bit
    nb = capi.vk_to_bytes(_vk_struct(capi, dict(c["vk"], g2s=PR.g2_neg(PR.G2))))[532:]
    assert nb[0] == g2[0] | 0x20 and nb[1:] == g2[1:] and nb == W.g2_compress(PR.g2_neg(PR.G2))


def test_bad_fields_of_proofs_and_keys_are_named(capi):
    c, proofs = _circuit_and_proofs()
    good = W.proof_to_bytes(proofs[0][0])
    q = cofactor_points()[1]
    cases = []
    for field in (0, 3, 8):                                                            # a cofactor-order point
        cases.append((good[:48 * field] + W.g1_compress(q) + good[48 * field + 48:], W.NOT_IN_SUBGROUP, field))
    cases.append((good[:48 * 4] + _x_bytes(P) + good[48 * 5:], W.X_RANGE, 4))
    cases.append((good[:48 * 7] + _x_bytes(1) + good[48 * 8:], W.NOT_ON_CURVE, 7))
    cases.append((bytes([good[0] & 0x7F]) + good[1:], W.ENCODING, 0))
    for i in (0, 6):                                                                   # an evaluation equal to r, r + 1, 2^256 - 1
        for v in (R, R + 1, 2 ** 256 - 1):
            cases.append((good[:432 + 32 * i] + v.to_bytes(32, "little") + good[464 + 32 * i:], W.SCALAR_RANGE, 9 + i))
    cases.append((W.g1_compress(q) + good[48:432] + R.to_bytes(32, "little") + good[464:], W.NOT_IN_SUBGROUP, 0))   # the first decides
    blob = b"".join(b for b, _, _ in cases) + good
    back, st = capi.proofs_from_bytes(blob)
    assert [capi.decode_status(int(s)) for s in st] == [(cls, f) for _, cls, f in cases] + [(0, 0)]
    assert [int(s) for s in st[:-1]] == [W.proof_from_bytes(b)[0] for b, _, _ in cases]
    ident = g1_pack([None])
    for d in back[:-1]:                                                                # a refused proof is all identities / zeros
        assert all(p[1] == 1 and p[0].tolist() == ident[0][0].tolist() for p in d["commit"] + d["witness"])
        assert not np.array(d["evals"]).any()
    # with the skip flag the cofactor-order cases decode, the others keep their class
    _, st2 = capi.proofs_from_bytes(blob, skip_subgroup=True)
    assert [int(s) for s in st2] == [W.proof_from_bytes(b, True)[0] for b, _, _ in cases] + [0]
    assert [int(s) for s in st2[:3]] == [0, 0, 0]
    # to_bytes refuses a non-canonical evaluation and a point off the curve
    s = _proof_struct(capi, proofs[0][0])
    s.evals[2][:] = [2 ** 64 - 1] * 4
    with pytest.raises(capi.TyplonkError):
        capi.proof_to_bytes(s)
    s = _proof_struct(capi, proofs[0][0])
    s.w_xy[1][6] ^= 1
    with pytest.raises(capi.TyplonkError):
        capi.proof_to_bytes(s)
    # keys
    vkb = W.vk_to_bytes(c["vk"])
    g2 = PR.G2
    # a point of the twist outside G2: the smallest x = (k, 0) with a root, times nothing
    k = 0
    while True:
        x = (k, 0)
        y = W.f2_sqrt(PR.f2_add(PR.f2_mul(PR.f2_mul(x, x), x), PR.B2))
        if y is not None and W.g2_mul_plain((x, y), R) is not None:
            break
        k += 1
    twist_only = W.g2_compress((x, y))
    kcases = [
        (vkb[:4] + R.to_bytes(32, "little") + vkb[36:], W.SCALAR_RANGE, 0),
        (vkb[:100 + 48 * 8] + W.g1_compress(q) + vkb[100 + 48 * 9:], W.NOT_IN_SUBGROUP, 11),
        (vkb[:100] + _x_bytes(P + 5) + vkb[148:], W.X_RANGE, 3),
        (vkb[:532] + twist_only, W.NOT_IN_SUBGROUP, 12),
        (vkb[:532] + bytes([vkb[532] & 0x7F]) + vkb[533:], W.ENCODING, 12),
        (vkb[:532] + bytes([0xC0]) + bytes(95), W.ENCODING, 12),
        (vkb[:580] + P.to_bytes(48, "big"), W.X_RANGE, 12),
    ]
    for b, cls, field in kcases:
        assert W.vk_from_bytes(b)[0] == cls | field << 8
        with pytest.raises(capi.TyplonkError) as e:
            capi.vk_from_bytes(b)
        assert e.value.code == capi.ERR_INVALID_ARG and capi.decode_status(e.value.status) == (cls, field)
    assert _vk_python(capi.vk_from_bytes(kcases[3][0], skip_subgroup=True))["g2s"] == W.g2_decompress(twist_only, True)[1]
    assert g2 == PR.G2
