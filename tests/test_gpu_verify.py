"""The GPU verifier: typlonk_poly_eval_dev against Horner, typlonk_circuit_commitments against MSMs of the interpolated tables,
and typlonk_verify -- one proof or a batch folded into one pairing product -- against plonk::proof::verify
(plonk/src/proof.rs:195-281): valid proofs are accepted, every tampering rejects exactly the tampered proof."""
import numpy as np
import pytest

from helpers import O, fr_pack, g1_pack, g1_unpack_one
from oracle import coracle as CO

pytestmark = pytest.mark.gpu

R = O.R
SECRET = 0x5EC2E7D00D51


def _limbs(v):
    return np.array(O.fr_to_mont_limbs(v % R), dtype=np.uint64)


def _fr(a):
    return O.fr_from_mont_limbs([int(v) for v in np.asarray(a).reshape(4)])


def _rand_canon(rng, n):
    """n random Montgomery words below 2^252 < r (canonical residues)"""
    a = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64(0x0FFFFFFFFFFFFFFF)
    return a


def _g2s_limbs(secret):
    from oracle import pairing as PR

    (x0, x1), (y0, y1) = PR.srs_g2(secret)[1]
    return np.array([limb for c in (x0, x1, y0, y1) for limb in O.fq_to_mont_limbs(c)], dtype=np.uint64)


G2S = None


def g2s():
    global G2S
    if G2S is None:
        G2S = _g2s_limbs(SECRET)
    return G2S


# ---- typlonk_poly_eval_dev --------------------------------------------------------------------------------------------
def _points(rng, k, log_w=5):
    pts = [_limbs(0), _limbs(1), _limbs(O.domain_root(log_w))] + list(_rand_canon(rng, max(k - 3, 0)))
    return np.array(pts[:k], dtype=np.uint64).reshape(-1, 4)


@pytest.mark.parametrize("m,count,n_points,offset", [
    (1, 1, 1, 0), (2, 3, 5, 1), (1023, 2, 3, 0), (1024, 1, 256, 0), (1025, 16, 4, 7), (1000, 5, 1024, 2),
    (1 << 16, 2, 64, 3), ((1 << 20) + 3, 2, 3, 1)])
def test_poly_eval_equals_horner(ctx, m, count, n_points, offset):
    """every (polynomial, point) value equals the C oracle's Horner; points 0, 1 and a root of unity are among them; the
    first point of every polynomial also equals typlonk_open_dev's y"""
    rng = np.random.default_rng(m * 131 + count)
    polys = [_rand_canon(rng, m + offset + 2) for _ in range(count)]
    bufs = [ctx.alloc(p.shape[0]) for p in polys]
    for b, p in zip(bufs, polys):
        b.upload(p)
    pts = _points(rng, n_points)
    got = ctx.poly_eval_dev(bufs, m, pts, offset=offset)
    assert got.shape == (count, n_points, 4)
    check_pts = range(n_points) if m * n_points * count <= (1 << 22) else [0, 1, 2, n_points - 1]
    for p in range(count):
        for k in check_pts:
            assert (got[p, k] == CO.poly_eval(polys[p][offset:offset + m], pts[k])).all(), (p, k)
        if n_points > 3:
            assert (got[p, 3] == ctx.open_dev(bufs[p], m, pts[3], offset=offset)).all()
    # small cases also against Python big integers
    if m <= 1025:
        for p in range(min(count, 2)):
            coeffs = [_fr(c) for c in polys[p][offset:offset + m]]
            assert [_fr(got[p, k]) for k in range(n_points)] == [O.poly_eval(coeffs, _fr(x)) for x in pts]
    for b in bufs:
        b.free()


@pytest.mark.slow
def test_poly_eval_at_2_25_coefficients(built):
    """the largest length: 2^25 coefficients, three polynomials at 5 points (several point tiles of partials)"""
    from conftest import need_resources

    import typlonk_amd

    need_resources(host_gib=8, hbm_gib=8)
    ctx = typlonk_amd.Context(0)
    try:
        m = 1 << 25
        rng = np.random.default_rng(25)
        polys = [_rand_canon(rng, m) for _ in range(3)]
        bufs = [ctx.alloc(m) for _ in range(3)]
        for b, p in zip(bufs, polys):
            b.upload(p)
        pts = _points(rng, 5)
        got = ctx.poly_eval_dev(bufs, m, pts)
        for p in range(3):
            for k in (0, 2, 4):
                assert (got[p, k] == ctx.open_dev(bufs[p], m, pts[k])).all(), (p, k)
        assert (got[0, 4] == CO.poly_eval(polys[0], pts[4])).all()
        for b in bufs:
            b.free()
    finally:
        ctx.close()


def test_poly_eval_argument_errors(ctx):
    from typlonk_amd.capi import ERR_INVALID_ARG, ERR_LENGTH, ERR_RANGE, TyplonkError

    b = ctx.alloc(16)
    b.upload(np.zeros((16, 4), dtype=np.uint64))
    pts = _points(np.random.default_rng(1), 2)
    for args, kw, code in [(([b], 0, pts), {}, ERR_LENGTH), (([b], 17, pts), {}, ERR_RANGE), (([b], 10, pts), {"offset": 7}, ERR_RANGE),
                           (([b] * 17, 4, pts), {}, ERR_INVALID_ARG),
                           (([b], 4, np.array([[~np.uint64(0)] * 4], dtype=np.uint64)), {}, ERR_INVALID_ARG)]:
        with pytest.raises(TyplonkError) as e:
            ctx.poly_eval_dev(*args, **kw)
        assert e.value.code == code
    b.free()


# ---- proofs -----------------------------------------------------------------------------------------------------------
class Chain:
    """the squaring-chain circuit of typlonk_amd.circuits with many witnesses: other blinding rows, or public inputs"""

    def __init__(self, ctx, log_n, secret=SECRET):
        from typlonk_amd.circuits import SquaringChain

        self.ctx, self.log_n, self.n = ctx, log_n, 1 << log_n
        self.chain = SquaringChain(ctx, log_n, keep_host=True)
        self.cid, self.cosets = self.chain.circuit, self.chain.cosets
        self.host = self.chain.host_inputs()
        self.sid = ctx.srs_generate(_limbs(secret), self.n + 3)

    def prove(self, variant=0, pi=None):
        """variant: other blinding rows (a different valid proof); pi: list of ints, the public-input column (rows < n - 3)"""
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
        bufs = [self.ctx.alloc(n) for _ in range(3)]
        for b, c in zip(bufs, cols):
            b.upload(c)
        pib = None
        if pi is not None:
            pib = self.ctx.alloc(n)
            pib.upload(fr_pack(list(pi) + [0] * (n - len(pi))))
        try:
            return self.ctx.prove_native(self.sid, self.cid, bufs, pib, self.cosets)
        finally:
            for b in bufs + ([pib] if pib else []):
                b.free()

    def verify(self, proofs, **kw):
        return self.ctx.verify(self.sid, self.cid, kw.pop("g2s", g2s()), self.cosets, proofs, **kw)

    def free(self):
        self.chain.free()
        self.ctx.srs_free(self.sid)


@pytest.fixture(scope="module")
def chain5(ctx):
    c = Chain(ctx, 5)
    c.proofs = [c.prove(v) for v in range(16)]
    yield c
    c.free()


def test_circuit_commitments_equal_msms_of_the_tables(ctx, chain5):
    """the eight cached commitments equal ctx.msm of the interpolated selector / sigma columns (what tests/test_gpu_prove.py
    commits as the fixed commitments) and [p(s)]G; a second call returns the cached points"""
    c = chain5
    got = ctx.circuit_commitments(c.sid, c.cid)
    tables = c.host["selectors"] + c.host["sigma"]
    for k, t in enumerate(tables):
        coeffs = ctx.ntt(t, c.log_n, inverse=True)
        exp = ctx.msm(c.sid, coeffs)
        assert (got[k][0] == exp[0]).all() and got[k][1] == exp[1], k
        ps = O.poly_eval([_fr(x) for x in coeffs], SECRET)
        assert g1_unpack_one(*got[k]) == O.g1_mul(O.G1, ps), k
    again = ctx.circuit_commitments(c.sid, c.cid)
    assert all((a[0] == b[0]).all() and a[1] == b[1] for a, b in zip(got, again))


def _oracle_verify(c, d):
    """oracle/pairing.plonk_verify of a prove_native proof (challenges recomputed by the native transcript)"""
    from oracle import pairing as PR
    from oracle import plonk_oracle as PO

    pt = lambda t: g1_unpack_one(t[0], t[1])   # noqa: E731
    ev = [_fr(e) for e in d["evals"]]
    wit = [pt(w) for w in d["witness"]]
    proof = {"commit": [pt(x) for x in d["commit"]], "open": [(wit[i], ev[i]) for i in range(3)], "z_commit": pt(d["z_commit"]),
             "z_open": (wit[3], ev[3]), "zw_open": (wit[4], ev[4]), "t_commit": [pt(x) for x in d["t_commit"]],
             "r_open": (wit[5], ev[5])}
    ch = {k: _fr(v) for k, v in d["challenges"].items()}
    cm = [pt(x) for x in c.ctx.circuit_commitments(c.sid, c.cid)]
    sigma_polys = [[_fr(x) for x in c.ctx.ntt(s, c.log_n, inverse=True)] for s in c.host["sigma"]]
    g2, g2s_pt = PR.srs_g2(SECRET)
    return PR.plonk_verify(c.log_n, proof, cm[:5], sigma_polys, cm[5:], PO.COSETS, [0] * c.n, (ch["alpha"], ch["beta"], ch["gamma"]),
                           ch["zeta"], g2, g2s_pt)


def test_verdicts_equal_the_pairing_oracle_at_2_5(chain5):
    c = chain5
    good = c.proofs[0]
    bad = dict(good, evals=[good["evals"][0]] + [_limbs(_fr(good["evals"][1]) + 1)] + good["evals"][2:])
    got = c.verify([good, bad])
    assert list(got) == [_oracle_verify(c, good), _oracle_verify(c, bad)] == [True, False]


@pytest.mark.parametrize("log_n", [3, 5, 8, 12])
def test_valid_proofs_are_accepted_alone_and_in_batches(ctx, log_n):
    c = Chain(ctx, log_n)
    proofs = [c.prove(v) for v in range(64)]
    assert c.verify(proofs[:1]).tolist() == [True]
    for k in (2, 7, 64):
        assert c.verify(proofs[:k]).all(), k
    assert c.verify([]).shape == (0,)
    c.free()


def _tamper_point(d, key, i=None):
    """replace a point by itself + G (still on the curve)"""
    d = dict(d)
    if i is None:
        xy, f = d[key]
        d[key] = g1_pack([O.g1_add(g1_unpack_one(xy, f), O.G1)])
        d[key] = (d[key][0][0], int(d[key][1][0]))
    else:
        lst = list(d[key])
        xy, f = lst[i]
        p = g1_pack([O.g1_add(g1_unpack_one(xy, f), O.G1)])
        lst[i] = (p[0][0], int(p[1][0]))
        d[key] = lst
    return d


def _tampered(d):
    out = []
    for i in range(3):
        out.append((f"commit{i}", _tamper_point(d, "commit", i)))
        out.append((f"t{i}", _tamper_point(d, "t_commit", i)))
    out.append(("z_commit", _tamper_point(d, "z_commit")))
    for i in range(6):
        out.append((f"witness{i}", _tamper_point(d, "witness", i)))
    for i in range(6):                                  # evals[5] != 0 is r(zeta) != 0
        ev = list(d["evals"])
        ev[i] = _limbs(_fr(ev[i]) + 1)
        out.append((f"eval{i}", dict(d, evals=ev)))
    ch = dict(d["challenges"])
    ch["zeta"] = _limbs(_fr(ch["zeta"]) + 1)
    out.append(("zeta", dict(d, challenges=ch)))
    w = list(d["witness"])
    xy = w[2][0].copy()
    xy[6] ^= np.uint64(1)                               # y + 1: off the curve
    w[2] = (xy, 0)
    out.append(("off_curve", dict(d, witness=w)))
    return out


def test_each_tampering_rejects_only_its_proof(chain5):
    c = chain5
    for name, bad in _tampered(c.proofs[5]):
        batch = c.proofs[:5] + [bad] + c.proofs[6:]
        got = c.verify(batch)
        assert got.tolist() == [k != 5 for k in range(16)], name


def test_several_bad_proofs_in_one_batch(chain5):
    c = chain5
    batch = list(c.proofs)
    batch[1] = _tamper_point(c.proofs[1], "witness", 5)
    batch[9] = dict(c.proofs[9], evals=[_limbs(7)] + c.proofs[9]["evals"][1:])
    batch[15] = _tamper_point(c.proofs[15], "t_commit", 2)
    assert c.verify(batch).tolist() == [k not in (1, 9, 15) for k in range(16)]
    assert not c.verify([batch[1], batch[9]]).any()


def test_bisection_schedule_is_the_replayed_one(ctx, chain5):
    """three rejected proofs and one that never enters the fold (off the curve), 16 proofs: the verdicts, and exactly the
    folds of verify_ref.bisection_folds -- four levels of splitting"""
    import verify_ref as V

    c = chain5
    batch = list(c.proofs)
    batch[1] = _tamper_point(c.proofs[1], "witness", 5)
    batch[9] = dict(c.proofs[9], evals=[_limbs(7)] + c.proofs[9]["evals"][1:])
    batch[15] = _tamper_point(c.proofs[15], "t_commit", 2)
    batch[4] = dict(_tampered(c.proofs[4]))["off_curve"]
    ctx.set_profiling(1)
    try:
        got = c.verify(batch)
        prof = dict(ctx.profile())
    finally:
        ctx.set_profiling(0)
    assert got.tolist() == [k not in (1, 4, 9, 15) for k in range(16)]
    want = V.bisection_folds([k != 4 for k in range(16)], [k in (1, 9, 15) for k in range(16)])
    print("verify_folds", prof["verify_folds"], "replayed", want)
    assert prof["verify_folds"] == want


def test_wrong_circuit_or_wrong_g2s_rejects(ctx, chain5):
    c = chain5
    # another circuit of the same size: the identity permutation instead of the chain's copy constraints
    n = c.n
    bufs = []
    for ev in c.host["selectors"]:
        b = ctx.alloc(n)
        b.upload(ev)
        ctx.ntt_dev(b, c.log_n, inverse=True)
        bufs.append(b)
    for k in (2, 3, 4):
        b = ctx.alloc(n)
        col = np.zeros((n, 4), dtype=np.uint64)
        col[1] = _limbs(k)
        b.upload(col)                                   # k * X: the identity sigma k * w^j
        bufs.append(b)
    other = ctx.circuit_load(c.log_n, bufs[:5], bufs[5:])
    for b in bufs:
        b.free()
    assert not ctx.verify(c.sid, other, g2s(), c.cosets, c.proofs[:4]).any()
    ctx.circuit_free(other)
    assert not c.verify(c.proofs[:4], g2s=_g2s_limbs(SECRET + 1)).any()


def _pi_column(n, length, seed):
    rng = np.random.default_rng(seed)
    pi = [int(v) for v in rng.integers(1, 1 << 60, size=min(length, n - 3))]
    return pi + [0] * (length - len(pi))


@pytest.mark.parametrize("length", [8, 2048, 2049, 4096])
def test_public_inputs_sign_and_binding(ctx, length):
    """a proof with a non-zero public-input column (host barycentric sum up to 2048 values, the device's inverse NTT +
    evaluation above, up to l = n) is accepted with TYPLONK_VERIFY_PI_AS_PROVER and rejected with the reference's sign --
    the two outcomes of the mirror's verify (AsProver / AsReference, tests/cpp/test_plonk_host.cpp) --, and it does not
    verify without its column"""
    c = Chain(ctx, 12)
    pi = _pi_column(c.n, length, length)
    col = fr_pack(pi)
    d = c.prove(pi=pi)
    plain = c.prove(3)
    assert c.verify([d, plain], pi=[col, None], pi_as_prover=True).tolist() == [True, True]
    assert c.verify([d, plain], pi=[col, None]).tolist() == [False, True]
    assert c.verify([d], pi_as_prover=True).tolist() == [False]
    # a NULL column is the zero column
    zero = np.zeros((c.n, 4), dtype=np.uint64)
    assert c.verify([plain, plain], pi=[zero, zero[:5]]).tolist() == [True, True]
    assert c.verify([plain], pi=[None]).tolist() == [True]
    c.free()


@pytest.mark.slow
def test_batches_at_2_20_and_a_proof_at_2_22(built):
    from conftest import need_resources

    import typlonk_amd

    need_resources(host_gib=16, hbm_gib=24)
    ctx = typlonk_amd.Context(0)
    try:
        for log_n, k in ((20, 8), (22, 1)):
            c = Chain(ctx, log_n)
            proofs = [c.prove(v) for v in range(k)]
            assert c.verify(proofs).all()
            bad = dict(proofs[-1], evals=proofs[-1]["evals"][:2] + [_limbs(_fr(proofs[-1]["evals"][2]) + 1)] + proofs[-1]["evals"][3:])
            assert c.verify(proofs[:-1] + [bad]).tolist() == [True] * (k - 1) + [False]
            c.free()
    finally:
        ctx.close()


def test_verify_argument_errors(ctx, chain5):
    from typlonk_amd.capi import ERR_INVALID_ARG, ERR_LENGTH, TyplonkError

    c = chain5
    p = c.proofs[:1]

    def code(fn):
        with pytest.raises(TyplonkError) as e:
            fn()
        return e.value.code

    assert code(lambda: c.verify(p, pi=[np.zeros((c.n + 1, 4), dtype=np.uint64)])) == ERR_LENGTH
    assert code(lambda: ctx.verify(c.sid, 99999, g2s(), c.cosets, p)) == ERR_INVALID_ARG
    assert code(lambda: ctx.verify(99999, c.cid, g2s(), c.cosets, p)) == ERR_INVALID_ARG
    short = ctx.srs_generate(_limbs(SECRET), c.n - 1)
    assert code(lambda: ctx.verify(short, c.cid, g2s(), c.cosets, p)) == ERR_LENGTH
    assert code(lambda: ctx.circuit_commitments(short, c.cid)) == ERR_LENGTH
    ctx.srs_free(short)
    shard = ctx.srs_generate(_limbs(SECRET), c.n + 3)
    ctx.srs_set_shard(shard, 0, 2 * c.n)
    assert code(lambda: ctx.verify(shard, c.cid, g2s(), c.cosets, p)) == ERR_INVALID_ARG
    ctx.srs_free(shard)
    bad_g2 = g2s().copy()
    bad_g2[12] ^= np.uint64(1)
    assert code(lambda: ctx.verify(c.sid, c.cid, bad_g2, c.cosets, p)) == ERR_INVALID_ARG
    lib = ctx.lib
    ok = np.zeros(1, dtype=np.uint8)
    from typlonk_amd.capi import _u8p

    assert lib.typlonk_verify(ctx.h, c.sid, c.cid, None, None, None, 1, None, None, 0, _u8p(ok)) == ERR_INVALID_ARG
    assert lib.typlonk_circuit_commitments(ctx.h, c.sid, c.cid, None, None) == ERR_INVALID_ARG
    assert lib.typlonk_poly_eval_dev(ctx.h, None, 1, 0, 1, None, 1, None) == ERR_INVALID_ARG


def test_mirror_verify_batch_agrees_with_verify(built):
    """tests/cpp/test_verify_host: plonk::CompiledCircuit::verify_batch (typlonk_verify) gives the verdicts of the mirror's
    own verify -- valid proofs, a tampered one, public inputs under both signs"""
    import os
    import subprocess

    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "test_verify_host")
    r = subprocess.run([exe, "6"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "verify_batch agrees with verify ok" in r.stdout
