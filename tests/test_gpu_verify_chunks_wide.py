"""typlonk_verify_chunks on wide domains, judged by the big-integer reference: (log_n, log_l) = (12, 3), (10, 0) and (14, 6), two
polynomials each -- r = 512, 1024 and 256 cosets, where tests/test_gpu_verify_chunks.py stops at 32 --, N = 2 r cells a call.

The cells come from the device's own open_chunks (pinned to the reference at these sizes by tests/test_gpu_g1_wide.py), but what
the verifier is judged against does not: the evaluations must equal the C oracle's transform word for word, the commitments are
[f(s)] G from the oracle, sixteen proofs of every shape -- cosets 0, 31, 32, r/2 and r - 1 among them -- are replaced by
[q_k(s)] G from the closed forms of tests/g1_wide_ref.py, and every verdict AND the number of folds must equal
verify_chunks_ref.check over the same cells on scalars (a proof moved by G is a scalar moved by 1).  Tamperings: a coset moved
by XOR 32, by XOR r/2 and by + 32 past r; an evaluation at t = 0 and at t = l/2; the proof; three at once; a commitment
replaced by another group element; a point that is no group element as a commitment no cell names; one copy of a repeated
cell; batches whose proofs are all the identity; and the profiled path of the call, which must answer as the unprofiled one.
No verdict is retried or tolerated: a fold accepts a bad batch with probability at most N l / r, r about 2^255.  A fold costs
one pairing product on the host, so the batches are sized by their folds."""
import numpy as np
import pytest

import g1_wide_ref as W
import verify_chunks_ref as VR
from helpers import O, g1_pack, g1_unpack_one
from oracle import coracle as CO

pytestmark = pytest.mark.gpu

R = O.R
ORDER3 = (0, 2)                                  # on y^2 = x^3 + 4, of order 3: not a multiple of G
SHAPES = [(12, 3), (10, 0), (14, 6)]
SEED = bytes(range(7, 39))
RHO = 0x9E3779B97F4A7C15F39CC0605CEDC834 % R    # the reference's weight: its verdicts and folds do not depend on it
OK, BAD_PROOF = VR.OK, VR.BAD_PROOF
PROFILE_NAMES = ["chunks_upload", "chunks_membership", "chunks_kernels", "chunks_msm", "chunks_pairing", "chunks_folds"]


def _rand(rng, k):
    return [int.from_bytes(rng.bytes(32), "little") % R for _ in range(k)]


def _bound(b, N):
    return 2 * b * max((N - 1).bit_length(), 1) + 1


def _generator_times(e):
    """[e] G as (xy, inf), by the C oracle"""
    return CO.g1_mul_generator(W.pack([e])[0])


class Wide:
    """an SRS for a known full-width s, `polys` polynomials, every cell the device's prover makes of them, and the same cells on
    scalars from g1_wide_ref"""

    def __init__(self, ctx, log_n, log_l, polys):
        from oracle import pairing as OP

        self.ctx, self.log_n, self.log_l = ctx, log_n, log_l
        self.n, self.l, self.r = 1 << log_n, 1 << log_l, 1 << (log_n - log_l)
        n, l, r = self.n, self.l, self.r
        rng = np.random.default_rng(0x1DE0 + 64 * log_n + log_l)
        self.s = _rand(rng, 1)[0]
        self.fs = polys(rng, n, l)
        self.M = M = len(self.fs)
        self.sid = ctx.srs_generate(W.pack([self.s])[0], n + 3)
        tab = ctx.srs_open_chunks_table(self.sid, log_n, log_l)
        try:
            self.pxy, self.pinf, self.ev = ctx.open_chunks(tab, [W.pack(f) for f in self.fs])
        finally:
            ctx.srs_free(tab)
        self.pxy, self.pinf = self.pxy.copy(), self.pinf.copy()
        # the reference's side: evaluations (which the device's must equal), proof scalars, commitments
        self.ys, self.pis, self.cs = [], [], []
        for p, f in enumerate(self.fs):
            ev = W.chunk_major(W.domain_evaluations(f, log_n), log_n, log_l)
            assert (self.ev[p].reshape(n, 4) == ev).all(), p
            self.ys.append(W.unpack(ev))
            self.pis.append(W.open_chunks_scalars(f, self.s, log_n, log_l))
            self.cs.append(W.horner(f, self.s))
        cm = [_generator_times(c) for c in self.cs]
        self.cxy = np.array([c[0] for c in cm], dtype=np.uint64).reshape(M, 12)
        self.cinf = np.array([c[1] for c in cm], dtype=np.uint8).reshape(M)
        # sixteen proofs the prover under test did not make
        ks = [0, 31, 32, r // 2, r - 1]
        self.sample = {(i % M, k) for i, k in enumerate(ks) if k < r}
        while len(self.sample) < min(16, M * r):
            self.sample.add((int(rng.integers(M)), int(rng.integers(r))))
        self.sample = sorted(self.sample)
        for p, k in self.sample:
            self.pxy[p, k], self.pinf[p, k] = _generator_times(self.pis[p][k])
        self.g2sl = np.array(VR.g2_limbs(OP.srs_g2(pow(self.s, l, R))[1]), dtype=np.uint64)
        self.all_cells = [(p, k) for p in range(M) for k in range(r)]

    def free(self):
        self.ctx.srs_free(self.sid)

    def shuffled(self, seed):
        cells = list(self.all_cells)
        np.random.default_rng(seed).shuffle(cells)
        return [tuple(int(x) for x in c) for c in cells]

    def batch(self, cells):
        """(the arrays of a call over the cells (p, k), the same cells on scalars): `tamper` edits both"""
        ps, ks, l = [c[0] for c in cells], [c[1] for c in cells], self.l
        b = {"cc": np.array(ps, dtype=np.uint32), "ck": np.array(ks, dtype=np.uint32), "ev": self.ev[ps, ks].copy(),
             "pxy": self.pxy[ps, ks].copy(), "pinf": self.pinf[ps, ks].copy(), "cxy": self.cxy.copy(), "cinf": self.cinf.copy()}
        return b, [(p, k, self.ys[p][k * l:(k + 1) * l], self.pis[p][k]) for p, k in cells]

    def verify(self, b):
        return self.ctx.verify_chunks(self.sid, self.log_n, self.log_l, self.g2sl, SEED, (b["cxy"], b["cinf"]), b["cc"], b["ck"], b["ev"],
                                      (b["pxy"], b["pinf"]))

    def check(self, ref, commitments=None):
        return VR.check(ref, self.cs if commitments is None else commitments, self.s, RHO, self.log_n, self.log_l)

    def tamper(self, b, ref, i, how):
        """one tampering of cell i, on the arrays of the call and on the reference's cell alike"""
        c, k, ys, pi = ref[i]
        r, l = self.r, self.l
        if how in ("coset^32", "coset^half", "coset+32"):
            k2 = k ^ 32 if how == "coset^32" else k ^ (r // 2) if how == "coset^half" else (k + 32) % r
            assert how != "coset+32" or k >= r - 32            # k + 32 is no coset: the claim wraps to a low one
            assert k2 != k and 0 <= k2 < r
            b["ck"][i] = k2
            ref[i] = (c, k2, ys, pi)
        elif how in ("eval@0", "eval@half"):
            t = 0 if how == "eval@0" else l // 2
            assert how == "eval@0" or t > 0
            y = (ys[t] + 1) % R
            b["ev"][i, t] = W.pack([y])[0]
            ref[i] = (c, k, ys[:t] + [y] + ys[t + 1:], pi)
        else:
            assert how == "proof"
            xy, inf = g1_pack([O.g1_add(g1_unpack_one(b["pxy"][i], b["pinf"][i]), O.G1)])
            b["pxy"][i], b["pinf"][i] = xy[0], inf[0]
            ref[i] = (c, k, ys, (pi + 1) % R)


def _random_polys(count):
    return lambda rng, n, l: [_rand(rng, n) for _ in range(count)]


def _low_poly(rng, n, l):
    """one polynomial of degree < l: its own interpolant on every coset, so every proof is the identity"""
    return [_rand(rng, l) + [0] * (n - l)]


_wides = {}


@pytest.fixture(scope="module")
def wide(ctx):
    def get(log_n, log_l, low=False):
        key = (log_n, log_l, low)
        if key not in _wides:
            _wides[key] = Wide(ctx, log_n, log_l, _low_poly if low else _random_polys(2))
        return _wides[key]

    yield get
    for sh in _wides.values():
        sh.free()
    _wides.clear()
    _three.clear()


def _same_as_reference(sh, b, ref, bad, commitments=None):
    """the call's verdicts are BAD_PROOF at exactly `bad`, and they and the folds are the reference's, within the bound"""
    N = len(ref)
    out = sh.verify(b)
    status, folds = sh.check(ref, commitments)
    assert status == [BAD_PROOF if i in bad else OK for i in range(N)]          # the reference blames what was tampered with
    assert out["status"].tolist() == status
    assert out["folds"] == folds and folds <= _bound(max(len(bad), 1), N), (out["folds"], folds)
    assert out["live"] == N and out["count"] == [N - len(bad), 0, 0, 0, len(bad)]
    return out


# ---- 1. accept ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_the_honest_batch_is_accepted_in_one_fold(wide, log_n, log_l):
    sh = wide(log_n, log_l)
    assert len(sh.sample) == 16 and {0, 31, 32, sh.r // 2, sh.r - 1} <= {k for _, k in sh.sample}
    b, ref = sh.batch(sh.shuffled(0x5F1))
    out = _same_as_reference(sh, b, ref, set())
    assert out["folds"] == 1


# ---- 2. reject and locate -----------------------------------------------------------------------------------------------------
HOWS = ["coset^32", "coset^half", "coset+32", "eval@0", "eval@half", "proof"]


@pytest.mark.parametrize("log_n,log_l,how", [(n, l, how) for n, l in SHAPES for how in HOWS if l or how != "eval@half"])
def test_each_tampering_is_located(wide, log_n, log_l, how):
    sh = wide(log_n, log_l)
    cells = sh.shuffled(0x7A3)
    N = len(cells)
    at = next(i for i in range(N // 2, N) if cells[i][1] >= sh.r - 32) if how == "coset+32" else N // 2
    b, ref = sh.batch(cells)
    sh.tamper(b, ref, at, how)
    assert not VR.cell_holds(ref[at], sh.cs, sh.s, log_n, log_l)
    out = _same_as_reference(sh, b, ref, {at})
    assert out["folds"] > 1


_three = {}


def _three_at_once(sh):
    """(batch, the call's unprofiled answer) for the tamperings at 5, N/2 + 37 and N - 1; made once a shape"""
    key = (sh.log_n, sh.log_l)
    if key not in _three:
        cells = sh.shuffled(0xF01D)
        N = len(cells)
        b, ref = sh.batch(cells)
        plan = {5: "coset^32", N // 2 + 37: "eval@half" if sh.l > 1 else "eval@0", N - 1: "proof"}
        for i, how in plan.items():
            sh.tamper(b, ref, i, how)
        _three[key] = (b, _same_as_reference(sh, b, ref, set(plan)))
    return _three[key]


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_three_tamperings_at_once(wide, log_n, log_l):
    _, out = _three_at_once(wide(log_n, log_l))
    assert out["count"][BAD_PROOF] == 3 and out["folds"] > 3


def test_a_wrong_commitment_point(wide):
    """commitment 1 replaced by C + G, a group element that commits to another polynomial: exactly its cells fail.  Every one of
    them costs the bisection its own folds (about two a cell, each a pairing product on the host), so the batch is 64 cells of
    either commitment, in alternating runs of 16, not all 2 r = 1024."""
    sh = wide(12, 3)
    picked = {p: [k for q, k in sh.shuffled(0xC0C0) if q == p][:64] for p in (0, 1)}
    assert all(max(ks) >= 32 for ks in picked.values())
    cells = [(p, k) for run in range(4) for p in (0, 1) for k in picked[p][16 * run:16 * run + 16]]
    b, ref = sh.batch(cells)
    xy, inf = _generator_times((sh.cs[1] + 1) % R)
    b["cxy"][1], b["cinf"][1] = xy, inf
    bad = {i for i, (p, _) in enumerate(cells) if p == 1}
    assert len(bad) == 64
    _same_as_reference(sh, b, ref, bad, commitments=[sh.cs[0], (sh.cs[1] + 1) % R])


def test_a_non_member_commitment_nobody_names(wide):
    """M = 3, the third commitment the order-3 point (0, 2): its membership flag is raised and its record cleared, and no cell is
    blamed for it"""
    sh = wide(12, 3)
    b, ref = sh.batch(sh.shuffled(0x03D3))
    xy, inf = g1_pack([ORDER3])
    b["cxy"], b["cinf"] = np.vstack([b["cxy"], xy]), np.concatenate([b["cinf"], inf])
    N = len(ref)
    out = sh.verify(b)
    assert (out["status"] == OK).all() and out["folds"] == 1 and out["live"] == N and out["count"] == [N, 0, 0, 0, 0]
    assert sh.check(ref, sh.cs + [0]) == ([OK] * N, 1)


def test_one_copy_of_a_repeated_cell(wide):
    sh = wide(12, 3)
    cells = sh.shuffled(0x2C0F)
    N = len(cells) + 1
    at = N // 3
    cells.insert(at, cells[N - 7])                               # the same cell at `at` and, shifted by the insertion, at N - 6
    assert cells[at] == cells[N - 6] and cells.count(cells[at]) == 2
    b, ref = sh.batch(cells)
    sh.tamper(b, ref, at, "eval@0")
    _same_as_reference(sh, b, ref, {at})


@pytest.mark.parametrize("log_n,log_l", [(6, 3), (12, 3)])
def test_batches_of_identity_proofs_only(wide, log_n, log_l):
    """a polynomial of degree < l: every proof is the identity, so both MSMs over the proofs give the identity and the honest
    fold's pairing product is over two identities"""
    sh = wide(log_n, log_l, low=True)
    assert sh.pinf.all() and not any(sh.pis[0])
    cells = sh.shuffled(0x1D)
    N = len(cells)
    b, ref = sh.batch(cells)
    assert _same_as_reference(sh, b, ref, set())["folds"] == 1
    at = N - 3
    sh.tamper(b, ref, at, "eval@half")
    assert b["pinf"].all()
    _same_as_reference(sh, b, ref, {at})


# ---- 3. the profiled path -------------------------------------------------------------------------------------------------------
def test_a_profiled_call_answers_as_an_unprofiled_one(wide, ctx):
    """with profiling on the call drains the stream after the kernels of every fold and reports six entries; the answers are
    those of the unprofiled call, and the MSM after it reports its own stages"""
    sh = wide(12, 3)
    honest, _ = sh.batch(sh.shuffled(0x5F1))
    plain = [(honest, sh.verify(honest)), _three_at_once(sh)]
    assert plain[0][1]["folds"] == 1 and plain[1][1]["folds"] > 3
    ctx.set_profiling(1)
    try:
        for b, want in plain:
            got = sh.verify(b)
            prof = ctx.profile()
            assert (got["status"] == want["status"]).all()
            assert (got["folds"], got["live"], got["count"]) == (want["folds"], want["live"], want["count"])
            assert [name for name, _ in prof] == PROFILE_NAMES
            assert dict(prof)["chunks_folds"] == got["folds"]
            assert all(ms >= 0 for _, ms in prof)
        xy, inf = ctx.msm(sh.sid, W.pack(sh.fs[0]))
        names = [name for name, _ in ctx.profile()]
        assert "msm_accum" in names and not any(name.startswith("chunks_") for name in names), names
        assert (xy == sh.cxy[0]).all() and inf == sh.cinf[0]
    finally:
        ctx.set_profiling(0)
