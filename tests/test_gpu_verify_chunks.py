"""typlonk_verify_chunks on the GPU: the multi-proofs of typlonk_open_chunks_*, a batch of cells per call, for a known full-width s
at (log_n, log_l) in {(4,2), (6,3), (5,0), (7,6), (11,10)} with [s^l]G2 from the oracle.  Honest cells in a shuffled order, a
subset with a repeated cell and proofs the big-integer reference made are accepted in one fold; each of four tamperings -- one
evaluation, the proof, a neighbour's coset index, the wrong commitment index --, alone and three at once, is located exactly, within
2 b ceil(log2 N) + 1 folds, under two seeds and word for word the same in two calls; points that are no group elements and
evaluations that are no residues get their own statuses and leave the other cells accepted; the degenerate polynomials and
secrets; every refusal, with the outputs untouched; and the C++ mirror.  No verdict is retried or tolerated: a fold accepts a bad
batch with probability at most N l / r, r about 2^255."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import open_chunks_ref as FK
import verify_chunks_ref as VR
from helpers import O, fr_pack, g1_pack, g1_unpack_one

pytestmark = pytest.mark.gpu

R = O.R
ORDER3 = (0, 2)                                  # on y^2 = x^3 + 4, of order 3: not a multiple of G
OFF_CURVE = (O.GX, (O.GY + 1) % O.P)
SHAPES = [(4, 2), (6, 3), (5, 0), (7, 6), (11, 10)]
SEED_A, SEED_B = bytes(range(32)), bytes(range(100, 132))
OK, BAD_EVAL, BAD_POINT, BAD_COMMITMENT, BAD_PROOF = VR.OK, VR.BAD_EVAL, VR.BAD_POINT, VR.BAD_COMMITMENT, VR.BAD_PROOF


def _limbs(v):
    return np.array(O.fr_to_mont_limbs(v % R), dtype=np.uint64)


def _rand(rng, k):
    return [int.from_bytes(rng.bytes(32), "little") % R for _ in range(k)]


class Shape:
    """an SRS for a known s, `polys` polynomials, their commitments and every cell the device's prover makes of them"""

    def __init__(self, ctx, log_n, log_l, polys=None, s=None, seed=0):
        from oracle import pairing as OP

        self.ctx, self.log_n, self.log_l = ctx, log_n, log_l
        self.n, self.l, self.r = FK.shape(log_n, log_l)
        rng = np.random.default_rng(0xCE11 + 64 * log_n + log_l + seed)
        self.s = _rand(rng, 1)[0] if s is None else s
        self.fs = polys if polys is not None else [_rand(rng, self.n) for _ in range(2 if log_n > 10 else 3)]
        self.M = len(self.fs)
        self.sid = ctx.srs_generate(_limbs(self.s), self.n + 3)
        tab = ctx.srs_open_chunks_table(self.sid, log_n, log_l)
        try:
            self.pxy, self.pinf, self.ev = ctx.open_chunks(tab, [fr_pack(f) for f in self.fs])
        finally:
            ctx.srs_free(tab)
        cm = [ctx.msm(self.sid, fr_pack(f)) for f in self.fs]
        self.cxy = np.array([c[0] for c in cm], dtype=np.uint64).reshape(self.M, 12)
        self.cinf = np.array([c[1] for c in cm], dtype=np.uint8).reshape(self.M)
        self.g2sl = np.array(VR.g2_limbs(OP.srs_g2(pow(self.s, self.l, R))[1]), dtype=np.uint64)
        self.g2s = np.array(VR.g2_limbs(OP.srs_g2(self.s)[1]), dtype=np.uint64)
        self.all_cells = [(p, k) for p in range(self.M) for k in range(self.r)]

    def free(self):
        self.ctx.srs_free(self.sid)

    def batch(self, cells):
        """the arrays of a call over the cells (p, k), in that order: a dict the tamperings edit in place"""
        ps, ks = [c[0] for c in cells], [c[1] for c in cells]
        return {"cc": np.array(ps, dtype=np.uint32), "ck": np.array(ks, dtype=np.uint32), "ev": self.ev[ps, ks].copy(),
                "pxy": self.pxy[ps, ks].copy(), "pinf": self.pinf[ps, ks].copy(), "cxy": self.cxy.copy(), "cinf": self.cinf.copy()}

    def verify(self, b, seed=SEED_A, g2=None):
        return self.ctx.verify_chunks(self.sid, self.log_n, self.log_l, self.g2sl if g2 is None else g2, seed, (b["cxy"], b["cinf"]),
                                      b["cc"], b["ck"], b["ev"], (b["pxy"], b["pinf"]))


_shapes = {}


@pytest.fixture(scope="module")
def shape(ctx):
    def get(log_n, log_l):
        if (log_n, log_l) not in _shapes:
            _shapes[(log_n, log_l)] = Shape(ctx, log_n, log_l)
        return _shapes[(log_n, log_l)]

    yield get
    for sh in _shapes.values():
        sh.free()
    _shapes.clear()


def _set_point(xy, inf, i, pt):
    one_xy, one_inf = g1_pack([pt])
    xy[i], inf[i] = one_xy[0], one_inf[0]


def tamper(sh, b, i, how):
    """the four tamperings of tests/test_verify_chunks_ref.py, on the arrays of a call"""
    if how == "eval":
        b["ev"][i, sh.l - 1] = _limbs(O.fr_from_mont_limbs([int(x) for x in b["ev"][i, sh.l - 1]]) + 1)
    elif how == "proof":
        _set_point(b["pxy"], b["pinf"], i, O.g1_add(g1_unpack_one(b["pxy"][i], b["pinf"][i]), O.G1))
    elif how == "coset":
        b["ck"][i] = (int(b["ck"][i]) + 1) % sh.r
    else:
        assert how == "commitment"
        b["cc"][i] = (int(b["cc"][i]) + 1) % sh.M


def _bound(b, N):
    return 2 * b * max((N - 1).bit_length(), 1) + 1


def _shuffled(sh, seed):
    cells = list(sh.all_cells)
    np.random.default_rng(seed).shuffle(cells)
    return [tuple(c) for c in cells]


# ---- 1. accept ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_every_cell_is_accepted_in_one_fold(shape, log_n, log_l):
    sh = shape(log_n, log_l)
    cells = _shuffled(sh, 0x5F1)
    N = len(cells)
    out = sh.verify(sh.batch(cells))
    assert (out["status"] == OK).all() and out["folds"] == 1 and out["live"] == N and out["count"] == [N, 0, 0, 0, 0]
    # a strict subset, one cell twice
    sub = cells[1:max(N // 2, 2)] + [cells[1]]
    out = sh.verify(sh.batch(sub), SEED_B)
    assert (out["status"] == OK).all() and out["folds"] == 1 and out["count"][0] == len(sub)


def test_proofs_of_the_reference_are_accepted(shape):
    """the verifier is not judged only by the prover it ships with: the proofs are [q_k(s)] G from the big-integer division"""
    sh = shape(4, 2)
    b = sh.batch(sh.all_cells)
    for p, f in enumerate(sh.fs):
        xy, inf = g1_pack(FK.points(FK.openings_known_secret(f, sh.s, sh.log_n, sh.log_l)))
        b["pxy"][p * sh.r:(p + 1) * sh.r], b["pinf"][p * sh.r:(p + 1) * sh.r] = xy, inf
    out = sh.verify(b)
    assert (out["status"] == OK).all() and out["folds"] == 1
    tamper(sh, b, 5, "proof")
    assert sh.verify(b)["status"].tolist() == [BAD_PROOF if i == 5 else OK for i in range(len(sh.all_cells))]


# ---- 2. reject and locate -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_tamperings_are_located(shape, log_n, log_l):
    sh = shape(log_n, log_l)
    cells = _shuffled(sh, 0x7A3)
    N = len(cells)
    for plan in [{N // 2: how} for how in ("eval", "proof", "coset", "commitment")] + [_three(N)]:
        _located(sh, cells, plan, SEED_A)


def _three(N):
    """three tamperings at scattered positions"""
    return {0: "coset", N // 3 + 1: "eval", N - 1: "proof"} if N >= 6 else {0: "coset", 1: "eval", N - 1: "proof"}


def _located(sh, cells, plan, seed):
    """exactly the tampered cells are BAD_PROOF, every other cell is OK, within the bound on the folds"""
    N = len(cells)
    b = sh.batch(cells)
    for i, how in plan.items():
        tamper(sh, b, i, how)
    out = sh.verify(b, seed)
    assert out["status"].tolist() == [BAD_PROOF if i in plan else OK for i in range(N)], plan
    assert 1 < out["folds"] <= _bound(len(plan), N), (plan, out["folds"])
    assert out["live"] == N and out["count"] == [N - len(plan), 0, 0, 0, len(plan)]
    return out


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_verdicts_under_another_seed_and_twice(shape, log_n, log_l):
    """the three tamperings are located under a second seed as under the first (test_tamperings_are_located), and two identical
    calls give the same words"""
    sh = shape(log_n, log_l)
    cells = _shuffled(sh, 0x7A3)
    N = len(cells)
    _located(sh, cells, _three(N), SEED_B)
    one, two = (_located(sh, cells, {N // 2: "eval"}, SEED_B) for _ in range(2))
    assert (one["status"] == two["status"]).all() and one["folds"] == two["folds"] and one["count"] == two["count"]


def test_folds_are_the_reference_bisection(shape):
    """the folds of a call are those of the reference's bisection over the same verdicts"""
    sh = shape(6, 3)
    cells = _shuffled(sh, 0xF01D)
    b = sh.batch(cells)
    bad = {2: "proof", 11: "eval", 12: "commitment"}
    for i, how in bad.items():
        tamper(sh, b, i, how)
    out = sh.verify(b)
    # the reference on scalars: honest cells with a proof scalar moved at the bad positions fail the same folds
    ref_cells = []
    for i, (p, k) in enumerate(cells):
        ys = [O.fr_from_mont_limbs([int(x) for x in row]) for row in sh.ev[p, k]]
        pi = FK.openings_known_secret(sh.fs[p], sh.s, sh.log_n, sh.log_l)[k]
        ref_cells.append((p, k, ys, (pi + 1) % R if i in bad else pi))
    status, folds = VR.check(ref_cells, [O.poly_eval(f, sh.s) for f in sh.fs], sh.s, 12345, sh.log_n, sh.log_l)
    assert out["status"].tolist() == status and out["folds"] == folds


def test_a_bisection_whose_halves_would_plan_more_workgroups_than_the_call(ctx):
    """N = 4097 cells of l = 128: the call's own plan has 1366 workgroups (strips of 3), a plan of its 2048-cell half alone would
    have 2048.  Every fold of the bisection is planned with the call's strip and stays inside the partial vectors allocated once;
    the one bad cell is located within the bound.  (The four distinct cells of this domain, repeated.)"""
    sh = Shape(ctx, 8, 7, seed=5)
    try:
        N = 4097
        cells = [sh.all_cells[i % len(sh.all_cells)] for i in range(N)]
        b = sh.batch(cells)
        out = sh.verify(b)
        assert (out["status"] == OK).all() and out["folds"] == 1
        tamper(sh, b, 3000, "eval")
        out = sh.verify(b)
        assert out["status"].tolist() == [BAD_PROOF if i == 3000 else OK for i in range(N)]
        assert 1 < out["folds"] <= _bound(1, N) and out["count"] == [N - 1, 0, 0, 0, 1]
    finally:
        sh.free()


# ---- 3. the other statuses ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,log_l", [(4, 2), (7, 6)])
def test_points_that_are_no_group_elements(shape, log_n, log_l):
    sh = shape(log_n, log_l)
    cells = list(sh.all_cells)
    N = len(cells)
    b = sh.batch(cells)
    _set_point(b["pxy"], b["pinf"], 1, ORDER3)
    _set_point(b["pxy"], b["pinf"], N - 2, OFF_CURVE)
    out = sh.verify(b)
    assert out["status"].tolist() == [BAD_POINT if i in (1, N - 2) else OK for i in range(N)]
    assert out["folds"] == 1 and out["live"] == N - 2 and out["count"] == [N - 2, 0, 2, 0, 0]
    # the same as a commitment: its cells only
    for pt in (ORDER3, OFF_CURVE):
        b = sh.batch(cells)
        _set_point(b["cxy"], b["cinf"], 1, pt)
        out = sh.verify(b)
        assert out["status"].tolist() == [BAD_COMMITMENT if p == 1 else OK for p, _ in cells]
        assert out["folds"] == 1 and out["count"] == [N - sh.r, 0, 0, sh.r, 0]
    # with a bad proof among the live cells, and the first class winning
    b = sh.batch(cells)
    _set_point(b["cxy"], b["cinf"], 1, ORDER3)
    _set_point(b["pxy"], b["pinf"], sh.r, OFF_CURVE)                     # a cell of commitment 1: BAD_POINT comes first
    tamper(sh, b, 0, "proof")
    out = sh.verify(b)
    assert out["status"].tolist() == [BAD_PROOF if i == 0 else BAD_POINT if i == sh.r else BAD_COMMITMENT if p == 1 else OK
                                      for i, (p, _) in enumerate(cells)]


@pytest.mark.parametrize("log_n,log_l", [(4, 2), (5, 0)])
def test_evaluations_that_are_no_residues(shape, log_n, log_l):
    sh = shape(log_n, log_l)
    cells = list(sh.all_cells)
    N = len(cells)
    b = sh.batch(cells)
    b["ev"][3, sh.l - 1] = np.array([0xFFFFFFFF00000001, 0x53BDA402FFFE5BFE, 0x3339D80809A1D805, 0x73EDA753299D7D48], dtype=np.uint64)   # r itself
    b["ev"][N - 1, 0] = np.full(4, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    _set_point(b["pxy"], b["pinf"], N - 1, ORDER3)                       # BAD_EVAL comes first
    out = sh.verify(b)
    assert out["status"].tolist() == [BAD_EVAL if i in (3, N - 1) else OK for i in range(N)]
    assert out["folds"] == 1 and out["live"] == N - 2 and out["count"] == [N - 2, 2, 0, 0, 0]
    b["ev"][3, sh.l - 1] -= np.array([1, 0, 0, 0], dtype=np.uint64)        # r - 1 is a residue: now the equation decides
    assert sh.verify(b)["status"].tolist() == [BAD_PROOF if i == 3 else BAD_EVAL if i == N - 1 else OK for i in range(N)]


def test_no_live_cell_runs_no_fold(shape):
    sh = shape(4, 2)
    b = sh.batch(sh.all_cells[:2])
    b["ev"][:, 0] = np.full(4, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    out = sh.verify(b)
    assert out["status"].tolist() == [BAD_EVAL] * 2 and out["folds"] == 0 and out["live"] == 0


# ---- 4. degenerate inputs -----------------------------------------------------------------------------------------------------
def test_identity_proofs_and_identity_commitment(ctx):
    """a polynomial of degree < l opens to identity proofs, f = 0 has the identity as its commitment: both are group elements"""
    log_n, log_l = 6, 3
    rng = np.random.default_rng(0x1DE)
    n, l, r = FK.shape(log_n, log_l)
    sh = Shape(ctx, log_n, log_l, polys=[_rand(rng, l) + [0] * (n - l), [0] * n, _rand(rng, n)])
    try:
        assert sh.pinf[0].all() and sh.pinf[1].all() and sh.cinf[1] == 1 and not sh.pinf[2].any()
        out = sh.verify(sh.batch(_shuffled(sh, 3)))
        assert (out["status"] == OK).all() and out["folds"] == 1
        b = sh.batch(sh.all_cells)
        tamper(sh, b, 1, "eval")                                          # a cell of the low polynomial
        tamper(sh, b, r + 2, "commitment")                                # a cell of f = 0 claimed against the random one
        out = sh.verify(b)
        assert out["status"].tolist() == [BAD_PROOF if i in (1, r + 2) else OK for i in range(3 * r)]
    finally:
        sh.free()


def test_the_wrong_g2_element_rejects_every_cell(shape):
    """[s]G2 where [s^l]G2 belongs, l > 1"""
    sh = shape(4, 2)
    cells = sh.all_cells
    out = sh.verify(sh.batch(cells), g2=sh.g2s)
    assert (out["status"] == BAD_PROOF).all() and out["folds"] <= 2 * len(cells) - 1


def test_secret_one(ctx):
    """s = 1: every SRS point is G and [s^l]G2 = G2"""
    sh = Shape(ctx, 4, 2, s=1)
    try:
        out = sh.verify(sh.batch(_shuffled(sh, 9)))
        assert (out["status"] == OK).all() and out["folds"] == 1
        b = sh.batch(sh.all_cells)
        tamper(sh, b, 7, "coset")
        assert sh.verify(b)["status"].tolist() == [BAD_PROOF if i == 7 else OK for i in range(len(sh.all_cells))]
    finally:
        sh.free()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(shape, ctx):
    """every refusal the header lists but TYPLONK_ERR_OOM (no allocation a test can afford is refused), status and report filled
    with a marker beforehand and found unchanged"""
    from typlonk_amd.capi import ERR_DOMAIN, ERR_INVALID_ARG, ERR_LENGTH, ERR_RANGE, ChunksReport, _u8p, _u64p

    sh = shape(4, 2)
    lib = ctx.lib
    cells = sh.all_cells
    N, M = len(cells), sh.M
    u32 = C.POINTER(C.c_uint32)

    def refused(handle=None, sid=None, log_n=sh.log_n, log_l=sh.log_l, g2=sh.g2sl, n=N, m=M, null=None, edit=None):
        b = sh.batch(cells)
        if edit:
            edit(b)
        seed = np.frombuffer(SEED_A, dtype=np.uint8).copy()
        status = np.full(N, 0x5A, dtype=np.uint8)
        rep = ChunksReport()
        C.memset(C.byref(rep), 0xC3, C.sizeof(rep))
        args = {"g2": _u64p(np.ascontiguousarray(g2)), "seed": _u8p(seed), "cxy": _u64p(b["cxy"]), "cinf": _u8p(b["cinf"]),
                "cc": b["cc"].ctypes.data_as(u32), "ck": b["ck"].ctypes.data_as(u32), "ev": _u64p(b["ev"]), "pxy": _u64p(b["pxy"]),
                "pinf": _u8p(b["pinf"]), "status": _u8p(status), "report": C.byref(rep)}
        if null:
            args[null] = None
        rc = lib.typlonk_verify_chunks(ctx.h if handle is None else handle[0], sh.sid if sid is None else sid, log_n, log_l, args["g2"],
                                       args["seed"], args["cxy"], args["cinf"], m, args["cc"], args["ck"], args["ev"], args["pxy"],
                                       args["pinf"], n, args["status"], args["report"])
        assert (status == 0x5A).all() and bytes(rep) == b"\xC3" * C.sizeof(rep), "a refused call wrote to its outputs"
        return rc

    # INVALID_ARG: a null pointer
    assert refused(handle=(None,)) == ERR_INVALID_ARG
    for name in ("g2", "seed", "cxy", "cinf", "cc", "ck", "ev", "pxy", "pinf", "status", "report"):
        assert refused(null=name) == ERR_INVALID_ARG, name
    # DOMAIN
    for lg in (0, 25, 64, 0xFFFFFFFF):
        assert refused(log_n=lg, log_l=0) == ERR_DOMAIN
    for lg_l in (sh.log_n, sh.log_n + 1, 0xFFFFFFFF):
        assert refused(log_l=lg_l) == ERR_DOMAIN
    assert refused(log_n=12, log_l=11) == ERR_DOMAIN                               # log_l > 10
    assert b"log_l" in lib.typlonk_last_error(ctx.h)
    # LENGTH
    assert refused(n=0) == ERR_LENGTH and refused(m=0) == ERR_LENGTH
    assert refused(n=(1 << 25 >> sh.log_l) + 1) == ERR_LENGTH                      # N l > 2^25
    assert refused(log_n=5, log_l=0, n=1 << 25) == ERR_LENGTH                      # N + M > 2^25
    assert refused(m=(1 << 25) - N + 1) == ERR_LENGTH
    # INVALID_ARG: the entry and g2sl
    assert refused(sid=999999) == ERR_INVALID_ARG
    shard = ctx.srs_generate(_limbs(sh.s), sh.n + 3)
    ctx.srs_set_shard(shard, 0, 2 * sh.n + 6)
    assert refused(sid=shard) == ERR_INVALID_ARG
    ctx.srs_free(shard)
    tab = ctx.srs_open_chunks_table(sh.sid, sh.log_n, sh.log_l)
    assert refused(sid=tab) == ERR_INVALID_ARG
    assert b"table" in lib.typlonk_last_error(ctx.h)
    ctx.srs_free(tab)
    short = ctx.srs_generate(_limbs(sh.s), sh.l - 1)
    assert refused(sid=short) == ERR_INVALID_ARG                                    # fewer than l points
    ctx.srs_free(short)
    off = sh.g2sl.copy()
    off[0] ^= 1
    assert refused(g2=off) == ERR_INVALID_ARG                                       # off the twist
    # RANGE
    def commit_out(b):
        b["cc"][N - 1] = M

    def coset_out(b):
        b["ck"][0] = sh.r

    assert refused(edit=commit_out) == ERR_RANGE and refused(edit=coset_out) == ERR_RANGE
    # the challenge
    from typlonk_amd.capi import verify_chunks_challenge
    rho = np.zeros(4, dtype=np.uint64)
    assert lib.typlonk_verify_chunks_challenge(None, 4, 2, N, M, _u64p(sh.g2sl), _u64p(rho)) == ERR_INVALID_ARG
    got = verify_chunks_challenge(SEED_A, sh.log_n, sh.log_l, N, M, sh.g2sl)
    from oracle import pairing as OP
    assert O.fr_from_mont_limbs([int(x) for x in got]) == VR.rho(SEED_A, sh.log_n, sh.log_l, N, M, OP.srs_g2(pow(sh.s, sh.l, R))[1])
    # nothing was created or changed, and a good call still succeeds
    assert ctx.srs_len(sh.sid) == sh.n + 3
    out = sh.verify(sh.batch(cells))
    assert (out["status"] == OK).all() and out["folds"] == 1


# ---- 6. the C++ mirror --------------------------------------------------------------------------------------------------------
def test_mirror_verify_chunks(built):
    """tests/cpp/test_verify_chunks_host: kzg::KzgScheme::verify_chunks of the C++ mirror"""
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "test_verify_chunks_host")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for t in ("accept ok", "reject ok", "refusals ok"):
        assert t in r.stdout
