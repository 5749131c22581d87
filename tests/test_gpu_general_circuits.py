"""Every prover and verifier entry point on circuits with general selectors (tests/general_circuits.py): all five selectors
uniform in [0, r) and non-zero on every row, q_l != q_r, an arbitrary permutation, non-zero public values of full range.  On the
squaring chain and the README circuit three of the five gate terms multiply zeros; here a swap of q_l with q_r, a dropped or
mis-signed q_c, or a selector index off by one changes a value that a test compares.

2^3 .. 2^6 rows: bit for bit against the Python provers (tests/compact_ref.py, oracle/plonk_oracle.py) and verdict for verdict
against the Python verifiers, single proofs and batches of 1, 4 and 5 (two groups of the batched kernels) with public-input
lengths that differ between neighbours, under cosets (2, 3, 4) and (1, k1, k2).  2^12 rows (two workgroups of every
2048-element scan, four chunks of the evaluation kernel): each stage against its own Python statement.  Every comparison is
integer equality or accept / reject."""
import numpy as np
import pytest

import compact_ref as CR
import general_circuits as G
import transcript_ref as T
import witness_check_ref as W
from helpers import O, fr_pack, fr_unpack, g1_unpack_one
from oracle import coracle as CO
from oracle import pairing as PR
from oracle import plonk_oracle as PO
from test_gpu_compact import _g2s, _limbs, _tamper_point, _to_python
from test_gpu_prove_batch import same
from test_gpu_prove_batch import single as single_reference
from test_gpu_prove_batch_compact import _bytes, _free, _upload
from test_gpu_prove_batch_compact import single as single_compact
from test_gpu_witness_check import Loaded, _expected

pytestmark = pytest.mark.gpu

R = O.R
SECRET = 0x5EC2E7D00D51
CH = (0x1234567DEADBEEF, 0xABCDEF0123456789ABCDEF, 0x55AA55AA77)   # alpha, beta, gamma injected into the round API
ZETA = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0
V_BATCH = 0x7E57AB1E0F0F0F0F1234
MID = {3: 1, 4: 5, 5: 1, 6: 1, 12: 2049}                            # pi_len of witness 1; the five lengths are 0, mid, n, 0, n
MEMBERS = {1: [2], 4: [0, 1, 2, 3], 5: [0, 1, 2, 3, 4]}             # the witnesses of a batch of 1, 4 and 5
COMPACT_KEYS = ("commit", "z_commit", "t_commit", "witness", "evals")


def _pt(p):
    return g1_unpack_one(p[0], p[1])


def _fr(a):
    return fr_unpack(a)[0]


def _col(pi):
    return fr_pack(pi) if pi else None


def _other(pi):
    """public values that differ from `pi` in one entry (from no public values: in having one)"""
    return [(pi[0] + 1) % R] + list(pi[1:]) if pi else [1]


class Case:
    """circuit(log_n) on the device under `cosets`, its five witnesses, and (python=True) its Python setup and proofs, each
    computed once"""

    def __init__(self, ctx, log_n, cosets=PO.COSETS, python=True):
        self.ctx, self.log_n, self.ks = ctx, log_n, tuple(cosets)
        self.n, _, self.q, self.perm = G.circuit(log_n)
        assert G.cosets_are_disjoint(self.ks, self.n)
        self.loaded = Loaded(ctx, log_n, [W.mont_words(self.q[name]) for name in W.SELECTORS], self.perm, self.ks)
        self.cid, self.cosets = self.loaded.cid, self.loaded.cosets
        self.sid = ctx.srs_generate(_limbs(SECRET), self.n + 3)
        self.vk = ctx.circuit_vk(self.sid, self.cid, self.cosets, _g2s())
        self.wits = G.witnesses(log_n, MID[log_n])
        self.words = [[W.mont_words(col) for col in cols] for cols, _ in self.wits]
        self.alias = [next(j for j in range(k + 1) if self.wits[j] == self.wits[k]) for k in range(5)]
        self.ids, self.sig = PO.compile_permutation(self.perm, self.n, log_n, self.ks)
        self.ref = None
        if python:
            srs = O.srs_from_secret_fast(SECRET, self.n + 3)
            self.ref = CR.setup(log_n, self.q, self.perm, srs, PR.srs_g2(SECRET)[1], cosets=self.ks)
        self._srs_words = None
        self._compact, self._reference = {}, {}

    def free(self):
        self.loaded.free()
        self.ctx.srs_free(self.sid)

    # ---- the Python provers ----
    def commit(self, coeffs):
        """the C oracle's MSM against the device's SRS"""
        if self._srs_words is None:
            self._srs_words = self.ctx.srs_download(self.sid)
        xy, inf = self._srs_words
        out, oi = CO.msm_reference(fr_pack(coeffs) if coeffs else np.zeros((0, 4), dtype=np.uint64), xy, inf)
        return g1_unpack_one(out, oi)

    def py_compact(self, k):
        k = self.alias[k]
        if k not in self._compact:
            cols, pi = self.wits[k]
            self._compact[k] = CR.prove(self.ref, cols, pi)
            assert self._compact[k]["r_zeta"] == 0
        return self._compact[k]

    def py_reference(self, k, ch, zeta):
        key = (self.alias[k], tuple(ch), zeta)
        if key not in self._reference:
            cols, pi = self.wits[k]
            ref = PO.prove(self.log_n, cols, self.q, self.perm, G.full_column(pi, self.n), ch, zeta, self.commit, cosets=self.ks)
            assert ref["rem"] == [] and ref["r_open"][1] == 0
            self._reference[key] = ref
        return self._reference[key]

    # ---- the device, one witness ----
    def compact_inputs(self, members):
        return [(self.words[k], self.wits[k][1]) for k in members]

    def prove_compact(self, k, host=False, words=None, pi=None):
        words = self.words[k] if words is None else words
        pi = self.wits[k][1] if pi is None else pi
        if host:
            return self.ctx.prove_compact_host(self.sid, self.cid, words, _col(pi), self.cosets)
        bufs, pibs = _upload(self.ctx, self.n, [(words, pi)])
        try:
            return self.ctx.prove_compact(self.sid, self.cid, bufs[0], pibs[0], len(pi), self.cosets)
        finally:
            _free(bufs, pibs)

    def upload_reference(self, inputs):
        """[(three limb columns, public values)] -> device columns and full public-input columns (None under no public values)"""
        bufs, pibs = [], []
        for words, pi in inputs:
            bs = [self.ctx.alloc(self.n) for _ in range(3)]
            for b, w in zip(bs, words):
                b.upload(w)
            bufs.append(bs)
            pb = None
            if pi:
                pb = self.ctx.alloc(self.n)
                pb.upload(W.mont_words(G.full_column(pi, self.n)))
            pibs.append(pb)
        return bufs, pibs

    def prove_rounds(self, k, batched=False):
        """the round API under the injected challenges"""
        bufs, pibs = self.upload_reference(self.compact_inputs([k]))
        alpha, beta, gamma = CH
        try:
            return self.ctx.prove(self.sid, self.cid, bufs[0], pibs[0], self.cosets,
                                  lambda commits: (_limbs(beta), _limbs(gamma)), lambda commits: (_limbs(alpha), _limbs(ZETA)),
                                  challenge_v=(lambda evals: _limbs(V_BATCH)) if batched else None)
        finally:
            _free(bufs, pibs)

    def prove_native(self, k, words=None, pi=None):
        bufs, pibs = self.upload_reference([(self.words[k] if words is None else words, self.wits[k][1] if pi is None else pi)])
        try:
            return self.ctx.prove_native(self.sid, self.cid, bufs[0], pibs[0], self.cosets)
        finally:
            _free(bufs, pibs)

    def verify(self, proofs, pis, **kw):
        return self.ctx.verify(self.sid, self.cid, _g2s(), self.cosets, proofs, pi=[_col(pi) for pi in pis], **kw)

    # ---- the device, batches: every entry point on the same inputs ----
    def compact_batches(self, inputs):
        """{"device": (proofs, statuses), "host": ..., "single": [(rc, proof)]} of [(limb columns, public values)]"""
        ctx, lens = self.ctx, [len(pi) for _, pi in inputs]
        bufs, pibs = _upload(ctx, self.n, inputs)
        try:
            dev = ctx.prove_batch_compact(self.sid, self.cid, bufs, pibs, lens, self.cosets)
            one = [single_compact(ctx, self, bufs[i], pibs[i], lens[i]) for i in range(len(inputs))]
        finally:
            _free(bufs, pibs)
        host = ctx.prove_batch_compact_host(self.sid, self.cid, [w for w, _ in inputs], [_col(pi) for _, pi in inputs], self.cosets)
        return {"device": dev, "host": host, "single": one}

    def reference_batches(self, inputs):
        ctx = self.ctx
        bufs, pibs = self.upload_reference(inputs)
        try:
            dev = ctx.prove_batch(self.sid, self.cid, bufs, pibs, self.cosets)
            one = [single_reference(ctx, self.sid, self.cid, bufs[i], pibs[i], self.cosets) for i in range(len(inputs))]
        finally:
            _free(bufs, pibs)
        full = [W.mont_words(G.full_column(pi, self.n)) if pi else None for _, pi in inputs]
        host = ctx.prove_batch_host(self.sid, self.cid, [w for w, _ in inputs], full, self.cosets)
        return {"device": dev, "host": host, "single": one}


@pytest.fixture(scope="module")
def cases(ctx):
    """cases(log_n, ones=False): the Case of that size, under cosets (2, 3, 4) or (1, k1, k2); made once, freed at the end"""
    made = {}

    def get(log_n, ones=False):
        if (log_n, ones) not in made:
            made[log_n, ones] = Case(ctx, log_n, G.large_cosets(log_n) if ones else PO.COSETS, python=log_n < 12)
        return made[log_n, ones]

    yield get
    for c in made.values():
        c.free()


def _assert_compact_equals_python(got, exp, what=None):
    assert _to_python(got) == {key: exp[key] for key in COMPACT_KEYS}, what
    assert {key: _fr(v) for key, v in got["challenges"].items()} == exp["challenges"], what


def _assert_reference_equals_python(got, ref, what=None):
    """a six-opening proof dict against oracle/plonk_oracle.prove, element by element"""
    assert [_pt(p) for p in got["commit"]] == ref["commit"], what
    assert _pt(got["z_commit"]) == ref["z_commit"], what
    assert [_pt(p) for p in got["t_commit"]] == ref["t_commit"], what
    assert [_pt(p) for p in got["witness"]] == [o[0] for o in ref["open"]] + [ref["z_open"][0], ref["zw_open"][0], ref["r_open"][0]], what
    assert [_fr(e) for e in got["evals"]] == [o[1] for o in ref["open"]] + [ref["z_open"][1], ref["zw_open"][1], ref["r_open"][1]], what
    assert _fr(got["evals"][5]) == 0, what


# ---- 2^3 .. 2^6: the verifying key ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,ones", [(3, False), (4, False), (4, True), (5, False)])
def test_verifying_key_equals_the_python_setup(cases, log_n, ones):
    """all eight commitments in their slots ([q_l] and [q_r] differ here), P0, the cosets"""
    c = cases(log_n, ones)
    vk_py = c.ref["vk"]
    assert len(set(vk_py["commitments"])) == 8
    assert [_pt((c.vk.commit_xy[i], c.vk.commit_inf[i])) for i in range(8)] == vk_py["commitments"]
    assert _pt((c.vk.srs0_xy, c.vk.srs0_inf)) == vk_py["srs0"]
    assert [_fr(np.array(c.vk.cosets[i], dtype=np.uint64)) for i in range(3)] == vk_py["cosets"]
    assert c.vk.log_n == log_n
    got = c.ctx.circuit_commitments(c.sid, c.cid)
    assert [_pt(p) for p in got] == vk_py["commitments"]


# ---- the compact shape ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,k", [(3, 0), (3, 1), (3, 2), (4, 1), (5, 0), (5, 1), (5, 2), (6, 1)])
def test_compact_proof_equals_the_python_prover(ctx, cases, log_n, k):
    """typlonk_prove_compact and _host: every point, the seven evaluations, the five challenges; the device verifier and the
    Python one agree on the proof, on a tampered copy and on the proof under public values that differ in one entry (the 2^6
    proof is the Python prover's one big job: the device verifier alone judges it)"""
    from typlonk_amd.capi import proof_to_bytes

    c = cases(log_n)
    pi = c.wits[k][1]
    assert len(pi) == G.pi_lens(log_n, MID[log_n])[k]
    exp = c.py_compact(k)
    dev = c.prove_compact(k)
    _assert_compact_equals_python(dev, exp, "device form")
    _assert_compact_equals_python(c.prove_compact(k, host=True), exp, "host form")
    bad = _tamper_point(dev, "witness", 0)
    other = _other(pi)
    pis = [_col(pi), _col(pi), _col(other)]
    assert ctx.verify_compact(c.vk, [dev, bad, dev], pi=pis).tolist() == [True, False, False]
    data = b"".join(proof_to_bytes(d) for d in (dev, bad, dev))
    assert ctx.verify_compact_bytes(c.vk, data, pi=pis).tolist() == [True, False, False]
    if log_n < 6:
        vk_py = c.ref["vk"]
        assert CR.verify_batch(vk_py, [_to_python(dev), _to_python(bad)], [pi, pi]) == [True, False]
        assert not CR.verify_one(vk_py, _to_python(dev), other)


# ---- the reference shape -----------------------------------------------------------------------------------------------------------
REFERENCE_CASES = [(3, 0), (3, 1), (3, 2), (4, 1), (5, 0), (5, 1), (5, 2)]


@pytest.mark.parametrize("log_n,k", REFERENCE_CASES)
def test_round_api_equals_the_reference_flow(cases, log_n, k):
    """injected challenges: the six-opening proof element by element, and the batched form's two witnesses"""
    c = cases(log_n)
    ref = c.py_reference(k, CH, ZETA)
    six = c.prove_rounds(k)
    _assert_reference_equals_python(six, ref)
    bat = c.prove_rounds(k, batched=True)
    assert bat["batched"] and len(bat["witness"]) == 2
    for key in ("commit", "t_commit"):
        assert [_pt(p) for p in bat[key]] == ref[key]
    assert _pt(bat["z_commit"]) == ref["z_commit"]
    assert all((x == y).all() for x, y in zip(bat["evals"], six["evals"]))
    w_ref, y_ref = PO.batched_opening(ref["wires"] + [ref["z"], ref["r"]], V_BATCH, ZETA, c.commit)
    ev = [_fr(e) for e in bat["evals"]]
    assert _pt(bat["witness"][0]) == w_ref
    assert y_ref == sum(pow(V_BATCH, i, R) * ev[j] for i, j in enumerate((0, 1, 2, 3, 5))) % R
    assert _pt(bat["witness"][1]) == ref["zw_open"][0]


@pytest.mark.parametrize("log_n,k", REFERENCE_CASES)
def test_native_proof_verifies_with_its_public_values(cases, log_n, k):
    """typlonk_prove draws the reference's challenges from its own commitments, and typlonk_verify accepts the proof with the
    prover's sign of PI (the convention test_gpu_verify.test_public_inputs_sign_and_binding pins), rejects it with the
    reference verifier's sign and under public values that differ in one entry"""
    c = cases(log_n)
    pi = c.wits[k][1]
    d = c.prove_native(k)
    assert not d["evals"][5].any()
    beta, gamma = T.challenge12(d["commit"])
    alpha, zeta = T.challenge34(d["commit"] + [d["z_commit"]])
    for name, want in (("beta", beta), ("gamma", gamma), ("alpha", alpha), ("zeta", zeta)):
        assert (d["challenges"][name] == want).all(), name
    assert c.verify([d, d], [pi, _other(pi)], pi_as_prover=True).tolist() == [True, False]
    if pi:
        assert c.verify([d, d], [pi, None]).tolist() == [False, False]
    else:
        assert c.verify([d], [None]).tolist() == [True]


@pytest.mark.parametrize("log_n,k", [(3, 2), (4, 1), (5, 1)])
def test_native_proof_passes_the_python_pairing_verifier(cases, log_n, k):
    """oracle/pairing.plonk_verify (12 pairings, the linearisation commitment from the key's eight commitments) under the
    challenges recomputed with tests/transcript_ref.py.  plonk_verify subtracts PI(zeta) where the prover added it -- the
    reference's two signs -- so it is handed the negated column, as tests/compact_ref.kzg_checks does."""
    c = cases(log_n)
    pi = c.wits[k][1]
    d = c.prove_native(k)
    ev = [_fr(e) for e in d["evals"]]
    wit = [_pt(p) for p in d["witness"]]
    proof = {"commit": [_pt(p) for p in d["commit"]], "open": [(wit[i], ev[i]) for i in range(3)], "z_commit": _pt(d["z_commit"]),
             "z_open": (wit[3], ev[3]), "zw_open": (wit[4], ev[4]), "t_commit": [_pt(p) for p in d["t_commit"]],
             "r_open": (wit[5], ev[5])}
    beta, gamma = [_fr(x) for x in T.challenge12(d["commit"])]
    alpha, zeta = [_fr(x) for x in T.challenge34(d["commit"] + [d["z_commit"]])]
    cm = c.ref["vk"]["commitments"]
    g2, g2s = PR.srs_g2(SECRET)
    column = [-v % R for v in G.full_column(pi, c.n)]
    assert PR.plonk_verify(log_n, proof, cm[:5], c.ref["sigma"], cm[5:], c.ks, column, (alpha, beta, gamma), zeta, g2, g2s)
    if log_n == 3:
        column[0] = (column[0] + 1) % R
        assert not PR.plonk_verify(log_n, proof, cm[:5], c.ref["sigma"], cm[5:], c.ks, column, (alpha, beta, gamma), zeta, g2, g2s)


# ---- batches ------------------------------------------------------------------------------------------------------------------------
def _check_compact_batch(c, members, python=(0, -1)):
    inputs = c.compact_inputs(members)
    out = c.compact_batches(inputs)
    count = len(members)
    assert [rc for rc, _ in out["single"]] == [0] * count
    for form in ("device", "host"):
        proofs, st = out[form]
        assert st == [0] * count and len(proofs) == count, form
        assert [_bytes(d) for d in proofs] == [_bytes(d) for _, d in out["single"]], form
    for i in python:
        _assert_compact_equals_python(out["device"][0][i], c.py_compact(members[i]), members[i])
    assert c.ctx.verify_compact(c.vk, out["device"][0], pi=[_col(pi) for _, pi in inputs]).all()
    return out["device"][0]


def _check_reference_batch(c, members, python=(0, -1)):
    inputs = c.compact_inputs(members)
    out = c.reference_batches(inputs)
    count = len(members)
    assert [rc for rc, _ in out["single"]] == [0] * count
    for form in ("device", "host"):
        proofs, st = out[form]
        assert st == [0] * count and len(proofs) == count, form
        assert all(same(a, b) for a, (_, b) in zip(proofs, out["single"])), form
    for i in python:
        d = out["device"][0][i]
        ch = {name: _fr(v) for name, v in d["challenges"].items()}
        assert (d["challenges"]["beta"] == T.challenge12(d["commit"])[0]).all()
        assert (d["challenges"]["zeta"] == T.challenge34(d["commit"] + [d["z_commit"]])[1]).all()
        ref = c.py_reference(members[i], (ch["alpha"], ch["beta"], ch["gamma"]), ch["zeta"])
        _assert_reference_equals_python(d, ref, members[i])
    assert c.verify(out["device"][0], [pi for _, pi in inputs], pi_as_prover=True).all()
    return out["device"][0]


@pytest.mark.parametrize("log_n", [3, 4, 5])
@pytest.mark.parametrize("count", [1, 4, 5])
def test_compact_batches_equal_single_proofs_and_the_python_prover(cases, log_n, count):
    """typlonk_prove_batch_compact and _host: one group of four with public-input lengths 0, mid, n, 0 (the per-proof has_pi
    branch differs between neighbours), and with five a proof alone in a second group"""
    _check_compact_batch(cases(log_n), MEMBERS[count])


@pytest.mark.parametrize("log_n", [3, 4, 5])
@pytest.mark.parametrize("count", [1, 4, 5])
def test_reference_batches_equal_single_proofs_and_the_python_prover(cases, log_n, count):
    """typlonk_prove_batch and _host, the same batches"""
    _check_reference_batch(cases(log_n), MEMBERS[count])


@pytest.mark.parametrize("log_n", [3, 4, 5])
def test_gate_only_broken_witness_in_position_2_fails_alone(cases, log_n):
    from typlonk_amd.capi import ERR_UNSATISFIED

    c = cases(log_n)
    good = c.compact_inputs(MEMBERS[5])
    bad_cols, row = G.break_gate_only(c.perm, c.wits[2][0])
    assert W.check(c.q, c.perm, bad_cols, c.wits[2][1]) == ([row], [])
    inputs = list(good)
    inputs[2] = ([W.mont_words(col) for col in bad_cols], c.wits[2][1])
    exp = [ERR_UNSATISFIED if i == 2 else 0 for i in range(5)]
    clean, broken = c.compact_batches(good), c.compact_batches(inputs)
    for form in ("device", "host"):
        assert broken[form][1] == exp, form
        assert [_bytes(a) == _bytes(b) for a, b in zip(broken[form][0], clean[form][0])] == [i != 2 for i in range(5)], form
    assert [rc for rc, _ in broken["single"]] == exp
    assert c.ctx.verify_compact(c.vk, broken["device"][0], pi=[_col(pi) for _, pi in inputs]).tolist() == [i != 2 for i in range(5)]
    clean, broken = c.reference_batches(good), c.reference_batches(inputs)
    for form in ("device", "host"):
        assert broken[form][1] == exp, form
        assert [same(a, b) for a, b in zip(broken[form][0], clean[form][0])] == [i != 2 for i in range(5)], form
    assert [rc for rc, _ in broken["single"]] == exp
    assert c.verify(broken["device"][0], [pi for _, pi in inputs], pi_as_prover=True).tolist() == [i != 2 for i in range(5)]


# ---- cosets (1, k1, k2) ---------------------------------------------------------------------------------------------------------------
def test_cosets_1_k1_k2_single_compact_proof(ctx, cases):
    c = cases(4, ones=True)
    assert c.ks[0] == 1 and c.ks != tuple(PO.COSETS)
    exp = c.py_compact(1)
    dev = c.prove_compact(1)
    _assert_compact_equals_python(dev, exp, "device form")
    _assert_compact_equals_python(c.prove_compact(1, host=True), exp, "host form")
    pi = c.wits[1][1]
    assert ctx.verify_compact(c.vk, [dev, dev], pi=[_col(pi), _col(_other(pi))]).tolist() == [True, False]
    # the same witness under the other cosets is another proof
    assert _bytes(cases(4).prove_compact(1)) != _bytes(dev)


def test_cosets_1_k1_k2_batches(cases):
    """the k_0 = 1 path of the batched quotient kernel, both shapes"""
    c = cases(4, ones=True)
    _check_compact_batch(c, MEMBERS[5])
    _check_reference_batch(c, MEMBERS[5], python=(2,))


# ---- 2^12 rows --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case12(cases):
    c = cases(12)
    c.sigma_polys = [O.interpolate(s, 12) for s in c.sig]
    return c


def _up(ctx, words):
    b = ctx.alloc(len(words))
    b.upload(words)
    return b


def test_grand_product_at_2_12(ctx, case12):
    """typlonk_grand_product_dev against CompiledPermutation::prove value for value: the honest witness (the product closes)
    and the copy-only broken one (it does not)"""
    c = case12
    beta, gamma = CH[1], CH[2]
    cols, pi = c.wits[2]
    bad, bad_pi, pairs = G.break_copy_only(c.q, c.perm, cols, pi)
    assert W.check(c.q, c.perm, bad, bad_pi) == ([], pairs)
    sb = [_up(ctx, W.mont_words(s)) for s in c.sig]
    z = ctx.alloc(c.n)
    try:
        for wc, closes in ((cols, True), (bad, False)):
            ref = PO.grand_product(wc, c.ids, c.sig, beta, gamma, c.n)
            assert (ref[c.n] == 1) == closes and ref[0] == 1
            wb = [_up(ctx, W.mont_words(col)) for col in wc]
            ctx.grand_product_dev(c.log_n, wb, sb, _limbs(beta), _limbs(gamma), c.cosets, z)
            got = z.download()
            for b in wb:
                b.free()
            assert (got == W.mont_words(ref[:c.n])).all(), closes
    finally:
        for b in sb + [z]:
            b.free()


def test_quotient_identity_at_2_12(ctx, case12):
    """typlonk_quotient_dev on the loaded circuit with a non-zero PI polynomial: t(x) (x^n - 1) == numerator(x) at two points,
    the numerator's first line with all five selector terms and PI, the circuit's own cosets; nothing above degree 3n - 4"""
    c = case12
    n, log_n = c.n, c.log_n
    alpha, beta, gamma = CH
    cols, pi = c.wits[1]
    assert len(pi) == 2049 and any(pi)
    acc = PO.grand_product(cols, c.ids, c.sig, beta, gamma, n)
    assert acc[n] == 1
    polys = {"wires": [O.interpolate(col, log_n) for col in cols], "z": O.interpolate(acc[:n], log_n),
             "q": {name: O.interpolate(c.q[name], log_n) for name in W.SELECTORS},
             "pi": O.interpolate(G.full_column(pi, n), log_n)}
    pad = lambda p: W.mont_words(list(p) + [0] * (n - len(p)))   # noqa: E731
    bufs = [_up(ctx, pad(p)) for p in polys["wires"] + [polys["z"], polys["pi"]]]
    t_out = ctx.alloc(4 * n)
    try:
        ctx.quotient_dev(log_n, bufs[:3], bufs[3], None, None, bufs[4], _limbs(alpha), _limbs(beta), _limbs(gamma), c.cosets,
                         t_out, circuit=c.cid)
        t = fr_unpack(t_out.download())
    finally:
        for b in bufs + [t_out]:
            b.free()
    assert len(t) == 4 * n and not any(t[3 * n - 3:])
    wroot = O.domain_root(log_n)
    for x in (0x1234567, 0xFEDCBA9876543210FEDCBA):
        ev = lambda p: O.poly_eval(p, x)  # noqa: E731
        a, b, cc = (ev(p) for p in polys["wires"])
        z, zw = ev(polys["z"]), O.poly_eval(polys["z"], x * wroot % R)
        q = {name: ev(p) for name, p in polys["q"].items()}
        s = [ev(p) for p in c.sigma_polys]
        line1 = q["q_l"] * a + q["q_r"] * b - q["q_o"] * cc + q["q_m"] * a * b + q["q_c"] + ev(polys["pi"])
        line2 = (a + beta * c.ks[0] * x + gamma) * (b + beta * c.ks[1] * x + gamma) * (cc + beta * c.ks[2] * x + gamma) * z
        line3 = (a + beta * s[0] + gamma) * (b + beta * s[1] + gamma) * (cc + beta * s[2] + gamma) * zw
        zh = pow(x, n, R) - 1
        l0 = zh * pow(n * (x - 1), -1, R)
        num = (line1 + alpha * (line2 - line3) + alpha * alpha * (z - 1) * l0) % R
        assert O.poly_eval(t, x) * zh % R == num
        assert all(q.values()) and q["q_l"] != q["q_r"]


def test_verifying_key_at_2_12(ctx, case12):
    """the eight commitments equal the C oracle's MSM of the C oracle's interpolation of each table"""
    c = case12
    xy, inf = ctx.srs_download(c.sid)
    tables = [c.q[name] for name in W.SELECTORS] + c.sig
    got = ctx.circuit_commitments(c.sid, c.cid)
    for i, t in enumerate(tables):
        coeffs = CO.ntt(W.mont_words(t), c.log_n, inverse=True)
        exp, einf = CO.msm_reference(coeffs, xy[:c.n], inf[:c.n])
        assert (np.array(c.vk.commit_xy[i], dtype=np.uint64) == exp).all() and int(c.vk.commit_inf[i]) == int(einf), i
        assert (got[i][0] == exp).all() and got[i][1] == int(einf), i
    assert _pt((c.vk.srs0_xy, c.vk.srs0_inf)) == O.G1


def _python_vk(c):
    return {"log_n": c.log_n, "cosets": list(c.ks), "commitments": [_pt((c.vk.commit_xy[i], c.vk.commit_inf[i])) for i in range(8)],
            "srs0": _pt((c.vk.srs0_xy, c.vk.srs0_inf)), "g2s": PR.srs_g2(SECRET)[1]}


@pytest.mark.parametrize("k", [0, 1, 2])
def test_compact_proof_at_2_12(ctx, case12, k):
    """public-input lengths 0, 2049 and n: the seven evaluations equal Horner on the interpolated columns at the proof's own
    zeta (Z from CompiledPermutation::prove under the proof's beta and gamma); with the key test_verifying_key_at_2_12 checks,
    the Python verifier accepts the proof and rejects it under one changed public value, and so does the device"""
    c = case12
    n, log_n = c.n, c.log_n
    cols, pi = c.wits[k]
    assert len(pi) == (0, 2049, n)[k]
    d = c.prove_compact(k)
    host = c.prove_compact(k, host=True)
    assert _bytes(d) == _bytes(host)
    ch = {name: _fr(v) for name, v in d["challenges"].items()}
    zeta, w = ch["zeta"], O.domain_root(log_n)
    acc = PO.grand_product(cols, c.ids, c.sig, ch["beta"], ch["gamma"], n)
    assert acc[n] == 1
    z = O.interpolate(acc[:n], log_n)
    exp = [O.poly_eval(O.interpolate(col, log_n), zeta) for col in cols]
    exp += [O.poly_eval(z, zeta), O.poly_eval(z, zeta * w % R), O.poly_eval(c.sigma_polys[0], zeta), O.poly_eval(c.sigma_polys[1], zeta)]
    assert fr_unpack(np.array(d["evals"])) == exp
    vk_py, pf, other = _python_vk(c), _to_python(d), _other(pi)
    assert list(CR.challenges(vk_py, pf, pi)) == [ch[name] for name in ("beta", "gamma", "alpha", "zeta", "v")]
    assert CR.verify_one(vk_py, pf, pi)
    if pi:
        assert not CR.verify_one(vk_py, pf, other)
    assert ctx.verify_compact(c.vk, [d, d], pi=[_col(pi), _col(other)]).tolist() == [True, False]


def test_batches_at_2_12_equal_single_proofs_and_verify_in_one_call(case12):
    """five proofs in each shape, public-input lengths 0, 2049, n, 0, n"""
    c = case12
    _check_compact_batch(c, MEMBERS[5], python=())
    _check_reference_batch(c, MEMBERS[5], python=())


def test_broken_witnesses_at_2_12(ctx, case12):
    """the gate-only and the copy-only broken witness: TYPLONK_ERR_UNSATISFIED from both proof shapes, the context proves the
    honest witness afterwards, and typlonk_witness_check on the same buffers reports what the Python checker predicts"""
    from typlonk_amd.capi import ERR_UNSATISFIED, TyplonkError

    c = case12
    gate_cols, row = G.break_gate_only(c.perm, c.wits[1][0])
    copy_cols, copy_pi, pairs = G.break_copy_only(c.q, c.perm, *c.wits[2])
    broken = [(gate_cols, c.wits[1][1]), (copy_cols, copy_pi)]
    assert [W.check(c.q, c.perm, wc, pi) for wc, pi in broken] == [([row], []), ([], pairs)]
    before = [c.prove_compact(k) for k in (1, 2)]
    for wc, pi in broken:
        words = [W.mont_words(col) for col in wc]
        bufs, pibs = _upload(ctx, c.n, [(words, pi)])
        try:
            with pytest.raises(TyplonkError) as e:
                ctx.prove_compact(c.sid, c.cid, bufs[0], pibs[0], len(pi), c.cosets)
            assert e.value.code == ERR_UNSATISFIED
            report = ctx.witness_check(c.cid, bufs, pibs, [len(pi)], c.cosets, cap=16)
        finally:
            _free(bufs, pibs)
        assert report == [_expected(c.q, c.perm, wc, pi, 16)]
        with pytest.raises(TyplonkError) as e:
            c.prove_compact(0, host=True, words=words, pi=pi)
        assert e.value.code == ERR_UNSATISFIED
        with pytest.raises(TyplonkError) as e:
            c.prove_native(0, words=words, pi=pi)
        assert e.value.code == ERR_UNSATISFIED
        bufs, pibs = c.upload_reference([(words, pi)])
        try:
            with pytest.raises(TyplonkError) as e:
                ctx.prove(c.sid, c.cid, bufs[0], pibs[0], c.cosets)
            assert e.value.code == ERR_UNSATISFIED
        finally:
            _free(bufs, pibs)
    assert [_bytes(c.prove_compact(k)) for k in (1, 2)] == [_bytes(d) for d in before]
    assert not c.prove_native(1)["evals"][5].any()
    # the honest witnesses on the same entry point: no failure
    bufs, pibs = _upload(ctx, c.n, c.compact_inputs([1, 2]))
    try:
        report = ctx.witness_check(c.cid, bufs, pibs, [len(c.wits[1][1]), len(c.wits[2][1])], c.cosets, cap=16)
    finally:
        _free(bufs, pibs)
    assert report == [{"gate_failures": 0, "copy_failures": 0, "gate_rows": [], "copy_cells": []}] * 2
