"""Circuits of 2^23 and 2^24 rows on one GPU (quotient domains of 2^25 and 2^26 points), against the C oracle:

  * KzgScheme::open (kzg/src/lib.rs:55-61) beyond 2^22 coefficients, where the carries of more than 2048 workgroups are
    scanned in rounds by the single-workgroup top stage (plonk_ops.hip, open_top_rounds);
  * the grand product (permutation/src/proving.rs:7-31) at 2^23 rows: 4096 block products in pscan_top_kernel's loop;
  * fixed-base tables over a (2^24 + 3)-point SRS: table mode for MSMs of up to 2^24 + 3 terms, chunk by chunk;
  * whole proofs at 2^23 and 2^24 rows in both proof shapes, checked as test_config5_prove_at_2_22_both_shapes checks
    the 2^22 proof, plus the native and host-column entry points, and the pairing verifier at 2^23;
  * the prover's cap: 2^25 rows are still refused.

The heavy cases run in a context of their own, closed at the end, so that the suite's shared context does not keep
their workspaces (tens of GiB: include/typlonk.h lists the footprint)."""
import numpy as np
import pytest

from helpers import O, g1_unpack_one

pytestmark = pytest.mark.gpu

R = O.R
ALPHA, BETA, GAMMA = 0x1234567DEADBEEF, 0xABCDEF0123456789ABCDEF, 0x55AA55AA77
ZETA = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0
V_BATCH = 0x1F2E3D4C5B6A7988
SECRET = 0x0123456789ABCDEF0123456789ABCDEF
KS = (1, 7, 13)


def _limbs(v):
    return np.array(O.fr_to_mont_limbs(v % R), dtype=np.uint64)


def _rand(rng, n):
    """n random Montgomery-form words below 2^255 (every such word is a valid input of these functions)"""
    a = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64(0x0FFFFFFFFFFFFFFF)
    return a


def _up(ctx, a):
    b = ctx.alloc(a.shape[0])
    b.upload(a)
    return b


@pytest.fixture
def big_ctx(built):
    """a context of its own: its workspaces go with it"""
    import torch

    import typlonk_amd

    c = typlonk_amd.Context(0)
    try:
        yield c
    finally:
        c.close()
        torch.cuda.empty_cache()


@pytest.mark.slow
def test_open_beyond_2_22_coefficients(big_ctx):
    """y = p(z) and every word of (p - y) / (X - z) equal the C oracle's synthetic division for m around the old 2^22 limit
    (one round of carries: 2047 or 2048 workgroups; 2049: two rounds, the upper one a single entry) and at 2^23 + 5 and
    2^24 (4097 and 8192 workgroups)"""
    from conftest import need_resources
    from oracle import coracle as CO

    need_resources(host_gib=6, hbm_gib=2)
    ctx = big_ctx
    top = 1 << 24
    rng = np.random.default_rng(0x0BE7)
    p = _rand(rng, top)
    pb, qb = _up(ctx, p), ctx.alloc(top)
    zpt = _limbs(0xDEADBEEFCAFEF00D0123456789ABCDEF)
    for m in ((1 << 22) - 1, 1 << 22, (1 << 22) + 1, (1 << 23) + 5, 1 << 24):
        q_exp, y_exp = CO.poly_div_linear(p[:m], zpt)
        y = ctx.open_dev(pb, m, zpt, qb)
        assert (y == y_exp).all(), m
        assert (qb.download(0, m - 1) == q_exp).all(), m
        # evaluation only (no quotient), and at an offset
        assert (ctx.open_dev(pb, m - 1, zpt, offset=1) == CO.poly_eval(p[1:m], zpt)).all(), m
    pb.free()
    qb.free()


@pytest.mark.slow
def test_grand_product_at_2_23_rows(big_ctx):
    """Z over 2^23 rows equals oracle_grand_product word for word (as tests/test_gpu_full_size_vs_cpu.py does up to 2^22)"""
    import ctypes as C

    from conftest import need_resources
    from oracle import coracle as CO
    from oracle.cpu_prover import _p64, _ptrs

    need_resources(host_gib=8, hbm_gib=6)
    ctx = big_ctx
    log_n = 23
    n = 1 << log_n
    rng = np.random.default_rng(300 + log_n)
    wires = [_rand(rng, n) for _ in range(3)]
    sigma = [_rand(rng, n) for _ in range(3)]
    k_l = np.ascontiguousarray(np.stack([_limbs(k) for k in KS]))
    exp = np.zeros((n, 4), dtype=np.uint64)
    last = np.zeros(4, dtype=np.uint64)
    rc = CO.lib().oracle_grand_product(_ptrs(wires), _ptrs(sigma), _p64(_limbs(BETA)), _p64(_limbs(GAMMA)), _p64(k_l),
                                       C.c_uint32(log_n), _p64(exp), _p64(last))
    assert rc == 0
    wb, sb = [_up(ctx, w) for w in wires], [_up(ctx, s) for s in sigma]
    z = ctx.alloc(n)
    ctx.grand_product_dev(log_n, wb, sb, _limbs(BETA), _limbs(GAMMA), [_limbs(k) for k in KS], z)
    assert (z.download() == exp).all()
    for bf in wb + sb + [z]:
        bf.free()


@pytest.mark.slow
def test_tables_over_a_2_24_plus_3_point_srs(big_ctx):
    """srs_precompute(sid, 20) accepts the SRS of a 2^24-row proof; stand-alone MSMs and one batch of every length from the
    full SRS down to len / 4 equal [p(s)]G (kzg/src/lib.rs:102-105), and the profile shows the table-mode segmented sort
    -- never the counting sort (msm_digits, msm_scan) that a plain MSM of more than 2^23 terms takes"""
    from conftest import need_resources
    from oracle import coracle as CO

    need_resources(host_gib=6, hbm_gib=48)
    ctx = big_ctx
    length = (1 << 24) + 3
    s_limbs = _limbs(SECRET)
    sid = ctx.srs_generate(s_limbs, length)
    ctx.srs_precompute(sid, 20)
    rng = np.random.default_rng(0x7AB1E5)
    sc = _rand(rng, length)
    buf = _up(ctx, sc)
    ms = [length, 1 << 24, (1 << 23) + 1, (length + 3) // 4]
    exp = [CO.g1_mul_generator(CO.poly_eval(sc[:m], s_limbs)) for m in ms]
    for m, (exp_xy, exp_inf) in zip(ms, exp):
        ctx.set_profiling(True)
        got, ginf = ctx.msm_devptr(sid, buf.devptr, m)
        names = [nm for nm, _ in ctx.profile()]
        ctx.set_profiling(False)
        assert (got == exp_xy).all() and ginf == exp_inf, m
        assert any(nm.startswith("msm_sort") for nm in names), (m, names)
        assert not any(nm in ("msm_digits", "msm_scan") for nm in names), (m, names)
    ctx.set_profiling(True)
    outs = ctx.msm_batch_devptr(sid, [buf.devptr] * len(ms), ms)
    names = [nm for nm, _ in ctx.profile()]
    ctx.set_profiling(False)
    for m, (got, ginf), (exp_xy, exp_inf) in zip(ms, outs, exp):
        assert (np.asarray(got) == exp_xy).all() and ginf == exp_inf, ("batch", m)
    assert not any(nm in ("msm_digits", "msm_scan") for nm in names), names
    buf.free()
    ctx.srs_free(sid)


def _same(a, b):
    return bool((np.asarray(a[0]) == np.asarray(b[0])).all() and int(a[1]) == int(b[1]))


def _same_proof(got, ref):
    for key in ("commit", "t_commit", "witness"):
        assert len(got[key]) == len(ref[key]) and all(_same(a, b) for a, b in zip(got[key], ref[key])), key
    assert _same(got["z_commit"], ref["z_commit"])
    assert all((np.asarray(a) == np.asarray(b)).all() for a, b in zip(got["evals"], ref["evals"]))


@pytest.fixture
def fast_poly_ops(monkeypatch):
    """oracle.pairing's O(n) steps -- interpolate the public inputs, evaluate the sigma polynomials at zeta -- on the C oracle
    for inputs given as limb arrays (pure Python would take minutes at 2^23 rows); integer lists keep the Python forms"""
    from oracle import coracle as CO
    from oracle import pairing as PR

    interp, peval = PR.O.interpolate, PR.O.poly_eval

    def interpolate(evals, log_n):
        if isinstance(evals, np.ndarray):
            return CO.ntt(evals, log_n, inverse=True, threads=0)
        return interp(evals, log_n)

    def poly_eval(coeffs, x):
        if isinstance(coeffs, np.ndarray):
            return O.fr_from_mont_limbs([int(v) for v in CO.poly_eval(coeffs, _limbs(x))])
        return peval(coeffs, x)

    monkeypatch.setattr(PR.O, "interpolate", interpolate)
    monkeypatch.setattr(PR.O, "poly_eval", poly_eval)


@pytest.mark.slow
@pytest.mark.parametrize("log_n,hbm_gib", [(23, 56), (24, 96)])
def test_prove_at_large_domains_both_shapes(big_ctx, fast_poly_ops, log_n, hbm_gib):
    """A 2^23- and a 2^24-row squaring chain proved on one GPU in both proof shapes, checked as the 2^22 proof is
    (tests/test_gpu_prove.py::test_config5_prove_at_2_22_both_shapes): r(zeta) = 0, the wire commitments equal [p(s)]G,
    every opening satisfies the verifier's equation in trapdoor form -- for [r] the verifier's own linearisation
    commitment --, and the batched witness is the v-combination of the six.  typlonk_prove equals the round-by-round flow
    and typlonk_prove_host equals typlonk_prove; at 2^23 the pairing verifier accepts the proof and rejects a changed
    evaluation."""
    from conftest import need_resources
    from oracle import coracle as CO
    from oracle import pairing as PR
    from oracle import plonk_oracle as PO
    from typlonk_amd.circuits import SquaringChain

    need_resources(host_gib=24, hbm_gib=hbm_gib)
    ctx = big_ctx
    n = 1 << log_n
    s_l = _limbs(SECRET)
    chain = SquaringChain(ctx, log_n, keep_host=True)
    sid = ctx.srs_generate(s_l, n + 3)
    ctx.srs_precompute(sid, 20)
    chal = (lambda c: (_limbs(BETA), _limbs(GAMMA)), lambda c: (_limbs(ALPHA), _limbs(ZETA)))
    six = ctx.prove(sid, chain.circuit, chain.wire_evals, chain.pi_evals, chain.cosets, *chal)
    bat = ctx.prove(sid, chain.circuit, chain.wire_evals, chain.pi_evals, chain.cosets, *chal,
                    challenge_v=lambda e: _limbs(V_BATCH))
    # the native entry points: one call with the transcript inside, from device buffers and from host columns
    ref = ctx.prove(sid, chain.circuit, chain.wire_evals, None, chain.cosets)
    nat = ctx.prove_native(sid, chain.circuit, chain.wire_evals, None, chain.cosets)
    _same_proof(nat, ref)
    host = chain.host_inputs()
    hst = ctx.prove_native_host(sid, chain.circuit, host["wires"], None, chain.cosets)
    _same_proof(hst, nat)
    assert all((hst["challenges"][k] == nat["challenges"][k]).all() for k in ("beta", "gamma", "alpha", "zeta"))
    assert not nat["evals"][5].any()
    del ref, nat, hst

    pt = lambda t: g1_unpack_one(t[0], t[1])                   # noqa: E731
    fr = lambda a: O.fr_from_mont_limbs([int(x) for x in a])   # noqa: E731
    ev = [fr(e) for e in six["evals"]]
    assert ev[5] == 0 and [fr(e) for e in bat["evals"]] == ev

    def at_s(evals):      # p(s) for p = interpolate(evals)
        coeffs = CO.ntt(evals, log_n, inverse=True, threads=0)
        return coeffs, fr(CO.poly_eval(coeffs, s_l))

    commits = [pt(c) for c in six["commit"]]
    for i in range(3):
        _, ps = at_s(host["wires"][i])
        assert commits[i] == O.g1_mul(O.G1, ps), f"wire commitment {i}"
    assert [pt(c) for c in bat["commit"]] == commits and pt(bat["z_commit"]) == pt(six["z_commit"])
    assert [pt(c) for c in bat["t_commit"]] == [pt(c) for c in six["t_commit"]]
    w = O.domain_root(log_n)
    wit = [pt(x) for x in six["witness"]]
    zc = pt(six["z_commit"])
    trapdoor = lambda W, C, z, y: O.g1_mul(W, (SECRET - z) % R) == O.g1_add(C, O.g1_neg(O.g1_mul(O.G1, y)))   # noqa: E731
    for i in range(3):
        assert trapdoor(wit[i], commits[i], ZETA, ev[i]), f"opening {i}"
    assert trapdoor(wit[3], zc, ZETA, ev[3]) and trapdoor(wit[4], zc, ZETA * w % R, ev[4])
    _, sel_s = at_s(host["selectors"][2])                      # q_o = q_m; q_l = q_r = q_c = 0
    q_pt = O.g1_mul(O.G1, sel_s)
    fixed = [None, None, q_pt, q_pt, None]
    sig = [at_s(x) for x in host["sigma"]]
    sigma_polys = [cf for cf, _ in sig]
    sigma_c = [O.g1_mul(O.G1, ps) for _, ps in sig]
    sigma_ev = [fr(CO.poly_eval(cf, _limbs(ZETA))) for cf in sigma_polys]
    t_commit = [pt(c) for c in six["t_commit"]]
    r_commit = PR.linearisation_commitment(log_n, fixed, sigma_c, sigma_ev, PO.COSETS, ev[:3], zc, (ev[3], ev[4]), ZETA,
                                           t_commit, (ALPHA, BETA, GAMMA), 0)
    assert trapdoor(wit[5], r_commit, ZETA, 0), "opening of r"
    bw = [pt(x) for x in bat["witness"]]
    comb = None
    for k, i in enumerate((0, 1, 2, 3, 5)):
        comb = O.g1_add(comb, O.g1_mul(wit[i], pow(V_BATCH, k, R)))
    assert bw[0] == comb and bw[1] == wit[4]
    if log_n == 23:
        proof = {"commit": commits, "open": [(wit[i], ev[i]) for i in range(3)], "z_commit": zc, "z_open": (wit[3], ev[3]),
                 "zw_open": (wit[4], ev[4]), "t_commit": t_commit, "r_open": (wit[5], ev[5])}
        g2, g2s = PR.srs_g2(SECRET)
        args = (fixed, sigma_polys, sigma_c, PO.COSETS, np.zeros((n, 4), dtype=np.uint64), (ALPHA, BETA, GAMMA), ZETA, g2, g2s)
        assert PR.plonk_verify(log_n, proof, *args)
        bad = dict(proof, open=[(wit[0], (ev[0] + 1) % R)] + proof["open"][1:])
        assert not PR.plonk_verify(log_n, bad, *args)
    chain.free()
    ctx.srs_free(sid)


def test_circuit_load_refuses_2_25_rows(ctx):
    """the single-GPU prover stops at 2^24 rows (TYPLONK_MAX_PROVER_LOG_N): log_n = 25 is refused before any buffer is read"""
    from typlonk_amd.capi import ERR_DOMAIN, TyplonkError

    bufs = [ctx.alloc(4) for _ in range(8)]
    with pytest.raises(TyplonkError) as e:
        ctx.circuit_load(25, bufs[:5], bufs[5:])
    assert e.value.code == ERR_DOMAIN
    for b in bufs:
        b.free()
