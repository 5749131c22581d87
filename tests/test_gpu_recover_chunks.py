"""typlonk_recover_chunks on the GPU: polynomials from a subset of their cells.  The truth is the polynomial the cells were made
from -- nothing here trusts the recipe of tests/recover_chunks_ref.py --: its coefficients word for word, its evaluations in
typlonk_open_chunks_*'s order from tests/open_chunks_ref.py, the host and the device outputs against each other, the device
outputs at a nonzero offset with the words around them kept.

These tests FAIL on a commit before typlonk_recover_chunks: the symbol and Context.recover_chunks do not exist there.  That is
expected and they do not skip.

  1. every (log_n, log_l) with log_n <= 6, K in {ceil(m / l), r / 2, r - 1, r}, m in {1, l, K l - 1, K l}, random known sets
  2. the sampler's shape (13, 6), m = 4096, K = 64: a random half, the first half, the odd cosets; then typlonk_open_chunks_dev on the
     returned buffers gives the proofs of the original polynomials, and typlonk_verify_chunks accepts recovered cells in one fold
  3. more missing cosets than one tile and one slice: (10, 0) with K = m = 400, (12, 2) with K = 512, and (14, 0) with K = 8192, where
     a slice of the plan's own holds whole tiles
  4. inconsistent inputs by construction (first_excess is where the coefficient was put), one evaluation changed under redundancy,
     the same change at m = K l against Lagrange interpolation, a bad polynomial between two good ones
  5. evaluations that are no canonical residues   6. every refusal, with every output untouched
  7. the order of the cosets, and two calls in a row   8. under profiling   9. the C++ mirror"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import open_chunks_ref as FK
import recover_chunks_ref as RR
from helpers import O, fr_pack, fr_unpack, g1_pack

pytestmark = pytest.mark.gpu

R = O.R
OK, BAD_EVAL, INCONSISTENT, NO_EXCESS = RR.OK, RR.BAD_EVAL, RR.INCONSISTENT, RR.NO_EXCESS
MARK = 0x0123456789ABCDEF          # what a buffer holds around the words a call may write
PAD = 3                            # the offset of a device output, and the words kept behind it


def _limbs(v):
    return np.array(O.fr_to_mont_limbs(v % R), dtype=np.uint64)


def _rand(rng, k):
    return [int.from_bytes(rng.bytes(32), "little") % R for _ in range(k)]


def _cells(fs, cosets, log_n, log_l):
    """(count, K, l, 4): the cells of the polynomials on the named cosets, in that order, and the chunk-major evaluations"""
    n, l, r = RR.shape(log_n, log_l)
    evs = [FK.evaluations(f, log_n, log_l) for f in fs]
    packed = [fr_pack(e).reshape(r, l, 4) for e in evs]
    return np.ascontiguousarray(np.stack([p[list(cosets)] for p in packed])), np.stack(packed)


def _recover(ctx, log_n, log_l, m, cosets, cells, want_evals=True, dev=True):
    """the call with every output; the device outputs at offset PAD of marked buffers, checked against the host's and for the marks"""
    count = cells.shape[0]
    bufs = None
    if dev:
        bufs = [ctx.alloc(m + 2 * PAD) for _ in range(count)]
        for b in bufs:
            b.upload(np.full((m + 2 * PAD, 4), MARK, dtype=np.uint64))
    out = ctx.recover_chunks(log_n, log_l, m, cosets, cells, out_bufs=bufs, offsets=None if bufs is None else [PAD] * count,
                             want_coeffs=True, want_evals=want_evals)
    if dev:
        for p, b in enumerate(bufs):
            got = b.download()
            assert (got[:PAD] == MARK).all() and (got[PAD + m:] == MARK).all(), "a word outside the destination was written"
            assert (got[PAD:PAD + m] == out["coeffs"][p]).all(), "the host and the device outputs differ"
        out["bufs"] = bufs
    return out


def _check_exact(out, fs, m, all_evals, log_n):
    count = len(fs)
    assert (out["status"] == OK).all() and (out["first_excess"] == NO_EXCESS).all() and out["count"] == [count, 0, 0]
    for p, f in enumerate(fs):
        assert (out["coeffs"][p] == fr_pack(f + [0] * (m - len(f)))).all(), p
        if "evals" in out:
            assert (out["evals"][p] == all_evals[p]).all(), p


# ---- 1. every small shape -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,log_l", [(a, b) for a in range(1, 7) for b in range(a)])
def test_every_small_shape(ctx, log_n, log_l):
    n, l, r = RR.shape(log_n, log_l)
    rng = np.random.default_rng(100 * log_n + log_l)
    tried = set()
    for K0 in sorted({1, max(r // 2, 1), max(r - 1, 1), r}):
        for m in sorted({1, l, max(K0 * l - 1, 1), K0 * l}):
            for K in sorted({K0, -(-m // l)}):                      # and the fewest cells this m admits
                if m > K * l or (K, m) in tried:
                    continue
                tried.add((K, m))
                cosets = [int(x) for x in rng.permutation(r)[:K]]
                fs = [_rand(rng, m), _rand(rng, m)]
                cells, all_evals = _cells(fs, cosets, log_n, log_l)
                out = _recover(ctx, log_n, log_l, m, cosets, cells)
                assert (out["known"], out["missing"]) == (K, r - K)
                _check_exact(out, fs, m, all_evals, log_n)


# ---- 2. the sampler's shape, and on to the proofs -------------------------------------------------------------------------------
def test_the_samplers_shape_then_open_and_verify(ctx):
    from oracle import pairing as OP
    import verify_chunks_ref as VR

    log_n, log_l, m, K = 13, 6, 4096, 64
    n, l, r = RR.shape(log_n, log_l)
    rng = np.random.default_rng(0x5A)
    s = _rand(rng, 1)[0]
    fs = [_rand(rng, m) for _ in range(3)]
    sid = ctx.srs_generate(_limbs(s), n)
    tab = ctx.srs_open_chunks_table(sid, log_n, log_l)
    try:
        want_xy, want_inf, want_ev = ctx.open_chunks(tab, [fr_pack(f) for f in fs])        # the proofs of the original polynomials
        # (a few of them against the big integers: [q_k(s)] G by schoolbook division)
        for k in (0, 77, r - 1):
            q, _ = FK.divide(fs[0], l, pow(O.domain_root(log_n), k * l, R))
            xy, inf = g1_pack([O.g1_mul(O.G1, O.poly_eval(q, s))])
            assert (want_xy[0, k] == xy[0]).all() and want_inf[0, k] == inf[0]
        known_sets = {"a random half": [int(x) for x in rng.permutation(r)[:K]], "the first half": list(range(K)),
                      "the odd cosets": list(range(1, r, 2))}
        all_evals = None
        for name, cosets in known_sets.items():
            cells, all_evals = _cells(fs, cosets, log_n, log_l) if all_evals is None else (np.ascontiguousarray(all_evals[:, cosets]), all_evals)
            assert (all_evals == want_ev).all()
            out = _recover(ctx, log_n, log_l, m, cosets, cells)
            _check_exact(out, fs, m, all_evals, log_n)
            xy, inf, ev = ctx.open_chunks(tab, out["bufs"], m=m, offsets=[PAD] * 3)
            assert (xy == want_xy).all() and (inf == want_inf).all() and (ev == want_ev).all(), name
        # eight recovered cells -- of cosets the last call was NOT given -- with their proofs, in one fold
        missing = [k for k in range(r) if k not in set(cosets)]
        picks = [(p, missing[i]) for i, p in enumerate([0, 1, 2, 0, 1, 2, 0, 1])]
        cm = [ctx.msm(sid, fr_pack(f)) for f in fs]
        cxy = np.array([c[0] for c in cm], dtype=np.uint64).reshape(3, 12)
        cinf = np.array([c[1] for c in cm], dtype=np.uint8).reshape(3)
        g2sl = np.array(VR.g2_limbs(OP.srs_g2(pow(s, l, R))[1]), dtype=np.uint64)
        ps, ks = [c[0] for c in picks], [c[1] for c in picks]
        got = ctx.verify_chunks(sid, log_n, log_l, g2sl, bytes(range(32)), (cxy, cinf), np.array(ps, dtype=np.uint32),
                                np.array(ks, dtype=np.uint32), out["evals"][ps, ks].copy(), (xy[ps, ks].copy(), inf[ps, ks].copy()))
        assert (got["status"] == 0).all() and got["folds"] == 1
    finally:
        ctx.srs_free(tab)
        ctx.srs_free(sid)


# ---- 3. past one tile and one slice ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,log_l,K,m", [(10, 0, 400, 400), (12, 2, 512, 1500), (14, 0, 8192, 5000)])
def test_more_missing_cosets_than_one_tile_and_one_slice(ctx, log_n, log_l, K, m):
    n, l, r = RR.shape(log_n, log_l)
    rng = np.random.default_rng(K)
    cosets = [int(x) for x in rng.permutation(r)[:K]]
    fs = [_rand(rng, m), _rand(rng, m - 1)]
    cells, all_evals = _cells(fs, cosets, log_n, log_l)
    _check_exact(_recover(ctx, log_n, log_l, m, cosets, cells), fs, m, all_evals, log_n)


# ---- 4. inconsistent inputs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,log_l,K,m", [(6, 2, 9, 17), (5, 0, 31, 1), (6, 5, 2, 33), (10, 3, 100, 300)])
def test_inconsistent_by_construction(ctx, log_n, log_l, K, m):
    n, l, r = RR.shape(log_n, log_l)
    kl = K * l
    rng = np.random.default_rng(m)
    cosets = [int(x) for x in rng.permutation(r)[:K]]
    spots = sorted({m, (m + kl) // 2, kl - 1})
    good = _rand(rng, m)
    hs = []
    for j in spots:                                                   # h of degree < K l with one chosen coefficient at j >= m
        h = _rand(rng, m) + [0] * (kl - m)
        h[j] = _rand(rng, 1)[0] or 1
        hs.append(h)
    fs = hs[:1] + [good] + hs[1:]
    cells, all_evals = _cells(fs, cosets, log_n, log_l)
    out = _recover(ctx, log_n, log_l, m, cosets, cells)
    want_status = [INCONSISTENT, OK] + [INCONSISTENT] * (len(spots) - 1)
    assert list(out["status"]) == want_status and out["count"] == [1, 0, len(spots)]
    assert list(out["first_excess"]) == [spots[0], NO_EXCESS] + spots[1:]
    for p in range(len(fs)):
        if p == 1:
            assert (out["coeffs"][p] == fr_pack(good)).all() and (out["evals"][p] == all_evals[p]).all()
        else:
            assert not out["coeffs"][p].any() and not out["evals"][p].any()
    # the same cells with m = K l: an interpolation, every h exactly
    _check_exact(_recover(ctx, log_n, log_l, kl, cosets, cells), fs, kl, all_evals, log_n)


def test_one_changed_evaluation(ctx):
    log_n, log_l, K, m = 5, 2, 5, 9
    n, l, r = RR.shape(log_n, log_l)
    kl = K * l
    rng = np.random.default_rng(11)
    cosets = [6, 0, 3, 7, 2]
    fs = [_rand(rng, m) for _ in range(3)]
    cells, all_evals = _cells(fs, cosets, log_n, log_l)
    changed = cells.copy()
    bad_value = (RR.cells_of(fs[1], cosets, log_n, log_l)[2][1] + 1) % R
    changed[1, 2, 1] = _limbs(bad_value)
    out = _recover(ctx, log_n, log_l, m, cosets, changed)
    # the middle one is bad: the outer two exactly, the middle outputs zeros
    assert list(out["status"]) == [OK, INCONSISTENT, OK] and out["count"] == [2, 0, 1] and m <= out["first_excess"][1] < kl
    for p in (0, 2):
        assert (out["coeffs"][p] == fr_pack(fs[p])).all() and (out["evals"][p] == all_evals[p]).all()
    assert not out["coeffs"][1].any() and not out["evals"][1].any()
    # with m = K l the changed values are interpolated: Lagrange through the K l points
    out = _recover(ctx, log_n, log_l, kl, cosets, changed)
    assert (out["status"] == OK).all()
    ys = [y for c in RR.cells_of(fs[1], cosets, log_n, log_l) for y in c]
    ys[2 * l + 1] = bad_value
    want = RR.lagrange(RR.points(cosets, log_n, log_l), ys)
    assert want[m:] != [0] * (kl - m)
    assert (out["coeffs"][1] == fr_pack(want)).all()
    assert (out["evals"][1] == fr_pack(FK.evaluations(want, log_n, log_l)).reshape(r, l, 4)).all()


# ---- 5. evaluations that are no residues ----------------------------------------------------------------------------------------
def test_evaluations_that_are_no_residues(ctx):
    log_n, log_l, K, m = 6, 3, 5, 33
    rng = np.random.default_rng(12)
    cosets = [1, 7, 4, 2, 0]
    fs = [_rand(rng, m) for _ in range(4)]
    cells, all_evals = _cells(fs, cosets, log_n, log_l)
    cells[1, 3, 5] = [(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]      # the modulus itself
    cells[3, 0, 0] = [0xFFFFFFFFFFFFFFFF] * 4                                       # 2^256 - 1
    out = _recover(ctx, log_n, log_l, m, cosets, cells)
    assert list(out["status"]) == [OK, BAD_EVAL, OK, BAD_EVAL] and out["count"] == [2, 2, 0]
    assert (out["first_excess"] == NO_EXCESS).all()
    for p in (0, 2):
        assert (out["coeffs"][p] == fr_pack(fs[p])).all() and (out["evals"][p] == all_evals[p]).all()
    for p in (1, 3):
        assert not out["coeffs"][p].any() and not out["evals"][p].any()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    """every refusal the header lists but TYPLONK_ERR_OOM (no allocation a test can afford is refused); status, report, the host
    outputs and the device buffers are filled with a marker beforehand and found unchanged"""
    from typlonk_amd.capi import ERR_DOMAIN, ERR_INVALID_ARG, ERR_LENGTH, ERR_RANGE, RecoverReport, _u8p, _u64p

    lib = ctx.lib
    log_n, log_l, K, m, count = 5, 2, 4, 10, 2
    n, l, r = RR.shape(log_n, log_l)
    rng = np.random.default_rng(13)
    cells, _ = _cells([_rand(rng, m) for _ in range(count)], [5, 1, 2, 6], log_n, log_l)
    bufs = [ctx.alloc(16), ctx.alloc(16)]
    u32 = C.POINTER(C.c_uint32)

    def refused(handle=None, log_n=log_n, log_l=log_l, m=m, cosets=(5, 1, 2, 6), K=None, count=count, null=(), dev=None, offsets=None):
        ck = np.array(cosets, dtype=np.uint32)
        for b in bufs:
            b.upload(np.full((16, 4), MARK, dtype=np.uint64))
        status = np.full(8, 0x5A, dtype=np.uint8)
        first = np.full(8, MARK, dtype=np.uint64)
        co = np.full((8 * 64, 4), MARK, dtype=np.uint64)
        eo = np.full((8 * 64, 4), MARK, dtype=np.uint64)
        rep = RecoverReport()
        C.memset(C.byref(rep), 0xC3, C.sizeof(rep))
        dev = bufs if dev is None else dev
        handles = (C.c_void_p * max(len(dev), 1))(*[None if b is None else b.handle for b in dev])
        args = {"cosets": ck.ctypes.data_as(u32), "evals": _u64p(cells), "dev": handles, "coeffs": _u64p(co), "evals_out": _u64p(eo),
                "status": _u8p(status), "first": _u64p(first), "report": C.byref(rep),
                "offsets": None if offsets is None else (C.c_size_t * len(offsets))(*offsets)}
        for name in null:
            args[name] = None
        rc = lib.typlonk_recover_chunks(ctx.h if handle is None else handle[0], log_n, log_l, m, args["cosets"], len(ck) if K is None else K,
                                        args["evals"], count, args["dev"], args["offsets"], args["coeffs"], args["evals_out"], args["status"],
                                        args["first"], args["report"])
        assert (status == 0x5A).all() and (first == MARK).all() and bytes(rep) == b"\xC3" * C.sizeof(rep), "a refused call wrote to its outputs"
        assert (co == MARK).all() and (eo == MARK).all(), "a refused call wrote to its host outputs"
        for b in bufs:
            assert (b.download() == MARK).all(), "a refused call wrote to a device buffer"
        return rc

    # INVALID_ARG: the null pointers, no output at all, a null entry
    assert refused(handle=(None,)) == ERR_INVALID_ARG
    for name in ("cosets", "evals", "status", "report"):
        assert refused(null=(name,)) == ERR_INVALID_ARG, name
    assert refused(null=("dev", "coeffs", "evals_out")) == ERR_INVALID_ARG and b"no output" in lib.typlonk_last_error(ctx.h)
    assert refused(dev=[bufs[0], None]) == ERR_INVALID_ARG and b"null entry" in lib.typlonk_last_error(ctx.h)
    # DOMAIN
    for lg in (0, 25, 64, 0xFFFFFFFF):
        assert refused(log_n=lg, log_l=0) == ERR_DOMAIN
    for lg_l in (log_n, log_n + 1, 0xFFFFFFFF):
        assert refused(log_l=lg_l) == ERR_DOMAIN
    assert refused(log_n=17, log_l=0) == ERR_DOMAIN and refused(log_n=24, log_l=7) == ERR_DOMAIN
    assert b"quadratic" in lib.typlonk_last_error(ctx.h)
    # LENGTH
    assert refused(K=0) == ERR_LENGTH and refused(K=r + 1) == ERR_LENGTH and refused(count=0) == ERR_LENGTH and refused(m=0) == ERR_LENGTH
    assert refused(m=K * l + 1) == ERR_LENGTH and b"too few cells for this degree bound" in lib.typlonk_last_error(ctx.h)
    assert refused(count=(1 << 26 >> log_n) + 1, null=("dev",)) == ERR_LENGTH
    # RANGE
    assert refused(cosets=(5, 1, r, 6)) == ERR_RANGE
    assert refused(offsets=[0, 7]) == ERR_RANGE and refused(offsets=[17, 0]) == ERR_RANGE and refused(m=16, cosets=(5, 1, 2, 6), offsets=[1, 0]) == ERR_RANGE
    # INVALID_ARG: a coset twice, a range twice
    assert refused(cosets=(5, 1, 5, 6)) == ERR_INVALID_ARG and b"twice" in lib.typlonk_last_error(ctx.h)
    assert refused(m=4, dev=[bufs[0], bufs[0]], offsets=[2, 5]) == ERR_INVALID_ARG and b"same range" in lib.typlonk_last_error(ctx.h)
    assert refused(m=4, dev=[bufs[0], bufs[0]]) == ERR_INVALID_ARG
    # two at once: the earlier in the header's order
    assert refused(log_n=0, null=("status",)) == ERR_INVALID_ARG and refused(log_l=9, K=0) == ERR_DOMAIN
    assert refused(cosets=(5, r, 5, 6)) == ERR_RANGE and refused(K=0, cosets=(5, 5, 5, 5)) == ERR_LENGTH
    # a good call still succeeds, one buffer for both polynomials at ranges that touch
    out = ctx.recover_chunks(log_n, log_l, 8, [5, 1, 2, 6], cells, out_bufs=[bufs[0], bufs[0]], offsets=[0, 8])
    assert list(out["status"]) == [INCONSISTENT, INCONSISTENT] and list(out["first_excess"]) == [8, 8] and not bufs[0].download().any()
    out = ctx.recover_chunks(log_n, log_l, m, [5, 1, 2, 6], cells, out_bufs=bufs)
    assert (out["status"] == OK).all() and (bufs[1].download(0, m) == out["coeffs"][1]).all()


# ---- 7. the order of the cosets; twice ------------------------------------------------------------------------------------------
def test_the_order_of_the_cosets_and_twice(ctx):
    log_n, log_l, K, m = 8, 3, 20, 150
    n, l, r = RR.shape(log_n, log_l)
    rng = np.random.default_rng(14)
    cosets = [int(x) for x in rng.permutation(r)[:K]]
    fs = [_rand(rng, m), _rand(rng, m), _rand(rng, 160)]                 # the last one is inconsistent with m
    cells, _ = _cells(fs, cosets, log_n, log_l)
    first = _recover(ctx, log_n, log_l, m, cosets, cells)
    assert list(first["status"]) == [OK, OK, INCONSISTENT] and first["first_excess"][2] == 150
    again = _recover(ctx, log_n, log_l, m, cosets, cells)
    order = [int(x) for x in rng.permutation(K)]
    moved = _recover(ctx, log_n, log_l, m, [cosets[i] for i in order], np.ascontiguousarray(cells[:, order]))
    for other in (again, moved, _recover(ctx, log_n, log_l, m, sorted(cosets), np.ascontiguousarray(cells[:, np.argsort(cosets)]))):
        for key in ("status", "first_excess", "coeffs", "evals"):
            assert (other[key] == first[key]).all(), key


# ---- 8. under profiling ---------------------------------------------------------------------------------------------------------
def test_under_profiling(ctx):
    log_n, log_l, K, m = 9, 4, 17, 260
    rng = np.random.default_rng(15)
    cosets = [int(x) for x in rng.permutation(32)[:K]]
    fs = [_rand(rng, m), _rand(rng, 270)]
    cells, _ = _cells(fs, cosets, log_n, log_l)
    plain = _recover(ctx, log_n, log_l, m, cosets, cells)
    assert list(plain["status"]) == [OK, INCONSISTENT]
    names = ["recover_vanish", "recover_scatter", "recover_interp", "recover_divide", "recover_finish", "recover_evals"]
    s = _rand(rng, 1)[0]
    sid = ctx.srs_generate(_limbs(s), 64)
    ctx.set_profiling(1)
    try:
        for want_evals in (True, False):
            got = _recover(ctx, log_n, log_l, m, cosets, cells, want_evals=want_evals)
            prof = ctx.profile()
            assert [name for name, _ in prof] == (names if want_evals else names[:-1]), prof
            assert all(ms >= 0 for _, ms in prof)
            for key in ("status", "first_excess", "coeffs") + (("evals",) if want_evals else ()):
                assert (got[key] == plain[key]).all(), key
        ctx.msm(sid, fr_pack(_rand(rng, 64)))
        after = [name for name, _ in ctx.profile()]
        assert after and not any(name.startswith("recover_") for name in after), after
    finally:
        ctx.set_profiling(0)
        ctx.srs_free(sid)


# ---- 9. the C++ mirror ----------------------------------------------------------------------------------------------------------
def test_mirror_recover_chunks(built):
    """tests/cpp/test_recover_chunks_host: kzg::KzgScheme::recover_chunks of the C++ mirror at (8, 3), then open and verify"""
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "test_recover_chunks_host")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for t in ("recover ok", "open ok", "verify ok", "verdicts ok"):
        assert t in r.stdout
