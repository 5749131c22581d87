"""typlonk_srs_g1_ntt, typlonk_open_all_* and typlonk_open_chunks_* on the GPU past 128-point domains, where the other test
files of these calls stop (their references are quadratic): at the smallest domains that take the inner Fr transforms through
their two-pass (2^11 elements) and three-pass (2^17) plans, the batched transform through more than one launch group, the
pointwise pass through three launch shapes, and the G1 stage kernels through strides far past a wavefront.  The references are
the O(n log n) closed forms of tests/g1_wide_ref.py for a known full-width secret; a whole vector of records is compared by one
MSM of the C oracle plus a 64-record sample word for word (`combination_check`), every evaluation with the C oracle's NTT word
for word.  Device words meet device words in three places only -- host form against device-buffer form, a batch against its
single calls, the two Fr butterfly kernels -- and each time one side has passed the oracle comparison first."""
import json
import os
import subprocess

import numpy as np
import pytest

import g1_wide_ref as W
import open_all_ref as FA
from helpers import O, ROOT
from oracle import coracle as CO

pytestmark = pytest.mark.gpu

R = O.R


def _rand(rng, k):
    return [int.from_bytes(rng.bytes(32), "little") % R for _ in range(k)]


def _same(got, want):
    return (got[0] == want[0]).all() and (got[1] == want[1]).all()


def _plan_g(count, r, l):
    """open_chunks_plan's number of slices for this launch, from the host program that compiles the header on its own"""
    exe = os.path.join(ROOT, "tests", "cpp", "open_chunks_plan_host")
    out = subprocess.run([exe], input=f"{count} {r} {l}\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    return json.loads(out.stdout.splitlines()[0])["g"]


# ---- 1. the Lagrange form -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [10, 14])
def test_lagrange_form(ctx, log_n):
    """[L_i(s)] G for all 2^log_n records of a device-generated SRS; back again gives the source's first 2^log_n records word for
    word, which are [s^m] G by the same check; the source entry is unchanged.  2^10: stages at strides up to 8 wavefronts of
    records; 2^14: 128 blocks of butterflies a stage, fr_pow_u64 exponents to 2^13."""
    n = 1 << log_n
    s = _rand(np.random.default_rng(0x1A60 + log_n), 1)[0]
    sid = ctx.srs_generate(W.pack([s])[0], n + 3)
    lag = back = None
    try:
        before = ctx.srs_download(sid)
        lag = ctx.srs_lagrange(sid, log_n)
        assert ctx.srs_len(lag) == n
        W.combination_check(*ctx.srs_download(lag), W.lagrange_scalars(s, log_n), 0x1A6 + log_n)
        back = ctx.srs_from_lagrange(lag, log_n)
        assert ctx.srs_len(back) == n
        got = ctx.srs_download(back)
        W.combination_check(*got, W.powers(s, n), 0x2A6 + log_n)
        assert _same(got, ctx.srs_download(sid, 0, n))
        assert ctx.srs_len(sid) == n + 3 and _same(ctx.srs_download(sid), before)   # the source entry is untouched
    finally:
        for t in (sid, lag, back):
            if t is not None:
                ctx.srs_free(t)


# ---- 2. open_all --------------------------------------------------------------------------------------------------------------
def _open_all_checked(c, tab, f, s, log_n, seed):
    """open_all over host coefficients: the proofs against q_k(s), the evaluations against the C oracle's transform"""
    xy, inf, ev = c.open_all(tab, W.pack(f))
    assert xy.shape == (1 << log_n, 12) and inf.shape == (1 << log_n,) and ev.shape == (1 << log_n, 4)
    W.combination_check(xy, inf, W.open_all_scalars(f, s, log_n), seed)
    assert (ev == W.domain_evaluations(f, log_n)).all()
    return xy, inf, ev


def _open_all_dev_form(c, tab, f, host):
    """the device-buffer form at offset 3 gives the words of the host form (which has passed the oracle's check)"""
    buf = c.alloc(len(f) + 3)
    try:
        buf.upload(W.pack([5, 6, 7] + list(f)))
        dev = c.open_all(tab, buf, len(f), offset=3)
    finally:
        buf.free()
    assert all((a == b).all() for a, b in zip(host, dev))


@pytest.mark.parametrize("log_n", [10, 13, 16])
def test_open_all(ctx, log_n):
    """log_n = 10: the inner transform of 2n = 2^11 elements is the smallest two-pass one, at m = n and m = n - 5; 13: the
    evaluation transform of n is two-pass as well; 16: 2n = 2^17 is the smallest three-pass one."""
    n = 1 << log_n
    rng = np.random.default_rng(0xF200 + log_n)
    s = _rand(rng, 1)[0]
    sid = ctx.srs_generate(W.pack([s])[0], n + 3)
    tab = None
    try:
        tab = ctx.srs_open_all_table(sid, log_n)
        assert ctx.srs_len(tab) == 2 * n
        for m in (n, n - 5) if log_n == 10 else (n,):
            f = _rand(rng, m)
            host = _open_all_checked(ctx, tab, f, s, log_n, 0xF20 + m)
            if log_n <= 13:
                _open_all_dev_form(ctx, tab, f, host)
    finally:
        ctx.srs_free(sid)
        if tab is not None:
            ctx.srs_free(tab)


def test_open_all_under_both_butterfly_kernels(built, monkeypatch):
    """log_n = 10 with TYPLONK_NTT_FR30 = 0 (the 8 x 32-bit pass kernels everywhere) and = 2 (the 30-bit ones everywhere), a
    context each: the first run against the oracle, the second run the same words"""
    import typlonk_amd

    log_n, n = 10, 1 << 10
    rng = np.random.default_rng(0xF230)
    s = _rand(rng, 1)[0]
    f = _rand(rng, n)
    runs = []
    for mode in (0, 2):
        monkeypatch.setenv("TYPLONK_NTT_FR30", str(mode))
        c2 = typlonk_amd.Context(0)
        sid = tab = None
        try:
            sid = c2.srs_generate(W.pack([s])[0], n + 3)
            tab = c2.srs_open_all_table(sid, log_n)
            runs.append(_open_all_checked(c2, tab, f, s, log_n, 0xF23) if not runs else c2.open_all(tab, W.pack(f)))
        finally:
            for t in (sid, tab):
                if t is not None:
                    c2.srs_free(t)
            c2.close()
    assert all((a == b).all() for a, b in zip(*runs))


# ---- 3. open_chunks -----------------------------------------------------------------------------------------------------------
def _open_chunks_case(ctx, log_n, log_l, fs, g, seed, singles=False, dev_form=False):
    """every polynomial of the batch: its r proofs against q_k(s), its n evaluations in chunk-major order against the C oracle's
    transform; the launch shape of the pointwise pass is the g the docstring of the caller names"""
    n, l = 1 << log_n, 1 << log_l
    r = n // l
    count, m = len(fs), len(fs[0])
    assert _plan_g(count, r, l) == g
    s = _rand(np.random.default_rng(seed), 1)[0]
    sid = ctx.srs_generate(W.pack([s])[0], n + 3)
    tab = None
    bufs = []
    try:
        tab = ctx.srs_open_chunks_table(sid, log_n, log_l)
        assert ctx.srs_len(tab) == 2 * n
        xy, inf, ev = ctx.open_chunks(tab, [W.pack(f) for f in fs])
        assert xy.shape == (count, r, 12) and inf.shape == (count, r) and ev.shape == (count, r, l, 4)
        for p, f in enumerate(fs):
            W.combination_check(xy[p], inf[p], W.open_chunks_scalars(f, s, log_n, log_l), seed + p)
            assert (ev[p].reshape(n, 4) == W.chunk_major(W.domain_evaluations(f, log_n), log_n, log_l)).all(), p
        if singles:                                          # (the batch has passed the oracle's check)
            for p, f in enumerate(fs):
                one = ctx.open_chunks(tab, [W.pack(f)])
                assert (xy[p] == one[0][0]).all() and (inf[p] == one[1][0]).all() and (ev[p] == one[2][0]).all(), p
        if dev_form:                                         # device buffers at offset 3: the words of the host form
            for f in fs:
                bufs.append(ctx.alloc(m + 3))
                bufs[-1].upload(W.pack([5, 6, 7] + list(f)))
            dev = ctx.open_chunks(tab, bufs, m, offsets=[3] * count)
            assert (xy == dev[0]).all() and (inf == dev[1]).all() and (ev == dev[2]).all()
    finally:
        for b in bufs:
            b.free()
        ctx.srs_free(sid)
        if tab is not None:
            ctx.srs_free(tab)


def test_open_chunks_batch_of_three(ctx):
    """(log_n, log_l) = (12, 2), count = 3, g = 4: the inner transforms are 12 vectors of 2r = 2^11 elements -- two-pass, more
    than one launch group; the evaluation transforms of 2^12 are two-pass.  The third polynomial has n/2 + 3 coefficients,
    zero-padded by the caller to the common m = n.  Each polynomial equals its own count = 1 call word for word (2048 outputs
    of 4 terms: g = 4 as well, in 4 inner vectors, one launch group), and the device-buffer form the host form."""
    log_n, log_l = 12, 2
    n = 1 << log_n
    rng = np.random.default_rng(0xC122)
    fs = [_rand(rng, n), _rand(rng, n), _rand(rng, n // 2 + 3) + [0] * (n // 2 - 3)]
    assert all(len(f) == n for f in fs)
    assert _plan_g(1, n >> log_l, 1 << log_l) == 4
    _open_chunks_case(ctx, log_n, log_l, fs, g=4, seed=0xC1220, singles=True, dev_form=True)


def test_open_chunks_most_slices(ctx):
    """(13, 6), count = 2, g = 64: l = 64, the most slices an output can have; the inner transforms are 128 vectors of 2^8"""
    log_n, log_l = 13, 6
    rng = np.random.default_rng(0xC136)
    fs = [_rand(rng, 1 << log_n), _rand(rng, (1 << log_n) - 7)]
    fs[1] += [0] * 7
    _open_chunks_case(ctx, log_n, log_l, fs, g=64, seed=0xC1360, dev_form=True)


def test_open_chunks_three_pass_evaluations(ctx):
    """(17, 3), count = 1, g = 2: the evaluation transform of 2^17 is three-pass; r = 2^14 proofs, 8 inner vectors of 2^15"""
    log_n, log_l = 17, 3
    fs = [_rand(np.random.default_rng(0xC173), 1 << log_n)]
    _open_chunks_case(ctx, log_n, log_l, fs, g=2, seed=0xC1730)


# ---- 4. arbitrary points ------------------------------------------------------------------------------------------------------
def test_open_all_of_arbitrary_points(ctx):
    """log_n = 10 over [k_m] G from the C oracle for seeded k_m, with identity records at 0, 5 and n - 2 and records 64 .. 127
    all equal, against open_all_ref's double sum on scalars (2^19 big-integer products)"""
    log_n, n = 10, 1 << 10
    rng = np.random.default_rng(0xA4E)
    ks = _rand(rng, n + 3)
    for i in (0, 5, n - 2):
        ks[i] = 0
    ks[64:128] = [ks[64]] * 64
    f = _rand(rng, n)
    xy = np.zeros((n + 3, 12), dtype=np.uint64)
    inf = np.zeros(n + 3, dtype=np.uint8)
    for i, k in enumerate(W.pack(ks)):
        xy[i], inf[i] = CO.g1_mul_generator(k)
    assert inf.nonzero()[0].tolist() == [0, 5, n - 2] and (xy[64:128] == xy[64]).all()
    sid = ctx.srs_load(xy, inf)
    tab = None
    try:
        tab = ctx.srs_open_all_table(sid, log_n)
        pxy, pinf, ev = ctx.open_all(tab, W.pack(f))
        W.combination_check(pxy, pinf, FA.openings_of_point_scalars(f, ks, log_n), 0xA4E0)
        assert (ev == W.domain_evaluations(f, log_n)).all()
    finally:
        ctx.srs_free(sid)
        if tab is not None:
            ctx.srs_free(tab)
