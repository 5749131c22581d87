"""The kernels of typlonk_recover_chunks -- recover_chunks.hip compiled as the library compiles it, behind the test-only harness
tests/cpp/libdevice_recover_chunks.so -- each run alone through its launcher, against big integers word for word.

These tests FAIL on a commit before typlonk_recover_chunks: the harness and the plan program do not exist there.  That is
expected and they do not skip.

recover_vanish_kernel / recover_vanish_combine_kernel / recover_invert_kernel: Zd and Zc for r = 2 .. 1024 with 0, 1, tile - 1,
tile, tile + 1, 600 and r - 1 missing cosets (the tile size read from the plan program, not restated here) -- the first half, the
odd cosets (Z' = Y^(r/2) + 1), one coset only, random sets -- with 1, 2 and 3 slices and the plan's own, which must give the same
words; Zd zero exactly on the missing cosets; Zc ZcInv = 1 at every index.
recover_scatter_kernel: every one of the n count words, the zeros included, with guard bands on both sides of the output, for
(r, l) in {(2, 1), (2, 1024), (1024, 1), (8, 8), (64, 64)}, count 1 and 3, K = 1, K = r and between, the cosets in a shuffled order.
recover_scale_kernel: index i and i + r get the same factor, at r = 2 and r = n / 2.
recover_excess_kernel / recover_finish_kernel: a nonzero coefficient at exactly m, at m - 1 (not counted), at K l - 1, at K l (not
counted), at the first and last index of a workgroup's span, in two places at once (the lower is reported), the empty range
m = K l; the copy of the m low coefficients, zeros for a flagged polynomial, and the words between the destinations untouched."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import recover_chunks_ref as RR
from helpers import O, ROOT, fr_pack, fr_unpack

pytestmark = pytest.mark.gpu

R = O.R
U32P = ctypes.POINTER(ctypes.c_uint32)
U8P = ctypes.POINTER(ctypes.c_uint8)
U64P = ctypes.POINTER(ctypes.c_uint64)
NO_CELL = 0xFFFFFFFF
FILL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def lib(built):
    try:    # PyTorch's bundled HIP runtime must be loaded before the system one the harness links (typlonk_amd.capi.load_library says
        import torch  # noqa: F401  why), or the tests that use torch later in the same process find no device
    except ImportError:
        pass
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpp", "libdevice_recover_chunks.so"))
    lib.drc_vanish.restype = ctypes.c_int
    lib.drc_vanish.argtypes = [U32P, ctypes.c_uint32, U32P, ctypes.c_uint64, U32P, ctypes.c_uint32, U32P, U32P, U32P, U32P, U32P]
    lib.drc_scatter.restype = ctypes.c_int
    lib.drc_scatter.argtypes = [U32P, U32P, U32P, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, U32P, U32P]
    lib.drc_scale.restype = ctypes.c_int
    lib.drc_scale.argtypes = [U32P, U32P, ctypes.c_uint32, ctypes.c_uint64, U32P]
    lib.drc_finish.restype = ctypes.c_int
    lib.drc_finish.argtypes = [U32P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, U8P, U64P, U32P, U32P,
                               U32P, U32P]
    return lib


def _plan(log_n, log_l, m, K, count=1):
    """the plan program's line for an admitted call with the host coefficients as its output"""
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "recover_chunks_plan_host")], input=f"{log_n} {log_l} {m} {K} {count} 0 0 1 0 0 0\n",
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert p["code"] == 0, p
    return p


@pytest.fixture(scope="module")
def tile(built):
    return _plan(4, 1, 1, 1)["tile"]


def _words(vals) -> np.ndarray:
    """canonical ints -> (k, 8) uint32: the Montgomery limbs as the kernels' 32-bit words"""
    return np.ascontiguousarray(fr_pack(list(vals))).view(np.uint32).reshape(-1, 8)


def _ints(words) -> list:
    return fr_unpack(np.ascontiguousarray(words).view(np.uint64).reshape(-1, 4))


def _p(a, t=U32P):
    return a.ctypes.data_as(t)


def _rand(rng, k):
    return [int.from_bytes(rng.bytes(32), "little") % R for _ in range(k)]


# ---- the vanishing products ----------------------------------------------------------------------------------------------------
def _vanish(lib, log_r, missing, slices):
    r = 1 << log_r
    a = [pow(O.domain_root(log_r), k, R) for k in range(r)]
    gl = _rand(np.random.default_rng(log_r), 1)[0]                # any shift: the kernel is told g^l, it does not know g
    idx = np.array(list(missing) or [0], dtype=np.uint32)
    z = np.full((2 * r, 8), 0x11111111, dtype=np.uint32)
    zi = np.full((r, 8), 0x11111111, dtype=np.uint32)
    used, tl, guard = (np.zeros(1, dtype=np.uint32) for _ in range(3))
    rc = lib.drc_vanish(_p(_words(a)), log_r, _p(idx), len(missing), _p(_words([gl])), slices, _p(z), _p(zi), _p(used), _p(tl), _p(guard))
    assert rc == 0, rc
    assert guard[0] == 1
    return a, gl, z, zi, int(used[0])


def _vanish_ref(log_r, gl, missing):
    """(Zd, Zc) by another route than the kernel's: the coefficients of Z' from its roots, then Z' at the r points a_k and at the r
    points gl a_k as two transforms of size r"""
    r = 1 << log_r
    w = O.domain_root(log_r)
    z = [1]
    for j in missing:
        a = pow(w, j, R)
        z = [((z[i - 1] if i else 0) - a * (z[i] if i < len(z) else 0)) % R for i in range(len(z) + 1)]
    z += [0] * (r - len(z))
    return O.ntt(z, log_r), O.ntt(z, log_r, coset=gl)


def _missing_sets(log_r, tile):
    r = 1 << log_r
    rng = np.random.default_rng(77 + log_r)
    sets = {}
    for size in sorted({0, 1, tile - 1, tile, tile + 1, 600, r - 1}):
        if size < r:
            sets[f"random {size}"] = sorted(int(x) for x in rng.choice(r, size=size, replace=False))
    sets["the first half"] = list(range(r // 2))
    sets["the odd cosets"] = list(range(1, r, 2))
    sets["one coset only is known"] = [k for k in range(r) if k != r // 3]
    sets["descending order"] = list(range(r - 1, r // 2, -1))[: max(1, r // 4)] if r > 2 else [1]
    return sets


@pytest.mark.parametrize("log_r", [1, 2, 7, 9, 10])
def test_vanishing_products(lib, tile, log_r):
    r = 1 << log_r
    for name, missing in _missing_sets(log_r, tile).items():
        first = None
        ref = None
        for slices in (0, 1, 2, 3):
            a, gl, z, zi, used = _vanish(lib, log_r, missing, slices)
            assert 1 <= used <= max(1, len(missing)) and (slices == 0 or used <= slices), (name, slices, used)
            if first is None:
                first = (z.copy(), zi.copy())
                ref = _vanish_ref(log_r, gl, missing)
                got = _ints(z)
                assert got[:r] == ref[0], (log_r, name, "Zd")
                assert got[r:] == ref[1], (log_r, name, "Zc")
                assert [x == 0 for x in got[:r]] == [k in set(missing) for k in range(r)]   # zero exactly on the missing cosets
                inv = _ints(zi)
                assert all(x * y % R == 1 for x, y in zip(got[r:], inv)), (log_r, name, "Zc ZcInv = 1")
            else:
                assert np.array_equal(z, first[0]) and np.array_equal(zi, first[1]), (log_r, name, slices, "every slicing gives the same words")
        if name == "the odd cosets" and r >= 2:
            assert _ints(first[0])[:r] == [(pow(x, r // 2, R) + 1) % R for x in a]      # Z' = Y^(r/2) + 1


# ---- the scatter ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_r,log_l", [(1, 0), (1, 10), (10, 0), (3, 3), (6, 6)])
@pytest.mark.parametrize("count", [1, 3])
def test_scatter_writes_every_word(lib, log_r, log_l, count):
    r, l = 1 << log_r, 1 << log_l
    n = r * l
    rng = np.random.default_rng(1000 * log_r + 10 * log_l + count)
    zd_vals = _rand(rng, r)
    zd = _words(zd_vals)
    for K in sorted({1, max(r // 2, 1), max(r - 1, 1), r}):
        cosets = [int(x) for x in rng.permutation(r)[:K]]                          # a shuffled order
        pos = np.full(r, NO_CELL, dtype=np.uint32)
        for i, k in enumerate(cosets):
            pos[k] = i
        cells = rng.integers(0, 1 << 32, size=(count * K * l, 8), dtype=np.uint64).astype(np.uint32)
        cells[:, 7] &= 0x3FFFFFFF                                                   # below r, whatever the other words
        cell_vals = _ints(cells)
        v = np.full((count * n, 8), 0x11111111, dtype=np.uint32)
        guard = np.zeros(1, dtype=np.uint32)
        rc = lib.drc_scatter(_p(cells), _p(pos), _p(zd), K, log_r + log_l, log_l, count, _p(v), _p(guard))
        assert rc == 0, rc
        assert guard[0] == 1, "a word outside the output was written"
        want = [0] * (count * n)
        for p in range(count):
            for i, k in enumerate(cosets):
                for t in range(l):
                    want[p * n + k + r * t] = cell_vals[(p * K + i) * l + t] * zd_vals[k] % R
        assert np.array_equal(v, _words(want)), (log_r, log_l, count, K)


# ---- the scale -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,log_r", [(6, 1), (6, 5), (10, 9), (10, 3)])
def test_scale_has_period_r(lib, log_n, log_r):
    n, r = 1 << log_n, 1 << log_r
    rng = np.random.default_rng(log_n * 100 + log_r)
    count = 2
    zc = _rand(rng, r)
    vals = _rand(rng, count * n)
    vals[5], vals[5 + r] = 1, 1                                   # i and i + r: the same factor
    v = _words(vals)
    guard = np.zeros(1, dtype=np.uint32)
    rc = lib.drc_scale(_p(v), _p(_words(zc)), log_r, count * n, _p(guard))
    assert rc == 0 and guard[0] == 1
    got = _ints(v)
    assert got == [x * zc[i % r] % R for i, x in enumerate(vals)]
    assert got[5] == got[5 + r] == zc[5 % r]


# ---- the finish ----------------------------------------------------------------------------------------------------------------
def _finish(lib, log_n, log_l, K, m, vecs, fixed):
    """vecs: count lists of n ints -> (first_excess, status, out (count, m), dst with its gaps (count, m + 2), blocks)"""
    n, count = 1 << log_n, len(vecs)
    v = _words([x for vec in vecs for x in vec])
    verdict = np.zeros(2 * count, dtype=np.uint64)
    out = np.full((count * m, 8), 0x11111111, dtype=np.uint32)
    dst = np.full((count * (m + 2), 8), 0x11111111, dtype=np.uint32)
    blocks, guard = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    rc = lib.drc_finish(_p(v), log_n, log_l, K, m, count, _p(np.array(fixed, dtype=np.uint8), U8P), _p(verdict, U64P), _p(out), _p(dst),
                        _p(blocks), _p(guard))
    assert rc == 0, rc
    assert guard[0] == 1
    return [int(x) for x in verdict[:count]], [int(x) for x in verdict[count:]], out.reshape(count, m, 8), dst.reshape(count, m + 2, 8), int(blocks[0])


def _check_copies(vecs, m, status, out, dst):
    for p, vec in enumerate(vecs):
        want = _words(vec[:m]) if status[p] == RR.OK else np.zeros((m, 8), dtype=np.uint32)
        assert np.array_equal(out[p], want) and np.array_equal(dst[p, 1:m + 1], want), p
        assert (dst[p, 0] == FILL).all() and (dst[p, m + 1] == FILL).all(), "a neighbour's word was written"


def test_finish_where_a_nonzero_counts(lib):
    log_n, log_l, K = 6, 2, 10                       # n = 64, l = 4, K l = 40
    n, kl, m = 64, 40, 13
    rng = np.random.default_rng(5)
    base = _rand(rng, m) + [0] * (n - m)
    def with_at(*js):
        vec = list(base)
        for j in js:
            vec[j] = 1 + j
        return vec
    vecs = [with_at(), with_at(m), with_at(m - 1), with_at(kl - 1), with_at(kl), with_at(30, 20), with_at(n - 1), with_at(m, kl - 1)]
    first, status, out, dst, blocks = _finish(lib, log_n, log_l, K, m, vecs, [0] * 8)
    assert status == [RR.OK, RR.INCONSISTENT, RR.OK, RR.INCONSISTENT, RR.OK, RR.INCONSISTENT, RR.OK, RR.INCONSISTENT]
    assert first == [RR.NO_EXCESS, m, RR.NO_EXCESS, kl - 1, RR.NO_EXCESS, 20, RR.NO_EXCESS, m]
    _check_copies(vecs, m, status, out, dst)


def test_finish_the_empty_range_and_the_fixed_flag(lib):
    log_n, log_l, K = 5, 1, 8                        # n = 32, K l = 16 = m: nothing is scanned
    rng = np.random.default_rng(6)
    vecs = [_rand(rng, 32) for _ in range(3)]        # nonzero everywhere, above m too
    first, status, out, dst, _ = _finish(lib, log_n, log_l, K, 16, vecs, [0, RR.BAD_EVAL, 0])
    assert status == [RR.OK, RR.BAD_EVAL, RR.OK] and first == [RR.NO_EXCESS] * 3
    _check_copies(vecs, 16, status, out, dst)        # the middle one: zeros; its neighbours whole
    # a fixed flag stands even where a coefficient is found, and names no index
    vecs = [[1] * 32 for _ in range(2)]
    first, status, out, dst, _ = _finish(lib, log_n, log_l, K, 3, vecs, [RR.BAD_EVAL, 0])
    assert status == [RR.BAD_EVAL, RR.INCONSISTENT] and first == [RR.NO_EXCESS, 3]
    _check_copies(vecs, 3, status, out, dst)


def test_finish_across_workgroups(lib):
    """more than one workgroup a polynomial: the first and last index of a workgroup's span, and two spans at once"""
    log_n, log_l, K, m = 15, 3, 1 << 12, 300          # n = 2^15, K l = 2^15: the range is [300, 32768)
    pl = _plan(log_n, log_l, m, K)
    blocks, span = pl["excess_blocks"], pl["excess_span"]
    assert blocks >= 3 and pl["excess_len"] == (1 << 15) - m
    n = 1 << log_n
    spots = [m + span - 1, m + span, m + 2 * span - 1, m + (blocks - 1) * span, n - 1, m + 255, m + 256]
    cases = [[j] for j in spots] + [[m + 2 * span + 5, m + span + 9], [n - 1, m + span]]
    rng = np.random.default_rng(8)
    low = _rand(rng, m)
    for at in range(0, len(cases), 4):
        vecs = []
        for js in cases[at:at + 4]:
            vec = low + [0] * (n - m)
            for j in js:
                vec[j] = 7
            vecs.append(vec)
        first, status, out, dst, got_blocks = _finish(lib, log_n, log_l, K, m, vecs, [0] * len(vecs))
        assert got_blocks == blocks
        assert status == [RR.INCONSISTENT] * len(vecs) and first == [min(js) for js in cases[at:at + 4]]
        _check_copies(vecs, m, status, out, dst)
