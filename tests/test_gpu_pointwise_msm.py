"""The two kernels the FK20 openings run on their hot path -- g1_fft.hip compiled as the library compiles it, behind the test-only
harness tests/cpp/libdevice_chunks.so -- with their launchers called directly.

g1_pointwise_msm_kernel: dst[o] = sum_{j<l} [k_(o,j)] y_(o,j).  Through the library a small shape only ever reaches the largest
number of slices g the plan allows, so every g is named here: l in {1, 2, 8, 64}, outputs in {1, 63, 64, 65, 130} (spare lanes,
exactly one wavefront, more than one), every power of two g <= l.  The records come from a pool of known multiples e G, the
expected record is [sum_j k_j e_j] G computed on scalars, and every comparison is word for word on canonical affine records; all
g give identical words, and the guard band behind the outputs stays intact.

srs_g1_ntt_batch_stage_kernel: 1, 3 and 4 blocks of 2^l records, l in {1, 2, 6, 7}, at distinct source and destination strides, in
both directions, each block against typlonk_srs_g1_ntt's result for that block alone."""
import ctypes
import os

import numpy as np
import pytest

import arith_cases as AC
from helpers import O, ROOT, g1_pack, g1_unpack_one

pytestmark = pytest.mark.gpu

R = O.R
U32P = ctypes.POINTER(ctypes.c_uint32)
FILL = 0xA5A5A5A5      # the harness's fill byte, as a word: what a launcher did not write
PT_WORDS = 32
LS = [1, 2, 8, 64]
OUTPUTS = [1, 63, 64, 65, 130]


@pytest.fixture(scope="module")
def lib(built):
    try:    # PyTorch's bundled HIP runtime must be loaded before the system one the harness links (typlonk_amd.capi.load_library says
        import torch  # noqa: F401  why), or the tests that use torch later in the same process find no device
    except ImportError:
        pass
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "cpp", "libdevice_chunks.so"))
    lib.dc_pointwise_msm.restype = ctypes.c_int
    lib.dc_pointwise_msm.argtypes = [U32P, U32P, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, U32P, U32P]
    lib.dc_ntt_stages.restype = ctypes.c_int
    lib.dc_ntt_stages.argtypes = [U32P, U32P, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, U32P, U32P]
    return lib


def _p(a):
    return a.ctypes.data_as(U32P)


def record(pt) -> list[int]:
    """a point (affine integers or None) as the PT_WORDS words of an SRS record: x, y canonical in Montgomery form, 12 words each"""
    if pt is None:
        return [0] * PT_WORDS
    return AC.limbs(AC.mont(pt[0]), 12, 32) + AC.limbs(AC.mont(pt[1]), 12, 32) + [0] * 8


class Pool:
    """e[i] and the record of e[i] G: entry 0 the identity, then 1 G, then random multiples, each followed by its negative"""

    def __init__(self):
        rng = np.random.default_rng(0x9001)
        es = [0, 1]
        for _ in range(11):
            e = int.from_bytes(rng.bytes(32), "little") % R
            es += [e, R - e]
        self.e = es
        self.points = [O.g1_mul(O.G1, e) for e in es]
        self.words = np.array([record(p) for p in self.points], dtype=np.uint32)
        self._cache = {}

    def expected(self, scalar: int) -> list[int]:
        scalar %= R
        if scalar not in self._cache:
            self._cache[scalar] = record(O.g1_mul(O.G1, scalar))[:24]
        return self._cache[scalar]


@pytest.fixture(scope="module")
def pool():
    return Pool()


def _scalar_words(ks) -> np.ndarray:
    return np.array([AC.limbs(k, 8, 32) for k in ks], dtype=np.uint32)


def _inputs(kind: str, pool: Pool, outputs: int, l: int, seed: int):
    """(k[j][o], idx[j][o]): the scalar and the pool entry of term j of output o.  count = 1: period = outputs."""
    rng = np.random.default_rng(seed)
    rand = lambda: int.from_bytes(rng.bytes(32), "little") % R   # noqa: E731
    npool = len(pool.e)
    k = [[rand() for _ in range(outputs)] for _ in range(l)]
    idx = [[int(rng.integers(1, npool)) for _ in range(outputs)] for _ in range(l)]
    if kind == "zero_scalars":
        k = [[0] * outputs for _ in range(l)]
    elif kind == "one_term":                         # one non-zero term per output, at a term that moves with the output
        k = [[k[j][o] if j == o % l else 0 for o in range(outputs)] for j in range(l)]
    elif kind == "r_minus_1":
        k = [[R - 1] * outputs for _ in range(l)]
    elif kind == "identity_records":                 # every other term's record the identity, and whole outputs of identities
        idx = [[0 if (j + o) % 2 == 0 or o % 7 == 3 else idx[j][o] for o in range(outputs)] for j in range(l)]
    elif kind == "equal_records":                    # every addition of an output meets its own base: the doubling branch
        idx = [list(idx[0]) for _ in range(l)]      # under one scalar, 1 at the odd outputs: P + P at the top bit of every chain
        k = [[1 if o & 1 else k[0][o] for o in range(outputs)] for _ in range(l)]
    elif kind == "cancelling_pairs":                 # terms 2i and 2i + 1: P and -P under one scalar (l = 1: a zero scalar)
        for j in range(0, l - 1, 2):
            for o in range(outputs):
                i = 2 + 2 * int(rng.integers(0, (npool - 2) // 2))
                idx[j][o], idx[j + 1][o] = i, i + 1
                k[j + 1][o] = k[j][o]
        if l == 1:
            k = [[0] * outputs]
    else:
        assert kind == "random"
    return k, idx


def _run(lib, pool, k, idx, outputs, l, g):
    kw = np.ascontiguousarray(np.concatenate([_scalar_words(row) for row in k]))                     # [j][o]: (0 l + j) period + o
    tab = np.ascontiguousarray(np.concatenate([pool.words[np.array(row)] for row in idx]))           # [j][o]: j period + o
    out = np.full((outputs, PT_WORDS), 0x11111111, dtype=np.uint32)
    guard = np.zeros(1, dtype=np.uint32)
    rc = lib.dc_pointwise_msm(_p(kw), _p(tab), outputs, outputs, l, g, _p(out), _p(guard))
    assert rc == 0, rc
    assert guard[0] == 1, "the launcher wrote behind its outputs"
    assert (out[:, 24:] == FILL).all(), "a record's padding was written"
    return out[:, :24]


KINDS = ["random", "zero_scalars", "one_term", "r_minus_1", "identity_records", "equal_records", "cancelling_pairs"]


@pytest.mark.parametrize("l", LS)
@pytest.mark.parametrize("kind", KINDS)
def test_pointwise_msm(lib, pool, kind, l):
    """random scalars at every output count; the special inputs at 65 outputs, two wavefronts with 63 spare lanes at g = 1"""
    for outputs in (OUTPUTS if kind == "random" else [65]):
        k, idx = _inputs(kind, pool, outputs, l, 0x9A5 + 131 * l + outputs)
        want = np.array([pool.expected(sum(k[j][o] * pool.e[idx[j][o]] for j in range(l))) for o in range(outputs)], dtype=np.uint32)
        if kind in ("zero_scalars", "cancelling_pairs"):
            assert not want.any()                                                  # every sum the identity: the all-zero record
        first = None
        g = 1
        while g <= min(l, 64):
            got = _run(lib, pool, k, idx, outputs, l, g)
            bad = [o for o in range(outputs) if not (got[o] == want[o]).all()]
            assert not bad, (kind, l, outputs, g, bad[:8])
            assert first is None or (got == first).all()                           # all g give identical words
            first = got
            g *= 2


def test_two_polynomials_over_one_table(lib, pool):
    """outputs = 2 x period: the second polynomial's scalars lie l x period further on and it reads the same table"""
    l, period = 8, 33
    rng = np.random.default_rng(0x2B01)
    ks = [[[int.from_bytes(rng.bytes(32), "little") % R for _ in range(period)] for _ in range(l)] for _ in range(2)]
    idx = [[int(rng.integers(0, len(pool.e))) for _ in range(period)] for _ in range(l)]
    kw = np.ascontiguousarray(np.concatenate([_scalar_words(row) for p in range(2) for row in ks[p]]))
    tab = np.ascontiguousarray(np.concatenate([pool.words[np.array(row)] for row in idx]))
    want = np.array([pool.expected(sum(ks[p][j][i] * pool.e[idx[j][i]] for j in range(l))) for p in range(2) for i in range(period)],
                    dtype=np.uint32)
    for g in (1, 4, 8):
        out = np.full((2 * period, PT_WORDS), 0x11111111, dtype=np.uint32)
        guard = np.zeros(1, dtype=np.uint32)
        assert lib.dc_pointwise_msm(_p(kw), _p(tab), 2 * period, period, l, g, _p(out), _p(guard)) == 0
        assert guard[0] == 1 and (out[:, :24] == want).all(), g


def test_harness_refuses_shapes_outside_the_contract(lib, pool):
    kw = np.zeros((8, 8), dtype=np.uint32)
    tab = np.zeros((8, PT_WORDS), dtype=np.uint32)
    out = np.zeros((4, PT_WORDS), dtype=np.uint32)
    guard = np.zeros(1, dtype=np.uint32)
    for outputs, period, l, g in ((4, 4, 2, 4), (4, 4, 3, 1), (4, 4, 2, 0), (4, 3, 2, 1), (0, 1, 2, 1), (4, 0, 2, 1)):
        assert lib.dc_pointwise_msm(_p(kw), _p(tab), outputs, period, l, g, _p(out), _p(guard)) == 1      # hipErrorInvalidValue
    assert not out.any()


# ---- the batched stage kernel -----------------------------------------------------------------------------------------------
def _point_of_words(words):
    x, y = AC.val(words[:12], 32), AC.val(words[12:24], 32)
    assert x < AC.P and y < AC.P, "a record is not canonical"
    return None if x == 0 and y == 0 else (AC.unmont(x), AC.unmont(y))


@pytest.mark.parametrize("l", [1, 2, 6, 7])
@pytest.mark.parametrize("blocks", [1, 3, 4])
def test_batched_stages(ctx, lib, pool, l, blocks):
    """block b of the launch equals typlonk_srs_g1_ntt over that block alone: forward as TYPLONK_SRS_FROM_LAGRANGE gives it, the
    inverse direction, which the stages leave unscaled, as the same records in the order 0, N - 1, ..., 1.
    typlonk_srs_g1_ntt shares the stage loop and the butterfly with this launcher but runs its single block through
    srs_g1_ntt_stage_kernel, so the two sides differ in the indexing kernel only; the independent check of the butterfly is
    tests/test_gpu_srs_lagrange.py, against closed forms."""
    n = 1 << l
    src_stride, dst_stride = n + 3, n + 1
    rng = np.random.default_rng(0x57A + 16 * l + blocks)
    idx = rng.integers(0, len(pool.e), size=(blocks, n))
    src = np.full(((blocks - 1) * src_stride + n, PT_WORDS), 0x22222222, dtype=np.uint32)      # (between the blocks: never read)
    for b in range(blocks):
        src[b * src_stride:b * src_stride + n] = pool.words[idx[b]]
    fwd = []
    for b in range(blocks):
        sid = ctx.srs_load(*g1_pack([pool.points[i] for i in idx[b]]))
        tid = ctx.srs_from_lagrange(sid, l)
        xy, inf = ctx.srs_download(tid)
        fwd.append([g1_unpack_one(xy[i], int(inf[i])) for i in range(n)])
        ctx.srs_free(sid)
        ctx.srs_free(tid)
    for inverse in (False, True):
        roots = []
        for stage in range(1, l + 1):
            w = O.domain_root(stage)
            limbs = O.fr_to_mont_limbs(pow(w, -1, R) if inverse else w)                     # 4 x 64 bits
            roots.append([(int(v) >> s) & 0xFFFFFFFF for v in limbs for s in (0, 32)])
        roots = np.array(roots, dtype=np.uint32)
        out = np.full(((blocks - 1) * dst_stride + n, PT_WORDS), 0x11111111, dtype=np.uint32)
        guard = np.zeros(1, dtype=np.uint32)
        assert lib.dc_ntt_stages(_p(src), _p(roots), l, blocks, src_stride, dst_stride, _p(out), _p(guard)) == 0
        assert guard[0] == 1, "the launcher wrote behind its last block"
        for b in range(blocks):
            got = [_point_of_words(out[b * dst_stride + i]) for i in range(n)]
            want = [fwd[b][(n - i) % n] for i in range(n)] if inverse else fwd[b]
            assert got == want, (l, blocks, inverse, b)
            assert (out[b * dst_stride:b * dst_stride + n, 24:] == FILL).all()
            if b + 1 < blocks:                                                              # between the blocks: untouched
                assert (out[b * dst_stride + n:(b + 1) * dst_stride] == FILL).all()
