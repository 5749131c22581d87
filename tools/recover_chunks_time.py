"""Cost of typlonk_recover_chunks -- `count` polynomials from K of the r cosets of their domain -- in one session.  Median host wall
time of REPS blocking calls after one untimed call, the cells in host memory as the call takes them and the coefficients left in
device buffers (the form a following typlonk_open_chunks_dev reads); the same with the n evaluations copied back as well, through
Context.recover_chunks (which allocates the output per call) and through the C ABI into an array that is reused.  Per
shape: the call's own stage times from one more call with profiling on, where the stream is drained between the stages; and two
yardsticks taken here, never from the code under test:
  * four typlonk_ntt_fr_batch_devptr calls of the same size and count (inverse, coset forward, coset inverse, forward), drained
    once at the end -- what the transforms alone cost; "outside_transforms" is the share of the call not spent there (uploads,
    the new kernels, the verdict's round trip), the figure of merit for the new kernels;
  * the CPU route the call replaces, for ONE polynomial: the same three transforms of the interpolation on the C oracle, one
    thread (its pointwise steps and the vanishing products left out: a lower bound), and all of tests/recover_chunks_ref.py in
    Python where n <= 2^13.

    SHAPES=13:6:64:1,13:6:64:64,13:6:64:128,20:6:8192:1,16:0:32768:1 REPS=10 python tools/recover_chunks_time.py
(a shape: log_n:log_l:K:count; the known cosets are a random K of the r, m = K l)
"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, typlonk_amd
from bench import fr_mont_limbs
from oracle import bls12_381 as O
from oracle import coracle

REPS = int(os.environ.get("REPS", "10"))
COSET_G = fr_mont_limbs(7)


def median_ms(fn, reps):
    fn()   # first-launch costs out of the way
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3)


ctx = typlonk_amd.Context(0)
shapes = [tuple(int(v) for v in s.split(":")) for s in
          os.environ.get("SHAPES", "13:6:64:1,13:6:64:64,13:6:64:128,20:6:8192:1,16:0:32768:1").split(",")]

for log_n, log_l, K, count in shapes:
    n, l = 1 << log_n, 1 << log_l
    r = n // l
    m = K * l
    out = {"log_n": log_n, "l": l, "r": r, "K": K, "m": m, "count": count, "reps": REPS}
    rng = np.random.default_rng(17)
    cosets = np.sort(rng.permutation(r)[:K]).astype(np.uint32)
    # the polynomials on the device, their evaluations from the library's own forward transform, the cells picked on the host
    bufs = []
    cells = np.empty((count, K, l, 4), dtype=np.uint64)
    coeffs = rng.integers(0, 1 << 62, size=(count, m, 4), dtype=np.uint64)   # < 2^254 < r: canonical Montgomery residues of something
    for p in range(count):
        b = ctx.alloc(n)
        b.zero()
        b.upload(coeffs[p])
        ctx.ntt_dev(b, log_n)
        ev = b.download().reshape(l, r, 4)                                 # ev[t, k] = f(w^(k + r t))
        cells[p] = ev[:, cosets].transpose(1, 0, 2)
        bufs.append(b)

    def call(want_evals=False):
        return ctx.recover_chunks(log_n, log_l, m, cosets, cells, out_bufs=bufs, want_coeffs=False, want_evals=want_evals)

    res = call(True)
    assert (res["status"] == 0).all()
    assert all((bufs[p].download(0, m) == coeffs[p]).all() for p in range(min(count, 2)))
    out["recover_chunks_ms"] = median_ms(call, REPS)
    out["with_evals_ms"] = median_ms(lambda: call(True), REPS)
    # the same through the C ABI into ONE output array, written once before: Context.recover_chunks allocates its outputs per call,
    # and a copy into pages that were never touched pays for them
    import ctypes as C
    from typlonk_amd.capi import RecoverReport, _u8p, _u64p
    eo, st, fe, rep = np.ones((count, n, 4), dtype=np.uint64), np.zeros(count, dtype=np.uint8), np.zeros(count, dtype=np.uint64), RecoverReport()
    handles = (C.c_void_p * count)(*[b.handle for b in bufs])
    flat = np.ascontiguousarray(cells).reshape(-1)

    def call_reused():
        rc = ctx.lib.typlonk_recover_chunks(ctx.h, log_n, log_l, m, cosets.ctypes.data_as(C.POINTER(C.c_uint32)), K, _u64p(flat), count, handles,
                                            None, None, _u64p(eo), _u8p(st), _u64p(fe), C.byref(rep))
        assert rc == 0

    out["with_evals_reused_output_ms"] = median_ms(call_reused, REPS)
    assert (eo.reshape(count, r, l, 4) == res["evals"]).all()
    ctx.set_profiling(1)
    try:
        call(True)
        out["split"] = {k: round(v, 3) for k, v in ctx.profile() if k.startswith("recover_")}
    finally:
        ctx.set_profiling(0)
    ptrs = [b.devptr for b in bufs]

    def transforms():
        ctx.ntt_batch_devptr(ptrs, log_n, inverse=True)
        ctx.ntt_batch_devptr(ptrs, log_n, coset=COSET_G)
        ctx.ntt_batch_devptr(ptrs, log_n, inverse=True, coset=COSET_G)
        ctx.ntt_batch_devptr(ptrs, log_n)
        ctx.sync()

    out["four_transforms_ms"] = median_ms(transforms, REPS)
    out["outside_transforms"] = round(1 - out["four_transforms_ms"] / out["with_evals_reused_output_ms"], 3)
    for b in bufs:
        b.free()
    one = np.zeros((n, 4), dtype=np.uint64)
    one[:m] = coeffs[0]

    def cpu_transforms():
        v = coracle.ntt(one, log_n, inverse=True)
        v = coracle.ntt(v, log_n, coset=COSET_G)
        coracle.ntt(v, log_n, inverse=True, coset=COSET_G)

    out["cpu_three_transforms_one_poly_ms"] = median_ms(cpu_transforms, 3)
    if log_n <= 13:
        import recover_chunks_ref as RR
        from helpers import fr_unpack
        ys = fr_unpack(cells[0].reshape(-1, 4))
        cl = [ys[i * l:(i + 1) * l] for i in range(K)]
        t0 = time.perf_counter()
        got = RR.recover_chunks(cl, [int(k) for k in cosets], m, log_n, log_l)
        out["python_ref_one_poly_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        assert got[0] == 0 and got[2] == fr_unpack(coeffs[0])
    print(json.dumps(out), flush=True)
