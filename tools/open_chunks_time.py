"""Cost of typlonk_srs_open_chunks_table and typlonk_open_chunks_dev -- a polynomial's multi-proofs on every coset of its domain
in one call -- beside typlonk_srs_open_all_table / typlonk_open_all_dev at the same n, the existing code and the yardstick, in one
session.  Median host wall time of REPS blocking calls (REPS_BIG at 2^20 and above; 3 table builds) after one untimed call.

Then the pointwise pass alone, through the test harness tests/cpp/libdevice_chunks.so (event times of the launch, median of
REPS_KERNEL after one untimed launch): g1_pointwise_msm_kernel at g = 1, at the plan's g (tests/cpp/open_chunks_plan_host) and at
the largest g, and the same kernel at l = 1, g = 1 -- one ladder per record, one launch per polynomial, as the one-point opening
runs it -- over the same count x 2n (scalar, record) pairs one by one, which is what the plain route pays before it has summed
anything (pointwise_mul_same_pairs_ms; up to profiles/r31 that figure was g1_pointwise_mul_kernel's, which is gone).  The records are multiples of G drawn from a small pool and the
scalars random below 2^254; one shape's outputs at the plan's g are compared word for word with those at g = 1.

    SHAPES=16:4:1:1,20:6:1:1,13:6:2:1,13:6:2:64 REPS=10 REPS_BIG=3 python tools/open_chunks_time.py
(a shape: log_n:log_l:d:count, m = n / d; SWEEP_G=1 times the pointwise pass at every power of two g <= min(l, 64))
"""
import ctypes, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, typlonk_amd
from bench import fr_mont_limbs
from oracle import bls12_381 as O

REPS, REPS_BIG = int(os.environ.get("REPS", "10")), int(os.environ.get("REPS_BIG", "3"))
REPS_KERNEL = int(os.environ.get("REPS_KERNEL", "3"))
S = 0x5EC2E7D00D51
U32P = ctypes.POINTER(ctypes.c_uint32)
F32P = ctypes.POINTER(ctypes.c_float)
FQ_R = 1 << 390


def median_ms(fn, reps):
    fn()   # first-launch costs out of the way
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3)


def plan_g(count, r, l):
    exe = os.path.join(ROOT, "tests", "cpp", "open_chunks_plan_host")
    out = subprocess.run([exe], input=f"{count} {r} {l}\n", capture_output=True, text=True, check=True).stdout
    return json.loads(out)["g"]


def pool_records():
    """24 records of multiples of G in the SRS's internal form (tests/test_gpu_pointwise_msm.py: record)"""
    rng = np.random.default_rng(0x9001)
    recs = []
    for _ in range(24):
        x, y = O.g1_mul(O.G1, int.from_bytes(rng.bytes(32), "little") % O.R)
        recs.append([(v * FQ_R % O.P >> (32 * i)) & 0xFFFFFFFF for v in (x, y) for i in range(12)] + [0] * 8)
    return np.array(recs, dtype=np.uint32)


ctx = typlonk_amd.Context(0)
harness = ctypes.CDLL(os.path.join(ROOT, "tests", "cpp", "libdevice_chunks.so"))
harness.dc_time_pointwise.restype = ctypes.c_int
harness.dc_time_pointwise.argtypes = [U32P, U32P, ctypes.c_uint64, ctypes.c_uint64] + [ctypes.c_uint32] * 3 + [F32P, F32P]
harness.dc_pointwise_msm.restype = ctypes.c_int
harness.dc_pointwise_msm.argtypes = [U32P, U32P, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, U32P, U32P]
POOL = pool_records()
shapes = [tuple(int(v) for v in s.split(":")) for s in os.environ.get("SHAPES", "16:4:1:1,20:6:1:1,13:6:2:1,13:6:2:64").split(",")]
open_all_done = {}

for log_n, log_l, d, count in shapes:
    n, l = 1 << log_n, 1 << log_l
    r, m = n // l, n // d
    reps = REPS_BIG if log_n >= 20 else REPS
    out = {"log_n": log_n, "l": l, "r": r, "m": m, "count": count, "reps": reps}
    sid = ctx.srs_generate(fr_mont_limbs(S), n + 3)
    out["table_build_ms"] = median_ms(lambda: ctx.srs_free(ctx.srs_open_chunks_table(sid, log_n, log_l)), 3)
    tab = ctx.srs_open_chunks_table(sid, log_n, log_l)
    rng = np.random.default_rng(11)
    polys = []
    for _ in range(count):
        b = ctx.alloc(m)
        b.upload(rng.integers(0, 1 << 62, size=(m, 4), dtype=np.uint64))   # < 2^254 < r: canonical Montgomery residues of something
        polys.append(b)
    out["open_chunks_ms"] = median_ms(lambda: ctx.open_chunks(tab, polys, m), reps)
    out["open_chunks_no_evals_ms"] = median_ms(lambda: ctx.open_chunks(tab, polys, m, evals=False), reps)
    out["per_polynomial_ms"] = round(out["open_chunks_ms"] / count, 3)
    ctx.srs_free(tab)
    if log_n not in open_all_done:                                         # the yardstick, once per n
        t1 = {"open_all_table_build_ms": median_ms(lambda: ctx.srs_free(ctx.srs_open_all_table(sid, log_n)), 3)}
        tab1 = ctx.srs_open_all_table(sid, log_n)
        t1["open_all_ms"] = median_ms(lambda: ctx.open_all(tab1, polys[0], m), reps)
        ctx.srs_free(tab1)
        open_all_done[log_n] = t1
    out.update(open_all_done[log_n])
    out["open_all_over_open_chunks_per_polynomial"] = round(out["open_all_ms"] / out["per_polynomial_ms"], 1)
    for b in polys:
        b.free()
    ctx.srs_free(sid)

    # the pointwise pass alone
    outputs, period = count * 2 * r, 2 * r
    k = rng.integers(0, 1 << 32, size=(outputs * l, 8), dtype=np.uint64).astype(np.uint32)
    k[:, 7] &= 0x3FFFFFFF                                                  # < 2^254 < r, canonical
    recs = np.ascontiguousarray(POOL[rng.integers(0, len(POOL), size=l * period)])
    gp, gmax = plan_g(count, r, l), min(l, 64)
    out["plan_g"] = gp
    kp, rp = k.ctypes.data_as(U32P), recs.ctypes.data_as(U32P)
    gs = {1, gp, gmax} | ({1 << i for i in range(gmax.bit_length())} if os.environ.get("SWEEP_G") else set())
    for g in sorted(gs):
        ms = (ctypes.c_float * REPS_KERNEL)()
        rc = harness.dc_time_pointwise(kp, rp, outputs, period, l, g, REPS_KERNEL, ms, None)
        assert rc == 0, rc
        out[f"pointwise_msm_g{g}_ms"] = round(statistics.median(ms), 3)
    ms = (ctypes.c_float * REPS_KERNEL)()
    rc = harness.dc_time_pointwise(kp, rp, outputs, period, l, 0, REPS_KERNEL, None, ms)
    assert rc == 0, rc
    out["pointwise_mul_same_pairs_ms"] = round(statistics.median(ms), 3)
    out["mul_over_msm_plan_g"] = round(out["pointwise_mul_same_pairs_ms"] / out[f"pointwise_msm_g{gp}_ms"], 2)
    if outputs <= 1 << 12 and gp != 1:                                     # the plan's g against g = 1, word for word
        a, b = (np.zeros((outputs, 32), dtype=np.uint32) for _ in range(2))
        guard = np.zeros(1, dtype=np.uint32)
        assert harness.dc_pointwise_msm(kp, rp, outputs, period, l, 1, a.ctypes.data_as(U32P), guard.ctypes.data_as(U32P)) == 0
        assert harness.dc_pointwise_msm(kp, rp, outputs, period, l, gp, b.ctypes.data_as(U32P), guard.ctypes.data_as(U32P)) == 0
        assert (a == b).all()
        out["plan_g_equals_g1"] = True
    print(json.dumps(out), flush=True)
