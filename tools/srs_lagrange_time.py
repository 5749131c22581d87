"""Cost of typlonk_srs_g1_ntt, the Lagrange form of an SRS and back, beside typlonk_srs_contribute on the same entry -- one
255-step ladder per point, the unit the transform's (n/2)(log_n - 1) + n ladders are counted in -- and, at the largest size,
what the Lagrange entry buys: a commitment from evaluations as one MSM against inverse transform + MSM.  Median wall time of
REPS blocking calls each (REPS_BIG at 2^20 and above) after one untimed call.  The round trip is compared word for word with
the source and the two commitments with each other.

    SIZES=16,20 REPS=20 REPS_BIG=5 python tools/srs_lagrange_time.py
"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, typlonk_amd
from bench import fr_mont_limbs
from oracle import bls12_381 as O
from oracle import pairing as PR

REPS, REPS_BIG = int(os.environ.get("REPS", "20")), int(os.environ.get("REPS_BIG", "5"))
S, T = 0x5EC2E7D00D51, 0x2F7A11C0FFEE5EED2F7A11C0FFEE5EED2F7A11C0FFEE5EED2F7A11C0FFEE5EED % O.R


def median_ms(fn, reps):
    fn()   # first-launch costs out of the way
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3)


ctx = typlonk_amd.Context(0)
(x0, x1), (y0, y1) = PR.g2_mul(PR.G2, S)
g2s = np.array([l for c in (x0, x1, y0, y1) for l in O.fq_to_mont_limbs(c)], dtype=np.uint64)
sizes = [int(x) for x in os.environ.get("SIZES", "16,20").split(",")]

for log_n in sizes:
    n = 1 << log_n
    reps = REPS_BIG if log_n >= 20 else REPS
    out = {"log_n": log_n, "len": n + 3, "reps": reps}
    sid = ctx.srs_generate(fr_mont_limbs(S), n + 3)
    out["srs_contribute_ms"] = median_ms(lambda: ctx.srs_free(ctx.srs_contribute(sid, fr_mont_limbs(T), g2s)[0]), reps)
    out["to_lagrange_ms"] = median_ms(lambda: ctx.srs_free(ctx.srs_lagrange(sid, log_n)), reps)
    lag = ctx.srs_lagrange(sid, log_n)
    out["from_lagrange_ms"] = median_ms(lambda: ctx.srs_free(ctx.srs_from_lagrange(lag, log_n)), reps)
    back = ctx.srs_from_lagrange(lag, log_n)
    a, b = ctx.srs_download(back), ctx.srs_download(sid, 0, n)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
    out["round_trip_equals_source"] = True
    del a, b
    ctx.srs_free(back)
    unit = out["srs_contribute_ms"] * log_n / 2
    out["to_lagrange_over_contribute_x_log_n_half"] = round(out["to_lagrange_ms"] / unit, 3)
    out["from_lagrange_over_contribute_x_log_n_half"] = round(out["from_lagrange_ms"] / unit, 3)
    if log_n == max(sizes):
        rng = np.random.default_rng(7)
        evals = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)   # < 2^254 < r: canonical Montgomery residues of something
        buf = ctx.alloc(n)
        work = ctx.alloc(n)
        buf.upload(evals)

        def from_evaluations():
            return ctx.msm_dev(lag, buf, 0, n)

        def from_coefficients():
            work.upload(evals)                     # the column as the caller holds it; the transform is in place
            ctx.ntt_dev(work, log_n, inverse=True)
            return ctx.msm_dev(sid, work, 0, n)

        def upload_only():
            work.upload(evals)

        p, q = from_evaluations(), from_coefficients()
        assert (p[0] == q[0]).all() and p[1] == q[1]
        out["commit_from_evaluations_equal"] = True
        out["commit_msm_over_lagrange_ms"] = median_ms(from_evaluations, REPS)
        out["commit_upload_intt_msm_ms"] = median_ms(from_coefficients, REPS)
        out["upload_ms"] = median_ms(upload_only, REPS)
        for tables in (sid, lag):
            ctx.srs_precompute(tables)
        out["commit_msm_over_lagrange_tables_ms"] = median_ms(from_evaluations, REPS)
        out["commit_upload_intt_msm_tables_ms"] = median_ms(from_coefficients, REPS)
        buf.free()
        work.free()
    ctx.srs_free(lag)
    ctx.srs_free(sid)
    print(json.dumps(out), flush=True)
