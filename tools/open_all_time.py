"""Cost of typlonk_srs_open_all_table and typlonk_open_all_dev -- a polynomial's openings at every point of its domain in one
call -- beside the only other route: typlonk_open_dev + one MSM per point, measured on 16 points in the same session, reported
per opening and multiplied by n.  Median wall time of REPS blocking calls (REPS_BIG at 2^20 and above; 3 table builds) after
one untimed call.  The 16 openings of the existing route are compared word for word with the same proofs and evaluations of
open_all.  `ladders` counts the 255-step scalar multiplications of a call, 2n + n log_n + (n/2)(log_n - 1), and
`open_all_over_ladders` divides the measured time by ladders x 29 ms per 2^19, the rate of a filled stage of
typlonk_srs_g1_ntt (profiles/r29_srs_lagrange.txt).  `download_n_ms` is typlonk_srs_download of n records: the copy and the
host's conversion of n proofs, which open_all's wall time contains.

    SIZES=16,20 REPS=20 REPS_BIG=5 python tools/open_all_time.py
"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, typlonk_amd
from bench import fr_mont_limbs
from oracle import bls12_381 as O

REPS, REPS_BIG = int(os.environ.get("REPS", "20")), int(os.environ.get("REPS_BIG", "5"))
S = 0x5EC2E7D00D51
STAGE_MS_PER_2_19 = 29.0
POINTS = 16


def median_ms(fn, reps):
    fn()   # first-launch costs out of the way
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3)


ctx = typlonk_amd.Context(0)
sizes = [int(x) for x in os.environ.get("SIZES", "16,20").split(",")]

for log_n in sizes:
    n = 1 << log_n
    reps = REPS_BIG if log_n >= 20 else REPS
    out = {"log_n": log_n, "srs_len": n + 3, "reps": reps}
    sid = ctx.srs_generate(fr_mont_limbs(S), n + 3)
    out["table_build_ms"] = median_ms(lambda: ctx.srs_free(ctx.srs_open_all_table(sid, log_n)), 3)
    tab = ctx.srs_open_all_table(sid, log_n)
    rng = np.random.default_rng(11)
    coeffs = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)   # < 2^254 < r: canonical Montgomery residues of something
    poly, q = ctx.alloc(n), ctx.alloc(n)
    poly.upload(coeffs)
    out["open_all_ms"] = median_ms(lambda: ctx.open_all(tab, poly), reps)
    out["open_all_no_evals_ms"] = median_ms(lambda: ctx.open_all(tab, poly, evals=False), reps)
    out["download_n_ms"] = median_ms(lambda: ctx.srs_download(tab, 0, n), reps)
    xy, inf, ev = ctx.open_all(tab, poly)

    w = O.domain_root(log_n)
    ks = sorted({0, 1, n // 2, n - 1} | {int(k) for k in rng.integers(0, n, size=POINTS)})[:POINTS]
    zs = [fr_mont_limbs(pow(w, k, O.R)) for k in ks]

    def one_by_one():
        return [(ctx.open_dev(poly, n, z, q), ctx.msm_dev(sid, q, 0, n - 1)) for z in zs]

    for k, (y, (pxy, pinf)) in zip(ks, one_by_one()):
        assert (y == ev[k]).all() and (pxy == xy[k]).all() and pinf == inf[k], k
    out["points_compared"] = len(ks)
    out["open_dev_msm_per_opening_ms"] = round(median_ms(one_by_one, reps) / len(ks), 4)
    ctx.srs_precompute(sid)
    out["open_dev_msm_tables_per_opening_ms"] = round(median_ms(one_by_one, reps) / len(ks), 4)
    best = min(out["open_dev_msm_per_opening_ms"], out["open_dev_msm_tables_per_opening_ms"])
    out["n_openings_one_by_one_s"] = round(best * n / 1e3, 1)
    out["one_by_one_over_open_all"] = round(best * n / out["open_all_ms"], 1)
    ladders = 2 * n + n * log_n + (n // 2) * (log_n - 1)
    out["ladders"] = ladders
    out["open_all_over_ladders"] = round(out["open_all_ms"] / (ladders * STAGE_MS_PER_2_19 / (1 << 19)), 3)
    out["table_over_ladders"] = round(out["table_build_ms"] / (n * log_n * STAGE_MS_PER_2_19 / (1 << 19)), 3)
    poly.free()
    q.free()
    ctx.srs_free(tab)
    ctx.srs_free(sid)
    print(json.dumps(out), flush=True)
