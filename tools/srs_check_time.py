"""Cost of a powers-of-tau step on the device: typlonk_srs_check (without and with fixed-base tables, and with one bad link, so
that the bisection runs) and typlonk_srs_contribute, beside typlonk_srs_generate and typlonk_srs_load_compressed of the same
session.  Median wall time of REPS blocking calls each; every verdict is asserted, and the contribution is compared with
typlonk_srs_generate(s t).  The check of a 2-point SRS is printed too: one fold with next to nothing on the device, i.e. the
host pairing product's own time.

    SIZES=16,20 REPS=20 python tools/srs_check_time.py
"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, typlonk_amd
from bench import fr_mont_limbs
from oracle import bls12_381 as O
from oracle import pairing as PR

REPS = int(os.environ.get("REPS", "20"))
S, T = 0x5EC2E7D00D51, 0x2F7A11C0FFEE5EED2F7A11C0FFEE5EED2F7A11C0FFEE5EED2F7A11C0FFEE5EED % O.R
SEED = bytes(range(32))


def g2_limbs(q):
    (x0, x1), (y0, y1) = q
    return np.array([l for c in (x0, x1, y0, y1) for l in O.fq_to_mont_limbs(c)], dtype=np.uint64)


def median_ms(fn, reps=REPS):
    fn()   # first-launch costs out of the way
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3)


ctx = typlonk_amd.Context(0)
g2s = g2_limbs(PR.g2_mul(PR.G2, S))
two = ctx.srs_generate(fr_mont_limbs(S), 2)
assert ctx.srs_check(two, g2s, SEED) == {"verdict": 0, "point_class": 0, "index": 0, "bad_points": 0, "folds": 1}
print(json.dumps({"len": 2, "srs_check_ms": median_ms(lambda: ctx.srs_check(two, g2s, SEED)), "folds": 1}), flush=True)
ctx.srs_free(two)

for log_n in [int(x) for x in os.environ.get("SIZES", "16,20").split(",")]:
    n = (1 << log_n) + 3
    out = {"log_n": log_n, "len": n, "reps": REPS}
    out["srs_generate_ms"] = median_ms(lambda: ctx.srs_free(ctx.srs_generate(fr_mont_limbs(S), n)))
    sid = ctx.srs_generate(fr_mont_limbs(S), n)
    blob = ctx.srs_download_compressed(sid)
    out["srs_load_compressed_ms"] = median_ms(lambda: ctx.srs_free(ctx.srs_load_compressed(blob)))
    del blob

    def valid(s):
        rep = ctx.srs_check(s, g2s, SEED)
        assert (rep["verdict"], rep["folds"]) == (0, 1), rep

    out["srs_check_ms"] = median_ms(lambda: valid(sid))
    # one bad link in the middle: the whole-SRS fold and the bisection's
    xy, inf = ctx.srs_download(sid)
    j = n // 2 + 1
    p = O.g1_add(O.g1_from_limbs([int(v) for v in xy[j]], int(inf[j])), O.G1)
    xy[j] = O.g1_to_limbs(p)[0]
    bad = ctx.srs_load(xy, inf)
    del xy, inf
    folds = []

    def broken():
        rep = ctx.srs_check(bad, g2s, SEED)
        assert (rep["verdict"], rep["index"]) == (3, j - 1), rep
        folds.append(rep["folds"])

    out["srs_check_bad_link_ms"] = median_ms(broken, reps=max(3, REPS // 4))
    out["srs_check_bad_link_folds"] = folds[-1]
    ctx.srs_free(bad)

    def contribute():
        new, _ = ctx.srs_contribute(sid, fr_mont_limbs(T), g2s)
        ctx.srs_free(new)

    out["srs_contribute_ms"] = median_ms(contribute)
    new, g2n = ctx.srs_contribute(sid, fr_mont_limbs(T), g2s)
    ref = ctx.srs_generate(fr_mont_limbs(S * T % O.R), n)
    a, b = ctx.srs_download(new), ctx.srs_download(ref)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
    out["contribute_equals_generate"] = True
    del a, b
    ctx.srs_free(ref)
    assert ctx.srs_check(new, g2n, SEED)["verdict"] == 0
    ctx.srs_free(new)
    t0 = time.perf_counter()
    ctx.srs_precompute(sid, 0)
    out["srs_precompute_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    out["srs_check_tables_ms"] = median_ms(lambda: valid(sid))
    ctx.srs_free(sid)
    print(json.dumps(out), flush=True)
