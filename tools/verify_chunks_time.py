"""Cost of typlonk_verify_chunks -- the multi-proofs of typlonk_open_chunks_*, a batch of cells per call -- beside checking the same
cells one by one, in one session.  Median host wall time of REPS blocking calls after one untimed call, all inputs in host memory
as the call takes them.  Per shape: the honest batch; its split into upload, membership, weights + fold kernels, MSMs and pairing
(the call's own stage times, from one more call with profiling on, where the stages are drained one by one); the same batch with
ONE bad cell, for the bisection's cost, with its folds and its split; and the yardstick -- ONE_BY_ONE cells checked by a call of
their own each (N = 1, M = 1: two MSMs over the proof and the commitment, one l-term MSM and one pairing product per cell), as
milliseconds per cell, and the ratio of N such calls to the batch.

    SHAPES=13:6:128:16384,13:6:1:128,20:6:1:1024 REPS=10 ONE_BY_ONE=64 python tools/verify_chunks_time.py
(a shape: log_n:log_l:polynomials:cells; the cells are the first `cells` of the polynomials' cosets, polynomial-major)
"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, typlonk_amd
from bench import fr_mont_limbs
from oracle import bls12_381 as O
from oracle import pairing as OP

REPS = int(os.environ.get("REPS", "10"))
ONE_BY_ONE = int(os.environ.get("ONE_BY_ONE", "64"))
S = 0x5EC2E7D00D51
SEED = bytes(range(32))


def median_ms(fn, reps):
    fn()   # first-launch costs out of the way
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3)


def g2_limbs(q):
    (x0, x1), (y0, y1) = q
    return np.array([limb for c in (x0, x1, y0, y1) for limb in O.fq_to_mont_limbs(c)], dtype=np.uint64)


ctx = typlonk_amd.Context(0)
shapes = [tuple(int(v) for v in s.split(":")) for s in os.environ.get("SHAPES", "13:6:128:16384,13:6:1:128,20:6:1:1024").split(",")]

for log_n, log_l, polys, cells in shapes:
    n, l = 1 << log_n, 1 << log_l
    r = n // l
    assert cells <= polys * r
    out = {"log_n": log_n, "l": l, "r": r, "commitments": polys, "cells": cells, "reps": REPS}
    sid = ctx.srs_generate(fr_mont_limbs(S), n + 3)
    tab = ctx.srs_open_chunks_table(sid, log_n, log_l)
    rng = np.random.default_rng(11)
    bufs = []
    for _ in range(polys):
        b = ctx.alloc(n)
        b.upload(rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64))   # < 2^254 < r: canonical Montgomery residues of something
        bufs.append(b)
    pxy, pinf, ev = ctx.open_chunks(tab, bufs, n)
    cm = [ctx.msm_dev(sid, b, 0, n) for b in bufs]
    for b in bufs:
        b.free()
    ctx.srs_free(tab)
    cxy = np.array([c[0] for c in cm], dtype=np.uint64).reshape(polys, 12)
    cinf = np.array([c[1] for c in cm], dtype=np.uint8).reshape(polys)
    g2sl = g2_limbs(OP.srs_g2(pow(S, l, O.R))[1])
    cc = np.repeat(np.arange(polys, dtype=np.uint32), r)[:cells].copy()
    ck = np.tile(np.arange(r, dtype=np.uint32), polys)[:cells].copy()
    pxy = np.ascontiguousarray(pxy.reshape(-1, 12)[:cells])
    pinf = np.ascontiguousarray(pinf.reshape(-1)[:cells])
    ev = np.ascontiguousarray(ev.reshape(-1, l, 4)[:cells])

    def call(e=ev, first=0, count=cells, commits=(cxy, cinf), commit_index=cc):
        sl = slice(first, first + count)
        return ctx.verify_chunks(sid, log_n, log_l, g2sl, SEED, commits, commit_index[sl], ck[sl], e[sl], (pxy[sl], pinf[sl]))

    def split(fn):
        ctx.set_profiling(1)
        try:
            res = fn()
            return res, {k: round(v, 3) for k, v in ctx.profile() if k.startswith("chunks_")}
        finally:
            ctx.set_profiling(0)

    res = call()
    assert (res["status"] == 0).all() and res["folds"] == 1
    out["verify_chunks_ms"] = median_ms(call, REPS)
    out["split"] = split(call)[1]
    bad = ev.copy()
    bad[cells // 3, l - 1, 0] ^= np.uint64(1)                                # one evaluation of one cell
    res = call(bad)
    assert res["status"].tolist() == [4 if i == cells // 3 else 0 for i in range(cells)]
    out["one_bad_cell_folds"] = res["folds"]
    out["one_bad_cell_ms"] = median_ms(lambda: call(bad), REPS)
    out["one_bad_cell_split"] = split(lambda: call(bad))[1]
    # the yardstick: the first ONE_BY_ONE cells, a call of its own each
    k1 = min(ONE_BY_ONE, cells)
    zero = np.zeros(cells, dtype=np.uint32)

    def one_by_one():
        for i in range(k1):
            c = int(cc[i])
            res = call(first=i, count=1, commits=(cxy[c:c + 1], cinf[c:c + 1]), commit_index=zero)
            assert res["status"][0] == 0

    out["one_by_one_cells"] = k1
    out["one_by_one_ms_per_cell"] = round(median_ms(one_by_one, 3) / k1, 3)
    out["one_by_one_over_batch"] = round(out["one_by_one_ms_per_cell"] * cells / out["verify_chunks_ms"], 1)
    ctx.srs_free(sid)
    print(json.dumps(out), flush=True)
