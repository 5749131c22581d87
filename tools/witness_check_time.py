"""typlonk_witness_check against the proof it pre-empts (profiles/r15_witness_check.txt), in one process on one device.
Per --log-n (squaring chain of typlonk_amd.circuits, SRS with fixed-base tables, no public inputs) and per --counts:
  perm_ms    typlonk_circuit_permutation alone on a freshly loaded circuit (the recovery kernels + one 16-byte readback)
  first_ms   the first typlonk_witness_check on another freshly loaded circuit: recovery + the five selector transforms + the check
  steady_ms  the call once both caches exist: median (best) of --reps after --warmup calls, cap = 16
  prove_ms   typlonk_prove_compact on the same circuit and witness, alternated call by call with the steady check
  ratio      steady_ms / prove_ms
Wall time on the host around the blocking calls.  `--trace-run` makes only a few steady calls at the first --log-n, for a
`rocprofv3 --kernel-trace --stats` run (kernel times: tools/rocpd_stats.py).

    python tools/witness_check_time.py [--log-n 16 20] [--counts 1 4] [--reps 20] [--warmup 3] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SECRET = 0x5EC2E7D00D51


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()

    import typlonk_amd
    from typlonk_amd import capi
    from typlonk_amd.circuits import SquaringChain, fr_mont_limbs

    ctx = typlonk_amd.Context(0)
    lines = []
    for log_n in args.log_n:
        n = 1 << log_n
        chain = SquaringChain(ctx, log_n)
        def check(k):
            return ctx.witness_check(chain.circuit, [chain.wire_evals] * k, None, None, chain.cosets, cap=16)

        if args.trace_run:
            for _ in range(3):
                assert check(1)[0]["gate_failures"] == 0
            chain.free()
            break
        defects = C.c_uint64()
        ks = capi._cosets_arg(chain.cosets)
        perm_ms = timed(lambda: ctx._chk(ctx.lib.typlonk_circuit_permutation(ctx.h, chain.circuit, C.byref(ks), None, C.byref(defects))))
        assert defects.value == 0
        chain.free()
        chain = SquaringChain(ctx, log_n)
        first_ms = timed(lambda: check(1))
        sid = ctx.srs_generate(fr_mont_limbs(SECRET), n + 3)
        ctx.srs_precompute(sid)
        def prove():
            return ctx.prove_compact(sid, chain.circuit, chain.wire_evals, None, 0, chain.cosets)

        for k in args.counts:
            t_check, t_prove = [], []
            for r in range(args.warmup + args.reps):
                a, b = timed(lambda: check(k)), timed(prove)
                if r >= args.warmup:
                    t_check.append(a)
                    t_prove.append(b)
            rep = check(k)
            assert all(x["gate_failures"] == 0 and x["copy_failures"] == 0 for x in rep)
            rec = {"log_n": log_n, "count": k, "perm_ms": round(perm_ms, 3), "first_ms": round(first_ms, 3),
                   "steady_ms": round(statistics.median(t_check), 4), "steady_best_ms": round(min(t_check), 4),
                   "prove_compact_ms": round(statistics.median(t_prove), 3),
                   "ratio": round(statistics.median(t_check) / statistics.median(t_prove), 5),
                   "ratio_per_witness": round(statistics.median(t_check) / k / statistics.median(t_prove), 5)}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        ctx.srs_free(sid)
        chain.free()
    ctx.close()
    if args.out and lines:
        with open(args.out, "w") as f:
            f.write("# python tools/witness_check_time.py " + " ".join(sys.argv[1:]) + "\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
