"""Batched proving measurement (profiles/r09_prove_batch.txt): proofs per second of typlonk_prove_batch against a loop of
typlonk_prove on the same context, the two alternated call by call so that both see the same clocks.  The witness of every
proof is the squaring chain's (typlonk_amd.circuits); the columns are on the device.  Wall time on the host per call, best
and median of --reps; kernel times come from a separate rocprofv3 --kernel-trace --stats run.

    python tools/prove_batch_bench.py [--log-n 12 16 18 20] [--counts 1 8 32] [--reps 5] [--shape {reference,compact}]

--shape compact (profiles/r12_prove_batch_compact.txt) alternates typlonk_prove_batch_compact against a loop of
typlonk_prove_compact instead, and times typlonk_prove_batch (the reference shape) in the same alternation for context; its
rows also carry the loop's worst repetition, for the loop's own spread.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[12, 16, 18, 20])
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", choices=["reference", "compact"], default="reference")
    args = ap.parse_args()

    import typlonk_amd
    from typlonk_amd.circuits import SquaringChain, fr_mont_limbs

    ctx = typlonk_amd.Context(0)
    rows = []
    for log_n in args.log_n:
        n = 1 << log_n
        chain = SquaringChain(ctx, log_n)
        sid = ctx.srs_generate(fr_mont_limbs(0x5EC2E7D00D51), n + 3)
        cols = chain.wire_evals
        for count in args.counts:
            wires = [cols] * count

            compact = args.shape == "compact"

            def ref_batch():
                _, st = ctx.prove_batch(sid, chain.circuit, wires, None, chain.cosets)
                assert st == [0] * count

            def compact_batch():
                _, st = ctx.prove_batch_compact(sid, chain.circuit, wires, None, None, chain.cosets)
                assert st == [0] * count

            def loop():
                for _ in range(count):
                    if compact:
                        ctx.prove_compact(sid, chain.circuit, cols, None, 0, chain.cosets)
                    else:
                        ctx.prove_native(sid, chain.circuit, cols, None, chain.cosets)

            batch = compact_batch if compact else ref_batch
            batch()   # warm: workspaces of both forms, tables
            loop()
            tb, tl, tr = [], [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                batch()
                tb.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                loop()
                tl.append(time.perf_counter() - t0)
                if compact:
                    t0 = time.perf_counter()
                    ref_batch()
                    tr.append(time.perf_counter() - t0)
            r = {"log_n": log_n, "count": count,
                 "batch_ms": round(1e3 * statistics.median(tb), 3), "loop_ms": round(1e3 * statistics.median(tl), 3),
                 "batch_best_ms": round(1e3 * min(tb), 3), "loop_best_ms": round(1e3 * min(tl), 3)}
            r["batch_proofs_per_s"] = round(count / statistics.median(tb), 1)
            r["loop_proofs_per_s"] = round(count / statistics.median(tl), 1)
            r["speedup"] = round(statistics.median(tl) / statistics.median(tb), 3)
            if compact:
                r["shape"] = "compact"
                r["loop_worst_ms"] = round(1e3 * max(tl), 3)
                r["batch_worst_ms"] = round(1e3 * max(tb), 3)
                r["reference_batch_ms"] = round(1e3 * statistics.median(tr), 3)
            rows.append(r)
            print(f"log_n={log_n:2d} count={count:3d}  batch {r['batch_ms']:9.2f} ms ({r['batch_proofs_per_s']:8.1f} proofs/s)  "
                  f"loop {r['loop_ms']:9.2f} ms ({r['loop_proofs_per_s']:8.1f} proofs/s)  x{r['speedup']:.2f}  "
                  f"(best {r['batch_best_ms']:.2f} / {r['loop_best_ms']:.2f} ms)"
                  + (f"  worst {r['batch_worst_ms']:.2f} / {r['loop_worst_ms']:.2f} ms  reference batch {r['reference_batch_ms']:.2f} ms"
                     if compact else ""), flush=True)
        ctx.srs_free(sid)
        chain.free()
    ctx.close()
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
