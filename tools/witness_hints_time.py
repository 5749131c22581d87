"""typlonk_witness_solve with and without hints (profiles/r27_witness_hints.txt), in one process on one device.

  --plain    the solve of a circuit WITHOUT hints, which typlonk_circuit_set_hints must not slow down: the layered circuit of
             tools/witness_solve_time.py (32 levels, rows shuffled) per --log-n, one witness.  Each of --runs runs is a fresh
             median (best) of --reps calls after --warmup.  Run it against two builds of the library (TYPLONK_LIB_PATH names the
             other one) in turn and compare the medians: --label says which build a line belongs to.
  --hinted   a circuit of (n - 3) / 32 range-check blocks with k = 16 (tests/witness_hints_ref.py, range_check: s = x + y, 16 BITS
             hints, 16 boolean rows, 15 recomposition rows; a sixteenth of the rows feed hints) per --log-n and --counts:
             set_hints_ms (the plan under the hints, one-time), solve_ms, and beside it the same columns filled on one CPU thread
             (tools/witness_hints_fill_cpu, built beside this file) and uploaded, times count.  Every solve is checked once by
             typlonk_witness_check (no failure).
  --inv-chain D   D INV0 hints in a row, each reading the one before (a narrow run of D levels, one hint per level, no rows), at
             2^11 rows, one witness: what a level that holds an inversion costs.
Wall time on the host around the blocking calls.

    python tools/witness_hints_time.py --plain --hinted [--log-n 16 20] [--counts 1 4] [--runs 3] [--reps 20] [--label NAME] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from witness_solve_time import layered_tables, timed   # noqa: E402

K = 16
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def range_blocks(n, k=K):
    """(selector columns as {value: row mask} per selector, perm, hints, input cells) of (n - 3) // 2k range-check blocks"""
    blocks = (n - 3) // (2 * k)
    base = np.arange(blocks, dtype=np.int64) * 2 * k
    sel = [dict() for _ in range(5)]                       # q_l, q_r, q_o, q_m, q_c: value -> rows

    def put(s, value, rows):
        sel[s].setdefault(value, []).append(rows)

    put(0, 1, base), put(1, 1, base), put(2, 1, base)      # s = x + y
    perm = np.arange(3 * n, dtype=np.uint32)

    def tie(*cells):
        for u, v in zip(cells, cells[1:] + cells[:1]):
            perm[u] = v

    tie(2 * n + base, 2 * n + base + 2 * k - 1)
    for i in range(k):
        put(3, 1, base + 1 + i), put(0, R - 1, base + 1 + i)             # b (b - 1) = 0
        tie(base + 1 + i, n + base + 1 + i, base + k + 1 if i == 0 else n + base + k + i)
        if i:
            j = base + k + i                                                # acc + 2^i b_i
            put(0, 1, j), put(1, 1 << i, j), put(2, 1, j)
            if i < k - 1:
                tie(2 * n + j, j + 1)
    hints = np.zeros(blocks * k, dtype=[("kind", "<u4"), ("dst", "<u4"), ("src", "<u4"), ("shift", "<u2"), ("width", "<u2")])
    hints["kind"], hints["width"] = 2, 1
    hints["dst"] = (base[:, None] + 1 + np.arange(k)[None, :]).ravel()
    hints["src"] = np.repeat(2 * n + base, k)
    hints["shift"] = np.tile(np.arange(k), blocks)
    cells = np.concatenate([base, n + base])
    return sel, perm, hints, cells


def compile_circuit(ctx, log_n, columns, perm, cosets):
    bufs = []
    for col in columns:
        b = ctx.alloc(1 << log_n)
        b.upload(col)
        bufs.append(b)
    cid = ctx.circuit_compile(log_n, bufs, perm, cosets)
    for b in bufs:
        b.free()
    return cid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--hinted", action="store_true")
    ap.add_argument("--log-n", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inv-chain", type=int, default=0)
    ap.add_argument("--label", default="branch")
    ap.add_argument("--out")
    args = ap.parse_args()

    import typlonk_amd
    from typlonk_amd.circuits import fr_mont_limbs

    ctx = typlonk_amd.Context(0)
    cosets = [fr_mont_limbs(k) for k in (2, 3, 4)]
    one = fr_mont_limbs(1)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def solve_times(cid, cells, values, outs):
        solve = lambda: ctx.witness_solve(cid, cosets, cells, values, outs)   # noqa: E731
        t = [timed(solve) for _ in range(args.warmup + args.reps)][args.warmup:]
        rep = ctx.witness_check(cid, outs, None, None, cosets, cap=4)
        assert all(r["gate_failures"] == 0 and r["copy_failures"] == 0 for r in rep), rep[0]
        return t

    for log_n in args.log_n:
        n = 1 << log_n
        if args.plain:
            flags, perm, inputs = layered_tables(n)
            columns = []
            for f in flags:
                col = np.zeros((n, 4), dtype=np.uint64)
                col[f] = one
                columns.append(col)
            cid = compile_circuit(ctx, log_n, columns, perm, cosets)
            info = ctx.witness_solve_plan(cid, cosets)
            cells = inputs + [i * n + n - 3 + k for i in range(3) for k in range(3)]
            rng = np.random.default_rng(log_n)
            values = np.stack([fr_mont_limbs(int(v)) for v in rng.integers(2, 1 << 62, size=len(cells))])[None]
            outs = [[ctx.alloc(n) for _ in range(3)]]
            for run in range(args.runs):
                t = solve_times(cid, cells, values, outs)
                emit({"what": "plain", "lib": args.label, "log_n": log_n, "shape": "layered", "count": 1, "run": run, **info, "reps": args.reps,
                      "solve_ms": round(statistics.median(t), 4), "solve_best_ms": round(min(t), 4)})
            for b in outs[0]:
                b.free()
            ctx.circuit_free(cid)
        if args.hinted:
            sel, perm, hints, cells = range_blocks(n)
            columns = []
            for s in sel:
                col = np.zeros((n, 4), dtype=np.uint64)
                for value, rows in s.items():
                    col[np.concatenate(rows)] = fr_mont_limbs(value)
                columns.append(col)
            cid = compile_circuit(ctx, log_n, columns, perm, cosets)
            set_ms = timed(lambda: ctx.circuit_set_hints(cid, cosets, hints))
            info = ctx.witness_solve_plan(cid, cosets)
            cpu = json.loads(subprocess.run([os.path.join(ROOT, "tools", "witness_hints_fill_cpu"), str(log_n), str(K), "5"], check=True,
                                            capture_output=True, text=True).stdout)
            column = np.zeros((n, 4), dtype=np.uint64)
            up = ctx.alloc(n)
            upload_ms = 3 * statistics.median(timed(lambda: up.upload(column)) for _ in range(5))
            up.free()
            rng = np.random.default_rng(100 + log_n)
            small = {int(v): fr_mont_limbs(int(v)) for v in range(1 << 12)}
            for count in args.counts:
                values = np.stack([np.stack([small[int(v)] for v in rng.integers(0, 1 << 12, size=len(cells))]) for _ in range(count)])
                outs = [[ctx.alloc(n) for _ in range(3)] for _ in range(count)]
                t = solve_times(cid, cells, values, outs)
                fill = cpu["fill_ms"]
                emit({"what": "hinted", "lib": args.label, "log_n": log_n, "shape": f"range_check k={K}", "count": count, "hints": len(hints),
                      "inputs": len(cells), **info, "set_hints_ms": round(set_ms, 2), "reps": args.reps,
                      "solve_ms": round(statistics.median(t), 3), "solve_best_ms": round(min(t), 3), "cpu_fill_ms": round(fill * count, 3),
                      "upload_ms": round(upload_ms * count, 3), "cpu_total_ms": round((fill + upload_ms) * count, 3),
                      "solve_over_cpu": round(statistics.median(t) / ((fill + upload_ms) * count), 4)})
                for b in [b for bs in outs for b in bs]:
                    b.free()
            ctx.circuit_free(cid)
    if args.inv_chain:
        log_n, d = 11, args.inv_chain
        n = 1 << log_n
        assert d < n - 3
        cid = compile_circuit(ctx, log_n, [np.zeros((n, 4), dtype=np.uint64)] * 5, np.arange(3 * n, dtype=np.uint32), cosets)
        ctx.circuit_set_hints(cid, cosets, [(1, i + 1, i, 0, 0) for i in range(d)])
        info = ctx.witness_solve_plan(cid, cosets)
        outs = [[ctx.alloc(n) for _ in range(3)]]
        t = solve_times(cid, [0], fr_mont_limbs(0x1234567)[None, None], outs)
        a = outs[0][0].download()
        assert np.array_equal(a[0], a[2]) and not np.array_equal(a[0], a[1])
        emit({"what": "inv_chain", "lib": args.label, "log_n": log_n, "count": 1, "hints": d, **info, "reps": args.reps,
              "solve_ms": round(statistics.median(t), 3), "us_per_level": round(1e3 * statistics.median(t) / d, 3)})
        for b in outs[0]:
            b.free()
        ctx.circuit_free(cid)
    ctx.close()
    if args.out and lines:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
