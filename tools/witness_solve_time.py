"""typlonk_witness_solve against what it replaces and what follows it (profiles/r25_witness_solve.txt), in one process on one
device.  Per --log-n, for two circuits of n - 3 gates -- the squaring chain (depth n - 3, one row per level) and a layered
circuit of 32 levels (gate i of a level takes outputs i and i + 1 of the level before; rows shuffled in the table) -- and per
--counts:
  plan_ms     the first typlonk_witness_solve_plan on the freshly compiled circuit: the check cache, the q_o kernel, two
              downloads, solve_plan on the host, three uploads (one-time, per circuit)
  solve_ms    typlonk_witness_solve of `count` witnesses once the plan exists: median (best) of --reps after --warmup calls; a
              shape whose call takes longer than --slow-ms gets --slow-reps instead
  cpu_fill_ms the same fill by the C++ front end's computing run on one thread (tools/witness_fill_cpu, built beside this file),
              times count; upload_ms: typlonk_buf_upload of the three columns it would then need, times count
  prove_ms    typlonk_prove_compact (count 1) / typlonk_prove_batch_compact of the solved witnesses
Every solve is checked once by typlonk_witness_check (no failure).  Wall time on the host around the blocking calls.

    python tools/witness_solve_time.py [--log-n 16 20] [--counts-at 16:1,64 20:1,4] [--reps 20] [--warmup 2] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SECRET = 0x5EC2E7D00D51
LEVELS = 32


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def chain_tables(n):
    """(selector rows as 0/1 flags (5, n), perm, input cells) of the squaring chain"""
    g = n - 3
    sel = np.zeros((5, n), dtype=bool)
    sel[2, :g] = sel[3, :g] = True                          # Mul = [0, 0, 1, 1, 0]
    perm = np.arange(3 * n, dtype=np.uint32)
    perm[0], perm[n] = n, 0                                 # (a_0 b_0)
    j = np.arange(g - 1)
    perm[2 * n + j], perm[j + 1], perm[n + j + 1] = j + 1, n + j + 1, 2 * n + j    # (c_j a_{j+1} b_{j+1})
    return sel, perm, [0]


def layered_tables(n, seed=25):
    """the layered circuit: LEVELS levels of (n - 3) // LEVELS rows (the last takes the remainder out of the first rows of a
    further level), multiplications and additions in turn, rows shuffled; the inputs are the a cells of level 0 (b_i = a_{i+1})"""
    g = n - 3
    width = g // LEVELS
    pos = np.random.default_rng(seed).permutation(g).astype(np.int64)    # logical row -> table row
    level, idx = np.arange(g) // width, np.arange(g) % width
    sel = np.zeros((5, n), dtype=bool)
    mul = ((level + idx) & 1) == 0
    sel[2, pos] = True
    sel[3, pos[mul]] = True
    sel[0, pos[~mul]] = sel[1, pos[~mul]] = True
    perm = np.arange(3 * n, dtype=np.uint32)
    # level 0: (a_i  b_{i-1}) -- one input per column position
    first = pos[:width]
    perm[first], perm[n + np.roll(first, 1)] = n + np.roll(first, 1), first
    # output i of level k - 1 feeds a of row i and b of row i - 1 of level k (rows that exist)
    for k in range(1, int(level.max()) + 1):
        rows = pos[k * width:(k + 1) * width]
        w = len(rows)
        src = pos[(k - 1) * width:k * width]
        a_of = np.full(width, -1, dtype=np.int64)
        b_of = np.full(width, -1, dtype=np.int64)
        a_of[:w] = rows
        b_of[(np.arange(w) + 1) % width] = n + rows
        for i in range(width):
            cyc = [2 * n + src[i]] + [x for x in (a_of[i], b_of[i]) if x >= 0]
            for u, v in zip(cyc, cyc[1:] + cyc[:1]):
                perm[u] = v
    return sel, perm, sorted(int(x) for x in first)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--counts-at", nargs="+", default=["16:1,64", "20:1,4"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--slow-ms", type=float, default=500.0)
    ap.add_argument("--slow-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    args = ap.parse_args()
    counts_at = {int(s.split(":")[0]): [int(x) for x in s.split(":")[1].split(",")] for s in args.counts_at}

    import typlonk_amd
    from typlonk_amd.circuits import fr_mont_limbs

    ctx = typlonk_amd.Context(0)
    cosets = [fr_mont_limbs(k) for k in (2, 3, 4)]
    one = fr_mont_limbs(1)
    lines = []
    for log_n in args.log_n:
        n = 1 << log_n
        cpu = json.loads(subprocess.run([os.path.join(ROOT, "tools", "witness_fill_cpu"), str(log_n), "5" if log_n >= 20 else "20"],
                                        check=True, capture_output=True, text=True).stdout)
        sid = ctx.srs_generate(fr_mont_limbs(SECRET), n + 3)
        ctx.srs_precompute(sid)
        column = np.zeros((n, 4), dtype=np.uint64)
        up = ctx.alloc(n)
        upload_ms = 3 * statistics.median(timed(lambda: up.upload(column)) for _ in range(5))
        up.free()
        for shape, (sel, perm, inputs) in (("chain", chain_tables(n)), ("layered", layered_tables(n))):
            bufs = []
            for flags in sel:
                col = np.zeros((n, 4), dtype=np.uint64)
                col[flags] = one
                b = ctx.alloc(n)
                b.upload(col)
                bufs.append(b)
            cid = ctx.circuit_compile(log_n, bufs, perm, cosets)
            for b in bufs:
                b.free()
            info = {}
            plan_ms = timed(lambda: info.update(ctx.witness_solve_plan(cid, cosets)))
            cells = inputs + [i * n + n - 3 + k for i in range(3) for k in range(3)]
            rng = np.random.default_rng(log_n)
            for count in counts_at.get(log_n, [1]):
                values = np.stack([np.stack([fr_mont_limbs(int(v)) for v in rng.integers(2, 1 << 62, size=len(cells))])
                                   for _ in range(count)])
                outs = [[ctx.alloc(n) for _ in range(3)] for _ in range(count)]
                solve = lambda: ctx.witness_solve(cid, cosets, cells, values, outs)   # noqa: E731
                probe = timed(solve)
                reps = args.reps if probe <= args.slow_ms else args.slow_reps
                t_solve = [timed(solve) for _ in range(args.warmup + reps)][args.warmup:]
                rep = ctx.witness_check(cid, outs, None, None, cosets, cap=4)
                assert all(r["gate_failures"] == 0 and r["copy_failures"] == 0 for r in rep), rep[0]
                if count == 1:
                    prove = lambda: ctx.prove_compact(sid, cid, outs[0], None, 0, cosets)   # noqa: E731
                else:
                    prove = lambda: ctx.prove_batch_compact(sid, cid, outs, None, None, cosets)   # noqa: E731
                t_prove = [timed(prove) for _ in range(1 + 3)][1:]
                fill = cpu["chain_fill_ms" if shape == "chain" else "layered_fill_ms"]
                rec = {"log_n": log_n, "shape": shape, "count": count, **info, "plan_ms": round(plan_ms, 2), "reps": reps,
                       "solve_ms": round(statistics.median(t_solve), 3), "solve_best_ms": round(min(t_solve), 3),
                       "cpu_fill_ms": round(fill * count, 3), "upload_ms": round(upload_ms * count, 3),
                       "cpu_total_ms": round((fill + upload_ms) * count, 3), "prove_ms": round(statistics.median(t_prove), 2),
                       "solve_over_cpu": round(statistics.median(t_solve) / ((fill + upload_ms) * count), 3),
                       "solve_over_prove": round(statistics.median(t_solve) / statistics.median(t_prove), 4)}
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
                for b in [b for bs in outs for b in bs]:
                    b.free()
            ctx.circuit_free(cid)
        ctx.srs_free(sid)
    ctx.close()
    if args.out and lines:
        with open(args.out, "w") as f:
            f.write("# python tools/witness_solve_time.py " + " ".join(sys.argv[1:]) + "\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
