"""typlonk_circuit_compile against the path it replaces (profiles/r18_circuit_compile.txt), in one process on one device, on the
squaring chain of typlonk_amd.circuits at --log-n rows:
  host_path_ms  what a caller does today between the tables and typlonk_circuit_load, as typlonk_amd/circuits.py does it: w^j as
                the transform of X, three lincombs and downloads, the sigma rows spliced in numpy, eight uploads and eight
                inverse transforms (the witness and typlonk_circuit_load itself not included)
  load_ms       typlonk_circuit_load of the eight coefficient vectors already on the device
  compile_ms    typlonk_circuit_compile of the five selector evaluation buffers already on the device and the host permutation
                (its 12n-byte upload included); alternated call by call with load_ms, median (best) of --reps after --warmup
  first_check_loaded_ms / first_check_compiled_ms
                the first typlonk_witness_check on a fresh circuit of either kind (the loaded one recovers its permutation)
Wall time on the host around the blocking calls; every circuit is freed again outside the timed region.  `--trace-run compiled`
makes three times (compile, first witness check, free) and nothing else, `--trace-run loaded` the same on loaded circuits, each
for a `rocprofv3 --kernel-trace --stats` run of its own: the kernel times, and which of the two runs perm_recover_kernel.

    python tools/circuit_compile_time.py [--log-n 20] [--reps 10] [--warmup 2] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/circuit_compile_time.py --trace-run compiled
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def chain_permutation(n: int, g: int) -> np.ndarray:
    """a_0 <-> b_0, and c_j -> a_{j+1} -> b_{j+1} -> c_j for j <= g - 2, over the flat cells col * n + row"""
    perm = np.arange(3 * n, dtype=np.uint32)
    j = np.arange(max(g - 1, 0), dtype=np.uint32)
    perm[0], perm[n] = n, 0
    perm[2 * n + j] = j + 1
    perm[j + 1] = n + j + 1
    perm[n + j + 1] = 2 * n + j
    return perm


def host_path(ctx, log_n, sel_evals, g):
    """typlonk_amd/circuits.py's way from the tables to the eight coefficient buffers"""
    from typlonk_amd.circuits import COSETS, fr_mont_limbs

    n = 1 << log_n
    xpoly = np.zeros((n, 4), dtype=np.uint64)
    xpoly[1 % n] = fr_mont_limbs(1)
    roots = ctx.alloc(n)
    roots.upload(xpoly)
    ctx.ntt_dev(roots, log_n)
    kr = []
    for k in COSETS:
        b = ctx.alloc(n)
        ctx.lincomb_dev([roots], [fr_mont_limbs(k)], n, b)
        kr.append(b.download())
        b.free()
    roots.free()
    ka, kb, kc = kr
    sa, sb, sc = ka.copy(), kb.copy(), kc.copy()
    sa[0] = kb[0]
    sb[0] = ka[0]
    if g >= 2:
        sc[0:g - 1] = ka[1:g]
        sa[1:g] = kb[1:g]
        sb[1:g] = kc[0:g - 1]
    bufs = []
    for ev in list(sel_evals) + [sa, sb, sc]:
        b = ctx.alloc(n)
        b.upload(ev)
        ctx.ntt_dev(b, log_n, inverse=True)
        bufs.append(b)
    ctx.sync()
    return bufs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace-run", choices=("compiled", "loaded"))
    ap.add_argument("--out")
    args = ap.parse_args()

    import typlonk_amd
    from typlonk_amd.circuits import SquaringChain

    ctx = typlonk_amd.Context(0)
    log_n = args.log_n
    chain = SquaringChain(ctx, log_n, keep_host=True)
    n, g = chain.n, chain.gates
    sel_evals = chain.host_inputs()["selectors"]
    perm = chain_permutation(n, g)
    sel_bufs = []
    for ev in sel_evals:
        b = ctx.alloc(n)
        b.upload(ev)
        sel_bufs.append(b)

    def compile_():
        return ctx.circuit_compile(log_n, sel_bufs, perm, chain.cosets)

    def check(cid):
        return ctx.witness_check(cid, [chain.wire_evals], None, None, chain.cosets, cap=16)

    if args.trace_run == "compiled":
        for _ in range(3):
            cid = compile_()
            check(cid)
            ctx.circuit_free(cid)
        ctx.close()
        return
    host_ms, coef = timed(lambda: host_path(ctx, log_n, sel_evals, g))
    if args.trace_run == "loaded":
        for _ in range(3):
            cid = ctx.circuit_load(log_n, coef[:5], coef[5:])
            check(cid)
            ctx.circuit_free(cid)
        ctx.close()
        return

    def load():
        return ctx.circuit_load(log_n, coef[:5], coef[5:])

    t_load, t_compile = [], []
    for r in range(args.warmup + args.reps):
        a, cid = timed(load)
        ctx.circuit_free(cid)
        b, cid = timed(compile_)
        ctx.circuit_free(cid)
        if r >= args.warmup:
            t_load.append(a)
            t_compile.append(b)
    cid = load()
    first_loaded, rep = timed(lambda: check(cid))
    assert rep[0]["gate_failures"] == 0 and rep[0]["copy_failures"] == 0
    ctx.circuit_free(cid)
    cid = compile_()
    first_compiled, rep = timed(lambda: check(cid))
    assert rep[0]["gate_failures"] == 0 and rep[0]["copy_failures"] == 0
    ctx.circuit_free(cid)
    rec = {"log_n": log_n, "reps": args.reps, "host_path_ms": round(host_ms, 1),
           "load_ms": round(statistics.median(t_load), 3), "load_best_ms": round(min(t_load), 3),
           "compile_ms": round(statistics.median(t_compile), 3), "compile_best_ms": round(min(t_compile), 3),
           "first_check_loaded_ms": round(first_loaded, 3), "first_check_compiled_ms": round(first_compiled, 3)}
    line = json.dumps(rec)
    print(line, flush=True)
    for b in sel_bufs + coef:
        b.free()
    chain.free()
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("# python tools/circuit_compile_time.py " + " ".join(sys.argv[1:]) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
