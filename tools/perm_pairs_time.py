"""typlonk_circuit_compile_pairs against what a caller did before it (profiles/r19_perm_pairs.txt), in one process on one device,
at --log-n rows (default 16 and 20), for two pair lists over the 3n cells:
  chain    the copy constraints of the squaring chain of typlonk_amd.circuits, as (x, perm[x]) for every cell that moves
  random   a random pairing of all 3n cells: 3n / 2 disjoint pairs
and per list
  pairs_ms    typlonk_circuit_compile_pairs of the five selector evaluation buffers already on the device and the host pair list
              (its 8 * count-byte upload included)
  builder_ms  PermutationBuilder::build of tests/cpp/circuit_host.hpp (the sequential union of cycles every caller wrote by hand),
              compiled -O2 into tools/_ub/libperm_builder.so on this box, from the same pair list to the 3n-entry map
  compile_ms  typlonk_circuit_compile of that map (its 12n-byte upload included)
  host_path_ms = builder_ms + compile_ms, call by call
The two paths are alternated call by call; median (best) of --reps after --warmup.  Wall time on the host around the blocking
calls; every circuit is freed again outside the timed region.  `--trace-run` makes three compiles from the `random` list at the
first --log-n and nothing else, for a `rocprofv3 --kernel-trace --stats` run of its own.

    python tools/perm_pairs_time.py [--log-n 16 20] [--reps 10] [--warmup 2] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/perm_pairs_time.py --log-n 20 --trace-run
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from circuit_compile_time import chain_permutation, timed  # noqa: E402


def builder_shim():
    """tools/_ub/libperm_builder.so: tools/perm_builder_shim.cpp, PermutationBuilder<3>::build behind a C entry point"""
    d = os.path.join(ROOT, "tools", "_ub")
    os.makedirs(d, exist_ok=True)
    src, out = os.path.join(ROOT, "tools", "perm_builder_shim.cpp"), os.path.join(d, "libperm_builder.so")
    hdr = os.path.join(ROOT, "tests", "cpp", "circuit_host.hpp")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        lib = os.path.join(ROOT, "typlonk_amd")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", out, "-L", lib, "-ltyplonk_hip",
                        "-Wl,-rpath," + lib], check=True)
    so = C.CDLL(out)
    so.perm_builder_build.argtypes = [C.POINTER(C.c_uint32), C.c_size_t, C.c_uint32, C.POINTER(C.c_uint32)]
    return so


def pair_lists(n: int, g: int):
    perm = chain_permutation(n, g)
    x = np.nonzero(perm != np.arange(3 * n, dtype=np.uint32))[0].astype(np.uint32)
    chain = np.ascontiguousarray(np.stack([x, perm[x]], axis=1))
    cells = np.random.default_rng(19).permutation(3 * n).astype(np.uint32)
    return {"chain": chain, "random": np.ascontiguousarray(cells[: 3 * n // 2 * 2].reshape(-1, 2))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()

    import typlonk_amd
    from typlonk_amd.circuits import SquaringChain

    ctx = typlonk_amd.Context(0)
    so = None if args.trace_run else builder_shim()   # (after the library is loaded: the shim names it as a dependency)
    lines = []
    for log_n in args.log_n:
        chain = SquaringChain(ctx, log_n, keep_host=True)
        n, g = chain.n, chain.gates
        sel_bufs = []
        for ev in chain.host_inputs()["selectors"]:
            b = ctx.alloc(n)
            b.upload(ev)
            sel_bufs.append(b)
        lists = pair_lists(n, g)
        if args.trace_run:
            for _ in range(3):
                cid, _ = ctx.circuit_compile_pairs(log_n, sel_bufs, lists["random"], chain.cosets)
                ctx.circuit_free(cid)
            ctx.close()
            return
        for name, pairs in lists.items():
            perm = np.empty(3 * n, dtype=np.uint32)
            u32p = C.POINTER(C.c_uint32)

            def build():
                assert so.perm_builder_build(pairs.ctypes.data_as(u32p), pairs.shape[0], log_n, perm.ctypes.data_as(u32p)) == 0

            t_pairs, t_build, t_compile = [], [], []
            classes = None
            for r in range(args.warmup + args.reps):
                a, (cid, classes) = timed(lambda: ctx.circuit_compile_pairs(log_n, sel_bufs, pairs, chain.cosets))
                ctx.circuit_free(cid)
                b, _ = timed(build)
                c, cid = timed(lambda: ctx.circuit_compile(log_n, sel_bufs, perm, chain.cosets))
                ctx.circuit_free(cid)
                if r >= args.warmup:
                    t_pairs.append(a)
                    t_build.append(b)
                    t_compile.append(c)
            # the same partition either way
            canon, classes2 = ctx.permutation_from_pairs(log_n, np.stack([np.arange(3 * n, dtype=np.uint32), perm], axis=1))
            assert classes2 == classes and np.array_equal(canon, ctx.permutation_from_pairs(log_n, pairs)[0])
            host = [x + y for x, y in zip(t_build, t_compile)]
            med = statistics.median
            rec = {"log_n": log_n, "pairs": name, "count": int(pairs.shape[0]), "classes": classes, "reps": args.reps,
                   "pairs_ms": round(med(t_pairs), 3), "pairs_best_ms": round(min(t_pairs), 3),
                   "builder_ms": round(med(t_build), 3), "compile_ms": round(med(t_compile), 3),
                   "host_path_ms": round(med(host), 3), "host_path_best_ms": round(min(host), 3)}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        for b in sel_bufs:
            b.free()
        chain.free()
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("# python tools/perm_pairs_time.py " + " ".join(sys.argv[1:]) + "\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
