"""Compact proof shape measurement (profiles/r10_compact.txt), in one process with the two shapes alternated call by call so
that both see the same clocks:
  - typlonk_prove vs typlonk_prove_compact (columns on the device) at each --log-n
  - typlonk_prove_host vs typlonk_prove_compact_host at --host-log-n
  - typlonk_verify (TYPLONK_VERIFY_PI_AS_PROVER) vs typlonk_verify_compact for --counts proofs at each --verify-log-n, with the
    stage split of one extra call (typlonk_profile_get: host checks, evaluations, the fold's MSMs, the host pairing, folds)
Squaring chain (typlonk_amd.circuits), SRS with fixed-base tables (typlonk_srs_precompute), no public inputs.  Wall time on
the host per call: median (and best) of --reps after --warmup calls; verify batches repeat 16 distinct valid proofs.

    python tools/compact_bench.py [--log-n 16 20 22] [--host-log-n 20] [--verify-log-n 16 22] [--counts 1 64 256]
                                  [--reps 10] [--warmup 3] [--out profiles/r10_compact.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SECRET = 0x5EC2E7D00D51


def alternate(fns, reps: int, warmup: int):
    """call every fn in turn, warmup + reps rounds; per fn: (median ms, best ms)"""
    times = [[] for _ in fns]
    for r in range(warmup + reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= warmup:
                times[i].append(dt)
    return [(statistics.median(t), min(t)) for t in times]


class Setup:
    def __init__(self, ctx, log_n):
        import numpy as np

        from typlonk_amd.circuits import SquaringChain, fr_mont_limbs
        from oracle import pairing as PR
        from oracle import bls12_381 as O

        self.ctx, self.log_n, self.n = ctx, log_n, 1 << log_n
        self.chain = SquaringChain(ctx, log_n)
        self.sid = ctx.srs_generate(fr_mont_limbs(SECRET), self.n + 3)
        ctx.srs_precompute(self.sid)
        (x0, x1), (y0, y1) = PR.srs_g2(SECRET)[1]
        self.g2s = np.array([lb for c in (x0, x1, y0, y1) for lb in O.fq_to_mont_limbs(c)], dtype=np.uint64)
        self.vk = ctx.circuit_vk(self.sid, self.chain.circuit, self.chain.cosets, self.g2s)

    def prove(self):
        return self.ctx.prove_native(self.sid, self.chain.circuit, self.chain.wire_evals, None, self.chain.cosets)

    def prove_compact(self):
        return self.ctx.prove_compact(self.sid, self.chain.circuit, self.chain.wire_evals, None, 0, self.chain.cosets)

    def distinct(self, k, compact):
        """k proofs with other blinding rows"""
        from helpers import fr_pack

        host = [b.download() for b in self.chain.wire_evals]
        out = []
        for v in range(k):
            cols = [c.copy() for c in host]
            for i in range(3):
                cols[i][self.n - 3:] = fr_pack([(v * 1000003 + 17 * i + j + 1) for j in range(3)])
            if compact:
                out.append(self.ctx.prove_compact_host(self.sid, self.chain.circuit, cols, None, self.chain.cosets))
            else:
                out.append(self.ctx.prove_native_host(self.sid, self.chain.circuit, cols, None, self.chain.cosets))
        return out

    def free(self):
        self.chain.free()
        self.ctx.srs_free(self.sid)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[16, 20, 22])
    ap.add_argument("--host-log-n", type=int, nargs="*", default=[20])
    ap.add_argument("--verify-log-n", type=int, nargs="*", default=[16, 22])
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 64, 256])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import typlonk_amd

    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    ctx = typlonk_amd.Context(0)
    emit("# compact vs reference proof shape, squaring chain, SRS with fixed-base tables, MI355X; one process, alternated")
    emit(f"# wall ms per call: median (best) of {args.reps} after {args.warmup} warm-up calls")
    sizes = sorted(set(args.log_n) | set(args.host_log_n) | set(args.verify_log_n))
    for log_n in sizes:
        s = Setup(ctx, log_n)
        if log_n in args.log_n:
            (m0, b0), (m1, b1) = alternate([s.prove, s.prove_compact], args.reps, args.warmup)
            emit(f"PROVE        2^{log_n:<2}  typlonk_prove {m0:8.2f} ({b0:8.2f})  typlonk_prove_compact {m1:8.2f} ({b1:8.2f})"
                 f"  ratio {m1 / m0:.3f}")
        if log_n in args.host_log_n:
            host = [b.download() for b in s.chain.wire_evals]
            f0 = lambda: ctx.prove_native_host(s.sid, s.chain.circuit, host, None, s.chain.cosets)   # noqa: E731
            f1 = lambda: ctx.prove_compact_host(s.sid, s.chain.circuit, host, None, s.chain.cosets)  # noqa: E731
            (m0, b0), (m1, b1) = alternate([f0, f1], args.reps, args.warmup)
            emit(f"PROVE_HOST   2^{log_n:<2}  typlonk_prove_host {m0:8.2f} ({b0:8.2f})  typlonk_prove_compact_host {m1:8.2f}"
                 f" ({b1:8.2f})  ratio {m1 / m0:.3f}")
        if log_n in args.verify_log_n:
            ref = s.distinct(16, compact=False)
            cmp_ = s.distinct(16, compact=True)
            for k in args.counts:
                pr = [ref[i % 16] for i in range(k)]
                pc = [cmp_[i % 16] for i in range(k)]
                f0 = lambda: ctx.verify(s.sid, s.chain.circuit, s.g2s, s.chain.cosets, pr, pi_as_prover=True)   # noqa: E731
                f1 = lambda: ctx.verify_compact(s.vk, pc)   # noqa: E731
                assert f0().all() and f1().all()
                (m0, b0), (m1, b1) = alternate([f0, f1], args.reps, args.warmup)
                split = []
                for f in (f0, f1):
                    ctx.set_profiling(1)
                    f()
                    split.append(" ".join(f"{name[7:]}={ms:.2f}" for name, ms in ctx.profile()))
                    ctx.set_profiling(0)
                emit(f"VERIFY       2^{log_n:<2}  K={k:<4} typlonk_verify {m0:8.2f} ({b0:8.2f})  typlonk_verify_compact {m1:8.2f}"
                     f" ({b1:8.2f})  ratio {m1 / m0:.3f}")
                emit(f"  split verify:         {split[0]}")
                emit(f"  split verify_compact: {split[1]}")
        s.free()
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
