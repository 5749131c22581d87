"""Wire-format measurement (profiles/r13_point_codec.txt), in one process with the compared calls alternated so that all see the
same clocks:
  - typlonk_srs_load_compressed with and without the subgroup check, typlonk_srs_load of the same points uncompressed
    (96 bytes per point over PCIe instead of 48, no decoding), typlonk_srs_generate and typlonk_srs_download_compressed,
    each at 2^--srs-log-n points
  - typlonk_verify_compact_bytes against typlonk_verify_compact on structs for --counts proofs at 2^--verify-log-n, and the
    decode alone (typlonk_proof_compact_from_bytes on the device and on the host)
Wall time on the host per call, every call ending in a device synchronise: median (and best; for the SRS calls best .. worst)
of --reps after --warmup calls.
Kernel time alone comes from runs of this tool with --kernel-only check / skip under `rocprofv3 --kernel-trace --stats`.

    python tools/point_codec_bench.py [--srs-log-n 20] [--verify-log-n 16] [--counts 1 64 256] [--reps 10] [--warmup 3]
                                      [--kernel-only check|skip] [--out profiles/r13_point_codec.txt]
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from compact_bench import SECRET, Setup, alternate  # noqa: E402


def alternate_spread(fns, reps: int, warmup: int):
    """compact_bench.alternate with the worst call as well: per fn (median ms, best ms, worst ms)"""
    import statistics
    import time

    times = [[] for _ in fns]
    for r in range(warmup + reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            if r >= warmup:
                times[i].append((time.perf_counter() - t0) * 1e3)
    return [(statistics.median(t), min(t), max(t)) for t in times]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--srs-log-n", type=int, default=20)
    ap.add_argument("--verify-log-n", type=int, default=16)
    ap.add_argument("--counts", type=int, nargs="*", default=[1, 64, 256])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-only", choices=["check", "skip"], default=None,
                    help="--reps decode launches (with / without the subgroup check) and encode launches, nothing else: for a "
                         "kernel trace, whose min / max columns then are the spread of that one variant")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import typlonk_amd
    from typlonk_amd import capi
    from typlonk_amd.circuits import fr_mont_limbs

    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    ctx = typlonk_amd.Context(0)
    n = 1 << args.srs_log_n
    secret = fr_mont_limbs(SECRET)
    sid = ctx.srs_generate(secret, n)
    data = ctx.srs_download_compressed(sid)
    xy, inf = ctx.srs_download(sid)

    def load(skip):
        ctx.srs_free(ctx.srs_load_compressed(data, skip_subgroup=skip))

    if args.kernel_only:
        for _ in range(args.reps):
            load(args.kernel_only == "skip")
            ctx.srs_download_compressed(sid)
        ctx.close()
        return

    emit("# wire format, MI355X; one process, alternated; wall ms per call: median (best .. worst) for the SRS rows, median (best) "
         f"for the VERIFY rows, of {args.reps} after {args.warmup} warm-up calls")
    fns = [lambda: load(False), lambda: load(True), lambda: ctx.srs_free(ctx.srs_load(xy, inf)),
           lambda: ctx.srs_free(ctx.srs_generate(secret, n)), lambda: ctx.srs_download_compressed(sid)]
    names = ["srs_load_compressed", "srs_load_compressed(skip subgroup)", "srs_load (uncompressed)", "srs_generate",
             "srs_download_compressed"]
    for name, (med, best, worst) in zip(names, alternate_spread(fns, args.reps, args.warmup)):
        emit(f"SRS     2^{args.srs_log_n:<2}  {name:<36} {med:9.2f} ({best:9.2f} .. {worst:9.2f})  {n / med / 1e3:8.2f} M points/s")
    # the same two loads back to back, not alternated with anything (the kernel trace's conditions, without the tracer)
    for name, fn in (("srs_load_compressed", fns[0]), ("srs_load_compressed(skip subgroup)", fns[1])):
        (med, best, worst), = alternate_spread([fn], args.reps, args.warmup)
        emit(f"SRS     2^{args.srs_log_n:<2}  {name + ', back to back':<50} {med:9.2f} ({best:9.2f} .. {worst:9.2f})")
    ctx.srs_free(sid)

    if args.counts:
        s = Setup(ctx, args.verify_log_n)
        distinct = s.distinct(16, compact=True)
        for k in args.counts:
            proofs = [distinct[i % 16] for i in range(k)]
            blob = b"".join(capi.proof_to_bytes(p) for p in proofs)
            # the library calls themselves, on arguments built once (no Python conversion inside the timed window)
            arr = (capi.ProofCompact * k)(*[capi.compact_struct(p) for p in proofs])
            buf = np.frombuffer(blob, dtype=np.uint8)
            ok = np.zeros(k, dtype=np.uint8)
            out = (capi.ProofCompact * k)()
            st = (C.c_uint32 * k)()
            vkp, okp, bufp = C.byref(s.vk), capi._u8p(ok), capi._u8p(buf)
            lib = ctx.lib

            def f0():
                assert lib.typlonk_verify_compact(ctx.h, vkp, arr, k, None, None, okp) == 0
                return ok

            def f1():
                assert lib.typlonk_verify_compact_bytes(ctx.h, vkp, bufp, k, None, None, 0, okp) == 0
                return ok

            f2 = lambda: lib.typlonk_proof_compact_from_bytes(ctx.h, bufp, k, 0, out, st)     # noqa: E731
            f3 = lambda: lib.typlonk_proof_compact_from_bytes(None, bufp, k, 0, out, st)      # noqa: E731
            assert f0().all() and f1().all()
            (m0, b0), (m1, b1), (m2, b2), (m3, b3) = alternate([f0, f1, f2, f3], args.reps, args.warmup)
            emit(f"VERIFY  2^{args.verify_log_n:<2}  K={k:<4} verify_compact {m0:8.2f} ({b0:8.2f})  verify_compact_bytes {m1:8.2f}"
                 f" ({b1:8.2f})  ratio {m1 / m0:.3f}")
            emit(f"                   decode alone: device {m2:8.2f} ({b2:8.2f})  host {m3:8.2f} ({b3:8.2f})"
                 f"  device decode share of verify_compact_bytes {m2 / m1:.3f}")
        s.free()
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
