"""Verifier measurement (profiles/r08_verify.txt): typlonk_verify per call and per proof, split into host checks, sigma / PI
evaluation, the fold's two MSMs and the host pairing product, beside the C++ mirror's CompiledCircuit::verify of one proof
of the same circuit (tests/cpp/test_verify_host bench); then the poly-eval kernel's rate in Fr multiply-adds per second next
to the NTT's butterfly rate.  Wall times on the host; kernel times come from a separate rocprofv3 --kernel-trace --stats run.

    python tools/verify_bench.py [--log-n 16 20 22] [--counts 1 8 64 256]
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def poly_eval_rate(log_m: int = 20, count: int = 2, points: int = 256):
    import numpy as np

    import typlonk_amd

    ctx = typlonk_amd.Context(0)
    m = 1 << log_m
    rng = np.random.default_rng(7)
    polys = []
    for _ in range(count):
        a = rng.integers(0, 1 << 62, size=(m, 4), dtype=np.uint64)
        b = ctx.alloc(m)
        b.upload(a)
        polys.append(b)
    pts = rng.integers(0, 1 << 62, size=(points, 4), dtype=np.uint64)
    ctx.poly_eval_dev(polys, m, pts)   # warm: workspace
    reps = 5
    t0 = time.perf_counter()
    for _ in range(reps):
        ctx.poly_eval_dev(polys, m, pts)
    dt = (time.perf_counter() - t0) / reps
    fma = count * points * m
    # NTT of the same length: n/2 log n butterflies, one Fr multiplication each
    buf = polys[0]
    ctx.ntt_dev(buf, log_m)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        ctx.ntt_dev(buf, log_m)
    ctx.sync()
    dn = (time.perf_counter() - t0) / reps
    muls = (m // 2) * log_m
    for b in polys:
        b.free()
    ctx.close()
    return dt, fma, dn, muls


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[16, 20, 22])
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 8, 64, 256])
    args = ap.parse_args()
    exe = os.path.join(ROOT, "tests", "cpp", "test_verify_host")
    print("# typlonk_verify (verify_batch of the C++ mirror) vs CompiledCircuit::verify, squaring chain, MI355X")
    print("# batches repeat 16 distinct valid proofs; best of 2 calls; split = host wall ms per stage (typlonk_profile_get)")
    for log_n in args.log_n:
        r = subprocess.run([exe, "bench", str(log_n)] + [str(c) for c in args.counts], capture_output=True, text=True, timeout=1800)
        sys.stdout.write(r.stdout)
        if r.returncode:
            sys.stdout.write(r.stderr[-2000:])
            sys.exit(r.returncode)
        sys.stdout.flush()
    dt, fma, dn, muls = poly_eval_rate()
    print(f"POLY_EVAL m=2^20 polys=2 points=256 ms={dt * 1e3:.2f} rate={fma / dt / 1e9:.2f} G Fr-muladd/s")
    print(f"NTT       n=2^20 forward           ms={dn * 1e3:.2f} rate={muls / dn / 1e9:.2f} G Fr-mul/s (butterflies)")


if __name__ == "__main__":
    main()
