"""A fixed number of NATIVE proofs (typlonk_prove: the library's own transcript between the rounds, no Python in between) on the
squaring-chain circuit, for rocprofv3 kernel traces.  HOST=1: typlonk_prove_host (columns in host memory).
SHAPE=compact: typlonk_prove_compact / typlonk_prove_compact_host instead (no public values)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch, typlonk_amd
from typlonk_amd.circuits import SquaringChain
from bench import fr_mont_limbs

log_n = int(os.environ.get("LOG_N", "20"))
n = 1 << log_n
ctx = typlonk_amd.Context(0)
t0 = time.perf_counter()
sid = ctx.srs_generate(fr_mont_limbs(2), n + 3)
t1 = time.perf_counter()
ctx.srs_precompute(sid, 20)
t2 = time.perf_counter()
load_s = []   # typlonk_circuit_load alone (it returns once the coset transforms are done), inside the chain's set-up
_load = ctx.circuit_load
def _timed_load(*a):
    t = time.perf_counter()
    r = _load(*a)
    load_s.append(time.perf_counter() - t)
    return r
ctx.circuit_load = _timed_load
chain = SquaringChain(ctx, log_n)
t3 = time.perf_counter()
print(f"setup log_n={log_n}: srs_generate {(t1 - t0) * 1e3:.0f} ms ({n + 3} points), srs_precompute(c=20) {(t2 - t1) * 1e3:.0f} ms, "
      f"circuit_load {sum(load_s) * 1e3:.0f} ms (squaring chain with witness {(t3 - t2) * 1e3:.0f} ms)", flush=True)
host = os.environ.get("HOST", "0") == "1"
cols = [b.download() for b in chain.wire_evals] if host else None
run = (lambda: ctx.prove_native_host(sid, chain.circuit, cols, None, chain.cosets)) if host else \
      (lambda: ctx.prove_native(sid, chain.circuit, chain.wire_evals, chain.pi_evals, chain.cosets))
shape = os.environ.get("SHAPE", "reference")
if shape == "compact":
    run = (lambda: ctx.prove_compact_host(sid, chain.circuit, cols, None, chain.cosets)) if host else \
          (lambda: ctx.prove_compact(sid, chain.circuit, chain.wire_evals, None, 0, chain.cosets))
    run()      # the circuit commitments for the statement digest: once per (circuit, SRS)
run()
torch.cuda.synchronize()
reps = int(os.environ.get("REPS", "5"))
gap = float(os.environ.get("GAP_MS", "0")) * 1e-3
tot = 0.0
for _ in range(reps):
    t0 = time.perf_counter()
    run()
    tot += time.perf_counter() - t0
    if gap:
        torch.cuda.synchronize()
        time.sleep(gap)
print(f"prove_native log_n={log_n} host={host} shape={shape}: {tot / reps * 1e3:.2f} ms per proof", flush=True)
