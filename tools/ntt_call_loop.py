"""Host time per transform call (profiles/r22_ab_ntt_plan.txt): CALLS typlonk_ntt_fr_devptr calls queued back to back and ONE
stream synchronisation behind them, per size (SIZES, default 12,16,20) forward and inverse on the coset 7; the best and the
median of REPS such loops, in microseconds per call -- the longer of the host's and the device's time per call.  enqueue_us:
the host side alone, the best of REPS bursts of 200 calls timed up to the return of the last call (the queue takes them
without waiting).  TYPLONK_LIB_PATH selects another build of the library for a same-box comparison."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch, typlonk_amd
from bench import synthetic_scalars, fr_mont_limbs

ctx = typlonk_amd.Context(0)
dev = torch.device("cuda", 0)
g = fr_mont_limbs(7)
calls, reps = int(os.environ.get("CALLS", "3000")), int(os.environ.get("REPS", "5"))
out = {}
for log_n in [int(x) for x in os.environ.get("SIZES", "12,16,20").split(",")]:
    x = synthetic_scalars(1 << log_n, 3, dev)
    for name, inverse, coset in (("fwd", False, None), ("inv_coset", True, g)):
        for _ in range(50):
            ctx.ntt_devptr(x.data_ptr(), log_n, inverse, coset)
        torch.cuda.synchronize()
        us = []
        for _ in range(reps):
            t = time.perf_counter()
            for _ in range(calls):
                ctx.ntt_devptr(x.data_ptr(), log_n, inverse, coset)
            torch.cuda.synchronize()
            us.append((time.perf_counter() - t) / calls * 1e6)
        enq = []
        for _ in range(reps):
            t = time.perf_counter()
            for _ in range(200):
                ctx.ntt_devptr(x.data_ptr(), log_n, inverse, coset)
            enq.append((time.perf_counter() - t) / 200 * 1e6)
            torch.cuda.synchronize()
        out[f"2^{log_n} {name}"] = {"best_us": round(min(us), 3), "median_us": round(statistics.median(us), 3), "enqueue_us": round(min(enq), 3)}
print("NTT_CALL_LOOP " + json.dumps(out), flush=True)
ctx.close()
