"""Worker of tests/test_gpu_dist_compact.py -- one FRESH process per rank, no torch: the compact proof shape on an SRS shard
(typlonk_prove_compact / _host, typlonk_circuit_vk, typlonk_circuit_commitments as collectives) with world > 1, all ranks on
GPU 0, the all-gather carried by the test-only stand-in tests/cpp/libfake_rccl.so (TYPLONK_RCCL_LIB).
usage: dist_compact_worker.py <rank> <world> <scratch dir> <log_n>
  TABLES   "0" none, "1" the library's own choice where the shard is long enough (typlonk_srs_precompute(0))
  SRS      "generate" (each rank its slice) or "bytes" (its slice of <dir>/srs.bin, a compressed SRS; rank 0's holds P0)
  STEPS    comma list of: staging, equal, unsat, fail, cache   (every rank runs the same list in the same order)
  PI_LENS  comma list of public-input lengths of the `equal` step, "n" = the row count
Writes <dir>/rank<r>.json.  The parent (which also imports the witness helpers below) compares every rank's results with
one context holding the whole SRS, byte for byte."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import typlonk_amd  # noqa: E402
from typlonk_amd.capi import (ERR_UNSATISFIED, G1_BYTES, TyplonkError, comm_unique_id, compact_struct, proof_to_bytes,  # noqa: E402
                              vk_to_bytes)
from typlonk_amd.circuits import FR_MODULUS, SquaringChain, _canon_limbs, _to_montgomery, fr_mont_limbs  # noqa: E402

SECRET = 0x5EC2E7D00D51
R = FR_MODULUS


def pi_values(n, length, seed):
    """`length` public values; rows n - 3 .. (the blinding rows, no gate) are zero"""
    rng = np.random.default_rng(seed)
    vals = [int(v) for v in rng.integers(1, 1 << 60, size=min(length, n - 3))]
    return vals + [0] * (length - len(vals))


def pi_lens(spec, n):
    return [n if s == "n" else int(s) for s in spec.split(",") if s]


class Witness:
    """the squaring chain under public values pi (x_{j+1} = x_j^2 + pi_j) with blinders of `variant`, as device columns; a
    device buffer of the public values (None when there are none); break_row: one gate row that no longer holds"""

    def __init__(self, ctx, log_n, pi=(), variant=1, break_row=None):
        n = 1 << log_n
        g = n - 3
        x = 3
        xs = [x]
        for j in range(g):
            x = (x * x + (pi[j] if j < len(pi) else 0)) % R
            xs.append(x)
        bl = [[(variant * 1000003 + 17 * i + k) % R for k in range(3)] for i in range(3)]
        cols = [xs[:g] + bl[0], xs[:g] + bl[1], xs[1:g + 1] + bl[2]]
        if break_row is not None:
            cols[2][break_row] = (cols[2][break_row] + 1) % R
        self.ctx, self.n, self.pi_len = ctx, n, len(pi)
        self.bufs = [_to_montgomery(ctx, _canon_limbs(c)) for c in cols]
        self.pib = _to_montgomery(ctx, _canon_limbs(pi)) if len(pi) else None

    def host(self):
        return [b.download() for b in self.bufs], (self.pib.download() if self.pib is not None else None)

    def free(self):
        for b in self.bufs + ([self.pib] if self.pib is not None else []):
            b.free()


def proof_hex(d):
    """every field of a compact proof (the struct's bytes: 9 points, 7 evaluations, 5 challenges) and its 656 wire bytes"""
    return {"struct": bytes(compact_struct(d)).hex(), "wire": proof_to_bytes(d).hex()}


def attempt(fn):
    """("ok", proof) | (code, message, proof of an unsatisfied witness or None)"""
    try:
        return ["ok", proof_hex(fn())]
    except TyplonkError as e:
        return [e.code, str(e), proof_hex(e.proof) if e.code == ERR_UNSATISFIED else None]


def main():
    rank, world, d, log_n = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4])
    steps = [s for s in os.environ.get("STEPS", "equal").split(",") if s]
    n = 1 << log_n
    total = n + 3
    ctx = typlonk_amd.Context(0)
    uid_path = os.path.join(d, "uid.bin")
    if rank == 0:
        uid = comm_unique_id()
        with open(uid_path + ".tmp", "wb") as f:
            f.write(uid)
        os.rename(uid_path + ".tmp", uid_path)
    else:
        t0 = time.time()
        while not os.path.exists(uid_path):
            if time.time() - t0 > 120:
                raise SystemExit("no unique id from rank 0")
            time.sleep(0.01)
        uid = open(uid_path, "rb").read()
    ctx.comm_init(uid, rank, world)
    out = {"rank": rank, "world": world, "log_n": log_n}

    lo, hi = rank * total // world, (rank + 1) * total // world
    if os.environ.get("SRS", "generate") == "bytes":
        with open(os.path.join(d, "srs.bin"), "rb") as f:
            f.seek(lo * G1_BYTES)
            sid = ctx.srs_load_compressed(f.read((hi - lo) * G1_BYTES))
    else:
        sid = ctx.srs_generate(fr_mont_limbs(SECRET), hi - lo, start=lo)
    ctx.srs_set_shard(sid, lo, total)
    if os.environ.get("TABLES") == "1":
        ctx.srs_precompute(sid, 0)           # the library's own choice; nothing below 2^14 points
    g2s = np.load(os.path.join(d, "g2s.npy"))
    chain = SquaringChain(ctx, log_n)
    cosets = chain.cosets
    plain = Witness(ctx, log_n)

    def prove(w, circuit=None, bufs=None, pi_len=None):
        return ctx.prove_compact(sid, chain.circuit if circuit is None else circuit, w.bufs if bufs is None else bufs, w.pib,
                                 w.pi_len if pi_len is None else pi_len, cosets)

    for step in steps:
        if step == "staging":
            # the LAST rank's first fold of the process loses its staging copy (TYPLONK_TEST_COMM_FAIL_STAGING=1 there): the
            # first fold of a proof, with its 12 records
            out["staging"] = attempt(lambda: prove(plain))
            out["staging_next"] = attempt(lambda: prove(plain))
        elif step == "equal":
            fresh = SquaringChain(ctx, log_n)            # a circuit whose commitments no rank has cached
            res = []
            for k, pl in enumerate(pi_lens(os.environ.get("PI_LENS", "0,1,n"), n)):
                w = Witness(ctx, log_n, pi_values(n, pl, 100 * log_n + k), variant=k + 1)
                cols, pic = w.host()
                res.append({"pi_len": pl, "dev": attempt(lambda: prove(w, fresh.circuit)),
                            "host": attempt(lambda: ctx.prove_compact_host(sid, fresh.circuit, cols, pic, cosets))})
                w.free()
            out["equal"] = res
            out["equal_cached"] = attempt(lambda: prove(plain, fresh.circuit))
            out["vk"] = vk_to_bytes(ctx.circuit_vk(sid, fresh.circuit, cosets, g2s)).hex()
            out["commitments"] = [[[int(v) for v in xy], int(f)] for xy, f in ctx.circuit_commitments(sid, fresh.circuit)]
            another = SquaringChain(ctx, log_n)          # the key FIRST, uncached: its own eight MSMs, then the proof on the cache
            out["vk_uncached"] = vk_to_bytes(ctx.circuit_vk(sid, another.circuit, cosets, g2s)).hex()
            out["after_vk"] = attempt(lambda: prove(plain, another.circuit))
            another.free()
            fresh.free()
        elif step == "unsat":
            bad = Witness(ctx, log_n, break_row=(n - 3) // 2)
            out["unsat"] = attempt(lambda: prove(bad))
            out["unsat_next"] = attempt(lambda: prove(plain))
            bad.free()
        elif step == "fail":
            short = ctx.alloc(n - 1)                     # a wire buffer shorter than n, on rank 1
            one = ctx.alloc(1)
            one.zero()
            out["short_wire"] = attempt(lambda: prove(plain, bufs=[plain.bufs[0], short, plain.bufs[2]] if rank == 1 else None))
            out["short_wire_next"] = attempt(lambda: prove(plain))
            # pi_len > n on rank 1
            out["pi_long"] = attempt(lambda: ctx.prove_compact(sid, chain.circuit, plain.bufs, one, n + 1, cosets) if rank == 1
                                     else prove(plain))
            out["pi_long_next"] = attempt(lambda: prove(plain))
            # an unknown circuit on rank 1 inside the key's collective, then the key
            try:
                ctx.circuit_vk(sid, 0x7FFFFFF0 if rank == 1 else chain.circuit, cosets, g2s)
                out["vk_fail"] = ["ok"]
            except TyplonkError as e:
                out["vk_fail"] = [e.code, str(e)]
            out["vk_fail_next"] = vk_to_bytes(ctx.circuit_vk(sid, chain.circuit, cosets, g2s)).hex()
            short.free()
            one.free()
        elif step == "cache":
            # what the fixed record counts exist for: ranks whose caches differ while a peer refuses its arguments
            short = ctx.alloc(n - 1)
            bad_bufs = [plain.bufs[0], short, plain.bufs[2]]
            b = SquaringChain(ctx, log_n)                # nobody cached; rank 1 refuses: every OTHER rank caches its sums
            out["cache_a1"] = attempt(lambda: prove(plain, b.circuit, bufs=bad_bufs if rank == 1 else None))
            out["cache_a2"] = attempt(lambda: prove(plain, b.circuit))     # rank 1 uncached, its peers cached
            c = SquaringChain(ctx, log_n)                # every rank BUT rank 1 refuses: only rank 1 caches
            out["cache_b1"] = attempt(lambda: prove(plain, c.circuit, bufs=bad_bufs if rank != 1 else None))
            out["cache_b2"] = attempt(lambda: prove(plain, c.circuit, bufs=bad_bufs if rank == 0 else None))   # cached rank 1, rank 0 refuses
            out["cache_b3"] = attempt(lambda: prove(plain, c.circuit))     # rank 1 cached, its peers not (all but rank 0 since b2)
            b.free()
            c.free()
            short.free()
        else:
            raise SystemExit(f"unknown step {step}")
    plain.free()
    chain.free()
    ctx.comm_destroy()
    ctx.close()
    with open(os.path.join(d, f"rank{rank}.json"), "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
