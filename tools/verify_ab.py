"""Another build of the library (the parent commit's, say) against this tree's, both loaded into one process: the verdicts,
verify_folds and typlonk_circuit_vk bytes must be equal; then the verifiers' time split (Context.profile) with the two
libraries alternated call by call, 64 proofs at 2^12 (all valid, and with five tampered) and one proof at 2^20, in both proof
shapes.  Usage: python tools/verify_ab.py <other libtyplonk_hip.so> <out file>   (AB_REPS: repetitions, default 9)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from typlonk_amd import capi  # noqa: E402

import test_gpu_compact as TC  # noqa: E402
import test_gpu_verify as TV  # noqa: E402

PARENT, OUT = sys.argv[1], sys.argv[2]
REPS = int(os.environ.get("AB_REPS", "9"))
out = open(OUT, "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


ctx_new = capi.Context(0)
capi._lib = None
capi.LIB_PATH = PARENT
ctx_par = capi.Context(0)
assert ctx_new.lib._name != ctx_par.lib._name
say("new   ", ctx_new.lib._name)
say("parent", ctx_par.lib._name)
LIBS = (("parent", ctx_par), ("new", ctx_new))


def profiled(ctx, fn):
    ctx.set_profiling(1)
    try:
        t = time.perf_counter()
        got = fn()
        wall = (time.perf_counter() - t) * 1e3
        prof = dict(ctx.profile())
    finally:
        ctx.set_profiling(0)
    prof["wall"] = wall
    return got, prof


def measure(label, fns):
    """fns: {lib name: callable}; alternated, REPS each, after one warm-up call each"""
    rows = {name: [] for name in fns}
    ref = None
    for name, (ctx, fn) in fns.items():
        got, prof = profiled(ctx, fn)
        if ref is None:
            ref = (got.tolist(), prof["verify_folds"])
        assert (got.tolist(), prof["verify_folds"]) == ref, (label, name, "verdicts / folds differ")
    for _ in range(REPS):
        for name, (ctx, fn) in fns.items():
            rows[name].append(profiled(ctx, fn)[1])
    say(f"{label}: verdicts equal, accepted {sum(ref[0])}/{len(ref[0])}, verify_folds {int(ref[1])} in both")
    verdict = True
    for key in ("wall", "verify_host", "verify_msm", "verify_pairing"):
        p = [r[key] for r in rows["parent"]]
        q = [r[key] for r in rows["new"]]
        inside = min(p) <= statistics.median(q) <= max(p)
        if key != "wall":
            verdict = verdict and inside
        say(f"  {key:15s} parent med {statistics.median(p):9.3f} [{min(p):9.3f} .. {max(p):9.3f}]   "
            f"new med {statistics.median(q):9.3f} [{min(q):9.3f} .. {max(q):9.3f}]   {'inside' if inside else 'OUTSIDE'} (ms)")
    return verdict


def case(log_n, count, bad):
    cn = TV.Chain(ctx_new, log_n)
    cc = TC.Chain(ctx_new, log_n)
    cp = TV.Chain(ctx_par, log_n)
    vk_new = cc.vk
    vk_par = ctx_par.circuit_vk(cp.sid, cp.cid, cp.cosets, TC._g2s())
    same = capi.vk_to_bytes(vk_new) == capi.vk_to_bytes(vk_par)
    say(f"2^{log_n}: typlonk_circuit_vk bytes equal: {same}")
    assert same
    ref = [cn.prove(v) for v in range(count)]
    com = [cc.prove(v) for v in range(count)]
    good = True
    batches = [("valid", ref, com)]
    if bad:
        tr, tc = list(ref), list(com)
        kinds = [("witness", 1), ("t_commit", 2), ("commit", 0), ("witness", 0), ("t_commit", 0)]
        for k, (key, i) in zip(bad, kinds):
            tr[k] = TV._tamper_point(ref[k], key, i)
            tc[k] = TC._tamper_point(com[k], key, i)
        k = bad[1]
        tr[k] = dict(ref[k], evals=[TV._limbs(7)] + ref[k]["evals"][1:])
        tc[k] = dict(com[k], evals=[TC._limbs(7)] + com[k]["evals"][1:])
        batches.append((f"tampered {bad}", tr, tc))
    for name, r, c in batches:
        good &= measure(f"typlonk_verify          {count} x 2^{log_n} {name}",
                        {"parent": (ctx_par, lambda: ctx_par.verify(cp.sid, cp.cid, TV.g2s(), cp.cosets, r)),
                         "new": (ctx_new, lambda: ctx_new.verify(cn.sid, cn.cid, TV.g2s(), cn.cosets, r))})
        good &= measure(f"typlonk_verify_compact  {count} x 2^{log_n} {name}",
                        {"parent": (ctx_par, lambda: ctx_par.verify_compact(vk_par, c)),
                         "new": (ctx_new, lambda: ctx_new.verify_compact(vk_new, c))})
    for c in (cn, cc, cp):
        c.free()
    return good


ok = case(12, 64, (3, 17, 31, 40, 63))
ok &= case(20, 1, ())
say("every new median of verify_host / verify_msm / verify_pairing inside the parent's spread:", ok)
ctx_new.close()
ctx_par.close()
