"""Launch parity of two builds of the library (profiles/r21_msm_plan_launch_parity.txt, profiles/r22_ntt_plan_launch_parity.txt,
profiles/r24_prove_plan_launch_parity.txt):
the same work under `rocprofv3 --kernel-trace` with each build, then the ordered kernel name, grid, workgroup size and LDS
bytes compared per stream.

    rocprofv3 --kernel-trace --output-format csv -d DIR_A -- python3 tools/msm_launch_parity.py run [ntt | prove]   (TYPLONK_LIB_PATH: build A)
    rocprofv3 --kernel-trace --output-format csv -d DIR_B -- python3 tools/msm_launch_parity.py run [ntt | prove]
    python tools/msm_launch_parity.py compare DIR_A DIR_B [OUT]

run: one MSM at 2^14 terms over a plain SRS, 2^17 with c = 17 tables, 2^20 with c = 20 tables from device and from host
scalars, and 2^21 with c = 20 tables queued in a batch of three.
run ntt: single transforms at 2^10, 2^16, 2^20 and 2^22 in both directions, transforms on the coset 7 at 2^20 and 2^22, a
group of three at 2^20, and one proof of the squaring chain at 2^16.
run prove: on one context, the squaring chain at 2^12 through typlonk_prove, typlonk_prove_compact, typlonk_prove_batch and
typlonk_prove_batch_compact of three, and the round-by-round session with batched openings; then typlonk_prove at 2^3."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run():
    import numpy as np
    import typlonk_amd

    ctx = typlonk_amd.Context(0)
    two = np.array([2, 0, 0, 0], dtype=np.uint64)   # any secret: the launches do not depend on it
    rng = np.random.default_rng(21)
    for log_m, window, how in ((14, 0, "dev"), (17, 17, "dev"), (20, 20, "dev host"), (21, 20, "batch")):
        m = 1 << log_m
        sc = rng.integers(0, 1 << 62, size=(m, 4), dtype=np.uint64)
        sid = ctx.srs_generate(two, m)
        if window:
            ctx.srs_precompute(sid, window)
        buf = ctx.alloc(m)
        buf.upload(sc)
        if "dev" in how:
            ctx.msm_devptr(sid, buf.devptr, m)
        if "host" in how:
            ctx.msm(sid, sc)
        if "batch" in how:
            ctx.msm_batch_devptr(sid, [buf.devptr] * 3, [m, m, m])
        buf.free()
        ctx.srs_free(sid)
        print(f"PARITY_RUN 2^{log_m} window {window} {how}: done", flush=True)
    ctx.close()


def run_ntt():
    import numpy as np
    import typlonk_amd
    from bench import fr_mont_limbs
    from typlonk_amd.circuits import SquaringChain

    ctx = typlonk_amd.Context(0)
    g = fr_mont_limbs(7)
    rng = np.random.default_rng(22)
    for log_n in (10, 16, 20, 22):
        n = 1 << log_n
        count = 3 if log_n == 20 else 1
        buf = ctx.alloc(n * count)
        buf.upload(rng.integers(0, 1 << 62, size=(n * count, 4), dtype=np.uint64))   # any values: the launches do not depend on them
        for inverse in (False, True):
            ctx.ntt_devptr(buf.devptr, log_n, inverse, None)
            if log_n >= 20:
                ctx.ntt_devptr(buf.devptr, log_n, inverse, g)
        if count > 1:
            ctx.ntt_batch_devptr([buf.devptr + 32 * n * v for v in range(count)], log_n)
        buf.download()
        buf.free()
        print(f"PARITY_RUN ntt 2^{log_n}: done", flush=True)
    sid = ctx.srs_generate(fr_mont_limbs(2), (1 << 16) + 3)
    chain = SquaringChain(ctx, 16)
    ctx.prove_native(sid, chain.circuit, chain.wire_evals, chain.pi_evals, chain.cosets)
    print("PARITY_RUN proof 2^16: done", flush=True)
    ctx.close()


def run_prove():
    import typlonk_amd
    from bench import fr_mont_limbs
    from typlonk_amd.circuits import SquaringChain

    ctx = typlonk_amd.Context(0)
    for log_n in (12, 3):
        sid = ctx.srs_generate(fr_mont_limbs(2), (1 << log_n) + 3)
        chain = SquaringChain(ctx, log_n)
        w, cosets = chain.wire_evals, chain.cosets
        ctx.prove_native(sid, chain.circuit, w, None, cosets)
        if log_n == 12:
            ctx.prove_compact(sid, chain.circuit, w, None, 0, cosets)
            ctx.prove_batch(sid, chain.circuit, [w] * 3, None, cosets)
            ctx.prove_batch_compact(sid, chain.circuit, [w] * 3, None, None, cosets)
            ctx.prove(sid, chain.circuit, w, None, cosets, challenge_v=lambda evals: fr_mont_limbs(5))
        print(f"PARITY_RUN prove 2^{log_n}: done", flush=True)
    ctx.close()


def launches(directory):
    """{stream (numbered by first appearance): [(kernel, grid, workgroup, lds)] in dispatch order}, and the column that told streams apart"""
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {directory}")
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            rows += list(csv.DictReader(fh))
    key = "Stream_Id" if "Stream_Id" in rows[0] else "Queue_Id"
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    streams, order = {}, {}
    for r in rows:
        sid = order.setdefault(r[key], len(order))
        streams.setdefault(sid, []).append((r["Kernel_Name"].split("(")[0],
                                            tuple(int(r["Grid_Size_" + a]) for a in "XYZ"),
                                            tuple(int(r["Workgroup_Size_" + a]) for a in "XYZ"),
                                            int(r["LDS_Block_Size"])))
    return streams, key, len(rows)


def compare(dir_a, dir_b, out=None):
    a, key_a, na = launches(dir_a)
    b, key_b, nb = launches(dir_b)
    lines = [f"A: {na} kernel launches on {len(a)} streams ({key_a}); B: {nb} on {len(b)} ({key_b})"]
    same = key_a == key_b and sorted(a) == sorted(b)
    moved = False   # only the runtime's own copy kernels (uploads from pageable memory) sit elsewhere among the library's kernels

    def own(launch_list, runtime):
        return [x for x in launch_list if x[0].startswith("__amd_rocclr_") == runtime]

    for s in sorted(set(a) | set(b)):
        la, lb = a.get(s, []), b.get(s, [])
        if la == lb:
            lines.append(f"stream {s}: {len(la)} launches, identical")
            continue
        if own(la, False) == own(lb, False) and own(la, True) == own(lb, True):
            moved = True
            lines.append(f"stream {s}: the {len(own(la, False))} launches of the library's kernels identical and in the same order; the "
                         f"{len(own(la, True))} copy kernels of the runtime identical and in the same order among themselves, but placed "
                         "differently between the library's:")
        else:
            same = False
            lines.append(f"stream {s}: DIFFERENT ({len(la)} against {len(lb)} launches)")
        for i in range(max(len(la), len(lb))):
            x, y = (la[i] if i < len(la) else None), (lb[i] if i < len(lb) else None)
            if x != y:
                lines.append(f"  launch {i}: A {x}\n  {' ' * len(str(i))}         B {y}")
    lines.append("VERDICT: the launch lists differ" if not same else
                 "VERDICT: the ordered (kernel, grid, workgroup size, LDS bytes) lists of the library's kernels are identical per stream; "
                 "copy kernels of the runtime are placed differently" if moved else
                 "VERDICT: the ordered (kernel, grid, workgroup size, LDS bytes) lists are identical per stream")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out:
        with open(out, "w") as f:
            f.write(text)
    return (2 if moved else 0) if same else 1


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        {"ntt": run_ntt, "prove": run_prove}.get((sys.argv[2:3] or [""])[0], run)()
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else None))
    else:
        sys.exit(__doc__)
