"""Build recipe for the in-tree native artefacts (gfx950 only).

  typlonk_amd/libtyplonk_hip.so   HIP kernels + C ABI (include/typlonk.h)       -- hipcc
  tests/cpp/hooks/libtyplonk_hip.so  the same library with the fault-injection hook (-DTYPLONK_TEST_HOOKS, tests only) -- hipcc
  tests/cpp/libff_host_shim.so    host shim over the shared arithmetic headers  -- g++
  tests/cpp/libdevice_arith.so    device harness over the same headers (tests/test_gpu_arith.py) -- hipcc
  tests/cpp/libdevice_reduce.so   device harness over msm_reduce.hip, the bucket reduction (tests/test_gpu_reduce.py) -- hipcc
  tests/cpp/libdevice_sort.so     device harness over msm_sort.hip, the MSM's bucket sorts (tests/test_gpu_msm_sort.py) -- hipcc
  tests/cpp/libdevice_accum.so    device harness over msm_accum.hip, the MSM's bucket accumulation (tests/test_gpu_accum.py) -- hipcc
  tests/cpp/libfq30_pair_host.so  host build of the paired Fq30 products (tests/test_fq30_pair.py) -- g++
  tests/cpp/libsigma_cell_host.so host build of sigma_cell, the per-cell body of typlonk_circuit_compile (tests/test_circuit_compile_host.py) -- g++
  tests/cpp/perm_pairs_host       host build of the union-find of typlonk_permutation_from_pairs, a program of its own (tests/test_perm_pairs_host.py) -- g++
  tests/cpp/msm_plan_host         host build of msm_plan, every decision of an MSM, a program of its own (tests/test_msm_plan_host.py) -- g++
  tests/cpp/libdevice_chunks.so   device harness over g1_fft.hip, the pointwise pass and the batched group transform of typlonk_open_chunks_*
                                  (tests/test_gpu_pointwise_msm.py) -- hipcc
  tests/cpp/open_chunks_plan_host host build of open_chunks_plan, the launch shape of that pointwise pass, a program of its own
                                  (tests/test_open_chunks_plan_host.py) -- g++
  tests/cpp/libdevice_verify_chunks.so  device harness over verify_chunks.hip, the membership flags, the weights and the fold of
                                  typlonk_verify_chunks (tests/test_gpu_verify_chunks_kernels.py) -- hipcc
  tests/cpp/verify_chunks_plan_host  host build of verify_chunks_plan, the launch shape of that fold, a program of its own
                                  (tests/test_verify_chunks_plan_host.py) -- g++
  tests/cpp/libdevice_recover_chunks.so  device harness over recover_chunks.hip, the vanishing products, the scatter, the scale and the finish of
                                  typlonk_recover_chunks, each alone (tests/test_gpu_recover_chunks_kernels.py) -- hipcc
  tests/cpp/recover_chunks_plan_host[_san]  host build of recover_chunks_plan, every decision of that call (refusals, sizes, launch shapes), a
                                  program of its own, once plain and once under the address and undefined-behaviour sanitizers
                                  (tests/test_recover_chunks_plan_host.py) -- g++
  tests/cpp/ntt_plan_host         host build of ntt_plan, every decision of a batch of NTTs, a program of its own (tests/test_ntt_plan_host.py) -- g++
  tests/cpp/solve_plan_host[_san] host build of solve_plan, every decision of a witness solve, a program of its own, once plain and once under the
                                  address and undefined-behaviour sanitizers (tests/test_solve_plan_host.py) -- g++
  tests/cpp/solve_hints_host[_san] the same header with hints (typlonk_circuit_set_hints): the hinted plan, plain and sanitized
                                  (tests/test_solve_hints_host.py) -- g++
  tests/cpp/prove_plan_host[_san] host build of prove_plan, where a proof's data lives and what each workspace of a prover call holds, a program of its
                                  own, once plain and once under the address and undefined-behaviour sanitizers (tests/test_prove_plan_host.py) -- g++
  tests/cpp/madd_acc_host[_san]   host build of g1_madd_acc / g1_acc_finish, the accumulation loops' mixed addition, a program of its own, once plain
                                  and once under the address and undefined-behaviour sanitizers (tests/test_madd_acc_host.py) -- g++
  tests/cpp/fq30_rows_host[_san]  host build of csrc/fq30_rows.hpp, Fq with one limb per lane and g1_add_rows over an array-of-64 wave, a program of its
                                  own, once plain and once under the address and undefined-behaviour sanitizers (tests/test_fq30_rows_host.py) -- g++
  tests/cpp/libdevice_reduce_rows.so  device harness over g1_add_rows and the row-form bit planes of msm_reduce.hip (tests/test_gpu_reduce_rows.py) -- hipcc
  tests/cpp/libdevice_pair.so     device build of the same (tests/test_gpu_fq30_pair.py) -- hipcc
  tests/cpp/test_{poly,kzg,plonk,wire,...}_host  tests of the C++ host mirror (typlonk_amd/host) -- g++

Every target is rebuilt only when one of its sources is newer than the output.
"""
from __future__ import annotations

import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "typlonk_amd", "csrc")
LIB = os.path.join(ROOT, "typlonk_amd", "libtyplonk_hip.so")


def _stale(out: str, srcs: list[str]) -> bool:
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(s) > t for s in srcs if os.path.exists(s))


def _run(cmd: list[str]) -> None:
    print("+", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)


def hipcc_path() -> str:
    p = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(p):
        raise RuntimeError("hipcc not found: the HIP library cannot be built (there is no CPU fallback)")
    return p


HIP_UNITS = ["ctx.hip", "ntt_host.hip", "msm_host.hip", "comm.hip", "prover.hip", "ntt_kernels.hip", "msm_sort.hip", "msm_accum.hip", "msm_reduce.hip", "srs_gen.hip", "quotient.hip", "plonk_ops.hip", "poly_eval.hip", "verify.hip", "prove_batch.hip", "point_codec.hip", "witness_check.hip", "perm_pairs.hip", "witness_solve.hip", "srs_check.hip", "g1_fft.hip", "open_chunks.hip", "verify_chunks.hip", "verify_chunks_host.hip",
             "recover_chunks.hip", "recover_chunks_host.hip"]
# per-unit flags (none in use).  -DFQ30_ASM_CHAIN for msm_accum.hip was measured: the micro-benchmark's mixed-add ceiling
# rises 7.0 -> 7.3-7.5 G/s (profiles/r02_ubench2_chain.txt) but the real accumulation kernel does not move in a same-box
# A/B (profiles/r02_ab_chain_ntt.txt: 1.85-1.90 ms either way), so the compiler-scheduled form stays.
UNIT_FLAGS: dict[str, list[str]] = {}


def build_hip(force: bool = False) -> str:
    """one object per .hip unit (compiled in parallel, each only when stale), then one link"""
    from concurrent.futures import ThreadPoolExecutor

    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    hdrs.append(os.path.join(ROOT, "include", "typlonk.h"))
    objdir = os.path.join(CSRC, "_obj")
    # a tree that came with its library but without the objects (they are intermediate files): nothing to do while the
    # library is newer than every source
    if not force and not _stale(LIB, [os.path.join(CSRC, u) for u in HIP_UNITS] + hdrs):
        return LIB
    os.makedirs(objdir, exist_ok=True)
    hipcc = hipcc_path()
    jobs, objs = [], []
    for u in HIP_UNITS:
        src = os.path.join(CSRC, u)
        obj = os.path.join(objdir, u.replace(".hip", ".o"))
        objs.append(obj)
        if force or _stale(obj, [src] + hdrs):
            jobs.append([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", *UNIT_FLAGS.get(u, []), "-c", src, "-o", obj])
    if jobs:
        with ThreadPoolExecutor(max_workers=min(6, len(jobs))) as ex:
            list(ex.map(_run, jobs))
    if jobs or not os.path.exists(LIB):
        _run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", LIB])
    return LIB


def build_hip_variant(name: str, unit_flags: dict[str, list[str]]) -> str:
    """a second build of the library under tools/_ab/<name>/ with extra per-unit flags: same-box A/B measurements load it
    through TYPLONK_LIB_PATH (python -m typlonk_amd.build variant <name> <unit.hip>:<flag>[,<flag>] ...)"""
    from concurrent.futures import ThreadPoolExecutor

    out_dir = os.path.join(ROOT, "tools", "_ab", name)
    os.makedirs(out_dir, exist_ok=True)
    hipcc = hipcc_path()
    base_obj = os.path.join(CSRC, "_obj")
    jobs, objs = [], []
    for u in HIP_UNITS:
        if u in unit_flags:
            obj = os.path.join(out_dir, u.replace(".hip", ".o"))
            jobs.append([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", *UNIT_FLAGS.get(u, []), *unit_flags[u], "-c",
                         os.path.join(CSRC, u), "-o", obj])
        else:
            obj = os.path.join(base_obj, u.replace(".hip", ".o"))   # the default build's object
        objs.append(obj)
    build_hip()
    with ThreadPoolExecutor(max_workers=min(6, max(1, len(jobs)))) as ex:
        list(ex.map(_run, jobs))
    lib = os.path.join(out_dir, "libtyplonk_hip.so")
    _run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", lib])
    return lib


def build_hip_test_hooks(force: bool = False) -> str:
    """tests/cpp/hooks/libtyplonk_hip.so: the library with comm.hip compiled under -DTYPLONK_TEST_HOOKS (the staging-failure
    injection of tests/test_gpu_dist.py).  Test-only: the shipped library carries no such switch; the dist tests load this
    build through TYPLONK_LIB_PATH in the rank that is meant to fail."""
    out_dir = os.path.join(ROOT, "tests", "cpp", "hooks")
    os.makedirs(out_dir, exist_ok=True)
    lib = os.path.join(out_dir, "libtyplonk_hip.so")
    hipcc = hipcc_path()
    build_hip()
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")] + [os.path.join(ROOT, "include", "typlonk.h")]
    src = os.path.join(CSRC, "comm.hip")
    obj = os.path.join(out_dir, "comm.o")
    base_obj = os.path.join(CSRC, "_obj")
    objs = [obj if u == "comm.hip" else os.path.join(base_obj, u.replace(".hip", ".o")) for u in HIP_UNITS]
    # (as build_hip: a hooks library newer than its sources and the base library stands without the objects)
    if not force and not _stale(lib, [src] + hdrs + [LIB]):
        return lib
    if not all(os.path.exists(o) for o in objs if o != obj):
        build_hip(force=True)
    # comm.o is linked with the base objects, so it must be compiled from the same headers (typlonk_ctx's layout): one older
    # than the base library may come from other sources with newer mtimes, and is rebuilt
    if force or _stale(obj, [src] + hdrs + [LIB]):
        _run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-DTYPLONK_TEST_HOOKS", "-c", src, "-o", obj])
    if force or _stale(lib, objs):
        _run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", lib])
    return lib


def build_host_shim(force: bool = False) -> str:
    src = os.path.join(ROOT, "tests", "cpp", "ff_host_shim.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "libff_host_shim.so")
    deps = [src, os.path.join(CSRC, "ff.hpp"), os.path.join(CSRC, "g1.hpp"), os.path.join(CSRC, "fq30.hpp"), os.path.join(CSRC, "g1_host64.hpp"),
            os.path.join(CSRC, "fr30.hpp"), os.path.join(CSRC, "fr_inv.hpp"), os.path.join(CSRC, "transcript.hpp"), os.path.join(CSRC, "lin_commit.hpp")]
    if force or _stale(out, deps):
        _run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", out])
    return out


def build_device_arith(force: bool = False) -> str:
    """tests/cpp/libdevice_arith.so: the arithmetic headers' device code behind element-wise test kernels
    (tests/test_gpu_arith.py).  Test-only and not linked into the shipped library; the flags are build_hip()'s."""
    src = os.path.join(ROOT, "tests", "cpp", "device_arith.hip")
    out = os.path.join(ROOT, "tests", "cpp", "libdevice_arith.so")
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if force or _stale(out, [src] + hdrs):
        _run([hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", src, "-o", out])
    return out


def build_device_reduce(force: bool = False) -> str:
    """tests/cpp/libdevice_reduce.so: csrc/harness/device_reduce.hip, msm_reduce.hip compiled as a unit behind an entry point that runs its launchers on a
    caller-made bucket array (tests/test_gpu_reduce.py).  Test-only and not linked into the shipped library; the flags are
    build_hip()'s."""
    src = os.path.join(CSRC, "harness", "device_reduce.hip")
    out = os.path.join(ROOT, "tests", "cpp", "libdevice_reduce.so")
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")] + [os.path.join(CSRC, "msm_reduce.hip")]
    if force or _stale(out, [src] + deps):
        _run([hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", src, "-o", out])
    return out


def build_device_sort(force: bool = False) -> str:
    """tests/cpp/libdevice_sort.so: csrc/harness/device_sort.hip, msm_sort.hip compiled as a unit behind an entry point that plans an MSM
    and runs one chunk's bucket sort -- segmented or atomic -- into guarded buffers of the plan's sizes (tests/test_gpu_msm_sort.py).
    Test-only and not linked into the shipped library; the flags are build_hip()'s."""
    src = os.path.join(CSRC, "harness", "device_sort.hip")
    out = os.path.join(ROOT, "tests", "cpp", "libdevice_sort.so")
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")] + [os.path.join(CSRC, "msm_sort.hip")]
    if force or _stale(out, [src] + deps):
        _run([hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", src, "-o", out])
    return out


def build_device_accum(force: bool = False) -> str:
    """tests/cpp/libdevice_accum.so: csrc/harness/device_accum.hip, msm_accum.hip compiled as a unit behind an entry point that runs the
    accumulation and the heavy-bucket pass on caller-made sort outputs, points and stored buckets, after checking on the host that no index
    leaves its array (tests/test_gpu_accum.py).  Test-only and not linked into the shipped library; the flags are build_hip()'s."""
    src = os.path.join(CSRC, "harness", "device_accum.hip")
    out = os.path.join(ROOT, "tests", "cpp", "libdevice_accum.so")
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")] + [os.path.join(CSRC, "msm_accum.hip")]
    if force or _stale(out, [src] + deps):
        _run([hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", src, "-o", out])
    return out


def build_device_chunks(force: bool = False) -> str:
    """tests/cpp/libdevice_chunks.so: csrc/harness/device_chunks.hip, g1_fft.hip compiled as a unit behind entry points that run the
    pointwise pass of typlonk_open_chunks_* with a named number of slices and the batched stages of the group transform at named
    strides (tests/test_gpu_pointwise_msm.py).  Test-only and not linked into the shipped library; the flags are build_hip()'s."""
    src = os.path.join(CSRC, "harness", "device_chunks.hip")
    out = os.path.join(ROOT, "tests", "cpp", "libdevice_chunks.so")
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")] + [os.path.join(CSRC, "g1_fft.hip")]
    if force or _stale(out, [src] + deps):
        _run([hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", src, "-o", out])
    return out


def build_open_chunks_plan_host(force: bool = False) -> str:
    """tests/cpp/open_chunks_plan_host: open_chunks_plan (csrc/open_chunks_plan.hpp) as the host compiles it, printing the plan of each
    case it reads"""
    src = os.path.join(ROOT, "tests", "cpp", "open_chunks_plan_host.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "open_chunks_plan_host")
    deps = [src, os.path.join(CSRC, "open_chunks_plan.hpp")]
    if force or _stale(out, deps):
        _run(["g++", "-O2", "-std=c++17", src, "-o", out])
    return out


def build_device_verify_chunks(force: bool = False) -> str:
    """tests/cpp/libdevice_verify_chunks.so: csrc/harness/device_verify_chunks.hip, verify_chunks.hip compiled as a unit behind entry
    points that run the weights, the fold with a named strip size and its sum, and the membership flags
    (tests/test_gpu_verify_chunks_kernels.py).  Test-only and not linked into the shipped library; the flags are build_hip()'s."""
    src = os.path.join(CSRC, "harness", "device_verify_chunks.hip")
    out = os.path.join(ROOT, "tests", "cpp", "libdevice_verify_chunks.so")
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")] + [os.path.join(CSRC, "verify_chunks.hip")]
    if force or _stale(out, [src] + deps):
        _run([hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", src, "-o", out])
    return out


def build_verify_chunks_plan_host(force: bool = False) -> str:
    """tests/cpp/verify_chunks_plan_host: verify_chunks_plan (csrc/verify_chunks_plan.hpp) as the host compiles it, printing the plan of
    each case it reads"""
    src = os.path.join(ROOT, "tests", "cpp", "verify_chunks_plan_host.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "verify_chunks_plan_host")
    deps = [src, os.path.join(CSRC, "verify_chunks_plan.hpp")]
    if force or _stale(out, deps):
        _run(["g++", "-O2", "-std=c++17", src, "-o", out])
    return out


def build_device_recover_chunks(force: bool = False) -> str:
    """tests/cpp/libdevice_recover_chunks.so: csrc/harness/device_recover_chunks.hip, recover_chunks.hip compiled as a unit behind entry
    points that run each kernel of typlonk_recover_chunks alone, the vanishing products with a named number of slices
    (tests/test_gpu_recover_chunks_kernels.py).  Test-only and not linked into the shipped library; the flags are build_hip()'s."""
    src = os.path.join(CSRC, "harness", "device_recover_chunks.hip")
    out = os.path.join(ROOT, "tests", "cpp", "libdevice_recover_chunks.so")
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")] + [os.path.join(CSRC, "recover_chunks.hip")]
    if force or _stale(out, [src] + deps):
        _run([hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", src, "-o", out])
    return out


def build_recover_chunks_plan_host(force: bool = False, sanitize: bool = False) -> str:
    """tests/cpp/recover_chunks_plan_host: recover_chunks_refusal and recover_chunks_plan (csrc/recover_chunks_plan.hpp) as the host compiles
    them, printing the verdict and the plan of each case it reads; sanitize: the same program as tests/cpp/recover_chunks_plan_host_san,
    compiled with -fsanitize=address,undefined"""
    src = os.path.join(ROOT, "tests", "cpp", "recover_chunks_plan_host.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "recover_chunks_plan_host_san" if sanitize else "recover_chunks_plan_host")
    deps = [src, os.path.join(CSRC, "recover_chunks_plan.hpp")]
    if force or _stale(out, deps):
        extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        _run(["g++", *extra, "-std=c++17", src, "-o", out])
    return out


def build_fq30_pair_host(force: bool = False) -> str:
    """tests/cpp/libfq30_pair_host.so: fq30_mul_pair / fq30_sqr_pair / fq30_mul2_add as the host compiles them"""
    src = os.path.join(ROOT, "tests", "cpp", "fq30_pair_host.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "libfq30_pair_host.so")
    deps = [src, os.path.join(ROOT, "tests", "cpp", "fq30_pair_harness.hpp"), os.path.join(CSRC, "ff.hpp"), os.path.join(CSRC, "fq30.hpp")]
    if force or _stale(out, deps):
        _run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", out])
    return out


def build_sigma_cell_host(force: bool = False) -> str:
    """tests/cpp/libsigma_cell_host.so: sigma_cell (csrc/sigma_cell.hpp) as the host compiles it, over tables built on the host"""
    src = os.path.join(ROOT, "tests", "cpp", "sigma_cell_host.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "libsigma_cell_host.so")
    deps = [src, os.path.join(CSRC, "ff.hpp"), os.path.join(CSRC, "sigma_cell.hpp")]
    if force or _stale(out, deps):
        _run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", out])
    return out


def build_perm_pairs_host(force: bool = False) -> str:
    """tests/cpp/perm_pairs_host: the find, hook and jump bodies of csrc/perm_pairs.hpp as the host compiles them, run by threads"""
    src = os.path.join(ROOT, "tests", "cpp", "perm_pairs_host.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "perm_pairs_host")
    deps = [src, os.path.join(CSRC, "ff.hpp"), os.path.join(CSRC, "perm_pairs.hpp")]
    if force or _stale(out, deps):
        _run(["g++", "-O2", "-std=c++17", "-pthread", src, "-o", out])
    return out


def build_msm_plan_host(force: bool = False) -> str:
    """tests/cpp/msm_plan_host: msm_plan (csrc/msm_plan.hpp) as the host compiles it, printing the plan of each case it reads"""
    src = os.path.join(ROOT, "tests", "cpp", "msm_plan_host.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "msm_plan_host")
    deps = [src, os.path.join(CSRC, "ff.hpp"), os.path.join(CSRC, "msm_plan.hpp")]
    if force or _stale(out, deps):
        _run(["g++", "-O2", "-std=c++17", src, "-o", out])
    return out


def build_ntt_plan_host(force: bool = False) -> str:
    """tests/cpp/ntt_plan_host: ntt_plan (csrc/ntt_plan.hpp) as the host compiles it, printing the plan of each case it reads"""
    src = os.path.join(ROOT, "tests", "cpp", "ntt_plan_host.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "ntt_plan_host")
    deps = [src, os.path.join(CSRC, "ff.hpp"), os.path.join(CSRC, "fr30.hpp"), os.path.join(CSRC, "ntt_args.hpp"), os.path.join(CSRC, "ntt_plan.hpp")]
    if force or _stale(out, deps):
        _run(["g++", "-O2", "-std=c++17", src, "-o", out])
    return out


def build_prove_plan_host(force: bool = False, sanitize: bool = False) -> str:
    """tests/cpp/prove_plan_host: prove_plan (csrc/prove_plan.hpp) as the host compiles it, printing the plan of each case it reads;
    sanitize: the same program as tests/cpp/prove_plan_host_san, compiled with -fsanitize=address,undefined"""
    src = os.path.join(ROOT, "tests", "cpp", "prove_plan_host.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "prove_plan_host_san" if sanitize else "prove_plan_host")
    deps = [src] + [os.path.join(CSRC, h) for h in ("ff.hpp", "fr30.hpp", "ntt_args.hpp", "ntt_plan.hpp", "prove_plan.hpp")]
    if force or _stale(out, deps):
        extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        _run(["g++", *extra, "-std=c++17", src, "-o", out])
    return out


def build_solve_plan_host(force: bool = False, sanitize: bool = False) -> str:
    """tests/cpp/solve_plan_host: solve_plan (csrc/solve_plan.hpp) as the host compiles it, printing the plan of each circuit it reads;
    sanitize: the same program as tests/cpp/solve_plan_host_san, compiled with -fsanitize=address,undefined"""
    src = os.path.join(ROOT, "tests", "cpp", "solve_plan_host.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "solve_plan_host_san" if sanitize else "solve_plan_host")
    deps = [src, os.path.join(CSRC, "solve_plan.hpp")]
    if force or _stale(out, deps):
        extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        _run(["g++", *extra, "-std=c++17", src, "-o", out])
    return out


def build_madd_acc_host(force: bool = False, sanitize: bool = False) -> str:
    """tests/cpp/madd_acc_host: g1_madd_acc / g1_acc_finish (csrc/g1.hpp) as the host compiles them, run over the cases it reads;
    sanitize: the same program as tests/cpp/madd_acc_host_san, compiled with -fsanitize=address,undefined"""
    src = os.path.join(ROOT, "tests", "cpp", "madd_acc_host.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "madd_acc_host_san" if sanitize else "madd_acc_host")
    deps = [src, os.path.join(CSRC, "ff.hpp"), os.path.join(CSRC, "fq30.hpp"), os.path.join(CSRC, "g1.hpp")]
    if force or _stale(out, deps):
        extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        _run(["g++", *extra, "-std=c++17", src, "-o", out])
    return out


def build_solve_hints_host(force: bool = False, sanitize: bool = False) -> str:
    """tests/cpp/solve_hints_host: solve_plan with hints (csrc/solve_plan.hpp) as the host compiles it, printing the hinted plan of each
    circuit it reads; sanitize: the same program as tests/cpp/solve_hints_host_san, compiled with -fsanitize=address,undefined"""
    src = os.path.join(ROOT, "tests", "cpp", "solve_hints_host.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "solve_hints_host_san" if sanitize else "solve_hints_host")
    deps = [src, os.path.join(CSRC, "solve_plan.hpp")]
    if force or _stale(out, deps):
        extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        _run(["g++", *extra, "-std=c++17", src, "-o", out])
    return out


def build_fq30_rows_host(force: bool = False, sanitize: bool = False) -> str:
    """tests/cpp/fq30_rows_host: csrc/fq30_rows.hpp as the host compiles it (the wave an array of 64), run over the commands it reads;
    sanitize: the same program as tests/cpp/fq30_rows_host_san, compiled with -fsanitize=address,undefined"""
    src = os.path.join(ROOT, "tests", "cpp", "fq30_rows_host.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "fq30_rows_host_san" if sanitize else "fq30_rows_host")
    deps = [src] + [os.path.join(CSRC, h) for h in ("ff.hpp", "fq30.hpp", "g1.hpp", "fq30_rows.hpp")]
    if force or _stale(out, deps):
        extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        _run(["g++", *extra, "-std=c++17", src, "-o", out])
    return out


def build_device_reduce_rows(force: bool = False) -> str:
    """tests/cpp/libdevice_reduce_rows.so: csrc/harness/device_reduce_rows.hip, msm_reduce.hip compiled as a unit behind entry points that
    run g1_add_rows on caller-made pairs and the four-launch reduction with its planes summed either way (tests/test_gpu_reduce_rows.py).
    Test-only and not linked into the shipped library; the flags are build_hip()'s."""
    src = os.path.join(CSRC, "harness", "device_reduce_rows.hip")
    out = os.path.join(ROOT, "tests", "cpp", "libdevice_reduce_rows.so")
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")] + [os.path.join(CSRC, "msm_reduce.hip")]
    if force or _stale(out, [src] + deps):
        _run([hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", src, "-o", out])
    return out


def build_device_pair(force: bool = False) -> str:
    """tests/cpp/libdevice_pair.so: the same functions' device code (the interleaved chains of fq30_pair.hpp) behind an
    element-wise test kernel.  Test-only; the flags are build_hip()'s."""
    src = os.path.join(ROOT, "tests", "cpp", "device_pair.hip")
    out = os.path.join(ROOT, "tests", "cpp", "libdevice_pair.so")
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    hdrs.append(os.path.join(ROOT, "tests", "cpp", "fq30_pair_harness.hpp"))
    if force or _stale(out, [src] + hdrs):
        _run([hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", src, "-o", out])
    return out


def build_host_tests(force: bool = False) -> list[str]:
    """test binaries of the C++ host mirror (typlonk_amd/host/typlonk_host.hpp), linked to the HIP library"""
    outs = []
    hdr = [os.path.join(ROOT, "typlonk_amd", "host", "typlonk_host.hpp"), os.path.join(ROOT, "typlonk_amd", "host", "pairing_host.hpp"),
           os.path.join(ROOT, "tests", "cpp", "circuit_host.hpp"),
           os.path.join(CSRC, "ff.hpp"), os.path.join(CSRC, "fq30.hpp"), os.path.join(CSRC, "g1_host64.hpp"),
           os.path.join(CSRC, "transcript.hpp"), LIB]
    for name in ("test_poly_host", "test_kzg_host", "test_plonk_host", "test_pairing_host", "test_circuit_tables_host", "test_circuit_host",
                 "test_comm_host", "test_comm_ranks_host", "test_compact_ranks_host", "test_verify_host", "test_prove_batch_host", "test_compact_host",
                 "test_prove_batch_compact_host", "test_wire_host", "test_witness_check_host", "test_circuit_compile_host",
                 "test_circuit_pairs_host", "test_witness_solve_host", "test_witness_hints_host", "test_srs_check_host",
                 "test_srs_lagrange_host", "test_open_all_host", "test_open_chunks_host", "test_verify_chunks_host", "test_recover_chunks_host"):
        src = os.path.join(ROOT, "tests", "cpp", name + ".cpp")
        out = os.path.join(ROOT, "tests", "cpp", name)
        if name in ("test_witness_hints_host", "test_srs_check_host", "test_srs_lagrange_host", "test_open_all_host", "test_open_chunks_host", "test_verify_chunks_host", "test_recover_chunks_host") and not os.path.exists(src):   # (an earlier commit's tests/, as in build_all)
            continue
        if force or _stale(out, [src] + hdr):
            _run(["g++", "-O2", "-std=c++17", src, "-o", out, "-L", os.path.join(ROOT, "typlonk_amd"), "-ltyplonk_hip",
                  "-Wl,-rpath," + os.path.join(ROOT, "typlonk_amd"), "-Wl,-rpath,$ORIGIN/../../typlonk_amd"])
        outs.append(out)
    return outs


def build_fake_rccl(force: bool = False) -> str:
    """tests/cpp/libfake_rccl.so: the test-only stand-in for librccl (N ranks on one GPU over POSIX shared memory) that
    tests/test_gpu_dist.py selects through TYPLONK_RCCL_LIB -- never loaded by the product on its own"""
    src = os.path.join(ROOT, "tests", "cpp", "fake_rccl.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "libfake_rccl.so")
    if force or _stale(out, [src]):
        _run([hipcc_path(), "-O2", "-std=c++17", "-shared", "-fPIC", "-x", "hip", "--offload-arch=gfx950", src, "-o", out, "-lrt"])
    return out


def build_all(force: bool = False) -> None:
    build_hip(force)
    build_hip_test_hooks(force)
    build_host_shim(force)
    build_device_arith(force)
    build_device_reduce(force)
    build_device_sort(force)
    build_device_accum(force)
    build_fq30_pair_host(force)
    build_sigma_cell_host(force)
    build_perm_pairs_host(force)
    # the tests/ of a commit before msm_plan.hpp, ntt_plan.hpp, prove_plan.hpp or g1_madd_acc, run against this library to compare the two, has
    # neither these programs' sources nor tests of them
    if os.path.exists(os.path.join(ROOT, "tests", "cpp", "msm_plan_host.cpp")):
        build_msm_plan_host(force)
    if os.path.exists(os.path.join(ROOT, "tests", "cpp", "ntt_plan_host.cpp")):
        build_ntt_plan_host(force)
    if os.path.exists(os.path.join(ROOT, "tests", "cpp", "prove_plan_host.cpp")):
        build_prove_plan_host(force)
        build_prove_plan_host(force, sanitize=True)
    if os.path.exists(os.path.join(ROOT, "tests", "cpp", "madd_acc_host.cpp")):
        build_madd_acc_host(force)
        build_madd_acc_host(force, sanitize=True)
    if os.path.exists(os.path.join(ROOT, "tests", "cpp", "solve_plan_host.cpp")):
        build_solve_plan_host(force)
        build_solve_plan_host(force, sanitize=True)
    if os.path.exists(os.path.join(ROOT, "tests", "cpp", "solve_hints_host.cpp")):
        build_solve_hints_host(force)
        build_solve_hints_host(force, sanitize=True)
    if os.path.exists(os.path.join(ROOT, "tests", "cpp", "fq30_rows_host.cpp")):
        build_fq30_rows_host(force)
        build_fq30_rows_host(force, sanitize=True)
    build_device_reduce_rows(force)
    build_device_pair(force)
    build_device_chunks(force)
    if os.path.exists(os.path.join(ROOT, "tests", "cpp", "open_chunks_plan_host.cpp")):
        build_open_chunks_plan_host(force)
    build_device_verify_chunks(force)
    if os.path.exists(os.path.join(ROOT, "tests", "cpp", "verify_chunks_plan_host.cpp")):
        build_verify_chunks_plan_host(force)
    build_device_recover_chunks(force)
    if os.path.exists(os.path.join(ROOT, "tests", "cpp", "recover_chunks_plan_host.cpp")):
        build_recover_chunks_plan_host(force)
        build_recover_chunks_plan_host(force, sanitize=True)
    build_host_tests(force)
    build_fake_rccl(force)


if __name__ == "__main__":
    import sys

    if len(sys.argv) >= 3 and sys.argv[1] == "variant":
        flags: dict[str, list[str]] = {}
        for spec in sys.argv[3:]:
            unit, _, fl = spec.partition(":")
            flags[unit] = [f for f in fl.split(",") if f]
        print(build_hip_variant(sys.argv[2], flags))
    else:
        build_all()
