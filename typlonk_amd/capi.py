"""ctypes binding of include/typlonk.h (libtyplonk_hip.so).  Plumbing only: device memory,
streams and torch.distributed live in Python; every computation on the MSM/NTT path happens in the
HIP library.  There is no CPU fallback: a missing library or device raises."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# TYPLONK_LIB_PATH: another build of the same library (same-box A/B measurements of kernel variants)
LIB_PATH = os.environ.get("TYPLONK_LIB_PATH") or os.path.join(_HERE, "libtyplonk_hip.so")

OK = 0
ERR_INVALID_ARG, ERR_LENGTH, ERR_DOMAIN, ERR_NO_DEVICE, ERR_HIP, ERR_OOM, ERR_RANGE, ERR_UNSATISFIED = -1, -2, -3, -4, -5, -6, -7, -8
ERR_COMM = -9
COMM_ID_BYTES = 128

# every symbol include/typlonk.h declares (tests check the library exports all of them)
SYMBOLS = [
    "typlonk_init", "typlonk_destroy", "typlonk_strerror", "typlonk_last_error", "typlonk_set_stream",
    "typlonk_sync", "typlonk_srs_load", "typlonk_srs_generate", "typlonk_srs_download", "typlonk_srs_precompute", "typlonk_srs_set_shard", "typlonk_srs_free", "typlonk_srs_len", "typlonk_msm_g1",
    "typlonk_msm_g1_dev", "typlonk_msm_g1_devptr", "typlonk_msm_g1_batch_devptr", "typlonk_ntt_fr", "typlonk_ntt_fr_dev",
    "typlonk_ntt_fr_devptr", "typlonk_ntt_fr_batch_devptr", "typlonk_quotient_dev", "typlonk_grand_product_dev", "typlonk_open_dev", "typlonk_lincomb_dev", "typlonk_prover_round1", "typlonk_prover_round2",
    "typlonk_prover_round3", "typlonk_prover_round3_evals", "typlonk_prover_round4_batched", "typlonk_prover_free",
    "typlonk_prove", "typlonk_prove_host", "typlonk_transcript_challenges", "typlonk_circuit_load", "typlonk_circuit_free", "typlonk_buf_alloc", "typlonk_buf_free", "typlonk_buf_upload",
    "typlonk_buf_download", "typlonk_buf_zero", "typlonk_buf_len", "typlonk_buf_devptr",
    "typlonk_g1_sum_host", "typlonk_set_profiling", "typlonk_profile_get", "typlonk_msm_plan", "typlonk_selftest_fq_inv",
    "typlonk_version",
    "typlonk_comm_available", "typlonk_comm_unique_id", "typlonk_comm_init", "typlonk_comm_destroy", "typlonk_comm_info", "typlonk_comm_fold_g1",
    "typlonk_msm_g1_sharded_devptr", "typlonk_msm_g1_sharded_batch_devptr", "typlonk_g1_fold_records_host",
    "typlonk_poly_eval_dev", "typlonk_circuit_commitments", "typlonk_verify", "typlonk_prove_batch", "typlonk_prove_batch_host",
    "typlonk_circuit_vk", "typlonk_prove_compact", "typlonk_prove_compact_host", "typlonk_verify_compact", "typlonk_compact_challenges",
    "typlonk_prove_batch_compact", "typlonk_prove_batch_compact_host",
    "typlonk_g1_compress", "typlonk_g1_decompress", "typlonk_srs_load_compressed", "typlonk_srs_download_compressed",
    "typlonk_proof_compact_to_bytes", "typlonk_vk_to_bytes", "typlonk_vk_from_bytes", "typlonk_proof_compact_from_bytes",
    "typlonk_verify_compact_bytes",
    "typlonk_circuit_permutation", "typlonk_witness_check", "typlonk_witness_check_host",
    "typlonk_circuit_compile", "typlonk_circuit_compile_host",
    "typlonk_permutation_from_pairs", "typlonk_circuit_compile_pairs", "typlonk_circuit_compile_pairs_host",
    "typlonk_witness_solve_plan", "typlonk_witness_solve", "typlonk_circuit_set_hints",
    "typlonk_srs_check", "typlonk_srs_check_challenge", "typlonk_srs_contribute", "typlonk_srs_g1_ntt",
    "typlonk_srs_open_all_table", "typlonk_open_all_dev", "typlonk_open_all_host",
    "typlonk_srs_open_chunks_table", "typlonk_open_chunks_dev", "typlonk_open_chunks_host",
    "typlonk_verify_chunks", "typlonk_verify_chunks_challenge",
    "typlonk_recover_chunks",
]
VERIFY_PI_AS_PROVER = 1
SRS_TO_LAGRANGE, SRS_FROM_LAGRANGE = 0, 1   # typlonk_srs_g1_ntt's direction
# the wire format (include/typlonk.h): reject classes of a decoded field, the decode flag, the sizes
POINT_ENCODING, POINT_X_RANGE, POINT_NOT_ON_CURVE, POINT_NOT_IN_SUBGROUP, SCALAR_RANGE = 1, 2, 3, 4, 5
DECODE_SKIP_SUBGROUP = 1
G1_BYTES, G2_BYTES, PROOF_COMPACT_BYTES, VK_WIRE_BYTES = 48, 96, 656, 628


def decode_status(status: int) -> tuple[int, int]:
    """a decode status -> (reject class, index of the first bad field)"""
    return status & 0xff, status >> 8


class TyplonkError(RuntimeError):
    def __init__(self, code: int, detail: str = ""):
        self.code = code
        super().__init__(f"typlonk error {code}: {detail}")


class QuotientArgs(C.Structure):
    """typlonk_quotient_args"""
    _fields_ = [("wires", C.c_void_p * 3), ("z", C.c_void_p), ("selectors", C.c_void_p * 5), ("sigma", C.c_void_p * 3),
                ("public_inputs", C.c_void_p), ("alpha", C.c_uint64 * 4), ("beta", C.c_uint64 * 4),
                ("gamma", C.c_uint64 * 4), ("cosets", (C.c_uint64 * 4) * 3), ("circuit", C.c_uint32)]


class ProofTail(C.Structure):
    """typlonk_proof_tail"""
    _fields_ = [("t_xy", (C.c_uint64 * 12) * 3), ("t_inf", C.c_uint8 * 3), ("w_xy", (C.c_uint64 * 12) * 6),
                ("w_inf", C.c_uint8 * 6), ("evals", (C.c_uint64 * 4) * 6)]


class ProofEvals(C.Structure):
    """typlonk_proof_evals"""
    _fields_ = [("evals", (C.c_uint64 * 4) * 6)]


class ProofBatched(C.Structure):
    """typlonk_proof_batched"""
    _fields_ = [("t_xy", (C.c_uint64 * 12) * 3), ("t_inf", C.c_uint8 * 3), ("w_xy", (C.c_uint64 * 12) * 2),
                ("w_inf", C.c_uint8 * 2)]


class Proof(C.Structure):
    """typlonk_proof"""
    _fields_ = [("commit_xy", (C.c_uint64 * 12) * 3), ("commit_inf", C.c_uint8 * 3), ("z_xy", C.c_uint64 * 12),
                ("z_inf", C.c_uint8), ("tail", ProofTail), ("beta", C.c_uint64 * 4), ("gamma", C.c_uint64 * 4),
                ("alpha", C.c_uint64 * 4), ("zeta", C.c_uint64 * 4)]


class Vk(C.Structure):
    """typlonk_vk: the verifying key of the compact proof shape"""
    _fields_ = [("log_n", C.c_uint32), ("cosets", (C.c_uint64 * 4) * 3), ("commit_xy", (C.c_uint64 * 12) * 8),
                ("commit_inf", C.c_uint8 * 8), ("srs0_xy", C.c_uint64 * 12), ("srs0_inf", C.c_uint8), ("g2s_xy", C.c_uint64 * 24)]


class WitnessReport(C.Structure):
    """typlonk_witness_report"""
    _fields_ = [("gate_failures", C.c_uint64), ("copy_failures", C.c_uint64), ("gate_listed", C.c_uint32), ("copy_listed", C.c_uint32)]


CELL_NONE = 0xFFFFFFFF   # TYPLONK_CELL_NONE


HINT_INV0, HINT_BITS = 1, 2   # TYPLONK_HINT_*


class Hint(C.Structure):
    """typlonk_hint"""
    _fields_ = [("kind", C.c_uint32), ("dst", C.c_uint32), ("src", C.c_uint32), ("shift", C.c_uint16), ("width", C.c_uint16)]


HINT_DTYPE = np.dtype([("kind", "<u4"), ("dst", "<u4"), ("src", "<u4"), ("shift", "<u2"), ("width", "<u2")])   # typlonk_hint, 16 bytes


SRS_VALID, SRS_BAD_POINT, SRS_BAD_P0, SRS_BAD_RATIO = 0, 1, 2, 3   # TYPLONK_SRS_*


class SrsReport(C.Structure):
    """typlonk_srs_report"""
    _fields_ = [("verdict", C.c_uint32), ("point_class", C.c_uint32), ("index", C.c_uint64), ("bad_points", C.c_uint64),
                ("folds", C.c_uint32)]


CELL_OK, CELL_BAD_EVAL, CELL_BAD_POINT, CELL_BAD_COMMITMENT, CELL_BAD_PROOF = 0, 1, 2, 3, 4   # TYPLONK_CELL_* of typlonk_verify_chunks


class ChunksReport(C.Structure):
    """typlonk_chunks_report"""
    _fields_ = [("folds", C.c_uint32), ("reserved", C.c_uint32), ("live", C.c_uint64), ("count", C.c_uint64 * 5)]


RECOVER_OK, RECOVER_BAD_EVAL, RECOVER_INCONSISTENT = 0, 1, 2   # TYPLONK_RECOVER_* of typlonk_recover_chunks
NO_EXCESS = 0xFFFFFFFFFFFFFFFF   # first_excess of a polynomial that is not RECOVER_INCONSISTENT


class RecoverReport(C.Structure):
    """typlonk_recover_report"""
    _fields_ = [("known", C.c_uint32), ("missing", C.c_uint32), ("count", C.c_uint64 * 3)]


class SolveInfo(C.Structure):
    """typlonk_solve_info"""
    _fields_ = [("driven_rows", C.c_uint64), ("free_classes", C.c_uint64), ("depth", C.c_uint32), ("launches", C.c_uint32)]


class ProofCompact(C.Structure):
    """typlonk_proof_compact"""
    _fields_ = [("commit_xy", (C.c_uint64 * 12) * 3), ("commit_inf", C.c_uint8 * 3), ("z_xy", C.c_uint64 * 12),
                ("z_inf", C.c_uint8), ("t_xy", (C.c_uint64 * 12) * 3), ("t_inf", C.c_uint8 * 3), ("w_xy", (C.c_uint64 * 12) * 2),
                ("w_inf", C.c_uint8 * 2), ("evals", (C.c_uint64 * 4) * 7), ("beta", C.c_uint64 * 4), ("gamma", C.c_uint64 * 4),
                ("alpha", C.c_uint64 * 4), ("zeta", C.c_uint64 * 4), ("v", C.c_uint64 * 4)]


COMPACT_CHALLENGES = ("beta", "gamma", "alpha", "zeta", "v")


def compact_dict(pr: ProofCompact) -> dict:
    """typlonk_proof_compact -> {"commit": [(xy, inf)] * 3, "z_commit", "t_commit": [...] * 3, "witness": [W_zeta, W_zeta_w],
    "evals": 7 x 4 limbs (a b c Z(zeta) Z(zeta w) sigma_1 sigma_2), "challenges": beta gamma alpha zeta v}"""
    pt = lambda xy, f: (np.array(xy, dtype=np.uint64), int(f))   # noqa: E731
    return {
        "commit": [pt(pr.commit_xy[i], pr.commit_inf[i]) for i in range(3)],
        "z_commit": pt(pr.z_xy, pr.z_inf),
        "t_commit": [pt(pr.t_xy[i], pr.t_inf[i]) for i in range(3)],
        "witness": [pt(pr.w_xy[i], pr.w_inf[i]) for i in range(2)],
        "evals": [np.array(pr.evals[i], dtype=np.uint64) for i in range(7)],
        "challenges": {k: np.array(getattr(pr, k), dtype=np.uint64) for k in COMPACT_CHALLENGES},
    }


def compact_struct(d) -> ProofCompact:
    """the inverse of compact_dict (a dict without "challenges" leaves them zero: the verifier recomputes them)"""
    if isinstance(d, ProofCompact):
        return d
    pr = ProofCompact()

    def put(dst, val, k):
        dst[:] = [int(v) for v in np.asarray(val, dtype=np.uint64).reshape(k)]

    for i, (xy, f) in enumerate(d["commit"]):
        put(pr.commit_xy[i], xy, 12)
        pr.commit_inf[i] = int(f)
    put(pr.z_xy, d["z_commit"][0], 12)
    pr.z_inf = int(d["z_commit"][1])
    for i, (xy, f) in enumerate(d["t_commit"]):
        put(pr.t_xy[i], xy, 12)
        pr.t_inf[i] = int(f)
    for i, (xy, f) in enumerate(d["witness"]):
        put(pr.w_xy[i], xy, 12)
        pr.w_inf[i] = int(f)
    for i, e in enumerate(d["evals"]):
        put(pr.evals[i], e, 4)
    for k, val in d.get("challenges", {}).items():
        put(getattr(pr, k), val, 4)
    return pr


def vk_from(log_n: int, cosets, commitments, srs0, g2s_xy) -> Vk:
    """a typlonk_vk from its parts: cosets = 3 x 4 limbs, commitments = [(xy, inf)] * 8, srs0 = (xy, inf), g2s_xy = 24 limbs"""
    vk = Vk()
    vk.log_n = log_n
    for i in range(3):
        vk.cosets[i][:] = [int(v) for v in np.asarray(cosets[i], dtype=np.uint64).reshape(4)]
    for i, (xy, f) in enumerate(commitments):
        vk.commit_xy[i][:] = [int(v) for v in np.asarray(xy, dtype=np.uint64).reshape(12)]
        vk.commit_inf[i] = int(f)
    vk.srs0_xy[:] = [int(v) for v in np.asarray(srs0[0], dtype=np.uint64).reshape(12)]
    vk.srs0_inf = int(srs0[1])
    vk.g2s_xy[:] = [int(v) for v in np.asarray(g2s_xy, dtype=np.uint64).reshape(24)]
    return vk


def _cosets_arg(cosets):
    ks = ((C.c_uint64 * 4) * 3)()
    for i in range(3):
        for j, limb in enumerate(np.asarray(cosets[i], dtype=np.uint64).reshape(4)):
            ks[i][j] = int(limb)
    return ks


def _pi_arg(pi, k: int):
    """None or one (l, 4) column (or None) per proof -> (keep-alive list, u64** or None, size_t* or None)"""
    if pi is None:
        return [], None, None
    keep = []
    pip = (C.POINTER(C.c_uint64) * max(k, 1))()
    lens = (C.c_size_t * max(k, 1))()
    for i, col in enumerate(pi):
        if col is None:
            continue
        c = np.ascontiguousarray(_as_u64(col, 4))
        keep.append(c)
        pip[i] = _u64p(c)
        lens[i] = c.shape[0]
    return keep, pip, lens


def compact_challenges(vk: Vk, proof, pi=None):
    """typlonk_compact_challenges (host-only): [beta, gamma, alpha, zeta, v] of a compact proof (dict or struct), 4 limbs each"""
    lib = load_library()
    pr = compact_struct(proof)
    col = np.ascontiguousarray(_as_u64(pi, 4)) if pi is not None else np.zeros((0, 4), dtype=np.uint64)
    out = ((C.c_uint64 * 4) * 5)()
    rc = lib.typlonk_compact_challenges(C.byref(vk), C.byref(pr), _u64p(col) if col.shape[0] else None, col.shape[0], out)
    if rc:
        raise TyplonkError(rc, lib.typlonk_strerror(rc).decode())
    return [np.array(out[i], dtype=np.uint64) for i in range(5)]


_lib = None


def load_library() -> C.CDLL:
    """dlopen the in-tree HIP library; fail loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch wheels bundle their own HIP / HSA runtime next to the system one this library links (/opt/rocm).  One
    # process can hold both only if PyTorch's copy is loaded FIRST (its libraries are global, so the system runtime
    # loaded afterwards shares its HSA layer); the other way round two independent HSA runtimes come up and whichever
    # initialises second reports "no device".  Importing torch here -- when it is installed -- fixes the order for every
    # Python process that uses both; C, C++ and Rust callers never see any of this.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(the MSM/NTT path has no CPU fallback)")
    lib = C.CDLL(LIB_PATH)
    u64p, u8p, vp = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.c_void_p
    lib.typlonk_init.argtypes = [C.POINTER(vp), C.c_int]
    lib.typlonk_destroy.argtypes = [vp]
    lib.typlonk_destroy.restype = None
    lib.typlonk_strerror.argtypes = [C.c_int]
    lib.typlonk_strerror.restype = C.c_char_p
    lib.typlonk_last_error.argtypes = [vp]
    lib.typlonk_last_error.restype = C.c_char_p
    lib.typlonk_set_stream.argtypes = [vp, vp]
    lib.typlonk_sync.argtypes = [vp]
    lib.typlonk_srs_load.argtypes = [vp, u64p, u8p, C.c_size_t, C.POINTER(C.c_uint32)]
    lib.typlonk_srs_generate.argtypes = [vp, u64p, C.c_uint64, C.c_size_t, C.POINTER(C.c_uint32)]
    lib.typlonk_srs_download.argtypes = [vp, C.c_uint32, C.c_size_t, C.c_size_t, u64p, u8p]
    lib.typlonk_srs_precompute.argtypes = [vp, C.c_uint32, C.c_uint32]
    lib.typlonk_srs_free.argtypes = [vp, C.c_uint32]
    lib.typlonk_srs_set_shard.argtypes = [vp, C.c_uint32, C.c_size_t, C.c_size_t]
    lib.typlonk_srs_len.argtypes = [vp, C.c_uint32, C.POINTER(C.c_size_t)]
    lib.typlonk_msm_g1.argtypes = [vp, C.c_uint32, u64p, C.c_size_t, u64p, u8p]
    lib.typlonk_msm_g1_dev.argtypes = [vp, C.c_uint32, vp, C.c_size_t, C.c_size_t, u64p, u8p]
    lib.typlonk_msm_g1_devptr.argtypes = [vp, C.c_uint32, vp, C.c_size_t, u64p, u8p]
    lib.typlonk_msm_g1_batch_devptr.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_size_t), C.c_size_t, u64p, u8p]
    lib.typlonk_g1_fold_records_host.argtypes = [u64p, C.c_size_t, C.c_size_t, u64p, u8p, C.POINTER(C.c_int)]
    lib.typlonk_comm_available.argtypes = []
    lib.typlonk_comm_available.restype = C.c_int
    lib.typlonk_comm_unique_id.argtypes = [u8p]
    lib.typlonk_comm_init.argtypes = [vp, u8p, C.c_int, C.c_int]
    lib.typlonk_comm_destroy.argtypes = [vp]
    lib.typlonk_comm_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.typlonk_comm_fold_g1.argtypes = [vp, u64p, u8p, C.c_size_t]
    lib.typlonk_msm_g1_sharded_devptr.argtypes = [vp, C.c_uint32, vp, C.c_size_t, u64p, u8p]
    lib.typlonk_msm_g1_sharded_batch_devptr.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_size_t), C.c_size_t, u64p, u8p]
    lib.typlonk_ntt_fr.argtypes = [vp, u64p, C.c_uint32, C.c_int, u64p]
    lib.typlonk_ntt_fr_dev.argtypes = [vp, vp, C.c_size_t, C.c_uint32, C.c_int, u64p]
    lib.typlonk_ntt_fr_devptr.argtypes = [vp, vp, C.c_uint32, C.c_int, u64p]
    # (an A/B build of an OLDER revision, loaded through TYPLONK_LIB_PATH for a same-box measurement, may predate this
    # entry point; the in-tree library must export it -- tests/test_host.py checks every symbol of the header)
    if hasattr(lib, "typlonk_ntt_fr_batch_devptr") or not os.environ.get("TYPLONK_LIB_PATH"):
        lib.typlonk_ntt_fr_batch_devptr.argtypes = [vp, C.POINTER(C.c_void_p), C.c_size_t, C.c_uint32, C.c_int, u64p]
    lib.typlonk_quotient_dev.argtypes = [vp, C.POINTER(QuotientArgs), C.c_uint32, vp]
    lib.typlonk_grand_product_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), u64p, u64p, C.POINTER((C.c_uint64 * 4) * 3),
                                              C.c_uint32, vp]
    lib.typlonk_open_dev.argtypes = [vp, vp, C.c_size_t, C.c_size_t, u64p, vp, u64p]
    lib.typlonk_poly_eval_dev.argtypes = [vp, C.POINTER(vp), C.c_size_t, C.c_size_t, C.c_size_t, u64p, C.c_size_t, u64p]
    lib.typlonk_circuit_commitments.argtypes = [vp, C.c_uint32, C.c_uint32, u64p, u8p]
    lib.typlonk_verify.argtypes = [vp, C.c_uint32, C.c_uint32, u64p, C.POINTER((C.c_uint64 * 4) * 3), C.POINTER(Proof),
                                   C.c_size_t, C.POINTER(u64p), C.POINTER(C.c_size_t), C.c_uint32, u8p]
    lib.typlonk_lincomb_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint64 * 4), C.c_size_t, u64p, C.c_size_t, vp]
    lib.typlonk_prover_round1.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(vp), vp, C.POINTER(vp),
                                          C.POINTER((C.c_uint64 * 12) * 3), C.POINTER(C.c_uint8 * 3)]
    lib.typlonk_prover_round2.argtypes = [vp, u64p, u64p, C.POINTER((C.c_uint64 * 4) * 3), u64p, u8p]
    lib.typlonk_prover_round3.argtypes = [vp, u64p, u64p, C.POINTER(ProofTail)]
    lib.typlonk_prover_round3_evals.argtypes = [vp, u64p, u64p, C.POINTER(ProofEvals)]
    lib.typlonk_prover_round4_batched.argtypes = [vp, u64p, C.POINTER(ProofBatched)]
    lib.typlonk_prove.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(vp), vp, C.POINTER((C.c_uint64 * 4) * 3), C.POINTER(Proof)]
    if hasattr(lib, "typlonk_prove_host") or not os.environ.get("TYPLONK_LIB_PATH"):   # (as typlonk_ntt_fr_batch_devptr above)
        lib.typlonk_prove_host.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(u64p), u64p, C.POINTER((C.c_uint64 * 4) * 3), C.POINTER(Proof)]
    if hasattr(lib, "typlonk_prove_batch") or not os.environ.get("TYPLONK_LIB_PATH"):   # (as typlonk_ntt_fr_batch_devptr above)
        lib.typlonk_prove_batch.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(vp), C.POINTER(vp), C.c_size_t,
                                            C.POINTER((C.c_uint64 * 4) * 3), C.POINTER(Proof), C.POINTER(C.c_int)]
        lib.typlonk_prove_batch_host.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(u64p), C.POINTER(u64p), C.c_size_t,
                                                 C.POINTER((C.c_uint64 * 4) * 3), C.POINTER(Proof), C.POINTER(C.c_int)]
    lib.typlonk_transcript_challenges.argtypes = [u64p, u8p, C.c_size_t, C.c_size_t, u64p]
    if hasattr(lib, "typlonk_prove_compact") or not os.environ.get("TYPLONK_LIB_PATH"):   # (as typlonk_ntt_fr_batch_devptr above)
        lib.typlonk_circuit_vk.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER((C.c_uint64 * 4) * 3), u64p, C.POINTER(Vk)]
        lib.typlonk_prove_compact.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(vp), vp, C.c_size_t,
                                              C.POINTER((C.c_uint64 * 4) * 3), C.POINTER(ProofCompact)]
        lib.typlonk_prove_compact_host.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(u64p), C.c_size_t, u64p, C.c_size_t,
                                                   C.POINTER((C.c_uint64 * 4) * 3), C.POINTER(ProofCompact)]
        lib.typlonk_verify_compact.argtypes = [vp, C.POINTER(Vk), C.POINTER(ProofCompact), C.c_size_t, C.POINTER(u64p),
                                               C.POINTER(C.c_size_t), u8p]
        lib.typlonk_compact_challenges.argtypes = [C.POINTER(Vk), C.POINTER(ProofCompact), u64p, C.c_size_t,
                                                   C.POINTER(C.c_uint64 * 4)]
    if hasattr(lib, "typlonk_prove_batch_compact") or not os.environ.get("TYPLONK_LIB_PATH"):   # (as typlonk_ntt_fr_batch_devptr above)
        lib.typlonk_prove_batch_compact.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t),
                                                    C.c_size_t, C.POINTER((C.c_uint64 * 4) * 3), C.POINTER(ProofCompact),
                                                    C.POINTER(C.c_int)]
        lib.typlonk_prove_batch_compact_host.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(u64p), C.c_size_t, C.POINTER(u64p),
                                                         C.POINTER(C.c_size_t), C.c_size_t, C.POINTER((C.c_uint64 * 4) * 3),
                                                         C.POINTER(ProofCompact), C.POINTER(C.c_int)]
    lib.typlonk_prover_free.argtypes = [vp]
    lib.typlonk_prover_free.restype = None
    lib.typlonk_circuit_load.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.c_uint32, C.POINTER(C.c_uint32)]
    lib.typlonk_circuit_free.argtypes = [vp, C.c_uint32]
    lib.typlonk_buf_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    lib.typlonk_buf_free.argtypes = [vp, vp]
    lib.typlonk_buf_upload.argtypes = [vp, vp, C.c_size_t, u64p, C.c_size_t]
    lib.typlonk_buf_download.argtypes = [vp, vp, C.c_size_t, u64p, C.c_size_t]
    lib.typlonk_buf_zero.argtypes = [vp, vp, C.c_size_t, C.c_size_t]
    lib.typlonk_buf_len.argtypes = [vp]
    lib.typlonk_buf_len.restype = C.c_size_t
    lib.typlonk_buf_devptr.argtypes = [vp]
    lib.typlonk_buf_devptr.restype = vp
    lib.typlonk_g1_sum_host.argtypes = [u64p, u8p, C.c_size_t, u64p, u8p]
    lib.typlonk_set_profiling.argtypes = [vp, C.c_int]
    lib.typlonk_profile_get.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]
    lib.typlonk_msm_plan.argtypes = [vp, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                     C.POINTER(C.c_uint64)]
    lib.typlonk_selftest_fq_inv.argtypes = [vp, C.c_uint64, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    lib.typlonk_version.restype = C.c_char_p
    if hasattr(lib, "typlonk_g1_decompress") or not os.environ.get("TYPLONK_LIB_PATH"):   # (as typlonk_ntt_fr_batch_devptr above)
        u32p = C.POINTER(C.c_uint32)
        lib.typlonk_g1_compress.argtypes = [u64p, u8p, C.c_size_t, u8p]
        lib.typlonk_g1_decompress.argtypes = [vp, u8p, C.c_size_t, C.c_uint32, u64p, u8p, u8p]
        lib.typlonk_srs_load_compressed.argtypes = [vp, u8p, C.c_size_t, C.c_uint32, u32p, C.POINTER(C.c_size_t)]
        lib.typlonk_srs_download_compressed.argtypes = [vp, C.c_uint32, C.c_size_t, C.c_size_t, u8p]
        lib.typlonk_proof_compact_to_bytes.argtypes = [C.POINTER(ProofCompact), u8p]
        lib.typlonk_vk_to_bytes.argtypes = [C.POINTER(Vk), u8p]
        lib.typlonk_vk_from_bytes.argtypes = [u8p, C.c_uint32, C.POINTER(Vk), u32p]
        lib.typlonk_proof_compact_from_bytes.argtypes = [vp, u8p, C.c_size_t, C.c_uint32, C.POINTER(ProofCompact), u32p]
        lib.typlonk_verify_compact_bytes.argtypes = [vp, C.POINTER(Vk), u8p, C.c_size_t, C.POINTER(u64p), C.POINTER(C.c_size_t),
                                                     C.c_uint32, u8p]
    if hasattr(lib, "typlonk_witness_check") or not os.environ.get("TYPLONK_LIB_PATH"):   # (as typlonk_ntt_fr_batch_devptr above)
        u32p = C.POINTER(C.c_uint32)
        lib.typlonk_circuit_permutation.argtypes = [vp, C.c_uint32, C.POINTER((C.c_uint64 * 4) * 3), u32p, C.POINTER(C.c_uint64)]
        lib.typlonk_witness_check.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t), C.c_size_t,
                                              C.POINTER((C.c_uint64 * 4) * 3), C.c_uint32, C.POINTER(WitnessReport), u32p, u32p]
        lib.typlonk_witness_check_host.argtypes = [vp, C.c_uint32, C.POINTER(u64p), C.c_size_t, C.POINTER(u64p),
                                                   C.POINTER(C.c_size_t), C.c_size_t, C.POINTER((C.c_uint64 * 4) * 3), C.c_uint32,
                                                   C.POINTER(WitnessReport), u32p, u32p]
    if hasattr(lib, "typlonk_circuit_compile") or not os.environ.get("TYPLONK_LIB_PATH"):   # (as typlonk_ntt_fr_batch_devptr above)
        u32p = C.POINTER(C.c_uint32)
        lib.typlonk_circuit_compile.argtypes = [vp, C.POINTER(vp), u32p, C.POINTER((C.c_uint64 * 4) * 3), C.c_uint32, u32p,
                                                C.POINTER(C.c_uint64)]
        lib.typlonk_circuit_compile_host.argtypes = [vp, C.POINTER(u64p), C.c_size_t, u32p, C.POINTER((C.c_uint64 * 4) * 3),
                                                     C.c_uint32, u32p, C.POINTER(C.c_uint64)]
    if hasattr(lib, "typlonk_permutation_from_pairs") or not os.environ.get("TYPLONK_LIB_PATH"):   # (as typlonk_ntt_fr_batch_devptr above)
        u32p = C.POINTER(C.c_uint32)
        lib.typlonk_permutation_from_pairs.argtypes = [vp, u32p, C.c_size_t, C.c_uint32, u32p, C.POINTER(C.c_uint64)]
        lib.typlonk_circuit_compile_pairs.argtypes = [vp, C.POINTER(vp), u32p, C.c_size_t, C.POINTER((C.c_uint64 * 4) * 3),
                                                      C.c_uint32, u32p, C.POINTER(C.c_uint64)]
        lib.typlonk_circuit_compile_pairs_host.argtypes = [vp, C.POINTER(u64p), C.c_size_t, u32p, C.c_size_t,
                                                           C.POINTER((C.c_uint64 * 4) * 3), C.c_uint32, u32p, C.POINTER(C.c_uint64)]
    if hasattr(lib, "typlonk_witness_solve") or not os.environ.get("TYPLONK_LIB_PATH"):   # (as typlonk_ntt_fr_batch_devptr above)
        u32p = C.POINTER(C.c_uint32)
        lib.typlonk_witness_solve_plan.argtypes = [vp, C.c_uint32, C.POINTER((C.c_uint64 * 4) * 3), C.POINTER(SolveInfo)]
        lib.typlonk_witness_solve.argtypes = [vp, C.c_uint32, C.POINTER((C.c_uint64 * 4) * 3), u32p, C.c_size_t, u64p, C.POINTER(vp),
                                              C.POINTER(C.c_size_t), C.c_size_t, C.POINTER(vp)]
    if hasattr(lib, "typlonk_circuit_set_hints") or not os.environ.get("TYPLONK_LIB_PATH"):
        lib.typlonk_circuit_set_hints.argtypes = [vp, C.c_uint32, C.POINTER((C.c_uint64 * 4) * 3), C.POINTER(Hint), C.c_size_t]
    if hasattr(lib, "typlonk_srs_check") or not os.environ.get("TYPLONK_LIB_PATH"):   # (as typlonk_ntt_fr_batch_devptr above)
        lib.typlonk_srs_check.argtypes = [vp, C.c_uint32, u64p, u8p, C.POINTER(SrsReport)]
        lib.typlonk_srs_check_challenge.argtypes = [u8p, C.c_uint64, u64p, u64p]
        lib.typlonk_srs_contribute.argtypes = [vp, C.c_uint32, u64p, u64p, C.POINTER(C.c_uint32), u64p]
    if hasattr(lib, "typlonk_srs_g1_ntt") or not os.environ.get("TYPLONK_LIB_PATH"):   # (as typlonk_ntt_fr_batch_devptr above)
        lib.typlonk_srs_g1_ntt.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    if hasattr(lib, "typlonk_open_all_dev") or not os.environ.get("TYPLONK_LIB_PATH"):   # (as typlonk_ntt_fr_batch_devptr above)
        lib.typlonk_srs_open_all_table.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
        lib.typlonk_open_all_dev.argtypes = [vp, C.c_uint32, vp, C.c_size_t, C.c_size_t, u64p, u8p, u64p]
        lib.typlonk_open_all_host.argtypes = [vp, C.c_uint32, u64p, C.c_size_t, u64p, u8p, u64p]
    if hasattr(lib, "typlonk_open_chunks_dev") or not os.environ.get("TYPLONK_LIB_PATH"):   # (as typlonk_ntt_fr_batch_devptr above)
        lib.typlonk_srs_open_chunks_table.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
        lib.typlonk_open_chunks_dev.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_size_t), C.c_size_t, C.c_size_t, u64p, u8p, u64p]
        lib.typlonk_open_chunks_host.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.c_size_t, C.c_size_t, u64p, u8p, u64p]
    if hasattr(lib, "typlonk_verify_chunks") or not os.environ.get("TYPLONK_LIB_PATH"):   # (as typlonk_ntt_fr_batch_devptr above)
        u32p = C.POINTER(C.c_uint32)
        lib.typlonk_verify_chunks.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, u64p, u8p, u64p, u8p, C.c_size_t, u32p, u32p, u64p,
                                              u64p, u8p, C.c_size_t, u8p, C.POINTER(ChunksReport)]
        lib.typlonk_verify_chunks_challenge.argtypes = [u8p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, u64p, u64p]
    if hasattr(lib, "typlonk_recover_chunks") or not os.environ.get("TYPLONK_LIB_PATH"):   # (as typlonk_ntt_fr_batch_devptr above)
        u32p = C.POINTER(C.c_uint32)
        lib.typlonk_recover_chunks.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_size_t, u32p, C.c_size_t, u64p, C.c_size_t, C.POINTER(vp),
                                               C.POINTER(C.c_size_t), u64p, u64p, u8p, u64p, C.POINTER(RecoverReport)]
    _lib = lib
    return lib


def _u64p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _u8p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _as_u64(a, cols: int) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a.reshape(-1, cols)


def comm_available() -> bool:
    """typlonk_comm_available: can librccl be loaded in this process?  Not collective -- ranks agree on it before comm_init"""
    return bool(load_library().typlonk_comm_available())


def comm_unique_id() -> bytes:
    """typlonk_comm_unique_id (rank 0): the 128-byte RCCL rendezvous id the other ranks need for Context.comm_init"""
    lib = load_library()
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    rc = lib.typlonk_comm_unique_id(buf)
    if rc:
        raise TyplonkError(rc, lib.typlonk_strerror(rc).decode())
    return bytes(buf)


def g1_fold_records_host(records, world: int, count: int):
    """typlonk_g1_fold_records_host: the library's post-all-gather fold on (world, count, 13) uint64 records; returns
    [(xy[12], inf)] * count, raises TyplonkError(ERR_COMM) naming the rank whose records are flagged.  No GPU needed."""
    lib = load_library()
    rec = np.ascontiguousarray(records, dtype=np.uint64).reshape(world, count, 13)
    out = np.zeros((max(count, 1), 12), dtype=np.uint64)
    oinf = np.zeros(max(count, 1), dtype=np.uint8)
    failed = C.c_int(-1)
    rc = lib.typlonk_g1_fold_records_host(_u64p(rec), world, count, _u64p(out), _u8p(oinf), C.byref(failed))
    if rc:
        raise TyplonkError(rc, f"{lib.typlonk_strerror(rc).decode()} (rank {failed.value})")
    return [(out[i].copy(), int(oinf[i])) for i in range(count)]


def g1_sum_host(xy, inf=None):
    """Deterministic index-order fold of affine points (typlonk_g1_sum_host); no GPU needed."""
    lib = load_library()
    xy = _as_u64(xy, 12)
    n = xy.shape[0]
    infp = None
    if inf is not None:
        inf = np.ascontiguousarray(inf, dtype=np.uint8)
        infp = _u8p(inf)
    out = np.zeros(12, dtype=np.uint64)
    oinf = np.zeros(1, dtype=np.uint8)
    rc = lib.typlonk_g1_sum_host(_u64p(xy), infp, n, _u64p(out), _u8p(oinf))
    if rc:
        raise TyplonkError(rc, lib.typlonk_strerror(rc).decode())
    return out, int(oinf[0])


def _bytes_arg(data, unit: int, what: str) -> np.ndarray:
    """bytes / a uint8 array whose length is a multiple of `unit` -> a contiguous uint8 array"""
    a = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else \
        np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    if a.size % unit:
        raise ValueError(f"{what}: {a.size} bytes is not a multiple of {unit}")
    return a


def _host_err(lib, rc: int):
    if rc:
        raise TyplonkError(rc, lib.typlonk_strerror(rc).decode())


def g1_compress(xy, inf=None) -> bytes:
    """typlonk_g1_compress (host-only): (count, 12) limbs + optional flags -> count * 48 bytes"""
    lib = load_library()
    xy = _as_u64(xy, 12)
    n = xy.shape[0]
    infp = None
    if inf is not None:
        inf = np.ascontiguousarray(inf, dtype=np.uint8).reshape(-1)
        if inf.size != n:
            raise ValueError("g1_compress: one infinity flag per point")
        infp = _u8p(inf)
    out = np.zeros(max(n, 1) * G1_BYTES, dtype=np.uint8)
    _host_err(lib, lib.typlonk_g1_compress(_u64p(xy), infp, n, _u8p(out)))
    return out[:n * G1_BYTES].tobytes()


def g1_decompress(data, skip_subgroup: bool = False, ctx: "Context | None" = None):
    """typlonk_g1_decompress: count * 48 bytes -> (xy (count, 12), inf (count,), status (count,)).  ctx = None: on the host."""
    lib = load_library()
    a = _bytes_arg(data, G1_BYTES, "g1_decompress")
    n = a.size // G1_BYTES
    xy = np.zeros((max(n, 1), 12), dtype=np.uint64)
    inf = np.zeros(max(n, 1), dtype=np.uint8)
    st = np.zeros(max(n, 1), dtype=np.uint8)
    rc = lib.typlonk_g1_decompress(ctx.h if ctx is not None else None, _u8p(a) if n else None, n,
                                   DECODE_SKIP_SUBGROUP if skip_subgroup else 0, _u64p(xy), _u8p(inf), _u8p(st))
    if ctx is not None:
        ctx._chk(rc)
    _host_err(lib, rc)
    return xy[:n], inf[:n], st[:n]


def proof_to_bytes(proof) -> bytes:
    """typlonk_proof_compact_to_bytes (host-only): a compact dict or struct -> 656 bytes"""
    lib = load_library()
    pr = compact_struct(proof)
    out = np.zeros(PROOF_COMPACT_BYTES, dtype=np.uint8)
    _host_err(lib, lib.typlonk_proof_compact_to_bytes(C.byref(pr), _u8p(out)))
    return out.tobytes()


def proofs_from_bytes(data, skip_subgroup: bool = False, ctx: "Context | None" = None):
    """typlonk_proof_compact_from_bytes: count * 656 bytes -> ([compact dict] * count, status (count,) uint32); a proof with a
    non-zero status (decode_status) is all identities.  ctx = None decodes on the host, a context on the device."""
    lib = load_library()
    a = _bytes_arg(data, PROOF_COMPACT_BYTES, "proofs_from_bytes")
    k = a.size // PROOF_COMPACT_BYTES
    arr = (ProofCompact * max(k, 1))()
    st = np.zeros(max(k, 1), dtype=np.uint32)
    rc = lib.typlonk_proof_compact_from_bytes(ctx.h if ctx is not None else None, _u8p(a) if k else None, k,
                                              DECODE_SKIP_SUBGROUP if skip_subgroup else 0, arr,
                                              st.ctypes.data_as(C.POINTER(C.c_uint32)))
    if ctx is not None:
        ctx._chk(rc)
    _host_err(lib, rc)
    return [compact_dict(arr[i]) for i in range(k)], st[:k]


def vk_to_bytes(vk: Vk) -> bytes:
    """typlonk_vk_to_bytes (host-only): the 628-byte wire form of a verifying key"""
    lib = load_library()
    out = np.zeros(VK_WIRE_BYTES, dtype=np.uint8)
    _host_err(lib, lib.typlonk_vk_to_bytes(C.byref(vk), _u8p(out)))
    return out.tobytes()


def vk_from_bytes(data, skip_subgroup: bool = False) -> Vk:
    """typlonk_vk_from_bytes (host-only).  A rejected field raises TyplonkError with .status = its decode status."""
    lib = load_library()
    a = _bytes_arg(data, 1, "vk_from_bytes")
    if a.size != VK_WIRE_BYTES:
        raise ValueError(f"vk_from_bytes: {a.size} bytes, a key has {VK_WIRE_BYTES}")
    vk = Vk()
    st = C.c_uint32(0)
    rc = lib.typlonk_vk_from_bytes(_u8p(a), DECODE_SKIP_SUBGROUP if skip_subgroup else 0, C.byref(vk), C.byref(st))
    if rc:
        err = TyplonkError(rc, lib.typlonk_strerror(rc).decode() + f" (decode status {decode_status(st.value)})")
        err.status = st.value
        raise err
    return vk


def transcript_challenges(points, n: int):
    """typlonk_transcript_challenges (host-only): points = [(xy[12], inf), ...] -> n challenges (4 limbs each)"""
    lib = load_library()
    k = len(points)
    xy = np.zeros((max(k, 1), 12), dtype=np.uint64)
    inf = np.zeros(max(k, 1), dtype=np.uint8)
    for i, (p, f) in enumerate(points):
        xy[i] = np.asarray(p, dtype=np.uint64).reshape(12)
        inf[i] = f
    out = np.zeros((n, 4), dtype=np.uint64)
    rc = lib.typlonk_transcript_challenges(_u64p(xy), _u8p(inf), k, n, _u64p(out))
    if rc:
        raise TyplonkError(rc, lib.typlonk_strerror(rc).decode())
    return [out[i].copy() for i in range(n)]


def _seed_arg(seed) -> np.ndarray:
    a = np.frombuffer(bytes(seed), dtype=np.uint8).copy()
    if a.size != 32:
        raise ValueError("the seed of an SRS check is 32 bytes")
    return a


def srs_check_challenge(seed, length: int, g2s_xy) -> np.ndarray:
    """typlonk_srs_check_challenge (host-only): the weight rho typlonk_srs_check derives from (seed, len, [s]G2), 4 Montgomery limbs"""
    lib = load_library()
    s = _seed_arg(seed)
    g = np.ascontiguousarray(g2s_xy, dtype=np.uint64).reshape(24)
    out = np.zeros(4, dtype=np.uint64)
    rc = lib.typlonk_srs_check_challenge(_u8p(s), length, _u64p(g), _u64p(out))
    if rc:
        raise TyplonkError(rc, lib.typlonk_strerror(rc).decode())
    return out


def verify_chunks_challenge(seed, log_n: int, log_l: int, n_cells: int, n_commits: int, g2sl_xy) -> np.ndarray:
    """typlonk_verify_chunks_challenge (host-only): the weight rho typlonk_verify_chunks derives from (seed, log_n, log_l, N, M,
    [s^l]G2), 4 Montgomery limbs"""
    lib = load_library()
    s = _seed_arg(seed)
    g = np.ascontiguousarray(g2sl_xy, dtype=np.uint64).reshape(24)
    out = np.zeros(4, dtype=np.uint64)
    rc = lib.typlonk_verify_chunks_challenge(_u8p(s), log_n, log_l, n_cells, n_commits, _u64p(g), _u64p(out))
    if rc:
        raise TyplonkError(rc, lib.typlonk_strerror(rc).decode())
    return out


class DeviceBuffer:
    """typlonk_buf: a device-resident vector of Fr elements."""

    def __init__(self, ctx: "Context", n: int):
        self.ctx = ctx
        self.handle = C.c_void_p()
        ctx._chk(ctx.lib.typlonk_buf_alloc(ctx.h, n, C.byref(self.handle)))
        self.n = n

    def upload(self, arr, offset: int = 0):
        arr = _as_u64(arr, 4)
        self.ctx._chk(self.ctx.lib.typlonk_buf_upload(self.ctx.h, self.handle, offset, _u64p(arr), arr.shape[0]))

    def download(self, offset: int = 0, n: int | None = None) -> np.ndarray:
        n = self.n - offset if n is None else n
        out = np.empty((n, 4), dtype=np.uint64)
        self.ctx._chk(self.ctx.lib.typlonk_buf_download(self.ctx.h, self.handle, offset, _u64p(out), n))
        return out

    def zero(self, offset: int = 0, n: int | None = None):
        n = self.n - offset if n is None else n
        self.ctx._chk(self.ctx.lib.typlonk_buf_zero(self.ctx.h, self.handle, offset, n))

    @property
    def devptr(self) -> int:
        return self.ctx.lib.typlonk_buf_devptr(self.handle)

    def free(self):
        if self.handle:
            self.ctx.lib.typlonk_buf_free(self.ctx.h, self.handle)
            self.handle = C.c_void_p()


class Context:
    """typlonk_ctx: one HIP device, its stream, MSM workspaces and cached NTT plans."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        self.h = C.c_void_p()
        rc = self.lib.typlonk_init(C.byref(self.h), device)
        if rc:
            raise TyplonkError(rc, self.lib.typlonk_strerror(rc).decode())
        self.device = device

    def _chk(self, rc: int):
        if rc < 0:
            raise TyplonkError(rc, (self.lib.typlonk_strerror(rc).decode() + ": " +
                                    self.lib.typlonk_last_error(self.h).decode()))
        return rc

    def close(self):
        if self.h:
            self.lib.typlonk_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_handle: int | None):
        """run the context's work on an existing hipStream_t (None / 0 = the context's own stream).  The *_devptr
        calls read caller memory in the order of the context's stream (see typlonk_set_stream in typlonk.h): the
        own stream is ordered after the legacy default stream, any other producer stream must be bound here
        (torch: `ctx.set_stream(torch.cuda.current_stream().cuda_stream)`) or synchronised first"""
        self._chk(self.lib.typlonk_set_stream(self.h, stream_handle))

    def sync(self):
        self._chk(self.lib.typlonk_sync(self.h))

    # ---- SRS / MSM ------------------------------------------------------------------------
    def srs_load(self, xy, inf=None) -> int:
        xy = _as_u64(xy, 12)
        infp = None
        if inf is not None:
            inf = np.ascontiguousarray(inf, dtype=np.uint8)
            infp = _u8p(inf)
        sid = C.c_uint32()
        self._chk(self.lib.typlonk_srs_load(self.h, _u64p(xy), infp, xy.shape[0], C.byref(sid)))
        return sid.value

    def srs_generate(self, secret_limbs, length: int, start: int = 0) -> int:
        """[secret^(start+i)] G on the device (Srs::from_secret); secret as 4 Montgomery limbs"""
        s = np.ascontiguousarray(secret_limbs, dtype=np.uint64).reshape(4)
        sid = C.c_uint32()
        self._chk(self.lib.typlonk_srs_generate(self.h, _u64p(s), start, length, C.byref(sid)))
        return sid.value

    def srs_set_shard(self, sid: int, first_index: int, total_len: int):
        """this entry = bases [first_index, first_index + len) of a total_len-point SRS: MSM / prover calls on it
        take the full coefficient vector and return this rank's partial sum"""
        self._chk(self.lib.typlonk_srs_set_shard(self.h, sid, first_index, total_len))

    def srs_download(self, sid: int, offset: int = 0, count: int | None = None):
        count = self.srs_len(sid) - offset if count is None else count
        xy = np.zeros((count, 12), dtype=np.uint64)
        inf = np.zeros(count, dtype=np.uint8)
        self._chk(self.lib.typlonk_srs_download(self.h, sid, offset, count, _u64p(xy), _u8p(inf)))
        return xy, inf

    def srs_load_compressed(self, data, skip_subgroup: bool = False) -> int:
        """typlonk_srs_load_compressed: 48 bytes per point, decoded (and subgroup-checked) on the device.  A rejected point
        raises TyplonkError with .first_bad = the lowest rejected index; no SRS is created."""
        a = _bytes_arg(data, 1, "srs_load_compressed")
        sid = C.c_uint32()
        bad = C.c_size_t(0)
        rc = self.lib.typlonk_srs_load_compressed(self.h, _u8p(a) if a.size else None, a.size,
                                                  DECODE_SKIP_SUBGROUP if skip_subgroup else 0, C.byref(sid), C.byref(bad))
        if rc:
            err = TyplonkError(rc, self.lib.typlonk_strerror(rc).decode() + ": " + self.lib.typlonk_last_error(self.h).decode())
            err.first_bad = bad.value
            raise err
        return sid.value

    def srs_download_compressed(self, sid: int, offset: int = 0, count: int | None = None) -> bytes:
        """typlonk_srs_download_compressed: count * 48 bytes, compressed on the device"""
        count = self.srs_len(sid) - offset if count is None else count
        out = np.zeros(max(count, 1) * G1_BYTES, dtype=np.uint8)
        self._chk(self.lib.typlonk_srs_download_compressed(self.h, sid, offset, count, _u8p(out)))
        return out[:count * G1_BYTES].tobytes()

    def srs_check(self, sid: int, g2s_xy, seed) -> dict:
        """typlonk_srs_check: is entry `sid` [s^i] G for the s of g2s_xy (24 limbs)?  seed: 32 bytes that whoever made the points
        cannot have known.  Returns {"verdict": SRS_*, "point_class", "index", "bad_points", "folds"}; an invalid SRS is a
        verdict, not an exception."""
        g = np.ascontiguousarray(g2s_xy, dtype=np.uint64).reshape(24)
        s = _seed_arg(seed)
        rep = SrsReport()
        self._chk(self.lib.typlonk_srs_check(self.h, sid, _u64p(g), _u8p(s), C.byref(rep)))
        return {"verdict": rep.verdict, "point_class": rep.point_class, "index": rep.index, "bad_points": rep.bad_points,
                "folds": rep.folds}

    def srs_contribute(self, sid: int, t_limbs, g2s_xy):
        """typlonk_srs_contribute: (new sid holding [t^i] P_i, [t] g2s as 24 limbs); t as 4 Montgomery limbs"""
        t = np.ascontiguousarray(t_limbs, dtype=np.uint64).reshape(4)
        g = np.ascontiguousarray(g2s_xy, dtype=np.uint64).reshape(24)
        new = C.c_uint32()
        out = np.zeros(24, dtype=np.uint64)
        self._chk(self.lib.typlonk_srs_contribute(self.h, sid, _u64p(t), _u64p(g), C.byref(new), _u64p(out)))
        return new.value, out

    def srs_lagrange(self, sid: int, log_n: int) -> int:
        """typlonk_srs_g1_ntt, TO_LAGRANGE: a new sid holding [L_i(s)] G, i < 2^log_n, for the monomial entry `sid`: the MSM of a
        column of evaluations over it is the commitment to the column's polynomial"""
        return self._srs_g1_ntt(sid, log_n, SRS_TO_LAGRANGE)

    def srs_from_lagrange(self, sid: int, log_n: int) -> int:
        """typlonk_srs_g1_ntt, FROM_LAGRANGE: a new sid holding the 2^log_n monomial points of the Lagrange entry `sid`"""
        return self._srs_g1_ntt(sid, log_n, SRS_FROM_LAGRANGE)

    def _srs_g1_ntt(self, sid: int, log_n: int, direction: int) -> int:
        new = C.c_uint32()
        self._chk(self.lib.typlonk_srs_g1_ntt(self.h, sid, log_n, direction, C.byref(new)))
        return new.value

    def srs_open_all_table(self, sid: int, log_n: int) -> int:
        """typlonk_srs_open_all_table: the id of the table `open_all` needs for the domain of 2^log_n points over the entry
        `sid` (2^(log_n + 1) records; released by srs_free)"""
        new = C.c_uint32()
        self._chk(self.lib.typlonk_srs_open_all_table(self.h, sid, log_n, C.byref(new)))
        return new.value

    def open_all(self, table: int, coeffs_or_buf, m: int | None = None, evals: bool = True, offset: int = 0):
        """typlonk_open_all_dev / _host: the openings of a polynomial at every point w^k of the table's domain, k < n.
        coeffs_or_buf: a DeviceBuffer (m coefficients from `offset`; m = None: all behind it) or host coefficients (k, 4) u64
        Montgomery.  Returns (xy (n, 12), inf (n,)[, evals (n, 4)])."""
        n = self.srs_len(table) // 2
        xy = np.zeros((n, 12), dtype=np.uint64)
        inf = np.zeros(n, dtype=np.uint8)
        ev = np.zeros((n, 4), dtype=np.uint64) if evals else None
        evp = _u64p(ev) if evals else None
        if isinstance(coeffs_or_buf, DeviceBuffer):
            m = coeffs_or_buf.n - offset if m is None else m
            self._chk(self.lib.typlonk_open_all_dev(self.h, table, coeffs_or_buf.handle, offset, m, _u64p(xy), _u8p(inf), evp))
        else:
            co = _as_u64(coeffs_or_buf, 4)
            m = co.shape[0] if m is None else m
            self._chk(self.lib.typlonk_open_all_host(self.h, table, _u64p(co), m, _u64p(xy), _u8p(inf), evp))
        return (xy, inf, ev) if evals else (xy, inf)

    def srs_open_chunks_table(self, sid: int, log_n: int, log_l: int) -> int:
        """typlonk_srs_open_chunks_table: the id of the table `open_chunks` needs for the domain of 2^log_n points cut into cosets
        of 2^log_l over the entry `sid` (2^(log_n + 1) records; released by srs_free).  log_l = 0 is srs_open_all_table's table."""
        new = C.c_uint32()
        self._chk(self.lib.typlonk_srs_open_chunks_table(self.h, sid, log_n, log_l, C.byref(new)))
        self._chunk_log_l = getattr(self, "_chunk_log_l", {})
        self._chunk_log_l[new.value] = log_l   # (the outputs of open_chunks are sized by it; ids are never reused)
        return new.value

    def open_chunks(self, table: int, polys, m: int | None = None, evals: bool = True, offsets=None):
        """typlonk_open_chunks_dev / _host: the multi-proofs of `count` polynomials on every coset of the table's domain.
        polys: a list of DeviceBuffers (m coefficients from offsets[p], default 0; m = None: all of the first behind its offset) or
        a list of host coefficient arrays (m, 4) u64 Montgomery, all of one length.  With r = n / l cosets of l points, returns
        (xy (count, r, 12), inf (count, r)[, evals (count, r, l, 4) -- evals[p, k, t] = f_p(w^(k + r t))])."""
        n = self.srs_len(table) // 2
        log_l = getattr(self, "_chunk_log_l", {}).get(table, 0)   # (a table of srs_open_all_table: 0)
        l = 1 << log_l
        r = n // l
        polys = list(polys)
        count = len(polys)
        xy = np.zeros((count, r, 12), dtype=np.uint64)
        inf = np.zeros((count, r), dtype=np.uint8)
        ev = np.zeros((count, r, l, 4), dtype=np.uint64) if evals else None
        evp = _u64p(ev) if evals else None
        if count and isinstance(polys[0], DeviceBuffer):
            offs = [0] * count if offsets is None else [int(o) for o in offsets]
            m = polys[0].n - offs[0] if m is None else m
            handles = (C.c_void_p * count)(*[p.handle for p in polys])
            self._chk(self.lib.typlonk_open_chunks_dev(self.h, table, handles, (C.c_size_t * count)(*offs), m, count, _u64p(xy), _u8p(inf), evp))
        else:
            cos = [_as_u64(p, 4) for p in polys]
            m = (cos[0].shape[0] if count else 0) if m is None else m
            if any(c.shape[0] < m for c in cos):
                raise ValueError("open_chunks: a polynomial holds fewer than m coefficients")
            ptrs = (C.c_void_p * max(count, 1))(*[c.ctypes.data for c in cos])
            self._chk(self.lib.typlonk_open_chunks_host(self.h, table, ptrs, m, count, _u64p(xy), _u8p(inf), evp))
        return (xy, inf, ev) if evals else (xy, inf)

    def verify_chunks(self, sid: int, log_n: int, log_l: int, g2sl_xy, seed, commits, cell_commit, cell_coset, evals, proofs) -> dict:
        """typlonk_verify_chunks: N cells of multi-proofs against M commitments in one call.  commits, proofs: (xy (k, 12), inf (k,))
        as srs_download gives points; cell_commit, cell_coset: N indices; evals: (N, l, 4) u64 Montgomery, evals[i, t] =
        f(w^(k_i + r t)); g2sl_xy: [s^l]G2, 24 limbs; seed: 32 bytes that whoever made the cells cannot have known.  Returns
        {"status": (N,) uint8 of CELL_*, "folds", "live", "count": [cells per status]}; a bad cell is a status, not an exception."""
        g = np.ascontiguousarray(g2sl_xy, dtype=np.uint64).reshape(24)
        s = _seed_arg(seed)
        cxy, cinf = _as_u64(commits[0], 12), np.ascontiguousarray(commits[1], dtype=np.uint8).reshape(-1)
        pxy, pinf = _as_u64(proofs[0], 12), np.ascontiguousarray(proofs[1], dtype=np.uint8).reshape(-1)
        cc = np.ascontiguousarray(cell_commit, dtype=np.uint32).reshape(-1)
        ck = np.ascontiguousarray(cell_coset, dtype=np.uint32).reshape(-1)
        n, m = pxy.shape[0], cxy.shape[0]
        ev = np.ascontiguousarray(evals, dtype=np.uint64).reshape(-1)
        if cinf.shape[0] != m or pinf.shape[0] != n or cc.shape[0] != n or ck.shape[0] != n or ev.shape[0] != (n << log_l) * 4:
            raise ValueError("verify_chunks: the arrays of a call do not agree on N, M or l")
        status = np.zeros(max(n, 1), dtype=np.uint8)
        rep = ChunksReport()
        u32 = C.POINTER(C.c_uint32)
        self._chk(self.lib.typlonk_verify_chunks(self.h, sid, log_n, log_l, _u64p(g), _u8p(s), _u64p(cxy), _u8p(cinf), m,
                                                 cc.ctypes.data_as(u32), ck.ctypes.data_as(u32), _u64p(ev), _u64p(pxy), _u8p(pinf), n,
                                                 _u8p(status), C.byref(rep)))
        return {"status": status[:n], "folds": rep.folds, "live": rep.live, "count": list(rep.count)}

    def recover_chunks(self, log_n: int, log_l: int, m: int, cosets, evals, out_bufs=None, offsets=None, want_coeffs: bool = True,
                       want_evals: bool = True) -> dict:
        """typlonk_recover_chunks: `count` polynomials of degree < m from K of the r = n / l cosets of their domain.  cosets: K distinct
        indices in any order, the same for every polynomial; evals: (count, K, l, 4) u64 Montgomery, evals[p, i, t] =
        f_p(w^(cosets[i] + r t)); out_bufs: None or `count` DeviceBuffers that receive the m coefficients at offsets[p] (default 0).
        Returns {"status": (count,) uint8 of RECOVER_*, "first_excess": (count,) uint64 (NO_EXCESS unless RECOVER_INCONSISTENT), "known",
        "missing", "count": [polynomials per status][, "coeffs": (count, m, 4)][, "evals": (count, r, l, 4), as open_chunks gives
        them]}; a polynomial that is not RECOVER_OK gets zeros in every output and is a status, not an exception."""
        ck = np.ascontiguousarray(cosets, dtype=np.uint32).reshape(-1)
        k, l, n = ck.shape[0], 1 << log_l, 1 << log_n
        ev = np.ascontiguousarray(evals, dtype=np.uint64)
        if k == 0 or ev.size % (k * l * 4):
            raise ValueError("recover_chunks: evals does not hold whole polynomials of K cells of l evaluations")
        count = ev.size // (k * l * 4)
        ev = ev.reshape(-1)
        handles = offs = None
        if out_bufs is not None:
            out_bufs = list(out_bufs)
            if len(out_bufs) != count or (offsets is not None and len(offsets) != count):
                raise ValueError("recover_chunks: one buffer and one offset per polynomial")
            handles = (C.c_void_p * max(count, 1))(*[b.handle for b in out_bufs])
            offs = None if offsets is None else (C.c_size_t * max(count, 1))(*[int(o) for o in offsets])
        co = np.zeros((count, m, 4), dtype=np.uint64) if want_coeffs else None
        eo = np.zeros((count, n // l, l, 4), dtype=np.uint64) if want_evals else None
        status = np.zeros(max(count, 1), dtype=np.uint8)
        first = np.zeros(max(count, 1), dtype=np.uint64)
        rep = RecoverReport()
        self._chk(self.lib.typlonk_recover_chunks(self.h, log_n, log_l, m, ck.ctypes.data_as(C.POINTER(C.c_uint32)), k, _u64p(ev), count,
                                                  handles, offs, _u64p(co) if want_coeffs else None, _u64p(eo) if want_evals else None,
                                                  _u8p(status), _u64p(first), C.byref(rep)))
        out = {"status": status[:count], "first_excess": first[:count], "known": rep.known, "missing": rep.missing, "count": list(rep.count)}
        if want_coeffs:
            out["coeffs"] = co
        if want_evals:
            out["evals"] = eo
        return out

    def g1_decompress(self, data, skip_subgroup: bool = False):
        """g1_decompress on this context's device"""
        return g1_decompress(data, skip_subgroup, ctx=self)

    def proofs_from_bytes(self, data, skip_subgroup: bool = False):
        """proofs_from_bytes with the points decoded on this context's device"""
        return proofs_from_bytes(data, skip_subgroup, ctx=self)

    def verify_compact_bytes(self, vk: Vk, data, pi=None, skip_subgroup: bool = False) -> np.ndarray:
        """typlonk_verify_compact_bytes: count * 656 bytes of proofs; pi as for verify_compact.  Returns a bool array; a proof
        that does not decode is False and does not reach the verifier."""
        a = _bytes_arg(data, PROOF_COMPACT_BYTES, "verify_compact_bytes")
        k = a.size // PROOF_COMPACT_BYTES
        if pi is not None and len(pi) != k:
            raise ValueError("verify_compact_bytes: one public-input entry per proof")
        keep, pip, lens = _pi_arg(pi, k)  # noqa: F841
        ok = np.zeros(max(k, 1), dtype=np.uint8)
        self._chk(self.lib.typlonk_verify_compact_bytes(self.h, C.byref(vk), _u8p(a) if k else None, k, pip, lens,
                                                        DECODE_SKIP_SUBGROUP if skip_subgroup else 0, _u8p(ok)))
        return ok[:k].astype(bool)

    def srs_precompute(self, sid: int, window_bits: int = 0):
        """fixed-base window tables for this SRS (typlonk_srs_precompute); 0 = the library picks the window by length"""
        self._chk(self.lib.typlonk_srs_precompute(self.h, sid, window_bits))

    def srs_free(self, sid: int):
        self._chk(self.lib.typlonk_srs_free(self.h, sid))

    def srs_len(self, sid: int) -> int:
        n = C.c_size_t()
        self._chk(self.lib.typlonk_srs_len(self.h, sid, C.byref(n)))
        return n.value

    def msm(self, sid: int, scalars, m: int | None = None):
        """host scalars (n,4) u64 Montgomery -> (xy[12] u64, inf)"""
        scalars = _as_u64(scalars, 4)
        m = scalars.shape[0] if m is None else m
        out = np.zeros(12, dtype=np.uint64)
        oinf = np.zeros(1, dtype=np.uint8)
        self._chk(self.lib.typlonk_msm_g1(self.h, sid, _u64p(scalars), m, _u64p(out), _u8p(oinf)))
        return out, int(oinf[0])

    def msm_dev(self, sid: int, buf: DeviceBuffer, offset: int, m: int):
        out = np.zeros(12, dtype=np.uint64)
        oinf = np.zeros(1, dtype=np.uint8)
        self._chk(self.lib.typlonk_msm_g1_dev(self.h, sid, buf.handle, offset, m, _u64p(out), _u8p(oinf)))
        return out, int(oinf[0])

    def msm_devptr(self, sid: int, devptr: int, m: int):
        out = np.zeros(12, dtype=np.uint64)
        oinf = np.zeros(1, dtype=np.uint8)
        self._chk(self.lib.typlonk_msm_g1_devptr(self.h, sid, devptr, m, _u64p(out), _u8p(oinf)))
        return out, int(oinf[0])

    def msm_batch_devptr(self, sid: int, devptrs, ms):
        """independent MSMs over one SRS, pipelined two at a time -> list of (xy[12], inf)"""
        n = len(devptrs)
        ptrs = (C.c_void_p * n)(*devptrs)
        lens = (C.c_size_t * n)(*ms)
        out = np.zeros((n, 12), dtype=np.uint64)
        oinf = np.zeros(n, dtype=np.uint8)
        self._chk(self.lib.typlonk_msm_g1_batch_devptr(self.h, sid, ptrs, lens, n, _u64p(out), _u8p(oinf)))
        return [(out[i], int(oinf[i])) for i in range(n)]

    # ---- RCCL exchange behind the C ABI (typlonk_comm_*) -------------------------------------
    def comm_init(self, uid: bytes, rank: int, world: int):
        """collective: ncclCommInitRank on this context's device"""
        assert len(uid) == COMM_ID_BYTES
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(uid)
        self._chk(self.lib.typlonk_comm_init(self.h, buf, rank, world))

    def comm_destroy(self):
        self._chk(self.lib.typlonk_comm_destroy(self.h))

    def comm_info(self):
        r, w = C.c_int(), C.c_int()
        self._chk(self.lib.typlonk_comm_info(self.h, C.byref(r), C.byref(w)))
        return r.value, w.value

    def comm_fold(self, points):
        """typlonk_comm_fold_g1: [(xy[12], inf), ...] -> the same list with every point summed over the ranks"""
        k = len(points)
        xy = np.zeros((max(k, 1), 12), dtype=np.uint64)
        inf = np.zeros(max(k, 1), dtype=np.uint8)
        for i, (p, f) in enumerate(points):
            xy[i] = np.asarray(p, dtype=np.uint64).reshape(12)
            inf[i] = f
        self._chk(self.lib.typlonk_comm_fold_g1(self.h, _u64p(xy), _u8p(inf), k))
        return [(xy[i].copy(), int(inf[i])) for i in range(k)]

    def msm_sharded_devptr(self, sid: int, devptr: int, m: int):
        """typlonk_msm_g1_sharded_devptr: local partial MSM over the SRS shard + RCCL all-gather + fold (collective)"""
        out = np.zeros(12, dtype=np.uint64)
        oinf = np.zeros(1, dtype=np.uint8)
        self._chk(self.lib.typlonk_msm_g1_sharded_devptr(self.h, sid, devptr, m, _u64p(out), _u8p(oinf)))
        return out, int(oinf[0])

    def msm_sharded_batch_devptr(self, sid: int, devptrs, ms):
        n = len(devptrs)
        ptrs = (C.c_void_p * n)(*devptrs)
        lens = (C.c_size_t * n)(*ms)
        out = np.zeros((n, 12), dtype=np.uint64)
        oinf = np.zeros(n, dtype=np.uint8)
        self._chk(self.lib.typlonk_msm_g1_sharded_batch_devptr(self.h, sid, ptrs, lens, n, _u64p(out), _u8p(oinf)))
        return [(out[i], int(oinf[i])) for i in range(n)]

    def msm_plan(self, m: int):
        c, w, ops = C.c_uint32(), C.c_uint32(), C.c_uint64()
        self._chk(self.lib.typlonk_msm_plan(self.h, m, C.byref(c), C.byref(w), C.byref(ops)))
        return c.value, w.value, ops.value

    def selftest_fq_inv(self, count: int, seed: int = 1):
        """device divsteps inversion vs the Fermat ladder on `count` residues -> (mismatches, max 30-divstep rounds)"""
        bad, rounds = C.c_uint64(), C.c_uint32()
        self._chk(self.lib.typlonk_selftest_fq_inv(self.h, seed, count, C.byref(bad), C.byref(rounds)))
        return bad.value, rounds.value

    # ---- NTT ------------------------------------------------------------------------------
    @staticmethod
    def _coset(coset):
        if coset is None:
            return None, None
        a = np.ascontiguousarray(coset, dtype=np.uint64).reshape(4)
        return a, _u64p(a)

    def ntt(self, data, log_n: int, inverse: bool = False, coset=None) -> np.ndarray:
        """host vector (2^log_n, 4) u64 -> transformed copy"""
        data = _as_u64(data, 4).copy()
        if data.shape[0] != (1 << log_n):
            raise ValueError("data length must be 2^log_n (caller zero-pads)")
        keep, cp = self._coset(coset)
        self._chk(self.lib.typlonk_ntt_fr(self.h, _u64p(data), log_n, int(inverse), cp))
        return data

    def ntt_dev(self, buf: DeviceBuffer, log_n: int, inverse: bool = False, coset=None, offset: int = 0):
        keep, cp = self._coset(coset)
        self._chk(self.lib.typlonk_ntt_fr_dev(self.h, buf.handle, offset, log_n, int(inverse), cp))

    def ntt_devptr(self, devptr: int, log_n: int, inverse: bool = False, coset=None):
        keep, cp = self._coset(coset)
        self._chk(self.lib.typlonk_ntt_fr_devptr(self.h, devptr, log_n, int(inverse), cp))

    def ntt_batch_devptr(self, devptrs, log_n: int, inverse: bool = False, coset=None):
        """typlonk_ntt_fr_batch_devptr: len(devptrs) vectors of 2^log_n Fr, each transformed in place, every pass one launch"""
        keep, cp = self._coset(coset)
        ptrs = (C.c_void_p * max(len(devptrs), 1))(*[int(p) for p in devptrs])
        self._chk(self.lib.typlonk_ntt_fr_batch_devptr(self.h, ptrs, len(devptrs), log_n, int(inverse), cp))

    def grand_product_dev(self, log_n: int, wire_evals, sigma_evals, beta, gamma, cosets, z_out):
        """typlonk_grand_product_dev: column / sigma EVALUATIONS (DeviceBuffers) -> Z evaluations"""
        w = (C.c_void_p * 3)(*[b.handle.value for b in wire_evals])
        sg = (C.c_void_p * 3)(*[b.handle.value for b in sigma_evals])
        be = np.ascontiguousarray(beta, dtype=np.uint64).reshape(4)
        ga = np.ascontiguousarray(gamma, dtype=np.uint64).reshape(4)
        ks = ((C.c_uint64 * 4) * 3)()
        for i in range(3):
            for j, limb in enumerate(np.asarray(cosets[i], dtype=np.uint64).reshape(4)):
                ks[i][j] = int(limb)
        self._chk(self.lib.typlonk_grand_product_dev(self.h, w, sg, _u64p(be), _u64p(ga), C.byref(ks), log_n, z_out.handle))

    def open_dev(self, poly: DeviceBuffer, m: int, z, q_out: DeviceBuffer | None = None, offset: int = 0) -> np.ndarray:
        """typlonk_open_dev: returns y = p(z) (4 limbs); q_out receives (p - y)/(X - z) when given"""
        zz = np.ascontiguousarray(z, dtype=np.uint64).reshape(4)
        y = np.zeros(4, dtype=np.uint64)
        self._chk(self.lib.typlonk_open_dev(self.h, poly.handle, offset, m, _u64p(zz), q_out.handle if q_out else None,
                                            _u64p(y)))
        return y

    def poly_eval_dev(self, polys, m: int, points, offset: int = 0) -> np.ndarray:
        """typlonk_poly_eval_dev: (len(polys), len(points), 4) u64 -- polys[p] (DeviceBuffers, m coefficients from `offset`)
        evaluated at every point (4-limb Montgomery arrays)"""
        ptrs = (C.c_void_p * max(len(polys), 1))(*[b.handle.value for b in polys])
        pts = np.ascontiguousarray(_as_u64(points, 4))
        out = np.zeros((max(len(polys), 1), max(pts.shape[0], 1), 4), dtype=np.uint64)
        self._chk(self.lib.typlonk_poly_eval_dev(self.h, ptrs, len(polys), offset, m, _u64p(pts), pts.shape[0], _u64p(out)))
        return out

    def circuit_commitments(self, sid: int, circuit: int):
        """typlonk_circuit_commitments: [(xy[12], inf)] * 8 -- [q_l] [q_r] [q_o] [q_m] [q_c] [sigma_1] [sigma_2] [sigma_3].
        On an SRS shard with a communicator: a COLLECTIVE (one fold of 8 records) every rank must call; every rank gets the
        whole-SRS commitments."""
        xy = np.zeros((8, 12), dtype=np.uint64)
        inf = np.zeros(8, dtype=np.uint8)
        self._chk(self.lib.typlonk_circuit_commitments(self.h, sid, circuit, _u64p(xy), _u8p(inf)))
        return [(xy[i].copy(), int(inf[i])) for i in range(8)]

    @staticmethod
    def proof_struct(d) -> "Proof":
        """a prove_native dict -> typlonk_proof (beta / gamma / alpha are not needed by the verifier and stay zero)"""
        pr = Proof()
        for i, (xy, f) in enumerate(d["commit"]):
            pr.commit_xy[i][:] = [int(v) for v in np.asarray(xy, dtype=np.uint64).reshape(12)]
            pr.commit_inf[i] = int(f)
        pr.z_xy[:] = [int(v) for v in np.asarray(d["z_commit"][0], dtype=np.uint64).reshape(12)]
        pr.z_inf = int(d["z_commit"][1])
        for i, (xy, f) in enumerate(d["t_commit"]):
            pr.tail.t_xy[i][:] = [int(v) for v in np.asarray(xy, dtype=np.uint64).reshape(12)]
            pr.tail.t_inf[i] = int(f)
        for i, (xy, f) in enumerate(d["witness"]):
            pr.tail.w_xy[i][:] = [int(v) for v in np.asarray(xy, dtype=np.uint64).reshape(12)]
            pr.tail.w_inf[i] = int(f)
        for i, e in enumerate(d["evals"]):
            pr.tail.evals[i][:] = [int(v) for v in np.asarray(e, dtype=np.uint64).reshape(4)]
        pr.zeta[:] = [int(v) for v in np.asarray(d["challenges"]["zeta"], dtype=np.uint64).reshape(4)]
        return pr

    def verify(self, sid: int, circuit: int, g2s_xy, cosets, proofs, pi=None, pi_as_prover: bool = False) -> np.ndarray:
        """typlonk_verify: proofs = dicts as prove_native returns them (or Proof structs); g2s_xy = 24 limbs of [s]G2
        (x.c0 x.c1 y.c0 y.c1); pi = None or one entry per proof, each None or an (l, 4) u64 column (l <= n, zero-padded).
        Returns a bool array, True = accepted."""
        k = len(proofs)
        arr = (Proof * max(k, 1))()
        for i, p in enumerate(proofs):
            arr[i] = p if isinstance(p, Proof) else self.proof_struct(p)
        g2 = np.ascontiguousarray(g2s_xy, dtype=np.uint64).reshape(24)
        ks = ((C.c_uint64 * 4) * 3)()
        for i in range(3):
            for j, limb in enumerate(np.asarray(cosets[i], dtype=np.uint64).reshape(4)):
                ks[i][j] = int(limb)
        keep, pip, lens = [], None, None
        if pi is not None:
            pip = (C.POINTER(C.c_uint64) * max(k, 1))()
            lens = (C.c_size_t * max(k, 1))()
            for i, col in enumerate(pi):
                if col is None:
                    continue
                c = np.ascontiguousarray(_as_u64(col, 4))
                keep.append(c)
                pip[i] = _u64p(c)
                lens[i] = c.shape[0]
        ok = np.zeros(max(k, 1), dtype=np.uint8)
        self._chk(self.lib.typlonk_verify(self.h, sid, circuit, _u64p(g2), C.byref(ks), arr, k, pip, lens,
                                          VERIFY_PI_AS_PROVER if pi_as_prover else 0, _u8p(ok)))
        return ok[:k].astype(bool)

    # ---- the compact proof shape (include/typlonk.h, typlonk_prove_compact) ----------------------------------------------
    def circuit_vk(self, sid: int, circuit: int, cosets, g2s_xy) -> Vk:
        """typlonk_circuit_vk: the verifying key (the cached circuit commitments, SRS point 0, the cosets, [s]G2).
        On an SRS shard with a communicator this is a COLLECTIVE every rank must call: one fold of 9 records (the ranks'
        partial sums of the eight commitments and the P0 record of the rank that holds index 0); every rank gets the key one
        context with the whole SRS returns.  A shard without a communicator is refused (ERR_INVALID_ARG)."""
        vk = Vk()
        g2 = np.ascontiguousarray(g2s_xy, dtype=np.uint64).reshape(24)
        self._chk(self.lib.typlonk_circuit_vk(self.h, sid, circuit, C.byref(_cosets_arg(cosets)), _u64p(g2), C.byref(vk)))
        return vk

    def _prove_compact(self, rc: int, pr: ProofCompact) -> dict:
        """a compact_dict; TYPLONK_ERR_UNSATISFIED raises with the filled proof attached as .proof"""
        d = compact_dict(pr)
        if rc == ERR_UNSATISFIED:
            err = TyplonkError(rc, self.lib.typlonk_strerror(rc).decode() + ": " + self.lib.typlonk_last_error(self.h).decode())
            err.proof = d
            raise err
        self._chk(rc)
        return d

    def prove_compact(self, sid: int, circuit: int, wire_evals, pi=None, pi_len: int | None = None, cosets=None) -> dict:
        """typlonk_prove_compact: wire_evals = [a, b, c] DeviceBuffers; pi = a DeviceBuffer of >= pi_len public values (pi_len
        defaults to its length) or None.  Returns compact_dict(proof).
        On an SRS shard with a communicator (comm_init) the call is a COLLECTIVE: four folds of 12, 1, 3 and 2 records, the same
        proof on every rank as from one context with the whole SRS.  A rank whose call fails raises its own error, its peers
        ERR_COMM naming it, all at the same fold; ERR_UNSATISFIED is raised on every rank with the same filled .proof."""
        w = (C.c_void_p * 3)(*[b.handle.value for b in wire_evals])
        if pi_len is None:
            pi_len = pi.n if pi is not None else 0
        pr = ProofCompact()
        rc = self.lib.typlonk_prove_compact(self.h, sid, circuit, w, pi.handle if pi is not None else None, pi_len,
                                            C.byref(_cosets_arg(cosets)), C.byref(pr))
        return self._prove_compact(rc, pr)

    def prove_compact_host(self, sid: int, circuit: int, wire_evals_host, pi=None, cosets=None) -> dict:
        """typlonk_prove_compact_host: three (n, 4) u64 host columns of equal length, pi = None or an (l, 4) column of l public
        values.  The row count is passed on and checked against the circuit's n by the library.  On an SRS shard with a
        communicator: the same collective as prove_compact."""
        cols = [np.ascontiguousarray(w, dtype=np.uint64) for w in wire_evals_host]
        if len(cols) != 3 or any(c.ndim != 2 or c.shape[1] != 4 or c.shape != cols[0].shape for c in cols):
            raise ValueError("prove_compact_host needs three (rows, 4) uint64 columns of equal length")
        w = (C.POINTER(C.c_uint64) * 3)(*[_u64p(c) for c in cols])
        pic = None
        if pi is not None:
            pic = np.ascontiguousarray(pi, dtype=np.uint64)
            if pic.ndim != 2 or pic.shape[1] != 4:
                raise ValueError("pi must be an (l, 4) uint64 column")
        pr = ProofCompact()
        rc = self.lib.typlonk_prove_compact_host(self.h, sid, circuit, w, cols[0].shape[0],
                                                 _u64p(pic) if pic is not None and pic.shape[0] else None,
                                                 pic.shape[0] if pic is not None else 0, C.byref(_cosets_arg(cosets)), C.byref(pr))
        return self._prove_compact(rc, pr)

    def verify_compact(self, vk: Vk, proofs, pi=None) -> np.ndarray:
        """typlonk_verify_compact: proofs = compact dicts (or ProofCompact structs); pi = None or one entry per proof, each
        None or an (l, 4) column of its public values.  Needs no SRS and no loaded circuit.  Returns a bool array."""
        k = len(proofs)
        arr = (ProofCompact * max(k, 1))()
        for i, p in enumerate(proofs):
            arr[i] = compact_struct(p)
        keep, pip, lens = _pi_arg(pi, k)  # noqa: F841 (keep: the columns stay alive across the call)
        ok = np.zeros(max(k, 1), dtype=np.uint8)
        self._chk(self.lib.typlonk_verify_compact(self.h, C.byref(vk), arr, k, pip, lens, _u8p(ok)))
        return ok[:k].astype(bool)

    def lincomb_dev(self, polys, scalars, n: int, out: DeviceBuffer, constant=None):
        k = len(polys)
        ptrs = (C.c_void_p * max(k, 1))(*[b.handle.value for b in polys])
        sc = ((C.c_uint64 * 4) * max(k, 1))()
        for i, s in enumerate(scalars):
            for j, limb in enumerate(np.asarray(s, dtype=np.uint64).reshape(4)):
                sc[i][j] = int(limb)
        cp = None
        if constant is not None:
            cc = np.ascontiguousarray(constant, dtype=np.uint64).reshape(4)
            cp = _u64p(cc)
        self._chk(self.lib.typlonk_lincomb_dev(self.h, ptrs, sc, k, cp, n, out.handle))

    def prove(self, sid: int, circuit: int, wire_evals, pi_evals, cosets, challenge12=None, challenge34=None,
              challenge_v=None, fold=None):
        """Three-round prover session.  challenge12(commitments) -> (beta, gamma) and
        challenge34(commitments + [Z]) -> (alpha, zeta) are callables returning 4-limb arrays (the
        caller's Fiat-Shamir).  Returns a dict of numpy arrays in the C-ABI form.
        challenge_v(evals) -> v selects the batched-opening shape (round3_evals + round4_batched):
        "witness" then holds [W at zeta of a + v b + v^2 c + v^3 Z + v^4 r, W of Z at zeta*w].
        fold(points) -> points combines per-rank partial commitments when `sid` is an SRS shard
        (typlonk_srs_set_shard): one all-gather + fixed-order sum per round (typlonk_amd.dist.ShardedProver).
        Raises TyplonkError(ERR_UNSATISFIED) when r(zeta) != 0, i.e. the witness does not satisfy the circuit (the
        reference panics in vanishes() or hands its verifier a proof it rejects, plonk/src/proof.rs:321, 361, 234)."""
        fold = fold or (lambda pts: pts)
        if challenge12 is None or challenge34 is None:
            # the reference's own Fiat-Shamir (plonk/src/proof/challenges.rs), native: csrc/transcript.hpp
            challenge12 = challenge12 or (lambda pts: transcript_challenges(pts, 2))
            challenge34 = challenge34 or (lambda pts: transcript_challenges(pts, 2))
        lib = self.lib
        w = (C.c_void_p * 3)(*[b.handle.value for b in wire_evals])
        pr = C.c_void_p()
        cxy = ((C.c_uint64 * 12) * 3)()
        cinf = (C.c_uint8 * 3)()
        self._chk(lib.typlonk_prover_round1(self.h, sid, circuit, w, pi_evals.handle if pi_evals is not None else None,
                                            C.byref(pr), C.byref(cxy), C.byref(cinf)))
        try:
            commits = fold([(np.array(cxy[i], dtype=np.uint64), int(cinf[i])) for i in range(3)])
            beta, gamma = [np.ascontiguousarray(x, dtype=np.uint64).reshape(4) for x in challenge12(commits)]
            ks = ((C.c_uint64 * 4) * 3)()
            for i in range(3):
                for j, limb in enumerate(np.asarray(cosets[i], dtype=np.uint64).reshape(4)):
                    ks[i][j] = int(limb)
            zxy = np.zeros(12, dtype=np.uint64)
            zinf = np.zeros(1, dtype=np.uint8)
            self._chk(lib.typlonk_prover_round2(pr, _u64p(beta), _u64p(gamma), C.byref(ks), _u64p(zxy), _u8p(zinf)))
            (zxy, zi), = fold([(zxy, int(zinf[0]))])
            zinf[0] = zi
            alpha, zeta = [np.ascontiguousarray(x, dtype=np.uint64).reshape(4)
                           for x in challenge34(commits + [(zxy, int(zinf[0]))])]
            if challenge_v is not None:
                pe = ProofEvals()
                self._chk(lib.typlonk_prover_round3_evals(pr, _u64p(alpha), _u64p(zeta), C.byref(pe)))
                evals = [np.array(pe.evals[i], dtype=np.uint64) for i in range(6)]
                v = np.ascontiguousarray(challenge_v(evals), dtype=np.uint64).reshape(4)
                pb = ProofBatched()
                self._chk(lib.typlonk_prover_round4_batched(pr, _u64p(v), C.byref(pb)))
                tw = fold([(np.array(pb.t_xy[i], dtype=np.uint64), int(pb.t_inf[i])) for i in range(3)] +
                          [(np.array(pb.w_xy[i], dtype=np.uint64), int(pb.w_inf[i])) for i in range(2)])
                return {
                    "commit": commits, "z_commit": (zxy, int(zinf[0])), "t_commit": tw[:3], "witness": tw[3:],
                    "evals": evals, "batched": True,
                }
            tail = ProofTail()
            self._chk(lib.typlonk_prover_round3(pr, _u64p(alpha), _u64p(zeta), C.byref(tail)))
        finally:
            lib.typlonk_prover_free(pr)
        tw = fold([(np.array(tail.t_xy[i], dtype=np.uint64), int(tail.t_inf[i])) for i in range(3)] +
                  [(np.array(tail.w_xy[i], dtype=np.uint64), int(tail.w_inf[i])) for i in range(6)])
        return {
            "commit": commits, "z_commit": (zxy, int(zinf[0])), "t_commit": tw[:3], "witness": tw[3:],
            "evals": [np.array(tail.evals[i], dtype=np.uint64) for i in range(6)],
        }

    def prove_native(self, sid: int, circuit: int, wire_evals, pi_evals, cosets):
        """typlonk_prove: the whole prove() in one native call, transcript included.  Same dict as prove() plus the
        challenges; raises TyplonkError(ERR_UNSATISFIED) for a witness that does not satisfy the circuit."""
        w = (C.c_void_p * 3)(*[b.handle.value for b in wire_evals])
        ks = ((C.c_uint64 * 4) * 3)()
        for i in range(3):
            for j, limb in enumerate(np.asarray(cosets[i], dtype=np.uint64).reshape(4)):
                ks[i][j] = int(limb)
        pr = Proof()
        self._chk(self.lib.typlonk_prove(self.h, sid, circuit, w, pi_evals.handle if pi_evals is not None else None,
                                         C.byref(ks), C.byref(pr)))
        t = pr.tail
        return {
            "commit": [(np.array(pr.commit_xy[i], dtype=np.uint64), int(pr.commit_inf[i])) for i in range(3)],
            "z_commit": (np.array(pr.z_xy, dtype=np.uint64), int(pr.z_inf)),
            "t_commit": [(np.array(t.t_xy[i], dtype=np.uint64), int(t.t_inf[i])) for i in range(3)],
            "witness": [(np.array(t.w_xy[i], dtype=np.uint64), int(t.w_inf[i])) for i in range(6)],
            "evals": [np.array(t.evals[i], dtype=np.uint64) for i in range(6)],
            "challenges": {k: np.array(getattr(pr, k), dtype=np.uint64) for k in ("beta", "gamma", "alpha", "zeta")},
        }

    def prove_native_host(self, sid: int, circuit: int, wire_evals_host, pi_evals_host, cosets):
        """typlonk_prove_host: the columns are (n, 4) u64 arrays in host memory; uploaded column by column beside round 1"""
        cols = [np.ascontiguousarray(_as_u64(w, 4)) for w in wire_evals_host]
        w = (C.POINTER(C.c_uint64) * 3)(*[_u64p(c) for c in cols])
        pi = np.ascontiguousarray(_as_u64(pi_evals_host, 4)) if pi_evals_host is not None else None
        ks = ((C.c_uint64 * 4) * 3)()
        for i in range(3):
            for j, limb in enumerate(np.asarray(cosets[i], dtype=np.uint64).reshape(4)):
                ks[i][j] = int(limb)
        pr = Proof()
        self._chk(self.lib.typlonk_prove_host(self.h, sid, circuit, w, _u64p(pi) if pi is not None else None, C.byref(ks), C.byref(pr)))
        t = pr.tail
        return {
            "commit": [(np.array(pr.commit_xy[i], dtype=np.uint64), int(pr.commit_inf[i])) for i in range(3)],
            "z_commit": (np.array(pr.z_xy, dtype=np.uint64), int(pr.z_inf)),
            "t_commit": [(np.array(t.t_xy[i], dtype=np.uint64), int(t.t_inf[i])) for i in range(3)],
            "witness": [(np.array(t.w_xy[i], dtype=np.uint64), int(t.w_inf[i])) for i in range(6)],
            "evals": [np.array(t.evals[i], dtype=np.uint64) for i in range(6)],
            "challenges": {k: np.array(getattr(pr, k), dtype=np.uint64) for k in ("beta", "gamma", "alpha", "zeta")},
        }

    @staticmethod
    def _proof_dict(pr) -> dict:
        t = pr.tail
        return {
            "commit": [(np.array(pr.commit_xy[i], dtype=np.uint64), int(pr.commit_inf[i])) for i in range(3)],
            "z_commit": (np.array(pr.z_xy, dtype=np.uint64), int(pr.z_inf)),
            "t_commit": [(np.array(t.t_xy[i], dtype=np.uint64), int(t.t_inf[i])) for i in range(3)],
            "witness": [(np.array(t.w_xy[i], dtype=np.uint64), int(t.w_inf[i])) for i in range(6)],
            "evals": [np.array(t.evals[i], dtype=np.uint64) for i in range(6)],
            "challenges": {k: np.array(getattr(pr, k), dtype=np.uint64) for k in ("beta", "gamma", "alpha", "zeta")},
        }

    def prove_batch(self, sid: int, circuit: int, wire_evals, pi_evals, cosets):
        """typlonk_prove_batch: wire_evals = one [a, b, c] list of DeviceBuffers per proof; pi_evals = None or one entry per
        proof (a DeviceBuffer or None).  Returns (proofs, statuses): the dicts prove_native returns, and per proof OK or
        ERR_UNSATISFIED (that proof's dict is filled all the same)."""
        k = len(wire_evals)
        w = (C.c_void_p * max(3 * k, 1))(*[b.handle.value for cols in wire_evals for b in cols])
        pi = None
        if pi_evals is not None:
            pi = (C.c_void_p * max(k, 1))(*[b.handle.value if b is not None else None for b in pi_evals])
        return self._prove_batch(self.lib.typlonk_prove_batch, sid, circuit, w, pi, k, cosets)

    def prove_batch_host(self, sid: int, circuit: int, wire_evals_host, pi_evals_host, cosets):
        """typlonk_prove_batch_host: the columns are (n, 4) u64 host arrays, one [a, b, c] list per proof; pi_evals_host =
        None or one entry per proof (an array or None).  Same result as prove_batch."""
        k = len(wire_evals_host)
        keep = [np.ascontiguousarray(_as_u64(c, 4)) for cols in wire_evals_host for c in cols]
        w = (C.POINTER(C.c_uint64) * max(3 * k, 1))(*[_u64p(c) for c in keep])
        pi = None
        if pi_evals_host is not None:
            pis = [np.ascontiguousarray(_as_u64(c, 4)) if c is not None else None for c in pi_evals_host]
            keep += [c for c in pis if c is not None]
            pi = (C.POINTER(C.c_uint64) * max(k, 1))(*[_u64p(c) if c is not None else None for c in pis])
        return self._prove_batch(self.lib.typlonk_prove_batch_host, sid, circuit, w, pi, k, cosets)

    def _prove_batch(self, fn, sid, circuit, w, pi, k, cosets):
        ks = ((C.c_uint64 * 4) * 3)()
        for i in range(3):
            for j, limb in enumerate(np.asarray(cosets[i], dtype=np.uint64).reshape(4)):
                ks[i][j] = int(limb)
        out = (Proof * max(k, 1))()
        st = (C.c_int * max(k, 1))()
        self._chk(fn(self.h, sid, circuit, w, pi, k, C.byref(ks), out, st))
        return [self._proof_dict(out[i]) for i in range(k)], [int(st[i]) for i in range(k)]

    def prove_batch_compact(self, sid: int, circuit: int, wire_evals, pi=None, pi_len=None, cosets=None):
        """typlonk_prove_batch_compact: wire_evals = one [a, b, c] list of DeviceBuffers per proof; pi = None or one entry per
        proof (a DeviceBuffer of >= pi_len[k] public values, or None); pi_len = None (each buffer's length, 0 for None) or
        one count per proof.  Returns (proofs, statuses): one compact_dict per proof as prove_compact returns it, and per
        proof OK or ERR_UNSATISFIED (that proof's dict is filled all the same)."""
        k = len(wire_evals)
        w = (C.c_void_p * max(3 * k, 1))(*[b.handle.value for cols in wire_evals for b in cols])
        pip = None
        if pi is not None:
            pip = (C.c_void_p * max(k, 1))(*[b.handle.value if b is not None else None for b in pi])
        if pi_len is None and pi is not None:
            pi_len = [b.n if b is not None else 0 for b in pi]
        lens = (C.c_size_t * max(k, 1))(*[int(x) for x in pi_len]) if pi_len is not None else None
        out = (ProofCompact * max(k, 1))()
        st = (C.c_int * max(k, 1))()
        self._chk(self.lib.typlonk_prove_batch_compact(self.h, sid, circuit, w, pip, lens, k, C.byref(_cosets_arg(cosets)), out, st))
        return [compact_dict(out[i]) for i in range(k)], [int(st[i]) for i in range(k)]

    def prove_batch_compact_host(self, sid: int, circuit: int, wire_evals_host, pi=None, cosets=None):
        """typlonk_prove_batch_compact_host: the columns are (rows, 4) u64 host arrays of equal length, one [a, b, c] list per
        proof; pi = None or one entry per proof (None or an (l, 4) column of l public values).  The row count is passed on and
        checked against the circuit's n by the library.  Same result as prove_batch_compact."""
        k = len(wire_evals_host)
        keep = [np.ascontiguousarray(c, dtype=np.uint64) for cols in wire_evals_host for c in cols]
        if any(c.ndim != 2 or c.shape[1] != 4 or c.shape != keep[0].shape for c in keep):
            raise ValueError("prove_batch_compact_host needs (rows, 4) uint64 columns of equal length")
        w = (C.POINTER(C.c_uint64) * max(3 * k, 1))(*[_u64p(c) for c in keep])
        pip = lens = None
        if pi is not None:
            pis = [np.ascontiguousarray(c, dtype=np.uint64) if c is not None else None for c in pi]
            if any(c is not None and (c.ndim != 2 or c.shape[1] != 4) for c in pis):
                raise ValueError("pi entries must be (l, 4) uint64 columns")
            keep += [c for c in pis if c is not None]
            pip = (C.POINTER(C.c_uint64) * max(k, 1))(*[_u64p(c) if c is not None and c.shape[0] else None for c in pis])
            lens = (C.c_size_t * max(k, 1))(*[c.shape[0] if c is not None else 0 for c in pis])
        out = (ProofCompact * max(k, 1))()
        st = (C.c_int * max(k, 1))()
        self._chk(self.lib.typlonk_prove_batch_compact_host(self.h, sid, circuit, w, keep[0].shape[0] if keep else 0, pip, lens, k,
                                                            C.byref(_cosets_arg(cosets)), out, st))
        return [compact_dict(out[i]) for i in range(k)], [int(st[i]) for i in range(k)]

    # ---- witness check --------------------------------------------------------------------
    def circuit_permutation(self, circuit: int, n: int, cosets):
        """typlonk_circuit_permutation: (perm, defects) -- the 3n-entry successor map over flat cells col * n + row recovered
        from the circuit's sigma columns (CELL_NONE where a sigma value is no cell id), and the number of defects"""
        perm = np.empty(3 * n, dtype=np.uint32)
        defects = C.c_uint64()
        self._chk(self.lib.typlonk_circuit_permutation(self.h, circuit, C.byref(_cosets_arg(cosets)),
                                                       perm.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(defects)))
        return perm, int(defects.value)

    @staticmethod
    def _witness_reports(k, cap, reports, gate, copy):
        out = []
        for i in range(k):
            r = reports[i]
            out.append({"gate_failures": int(r.gate_failures), "copy_failures": int(r.copy_failures),
                        "gate_rows": [int(x) for x in gate[i * cap:i * cap + r.gate_listed]],
                        "copy_cells": [(int(copy[2 * (i * cap + j)]), int(copy[2 * (i * cap + j) + 1])) for j in range(r.copy_listed)]})
        return out

    def witness_check(self, circuit: int, wire_evals, pi=None, pi_len=None, cosets=None, cap: int = 16):
        """typlonk_witness_check: wire_evals / pi / pi_len as prove_batch_compact.  One dict per witness: gate_failures,
        copy_failures (totals), gate_rows (the lowest failing rows, at most cap) and copy_cells (the lowest failing cells as
        (x, perm[x]) pairs, at most cap).  A witness satisfies the circuit exactly when both counts are 0."""
        k = len(wire_evals)
        w = (C.c_void_p * max(3 * k, 1))(*[b.handle.value for cols in wire_evals for b in cols])
        pip = None
        if pi is not None:
            pip = (C.c_void_p * max(k, 1))(*[b.handle.value if b is not None else None for b in pi])
        if pi_len is None and pi is not None:
            pi_len = [b.n if b is not None else 0 for b in pi]
        lens = (C.c_size_t * max(k, 1))(*[int(x) for x in pi_len]) if pi_len is not None else None
        reports = (WitnessReport * max(k, 1))()
        gate = (C.c_uint32 * max(k * cap, 1))()
        copy = (C.c_uint32 * max(2 * k * cap, 1))()
        self._chk(self.lib.typlonk_witness_check(self.h, circuit, w, pip, lens, k, C.byref(_cosets_arg(cosets)), cap, reports,
                                                 gate if cap else None, copy if cap else None))
        return self._witness_reports(k, cap, reports, gate, copy)

    def witness_check_host(self, circuit: int, wire_evals_host, pi=None, cosets=None, cap: int = 16):
        """typlonk_witness_check_host: the columns are (rows, 4) u64 host arrays of equal length, one [a, b, c] list per witness;
        pi = None or one entry per witness (None or an (l, 4) column of l public values).  Same result as witness_check."""
        k = len(wire_evals_host)
        keep = [np.ascontiguousarray(c, dtype=np.uint64) for cols in wire_evals_host for c in cols]
        if any(c.ndim != 2 or c.shape[1] != 4 or c.shape != keep[0].shape for c in keep):
            raise ValueError("witness_check_host needs (rows, 4) uint64 columns of equal length")
        w = (C.POINTER(C.c_uint64) * max(3 * k, 1))(*[_u64p(c) for c in keep])
        pip = lens = None
        if pi is not None:
            pis = [np.ascontiguousarray(c, dtype=np.uint64) if c is not None else None for c in pi]
            if any(c is not None and (c.ndim != 2 or c.shape[1] != 4) for c in pis):
                raise ValueError("pi entries must be (l, 4) uint64 columns")
            keep += [c for c in pis if c is not None]
            pip = (C.POINTER(C.c_uint64) * max(k, 1))(*[_u64p(c) if c is not None and c.shape[0] else None for c in pis])
            lens = (C.c_size_t * max(k, 1))(*[c.shape[0] if c is not None else 0 for c in pis])
        reports = (WitnessReport * max(k, 1))()
        gate = (C.c_uint32 * max(k * cap, 1))()
        copy = (C.c_uint32 * max(2 * k * cap, 1))()
        self._chk(self.lib.typlonk_witness_check_host(self.h, circuit, w, keep[0].shape[0] if keep else 0, pip, lens, k,
                                                      C.byref(_cosets_arg(cosets)), cap, reports, gate if cap else None,
                                                      copy if cap else None))
        return self._witness_reports(k, cap, reports, gate, copy)

    # ---- witness solve --------------------------------------------------------------------
    def witness_solve_plan(self, circuit: int, cosets) -> dict:
        """typlonk_witness_solve_plan: the plan of a solve of this circuit under these cosets (built on first use, cached with the
        circuit) as a dict: driven_rows, free_classes, depth (levels) and launches (kernel launches per solve)"""
        info = SolveInfo()
        self._chk(self.lib.typlonk_witness_solve_plan(self.h, circuit, C.byref(_cosets_arg(cosets)), C.byref(info)))
        return {"driven_rows": int(info.driven_rows), "free_classes": int(info.free_classes), "depth": int(info.depth),
                "launches": int(info.launches)}

    def circuit_set_hints(self, circuit: int, cosets, hints) -> None:
        """typlonk_circuit_set_hints: hints = (kind, dst, src, shift, width) tuples (kind HINT_INV0 or HINT_BITS; dst, src flat
        cells); replaces the circuit's whole set, an empty list removes it.  The solve plan is built at once: every refusal is
        raised here, and a refused call leaves the installed hints in force.  A numpy array of HINT_DTYPE is passed as it is."""
        if isinstance(hints, np.ndarray):
            keep = np.ascontiguousarray(hints, dtype=HINT_DTYPE)
            arr = keep.ctypes.data_as(C.POINTER(Hint))
        else:
            arr = (Hint * max(len(hints), 1))(*[Hint(*[int(v) for v in h]) for h in hints])
        self._chk(self.lib.typlonk_circuit_set_hints(self.h, circuit, C.byref(_cosets_arg(cosets)), arr if len(hints) else None,
                                                     len(hints)))

    def witness_solve(self, circuit: int, cosets, cells, values, wire_out, pi=None, pi_len=None) -> None:
        """typlonk_witness_solve: cells = the flat indices of the assigned cells (shared by all witnesses); values = a
        (count, len(cells), 4) u64 array of canonical Montgomery limbs, witness-major; wire_out = one [a, b, c] list of buffers
        (>= n elements each) per witness, written in place; pi / pi_len as witness_check."""
        k = len(wire_out)
        cl = np.ascontiguousarray(cells, dtype=np.uint32)
        vals = np.ascontiguousarray(values, dtype=np.uint64)
        if vals.size != k * cl.size * 4:
            raise ValueError("witness_solve needs count * len(cells) * 4 value limbs")
        w = (C.c_void_p * max(3 * k, 1))(*[b.handle.value for cols in wire_out for b in cols])
        pip = None
        if pi is not None:
            pip = (C.c_void_p * max(k, 1))(*[b.handle.value if b is not None else None for b in pi])
        if pi_len is None and pi is not None:
            pi_len = [b.n if b is not None else 0 for b in pi]
        lens = (C.c_size_t * max(k, 1))(*[int(x) for x in pi_len]) if pi_len is not None else None
        self._chk(self.lib.typlonk_witness_solve(self.h, circuit, C.byref(_cosets_arg(cosets)),
                                                 cl.ctypes.data_as(C.POINTER(C.c_uint32)) if cl.size else None, cl.size,
                                                 _u64p(vals) if vals.size else None, pip, lens, k, w))

    def circuit_load(self, log_n: int, selectors, sigma) -> int:
        sel = (C.c_void_p * 5)(*[b.handle.value for b in selectors])
        sig = (C.c_void_p * 3)(*[b.handle.value for b in sigma])
        cid = C.c_uint32()
        self._chk(self.lib.typlonk_circuit_load(self.h, sel, sig, log_n, C.byref(cid)))
        return cid.value

    DEFAULT_COSETS = (2, 3, 4)   # Permutation::compile's (permutation/src/lib.rs:141-154)

    def _compile_args(self, log_n: int, perm, cosets):
        """(keep-alive, perm pointer or None, cosets) of circuit_compile / circuit_compile_host"""
        if cosets is None:
            r = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
            cosets = [np.array([((k << 256) % r >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
                      for k in self.DEFAULT_COSETS]
        pp, keep = None, None
        if perm is not None:
            keep = np.ascontiguousarray(perm, dtype=np.uint32)
            if keep.shape != (3 << log_n,):
                raise ValueError("perm holds 3n successors over the flat cells col * n + row")
            pp = keep.ctypes.data_as(C.POINTER(C.c_uint32))
        return keep, pp, _cosets_arg(cosets)

    def circuit_compile(self, log_n: int, selector_evals, perm=None, cosets=None) -> int:
        """typlonk_circuit_compile: the circuit of five DeviceBuffers of selector evaluations (q_l q_r q_o q_m q_c) and the
        3n-entry successor map `perm` over the flat cells col * n + row (None: no copy constraints); cosets = three 4-limb
        Montgomery arrays (None: 2, 3, 4).  Returns the circuit id; a perm that is no permutation of the cells raises, with
        the number of defects and the lowest defective cell in the message (typlonk_last_error's)."""
        keep, pp, ks = self._compile_args(log_n, perm, cosets)
        sel = (C.c_void_p * 5)(*[b.handle.value for b in selector_evals])
        cid, defects = C.c_uint32(), C.c_uint64()
        self._chk(self.lib.typlonk_circuit_compile(self.h, sel, pp, C.byref(ks), log_n, C.byref(cid), C.byref(defects)))
        return cid.value

    def circuit_compile_host(self, log_n: int, selector_evals, perm=None, cosets=None) -> int:
        """typlonk_circuit_compile_host: the selector evaluations as five (rows, 4) u64 host arrays of equal length"""
        keep, pp, ks = self._compile_args(log_n, perm, cosets)
        cols = [np.ascontiguousarray(c, dtype=np.uint64) for c in selector_evals]
        if len(cols) != 5 or any(c.ndim != 2 or c.shape[1] != 4 or c.shape != cols[0].shape for c in cols):
            raise ValueError("circuit_compile_host needs five (rows, 4) uint64 columns of equal length")
        sel = (C.POINTER(C.c_uint64) * 5)(*[_u64p(c) for c in cols])
        cid, defects = C.c_uint32(), C.c_uint64()
        self._chk(self.lib.typlonk_circuit_compile_host(self.h, sel, cols[0].shape[0], pp, C.byref(ks), log_n, C.byref(cid),
                                                        C.byref(defects)))
        return cid.value

    @staticmethod
    def _pairs_arg(pairs):
        """(keep-alive, pointer or None, count) of a pair list: anything np.ascontiguousarray(..., dtype=np.uint32) turns into
        shape (count, 2)"""
        keep = np.ascontiguousarray(pairs, dtype=np.uint32)
        if keep.ndim != 2 or keep.shape[1] != 2:
            raise ValueError("pairs must have shape (count, 2): two flat cells col * n + row per copy constraint")
        return keep, (keep.ctypes.data_as(C.POINTER(C.c_uint32)) if keep.shape[0] else None), keep.shape[0]

    def permutation_from_pairs(self, log_n: int, pairs):
        """typlonk_permutation_from_pairs: (perm, classes) -- the canonical 3n-entry successor map of the partition the pairs
        of flat cells generate (every class ascending, its highest cell back to its lowest) and the number of classes.  A pair
        that names a cell >= 3n raises, with the count of bad pairs, the lowest bad pair and its cell in the message."""
        keep, pp, count = self._pairs_arg(pairs)
        perm = np.empty(3 << log_n if 1 <= log_n <= 24 else 0, dtype=np.uint32)   # (any other log_n is refused before perm is touched)
        classes = C.c_uint64()
        self._chk(self.lib.typlonk_permutation_from_pairs(self.h, pp, count, log_n, perm.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                          C.byref(classes)))
        return perm, int(classes.value)

    def circuit_compile_pairs(self, log_n: int, selector_evals, pairs, cosets=None):
        """typlonk_circuit_compile_pairs: (circuit id, classes) -- circuit_compile from copy constraints given as pairs of flat
        cells; the permutation is made and kept on the device"""
        keep, pp, count = self._pairs_arg(pairs)
        _, _, ks = self._compile_args(log_n, None, cosets)
        sel = (C.c_void_p * 5)(*[b.handle.value for b in selector_evals])
        cid, classes = C.c_uint32(), C.c_uint64()
        self._chk(self.lib.typlonk_circuit_compile_pairs(self.h, sel, pp, count, C.byref(ks), log_n, C.byref(cid), C.byref(classes)))
        return cid.value, int(classes.value)

    def circuit_compile_pairs_host(self, log_n: int, selector_evals, pairs, cosets=None):
        """typlonk_circuit_compile_pairs_host: the selector evaluations as five (rows, 4) u64 host arrays of equal length"""
        keep, pp, count = self._pairs_arg(pairs)
        _, _, ks = self._compile_args(log_n, None, cosets)
        cols = [np.ascontiguousarray(c, dtype=np.uint64) for c in selector_evals]
        if len(cols) != 5 or any(c.ndim != 2 or c.shape[1] != 4 or c.shape != cols[0].shape for c in cols):
            raise ValueError("circuit_compile_pairs_host needs five (rows, 4) uint64 columns of equal length")
        sel = (C.POINTER(C.c_uint64) * 5)(*[_u64p(c) for c in cols])
        cid, classes = C.c_uint32(), C.c_uint64()
        self._chk(self.lib.typlonk_circuit_compile_pairs_host(self.h, sel, cols[0].shape[0], pp, count, C.byref(ks), log_n,
                                                              C.byref(cid), C.byref(classes)))
        return cid.value, int(classes.value)

    def circuit_free(self, cid: int):
        self._chk(self.lib.typlonk_circuit_free(self.h, cid))

    def quotient_dev(self, log_n: int, wires, z, selectors, sigma, pi, alpha, beta, gamma, cosets, t_out, circuit=0):
        """typlonk_quotient_dev: all polynomial arguments are DeviceBuffers (n coefficients), scalars are
        4-limb Montgomery arrays; t_out is a DeviceBuffer of >= 4n elements"""
        a = QuotientArgs()
        a.circuit = circuit
        for i in range(3):
            a.wires[i] = wires[i].handle.value
            if not circuit:
                a.sigma[i] = sigma[i].handle.value
        a.z = z.handle.value
        for i in range(5):
            if not circuit:
                a.selectors[i] = selectors[i].handle.value
        a.public_inputs = pi.handle.value if pi is not None else None
        for name, val in (("alpha", alpha), ("beta", beta), ("gamma", gamma)):
            arr = getattr(a, name)
            for j, limb in enumerate(np.asarray(val, dtype=np.uint64).reshape(4)):
                arr[j] = int(limb)
        for i in range(3):
            for j, limb in enumerate(np.asarray(cosets[i], dtype=np.uint64).reshape(4)):
                a.cosets[i][j] = int(limb)
        self._chk(self.lib.typlonk_quotient_dev(self.h, C.byref(a), log_n, t_out.handle))

    def alloc(self, n: int) -> DeviceBuffer:
        return DeviceBuffer(self, n)

    # ---- measurement ----------------------------------------------------------------------
    def set_profiling(self, on):
        """False / 0 off, True / 1 every stage, 2 the bucket-accumulation launches only (cheap enough for a timed loop)"""
        self._chk(self.lib.typlonk_set_profiling(self.h, int(on)))

    def profile(self) -> list[tuple[str, float]]:
        cap = 32
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        n = self._chk(self.lib.typlonk_profile_get(self.h, names, ms, cap))
        return [(names[i].decode(), float(ms[i])) for i in range(min(n, cap))]
