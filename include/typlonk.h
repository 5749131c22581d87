/* typlonk.h -- C ABI of libtyplonk_hip.so: MI355X (gfx950) backend for TyPLONK's MSM + NTT hot path.
 *
 * The reference (fabrizio-m/TyPLONK, Rust) has no FFI of its own; these entry points are what a
 * Rust `extern "C"` block would bind to replace the two seams named in SURVEY.md section 8(b):
 *
 *   MSM seam  kzg::KzgScheme::evaluate_in_s            /root/reference/kzg/src/lib.rs:41-54
 *             (reached from commit :37-40, open :55-64, identity :82-85)
 *   SRS       kzg::srs::Srs::g1 / g1_ref               /root/reference/kzg/src/srs.rs:8-12, 43-45
 *   NTT seam  Evaluations::interpolate (ark-poly ifft) /root/reference/plonk/src/proof.rs:50,106,125,128,337,415
 *             DensePolynomial::evaluate_over_domain    /root/reference/plonk/src/proof.rs:115
 *
 * Data formats (all little-endian, exactly arkworks 0.3.0's in-memory form, so a Rust caller passes
 * `fr.0.0` / `pt.x.0.0` with no conversion):
 *   Fr  : 4 x uint64 limbs, Montgomery residue, R = 2^256
 *   Fq  : 6 x uint64 limbs, Montgomery residue, R = 2^384
 *   G1  : 12 x uint64 = x limbs then y limbs, plus a separate flag byte (1 = point at infinity).
 *         The identity is returned as x = 0, y = 1 (Montgomery one), inf = 1 -- ark-ec's
 *         GroupAffine::zero().
 *
 * Conventions: every function returns TYPLONK_OK (0) or a negative error code; the caller owns all
 * host buffers and the library never keeps a host pointer after returning; calls block until the
 * result is on the host unless documented otherwise; one host thread per context.  Results are
 * deterministic and bit-exact (modular integer arithmetic only).
 */
#ifndef TYPLONK_H
#define TYPLONK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TYPLONK_OK 0
#define TYPLONK_ERR_INVALID_ARG (-1)   /* NULL pointer, bad handle                                        */
#define TYPLONK_ERR_LENGTH (-2)        /* m > srs length: the reference's assert!, kzg/src/lib.rs:43      */
#define TYPLONK_ERR_DOMAIN (-3)        /* log_n outside 0..32: the reference's unwrap(), builder.rs:70    */
#define TYPLONK_ERR_NO_DEVICE (-4)     /* no usable HIP device (the library has NO CPU fallback)          */
#define TYPLONK_ERR_HIP (-5)           /* a HIP runtime call failed; see typlonk_last_error               */
#define TYPLONK_ERR_OOM (-6)           /* device allocation failed                                        */
#define TYPLONK_ERR_RANGE (-7)         /* offset/length outside a device buffer                            */
#define TYPLONK_ERR_UNSATISFIED (-8)   /* the witness does not satisfy the circuit: r(zeta) != 0.  The reference
                                          panics (vanishes(), plonk/src/proof.rs:321, 361, 504-507) or produces a
                                          proof its own verifier rejects (:234-235)                          */

#define TYPLONK_ERR_COMM (-9)          /* an RCCL call failed or librccl could not be loaded; see typlonk_last_error */
/* A bound that no input can reach was reached (the walks of typlonk_permutation_from_pairs): reported under
 * TYPLONK_ERR_HIP's code, with the cause in typlonk_last_error. */
#define TYPLONK_ERR_INTERNAL TYPLONK_ERR_HIP

typedef struct typlonk_ctx typlonk_ctx; /* one HIP device + stream + workspaces + cached NTT plans */
typedef struct typlonk_buf typlonk_buf; /* device-resident vector of Fr elements                   */

/* ---- context --------------------------------------------------------------------------------- */
int typlonk_init(typlonk_ctx** out, int device_ordinal);
void typlonk_destroy(typlonk_ctx* ctx);
const char* typlonk_strerror(int code);
const char* typlonk_last_error(const typlonk_ctx* ctx); /* detail text of the last failure on ctx  */
/* Run all subsequent work of `ctx` on an existing hipStream_t (e.g. the caller's torch stream);
 * NULL restores the context's own stream.
 *
 * STREAM ORDERING of device-resident inputs.  Every entry point that reads caller-owned device memory
 * (typlonk_msm_g1_devptr, typlonk_msm_g1_batch_devptr, typlonk_ntt_fr_devptr, typlonk_ntt_fr_batch_devptr, and the typlonk_buf forms when the
 * buffer was written through typlonk_buf_devptr) reads it in the order of the CONTEXT'S STREAM.  The context's own
 * stream is an ordinary (blocking) HIP stream, so it is also ordered after everything previously submitted to the
 * legacy default stream -- which is where PyTorch-ROCm runs unless told otherwise.  A producer on any OTHER stream
 * (a non-blocking stream, a torch side stream) must either be synchronised before the call or be made the
 * context's stream with typlonk_set_stream; otherwise the MSM / NTT may read half-written input. */
int typlonk_set_stream(typlonk_ctx* ctx, void* hip_stream);
int typlonk_sync(typlonk_ctx* ctx);

/* ---- SRS: the fixed MSM base vector ([s^i]G, affine), uploaded once per circuit ---------------- */
/* xy: len*12 limbs; inf: len flag bytes or NULL (= no identity points).  Returns a handle id.  Nothing is validated: points
 * from outside go through typlonk_srs_check (below, "a powers-of-tau step") before they are used. */
int typlonk_srs_load(typlonk_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t len, uint32_t* srs_id);
/* Build g1[i] = [secret^(start+i)] G, i < len, on the device (Srs::from_secret, kzg/src/srs.rs:15-34;
 * `start` lets each GPU create only its shard).  secret: 4 limbs (Montgomery).  Setup-time only. */
int typlonk_srs_generate(typlonk_ctx* ctx, const uint64_t secret[4], uint64_t start, size_t len, uint32_t* srs_id);
/* Copy `count` points starting at `offset` back to the host (xy: count*12 limbs; inf: count or NULL). */
int typlonk_srs_download(typlonk_ctx* ctx, uint32_t srs_id, size_t offset, size_t count, uint64_t* xy, uint8_t* inf);
/* Optional fixed-base precomputation (the SRS is immutable per circuit, plonk/src/lib.rs:22): builds the
 * tables 2^(c*t) * g1[i] for every window t (T = ceil(256/c) copies of the SRS in HBM -- 15 for c = 17 and 17 for
 * c = 15, which slice centred scalars |k| < 2^254 --, c = window_bits in 14..20, or 0 = chosen by length: 15 below
 * 2^16 points, 17 below 2^19 -- an index shard --, else 20, whose top window still has 15 bits; with 0 an SRS shorter than
 * TYPLONK_TABLES_AUTO_MIN_LEN points gets NO tables and the call returns TYPLONK_OK: 2^16 buckets for a handful of
 * terms would be slower than the plain path).  Later MSMs of at least len/4
 * terms over this SRS then let all windows share ONE bucket set: no cross-window doublings on the
 * host, fewer windows, fewer bucket additions.  Results are unchanged bit for bit.  Setup-time cost: T*c Jacobian doublings + ONE shared inversion per point
 * (plus T * len * 48 bytes of scratch for the duration of the call; TYPLONK_ERR_OOM if either allocation is refused).
 * The sort sees an MSM one chunk at a time (queued MSMs in chunks of <= 2^20 terms), so table mode holds for MSMs of any
 * length up to len; an MSM whose largest chunk the table-mode sort cannot handle silently takes the plain path over the
 * same SRS: precomputation never turns a valid MSM into an error.  1 <= len <= 2^25, and every gather index
 * j * len + i (j < T, i < len) must stay below 2^31 (bit 31 carries the sign): T * len <= 2^31, which every window
 * 14..20 meets at 2^25 points.  Any other length returns TYPLONK_ERR_LENGTH.
 * HBM: T * len * 128 bytes for the tables (c = 20: 26.0 GiB at 2^24 + 3 points, 13.0 GiB at 2^23 + 3). */
#define TYPLONK_TABLES_AUTO_MIN_LEN 16384
int typlonk_srs_precompute(typlonk_ctx* ctx, uint32_t srs_id, uint32_t window_bits);
/* Multi-GPU: declare that this entry holds bases [first_index, first_index + len) of a total_len-point SRS
 * (one process per GPU, each with its own slice).  Every MSM / prover call on it then takes the FULL
 * coefficient vector (pointer to coefficient 0, global length m <= total_len, same length check as
 * kzg/src/lib.rs:43) and returns this rank's PARTIAL sum over its index range -- the identity if the range is
 * empty.  The partial points are folded by typlonk_comm_fold_g1 / the *_sharded_* entry points below (RCCL), or by
 * the caller's own exchange + typlonk_g1_sum_host. */
int typlonk_srs_set_shard(typlonk_ctx* ctx, uint32_t srs_id, size_t first_index, size_t total_len);
int typlonk_srs_free(typlonk_ctx* ctx, uint32_t srs_id);
int typlonk_srs_len(typlonk_ctx* ctx, uint32_t srs_id, size_t* len);

/* ---- multi-GPU exchange: one process per GPU, RCCL over xGMI ------------------------------------------------------
 * The reference's evaluate_in_s returns the FULL sum (kzg/src/lib.rs:41-54); with the base vector index-sharded over
 * the GPUs of a node (typlonk_srs_set_shard) the full sum is the fold of the ranks' partial sums.  RCCL has no
 * elliptic-curve reduction, so the library's "all-reduce" is one ncclAllGather of 104-byte records (12 limbs + flag)
 * on the context's stream followed by a fold in rank order 0..world-1 on every rank: the same bits everywhere.
 * librccl is loaded on first use (dlopen "librccl.so.1"): single-GPU callers never need it.
 *   typlonk_comm_unique_id   rank 0 creates the rendezvous id (ncclGetUniqueId) and hands the 128 bytes to the other
 *                            ranks by whatever channel the host program has (a file, a socket, MPI, a Rust channel).
 *   typlonk_comm_init        every rank: ncclCommInitRank on the context's device (collective: blocks until all
 *                            `world` ranks have called it).  world = 1 is allowed (the exchange is then a local copy).
 *   typlonk_comm_fold_g1     in place: count points in, on return each holds sum over ranks of that rank's point
 *                            (collective).  What a caller that drives the prover rounds itself uses between rounds.
 *   typlonk_msm_g1_sharded_devptr / _batch_devptr
 *                            typlonk_msm_g1_devptr / _batch_devptr on an SRS shard + the fold: every rank passes the
 *                            full coefficient vector(s) and gets the full sum(s) (collective).
 * typlonk_prove on a context with a communicator and an SRS shard folds the commitments of every round itself, so
 * all ranks hash identical points, squeeze identical challenges and return the identical proof.
 * The compact shape on a shard -- a "folding context" is one with a communicator, used with an SRS id that has a shard set.
 * On it these five calls are COLLECTIVES that every rank must make, in the same order, and each returns on every rank exactly
 * what one context holding the whole SRS returns, byte for byte:
 *   typlonk_circuit_commitments            one fold of 8 records: the ranks' partial sums of the eight circuit commitments
 *   typlonk_circuit_vk                     one fold of 9 records: the same and the P0 record (SRS point 0 on the rank whose
 *                                          range starts at index 0, the identity on the others)
 *   typlonk_prove_compact / _compact_host  four folds of 12, 1, 3 and 2 records per proof, a FIXED schedule:
 *                                            1. [a] [b] [c], the eight partial circuit commitments, the P0 record  (-> beta, gamma)
 *                                            2. [Z]  (-> alpha)     3. [t_lo] [t_mid] [t_hi]  (-> zeta)     4. W_z, W_zw
 *                                          The statement digest d0 is formed from the folded key after fold 1.  The eight MSMs run
 *                                          once per (circuit, SRS) on a rank -- what is cached is that rank's PARTIAL sums -- and
 *                                          the nine records are sent with every proof (about 1 KB), so that no rank can disagree
 *                                          with its peers about a fold's record count, whatever its cache holds and whichever
 *                                          argument it refuses.
 * The record counts above are the contract: they depend on nothing that differs between ranks.  Failure: once such a call is
 * past its null-pointer checks every path ends in its next fold.  A rank that refuses its arguments (an unknown circuit, a
 * short wire column, pi_len > n, ...), meets a device error or fails a round joins that fold with flagged records and returns
 * ITS OWN code; every peer returns TYPLONK_ERR_COMM naming that rank; all ranks leave at the same fold, no proof is in flight
 * afterwards, and the communicator and the context stay usable.  An unsatisfied witness is not a failure of the exchange:
 * r(zeta) comes from replicated data, all four folds complete and every rank returns TYPLONK_ERR_UNSATISFIED with `out` filled
 * as on one GPU.  A shard WITHOUT a communicator is refused with TYPLONK_ERR_INVALID_ARG by all five (nothing can fold
 * mid-call from outside).  typlonk_verify, typlonk_prove_batch and typlonk_prove_batch_compact refuse shards with or without
 * one: sharding is for the latency of ONE large proof; a batch of small proofs belongs on one GPU per proof (a wave holds 4
 * proofs at 2^20 rows and 1 from 2^22 on).  Exercised with 2 and 8 ranks: tests/test_gpu_dist_compact.py.
 * Failure on one rank: a member of a communicator never leaves between "decided to fold" and the collective.  The
 * *_sharded_* entry points, typlonk_comm_fold_g1 and typlonk_prove join the collective of the step that failed with
 * flagged records -- whether the failure is the local MSM / prover round, a bad argument (a null output, m > len) or the
 * staging copy of the records itself (the send buffer is kept poisoned except between a successful copy and the
 * all-gather) -- so that rank returns its own error code and every other rank TYPLONK_ERR_COMM (typlonk_last_error
 * names the rank); nobody is left waiting and the communicator stays usable.  The exchange buffers are allocated by
 * typlonk_comm_init BEFORE it joins ncclCommInitRank (a rank that cannot allocate never becomes a member); a fold never
 * allocates (more than 32 points go through in pieces).  Exercised with 2 and 8 ranks: tests/test_gpu_dist.py.
 *   typlonk_comm_available   1 if librccl can be loaded in this process (TYPLONK_RCCL_LIB names it, default: the SONAME
 *                            librccl.so.1), else 0.  NOT collective: ranks agree on it BEFORE the collective
 *                            typlonk_comm_init, in which a rank that cannot load the library would leave the others waiting. */
#define TYPLONK_COMM_ID_BYTES 128
int typlonk_comm_available(void);
int typlonk_comm_unique_id(uint8_t id[TYPLONK_COMM_ID_BYTES]);
int typlonk_comm_init(typlonk_ctx* ctx, const uint8_t id[TYPLONK_COMM_ID_BYTES], int rank, int world);
int typlonk_comm_destroy(typlonk_ctx* ctx);
int typlonk_comm_info(const typlonk_ctx* ctx, int* rank, int* world); /* world = 0: no communicator */
int typlonk_comm_fold_g1(typlonk_ctx* ctx, uint64_t* xy /* count*12, in/out */, uint8_t* inf /* count, in/out */,
                         size_t count);
int typlonk_msm_g1_sharded_devptr(typlonk_ctx* ctx, uint32_t srs_id, const void* d_scalars, size_t m,
                                  uint64_t out_xy[12], uint8_t* out_inf);
int typlonk_msm_g1_sharded_batch_devptr(typlonk_ctx* ctx, uint32_t srs_id, const void* const* d_scalars, const size_t* m,
                                        size_t count, uint64_t* out_xy, uint8_t* out_inf);

/* ---- MSM: sum_{i<m} scalars[i] * srs[i]  (== evaluate_in_s with coeffs = scalars) --------------- */
/* scalars: m Fr elements (Montgomery).  0 <= m <= srs length, else TYPLONK_ERR_LENGTH.  m = 0 gives
 * the identity (the reference's empty `.sum()`). */
int typlonk_msm_g1(typlonk_ctx* ctx, uint32_t srs_id, const uint64_t* scalars, size_t m,
                   uint64_t out_xy[12], uint8_t* out_inf);
/* Same with the scalars already in HBM: a typlonk_buf range, or a raw device pointer. */
int typlonk_msm_g1_dev(typlonk_ctx* ctx, uint32_t srs_id, const typlonk_buf* scalars, size_t offset, size_t m,
                       uint64_t out_xy[12], uint8_t* out_inf);
int typlonk_msm_g1_devptr(typlonk_ctx* ctx, uint32_t srs_id, const void* d_scalars, size_t m,
                          uint64_t out_xy[12], uint8_t* out_inf);

/* `count` independent MSMs over the same SRS (prove() issues them in groups: the three wire
 * commitments plonk/src/proof.rs:107-110, the openings :147-175, the quotient slices :181).  Three
 * are kept in flight on separate workspaces/streams (TYPLONK_MSM_INFLIGHT=1..4), their accumulations one after the
 * other, so one MSM's sort and reduction tail run beside another's accumulation.  d_scalars[k]: device pointer to m[k] Fr elements; out_xy: count*12 limbs; out_inf: count. */
int typlonk_msm_g1_batch_devptr(typlonk_ctx* ctx, uint32_t srs_id, const void* const* d_scalars, const size_t* m,
                                size_t count, uint64_t* out_xy, uint8_t* out_inf);

/* ---- NTT over Fr: radix-2 domain of size 2^log_n with arkworks' generator -------------------------
 * omega = TWO_ADIC_ROOT_OF_UNITY^(2^(32-log_n)).  Natural order in, natural order out, in place.
 *   inverse = 0: data[k] <- sum_i data[i] * (g*omega^k)^i                (fft / coset_fft)
 *   inverse = 1: data[i] <- g^-i * n^-1 * sum_k data[k] * omega^(-ik)    (ifft / coset_ifft)
 * coset_shift: NULL (g = 1) or 4 limbs (Montgomery).  The caller zero-pads to 2^log_n.
 * Sizes: every log_n <= 32 is accepted (the reference's domain constructor fails above the two-adicity, builder.rs:70);
 * the parity suite compares whole vectors with the CPU restatement up to 2^27 (a 4-GiB vector); one-multiplication
 * twiddle tables are kept up to 2^24 points, larger transforms compose their twiddles from two-level tables.
 * Tables keyed by a caller-chosen coset shift are a cache (8 groups / 3 GiB): building a ninth evicts the least recently
 * used group after a hipDeviceSynchronize() -- a device-wide wait, so a caller that cycles through many shifts stalls
 * every stream of the device at each eviction (the prover uses one shift, which stays resident).
 * typlonk_ntt_fr blocks until the result is back on the host; the _dev / _devptr forms (and
 * typlonk_quotient_dev) are stream-ordered on the context's stream and return once enqueued -- any
 * later call on the same context, a typlonk_buf_download or typlonk_sync observes the result. */
int typlonk_ntt_fr(typlonk_ctx* ctx, uint64_t* data, uint32_t log_n, int inverse, const uint64_t* coset_shift);
int typlonk_ntt_fr_dev(typlonk_ctx* ctx, typlonk_buf* buf, size_t offset, uint32_t log_n, int inverse,
                       const uint64_t* coset_shift);
int typlonk_ntt_fr_devptr(typlonk_ctx* ctx, void* d_data, uint32_t log_n, int inverse,
                          const uint64_t* coset_shift);
/* `count` transforms of the same size, direction and coset in one call: d_data[v] is a device pointer to 2^log_n Fr
 * elements, transformed in place; the vectors must not overlap (TYPLONK_ERR_INVALID_ARG).  The reference always
 * transforms in groups -- `interpolate` of the three wire columns (plonk/src/proof.rs:50), their re-evaluation
 * (:113-115), the three sigma columns (:334-338, :412-418), the five selector columns (plonk/src/builder.rs:84-88) --
 * so every pass of the group is ONE launch carrying count x the tiles of a single vector over shared twiddle tables
 * (as typlonk_msm_g1_batch_devptr does for the group's commitments).  Bit-identical to `count` single calls;
 * count = 0 is a no-op; stream-ordered like the _devptr form. */
int typlonk_ntt_fr_batch_devptr(typlonk_ctx* ctx, void* const* d_data, size_t count, uint32_t log_n, int inverse,
                                const uint64_t* coset_shift);

/* ---- quotient polynomial (plonk::proof::quotient_polynomial, /root/reference/plonk/src/proof.rs:292-375)
 * All inputs are device-resident coefficient vectors of n = 2^log_n elements (zero padded), as
 * produced by typlonk_ntt_fr_dev(inverse): the wire polynomials a, b, c (proof.rs:50), the grand
 * product Z (:127), the five selector polynomials q_l q_r q_o q_m q_c (builder.rs:84-88), the three
 * sigma polynomials (proof.rs:334-338) and the public-input polynomial (:105).  Z(wX) is derived
 * internally; public_inputs may be NULL (= the zero polynomial, public inputs [0] as in the reference's
 * README and tests).  Scalars are 4-limb Montgomery Fr: challenges alpha, beta, gamma (proof.rs:111, 133) and
 * the identity-permutation cosets k_0..k_2 (permutation/src/lib.rs:141-154; 2, 3, 4 in the reference).
 * t_out must hold >= 4n elements; on return its first 3n hold the coefficients of t (degree <= 3n - 4;
 * the three commitments of SlicedPoly<3> are MSMs of [0,n), [n,2n), [2n,3n)), the rest is zero.
 * The schoolbook products of the reference are replaced by a 4n coset NTT: identical result
 * whenever the constraint numerator vanishes on the domain (every valid witness). */
/* The prover-side entry points (quotient, grand product, the rounds, typlonk_prove) take 1 <= log_n <= 24 -- up to 2^24
 * rows, a 2^26-point quotient domain, on one GPU; larger domains return TYPLONK_ERR_DOMAIN / _LENGTH.
 * HBM a context keeps after a proof of n = 2^log_n rows (grow-only workspaces, released by typlonk_free; 32 B per Fr):
 *                                        n = 2^22   n = 2^23   n = 2^24
 *   circuit cache (9 x 4n + 11 n Fr)       5.9 GiB   11.8 GiB   23.5 GiB   per typlonk_circuit_load
 *   quot_ext (5 x 4n Fr)                   2.5 GiB    5.0 GiB   10.0 GiB
 *   prover_mem (19 n Fr)                   2.4 GiB    4.8 GiB    9.5 GiB
 *   ops_tmp (4 n + n / 2048 + 8 Fr)        0.5 GiB    1.0 GiB    2.0 GiB   (grand product)
 *   ntt_scratch (a 2^25 / 2^26 batch)      1.0 GiB    1.0 GiB    2.0 GiB
 *   SRS of n + 3 points with c = 20 tables 6.5 GiB   13.0 GiB   26.0 GiB   (13 x 128 B per point)
 *   total                                 18.8 GiB   36.5 GiB   73.0 GiB   plus twiddle / coset tables and MSM workspaces
 *   check cache (5 n Fr + 12 n B)          0.7 GiB    1.3 GiB    2.7 GiB   per circuit, only once typlonk_witness_check /
 *                                                                           typlonk_circuit_permutation has run on it: the
 *                                                                           selector evaluations and the 3n-entry permutation
 *                                                                           (160 MiB + 12 MiB at 2^20); not in the total.
 *                                                                           A circuit made by typlonk_circuit_compile holds the
 *                                                                           12 n-byte permutation from the start
 *   solve cache (about 52 n B)             0.2 GiB    0.4 GiB    0.8 GiB   per circuit, only once typlonk_witness_solve* has run
 *                                                                           on it, on top of the check cache: src 12 n, order
 *                                                                           <= 4 n, level offsets <= 4 n, inverses 32 n bytes;
 *                                                                           not in the total
 * typlonk_prove_batch keeps one wave's arena in prover_mem instead (39 n Fr per proof in flight, one proof per wave here):
 *   prover_mem (39 n Fr)                   4.9 GiB    9.8 GiB   19.5 GiB   (quot_ext is not used by a batch)
 *   ops_tmp (8 n / 2048 Fr) + slots        4 MiB      8 MiB     16 MiB
 * (typlonk_srs_precompute itself needs another (T - 1) x 48 B per point while it runs: 9.0 GiB at 2^24 + 3.) */
#define TYPLONK_MAX_PROVER_LOG_N 24
typedef struct typlonk_quotient_args {
    const typlonk_buf* wires[3];
    const typlonk_buf* z;
    const typlonk_buf* selectors[5];
    const typlonk_buf* sigma[3];
    const typlonk_buf* public_inputs;
    uint64_t alpha[4], beta[4], gamma[4];
    uint64_t cosets[3][4];
    uint32_t circuit; /* 0, or an id from typlonk_circuit_load: selectors/sigma above are then ignored */
} typlonk_quotient_args;
/* Transform the per-circuit constants of the quotient (five selector + three sigma polynomials, and
 * L0) to the 4n coset domain once; they are fixed per CompiledCircuit (plonk/src/lib.rs:19-35). */
int typlonk_circuit_load(typlonk_ctx* ctx, const typlonk_buf* const selectors[5], const typlonk_buf* const sigma[3],
                         uint32_t log_n, uint32_t* circuit_id);
/* The same circuit from what a front end holds: the selector EVALUATIONS over the domain and the copy-constraint permutation
 * itself (Permutation { perm }, permutation/src/lib.rs:95-98), instead of eight interpolated polynomials.  The call is
 * Permutation::compile (permutation/src/lib.rs:101-128: sigma_i(w^j) = k_i' * w^j' for perm[i * n + j] = i' * n + j') on the
 * device, one batched inverse transform of the eight columns, and typlonk_circuit_load's coset extensions.
 *   selector_evals  q_l q_r q_o q_m q_c, n = 2^log_n evaluations each (Montgomery Fr, the contract of typlonk_ntt_fr_dev's
 *                   input; left as they are).  A buffer shorter than n returns TYPLONK_ERR_RANGE.
 *   perm            HOST array of 3n successors over the flat cells col * n + row (as typlonk_circuit_permutation returns it),
 *                   or NULL = the identity (no copy constraints)
 *   cosets          k_0 k_1 k_2.  TYPLONK_ERR_INVALID_ARG for a coset that is not a canonical residue, is zero, or meets
 *                   another: (k_i / k_j)^n = 1 (three ladders on the host).
 *   log_n           outside 1..TYPLONK_MAX_PROVER_LOG_N returns TYPLONK_ERR_DOMAIN
 *   result          a circuit id every other call accepts.  The circuit is the one typlonk_circuit_load builds from the inverse
 *                   transforms (typlonk_ntt_fr_dev) of the same selector evaluations and of the sigma evaluations
 *                   k_col(perm[x]) * w^row(perm[x]), word for word: every sigma value is written as a canonical residue.
 *   lint            *defects (may be NULL) = entries of perm that are not below 3n + cells that are the image of != 1 cells, the
 *                   definition of typlonk_circuit_permutation.  With defects != 0 no circuit is made: the call returns
 *                   TYPLONK_ERR_INVALID_ARG and typlonk_last_error names the lowest defective cell (as
 *                   typlonk_srs_load_compressed treats a rejected point).  *defects is written only when the lint has run.
 *   A refused call leaves the context and *circuit_id as they were.  Never a collective and no SRS involved: works on a
 *   sharded context.  Blocks until the circuit is usable, as typlonk_circuit_load does.
 *   The circuit keeps perm with the cosets it was compiled for (12 n bytes, device): typlonk_circuit_permutation and
 *   typlonk_witness_check under those cosets run no recovery; other cosets recover it from the sigma values, as for a loaded
 *   circuit.  The selector evaluations of the check cache are still made on the first check.
 * One thread per cell, two field products each: w^row = hi[row >> h] * lo[row & (2^h - 1)] from the two-level twiddle tables
 * (h = (log_n + 1) / 2), times the coset.  Device memory beyond the circuit's own: the permutation and, for the duration of the
 * call, 12 n bytes of indegrees. */
int typlonk_circuit_compile(typlonk_ctx* ctx, const typlonk_buf* const selector_evals[5], const uint32_t* perm,
                            const uint64_t cosets[3][4], uint32_t log_n, uint32_t* circuit_id, uint64_t* defects);
/* The same with the selector columns in HOST memory: each holds `rows` Fr elements, and rows must equal n (else
 * TYPLONK_ERR_LENGTH). */
int typlonk_circuit_compile_host(typlonk_ctx* ctx, const uint64_t* const selector_evals[5], size_t rows,
                                 const uint32_t* perm, const uint64_t cosets[3][4], uint32_t log_n,
                                 uint32_t* circuit_id, uint64_t* defects);
/* The copy-constraint permutation from what a front end holds: `count` pairs of cells that must carry one value
 * (PermutationBuilder::add_constrain and build, permutation/src/lib.rs:48-93), made on the device.
 *   pairs           HOST array of 2 * count flat cells x = col * n + row, pair i = (pairs[2i], pairs[2i + 1]).  NULL with
 *                   count != 0 returns TYPLONK_ERR_INVALID_ARG; count = 0 gives the identity (pairs may then be NULL);
 *                   count > 2^32 - 1 returns TYPLONK_ERR_LENGTH.
 *   log_n           outside 1..TYPLONK_MAX_PROVER_LOG_N returns TYPLONK_ERR_DOMAIN.  All of these are judged before a pair is read.
 *   perm            HOST array of 3n successors (may be NULL): the CANONICAL permutation of the partition the pairs generate.
 *                   Inside a class the cells ascend, x_0 < x_1 < ... < x_{k-1}, perm[x_i] = x_{i+1} and perm[x_{k-1}] = x_0; a
 *                   cell in no pair is a fixed point.  It depends on the partition alone: the order, orientation and
 *                   multiplicity of the pairs, self-pairs and redundant pairs change no word of it, nor does the run (the
 *                   reference walks a HashMap, lib.rs:68, and gives one circuit another sigma every time).
 *   classes         (may be NULL) the classes among the 3n cells, singletons included: the cells that are the lowest of theirs
 *   a bad pair      A pair that names a cell >= 3n returns TYPLONK_ERR_INVALID_ARG; typlonk_last_error names how many pairs
 *                   are bad, the lowest bad pair index and its cell (as the compile's lint names a cell).  perm and *classes
 *                   are then left as they were and the context stays usable.  (The reference's check_tag, lib.rs:44-47, lets
 *                   column 3 through and indexes out of bounds in build.)
 * Never a collective and no SRS involved: works on a sharded context.  Blocks for the result.
 * Kernels (perm_pairs.hip): one validation pass; a union-find over 3n parents, a thread per pair, the larger root hooked
 * under the smaller so that a class's root is its lowest cell; ceil((log_n + 2) / 3) rounds of pointer jumping; a stable
 * 8-bit LSD radix sort of the cells by root, ceil((log_n + 2) / 8) passes; one linking pass.  The launch count depends on
 * log_n alone.  A walk that exceeds 2 * 3n steps (no input can cause it) returns TYPLONK_ERR_INTERNAL.
 * Device memory for the duration of the call: 36.75 n + 8 * count bytes (+ 8 KiB), freed on return. */
int typlonk_permutation_from_pairs(typlonk_ctx* ctx, const uint32_t* pairs, size_t count, uint32_t log_n, uint32_t* perm,
                                   uint64_t* classes);
/* typlonk_circuit_compile from the pairs: the circuit is, word for word, the one typlonk_circuit_compile makes from the
 * canonical perm of the same pairs, and it keeps that perm with its cosets in the same way -- but the permutation is written
 * into the kept copy by the kernels above and never crosses to the host.  pairs, count, log_n and *classes as for
 * typlonk_permutation_from_pairs (refused first, in that order); selector_evals and cosets as for typlonk_circuit_compile,
 * with its refusals.  A refused call leaves the context, *circuit_id and *classes as they were. */
int typlonk_circuit_compile_pairs(typlonk_ctx* ctx, const typlonk_buf* const selector_evals[5], const uint32_t* pairs,
                                  size_t count, const uint64_t cosets[3][4], uint32_t log_n, uint32_t* circuit_id,
                                  uint64_t* classes);
/* The same with the selector columns in HOST memory, `rows` elements each (rows != n: TYPLONK_ERR_LENGTH). */
int typlonk_circuit_compile_pairs_host(typlonk_ctx* ctx, const uint64_t* const selector_evals[5], size_t rows,
                                       const uint32_t* pairs, size_t count, const uint64_t cosets[3][4], uint32_t log_n,
                                       uint32_t* circuit_id, uint64_t* classes);
int typlonk_circuit_free(typlonk_ctx* ctx, uint32_t circuit_id);
int typlonk_quotient_dev(typlonk_ctx* ctx, const typlonk_quotient_args* args, uint32_t log_n, typlonk_buf* t_out);

/* ---- grand product Z of the copy-constraint argument (permutation::CompiledPermutation::prove,
 * /root/reference/permutation/src/proving.rs:7-31, called at plonk/src/proof.rs:119-120).
 * wires[i] / sigma[i]: the i-th witness column and sigma column as EVALUATIONS over the size-2^log_n
 * domain (n elements each); cell (i, j) carries the identity tag cosets[i] * w^j.  z_evals_out receives
 * Z_0 = 1, Z_j = prod_{k<j} prod_i (w_ik + beta id_ik + gamma) / (w_ik + beta sigma_ik + gamma), j < n
 * (the reference's n+1 values without the last one).  Stream-ordered except for one 32-byte readback. */
int typlonk_grand_product_dev(typlonk_ctx* ctx, const typlonk_buf* const wires[3], const typlonk_buf* const sigma[3],
                              const uint64_t beta[4], const uint64_t gamma[4], const uint64_t cosets[3][4],
                              uint32_t log_n, typlonk_buf* z_evals_out);

/* ---- open(): the polynomial half of kzg::KzgScheme::open (/root/reference/kzg/src/lib.rs:55-61).
 * poly: m coefficients starting at `offset` of a device vector.  y_out <- p(z) (Horner, :57); when
 * q_out is not NULL it receives the m - 1 coefficients of (p - p(z)) / (X - z) (:58-61), ready for
 * typlonk_msm_g1_dev (:62).  q_out must not alias poly.  1 <= m <= 2^25.  Blocks for the 32-byte result. */
int typlonk_open_dev(typlonk_ctx* ctx, const typlonk_buf* poly, size_t offset, size_t m, const uint64_t z[4],
                     typlonk_buf* q_out, uint64_t y_out[4]);
/* out[i] = sum_k scalars[k] * polys[k][i] for i < n, plus `constant` (may be NULL) on coefficient 0: the
 * scalar-times-polynomial sums of linearisation_poly (/root/reference/plonk/src/proof.rs:376-439).
 * terms <= 12; every polys[k] holds >= n elements; out may alias none of them.  Stream-ordered. */
int typlonk_lincomb_dev(typlonk_ctx* ctx, const typlonk_buf* const* polys, const uint64_t (*scalars)[4], size_t terms,
                        const uint64_t* constant, size_t n, typlonk_buf* out);
/* out[(p * n_points + k) * 4 ..] = polys[p](points[k]) = sum_{i<m} polys[p][i] * points[k]^i, the value of
 * DensePolynomial::evaluate (ark-poly, reached from permutation/src/lib.rs:165-176 and plonk/src/proof.rs:205-210).
 * 1 <= m <= 2^25 coefficients from `offset` of each buffer; 1 <= count <= 16; n_points >= 1 (any count, processed in
 * tiles).  Results are canonical Montgomery Fr, as typlonk_open_dev's y_out.  Blocks for the result.
 * A point that is not a canonical residue (limbs >= r) returns TYPLONK_ERR_INVALID_ARG.  Workspace (grow-only): the points,
 * the results and at most 128 MiB of per-chunk partial sums. */
int typlonk_poly_eval_dev(typlonk_ctx* ctx, const typlonk_buf* const* polys, size_t count, size_t offset, size_t m,
                          const uint64_t (*points)[4], size_t n_points, uint64_t* out);

/* ---- the prover's device-side flow: plonk::proof::prove (/root/reference/plonk/src/proof.rs:26-57, 96-194)
 * split at its two Fiat-Shamir squeezes (challenges.rs is CPU-side and out of scope, so the caller
 * supplies the challenges):
 *   round1  columns (EVALUATIONS, n each, blinding rows included -- proof.rs:43-49) and the public-input
 *           column (NULL = all zero) -> a, b, c, PI by iNTT (:50, :105) and the commitments [a], [b], [c] (:107-110)
 *   round2  beta, gamma (:111) -> grand product Z (:119), iNTT (:127), [Z] (:129)
 *   round3  alpha, zeta (:133-136) -> quotient (:139), openings of a, b, c, Z at zeta and Z at zeta*w (:147-163),
 *           linearisation polynomial r and its opening (:165-175), [t_lo], [t_mid], [t_hi] (:181)
 * The circuit id comes from typlonk_circuit_load; the SRS must hold > n points.  n <= 2^24. */
typedef struct typlonk_prover typlonk_prover;
typedef struct typlonk_proof_tail {
    uint64_t t_xy[3][12];   /* quotient slice commitments                                   */
    uint8_t t_inf[3];
    uint64_t w_xy[6][12];   /* opening witnesses: a, b, c at zeta; Z at zeta; Z at zeta*w; r at zeta */
    uint8_t w_inf[6];
    uint64_t evals[6][4];   /* a(zeta) b(zeta) c(zeta) Z(zeta) Z(zeta w) r(zeta)  (r(zeta) = 0 for a valid witness) */
} typlonk_proof_tail;
int typlonk_prover_round1(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const typlonk_buf* const wire_evals[3],
                          const typlonk_buf* pi_evals, typlonk_prover** out, uint64_t commit_xy[3][12],
                          uint8_t commit_inf[3]);
int typlonk_prover_round2(typlonk_prover* p, const uint64_t beta[4], const uint64_t gamma[4], const uint64_t cosets[3][4],
                          uint64_t z_xy[12], uint8_t* z_inf);
/* round3 / round3_evals return TYPLONK_ERR_UNSATISFIED when r(zeta) != 0 (the identity the verifier checks,
 * proof.rs:234-235): the witness does not satisfy the circuit and the quotient had a remainder the slices silently
 * drop.  `out` is completely filled in that case too (what the reference's verifier would be handed), but the
 * proof will not verify. */
int typlonk_prover_round3(typlonk_prover* p, const uint64_t alpha[4], const uint64_t zeta[4], typlonk_proof_tail* out);
/* Batched openings -- the reference's own to-do (/root/reference/README.md:4, "opening batching"); the proof
 * shape differs from proof.rs:178-192, so this is a separate pair of calls and round3 above stays the default.
 *   round3_evals   quotient, linearisation polynomial and the six evaluations -- no commitment yet
 *   round4_batched v (squeezed by the caller from those evaluations) -> one batch of five MSMs: [t_lo], [t_mid],
 *                  [t_hi]; w[0] = witness of a + v b + v^2 c + v^3 Z + v^4 r at zeta, which equals sum_i v^i W_i of
 *                  round3's witnesses (a, b, c, Z, r order); w[1] = witness of Z at zeta*w.
 * 9 MSMs per proof instead of 13.  (As in the reference, t is committed after zeta -- and here v -- are known:
 * plonk/src/proof.rs:133-136 vs :181; the quotient commitments are never hashed.) */
typedef struct typlonk_proof_evals {
    uint64_t evals[6][4];   /* same order as typlonk_proof_tail.evals */
} typlonk_proof_evals;
typedef struct typlonk_proof_batched {
    uint64_t t_xy[3][12];
    uint8_t t_inf[3];
    uint64_t w_xy[2][12];
    uint8_t w_inf[2];
} typlonk_proof_batched;
int typlonk_prover_round3_evals(typlonk_prover* p, const uint64_t alpha[4], const uint64_t zeta[4],
                                typlonk_proof_evals* out);
int typlonk_prover_round4_batched(typlonk_prover* p, const uint64_t v[4], typlonk_proof_batched* out);
void typlonk_prover_free(typlonk_prover* p);

/* ---- prove(): plonk::proof::prove in ONE call (/root/reference/plonk/src/proof.rs:26-57, 96-194), the Fiat-Shamir
 * transcript included.  The rounds above are driven with the challenges the reference's ChallengeGenerator would
 * squeeze (/root/reference/plonk/src/proof/challenges.rs:9-46; restated natively in csrc/transcript.hpp from the
 * published behaviour of ark-serialize, blake2, rand and ark-ff -- not verifiable against Rust in this image):
 * (beta, gamma) from [a], [b], [c] (proof.rs:111), (alpha, zeta) from [a], [b], [c], [Z] (:133-136).  `out` holds the
 * fields of the reference's Proof (proof.rs:65-95): the three wire commitments with their openings, the permutation
 * commitment with its two openings, evaluation_point = zeta, the three quotient-slice commitments and the opening of
 * r; the challenges are returned too (the reference's verifier recomputes them, :236-246).
 * wire_evals / pi_evals / circuit / SRS exactly as for typlonk_prover_round1; cosets as for round2.
 * Returns TYPLONK_ERR_UNSATISFIED (with `out` filled) when r(zeta) != 0. */
typedef struct typlonk_proof {
    uint64_t commit_xy[3][12];  /* [a], [b], [c] */
    uint8_t commit_inf[3];
    uint64_t z_xy[12];          /* [Z] */
    uint8_t z_inf;
    typlonk_proof_tail tail;    /* [t_lo], [t_mid], [t_hi]; witnesses a, b, c, Z at zeta, Z at zeta*w, r; the six evaluations */
    uint64_t beta[4], gamma[4], alpha[4], zeta[4];
} typlonk_proof;
int typlonk_prove(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const typlonk_buf* const wire_evals[3],
                  const typlonk_buf* pi_evals, const uint64_t cosets[3][4], typlonk_proof* out);
/* The same with the columns still in HOST memory -- how the reference holds them when prove() starts (the padded, blinded
 * Vec<Fr> columns of plonk/src/proof.rs:43-49 and the padded public inputs :52-53): wire_evals[i] and pi_evals (NULL = the zero
 * polynomial) point at n = 2^log_n Fr elements each, 4 limbs per element.  Each column is copied to the device right before its
 * interpolation and commitment are queued, so column i + 1 crosses PCIe while column i is transformed, sorted and accumulated
 * (128 MiB of uploads at 2^20 that a caller of typlonk_prove pays before the first kernel starts).  Same proof, bit for bit. */
int typlonk_prove_host(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const uint64_t* const wire_evals[3],
                       const uint64_t* pi_evals, const uint64_t cosets[3][4], typlonk_proof* out);
/* ---- prove() for many witnesses of one circuit in one call, batched across proofs.
 * out[k] is bit for bit what typlonk_prove (typlonk_prove_host) returns for witness k -- commitments, evaluations, openings
 * and the four challenges; each proof keeps its own transcript.  The reference proof shape (six openings); the compact
 * shape has typlonk_prove_batch_compact below.
 *   wire_evals  count x 3 columns, proof-major (wire_evals[3 k + i] = column i of proof k), n = 2^log_n Fr each
 *   pi_evals    count entries, or NULL (every public-input column zero); an entry may be NULL (that proof's column is zero)
 *   status[k]   TYPLONK_OK, or TYPLONK_ERR_UNSATISFIED when r(zeta) != 0 for witness k: out[k] is filled exactly as
 *               typlonk_prove fills it, and the other proofs are not affected
 * The return value reports only bad arguments and device failures; count = 0 is a no-op.  Single GPU: a sharded SRS (or
 * a context whose communicator would fold) returns TYPLONK_ERR_INVALID_ARG, an SRS shorter than n TYPLONK_ERR_LENGTH.  A
 * call while a round-by-round prover (typlonk_prover_round1 .. typlonk_prover_free) is open is refused with
 * TYPLONK_ERR_INVALID_ARG.
 * The proofs run in waves of G = min(count, 64, max(1, 2^22 >> log_n)) -- 64 proofs at 2^16, 4 at 2^20, 1 from 2^22 on --,
 * any count is accepted.  Every stage of a wave is batched across its proofs (transforms, grand products, openings, the
 * quotient, the linearisation, each round's commitments), and the host waits three times per wave plus one final read.
 * HBM kept after a batch (grow-only, per proof in flight, n = 2^log_n rows; 32 B per Fr):
 *   prover_mem  39 n Fr per proof of a wave: the 19 n of typlonk_prove's arena + the 5 x 4n coset extensions
 *               (2^16: 64 x 80 MiB = 5.0 GiB; 2^20: 4 x 1.2 GiB = 4.9 GiB; 2^22: 4.9 GiB; 2^24: 19.5 GiB)
 *   ops_tmp     8 n / 2048 Fr per proof (the openings' carries); 16 pinned result slots per proof; ~230 KiB of tables */
int typlonk_prove_batch(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const typlonk_buf* const* wire_evals,
                        const typlonk_buf* const* pi_evals, size_t count, const uint64_t cosets[3][4], typlonk_proof* out,
                        int* status);
/* The same with the columns in HOST memory (as typlonk_prove_host): wire_evals[3 k + i] and pi_evals[k] point at n Fr. */
int typlonk_prove_batch_host(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const uint64_t* const* wire_evals,
                             const uint64_t* const* pi_evals, size_t count, const uint64_t cosets[3][4], typlonk_proof* out,
                             int* status);
/* The transcript alone (host-only, no GPU): digest `count` commitments (C-ABI form) in order and squeeze
 * n_challenges Fr elements (4 Montgomery limbs each) -- ChallengeGenerator::with_digest(..).generate_challenges::<N>(). */
int typlonk_transcript_challenges(const uint64_t* xy, const uint8_t* inf, size_t count, size_t n_challenges, uint64_t* out);

/* ---- verify(): plonk::proof::verify (plonk/src/proof.rs:195-281, 441-503) on the device + host ------------------
 * [q_l] [q_r] [q_o] [q_m] [q_c] [sigma_1] [sigma_2] [sigma_3]: the commitments of the eight per-circuit polynomials
 * typlonk_circuit_load keeps (CircuitEntry::coef), one batch of eight MSMs over srs_id (>= n points, no shard set).
 * Computed once per (circuit, srs) and cached with the circuit; GateConstrains::fixed_commitments (builder.rs) and
 * CompiledPermutation::sigma_commitments (permutation/src/lib.rs:178-194).  An SRS shorter than n returns
 * TYPLONK_ERR_LENGTH.  An SRS shard (typlonk_srs_set_shard): TYPLONK_ERR_INVALID_ARG on a context without a communicator; with
 * one the call is a COLLECTIVE every rank must make -- one fold of 8 records, this rank's cached partial sums -- and returns the
 * whole-SRS commitments on every rank ("The compact shape on a shard" above, failure protocol included). */
int typlonk_circuit_commitments(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, uint64_t xy[8][12], uint8_t inf[8]);

/* `count` proofs of one circuit.  ok[k] = 1 iff proof k is accepted.
 *   proofs   typlonk_prove's output; beta / gamma / alpha in it are ignored and recomputed from the commitments with the
 *            transcript (proof.rs:236-246); zeta is the proof's evaluation_point and must equal the recomputed one (:212-214).
 *   pi       pi[k] / pi_len[k]: host Fr column of proof k's public inputs, zero-padded to n by the library (either array or
 *            entry may be NULL / 0 = all zero; pi_len[k] > n -> TYPLONK_ERR_LENGTH).  PI(zeta) = interpolate(pi).evaluate(zeta)
 *            is a barycentric sum on the host for pi_len <= 2048, else an inverse NTT and typlonk_poly_eval_dev.
 *   g2s_xy   [s]G2 as x.c0 x.c1 y.c0 y.c1 (24 limbs; Srs::g2s_ref, kzg/src/srs.rs); not on the twist -> TYPLONK_ERR_INVALID_ARG.
 *            G2 is the fixed generator, and so is G1 in every KZG check (kzg/src/lib.rs:77); the linearisation's constant
 *            term uses SRS point 0 (scheme.identity()).
 *   flags    TYPLONK_VERIFY_PI_AS_PROVER: subtract PI(zeta), as the prover adds it to r (proof.rs:401-402).  Default: the
 *            reference's sign (:497-502), with which the reference rejects its own honest proofs whenever PI(zeta) != 0.
 * Per proof, on the host: the challenges, zeta, r(zeta) = 0 (:234-235) and that all 13 points lie on the curve (an in-memory
 * arkworks point is trusted by the reference; garbage is rejected here rather than paired).  Such a proof gets ok = 0 and
 * stays out of the rest.  On the device: sigma_1(zeta_k), sigma_2(zeta_k) for every proof in one typlonk_poly_eval_dev.
 * The six KZG checks e(W_j, [s]G2 - z_j G2) = e(C_j - y_j G, G2) of every proof are folded with weights rho^(6k + j + 1)
 * into e(sum rho_j W_j, [s]G2) * e(-sum rho_j (C_j + z_j W_j) + (sum rho_j y_j) G, G2) = 1: two MSMs on the device (the
 * linearisation commitment expanded into its 11 bases) and ONE host pairing product for a batch that is all valid.
 * rho = Blake2b-512 of the batch (n, [s]G2, the circuit's commitments, every proof's points, evaluations and PI(zeta),
 * the flags) read as a little-endian integer mod r: deterministic.  When the fold fails it is bisected with the same
 * weights, so every verdict is the per-proof decision of the reference (up to the fold's soundness error, <= 6 count / r);
 * b bad proofs cost at most 2 b ceil(log2 count) + 1 pairing products.  Single GPU: a sharded SRS returns
 * TYPLONK_ERR_INVALID_ARG, with or without a communicator (a verifier's two MSMs are short; nothing is gained by sharding them).  Returns an error only for bad arguments or device failures; a bad proof is ok[k] = 0.
 * count = 0 is a no-op.  With profiling on (typlonk_set_profiling), typlonk_profile_get reports the host wall time of the
 * stages: "verify_host", "verify_eval", "verify_msm", "verify_pairing", then "verify_folds" -- the number of
 * pairing products, a count, not milliseconds. */
#define TYPLONK_VERIFY_PI_AS_PROVER 1u
int typlonk_verify(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const uint64_t g2s_xy[24],
                   const uint64_t cosets[3][4], const typlonk_proof* proofs, size_t count,
                   const uint64_t* const* pi, const size_t* pi_len, uint32_t flags, uint8_t* ok);

/* ---- the COMPACT proof shape: batched KZG openings, a transcript that binds the statement, an O(1) verifier ----------
 * A shape this library defines (the reference's own to-do, /root/reference/README.md:4, "opening batching"); the reference
 * shape above is unchanged.  9 MSMs per proof instead of 13, and the verifier needs a verifying key, not the circuit.
 * Encodings: Fr = 32 bytes, little-endian canonical integer; a G1 point = the 96 bytes of serialize_unchecked that
 * typlonk_prove's transcript hashes; integers little-endian; H(x) = Blake2b-512(x) read as a little-endian integer mod r.
 * sigma_1..3 = the circuit's sigma polynomials in typlonk_circuit_commitments order; w = the domain root; G = the fixed G1
 * generator; P0 = SRS point 0.
 *   statement  vk_bytes = u32 log_n || k_0 || k_1 || k_2 || [q_l] [q_r] [q_o] [q_m] [q_c] [sigma_1] [sigma_2] [sigma_3] || P0
 *              d0 = Blake2b-512("typlonk/compact/v1" || vk_bytes || u64 pi_len || pi_0 .. pi_{pi_len-1})
 *              The statement is exactly the pi_len public values; rows pi_len.. of the public-input column are zero.
 *   transcript T starts as d0; each challenge is H(T || label), the label one ASCII byte:
 *              T ||= [a] [b] [c]                                   beta = H(T || 'b'), gamma = H(T || 'g')
 *              T ||= [Z]                                           alpha = H(T || 'a')
 *              T ||= [t_lo] [t_mid] [t_hi]                         zeta = H(T || 'z')
 *              T ||= a(z) b(z) c(z) Z(z) Z(z w) sigma_1(z) sigma_2(z)   v = H(T || 'v')
 *              The quotient is committed BEFORE zeta is drawn (the reference hashes only [a] [b] [c] [Z], so a prover holding
 *              any witness may pick t = N(zeta) / Z_H(zeta) and pass its verifier; here t is bound first).
 *   proof      a, b, c, Z, t, r exactly as typlonk_prove computes them (r with +PI(zeta)), and
 *              F = a + v b + v^2 c + v^3 Z + v^4 r + v^5 sigma_1 + v^6 sigma_2,
 *              W_z = [(F - F(z)) / (X - z)],  W_zw = [(Z - Z(z w)) / (X - z w)]  (typlonk_prove's Z-at-zeta*w witness).
 *              With the same challenges W_z = round4_batched(v).w[0] + v^5 [q_s1] + v^6 [q_s2], q_si = (sigma_i - sigma_i(z)) / (X - z).
 *              r(zeta) is not sent: it is 0 for a satisfying witness.
 *   verifier   per proof: the 9 points on the curve and the 7 scalars canonical (else ok = 0, kept out of the fold); the five
 *              challenges; zeta^n != 1; PI(zeta) (barycentric on the host up to 2048 values, else inverse NTT +
 *              typlonk_poly_eval_dev); [r] expanded into its 11 bases as typlonk_verify does with TYPLONK_VERIFY_PI_AS_PROVER,
 *              sigma_1(z), sigma_2(z) from the proof; then, with y_F = a + v b + v^2 c + v^3 Z(z) + v^5 sigma_1(z) + v^6 sigma_2(z)
 *              and F_C = [a] + v [b] + v^2 [c] + v^3 [Z] + v^4 [r] + v^5 [sigma_1] + v^6 [sigma_2]:
 *                e(W_z, [s]G2) = e(F_C - y_F G + z W_z, G2)      e(W_zw, [s]G2) = e([Z] - Z(z w) G + z w W_zw, G2)
 *   fold       weights rho^(2k + j + 1), rho = H("typlonk/compact/fold/v1" || vk_bytes || [s]G2 as its 24 limbs || per proof
 *              its 9 points and 7 evaluations || per proof PI(zeta), 0 for a proof the host checks rejected): two device MSMs
 *              (2K bases; 9K + 10: per proof a, b, c, Z, t x 3, W_z, W_zw, shared the 8 commitments, P0, G) and ONE host
 *              pairing product for a batch that is all valid; a failed fold is bisected as typlonk_verify bisects it. */
typedef struct typlonk_vk {
    uint32_t log_n;
    uint64_t cosets[3][4];       /* k_0 k_1 k_2 */
    uint64_t commit_xy[8][12];   /* [q_l] [q_r] [q_o] [q_m] [q_c] [sigma_1] [sigma_2] [sigma_3] */
    uint8_t commit_inf[8];
    uint64_t srs0_xy[12];        /* P0 */
    uint8_t srs0_inf;
    uint64_t g2s_xy[24];         /* [s]G2: x.c0 x.c1 y.c0 y.c1 */
} typlonk_vk;
typedef struct typlonk_proof_compact {
    uint64_t commit_xy[3][12];   /* [a] [b] [c] */
    uint8_t commit_inf[3];
    uint64_t z_xy[12];           /* [Z] */
    uint8_t z_inf;
    uint64_t t_xy[3][12];        /* [t_lo] [t_mid] [t_hi] */
    uint8_t t_inf[3];
    uint64_t w_xy[2][12];        /* W_z, W_zw */
    uint8_t w_inf[2];
    uint64_t evals[7][4];        /* a(z) b(z) c(z) Z(z) Z(z w) sigma_1(z) sigma_2(z) */
    uint64_t beta[4], gamma[4], alpha[4], zeta[4], v[4];   /* for the caller; the verifier recomputes them */
} typlonk_proof_compact;
/* The verifying key of a loaded circuit: the cached typlonk_circuit_commitments (one batch of eight MSMs the first time per
 * (circuit, SRS)), SRS point 0, the cosets and [s]G2.  A g2s that is not on the twist returns TYPLONK_ERR_INVALID_ARG; SRS
 * errors as for typlonk_circuit_commitments.  On an SRS shard with a communicator: a COLLECTIVE every rank must make, one fold
 * of 9 records (the eight partial sums and the P0 record); every rank gets the whole-SRS key, so a rank of a sharded job can
 * hand out the verifying key of its own circuit. */
int typlonk_circuit_vk(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const uint64_t cosets[3][4],
                       const uint64_t g2s_xy[24], typlonk_vk* vk);
/* One compact proof.  wire_evals as for typlonk_prove; pi: a buffer of >= pi_len elements of which only the first pi_len are
 * read (may be NULL when pi_len = 0), brought to the host once for d0.  The first compact proof of a (circuit, SRS) pair
 * computes the circuit commitments for d0 (a one-time cost, cached with the circuit).  Rounds 1 and 2 run as in typlonk_prove;
 * round 3 queues the quotient once alpha is known and waits for its three commitments before it draws zeta.
 * Returns TYPLONK_ERR_UNSATISFIED (with `out` completely filled) when r(zeta) != 0; TYPLONK_ERR_INVALID_ARG for an SRS shard
 * on a context without a communicator or while a round-by-round prover is open; TYPLONK_ERR_DOMAIN above 2^24 rows;
 * TYPLONK_ERR_LENGTH when pi_len > n or the SRS (a shard: its total length) is shorter than n.
 * On an SRS shard with a communicator the call is a COLLECTIVE: four folds of 12, 1, 3 and 2 records ("The compact shape on a
 * shard" above), the same proof on every rank as from one context with the whole SRS; a rank that fails returns its own code
 * and its peers TYPLONK_ERR_COMM, at the same fold. */
int typlonk_prove_compact(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const typlonk_buf* const wire_evals[3],
                          const typlonk_buf* pi, size_t pi_len, const uint64_t cosets[3][4], typlonk_proof_compact* out);
/* The same with the columns in HOST memory (uploaded column by column beside round 1, as typlonk_prove_host): wire_evals[i]
 * holds `rows` Fr elements, and rows must equal the circuit's n (else TYPLONK_ERR_LENGTH); pi holds pi_len values.  On a shard
 * with a communicator: the same collective as typlonk_prove_compact. */
int typlonk_prove_compact_host(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const uint64_t* const wire_evals[3],
                               size_t rows, const uint64_t* pi, size_t pi_len, const uint64_t cosets[3][4],
                               typlonk_proof_compact* out);
/* ---- typlonk_prove_compact for many witnesses of one circuit in one call, batched across proofs.
 * out[k] is bit for bit what typlonk_prove_compact (typlonk_prove_compact_host) returns for witness k -- the 9 points, the 7
 * evaluations and the five challenges.  Each proof has its own transcript, started from its own statement digest d0: the vk
 * bytes are shared by the batch, pi_len[k] and the public values are proof k's.
 *   wire_evals  count x 3 columns, proof-major, as for typlonk_prove_batch
 *   pi          count entries, or NULL; entry k is a buffer of >= pi_len[k] values of which only the first pi_len[k] are read
 *               (it may be NULL when pi_len[k] = 0).  The values of a whole wave are brought to the host behind one wait.
 *   pi_len      count entries, or NULL (= all 0)
 *   status[k]   TYPLONK_OK, or TYPLONK_ERR_UNSATISFIED when r(zeta) != 0 for witness k: out[k] is completely filled, as
 *               typlonk_prove_compact fills it, and the other proofs are not affected
 * The return value reports only bad arguments and device failures; count = 0 is a no-op.  TYPLONK_ERR_INVALID_ARG: a null
 * argument, an unknown circuit or SRS, a null wire column, pi_len[k] != 0 with pi or pi[k] NULL, a sharded SRS or a context
 * whose communicator would fold, a round-by-round prover open on the context.  TYPLONK_ERR_RANGE: a wire buffer shorter than n
 * or a pi buffer shorter than pi_len[k].  TYPLONK_ERR_LENGTH: pi_len[k] > n, an SRS shorter than n.  TYPLONK_ERR_DOMAIN:
 * log_n > TYPLONK_MAX_PROVER_LOG_N.  A refused call leaves `out` and the context as they were.
 * The first call for a (circuit, SRS) pair computes the eight circuit commitments for d0 once, through the cache of
 * typlonk_circuit_commitments -- not per proof or per wave.
 * Waves as typlonk_prove_batch: G = min(count, 64, max(1, 2^22 >> log_n)) proofs, every stage batched across them, in the
 * compact transcript's order: rounds 1 and 2 as there; then the quotient of every proof once every alpha is known and the 3G
 * commitments [t_lo] [t_mid] [t_hi] in one queue, which the host waits for before it draws any zeta; the evaluations of the
 * wave in one launch sequence and one wait; r and F of every proof from one fused kernel (a thread owns a coefficient and four
 * proofs: the circuit's eight coefficient vectors are read once per group, r is not read back to form F); F's opening and
 * r(zeta); the 2G commitments W_z, W_zw in one queue.  The host waits four times per wave plus one final read.
 * HBM: typlonk_prove_batch's arena, unchanged (39 n Fr per proof of a wave; this shape leaves 3 n of it unused). */
int typlonk_prove_batch_compact(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const typlonk_buf* const* wire_evals,
                                const typlonk_buf* const* pi, const size_t* pi_len, size_t count, const uint64_t cosets[3][4],
                                typlonk_proof_compact* out, int* status);
/* The same with the columns in HOST memory: wire_evals[3 k + i] holds `rows` Fr elements, and rows must equal the circuit's n
 * (else TYPLONK_ERR_LENGTH); pi[k] holds pi_len[k] values. */
int typlonk_prove_batch_compact_host(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const uint64_t* const* wire_evals,
                                     size_t rows, const uint64_t* const* pi, const size_t* pi_len, size_t count,
                                     const uint64_t cosets[3][4], typlonk_proof_compact* out, int* status);
/* `count` compact proofs against one verifying key: ok[k] = 1 iff proof k is accepted.  No SRS and no loaded circuit are
 * needed.  pi[k] / pi_len[k] as for typlonk_verify (pi_len[k] > n -> TYPLONK_ERR_LENGTH).  A vk point off the curve (or a
 * g2s off the twist, a log_n outside 1..24) returns TYPLONK_ERR_INVALID_ARG / TYPLONK_ERR_DOMAIN; a bad proof gets ok = 0;
 * count = 0 is a no-op.  Profiling stages as typlonk_verify's; "verify_eval" appears only when a PI column is longer than
 * 2048 values. */
int typlonk_verify_compact(typlonk_ctx* ctx, const typlonk_vk* vk, const typlonk_proof_compact* proofs, size_t count,
                           const uint64_t* const* pi, const size_t* pi_len, uint8_t* ok);
/* The compact transcript alone (host-only, no GPU): beta, gamma, alpha, zeta, v of `proof` (4 Montgomery limbs each) from
 * its points and evaluations, the vk and the public inputs.  pi_len > 2^log_n returns TYPLONK_ERR_LENGTH. */
int typlonk_compact_challenges(const typlonk_vk* vk, const typlonk_proof_compact* proof, const uint64_t* pi, size_t pi_len,
                               uint64_t out[5][4]);

/* ---- witness check: which gate rows and which copy constraints does a witness fail? -------------------------------------
 * The provers report an unsatisfied witness as TYPLONK_ERR_UNSATISFIED, after the whole proof has been computed, from one
 * probabilistic test (r(zeta) != 0) that names no row; the reference panics in vanishes() or emits a proof its own verifier
 * rejects (plonk/src/proof.rs:234-235, 504-507).  The calls below read the columns once, need no SRS and no communicator, are
 * never a collective (everything they read is replicated, so they work on a sharded context too), are exact, and may be made
 * while a round-by-round prover is open (they touch none of its arena).  Work runs on the context's stream; the calls block.
 * Cells are flat indices x = col * n + row, col in {0, 1, 2} (Tag::to_index, permutation/src/lib.rs).
 * Kept with the circuit after the first call (freed by typlonk_circuit_free / typlonk_destroy): the permutation (3n uint32) with
 * the cosets it was recovered for -- a call with other cosets recovers it again; a circuit made by typlonk_circuit_compile has
 * the one it was compiled from, and no recovery runs under its own cosets -- and the five selector columns as evaluations
 * (5n Fr, one batch of five forward transforms of the coefficient copies typlonk_circuit_load keeps). */
#define TYPLONK_CELL_NONE 0xffffffffu
/* The successor map of the copy-constraint permutation, recovered from the circuit's sigma columns (compiled by
 * permutation/src/lib.rs:101-128 into field values, which is all typlonk_circuit_load sees):
 * perm[x] = y  iff  sigma_col(x)(w^row(x)) = k_col(y) * w^row(y).  perm: 3n entries or NULL.
 * *defects = number of cells whose sigma value is no cell id (perm[x] = TYPLONK_CELL_NONE)
 *          + number of cells that are the image of != 1 cells.  0 = sigma is a permutation of the cells.
 * One thread per cell: the coset by u = sigma / k_i, u^n = 1; the row by Pohlig-Hellman over the order-2^log_n subgroup, about
 * log_n^2 / 2 + 4 log_n field products per cell.  Setup-time work, once per (circuit, cosets).  A coset that is not a canonical
 * residue returns TYPLONK_ERR_INVALID_ARG. */
int typlonk_circuit_permutation(typlonk_ctx* ctx, uint32_t circuit_id, const uint64_t cosets[3][4],
                                uint32_t* perm, uint64_t* defects);

typedef struct typlonk_witness_report {
    uint64_t gate_failures;  /* rows j with q_l a + q_r b - q_o c + q_m a b + q_c + PI != 0 at w^j (proof.rs:317-320)      */
    uint64_t copy_failures;  /* cells x whose value differs (mod r) from the value of perm[x]                              */
    uint32_t gate_listed, copy_listed;  /* min(failures, cap)                                                              */
} typlonk_witness_report;

/* `count` witnesses of one circuit.  wire_evals proof-major as typlonk_prove_batch; pi / pi_len per witness as
 * typlonk_prove_batch_compact (rows pi_len.. of the public-input column are zero; pi_len = n covers typlonk_prove's
 * full column; pi_len may be NULL = all 0).  gate_rows: count*cap; copy_cells: count*cap*2 (x, perm[x]); both may be NULL
 * when cap = 0.  Witness k's lists start at gate_rows[k * cap] and copy_cells[2 * k * cap].
 *   return value  reports only bad arguments and device failures; a failing witness is data in its report, as status[k] is
 *                 for the batch provers.  count = 0 is a no-op.  TYPLONK_ERR_INVALID_ARG: a null argument, an unknown circuit,
 *                 a null column, pi_len[k] != 0 with pi or pi[k] NULL.  TYPLONK_ERR_RANGE: a wire buffer shorter than n or a
 *                 pi buffer shorter than pi_len[k].  TYPLONK_ERR_LENGTH: pi_len[k] > n.  A refused call leaves every output
 *                 as it was.
 *   malformed     a circuit with defects != 0 (typlonk_circuit_permutation) returns TYPLONK_ERR_INVALID_ARG and
 *                 typlonk_last_error names the lowest defective cell.
 *   lists         the lowest failing rows / cells in ascending order, whatever the launch geometry; the counts are totals:
 *                 cap truncates the lists, not the counts.  Entries beyond gate_listed / copy_listed are not written.
 *   equality      of residues mod r, not of bits: a cell holding v + r in its limbs equals one holding v.
 *   agreement     gate_failures == 0 && copy_failures == 0 exactly when the witness satisfies the circuit, which is when the
 *                 provers do not return TYPLONK_ERR_UNSATISFIED (up to their soundness error).
 * One thread per row, the witness in the grid's second dimension; failure flags -> wave ballots -> block counts -> one
 * exclusive scan over the blocks -> an ordered write of the first cap entries. */
int typlonk_witness_check(typlonk_ctx* ctx, uint32_t circuit_id, const typlonk_buf* const* wire_evals,
                          const typlonk_buf* const* pi, const size_t* pi_len, size_t count,
                          const uint64_t cosets[3][4], uint32_t cap,
                          typlonk_witness_report* reports, uint32_t* gate_rows, uint32_t* copy_cells);
/* The same with the columns in HOST memory: wire_evals[3 k + i] holds `rows` Fr elements, and rows must equal the circuit's n
 * (else TYPLONK_ERR_LENGTH); pi[k] holds pi_len[k] values. */
int typlonk_witness_check_host(typlonk_ctx* ctx, uint32_t circuit_id, const uint64_t* const* wire_evals, size_t rows,
                               const uint64_t* const* pi, const size_t* pi_len, size_t count,
                               const uint64_t cosets[3][4], uint32_t cap,
                               typlonk_witness_report* reports, uint32_t* gate_rows, uint32_t* copy_cells);

/* ---- witness solve: the wire columns from the circuit's inputs ---------------------------------------------------------------
 * The reference's interface is circuit.prove([3, 4, 5], vec![0]) (plonk/src/proof.rs:26-57): it takes the circuit's INPUTS, and
 * C::run (builder.rs:381-396) fills the three advice columns gate by gate.  The call below is that step on the device: from a
 * loaded circuit, a handful of assigned cells and the public values it writes the full wire columns into device buffers, ready
 * for typlonk_witness_check and every prover -- the columns never leave HBM.  Deterministic: the library draws no randomness.
 * Cells are flat indices x = col * n + row.  A CLASS is a cycle of the circuit's permutation (the copy kept by
 * typlonk_circuit_compile*, or the one recovered as for typlonk_witness_check, under `cosets`); a circuit with defects != 0 is
 * refused exactly as the check refuses it.
 *   driven      row j is driven iff q_o[j] != 0 mod r.  A class is driven iff it contains the c cell 2n + j of a driven row; its
 *               driver is the lowest such row.  Every other class is free.
 *   values      a free class takes the value assigned to one of its cells through cells / values, or 0 if none is assigned
 *               (the reference's resize(rows - 3, Fr::zero())).  The three blinding rows are ordinary free cells that the
 *               caller assigns.  A driven class with driver d takes c_d = (q_l a + q_r b + q_m a b + q_c + PI_d) / q_o at row
 *               d, a and b being the values of the classes of cells d and n + d, and PI_d = 0 for d >= pi_len.
 *               Every cell gets its class's value, with one exception: the c cell of a driven row that is NOT its class's
 *               driver gets its OWN row's computed value -- two computed values tied by assert_eq.  If the two differ,
 *               typlonk_witness_check then names the copy constraint; solve never papers over it.
 *               Rows with q_o = 0 (constant rows, boolean rows) are not enforced by solve: they are the check's business.
 *               Outputs are canonical Montgomery residues: they compare word for word.
 *   order       row j depends on the drivers of the classes of its a and b cells; rows may be in any order in the table.  If
 *               the dependencies have a cycle the circuit cannot be solved by propagation: TYPLONK_ERR_INVALID_ARG, and
 *               typlonk_last_error names the lowest row that could not be scheduled.
 *   cells       HOST, n_cells flat indices shared by all witnesses; values: HOST, count * n_cells * 4 limbs, witness-major.
 *               Both may be NULL when n_cells = 0.
 *   pi, pi_len  as typlonk_witness_check.  wire_out: count * 3 buffers, proof-major, >= n elements each, all distinct.
 *   refusals    TYPLONK_ERR_INVALID_ARG: a null argument, an unknown circuit, a null output column, pi_len[k] != 0 with pi or
 *               pi[k] NULL, a cell >= 3n, a cell in a driven class, two cells of one class, a value >= r (as
 *               typlonk_poly_eval_dev refuses a point), an unsolvable or malformed circuit.  TYPLONK_ERR_RANGE: an output or pi
 *               buffer too short.  TYPLONK_ERR_LENGTH: pi_len[k] > n.  For the cell and value refusals typlonk_last_error names
 *               the index into cells.  A refused call leaves every output as it was; count = 0 is a no-op.
 * Like the check: blocks, runs on the context's stream, never a collective, no SRS, works on a sharded context.
 * The plan (host, O(n), once per (circuit, cosets), cached with the circuit, freed by typlonk_circuit_free / typlonk_destroy):
 * the level of a driven row is 1 + the larger level of its two sources, a free source being level 0.  A level wider than 256
 * rows is one launch over rows x witnesses; a maximal run of consecutive levels of <= 256 rows each is ONE launch of one
 * 256-thread workgroup per witness that steps through them (cut every 65,536 levels); one fill launch writes the undriven
 * rows.  No kernel waits on another workgroup.  Per driven row: two 32-byte gathers, seven fr30 products (five of the equation,
 * two radix fixes), three 32-byte stores.  Every cell is written exactly once per call.
 * Kept per circuit once solved (beside the check cache): src 12 n + order 4 n + level offsets <= 4 n + inverses 32 n bytes on the
 * device, about 52 n (52 MiB at 2^20), and src again on the host.  Per call: 4 bytes per free class and 32 * count * n_cells
 * bytes go up.
 * What a caller reads to decide (typlonk_solve_info): a solve costs `launches` kernel launches plus, inside run launches, one
 * dependent global-memory round trip and a barrier per level -- `depth` of them end to end.  A wide, shallow circuit (depth of
 * tens) is launch- and bandwidth-bound: 2^20 rows in 33 levels take 1.0 ms, 1/70 of the CPU fill and upload they replace.  A
 * deep, narrow one (the squaring chain: depth = n - 3, one row per level) is latency-bound at about 4.5 us per level and
 * LOSES to the CPU: 291 ms against 5 ms on one CPU thread at 2^16 rows for one witness, on par from 64 witnesses per call
 * (MI355X; DESIGN.md 8i has the measured table).  When depth is within a small factor of driven_rows, fill on the CPU. */
typedef struct typlonk_solve_info {
    uint64_t driven_rows, free_classes;
    uint32_t depth;    /* number of levels                                                                                  */
    uint32_t launches; /* kernel launches one solve queues, whatever count is (per group of 1024 witnesses)                 */
} typlonk_solve_info;
/* builds the plan on first use per (circuit, cosets), caches it with the circuit, reports it */
int typlonk_witness_solve_plan(typlonk_ctx* ctx, uint32_t circuit_id, const uint64_t cosets[3][4], typlonk_solve_info* info);
int typlonk_witness_solve(typlonk_ctx* ctx, uint32_t circuit_id, const uint64_t cosets[3][4],
                          const uint32_t* cells, size_t n_cells, const uint64_t* values,
                          const typlonk_buf* const* pi, const size_t* pi_len, size_t count, typlonk_buf* const* wire_out);

/* ---- hints: advice the solve computes -------------------------------------------------------------------------------------------
 * A circuit written for general selectors needs values that are no row's output: the bits of a computed value (a range check, a
 * comparison), the inverse of a computed value (a non-zero or an equality test).  A HINT says: this free class's value is
 * f(the value of that cell).  The solve schedules it as one more entry of its level lists, so the caller need not evaluate the
 * circuit on the host to know the advice.
 *   install     the hints are kept with the circuit; a call replaces the whole set; n_hints = 0 removes them (hints may then be
 *               NULL).  Freed by typlonk_circuit_free / typlonk_destroy.  The call builds the solve plan under `cosets` at once,
 *               so every refusal is reported here.  Blocks, never a collective, no SRS, works on a sharded context.
 *   dst, src    flat cells col * n + row.  dst names a FREE class, and every cell of that class gets the hint's value.  src is read
 *               as the value the solve writes to that very cell: for the c cell of a driven row that is not its class's driver
 *               that is the row's own computed value, as src[] of the solve already says.  src may lie in a driven, a free or a
 *               hinted class.
 *   kinds       TYPLONK_HINT_INV0: dst = 1 / src, and 0 when src = 0 mod r; Montgomery in and out, canonical (shift and width are
 *               not read).  TYPLONK_HINT_BITS: the value leaves Montgomery form, bits [shift, shift + width) of the integer in
 *               [0, r) are taken, and that integer (below 2^64) is stored as a canonical Montgomery residue; shift in 0..254,
 *               width in 1..64; bits 255 and above read as 0.
 *   levels      a hint's level is 1 + the level of its source, a free, unhinted source being level 0; a row counts a hinted
 *               source with the hint's level.  Within a level the rows come first, then the hints; a level's width, for the
 *               256-entry decision between a run and a wide launch, is rows + hints.  typlonk_solve_info keeps its layout:
 *               depth and launches include the hints' levels, driven_rows counts rows only, free_classes still counts every
 *               class without a driver, hinted ones included.  For a circuit without hints every word of the info and of the
 *               output is what it is without this call.
 *   refusals    all TYPLONK_ERR_INVALID_ARG, and typlonk_last_error names the lowest offending hint as hints[i]: NULL hints with
 *               n_hints != 0, an unknown circuit or a malformed one (as the solve refuses it), an unknown kind, dst or src >= 3n,
 *               for BITS a width outside 1..64 or a shift > 254, dst in a driven class, two hints into one class (the higher one
 *               is named, with the lower).  A dependency cycle is refused too -- src in dst's own class, two hints reading each
 *               other, a hint reading a row that reads the hint: the text names the lowest row that could not be scheduled, or,
 *               if every row could be, the lowest such hint.  A refused call leaves the installed hints, the cached plan and the
 *               context as they were.
 *   at solve    a cell of `cells` in a hinted class is refused: TYPLONK_ERR_INVALID_ARG, "cells[i] lies in a hinted class: its
 *               value is computed".  Nothing else of typlonk_witness_solve changes.  The solve never papers over a hint the
 *               circuit then contradicts: if x = 0 feeds INV0 and a row demands x * inv = 1, typlonk_witness_check names the row.
 * Cost: a hint's value goes to a table of count * n_hints * 32 bytes in the call's workspace and is read from there by later
 * levels and the fill; 16 bytes per hint are kept on the device with the plan.  A circuit with hints runs kernels of its own
 * (the row path of a circuit without hints is the code it was).  An INV0 hint is about 25 rounds of 30 divsteps, some 60 times
 * the work of a row, and a wavefront that holds one runs them for all its lanes; a BITS hint costs two Montgomery products.
 * Measured (MI355X): 2^20 rows of 16-bit range checks, 524,272 BITS hints among them, solve in 0.57 ms for one
 * witness (the one-thread CPU fill and upload: 43 ms).  In a narrow run every level that holds an INV0 hint adds the inversion's
 * latency to the level's: 29 us per level of dependent inverses against 4.5 us per level of rows.  A deep chain of inverses is
 * latency-bound like the deep circuits above, only six times more so: fill such a circuit on the CPU. */
#define TYPLONK_HINT_INV0 1u  /* dst = 1 / src, and 0 when src = 0 mod r                                              */
#define TYPLONK_HINT_BITS 2u  /* dst = (the canonical integer of src mod r, >> shift) & (2^width - 1), as a residue     */
typedef struct typlonk_hint { uint32_t kind, dst, src; uint16_t shift, width; } typlonk_hint;   /* 16 bytes */
int typlonk_circuit_set_hints(typlonk_ctx* ctx, uint32_t circuit_id, const uint64_t cosets[3][4],
                              const typlonk_hint* hints, size_t n_hints);

/* ---- wire format: compact proofs, verifying keys and SRS points as bytes, with compressed points ------------------------
 * Everything above works on in-memory arkworks limbs that the caller is trusted to have formed.  The byte forms below are
 * what leaves the process -- and what comes in from a peer that is NOT trusted: every decoded point is checked to lie on
 * the curve AND in the subgroup of order r.  Nothing that is hashed changes: the transcripts, d0, rho and vk_bytes above keep
 * their 96-byte uncompressed points.
 *   G1 point   48 bytes, the ZCash / IETF BLS12-381 compressed form: x as a big-endian canonical integer, with the three top
 *              bits of byte 0 used as flags:  bit 7 = compressed, always set;  bit 6 = infinity, and then every other bit of
 *              the 48 bytes is 0 (c0 00 .. 00);  bit 5 = y > (p - 1) / 2.  80 00 .. 00 is the order-3 point (0, 2), not infinity.
 *   G2 point   96 bytes, the same convention over Fq2: x.c1 then x.c0, big-endian; flags on byte 0; the sign bit is set iff
 *              y.c1 > (p - 1) / 2, or y.c1 = 0 and y.c0 > (p - 1) / 2.
 *   Fr         32 bytes, little-endian canonical integer (the encoding the compact transcript hashes).
 *   proof      TYPLONK_PROOF_COMPACT_BYTES = 656: [a] [b] [c] [Z] [t_lo] [t_mid] [t_hi] [W_z] [W_zw] (fields 0..8, 48 bytes each)
 *              then a(z) b(z) c(z) Z(z) Z(z w) sigma_1(z) sigma_2(z) (fields 9..15, 32 bytes each).  No challenges.
 *   key        TYPLONK_VK_WIRE_BYTES = 628 ("vk wire form"; NOT the transcript's vk_bytes): u32 log_n little-endian, k_0 k_1 k_2
 *              (Fr), [q_l] [q_r] [q_o] [q_m] [q_c] [sigma_1] [sigma_2] [sigma_3] P0 (48 bytes each), [s]G2 (96 bytes).
 * Accepted encodings are unique.  A point is rejected with the FIRST class that applies, in this order:
 *   TYPLONK_POINT_ENCODING         the compression bit clear, or the infinity bit with any other bit set
 *   TYPLONK_POINT_X_RANGE          x >= p (for G2: either coordinate of x)
 *   TYPLONK_POINT_NOT_ON_CURVE     x^3 + 4 is not a square (G2: x^3 + 4 (1 + u) over Fq2)
 *   TYPLONK_POINT_NOT_IN_SUBGROUP  [r] P != O; skipped -- this check only -- with TYPLONK_DECODE_SKIP_SUBGROUP
 * and a scalar >= r with TYPLONK_SCALAR_RANGE.  (The curve has points of order 3, 11, ... outside the subgroup; e.g. every
 * curve point with x in {0, 4, 5, 6, 8}.) */
#define TYPLONK_POINT_ENCODING 1
#define TYPLONK_POINT_X_RANGE 2
#define TYPLONK_POINT_NOT_ON_CURVE 3
#define TYPLONK_POINT_NOT_IN_SUBGROUP 4
#define TYPLONK_SCALAR_RANGE 5
#define TYPLONK_DECODE_SKIP_SUBGROUP 1u
#define TYPLONK_G1_BYTES 48
#define TYPLONK_G2_BYTES 96
#define TYPLONK_PROOF_COMPACT_BYTES 656
#define TYPLONK_VK_WIRE_BYTES 628
/* a decode status of a proof: 0, or the class of the first bad field (in wire order) and that field's index */
#define TYPLONK_DECODE_STATUS(cls, field) ((uint32_t)(cls) | ((uint32_t)(field) << 8))
#define TYPLONK_DECODE_CLASS(status) ((status) & 0xffu)
#define TYPLONK_DECODE_FIELD(status) ((status) >> 8)
/* Host-only.  xy: count*12 limbs, inf: count flags or NULL, out: count*48 bytes.  Coordinates that are not canonical
 * residues return TYPLONK_ERR_INVALID_ARG (the curve equation is not checked here); `out` is then left as it was. */
int typlonk_g1_compress(const uint64_t* xy, const uint8_t* inf, size_t count, uint8_t* out);
/* bytes: count*48 -> xy: count*12 limbs, inf: count flags, status: count classes (0 = decoded; may be NULL).  A rejected
 * slot gets the C-ABI identity (x = 0, y = 1, inf = 1).  With a context the points are decoded by one kernel launch, a
 * thread per point; ctx = NULL runs the same code on the host.  Word for word the same output either way.  A rejected
 * point is not an error of the call. */
int typlonk_g1_decompress(typlonk_ctx* ctx, const uint8_t* bytes, size_t count, uint32_t flags, uint64_t* xy, uint8_t* inf,
                          uint8_t* status);
/* typlonk_srs_load from len = 48 * points bytes (a ceremony file's points): 48 bytes per point cross PCIe and the kernel
 * writes the SRS's device records directly.  If any point is rejected NO SRS is created: the call returns
 * TYPLONK_ERR_INVALID_ARG, *first_bad (may be NULL) is the lowest rejected index and typlonk_last_error names its class.
 * len not a multiple of 48 returns TYPLONK_ERR_LENGTH. */
int typlonk_srs_load_compressed(typlonk_ctx* ctx, const uint8_t* bytes, size_t len, uint32_t flags, uint32_t* srs_id,
                                size_t* first_bad);
/* typlonk_srs_download as count*48 bytes, compressed on the device. */
int typlonk_srs_download_compressed(typlonk_ctx* ctx, uint32_t srs_id, size_t offset, size_t count, uint8_t* out);

/* ---- a powers-of-tau step: check a loaded SRS against [s]G2, add a contribution ------------------------------------------
 * typlonk_srs_load_compressed judges every point on its own and typlonk_srs_load judges nothing.  typlonk_srs_check decides
 * whether the entry as a whole is g1[i] = [s^i] G for the s of a given [s]G2 -- the one property the provers and verifiers
 * rely on -- and names the lowest point that breaks it.  An invalid SRS is DATA in the report, not an error of the call.
 *   membership  one thread per point over the device records every MSM reads: y^2 = x^3 + 4 and the subgroup of order r.
 *               (A record's coordinates are always canonical: typlonk_srs_load reduces a coordinate >= p mod p, every
 *               other way to make an entry writes canonical ones.)  An identity record passes; the next two steps deal with it.  The lowest failing
 *               index, its class and the total number of failing points are reported, and with bad_points != 0 the call
 *               stops here: nothing that is not a group element is summed or paired.
 *   P0          point 0 is the fixed G1 generator, word for word (the verifiers subtract y G where a constant commits to
 *               c P0).  Otherwise TYPLONK_SRS_BAD_P0, and the call stops here.
 *   ratio       rho = Blake2b-512("typlonk/srs/check/v1" || seed || u64 len || [s]G2 as its 24 limbs), the integers
 *               little-endian and the digest read as a little-endian integer mod r: the conventions of the compact
 *               transcript.  With A_k = sum_{i<k} rho^i g1[i] and B_k = sum_{i<k} rho^i g1[i+1] (two MSMs in one batch over
 *               the entry itself, in table mode where typlonk_srs_precompute has run), prefix k holds when
 *                   e(A_k, [s]G2) * e(-B_k, G2) = 1        (one pairing product on the host: a "fold")
 *               The whole SRS is k = len - 1.  If that fails, the least failing prefix is found by bisection on k with the
 *               same weights, at most ceil(log2 len) more folds, and index = k - 1.  len = 1 runs no fold.
 *   the seed    The library draws no randomness: the 32 bytes are the caller's.  THE SEED MUST BE UNKNOWN TO WHOEVER PRODUCED
 *               THE POINTS: someone who knows it can compute rho and craft defects that cancel under these weights.  Draw it
 *               after the points are fixed.  For a seed chosen independently of the points, a fold accepts a prefix with a
 *               broken link with probability at most len / r (a non-zero polynomial of degree < len in rho), so both the
 *               verdict and the bisection's index err with probability at most (1 + ceil(log2 len)) * len / r.
 *   refusals    TYPLONK_ERR_INVALID_ARG: a null argument, an unknown id, g2s_xy off the twist (as typlonk_verify refuses
 *               it), an SRS shard -- with or without a communicator.  An empty entry: TYPLONK_ERR_LENGTH.  A refused or failed
 *               call leaves *report as it was.
 * Blocks for the result; never a collective.  It uses the MSM lanes and allocations of its own, nothing of a prover's arena,
 * so it may be made while a round-by-round prover is open (between its round calls).  The two len-element weight vectors
 * (64 bytes per point together) are allocated by the call and freed on return. */
#define TYPLONK_SRS_VALID 0
#define TYPLONK_SRS_BAD_POINT 1   /* a point off the curve or outside the subgroup of order r */
#define TYPLONK_SRS_BAD_P0 2      /* point 0 is not the fixed G1 generator */
#define TYPLONK_SRS_BAD_RATIO 3   /* some g1[i+1] != [s] g1[i] for the s of g2s */
typedef struct typlonk_srs_report {
    uint32_t verdict;      /* the FIRST class that applies, in the order above */
    uint32_t point_class;  /* BAD_POINT: TYPLONK_POINT_NOT_ON_CURVE / _NOT_IN_SUBGROUP of the lowest bad point, else 0 */
    uint64_t index;        /* BAD_POINT: the lowest bad point.  BAD_RATIO: the lowest i with g1[i+1] != [s] g1[i].  else 0 */
    uint64_t bad_points;   /* how many points fail membership (a total, as the witness check's counts are) */
    uint32_t folds;        /* pairing products computed */
} typlonk_srs_report;
int typlonk_srs_check(typlonk_ctx* ctx, uint32_t srs_id, const uint64_t g2s_xy[24], const uint8_t seed[32],
                      typlonk_srs_report* report);
/* Host-only, no GPU: the weight rho the check derives from (seed, len, g2s_xy), as 4 Montgomery limbs.  It hashes the 24
 * limbs as given (no curve check); a null argument returns TYPLONK_ERR_INVALID_ARG. */
int typlonk_srs_check_challenge(const uint8_t seed[32], uint64_t len, const uint64_t g2s_xy[24], uint64_t rho[4]);
/* A new SRS entry new[i] = [t^i] g1[i], i < len (canonical affine records; no tables, no shard), and g2s_out = [t] g2s_in
 * (on the host): if the old pair was an SRS for s, the new one is an SRS for s t.  t: 4 Montgomery limbs.  The old entry is
 * untouched (it may hold tables; table 0 is read).  One thread per point: t^i, then 255 doublings and ~128 mixed additions.
 * The result is [t^i] P by the group law for ANY curve point in a record, points of small order included, and an identity
 * stays an identity.  The call does not demand a checked input: check first, or check the result.
 * TYPLONK_ERR_INVALID_ARG: a null argument, an unknown id, t not a canonical residue, t = 0, g2s_in off the twist, an SRS shard
 * (with or without a communicator), and [t] g2s_in = the identity -- which no g2s_in of order r gives; a twist point of
 * small order can, and 24 limbs cannot hold the identity; then *new_srs_id and g2s_out are left as they were.  Blocks.  Out of scope: a proof of knowledge of t and the transcript of
 * a ceremony -- whoever runs one publishes those beside the points. */
int typlonk_srs_contribute(typlonk_ctx* ctx, uint32_t srs_id, const uint64_t t[4], const uint64_t g2s_in[24],
                           uint32_t* new_srs_id, uint64_t g2s_out[24]);
/* The Lagrange form of an SRS and back: an NTT over the first n = 2^log_n points of the entry, taken in the group.
 *   TYPLONK_SRS_TO_LAGRANGE    out[i] = [1/n] sum_{j<n} [w^(-i j)] g1[j]: for g1[j] = [s^j] G this is [L_i(s)] G, L_i the
 *                              Lagrange basis of the domain {w^i}.  s stays unknown: only the points are needed.
 *   TYPLONK_SRS_FROM_LAGRANGE  out[j] = sum_{i<n} [w^(i j)] g1[i], no scaling: the exact inverse of the above, for a caller
 *                              who is handed only Lagrange points and wants the monomial prefix.
 * w is the generator of the size-n domain that typlonk_ntt_fr* uses for the same log_n, and the index order is natural: out[i]
 * goes with row i of an evaluation column, so a commitment to a column of EVALUATIONS (a wire column, selector evaluations)
 * is one typlonk_msm_g1* over the Lagrange entry, with no inverse transform in front.  The new entry has exactly n points
 * (canonical affine records, an identity the all-zero record with its flag; no tables, no shard) and is an SRS entry like
 * any other: every MSM entry point, typlonk_srs_precompute, typlonk_srs_download[_compressed], typlonk_srs_len and
 * typlonk_srs_free take it.  The old entry is untouched (it may hold tables; table 0 is read) and may hold more than n
 * points -- a PLONK SRS holds n + 3 --: the rest is ignored.  The result is the stated sum by the group law for ANY curve
 * points in the records: identities, points of small order, points that are no progression.  (Outside the group of order
 * r an element of Fr is no scalar; there each butterfly applies its twiddle as the canonical integer, -1 as a negation, and
 * the sum is the one the stages spell out -- no step fails on such a point, and the order-r part of every output is exact.)
 * typlonk_srs_check tests the MONOMIAL form only: check first, then convert (or convert back, then check).  The provers
 * keep taking the monomial entry: quotient and opening polynomials are not columns of evaluations.
 * One launch per stage, one thread per butterfly (P, Q) -> (P + [w^k]Q, P - [w^k]Q): about (n/2)(log_n - 1) scalar
 * multiplications of 255 doublings each, and n more for the 1/n of TO_LAGRANGE.  Setup-time.  Blocks.
 * TYPLONK_ERR_INVALID_ARG: a null ctx or new_srs_id, an unknown id, an SRS shard (with or without a communicator), a
 * direction other than the two, 2^log_n > the entry's length, log_n > 25 (the SRS length cap); then nothing is allocated
 * and *new_srs_id is left as it was.  TYPLONK_ERR_OOM if the n x 128 bytes of the new entry are refused. */
#define TYPLONK_SRS_TO_LAGRANGE 0
#define TYPLONK_SRS_FROM_LAGRANGE 1
int typlonk_srs_g1_ntt(typlonk_ctx* ctx, uint32_t srs_id, uint32_t log_n, uint32_t direction, uint32_t* new_srs_id);
/* ---- open() at EVERY point of the evaluation domain in one call (Feist-Khovratovich).  n = 2^log_n, w the generator of the
 * size-n domain that typlonk_ntt_fr* uses, S_m = g1[m] the source entry's points ([s^m]G for a valid SRS), f_0 .. f_(n-1) the
 * coefficients, zero above the m given.  The opening at w^k is pi_k = [q_k(s)]G, q_k = (f - f(w^k)) / (X - w^k); expanded,
 *     h_i  = sum_{m=0}^{n-2-i} f_(m+i+1) S_m   (i = 0 .. n-2),   h_(n-1) = O
 *     pi_k = sum_{i<n} [w^(i k)] h_i            (the direction of TYPLONK_SRS_FROM_LAGRANGE, no scaling)
 * and h, a correlation, is taken as a circular product of size 2n: the TABLE is y = DFT_2n(S_(n-2), ..., S_0, O x (n+1)) in
 * the group (root: the generator of the size-2n domain, no scaling), made once per (SRS, log_n); a call computes
 * v = NTT_2n(f_(n-1), 0 x n, f_0, ..., f_(n-2)) / 2n over Fr, u_i = [v_i] y_i (one scalar multiplication per record),
 * h^ = DFT_2n^-1(u) without scaling -- h_i = h^_i for i < n -- and pi = DFT_n(h).  About n log_n scalar
 * multiplications for the table and n (1.5 log_n + 1.5) per polynomial, where n separate openings cost n MSMs of n terms.
 * As for typlonk_srs_g1_ntt the sums hold by the group law for ANY curve points in the source's records; outside the
 * group of order r a twiddle acts as its canonical integer.
 *
 * typlonk_srs_open_all_table: a new entry of the SRS list holding the 2n records of y (canonical affine; 2n x 128 bytes, and as
 * much again while the call runs).  typlonk_srs_len reports 2n, typlonk_srs_free releases it, typlonk_srs_download reads it; it
 * is no SRS to commit over.  The source entry is untouched (it may hold tables; table 0 is read), may hold more than the
 * n - 1 points the table reads, and may be freed afterwards.  Blocks.
 *   TYPLONK_ERR_DOMAIN       log_n outside 1..24 (2n <= 2^25, the SRS length cap)
 *   TYPLONK_ERR_INVALID_ARG  a null ctx or table_id, an unknown id, an SRS shard (with or without a communicator), a source that
 *                            is itself such a table, a source of fewer than n - 1 points
 *   TYPLONK_ERR_OOM          an allocation is refused
 * A refused call leaves *table_id as it was. */
int typlonk_srs_open_all_table(typlonk_ctx* ctx, uint32_t srs_id, uint32_t log_n, uint32_t* table_id);
/* Opening k and evaluation k of the m coefficients from `offset` of poly, 1 <= m <= n, in natural order, k < n:
 *   proofs_xy / proofs_inf  n records of 12 limbs and n flags: canonical affine Montgomery coordinates, an identity flagged
 *                           -- exactly what typlonk_srs_download writes for the same points
 *   evals                   n x 4 limbs, f(w^k) as canonical Montgomery Fr -- what typlonk_ntt_fr gives for the padded
 *                           coefficients; may be NULL
 * (pi_k, evals[k]) is what typlonk_open_dev at z = w^k followed by typlonk_msm_g1_dev over the source entry gives.  A
 * constant polynomial opens to identities.  Blocks.  Temporaries, freed on return: two buffers of 2n records (2n x 128 bytes
 * each) and one of 2n Fr (2n x 32 bytes) -- 576 n bytes, 576 MiB at n = 2^20 -- beside the transforms' own workspace.
 *   TYPLONK_ERR_INVALID_ARG  a null pointer other than evals, an unknown id, an id that is not such a table
 *   TYPLONK_ERR_LENGTH       m = 0 or m > n
 *   TYPLONK_ERR_RANGE        offset / m outside poly
 *   TYPLONK_ERR_OOM          an allocation is refused
 * A refused call leaves the outputs as they were. */
int typlonk_open_all_dev(typlonk_ctx* ctx, uint32_t table_id, const typlonk_buf* poly, size_t offset, size_t m,
                         uint64_t* proofs_xy /* n*12 */, uint8_t* proofs_inf /* n */, uint64_t* evals /* n*4 or NULL */);
/* The same for m coefficients in HOST memory (4 Montgomery limbs each): they are uploaded into one of the temporaries. */
int typlonk_open_all_host(typlonk_ctx* ctx, uint32_t table_id, const uint64_t* coeffs, size_t m,
                          uint64_t* proofs_xy, uint8_t* proofs_inf, uint64_t* evals);
/* ---- open() on every COSET of the evaluation domain in one call: multi-proofs (Feist-Khovratovich, chunked).  n = 2^log_n,
 * l = 2^log_l, r = n / l >= 2; w, S_m, f as above, and w^l the generator of the size-r domain.  Coset k < r is
 * {w^(k + r t) : t < l}, the roots of X^l - a_k with a_k = w^(k l).  One proof opens f at all l points of a coset:
 *     f    = q_k (X^l - a_k) + I_k,   deg I_k < l,   I_k = f on coset k
 *     pi_k = [q_k(s)] G = sum_{i<r} [w^(l i k)] h_i
 *     h_i  = sum_{m=0}^{n-1-(i+1)l} f_(m+(i+1)l) S_m   (i <= r - 2),   h_(r-1) = O
 * and a verifier that holds [s^l]G2 checks e(C - [I_k(s)]G + [a_k] pi_k, G2) = e(pi_k, [s^l]G2).  With f^(j)_a = f_(a l + j)
 * and S^(j)_a = S_(a l + j) (j < l, a < r), h is the sum over j of the correlations above at size r, and the l of them are
 * summed in the Fourier domain: the TABLE is, for each j, y^(j) = DFT_2r(S^(j)_(r-2), ..., S^(j)_0, O x (r+1)) in the group
 * (root: the generator of the size-2r domain, no scaling), y^(j)_i at record j 2r + i; a call computes
 * v^(j) = NTT_2r(f^(j)_(r-1), 0 x r, f^(j)_0, ..., f^(j)_(r-2)) / 2r over Fr, u_i = sum_{j<l} [v^(j)_i] y^(j)_i for i < 2r
 * (2n scalar multiplications whose doublings are shared among the terms of a sum), h^ = DFT_2r^-1(u) without scaling --
 * h_i = h^_i for i < r -- and pi = DFT_r(h) with root w^l.  The group transforms are of 2r and r records, not 2n and n.
 * With log_l = 0 everything is the section above, record for record.
 *
 * typlonk_srs_open_chunks_table: a new entry of the SRS list holding the 2n records of the l blocks (canonical affine; 2n x 128
 * bytes, and as much again while the call runs); typlonk_srs_len reports 2n, typlonk_srs_free releases it.  With log_l = 0 it
 * holds, word for word, what typlonk_srs_open_all_table makes, and typlonk_open_all_* takes exactly the tables of log_l = 0,
 * of either constructor (others: TYPLONK_ERR_INVALID_ARG).  The source entry is untouched, may hold more than the n - l
 * points the table reads, and may be freed afterwards.  Blocks.
 *   TYPLONK_ERR_DOMAIN       log_n outside 1..24, or log_l >= log_n
 *   TYPLONK_ERR_INVALID_ARG  a null ctx or table_id, an unknown id, an SRS shard (with or without a communicator), a source that
 *                            is itself a table of either constructor, a source of fewer than n - l points
 *   TYPLONK_ERR_OOM          an allocation is refused
 * A refused call leaves *table_id as it was. */
int typlonk_srs_open_chunks_table(typlonk_ctx* ctx, uint32_t srs_id, uint32_t log_n, uint32_t log_l, uint32_t* table_id);
/* The r proofs and n evaluations of each of `count` polynomials over one table (of either constructor): polynomial p is the m
 * coefficients from offsets[p] (offsets = NULL: from 0) of polys[p], 1 <= m <= n, the same m for all.  The same buffer may
 * appear more than once.
 *   proofs_xy / proofs_inf  count x r records of 12 limbs and count x r flags, proof k of polynomial p at p r + k, as
 *                           typlonk_srs_download writes points
 *   evals                   count x n x 4 limbs, CHUNK-MAJOR: evals[(p n + k l + t) 4 ..] = f_p(w^(k + r t)), the l values
 *                           that go with proof k contiguous; canonical Montgomery Fr; may be NULL
 * A polynomial of degree < l opens to identities.  Blocks.  Temporaries, freed on return: two buffers of count x 2r records
 * (128 bytes each), one of count x 2n Fr (32 bytes each) and `count` pointers -- count x (512 r + 64 n + 8) bytes, 72 MiB for
 * one polynomial at n = 2^20, l = 64 -- beside the transforms' own workspace.
 *   TYPLONK_ERR_INVALID_ARG  a null pointer other than offsets / evals, a null entry of polys, an unknown id, an id that is
 *                            no table
 *   TYPLONK_ERR_LENGTH       m = 0 or m > n, count = 0, count x 2r > 2^25 records
 *   TYPLONK_ERR_RANGE        offsets[p] / m outside polys[p]
 *   TYPLONK_ERR_OOM          an allocation is refused
 * A refused call leaves the outputs as they were. */
int typlonk_open_chunks_dev(typlonk_ctx* ctx, uint32_t table_id, const typlonk_buf* const* polys, const size_t* offsets, size_t m,
                            size_t count, uint64_t* proofs_xy /* count*r*12 */, uint8_t* proofs_inf /* count*r */,
                            uint64_t* evals /* count*n*4, chunk-major, or NULL */);
/* The same for coefficients in HOST memory, coeffs[p]: m x 4 Montgomery limbs; they are uploaded into one more temporary of
 * count x m Fr. */
int typlonk_open_chunks_host(typlonk_ctx* ctx, uint32_t table_id, const uint64_t* const* coeffs, size_t m, size_t count,
                             uint64_t* proofs_xy, uint8_t* proofs_inf, uint64_t* evals);
/* ---- verify multi-proofs: a batch of cells per call.  n, l, r, w and a_k = w^(k l) as above.  A CELL i < N is
 * (c_i, k_i, E_i, pi_i): an index c_i < M into the M commitments, a coset index k_i < r, the l evaluations in the order
 * typlonk_open_chunks_* writes them, E_i[t] = f(w^(k_i + r t)), and a proof.  It is valid iff
 *     e(C_(c_i) - [I_i(s)] G + [a_(k_i)] pi_i, G2) = e(pi_i, [s^l] G2)
 * with I_i the polynomial of degree < l that takes the values E_i on coset k_i.  With the weights rho_i = rho^i, i the cell's
 * position in the call, the live cells of a range [lo, hi) are checked by ONE product (a "fold"):
 *     e(sum rho_i pi_i, [s^l]G2) * e(-(sum_c w_c C_c + sum rho_i a_(k_i) pi_i - [A(s)] G), G2) = 1
 *     w_c = sum_{c_i = c} rho_i,    A_j = sum_i rho_i w^(-k_i j) (1/l) sum_t E_i[t] mu^(-j t),   mu = w^r,  j < l
 * Two MSMs over a temporary entry holding the N proofs and the M commitments, one l-term MSM of A over the first l points of
 * entry srs_id (they must be [s^j] G of the same s as g2sl_xy: typlonk_srs_check decides that), a G1 addition and two Miller
 * loops with one final exponentiation on the host.  A, w_c and the weights are computed on the device.
 *   inputs      all in HOST memory.  commits_xy / commits_inf: M points, proofs_xy / proofs_inf: N points, 12 limbs and a flag
 *               each, as typlonk_srs_download writes them (a coordinate >= p is reduced mod p, as typlonk_srs_load does);
 *               cell_commit, cell_coset: N indices each; evals: N x l x 4 limbs, canonical Montgomery Fr; g2sl_xy: [s^l]G2 as
 *               x.c0 x.c1 y.c0 y.c1.
 *   status[i]   the FIRST class that applies to cell i; a bad cell is DATA, not an error of the call:
 *                 TYPLONK_CELL_OK              the equation holds
 *                 TYPLONK_CELL_BAD_EVAL        an evaluation is not a canonical residue (judged on the host before the upload)
 *                 TYPLONK_CELL_BAD_POINT       the proof is off the curve or outside the subgroup of order r
 *                 TYPLONK_CELL_BAD_COMMITMENT  the same, for the cell's commitment
 *                 TYPLONK_CELL_BAD_PROOF       the equation fails
 *               Membership of the N + M points is decided on the device, one flag per point; an identity proof or commitment
 *               is a group element.  A cell of one of the middle three classes is not LIVE: its weights are zero, a point that
 *               failed membership is replaced by the identity, and nothing that is not a group element is summed or paired.
 *   the fold    One fold over all live cells.  If it fails, the live cells are bisected: a range whose fold holds is
 *               accepted, one that fails is cut in half by its live cells, down to single cells; b bad cells cost at most
 *               2 b ceil(log2 N) + 1 folds.  rho_i stays the power of the cell's position in the whole call: the fold of a
 *               sub-range only zeroes the weights outside it.
 *   the seed    rho = Blake2b-512("typlonk/chunks/verify/v1" || seed || u64 log_n || u64 log_l || u64 N || u64 M || [s^l]G2 as
 *               its 24 limbs), read as typlonk_srs_check reads its digest.  The library draws no randomness.  THE SEED MUST BE
 *               UNKNOWN TO WHOEVER PRODUCED THE CELLS: someone who knows it can compute rho and craft defects that cancel
 *               under these weights.  Draw it after the cells are fixed.  For a seed chosen independently of the cells a fold
 *               accepts a range holding a bad cell with probability at most N l / r (r the group order, about 2^255), so a
 *               call errs with probability at most (2 b ceil(log2 N) + 1) N l / r.
 *   report      folds: the pairing products computed; live: the cells that reached the fold; count[s]: the cells of status s.
 *   refusals    judged in this order; a refused or failed call leaves status and *report as they were:
 *     TYPLONK_ERR_INVALID_ARG  a null pointer
 *     TYPLONK_ERR_DOMAIN       log_n outside 1..24; log_l >= log_n; log_l > 10 (a cell's l elements are held in the LDS)
 *     TYPLONK_ERR_LENGTH       N = 0, M = 0, N x l > 2^25 or N + M > 2^25
 *     TYPLONK_ERR_INVALID_ARG  an unknown id; an SRS shard (with or without a communicator) or a table of
 *                              typlonk_srs_open_*_table as srs_id; an entry of fewer than l points; g2sl_xy off the twist
 *     TYPLONK_ERR_RANGE        some cell_commit[i] >= M or cell_coset[i] >= r
 *     TYPLONK_ERR_OOM          an allocation is refused
 * Blocks for the result; never a collective.  Temporaries, allocated by the call and freed on return: (N + M) x 128 bytes of
 * records, N x l x 32 bytes of evaluations, 32 (6 N + 2 M) bytes of weights, 4 (2 N + M + 1) bytes of indices and at most
 * 2048 x l x 32 bytes of partial sums (allocated once, for the whole call's workgroups; every fold of a bisection is cut into
 * strips of the whole call's length and so never has more).  The temporary entry takes an id from the context's SRS ids for the
 * duration of the call, as the temporary entries of typlonk_verify do: the ids handed out afterwards are higher by one. */
#define TYPLONK_CELL_OK 0
#define TYPLONK_CELL_BAD_EVAL 1
#define TYPLONK_CELL_BAD_POINT 2
#define TYPLONK_CELL_BAD_COMMITMENT 3
#define TYPLONK_CELL_BAD_PROOF 4
typedef struct typlonk_chunks_report {
    uint32_t folds;      /* pairing products computed */
    uint32_t reserved;   /* 0 */
    uint64_t live;       /* cells that passed the per-cell checks and reached the fold */
    uint64_t count[5];   /* cells per status, indexed by TYPLONK_CELL_* */
} typlonk_chunks_report;
int typlonk_verify_chunks(typlonk_ctx* ctx, uint32_t srs_id, uint32_t log_n, uint32_t log_l, const uint64_t g2sl_xy[24],
                          const uint8_t seed[32], const uint64_t* commits_xy /* M*12 */, const uint8_t* commits_inf /* M */,
                          size_t M, const uint32_t* cell_commit /* N */, const uint32_t* cell_coset /* N */,
                          const uint64_t* evals /* N*l*4 */, const uint64_t* proofs_xy /* N*12 */,
                          const uint8_t* proofs_inf /* N */, size_t N, uint8_t* status /* N */, typlonk_chunks_report* report);
/* Host-only, no GPU: the weight rho the call derives from (seed, log_n, log_l, N, M, g2sl_xy), as 4 Montgomery limbs.  It
 * hashes the 24 limbs as given (no curve check); a null argument returns TYPLONK_ERR_INVALID_ARG. */
int typlonk_verify_chunks_challenge(const uint8_t seed[32], uint32_t log_n, uint32_t log_l, uint64_t N, uint64_t M,
                                    const uint64_t g2sl_xy[24], uint64_t rho[4]);

/* ---- Recovery of polynomials from a subset of their cells ------------------------------------------------------------------------
 * n = 2^log_n, l = 2^log_l, r = n / l, w the generator of the size-n domain; coset k is {w^(k + r t) : t < l} and a cell holds
 * the l evaluations on one coset in that order, as typlonk_open_chunks_* writes them and typlonk_verify_chunks reads them.
 * The call is given K DISTINCT coset indices cosets[0 .. K) in any order -- the same for all `count` polynomials, a node
 * lacking columns rather than single cells -- and per polynomial p its K cells, evals[((p K + i) l + t) 4 ..] =
 * f_p(w^(cosets[i] + r t)) (Montgomery), and a degree bound m, 1 <= m <= K l.
 * There is exactly one h_p of degree < K l through p's cells.  p is CONSISTENT iff h_p has no nonzero coefficient at an index
 * j, m <= j < K l; then h_p is the only polynomial of degree < m through them and the call returns its m coefficients and/or
 * its n evaluations.  With m = K l every input is consistent and the call is an interpolation.
 *   status[p]   TYPLONK_RECOVER_OK            the outputs hold h_p
 *               TYPLONK_RECOVER_BAD_EVAL      an evaluation of p is not a canonical residue (judged on the host before the upload)
 *               TYPLONK_RECOVER_INCONSISTENT  no polynomial of degree < m takes p's values; first_excess[p] (may be NULL) = the
 *                                             lowest j >= m with a nonzero coefficient of h_p, UINT64_MAX for any other status
 *               A polynomial that is not OK gets zeros in every output that was given.  It is data, not an error of the call:
 *               the other polynomials of the call are not affected.
 *   outputs     at least one of the three:
 *               coeffs_dev  `count` device buffers; coeffs_dev[p] receives m elements at offsets[p] (offsets NULL: at 0),
 *                           stream-ordered on the context's stream: a following typlonk_open_chunks_dev on the same buffers
 *                           makes the proofs
 *               coeffs      count * m elements on the host
 *               evals_out   count * n elements on the host, chunk-major: polynomial p, coset k, point t at ((p r + k) l + t) 4
 *   report      K and r - K, and the polynomials per status
 * The call blocks for the status.  It is not a collective and takes no SRS.
 * Method: with Z the polynomial that vanishes on the r - K missing cosets (constant on each coset of the domain, of period r on
 * the shifted domain g H), the values of h_p Z are known on the WHOLE domain -- the cell's times Z on a known coset, zero on a
 * missing one -- and deg h_p Z < n, so one inverse transform gives h_p Z and a division on g H (a coset transform, a pointwise
 * product with 1 / Z, the inverse coset transform) gives h_p: three batched transforms over the `count` vectors, a fourth for
 * evals_out.  Z on the r cosets and at the r distinct points of g H is 2r plain products of r - K factors: quadratic in r, hence
 * the bound on log_n - log_l.
 * Temporaries, freed when the call returns, in bytes: 32 (count n + count K l + 4 r + 2 r S) for the work vectors, the staged
 * cells, the constants and the S <= 64 partial products of the vanishing values; 4 (2 r - K) of indices (4 (r + 1) at K = r);
 * 32 count m when coeffs or evals_out is given and 32 count n more when evals_out is; count (25 + 8 B) for the verdicts, B <= 256.
 * Refusals, judged in this order (typlonk_last_error names the cause); a refused call leaves every output as it was:
 *     TYPLONK_ERR_INVALID_ARG  a null ctx, cosets, evals, status or report; all three outputs null; a null entry of coeffs_dev
 *     TYPLONK_ERR_DOMAIN       log_n outside 1..24; log_l >= log_n; log_n - log_l > 16
 *     TYPLONK_ERR_LENGTH       K = 0, K > r, count = 0, m = 0, m > K l ("too few cells for this degree bound"), count n > 2^26
 *     TYPLONK_ERR_RANGE        a coset >= r; offsets[p] / m outside coeffs_dev[p]
 *     TYPLONK_ERR_INVALID_ARG  a coset named twice; the same range of one buffer given for two polynomials
 *     TYPLONK_ERR_OOM          an allocation is refused
 * Under typlonk_set_profiling the call records recover_vanish, recover_scatter, recover_interp, recover_divide, recover_finish
 * and -- with evals_out -- recover_evals (ms, each with a wait for the device behind it). */
#define TYPLONK_RECOVER_OK 0
#define TYPLONK_RECOVER_BAD_EVAL 1
#define TYPLONK_RECOVER_INCONSISTENT 2
typedef struct typlonk_recover_report {
    uint32_t known, missing;   /* K, r - K */
    uint64_t count[3];         /* polynomials per status, indexed by TYPLONK_RECOVER_* */
} typlonk_recover_report;
int typlonk_recover_chunks(typlonk_ctx* ctx, uint32_t log_n, uint32_t log_l, size_t m, const uint32_t* cosets /* K */, size_t K,
                           const uint64_t* evals /* count*K*l*4 */, size_t count, typlonk_buf* const* coeffs_dev /* NULL, or count */,
                           const size_t* offsets /* NULL: 0 */, uint64_t* coeffs /* NULL, or count*m*4 */,
                           uint64_t* evals_out /* NULL, or count*n*4 */, uint8_t* status /* count */,
                           uint64_t* first_excess /* NULL, or count */, typlonk_recover_report* report);
/* Host-only.  A field that is not a canonical residue, or a point that is not on the curve, returns
 * TYPLONK_ERR_INVALID_ARG (vk: also a g2s off the twist; log_n outside 1..24 returns TYPLONK_ERR_DOMAIN). */
int typlonk_proof_compact_to_bytes(const typlonk_proof_compact* proof, uint8_t out[TYPLONK_PROOF_COMPACT_BYTES]);
int typlonk_vk_to_bytes(const typlonk_vk* vk, uint8_t out[TYPLONK_VK_WIRE_BYTES]);
/* Host-only (a verifier needs nothing else).  The nine G1 points go through the decoder above; [s]G2 by a square root in
 * Fq2, checked on the twist and -- unless skipped -- for [r] Q = O.  log_n outside 1..24 returns TYPLONK_ERR_DOMAIN; any
 * rejected field TYPLONK_ERR_INVALID_ARG with its decode status in *status (may be NULL; fields: 0..2 the cosets, 3..11
 * the G1 points, 12 [s]G2).  An infinite [s]G2 is TYPLONK_POINT_ENCODING. */
int typlonk_vk_from_bytes(const uint8_t bytes[TYPLONK_VK_WIRE_BYTES], uint32_t flags, typlonk_vk* vk, uint32_t* status);
/* bytes: count * 656.  All 9 * count points are decoded by ONE kernel launch (ctx = NULL: on the host), the scalars on the
 * host.  status[k] = 0: proofs[k] is decoded, its five challenge fields zero (the verifier recomputes them); otherwise
 * TYPLONK_DECODE_STATUS(class, field) of the first bad field and proofs[k] is all identities / zeros.  A rejected proof is
 * not an error of the call; count = 0 is a no-op. */
int typlonk_proof_compact_from_bytes(typlonk_ctx* ctx, const uint8_t* bytes, size_t count, uint32_t flags,
                                     typlonk_proof_compact* proofs, uint32_t* status);
/* typlonk_verify_compact over the wire form: ok[k] = 0 for a proof that does not decode; the others are handed to
 * typlonk_verify_compact together, and ok[k] is its verdict.  pi / pi_len as there, indexed by k.  The key and every pi entry
 * are judged before anything is decoded, by the checks of typlonk_verify_compact itself and with its error codes: a refusal
 * does not depend on which proofs decode. */
int typlonk_verify_compact_bytes(typlonk_ctx* ctx, const typlonk_vk* vk, const uint8_t* bytes, size_t count,
                                 const uint64_t* const* pi, const size_t* pi_len, uint32_t flags, uint8_t* ok);

/* ---- device-resident Fr vectors (so an iNTT result feeds an MSM without crossing PCIe) ---------- */
int typlonk_buf_alloc(typlonk_ctx* ctx, size_t n_elems, typlonk_buf** out);
int typlonk_buf_free(typlonk_ctx* ctx, typlonk_buf* buf);
int typlonk_buf_upload(typlonk_ctx* ctx, typlonk_buf* buf, size_t offset, const uint64_t* src, size_t n_elems);
int typlonk_buf_download(typlonk_ctx* ctx, const typlonk_buf* buf, size_t offset, uint64_t* dst, size_t n_elems);
int typlonk_buf_zero(typlonk_ctx* ctx, typlonk_buf* buf, size_t offset, size_t n_elems);
size_t typlonk_buf_len(const typlonk_buf* buf);
void* typlonk_buf_devptr(const typlonk_buf* buf);

/* ---- host-only helpers (no GPU needed) --------------------------------------------------------- */
/* Fold `count` affine points in index order: the deterministic combine step after an all-gather of
 * per-GPU partial MSM results (RCCL has no elliptic-curve reduction). */
int typlonk_g1_sum_host(const uint64_t* xy, const uint8_t* inf, size_t count, uint64_t out_xy[12], uint8_t* out_inf);
/* The fold the library applies after its all-gather, exposed for hosts that run their own exchange (MPI, sockets):
 * `records` = what an all-gather of the ranks' send buffers yields, rank-major: world x count records of 13 uint64
 * (12 limbs x || y, then the infinity flag in bits 0..31; bits 32.. non-zero = "this rank failed", its error code).
 * out point i = sum over ranks r of record (r, i), folded in rank order.  Returns TYPLONK_ERR_COMM and the failing
 * rank in *failed_rank (may be NULL) when a record is flagged.  Host-only, no GPU. */
#define TYPLONK_COMM_RECORD_WORDS 13
int typlonk_g1_fold_records_host(const uint64_t* records, size_t world, size_t count, uint64_t* out_xy /* count*12 */,
                                 uint8_t* out_inf /* count */, int* failed_rank);

/* ---- measurement -------------------------------------------------------------------------------
 * With profiling on, every kernel stage of the next MSM / NTT call is bracketed by HIP events on
 * the context's stream.  typlonk_profile_get returns up to `cap` (name, milliseconds) pairs of the
 * last call and the number of stages it had.
 *   on = 0  off
 *   on = 1  every stage (sort, accumulate, reduce, NTT passes ...): ~0.1 ms of event traffic per MSM, and NTT calls wait
 *           for their result
 *   on = 2  the dominant kernel only (the bucket accumulation launches, "msm_accum"): what a timed loop can afford */
int typlonk_set_profiling(typlonk_ctx* ctx, int on);
int typlonk_profile_get(typlonk_ctx* ctx, const char** names, float* ms, int cap);
/* Pippenger shape chosen for an m-term MSM: window bits c, number of windows, and the number of
 * group operations (mixed adds + full adds + doublings) the kernels execute for it. */
int typlonk_msm_plan(typlonk_ctx* ctx, size_t m, uint32_t* window_bits, uint32_t* n_windows, uint64_t* group_ops);

/* Self-test of the device's field inversion (the per-point `into_affine` of kzg/src/lib.rs:50 and kzg/src/srs.rs:20 is
 * one Fq inversion): `count` pseudo-random and edge residues, lazily reduced up to 8p, inverted by the divsteps routine
 * the kernels use and by the Fermat ladder a^(p-2); *mismatches = results that differ (or fail x * x^-1 = 1),
 * *max_rounds = the largest number of 30-divstep rounds any call ran (proven bound: 37). */
int typlonk_selftest_fq_inv(typlonk_ctx* ctx, uint64_t seed, size_t count, uint64_t* mismatches, uint32_t* max_rounds);

const char* typlonk_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TYPLONK_H */
