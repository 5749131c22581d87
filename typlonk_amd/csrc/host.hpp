// Shared state of the host driver of libtyplonk_hip.so (implementation of include/typlonk.h for gfx950).
//   ctx.hip       context, workspaces, profiling events, device vectors
//   ntt_host.hip  NTT staging: plan (ntt_plan.hpp: every decision, no device needed), acquire the tables it lists, queue its
//                 passes; the table cache + typlonk_ntt_*
//   msm_host.hip  MSM staging: plan (msm_plan.hpp: every decision, no device needed), size the workspace, queue the sort /
//                 accumulate / reduce launches; lanes of a batch, host finish + SRS + typlonk_msm_*
//   comm.hip      RCCL exchange behind the C ABI
//   prover.hip    quotient, grand product, openings, the prover rounds, typlonk_prove; the steps it shares with prove_batch.hip
//                 (declared below: prover_workspaces, coset_g, quotient_domain, round3_openings, lin_*); transcripts:
//                 proof_script.hpp
//   prove_batch.hip  typlonk_prove_batch: many witnesses of one circuit in waves, every stage batched across the wave
//   prove_plan.hpp   where a proof's data lives (no device needed): the arena's regions, the roles of q, the result slots, the
//                 scratch layouts, and the size of every workspace of a prover call.  ensure() on ops_tmp, prover_mem, quot_ext,
//                 quot_tab and batch_tab is called by prover_workspaces and the three stand-alone entry points of prover.hip only
//   verify.hip    typlonk_verify, typlonk_verify_compact (the prover of the compact shape is in prover.hip); which scalars and
//                 points they and the wire format admit: host_checks.hpp; the linearisation commitment: lin_commit.hpp
//   witness_solve.hip  typlonk_witness_solve: the wire columns of a witness from the circuit's inputs, level by level
//                 (solve_plan.hpp: every decision, no device needed); typlonk_circuit_set_hints: advice the solve computes
//   witness_check.hip  typlonk_circuit_permutation, typlonk_witness_check: which gate rows and copy constraints a witness fails;
//                 typlonk_circuit_compile: a circuit from selector evaluations and the permutation itself (sigma_cell.hpp)
//   srs_check.hip typlonk_srs_check, typlonk_srs_contribute: a loaded SRS against [s]G2, and [t^i] g1[i]; typlonk_srs_g1_ntt:
//                 the Lagrange form of an SRS and back (kernels: srs_gen.hip, g1_fft.hip)
//   open_chunks.hip  typlonk_srs_open_chunks_table, typlonk_open_chunks_*: a polynomial's openings on every coset of its domain,
//                 and typlonk_srs_open_all_table, typlonk_open_all_*: the same at one point per coset (kernels: g1_fft.hip)
// There is deliberately no CPU compute fallback: without a HIP device typlonk_init fails with TYPLONK_ERR_NO_DEVICE.
#pragma once
#include "../../include/typlonk.h"
#include "g1.hpp"
#include "g1_host64.hpp"
#include "launch.hpp"
#include "ntt_plan.hpp"
#include "prove_plan.hpp"
#include "solve_plan.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace typlonk {
namespace pairing {
struct G2Affine;   // host/pairing_host.hpp
}
}  // namespace typlonk

namespace tyh {
using namespace ty;

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

struct SrsEntry {
    uint32_t* d_points = nullptr;  // len * PT_WORDS u32 (96 B payload on a 128-B stride), identity = (0,0)
    size_t len = 0;
    uint32_t table_c = 0, table_T = 0;  // fixed-base tables 2^(c t) P_i at index t*len + i (typlonk_srs_precompute)
    bool table_centred = false;         // table_T counts the windows of CENTRED scalars (launch.hpp, msm_windows)
    // typlonk_srs_set_shard: this entry holds bases [shard_first, shard_first + len) of a total_len-point SRS
    size_t shard_first = 0, total_len = 0;
    // typlonk_srs_open_all_table: this entry is the table of the domain of 2^open_all_log_n points (len = twice that many
    // records); 0: not a table
    uint32_t open_all_log_n = 0;
    // typlonk_srs_open_chunks_table: the table's cosets hold 2^open_chunks_log_l points each (l blocks of 2n / l records);
    // 0: one point per coset, the table of typlonk_srs_open_all_table
    uint32_t open_chunks_log_l = 0;
    size_t total() const { return total_len ? total_len : len; }
    // part [off, off + ml) of an m-term MSM that falls into this entry
    void local_range(size_t m, size_t* off, size_t* ml) const {
        const size_t lo = std::min(shard_first, m), hi = std::min(shard_first + len, m);
        *off = lo;
        *ml = hi - lo;
    }
};

struct Table {
    Fr* d = nullptr;
    size_t n = 0;
    uint64_t last_use = 0;  // typlonk_ctx::table_tick at the last lookup (coset tables are evicted LRU)
};

// Per-circuit constants of the quotient: the 4n coset evaluations of q_l q_r q_o q_m q_c, sigma_0..2
// and L0 (9 vectors).  They are fixed per CompiledCircuit (plonk/src/lib.rs:19-35), so they are
// transformed once instead of on every proof.
struct CircuitEntry {
    Fr* ext = nullptr;     // 9 * 4n : coset evaluations of q_l q_r q_o q_m q_c sigma_0..2 L0
    Fr* coef = nullptr;    // 8 * n  : coefficient copies of the selectors and sigmas (linearisation, sigma(zeta))
    Fr* sig_ev = nullptr;  // 3 * n  : sigma evaluations over the domain (grand product)
    uint32_t log_n = 0;
    // typlonk_circuit_commitments: the eight commitments of `coef`, computed once per SRS id (ids are never reused)
    struct Commitments {
        uint64_t xy[8][12];
        uint8_t inf[8];
    };
    std::map<uint32_t, Commitments> commitments;
    // typlonk_circuit_permutation / typlonk_witness_check (witness_check.hip), built on first use -- a circuit made by
    // typlonk_circuit_compile holds the permutation it was compiled from, for the cosets it was compiled with, from the start:
    uint32_t* perm = nullptr;       // 3n : successor map of the cells recovered from sig_ev (TYPLONK_CELL_NONE: no cell id)
    uint64_t perm_cosets[3][4] = {};  //      the cosets it was recovered for (other cosets rebuild it)
    bool perm_ready = false;
    uint64_t perm_defects = 0;      //      cells without an image + cells that are the image of != 1 cells
    uint32_t perm_first_bad = 0;    //      the lowest such cell
    Fr* sel_ev = nullptr;           // 5n : selector evaluations over the domain
    // typlonk_witness_solve (witness_solve.hip), built on first use per (circuit, cosets): the plan (solve_plan.hpp; of its
    // tables the host keeps src, for the admission of a call's cells, and the schedule) and its tables on the device
    struct Solve {
        bool ready = false;
        uint64_t cosets[3][4] = {};
        SolvePlan plan;                 // order and level are dropped once the tables are uploaded
        uint32_t* d_src = nullptr;      // 3n
        uint32_t* d_order = nullptr;    // driven rows
        uint32_t* d_level_off = nullptr;  // depth + 1
        Fr* d_qo_inv = nullptr;         // n : 2^28 / q_o of a driven row, zero elsewhere
        void* d_hints = nullptr;        // the plan's hints as the kernels read them (witness_solve.hip), null without hints
        uint32_t n_hints = 0;           //   (= hints.size() of the entry when the cache was built)
    } solve;
    // typlonk_circuit_set_hints: the installed hints; every plan of this circuit is built under them
    std::vector<SolveHint> hints;
};

struct ProfStage {
    const char* name;
    hipEvent_t a, b;
};

// Everything one in-flight MSM needs: grow-only device workspaces, the stream it was enqueued on and
// the pinned landing zone of its window sums.  A context owns one per lane, so that a batch of independent
// MSMs (prove() issues them in groups: 3 wire commitments, 5-6 openings, 3 quotient slices --
// plonk/src/proof.rs:107-110, 147-175, 181) can overlap one MSM's host-side finish (window combine, affine
// normalisation) and kernel tail with the next one's sort + accumulate.
constexpr size_t HOST_WIN_POINTS = 32 * 2 * RC_NB;  // up to 32 bucket sets x {rows, columns} x RC_NB bit planes

// Outputs of the bucket sort of one chunk of terms; a workspace owns two sets so that the sort of chunk k + 1 can run
// (on the workspace's side stream) while chunk k is being accumulated.
struct SortBufs {
    DevBuf keys, sorted, counts, offsets, cursor, blocksums, order, ohist, blk_hist, blk_base, blk_cnt, seg_start, heavy, tasks, hpart;
    std::vector<DevBuf*> all() {
        return {&keys, &sorted, &counts, &offsets, &cursor, &blocksums, &order, &ohist, &blk_hist, &blk_base, &blk_cnt, &seg_start,
                &heavy, &tasks, &hpart};
    }
};
constexpr size_t MSM_FOUR_LANES_BELOW = (size_t)1 << 17;  // typlonk_ctx::msm_inflight

struct MsmWs {
    SortBufs sb[2];
    DevBuf buckets, part_a, part_b, rc_sums, rc_bits, rc_out;
    hipStream_t stream = nullptr;
    hipStream_t side = nullptr;     // sorts of the chunks after the first (created on first use)
    hipEvent_t ev_in = nullptr, ev_sorted[MSM_MAX_CHUNKS] = {}, ev_acc[MSM_MAX_CHUNKS] = {};
    uint32_t* host_wins = nullptr;  // pinned, HOST_WIN_POINTS x 48 words
    bool pending = false;
    uint32_t W = 0, c = 0;
    bool rc = false;                // row/column reduction: host_wins holds bit planes (launch.hpp)
    RcShape rcs{};
    uint64_t* out_xy = nullptr;
    uint8_t* out_inf = nullptr;
};

constexpr size_t COMM_REC = 13;  // 12 limbs + the infinity flag, one u64 each: 104 bytes per point and rank
struct Comm {
    void* comm = nullptr;        // ncclComm_t (comm.hip)
    int rank = 0, world = 0;
    uint64_t* d_send = nullptr;  // cap records
    uint64_t* d_recv = nullptr;  // world * cap records
    uint64_t* h_buf = nullptr;   // pinned: cap records out + world * cap records back
    size_t cap = 0;
};

}  // namespace tyh

struct typlonk_buf {
    ty::Fr* d = nullptr;
    size_t n = 0;
};

// Environment switches read by typlonk_init.  Each forces one of the forms the default policy itself picks by shape, so
// the parity tests can reach every form at every shape (every combination gives the same bits):
//   TYPLONK_MSM_INFLIGHT  MSMs of a batch in flight at once (1..4; default: by SRS length, MsmQueue)
//   TYPLONK_MSM_CHAIN     0 | 1: the lanes of a batch run free / chain their accumulations (default: by term count)
//   TYPLONK_MSM_CHUNKS    chunks of a stand-alone MSM (0 = by length)
//   TYPLONK_MSM_LANES     lanes per bucket of the accumulation (1, 2, 4, 8, 16; 0 = by bucket load)
//   TYPLONK_MSM_SCATTER   staged | direct: level 1 of the bucket sort stages its runs in the LDS / writes entry by entry
//   TYPLONK_MSM_REDUCE    rc4: always the four-launch row/column bucket reduction (default: two launches for small bucket sets)
//   TYPLONK_NTT_FR30      0 | 1 | 2: the 9 x 30-bit butterflies never / where they measure faster / always
//   TYPLONK_NTT_BIG       0 | 1 | 2: the two-pass 2^20 plan (4096-element tiles) never / where it measures faster / always
// (TYPLONK_RCCL_LIB, read by comm.hip, names the RCCL library to load.)
struct typlonk_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string err;
    std::map<uint32_t, tyh::SrsEntry> srs;
    uint32_t next_srs = 1;
    std::map<uint32_t, tyh::CircuitEntry> circuits;
    uint32_t next_circuit = 1;
    tyh::DevBuf srs_comb;          // fixed-base comb of G (typlonk_srs_generate, srs_gen.hip)
    bool srs_comb_ready = false;   // set once the comb's build kernel has run to completion
    // MSM
    tyh::DevBuf scal;
    static constexpr int MSM_LANES = 4;
    tyh::MsmWs ws[MSM_LANES];
    hipStream_t lane[MSM_LANES] = {};  // lanes 1.. of typlonk_msm_g1_batch* (lane 0 = stream)
    int msm_inflight = 0;           // MSMs of a batch in flight at once (1..MSM_LANES; 0 = by SRS length: 3, where the
                                    // accumulations are chained and a fourth lane only adds a sort competing for the same
                                    // slots (profiles/r03_msm_chain_ab.txt), 4 below 2^17 points, where they run free)
    hipEvent_t lane_evt[MSM_LANES] = {};  // "scalars ready" marks (MsmQueue::submit)
    hipEvent_t batch_fence = nullptr;   // typlonk_msm_g1_batch_devptr: everything queued before the call (MsmQueue::fence)
    // Queued MSMs (a batch, a prover round) run their accumulations ONE AFTER THE OTHER, whichever lanes they are on: the
    // kernel fills every SIMD by itself, so two of them side by side only take turns -- while the sort of the next MSM
    // and the reduction of the previous one, latency-bound kernels, do hide beside an accumulation.  Without the chain
    // the lanes move in lockstep (four sorts together, four accumulations together, four reductions together) and
    // nothing overlaps (profiles/r03_msm_batch_timeline_before.txt).
    hipEvent_t accum_chain = nullptr;
    bool accum_chain_live = false;
    // A short accumulation does NOT fill the chip: below 2^17 terms the lanes run free (profiles/r04_ab_chain_by_size.txt:
    // prove() at 2^16 5.75 -> 5.09 ms, 2^14 4.18 -> 3.41, 2^12 3.24 -> 3.05).  Free lanes also win inside a 2^17 / 2^18
    // proof (7.4 -> 7.2, 11.8 -> 11.4 ms) but lose in a pure batch of nine 2^17-term MSMs -- an 8-way shard's round,
    // 0.419 -> 0.464 ms per MSM -- so the switch sits below the shard size; from 2^19 on the chain is never worse and
    // 2^20 needs it.  -1 = by term count (MSM_CHAIN_MIN_TERMS), 0 / 1 = TYPLONK_MSM_CHAIN.
    int msm_chain = -1;
    tyh::Fr* eval_slots_host = nullptr;  // pinned, device-visible result slots: PROVE_SLOTS per proof in flight
    size_t eval_slots_cap = 0;           // (prover_workspaces grows them)
    int msm_chunks = 0;            // chunks of a stand-alone MSM (0 = choose by length)
    int msm_lanes = 0;             // lanes per bucket of the accumulation (0 = choose by bucket load)
    bool msm_scatter_staged = true;  // TYPLONK_MSM_SCATTER=direct: level 1 of the bucket sort writes every entry straight to global
                                   // memory (the rounds 1-5 form, the A/B reference) instead of staging runs in the LDS
    bool msm_rc4 = false;          // always the four-launch row/column reduction
    // NTT
    tyh::DevBuf ntt_scratch, ntt_io, quot_ext, quot_tab, ops_tmp, prover_mem;
    tyh::DevBuf wc_ws, wc_stage;   // typlonk_witness_check: masks, counts and lists of a launch; the host form's staged columns
    tyh::DevBuf eval_ws;           // typlonk_poly_eval_dev: points, results and chunk partials (poly_eval.hip)
    tyh::DevBuf batch_tab;         // typlonk_prove_batch: per-proof scalars and item tables of a wave (device copy of batch_host)
    void* batch_host = nullptr;    // pinned staging of batch_tab (PbTables, prove_plan.hpp)
    bool prover_busy = false;  // one proof in flight per context (the arena above is shared)
    int prover_rounds_active = 0;  // > 0 while a typlonk_prover_round* call is running (ProverRound)
    std::map<std::string, tyh::Table> tables;
    uint64_t table_tick = 0;
    // tables keyed by a caller-chosen coset shift ("cs:" keys) are a cache, not a plan: at most this many distinct
    // (direction, size, shift) groups / bytes stay resident, the least recently used group is dropped first
    static constexpr size_t COSET_GROUPS_MAX = 8;
    static constexpr size_t COSET_BYTES_MAX = (size_t)3 << 30;
    int ntt_fr30 = 1;              // 0 = the 8 x 32-bit kernel everywhere, 1 = the default policy (9 x 30-bit butterflies, fr30.hpp, for
                                   // every inverse transform and for forward ones up to 2^NTT_FR30_FWD_MAX_LOG), 2 = 30-bit everywhere
    int ntt_big = 1;               // TYPLONK_NTT_BIG: the two-pass 2^20 plan on 4096-element tiles 0 = never, 1 = where it measures
                                   // faster (ntt_plan), 2 = for every 2^20 transform outside a prover round
    // profiling
    bool profiling = false;
    bool prof_light = false;       // typlonk_set_profiling(ctx, 2): only the bucket-accumulation launches are bracketed
    std::vector<tyh::ProfStage> prof;
    std::vector<hipEvent_t> event_pool;  // timing events of finished stages, reused by the next call
    std::vector<std::pair<const char*, float>> prof_result;
    tyh::Comm comm;                // typlonk_comm_init: RCCL communicator of this rank (world = 0: none)
};

namespace tyh {

int fail(typlonk_ctx* c, int code, const std::string& msg);

#define HIPCHK(expr)                                                                                      \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess)                                                                             \
            return tyh::fail(ctx, _e == hipErrorOutOfMemory ? TYPLONK_ERR_OOM : TYPLONK_ERR_HIP,          \
                             std::string(#expr) + ": " + hipGetErrorString(_e));                          \
    } while (0)

// the same mapping for call sites that cannot return from the middle (a status to carry on with)
inline int hip_rc(typlonk_ctx* ctx, hipError_t e) {
    if (e == hipSuccess) return TYPLONK_OK;
    return fail(ctx, e == hipErrorOutOfMemory ? TYPLONK_ERR_OOM : TYPLONK_ERR_HIP, hipGetErrorString(e));
}

int ensure(typlonk_ctx* ctx, DevBuf& b, size_t bytes);   // grow-only device workspace
void release(DevBuf& b);

// Frees the device allocations registered with it unless dismiss()ed: setup functions allocate several
// buffers and may fail half-way (HIPCHK returns early).
struct DevGuard {
    std::vector<void*> ptrs;
    void* add(void* p) {
        ptrs.push_back(p);
        return p;
    }
    void dismiss() { ptrs.clear(); }
    ~DevGuard() {
        for (void* p : ptrs)
            if (p) (void)hipFree(p);
    }
};
struct ProverRound {
    typlonk_ctx* ctx;
    explicit ProverRound(typlonk_ctx* c) : ctx(c) { ++c->prover_rounds_active; }
    ~ProverRound() { --ctx->prover_rounds_active; }
};
// Stage events are per call: composite calls switch them off for their inner calls and restore on every exit path.
struct ProfilingOff {
    typlonk_ctx* ctx;
    bool saved;
    explicit ProfilingOff(typlonk_ctx* c) : ctx(c), saved(c->profiling) { c->profiling = false; }
    ~ProfilingOff() { ctx->profiling = saved; }
};

// ---- profiling ------------------------------------------------------------------------------
struct StageTimer {
    typlonk_ctx* ctx;
    bool on;
    hipEvent_t a = nullptr, b = nullptr;
    const char* name;
    hipStream_t st;
    StageTimer(typlonk_ctx* c, const char* n, hipStream_t s = nullptr)
        : ctx(c), on(c->profiling && (!c->prof_light || strcmp(n, "msm_accum") == 0)), name(n), st(s ? s : c->stream) {
        if (on) {
            a = take();
            b = take();
            (void)hipEventRecord(a, st);
        }
    }
    // events are recycled through the context (creating two per stage and call costs more than recording them)
    hipEvent_t take() {
        hipEvent_t e = nullptr;
        if (!ctx->event_pool.empty()) {
            e = ctx->event_pool.back();
            ctx->event_pool.pop_back();
        } else {
            (void)hipEventCreate(&e);
        }
        return e;
    }
    ~StageTimer() {
        if (on) {
            (void)hipEventRecord(b, st);
            ctx->prof.push_back({name, a, b});
        }
    }
};
void prof_begin(typlonk_ctx* ctx);
void prof_collect(typlonk_ctx* ctx);

// ---- ntt_host.hip ---------------------------------------------------------------------------------------------------
Fr fr_domain_root(uint32_t log_n);      // generator of the size-2^log_n domain (ark-poly Radix2EvaluationDomain::group_gen)
Fr fr_domain_root_inv(uint32_t log_n);
Fr fr_inv_pow2(uint32_t log_n);         // (2^log_n)^-1 (size_inv)
Fr fr_from_u64(uint64_t x);
// the forward two-level twiddles of the 2^log_n domain, w its generator: lo[j] = w^j (j < 2^h), hi[j] = w^(j 2^h)
// (j < 2^(log_n - h)) -- the very tables (one cache entry each) a transform's inter-pass twiddles of that row length are
int domain_twiddles(typlonk_ctx* ctx, uint32_t log_n, const Fr** lo, const Fr** hi, uint32_t* h);
// short_in / n_valid: the transform of a ZERO-PADDED vector -- the first pass reads short_in[0, n_valid) and takes every
// element beyond as zero (no padded copy, no reads of zeros or of their coset factors); the result lands in d_data.
int ntt_run(typlonk_ctx* ctx, Fr* d_data, uint32_t log_n, int inverse, const uint64_t* coset_shift, bool sync = true,
            const Fr* short_in = nullptr, uint64_t n_valid = ~0ull);
// `count` transforms of one size / direction / coset, pass by pass in shared launches (d_data[v] in place; short_in: NULL or
// one zero-padded source per vector, all n_valid long)
int ntt_run_batch(typlonk_ctx* ctx, Fr* const* d_data, size_t count, uint32_t log_n, int inverse, const uint64_t* coset_shift,
                  bool sync = true, const Fr* const* short_in = nullptr, uint64_t n_valid = ~0ull);

// ---- msm_host.hip ---------------------------------------------------------------------------------------------------
void write_affine_out(const G1Affine& a, uint64_t out_xy[12], uint8_t* out_inf);   // internal affine -> the C-ABI's arkworks form
int msm_validate(typlonk_ctx* ctx, uint32_t srs_id, size_t m, const SrsEntry** srs);
// d_scalars points at coefficient 0 of the m-term vector (ptr_is_local: at the first coefficient of this
// entry's share instead); an SRS shard sums only its own index range
// h_scalars != NULL (with ptr_is_local): the local share still lives on the host and is copied chunk by chunk beside the kernels
int msm_run(typlonk_ctx* ctx, uint32_t srs_id, const Fr* d_scalars, size_t m, uint64_t out_xy[12], uint8_t* out_inf,
            bool ptr_is_local = false, const uint64_t* h_scalars = nullptr);
// count independent MSMs over the same SRS, up to MSM_LANES in flight (separate workspaces/streams)
int msm_batch(typlonk_ctx* ctx, uint32_t srs_id, const void* const* d_scalars, const size_t* m, size_t count, uint64_t* out_xy,
              uint8_t* out_inf);
int msm_finish(typlonk_ctx* ctx, MsmWs& ws);
// `count` resident records from d_points -> the C-ABI's arkworks form (typlonk_srs_download's output); blocks
int points_to_host(typlonk_ctx* ctx, const uint32_t* d_points, size_t count, uint64_t* xy, uint8_t* inf);

// ---- srs_check.hip --------------------------------------------------------------------------------------------------
// the l >= 1 stages of `blocks` transforms of 2^l records each in the group, queued on the context's stream, one launch per
// stage: stage 1 reads block b at src + b * src_stride records through the bit reversal into dst + b * dst_stride, the later
// ones work on dst in place (strides >= 2^l; src and dst must not overlap).  No scaling.
int g1_ntt_stages(typlonk_ctx* ctx, uint32_t l, uint64_t blocks, const uint32_t* src, uint64_t src_stride, uint32_t* dst,
                  uint64_t dst_stride, bool inverse);

// Asynchronous MSM submissions over one SRS (a prover round, or typlonk_msm_g1_batch_devptr).
//   submit()    puts an MSM on the next lane of [lane_lo, lanes): the lane first waits for everything queued on the
//               context's stream so far -- the kernels that produce the scalars -- and a lane that still holds an
//               unfinished MSM is finished first (the only way submit() blocks).  Work queued on the context's stream
//               AFTER the call runs concurrently with the MSM.  Lane 0 is the context's stream itself.
//   wait_all()  finishes every MSM in flight (host-side window combine + affine normalisation of each).
// out_xy / out_inf of an MSM must stay valid until it has been finished.
struct MsmQueue {
    typlonk_ctx* ctx;
    const SrsEntry* srs;
    int lanes, lane_lo, next;
    hipEvent_t fence = nullptr;  // set: the lanes wait for this mark instead of for everything on the context's stream
    MsmQueue(typlonk_ctx* c, const SrsEntry* s, int first_lane = 0);
    // keep the context's stream (lane 0) free for other work when there is another lane to use
    void set_first_lane(int l);
    int submit(const Fr* d_scalars, size_t m, uint64_t* out_xy, uint8_t* out_inf, bool standalone = false);
    int wait_all();
};
// A round's queue outlives every early return of the round: its MSMs write into the caller's outputs.
struct WaitAll {
    MsmQueue& q;
    ~WaitAll() { (void)q.wait_all(); }
};

// ---- prover.hip: the linearisation polynomial r (proof.rs:376-439), shared by typlonk_prove and typlonk_prove_batch ------
// What it needs of zeta alone: zeta^n, Z_H(zeta) = zeta^n - 1 and L0(zeta) (one host inversion).
void lin_zeta_terms(const Fr& zeta, uint32_t log_n, Fr* zn, Fr* zh, Fr* l0z);
// r = sum_k scalar[k] * poly_k + constant, the ten polynomials in this order: q_l q_r q_o q_m q_c, Z, sigma_2, t_lo, t_mid,
// t_hi.  ev[0..4] = a, b, c, Z at zeta (Z(zeta) unused) and Z at zeta w; s0, s1 = sigma_0, sigma_1 at zeta; pi_z = PI(zeta).
void lin_scalars(const Fr* ev, const Fr& s0, const Fr& s1, const Fr& pi_z, const Fr& beta, const Fr& gamma, const Fr (&k)[3],
                 const Fr& alpha, const Fr& zeta, const Fr& zn, const Fr& zh, const Fr& l0z, Fr* scalar /* LIN_TERMS */, Fr* constant);

// where the ten polynomials lie: coef = the circuit's coefficient copies (CircuitEntry::coef), z and t = the proof's Z and
// quotient (t_lo, t_mid, t_hi are t's first 3n coefficients).  pb_fold_kernel (prove_batch.hip) reads the same ten fused.
TY_HD void lin_polys(const Fr* coef, const Fr* z, const Fr* t, uint64_t n, const Fr** poly /* LIN_TERMS */) {
    for (int k = 0; k < 5; ++k) poly[k] = coef + k * n;
    poly[5] = z;
    poly[6] = coef + 7 * n;
    for (int k = 0; k < 3; ++k) poly[7 + k] = t + k * n;
}

// ---- prover.hip: the steps typlonk_prove* and typlonk_prove_batch* share ---------------------------------------------------
// The quotient's coset generator: Fr's multiplicative generator 7 (7^(4n) != 1, so X^n - 1 never vanishes on g H_4n), as
// the limbs the transforms take; g_out: the same as an Fr.
const uint64_t* coset_g(Fr* g_out = nullptr);
// THE sizing site of a prover call: every workspace the plan names grown to its size (grow-only: the call drains the device and
// discards contents when it must re-allocate, so it comes before anything is queued), the pinned slots and a wave's staging
int prover_workspaces(typlonk_ctx* ctx, const ProvePlan& plan);
// The quotient's domain g H_4n for n = 2^log_n: x_i = g w_{4n}^i = g * w_lo[i & (2^w_h - 1)] * w_hi[i >> w_h] (n_hi entries of
// w_hi; a caller folds g and what else it has per call into a scaled copy), and X^n - 1 there, which takes only the four
// values g^n iota^k - 1 (iota = w_{4n}^n, k = i mod 4): their inverses.
struct QuotientDomain {
    const Fr* w_lo;
    const Fr* w_hi;
    uint64_t n_hi;
    uint32_t w_h;
    Fr g;
    const uint64_t* g_limbs;
    Fr zh_inv[4];
};
int quotient_domain(typlonk_ctx* ctx, uint32_t log_n, QuotientDomain* d);

// Round 3's openings and evaluations of one proof; where each result lands (a pinned slot per proof) depends on the proof
// shape: Round3Slots, prove_plan.hpp.  r(zeta) and F come after these and are not part of the list.
struct Round3Polys {
    const Fr* co;     // a, b, c: n apart (PR_CO)
    const Fr* z;
    const Fr* pi;     // null: the zero polynomial
    Fr* q;            // the proof's witness polynomials, n apart (PR_Q; roles: ProveQ)
    const Fr* coef;   // CircuitEntry::coef
    uint64_t n;
};
// emit(poly, quotient or null, slot, point) for every item; point 0 = zeta, 1 = zeta w.  with_quotients: a, b, c, Z are
// opened at zeta one by one (the reference shape's six openings); Z at zeta w always has its quotient.
template <class Emit>
void round3_openings(const Round3Slots& s, bool with_quotients, const Round3Polys& p, Emit emit) {
    for (int i = 0; i < 3; ++i) emit(p.co + i * p.n, with_quotients ? p.q + (Q_WIT_A + i) * p.n : nullptr, s.wire + i, 0);
    emit(p.z, with_quotients ? p.q + Q_WIT_Z * p.n : nullptr, s.z, 0);
    emit(p.coef + 5 * p.n, nullptr, s.sig0, 0);
    emit(p.coef + 6 * p.n, nullptr, s.sig1, 0);
    if (p.pi) emit(p.pi, nullptr, s.pi, 0);
    emit(p.z, p.q + Q_WIT_ZW * p.n, s.zw, 1);
}

// ---- prover.hip: the tail typlonk_circuit_load and typlonk_circuit_compile share ------------------------------------------
// e.ext <- the coset evaluations of the eight coefficient vectors src[0..8) (n each; they may be e.coef's own) and of L0;
// sigma_forward: e.sig_ev holds sigma's coefficients and is transformed to evaluations in place.  Blocks until the circuit is
// usable, then enters `e` into the context and hands out its id.  On failure nothing is entered and the caller still owns
// e's allocations.
int circuit_finish(typlonk_ctx* ctx, CircuitEntry& e, const Fr* const src[8], bool sigma_forward, uint32_t* circuit_id);

// ---- poly_eval.hip / verify.hip ----------------------------------------------------------------------------------------
// out[(p * n_points + k) * 4 ..] = polys[p](points[k]) over m coefficients each (device pointers; points / out on the host,
// 4 Montgomery limbs per element).  Blocks for the result.
int poly_eval_run(typlonk_ctx* ctx, const Fr* const* polys, size_t count, uint64_t m, const uint64_t* points, size_t n_points,
                  uint64_t* out);
// the eight commitments of a circuit over a whole SRS (>= n points): computed on first use per (circuit, SRS), then cached
int circuit_commitments(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const CircuitEntry::Commitments** out);
// an SRS SHARD's share of the statement, to be folded over the ranks by the caller: this rank's partial sums of the eight
// commitments (cached per (circuit, SRS) like the above) and its P0 record -- the point on the rank that holds index 0, the
// identity elsewhere.  Local: no collective inside.
int circuit_statement_partial(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, uint64_t xy[9][12], uint8_t inf[9]);
// THE assembly of a verifying key without [s]G2 (zero) from log_n, the cosets and the statement's nine records: the eight
// commitments, then SRS point 0 (whole, or folded over the ranks)
void vk_assemble(uint32_t log_n, const uint64_t cosets[3][4], const uint64_t (*rec_xy)[12], const uint8_t* rec_inf, typlonk_vk* vk);
// that key of a circuit over a whole SRS
int circuit_vk_fill(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const uint64_t cosets[3][4], typlonk_vk* vk);
// what typlonk_verify_compact refuses before it looks at a proof, in its order and with its codes: log_n outside 1..24, a
// pi_len[k] > n or a null pi[k] with pi_len[k] != 0, a g2s off the twist, a vk point off the curve, a non-canonical coset
// (typlonk_verify_compact_bytes judges its arguments by the same function, before it decodes anything).  *g2s = the key's
// [s]G2 as parsed.
int verify_compact_check_args(typlonk_ctx* ctx, const typlonk_vk* vk, size_t count, const uint64_t* const* pi, const size_t* pi_len,
                              typlonk::pairing::G2Affine* g2s);

// ---- the columns of a call (the provers, the witness check, the compiles) ----------------------------------------------
// One column: `rows` elements on the device or still on the HOST; the rest of the n it stands for are zero.
struct ColumnSrc {
    const Fr* dev = nullptr;
    const uint64_t* host = nullptr;
    uint64_t rows = 0;
    bool present() const { return dev || host; }
};
// dst[0, n) <- the column: its rows with the copy its place asks for, zeros behind them; stream-ordered
inline hipError_t column_to_device(Fr* dst, const ColumnSrc& c, uint64_t n, hipStream_t s) {
    hipError_t e = c.dev ? hipMemcpyAsync(dst, c.dev, c.rows * sizeof(Fr), hipMemcpyDeviceToDevice, s)
                         : hipMemcpyAsync(dst, c.host, c.rows * sizeof(Fr), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && c.rows < n) e = hipMemsetAsync(dst + c.rows, 0, (n - c.rows) * sizeof(Fr), s);
    return e;
}
// What a caller handed in: `count` items (witnesses, or the one circuit of a compile) of `k` columns each, item-major, as
// typlonk_buf handles or as host pointers; per item an optional public-input column, read by one of two rules.  A single
// proof is count == 1 over the addresses of the caller's own arguments.
struct ColumnsOf {
    enum PiRule {
        NO_PI,
        PI_FULL,    // the reference shape: the n rows of the column, where there is one
        PI_FIRST,   // the compact shape: the column's first pi_len[item] rows
    };
    struct Names {   // what the refusals call the columns
        const char *null_column, *short_column, *rows_not_n;
    };
    static constexpr Names WIRES{"null wire column", "wire column shorter than n", "wire columns must hold exactly n rows"};
    static constexpr Names SELECTORS{"null selector column", "selector column shorter than n",
                                     "selector columns must hold exactly n rows"};
    size_t count = 0;
    int k = 3;
    const Names* names = &WIRES;
    const typlonk_buf* const* bufs = nullptr;   // count * k handles, or
    const uint64_t* const* host = nullptr;      // count * k host pointers
    const typlonk_buf* const* pi_bufs = nullptr;   // null, or one (handle or null) per item
    const uint64_t* const* pi_host = nullptr;
    const size_t* pi_len = nullptr;             // PI_FIRST: null = no item has public inputs
    PiRule rule = NO_PI;
    bool rows_stated = false;                   // a host form that passes its columns' length: it must be n (admit_rows)
    size_t rows = 0;

    ColumnsOf(const typlonk_buf* const* cols, size_t items, PiRule r = NO_PI, const typlonk_buf* const* pi = nullptr, const size_t* len = nullptr)
        : count(items), bufs(cols), pi_bufs(pi), pi_len(len), rule(r) {}
    ColumnsOf(const uint64_t* const* cols, size_t items, PiRule r = NO_PI, const uint64_t* const* pi = nullptr, const size_t* len = nullptr)
        : count(items), host(cols), pi_host(pi), pi_len(len), rule(r) {}
    ColumnsOf& with_rows(size_t r) {
        rows_stated = true;
        rows = r;
        return *this;
    }
    ColumnsOf& selectors() {
        k = 5;
        names = &SELECTORS;
        return *this;
    }

    bool given() const { return bufs || host; }
    bool on_device() const { return bufs != nullptr; }
    ColumnSrc column(size_t item, int i, uint64_t n) const {
        ColumnSrc c;
        if (bufs) c.dev = bufs[k * item + i]->d;
        else c.host = host[k * item + i];
        c.rows = n;
        return c;
    }
    bool has_pi(size_t item) const { return bufs ? (pi_bufs && pi_bufs[item]) : (pi_host && pi_host[item]); }
    // rows of the item's public-input column that are read (0: the zero polynomial)
    uint64_t pi_rows(size_t item, uint64_t n) const {
        if (rule == PI_FIRST) return pi_len ? pi_len[item] : 0;
        return rule == PI_FULL && has_pi(item) ? n : 0;
    }
    ColumnSrc pi(size_t item, uint64_t n) const {   // (of admitted columns)
        ColumnSrc c;
        if (!(c.rows = pi_rows(item, n))) return c;
        if (bufs) c.dev = pi_bufs[item]->d;
        else c.host = pi_host[item];
        return c;
    }
};
// THE admission of a call's columns for a domain of n rows: the first refusal, or TYPLONK_OK.  Column by column a null one,
// then a handle of fewer than n elements; then item by item the public inputs.  tests/golden/column_refusals.json pins where
// each entry point places this among its other refusals, and which refusal wins when a call makes two mistakes.
inline int admit_columns(typlonk_ctx* ctx, const ColumnsOf& in, uint64_t n) {
    for (size_t c = 0; c < in.k * in.count; ++c) {
        if (in.bufs ? !in.bufs[c] : !in.host[c]) return fail(ctx, TYPLONK_ERR_INVALID_ARG, in.names->null_column);
        if (in.bufs && in.bufs[c]->n < n) return fail(ctx, TYPLONK_ERR_RANGE, in.names->short_column);
    }
    for (size_t item = 0; item < in.count; ++item) {
        if (in.rule == ColumnsOf::PI_FULL && in.bufs && in.has_pi(item) && in.pi_bufs[item]->n < n)
            return fail(ctx, TYPLONK_ERR_RANGE, "public-input column shorter than n");
        const uint64_t len = in.rule == ColumnsOf::PI_FIRST ? in.pi_rows(item, n) : 0;
        if (!len) continue;
        if (!in.has_pi(item)) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "pi_len != 0 without public inputs");
        if (in.bufs && in.pi_bufs[item]->n < len) return fail(ctx, TYPLONK_ERR_RANGE, "public-input buffer shorter than pi_len");
        if (len > n) return fail(ctx, TYPLONK_ERR_LENGTH, "more public inputs than rows");
    }
    return TYPLONK_OK;
}
// ... and of the length a host form states for its columns.  (A function of its own: the entry points judge it at three
// different places -- the compact prover before the columns, the witness check and the compiles right behind them, the batch
// provers behind the SRS.)
inline int admit_rows(typlonk_ctx* ctx, const ColumnsOf& in, uint64_t n) {
    if (in.rows_stated && in.rows != n) return fail(ctx, TYPLONK_ERR_LENGTH, in.names->rows_not_n);
    return TYPLONK_OK;
}

// ---- witness_check.hip ----------------------------------------------------------------------------------------------
// frees a circuit's recovered permutation, selector evaluations and solve tables (typlonk_circuit_free, typlonk_destroy)
void circuit_check_release(CircuitEntry& e);
// e.perm for these cosets and e.sel_ev, made on first use; a circuit whose sigma is no permutation of the cells is refused
// (TYPLONK_ERR_INVALID_ARG, the lowest defective cell named).  Blocks.  typlonk_witness_check and typlonk_witness_solve.
int circuit_check_prepare(typlonk_ctx* ctx, CircuitEntry& e, const uint64_t cosets[3][4]);
// ---- witness_solve.hip ----------------------------------------------------------------------------------------------
void circuit_solve_release(CircuitEntry& e);
// where the permutation a compile keeps comes from: 3n successors in HOST memory, or a producer that writes them into the
// kept copy on the device (perm_pairs.hip), or neither: the identity
struct PermSource {
    const uint32_t* host = nullptr;
    int (*fill)(typlonk_ctx* ctx, uint32_t* d_perm, void* arg) = nullptr;
    void* arg = nullptr;
};
// typlonk_circuit_compile behind its entry points and behind typlonk_circuit_compile_pairs
int circuit_compile_from(typlonk_ctx* ctx, const ColumnsOf& in, const PermSource& from, const uint64_t cosets[3][4], uint32_t log_n,
                         uint32_t* circuit_id, uint64_t* defects);

// ---- comm.hip -------------------------------------------------------------------------------------------------------
void comm_release(typlonk_ctx* ctx);
// every point <- sum over the ranks of that rank's point (all-gather + fold in rank order); local_rc: the status of the
// local work the points come from -- a failed rank still joins the collective, with flagged records
int comm_fold(typlonk_ctx* ctx, uint64_t* xy, uint8_t* inf, size_t count, int local_rc = TYPLONK_OK);
// does this MSM / prover call need the fold?  (an SRS shard on a context with a communicator)
bool comm_folds(typlonk_ctx* ctx, uint32_t srs_id);

}  // namespace tyh
