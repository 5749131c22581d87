// libtyplonk_hip.so -- typlonk_witness_solve_plan, typlonk_witness_solve: the three wire columns of a witness from a handful of
// assigned cells and the public values, on the device, for `count` witnesses per call.  The step between a compiled circuit and
// typlonk_witness_check / the provers (the reference's C::run filling the advice columns gate by gate, builder.rs:381-396).
// Part of the host driver of include/typlonk.h (see host.hpp for the shared state).
//
//   1. set-up, once per (circuit, cosets)   the permutation and the selector evaluations of the check cache; one kernel over
//                             q_o: the driven flags and 2^28 / q_o per driven row (fr_inv_divsteps); both tables' inputs are
//                             downloaded once and solve_plan() (solve_plan.hpp, host) says where every cell's value comes
//                             from, the level of every driven row and the launches; src, order and level_off go up.
//   2. a call                 the free-slot -> argument table and the values go up; then the plan's launches in stream order:
//                             a level wider than 256 rows is one launch over rows x witnesses, a run of narrow levels one
//                             launch of one workgroup per witness that steps through them (values travel through the output
//                             columns in global memory: a workgroup-scope fence and a barrier between levels); the fill launch
//                             writes the cells of the undriven rows.  Every cell is written exactly once.
//   No kernel waits on another workgroup: order across workgroups is stream order between launches.
//   3. hints (typlonk_circuit_set_hints)   a free class whose value is f(another cell's value): the inverse (fr_inv_divsteps) or
//                             a window of bits.  The plan lists a hint in its level like a row, after the level's rows; its value
//                             goes to a per-witness table in the call's workspace, which later levels and the fill read.  A
//                             circuit with hints runs the HINTS = true instances of the kernels, any other the code it always ran.
//
// Arithmetic is fr30.hpp's, as in witness_check.hip: operands may be any value below 2^256 (the public values are the caller's
// words), data stay in arkworks' form x * 2^256, and fr30_mul(q, a) = q a * 2^242 for two data words.  Per driven row
//   t = fr30_mul(q_l, a) + fr30_mul(q_r, b) + fr30_mul(fr30_mul(fr30_mul(a, b), 2^284), q_m) + fr30_mul(q_c + PI, 2^256)
// holds the numerator with the factor 2^242, and c = fr30_mul(t, 2^284 / q_o) is the data word of the quotient: five products
// of the equation and two radix fixes; the last product's result is below 2r and is stored as the canonical residue.
#include "host.hpp"
#include "host_checks.hpp"
#include "fr30.hpp"
#include "fr_inv.hpp"
#include "scan_ops.hpp"

using namespace ty;
using namespace tyh;

namespace {

constexpr uint32_t SV_BLOCK = SOLVE_NARROW;    // threads of every workgroup here
constexpr uint32_t SLOT_UNASSIGNED = 0xffffffffu;

// a witness of a call as the kernels see it
struct SvWitness {
    Fr* w[3];
    const Fr* pi;       // may be null when pi_len = 0
    uint64_t pi_len;
    const Fr* vals;     // this witness's n_cells values (canonical)
};

// a hint as the kernels read it: its source resolved to what src[] says of the cell the hint names
struct SvHint {
    uint32_t kind, from, shift, width;
};

struct SolveArgs {
    const Fr* sel;              // 5n selector evaluations
    const Fr* qo_inv;           // n
    const uint32_t* src;        // 3n
    const uint32_t* order;      // driven rows and hints by level
    const uint32_t* level_off;  // depth + 1
    const uint32_t* slot_arg;   // free slot -> index into the call's cells, or SLOT_UNASSIGNED
    const SvWitness* wit;
    uint64_t n;
    Fr c256, c284;              // 2^256 mod r, 2^284 mod r (canonical words; unpacked where they are used)
    // only a circuit with hints reads these (the kernels' HINTS = true instances)
    const SvHint* hints;
    Fr* htab;                   // the hint tables of this launch's witnesses: n_hints values each, witness-major
    uint32_t n_hints;
};

// q_o -> driven flag and 2^28 / q_o (Montgomery), zero for an undriven row.  Every lane runs the inversion (its early exit
// is a wave vote), lanes past n on zero.
__global__ __launch_bounds__(256) void solve_setup_kernel(const Fr* qo, uint64_t n, Fr c28, uint8_t* driven, Fr* qo_inv) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    Fr q = Fr::zero();
    if (j < n) q = fr30_to_canonical(fr30_reduce_lazy(fr30_unpack(p_ld(qo + j))));
    const Fr inv = fe_mul(fr_inv_divsteps(q), c28);
    if (j < n) {
        driven[j] = q.is_zero() ? 0 : 1;
        p_st(qo_inv + j, inv);
    }
}

// Every kernel below has two instances.  HINTS = false is the code of a circuit without hints: no entry of its level lists and
// no source is a hint, and nothing of the hint path is compiled in.  HINTS = true serves a circuit with hints installed.

// the value src names: the c column at a driven row (written by an earlier level), a hint's value in this witness's table
// `ht` (written by an earlier level), or a free slot's assigned value or zero
template <bool HINTS>
__device__ __forceinline__ Fr solve_fetch(const SolveArgs& a, const SvWitness& wt, const Fr* ht, uint32_t s) {
    if (!(s & SOLVE_FREE)) return p_ld(wt.w[2] + s);
    if (HINTS && solve_is_hint(s)) return p_ld(ht + (s & ~SOLVE_HINT));
    const uint32_t arg = a.slot_arg[s & ~SOLVE_FREE];
    return arg == SLOT_UNASSIGNED ? Fr::zero() : p_ld(wt.vals + arg);
}

// the three cells of driven row j
template <bool HINTS>
__device__ __forceinline__ void solve_row(const SolveArgs& a, const SvWitness& wt, const Fr* ht, uint32_t j) {
    const uint64_t n = a.n;
    const Fr wa = solve_fetch<HINTS>(a, wt, ht, a.src[j]), wb = solve_fetch<HINTS>(a, wt, ht, a.src[n + j]);
    const Fr30 a30 = fr30_unpack(wa), b30 = fr30_unpack(wb);
    Fr30 t = fr30_mul(fr30_unpack(p_ld(a.sel + j)), a30);
    t = fr30_add(t, fr30_mul(fr30_unpack(p_ld(a.sel + n + j)), b30));
    const Fr30 ab = fr30_mul(fr30_mul(a30, b30), fr30_unpack(a.c284));
    t = fr30_add(t, fr30_mul(ab, fr30_unpack(p_ld(a.sel + 3 * n + j))));
    Fr30 cst = fr30_unpack(p_ld(a.sel + 4 * n + j));
    if (j < wt.pi_len) cst = fr30_add(cst, fr30_unpack(p_ld(wt.pi + j)));
    t = fr30_add(t, fr30_mul(cst, fr30_unpack(a.c256)));
    const Fr c = fr30_to_canonical(fr30_mul(t, fr30_unpack(p_ld(a.qo_inv + j))));
    p_st(wt.w[0] + j, wa);
    p_st(wt.w[1] + j, wb);
    p_st(wt.w[2] + j, c);
}

// bits [shift, shift + width) of the integer x stands for, as a residue.  x leaves Montgomery form first: the window is cut from
// the eight 32-bit words of the integer in [0, r), three of them at most (width <= 64 and shift mod 32 <= 31 make 95 bits); words
// past the eighth read as zero, so do bits 255 and above.  The words are picked by comparison, not indexed: they stay registers.
__device__ __forceinline__ Fr hint_bits(const Fr& x, uint32_t shift, uint32_t width) {
    const Fr v = fe_from_mont(x);
    const uint32_t wi = shift >> 5, sh = shift & 31;
    uint32_t w0 = 0, w1 = 0, w2 = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) {
        w0 = wi == i ? v.v[i] : w0;
        w1 = wi + 1 == i ? v.v[i] : w1;
        w2 = wi + 2 == i ? v.v[i] : w2;
    }
    const uint64_t lo = ((uint64_t)w1 << 32) | w0;
    uint64_t bits = sh ? (lo >> sh) | ((uint64_t)w2 << (64 - sh)) : lo;
    if (width < 64) bits &= (1ull << width) - 1;
    Fr o = Fr::zero();
    o.v[0] = (uint32_t)bits;
    o.v[1] = (uint32_t)(bits >> 32);
    return fe_to_mont(o);
}

// Hint h of a level, for the lanes with `mine` set.  EVERY lane of a wavefront that holds a hint entry is sent here, not only
// the lanes that hold one: fr_inv_divsteps leaves its loop on a vote of the wavefront (__any over g != 0), so it is called
// outside any branch on a lane's own data, as solve_setup_kernel calls it -- a lane without an INV0 hint inverts zero, which is
// 0 -> 0 and keeps its g at zero, so the vote is decided by the lanes that do invert.  The branches around the inversion and
// around the window are on votes too: a wavefront of BITS hints alone skips the inversion whole, and the other way round.
__device__ __forceinline__ void solve_hint(const SolveArgs& a, const SvWitness& wt, Fr* ht, bool mine, uint32_t h) {
    SvHint t{0, SOLVE_FREE, 0, 1};
    Fr x = Fr::zero();
    if (mine) {
        t = a.hints[h];
        x = solve_fetch<true>(a, wt, ht, t.from);
    }
    const bool inv = mine && t.kind == SOLVE_HINT_INV0, bits = mine && t.kind == SOLVE_HINT_BITS;
    Fr out = Fr::zero();
    // (values are chosen word by word: a choice between two whole Fr is a choice between two addresses, and they go to scratch)
    if (__any(inv)) {
        Fr xi;
#pragma unroll
        for (int i = 0; i < 8; ++i) xi.v[i] = inv ? x.v[i] : 0;
        out = fr_inv_divsteps(xi);   // zero for a lane that does not invert
    }
    if (__any(bits)) {
        const Fr y = hint_bits(x, t.shift, t.width);
#pragma unroll
        for (int i = 0; i < 8; ++i) out.v[i] = bits ? y.v[i] : out.v[i];
    }
    if (mine) p_st(ht + h, out);
}

// entry e of a level list, held by the lanes with `live` set: a driven row, or SOLVE_HINT | h
template <bool HINTS>
__device__ __forceinline__ void solve_entry(const SolveArgs& a, const SvWitness& wt, Fr* ht, bool live, uint32_t e) {
    if (!HINTS) {
        if (live) solve_row<false>(a, wt, ht, e);
        return;
    }
    const bool hint = live && solve_is_hint(e);
    if (live && !hint) solve_row<true>(a, wt, ht, e);
    if (__any(hint)) solve_hint(a, wt, ht, hint, e & ~SOLVE_HINT);
}

// one level wider than a workgroup: entries order[off, off + rows), a thread per entry, the witness in blockIdx.y
template <bool HINTS>
__global__ __launch_bounds__(SV_BLOCK) void solve_wide_kernel(SolveArgs a, uint32_t off, uint32_t rows) {
    const uint32_t i = blockIdx.x * SV_BLOCK + threadIdx.x;
    if (!HINTS && i >= rows) return;
    const bool live = i < rows;
    solve_entry<HINTS>(a, a.wit[blockIdx.y], HINTS ? a.htab + (uint64_t)blockIdx.y * a.n_hints : nullptr, live, live ? a.order[off + i] : 0);
}

// levels [first, first + levels), each of at most SV_BLOCK entries: one workgroup per witness (blockIdx.x) steps through them.
// A level's c values and hint values are read by later levels through global memory: the fence orders this workgroup's stores
// (to the columns and to the witness's hint table alike) before the barrier, and no other workgroup touches this witness's
// columns or its table.
template <bool HINTS>
__global__ __launch_bounds__(SV_BLOCK) void solve_run_kernel(SolveArgs a, uint32_t first, uint32_t levels) {
    const SvWitness wt = a.wit[blockIdx.x];
    Fr* const ht = HINTS ? a.htab + (uint64_t)blockIdx.x * a.n_hints : nullptr;
    uint32_t lo = a.level_off[first];
    for (uint32_t l = 0; l < levels; ++l) {
        const uint32_t hi = a.level_off[first + l + 1];
        const bool live = lo + threadIdx.x < hi;
        if (HINTS) {
            solve_entry<true>(a, wt, ht, live, live ? a.order[lo + threadIdx.x] : 0);
        } else if (live) {
            solve_row<false>(a, wt, ht, a.order[lo + threadIdx.x]);
        }
        lo = hi;
        __threadfence_block();
        __syncthreads();
    }
}

// the cells of the undriven rows, a thread per row: each takes its class's value (a driven row's c cell names itself in src),
// a hinted class's from the witness's hint table
template <bool HINTS>
__global__ __launch_bounds__(SV_BLOCK) void solve_fill_kernel(SolveArgs a) {
    const uint64_t j = (uint64_t)blockIdx.x * SV_BLOCK + threadIdx.x, n = a.n;
    if (j >= n || a.src[2 * n + j] == (uint32_t)j) return;
    const SvWitness wt = a.wit[blockIdx.y];
    const Fr* ht = HINTS ? a.htab + (uint64_t)blockIdx.y * a.n_hints : nullptr;
#pragma unroll
    for (int i = 0; i < 3; ++i) p_st(wt.w[i] + j, solve_fetch<HINTS>(a, wt, ht, a.src[(uint64_t)i * n + j]));
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
static_assert(sizeof(SolveHint) == sizeof(typlonk_hint) && sizeof(typlonk_hint) == 16, "SolveHint is typlonk_hint, field for field");
static_assert(SOLVE_HINT_INV0 == TYPLONK_HINT_INV0 && SOLVE_HINT_BITS == TYPLONK_HINT_BITS, "the kinds of solve_plan.hpp are the header's");

void free_solve_tables(CircuitEntry::Solve& s) {
    (void)hipFree(s.d_src);
    (void)hipFree(s.d_order);
    (void)hipFree(s.d_level_off);
    (void)hipFree(s.d_qo_inv);
    (void)hipFree(s.d_hints);
    s = CircuitEntry::Solve{};
}

void free_solve_cache(CircuitEntry& e) { free_solve_tables(e.solve); }

// why solve_plan refused a circuit or its hints, in the caller's words
int refuse_plan(typlonk_ctx* ctx, const SolvePlan& p, const std::vector<SolveHint>& hints) {
    const std::string h = "hints[" + std::to_string(p.bad) + "]";
    switch (p.status) {
        case SOLVE_BAD_PERM:
            return fail(ctx, TYPLONK_ERR_INVALID_ARG, "malformed circuit: sigma is not a permutation of the cells (cell " + std::to_string(p.bad) + ")");
        case SOLVE_CYCLE:
            return fail(ctx, TYPLONK_ERR_INVALID_ARG,
                        std::string("the circuit cannot be solved by propagation: the ") + (hints.empty() ? "rows'" : "rows' and hints'") +
                            " dependencies have a cycle (row " + std::to_string(p.bad) + " is the lowest that could not be scheduled)");
        case SOLVE_HINT_CYCLE:
            return fail(ctx, TYPLONK_ERR_INVALID_ARG, "the hints' dependencies have a cycle: every row can be scheduled, " + h +
                                                          " is the lowest hint that could not be");
        case SOLVE_HINT_KIND: return fail(ctx, TYPLONK_ERR_INVALID_ARG, h + " has an unknown kind");
        case SOLVE_HINT_CELL: return fail(ctx, TYPLONK_ERR_INVALID_ARG, h + ": dst or src is no cell of the circuit");
        case SOLVE_HINT_RANGE: return fail(ctx, TYPLONK_ERR_INVALID_ARG, h + ": width must be in 1..64 and shift in 0..254");
        case SOLVE_HINT_DRIVEN: return fail(ctx, TYPLONK_ERR_INVALID_ARG, h + ": dst lies in a driven class: its value is a row's output");
        case SOLVE_HINT_CLASH:
            return fail(ctx, TYPLONK_ERR_INVALID_ARG, h + ": dst lies in the class hints[" + std::to_string(p.other) + "] writes");
        default: return TYPLONK_OK;
    }
}

// the plan and tables of a solve of `e` under these cosets and hints, built into `out` (which must be empty); on a refusal or
// an error nothing is kept and `e` is as it was (but for the check cache, which circuit_check_prepare may have made)
int build_solve(typlonk_ctx* ctx, CircuitEntry& e, const uint64_t cosets[3][4], const std::vector<SolveHint>& hints,
                CircuitEntry::Solve& out) {
    int rc = circuit_check_prepare(ctx, e, cosets);
    if (rc) return rc;
    const uint64_t n = 1ull << e.log_n, n3 = 3 * n;
    hipStream_t st = ctx->stream;
    Fr* d_inv = nullptr;
    uint8_t* d_flags = nullptr;
    DevGuard guard;
    HIPCHK(hipMalloc((void**)&d_inv, n * sizeof(Fr)));
    guard.add(d_inv);
    HIPCHK(hipMalloc((void**)&d_flags, n));
    DevGuard transient;
    transient.add(d_flags);
    hipLaunchKernelGGL(solve_setup_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const Fr*)(e.sel_ev + 2 * n), n,
                       fr_from_u64(1u << 28), d_flags, d_inv);
    HIPCHK(hipGetLastError());
    std::vector<uint32_t> perm(n3);
    std::vector<uint8_t> driven(n);
    HIPCHK(hipMemcpyAsync(perm.data(), e.perm, n3 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(driven.data(), d_flags, n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    SolvePlan p = solve_plan(perm.data(), driven.data(), n, hints.data(), hints.size());
    if (p.status != SOLVE_OK) return refuse_plan(ctx, p, hints);
    uint32_t *d_src = nullptr, *d_order = nullptr, *d_off = nullptr;
    SvHint* d_hints = nullptr;
    HIPCHK(hipMalloc((void**)&d_src, n3 * sizeof(uint32_t)));
    guard.add(d_src);
    HIPCHK(hipMalloc((void**)&d_order, std::max<size_t>(p.order.size(), 1) * sizeof(uint32_t)));
    guard.add(d_order);
    HIPCHK(hipMalloc((void**)&d_off, p.level_off.size() * sizeof(uint32_t)));
    guard.add(d_off);
    HIPCHK(hipMemcpyAsync(d_src, p.src.data(), n3 * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (!p.order.empty())
        HIPCHK(hipMemcpyAsync(d_order, p.order.data(), p.order.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_off, p.level_off.data(), p.level_off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    // a hint reads what src says of the cell it names: the value the solve writes to that very cell
    std::vector<SvHint> hv(hints.size());
    for (size_t h = 0; h < hints.size(); ++h) hv[h] = SvHint{hints[h].kind, p.src[hints[h].src], hints[h].shift, hints[h].width};
    if (!hv.empty()) {
        HIPCHK(hipMalloc((void**)&d_hints, hv.size() * sizeof(SvHint)));
        guard.add(d_hints);
        HIPCHK(hipMemcpyAsync(d_hints, hv.data(), hv.size() * sizeof(SvHint), hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    guard.dismiss();
    // what a call still reads on the host: src (the admission of its cells), level_off (a wide launch's entries), the schedule
    std::vector<uint32_t>().swap(p.order);
    std::vector<uint32_t>().swap(p.level);
    std::vector<uint32_t>().swap(p.hint_level);
    out.plan = std::move(p);
    out.d_src = d_src;
    out.d_order = d_order;
    out.d_level_off = d_off;
    out.d_qo_inv = d_inv;
    out.d_hints = d_hints;
    out.n_hints = (uint32_t)hints.size();
    memcpy(out.cosets, cosets, sizeof(out.cosets));
    out.ready = true;
    return TYPLONK_OK;
}

// e.solve for these cosets, under the installed hints: built on first use, and again when the cosets change
int ensure_solve(typlonk_ctx* ctx, CircuitEntry& e, const uint64_t cosets[3][4]) {
    if (e.solve.ready && memcmp(e.solve.cosets, cosets, sizeof(e.solve.cosets)) == 0) return circuit_check_prepare(ctx, e, cosets);
    free_solve_cache(e);
    return build_solve(ctx, e, cosets, e.hints, e.solve);
}

int find_circuit(typlonk_ctx* ctx, uint32_t circuit_id, CircuitEntry** e) {
    auto ci = ctx->circuits.find(circuit_id);
    if (ci == ctx->circuits.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown circuit id");
    *e = &ci->second;
    return TYPLONK_OK;
}

}  // namespace

namespace tyh {
void circuit_solve_release(CircuitEntry& e) { free_solve_cache(e); }
}  // namespace tyh

int typlonk_circuit_set_hints(typlonk_ctx* ctx, uint32_t circuit_id, const uint64_t cosets[3][4], const typlonk_hint* hints, size_t n_hints) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    if (!cosets || (n_hints && !hints)) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    if (n_hints >= (1u << 30)) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "too many hints");
    CircuitEntry* e = nullptr;
    int rc = find_circuit(ctx, circuit_id, &e);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    ProfilingOff prof_off(ctx);
    std::vector<SolveHint> hv(n_hints);
    for (size_t h = 0; h < n_hints; ++h) hv[h] = SolveHint{hints[h].kind, hints[h].dst, hints[h].src, hints[h].shift, hints[h].width};
    // the new plan is built beside the cached one, which stays in force if this one is refused
    CircuitEntry::Solve fresh;
    rc = build_solve(ctx, *e, cosets, hv, fresh);
    if (rc) return rc;
    free_solve_cache(*e);
    e->solve = std::move(fresh);
    e->hints = std::move(hv);
    return TYPLONK_OK;
}

int typlonk_witness_solve_plan(typlonk_ctx* ctx, uint32_t circuit_id, const uint64_t cosets[3][4], typlonk_solve_info* info) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    if (!cosets || !info) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    CircuitEntry* e = nullptr;
    int rc = find_circuit(ctx, circuit_id, &e);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    ProfilingOff prof_off(ctx);
    rc = ensure_solve(ctx, *e, cosets);
    if (rc) return rc;
    const SolvePlan& p = e->solve.plan;
    info->driven_rows = p.driven_rows;
    info->free_classes = p.free_classes;
    info->depth = p.depth;
    info->launches = p.launches();
    return TYPLONK_OK;
}

int typlonk_witness_solve(typlonk_ctx* ctx, uint32_t circuit_id, const uint64_t cosets[3][4], const uint32_t* cells, size_t n_cells,
                          const uint64_t* values, const typlonk_buf* const* pi, const size_t* pi_len, size_t count,
                          typlonk_buf* const* wire_out) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    if (count == 0) return TYPLONK_OK;
    if (!cosets || !wire_out || (n_cells && (!cells || !values))) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    CircuitEntry* ep = nullptr;
    int rc = find_circuit(ctx, circuit_id, &ep);
    if (rc) return rc;
    CircuitEntry& e = *ep;
    const uint64_t n = 1ull << e.log_n;
    const ColumnsOf out(wire_out, count, ColumnsOf::PI_FIRST, pi, pi_len);
    rc = admit_columns(ctx, out, n);
    if (rc) return rc;
    for (size_t i = 0; i < n_cells; ++i)
        if (cells[i] >= 3 * n) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "cells[" + std::to_string(i) + "] is no cell of the circuit");
    for (size_t k = 0; k < count; ++k)
        for (size_t i = 0; i < n_cells; ++i)
            if (!fr_canonical(values + (k * n_cells + i) * 4))
                return fail(ctx, TYPLONK_ERR_INVALID_ARG,
                            "the value of cells[" + std::to_string(i) + "] (witness " + std::to_string(k) + ") is not a canonical Fr residue");
    HIPCHK(hipSetDevice(ctx->device));
    ProfilingOff prof_off(ctx);
    rc = ensure_solve(ctx, e, cosets);
    if (rc) return rc;
    const CircuitEntry::Solve& sv = e.solve;
    const SolvePlan& p = sv.plan;
    // the free slot every assigned cell names
    std::vector<uint32_t> slot_arg(std::max<uint64_t>(p.free_classes, 1), SLOT_UNASSIGNED);
    for (size_t i = 0; i < n_cells; ++i) {
        const uint32_t s = p.src[cells[i]];
        if (solve_is_hint(s))
            return fail(ctx, TYPLONK_ERR_INVALID_ARG, "cells[" + std::to_string(i) + "] lies in a hinted class: its value is computed");
        if (!(s & SOLVE_FREE))
            return fail(ctx, TYPLONK_ERR_INVALID_ARG, "cells[" + std::to_string(i) + "] lies in a driven class: its value is computed");
        if (slot_arg[s & ~SOLVE_FREE] != SLOT_UNASSIGNED)
            return fail(ctx, TYPLONK_ERR_INVALID_ARG, "cells[" + std::to_string(i) + "] lies in the class of cells[" +
                                                          std::to_string(slot_arg[s & ~SOLVE_FREE]) + "]");
        slot_arg[s & ~SOLVE_FREE] = (uint32_t)i;
    }
    // witnesses per launch: the grid's second dimension, grouped as typlonk_witness_check groups them
    const size_t G = std::min<size_t>(count, 1024);
    // (the hint tables: count x n_hints values, written by the hints' levels and read by later levels and the fill)
    const size_t b_vals = count * n_cells * sizeof(Fr), b_hint = count * (size_t)sv.n_hints * sizeof(Fr), b_tab = G * sizeof(SvWitness),
                 b_slot = slot_arg.size() * sizeof(uint32_t);
    rc = ensure(ctx, ctx->wc_ws, b_vals + b_hint + b_tab + b_slot);
    if (rc) return rc;
    char* ws = (char*)ctx->wc_ws.p;
    Fr* d_vals = (Fr*)ws;
    Fr* d_htab = (Fr*)(ws + b_vals);
    SvWitness* d_tab = (SvWitness*)(ws + b_vals + b_hint);
    uint32_t* d_slot = (uint32_t*)(ws + b_vals + b_hint + b_tab);
    hipStream_t st = ctx->stream;
    if (b_vals) HIPCHK(hipMemcpyAsync(d_vals, values, b_vals, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_slot, slot_arg.data(), b_slot, hipMemcpyHostToDevice, st));
    SolveArgs a{};
    a.sel = e.sel_ev;
    a.qo_inv = sv.d_qo_inv;
    a.src = sv.d_src;
    a.order = sv.d_order;
    a.level_off = sv.d_level_off;
    a.slot_arg = d_slot;
    a.wit = d_tab;
    a.n = n;
    a.c256 = Fr::one();
    a.c284 = fr_from_u64(1u << 28);
    a.hints = (const SvHint*)sv.d_hints;
    a.n_hints = sv.n_hints;
    const bool hinted = sv.n_hints != 0;
    std::vector<SvWitness> tab;
    for (size_t first = 0; first < count; first += G) {
        const uint32_t g = (uint32_t)std::min(G, count - first);
        tab.assign(g, SvWitness{});
        for (uint32_t k = 0; k < g; ++k) {
            for (int i = 0; i < 3; ++i) tab[k].w[i] = wire_out[3 * (first + k) + i]->d;
            tab[k].pi_len = out.pi_rows(first + k, n);
            tab[k].pi = out.pi(first + k, n).dev;
            tab[k].vals = d_vals + (first + k) * n_cells;
        }
        // (the copy reads `tab` when it is queued: the source is pageable)
        HIPCHK(hipMemcpyAsync(d_tab, tab.data(), g * sizeof(SvWitness), hipMemcpyHostToDevice, st));
        a.htab = d_htab + first * sv.n_hints;
        for (const SolveLaunch& l : p.schedule) {
            if (l.wide) {
                const uint32_t off = p.level_off[l.first], rows = p.level_off[l.first + 1] - off;
                const dim3 grid((rows + SV_BLOCK - 1) / SV_BLOCK, g);
                if (hinted)
                    hipLaunchKernelGGL(solve_wide_kernel<true>, grid, dim3(SV_BLOCK), 0, st, a, off, rows);
                else
                    hipLaunchKernelGGL(solve_wide_kernel<false>, grid, dim3(SV_BLOCK), 0, st, a, off, rows);
            } else if (hinted) {
                hipLaunchKernelGGL(solve_run_kernel<true>, dim3(g), dim3(SV_BLOCK), 0, st, a, l.first, l.levels);
            } else {
                hipLaunchKernelGGL(solve_run_kernel<false>, dim3(g), dim3(SV_BLOCK), 0, st, a, l.first, l.levels);
            }
            HIPCHK(hipGetLastError());
        }
        const dim3 fill_grid((unsigned)((n + SV_BLOCK - 1) / SV_BLOCK), g);
        if (hinted)
            hipLaunchKernelGGL(solve_fill_kernel<true>, fill_grid, dim3(SV_BLOCK), 0, st, a);
        else
            hipLaunchKernelGGL(solve_fill_kernel<false>, fill_grid, dim3(SV_BLOCK), 0, st, a);
        HIPCHK(hipGetLastError());
        // the table is rewritten for the next group
        if (first + G < count) HIPCHK(hipStreamSynchronize(st));
    }
    HIPCHK(hipStreamSynchronize(st));
    return TYPLONK_OK;
}
