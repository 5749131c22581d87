// libtyplonk_hip.so -- typlonk_permutation_from_pairs, typlonk_circuit_compile_pairs: the copy-constraint permutation from what
// a front end holds, pairs of cells that must carry one value (PermutationBuilder::add_constrain / build,
// permutation/src/lib.rs:48-93), made on the device and handed to the compile without visiting the host.
// Part of the host driver of include/typlonk.h (see host.hpp for the shared state).
//
// The canonical permutation: the pairs generate an equivalence relation on the cells x = col * n + row; inside a class the
// cells are taken in ascending order x_0 < x_1 < ... < x_{k-1}, perm[x_i] = x_{i+1}, perm[x_{k-1}] = x_0.  It depends on the
// partition alone -- not on the pairs' order, orientation or multiplicity, and not on the run: the reference walks a HashMap
// (lib.rs:68) and gives one circuit a different sigma, and a different verifying key, every time.
//
//   1. validate   a thread per pair: both cells below 3n?  The count of bad pairs and the lowest (pair index, cell).
//   2. classes    parent[x] = x, then a thread per pair joins its two cells (perm_pairs.hpp: find with path halving, the
//                 larger root hooked under the smaller by compare-and-swap; relaxed agent-scope atomics, bounded loops,
//                 nobody waits).  ceil((log_n + 2) / 3) rounds of pointer jumping then leave label[x] = the lowest cell of
//                 x's class in parent[] itself.  The launch count depends on log_n only, never on the shape of a class.
//   3. cycles     a stable LSD radix sort of the cells by label, 8 bits a pass, ceil((log_n + 2) / 8) passes: per-workgroup
//                 digit counts, one exclusive scan over the (digit, workgroup) matrix, and a scatter that ranks a tile in
//                 order -- a wave takes 64 consecutive elements at a time, equal digits find each other with eight ballots,
//                 the lowest lane of a group draws the group's run from the wave's LDS cursor.  No cursor is global, so the
//                 order is the input order, run after run.  The cells start in ascending order, so they end ascending inside
//                 every label.  Then perm[order[i]] = order[i + 1] inside a run of equal labels; the last cell of a run
//                 links to the label, which is the run's first cell.  A run is a class: their count is `classes`.
//
// Device memory for the duration of a call, n = 2^log_n: 36 n bytes (labels and the sort's two cell arrays; one of the two
// receives perm when the caller wants it on the host) + 0.75 n + 8 KiB (digit counts) + 8 * count (the pairs), freed on return.
#include "host.hpp"
#include "host_checks.hpp"
#include "perm_pairs.hpp"

using namespace ty;
using namespace tyh;

namespace {

constexpr uint32_t PP_TILE = 4096;                 // cells per workgroup of a sort pass: four waves of 16 x 64
constexpr uint32_t PP_WAVE_STEPS = PP_TILE / 256;
constexpr uint32_t PP_SCAN_BLOCK = 2048;           // counters per workgroup of the scan: 256 threads x 8

struct PairFlags {
    unsigned long long bad;        // pairs that name a cell >= 3n
    unsigned long long first_bad;  // min over them of pair index << 32 | the offending cell
    unsigned long long classes;
    unsigned long long over;       // threads whose walk reached its bound
};

__global__ __launch_bounds__(256) void pp_validate_kernel(const uint32_t* pairs, uint64_t count, uint32_t n3, PairFlags* f) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t a = 0, b = 0;
    if (i < count) {
        a = pairs[2 * i];
        b = pairs[2 * i + 1];
    }
    const bool bad = a >= n3 || b >= n3;
    const uint32_t c = __popcll(__ballot(bad));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&f->bad, (unsigned long long)c);
    if (bad) atomicMin(&f->first_bad, (unsigned long long)i << 32 | (a >= n3 ? a : b));
}

__global__ __launch_bounds__(256) void pp_init_kernel(uint32_t* parent, uint32_t n3) {
    const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (x < n3) parent[x] = (uint32_t)x;
}

// (a pair with a cell outside the table is skipped here as well: this kernel never indexes past parent[3n - 1] on its own
// account, whatever the host did with the validation's answer)
__global__ __launch_bounds__(256) void pp_hook_kernel(const uint32_t* pairs, uint64_t count, uint32_t n3, uint32_t* parent,
                                                      PairFlags* f) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const uint32_t a = pairs[2 * i], b = pairs[2 * i + 1];
    if (a >= n3 || b >= n3) return;
    if (!pp_union(parent, a, b, 2 * n3)) atomicAdd(&f->over, 1ull);
}

__global__ __launch_bounds__(256) void pp_jump_kernel(uint32_t* parent, uint32_t n3) {
    const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (x < n3) pp_jump(parent, (uint32_t)x, PP_JUMP_HOPS);
}

// the digit of the tile's element at `pos` (src == null: the cells in ascending order, the first pass)
__device__ __forceinline__ bool pp_digit(const uint32_t* src, const uint32_t* label, uint64_t pos, uint32_t n3, uint32_t shift,
                                         uint32_t* cell, uint32_t* digit) {
    if (pos >= n3) return false;
    *cell = src ? src[pos] : (uint32_t)pos;
    *digit = (label[*cell] >> shift) & 255u;
    return true;
}

// hist[digit * nblocks + workgroup] = elements of the workgroup's tile with that digit
__global__ __launch_bounds__(256) void pp_hist_kernel(const uint32_t* src, const uint32_t* label, uint32_t n3, uint32_t shift,
                                                      uint32_t* hist) {
    __shared__ uint32_t cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * PP_TILE;
    for (uint32_t s = 0; s < PP_WAVE_STEPS; ++s) {
        uint32_t cell, digit;
        if (pp_digit(src, label, base + s * 256 + threadIdx.x, n3, shift, &cell, &digit)) atomicAdd(&cnt[digit], 1u);
    }
    __syncthreads();
    hist[(uint64_t)threadIdx.x * gridDim.x + blockIdx.x] = cnt[threadIdx.x];
}

// ---- exclusive scan of `len` counters in place: sums per 2048, one workgroup over the sums, finish ------------------------
__global__ __launch_bounds__(256) void pp_scan_sums_kernel(const uint32_t* v, uint32_t len, uint32_t* sums) {
    __shared__ uint32_t red[256];
    const uint64_t base = (uint64_t)blockIdx.x * PP_SCAN_BLOCK + threadIdx.x * 8;
    uint32_t s = 0;
    for (int e = 0; e < 8; ++e)
        if (base + e < len) s += v[base + e];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = red[0];
}
// inclusive Hillis-Steele scan of one value per thread; returns the thread's inclusive sum
__device__ __forceinline__ uint32_t pp_block_scan(uint32_t* buf, uint32_t v) {
    buf[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const uint32_t t = (int)threadIdx.x >= off ? buf[threadIdx.x - off] : 0;
        __syncthreads();
        buf[threadIdx.x] += t;
        __syncthreads();
    }
    return buf[threadIdx.x];
}
__global__ __launch_bounds__(256) void pp_scan_top_kernel(uint32_t* sums, uint32_t nsums) {
    __shared__ uint32_t buf[256];
    uint32_t running = 0;
    for (uint32_t base = 0; base < nsums; base += 256) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nsums ? sums[i] : 0;
        const uint32_t incl = pp_block_scan(buf, v);
        if (i < nsums) sums[i] = running + incl - v;
        running += buf[255];
        __syncthreads();   // the next round overwrites buf
    }
}
__global__ __launch_bounds__(256) void pp_scan_finish_kernel(uint32_t* v, uint32_t len, const uint32_t* sums) {
    __shared__ uint32_t buf[256];
    const uint64_t base = (uint64_t)blockIdx.x * PP_SCAN_BLOCK + threadIdx.x * 8;
    uint32_t c[8], s = 0;
    for (int e = 0; e < 8; ++e) {
        c[e] = base + e < len ? v[base + e] : 0;
        s += c[e];
    }
    uint32_t run = sums[blockIdx.x] + pp_block_scan(buf, s) - s;
    for (int e = 0; e < 8; ++e) {
        if (base + e < len) v[base + e] = run;
        run += c[e];
    }
}

// One stable pass.  offs: the scanned counts, so offs[digit * nblocks + workgroup] is where this tile's run of `digit` starts.
// Wave w owns elements [w * 1024, (w + 1) * 1024) of the tile and takes them 64 at a time, in order.
__global__ __launch_bounds__(256) void pp_scatter_kernel(const uint32_t* src, const uint32_t* label, uint32_t n3, uint32_t shift,
                                                         const uint32_t* offs, uint32_t* dst) {
    __shared__ uint32_t cur[4][256];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (uint32_t w = 0; w < 4; ++w) cur[w][threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * PP_TILE + (uint64_t)wave * (PP_TILE / 4) + lane;
    for (uint32_t s = 0; s < PP_WAVE_STEPS; ++s) {
        uint32_t cell, digit;
        if (pp_digit(src, label, base + s * 64, n3, shift, &cell, &digit)) atomicAdd(&cur[wave][digit], 1u);
    }
    __syncthreads();
    {
        // counts -> cursors: the tile's run of a digit, cut among the waves in order
        uint32_t run = offs[(uint64_t)threadIdx.x * gridDim.x + blockIdx.x];
        for (uint32_t w = 0; w < 4; ++w) {
            const uint32_t c = cur[w][threadIdx.x];
            cur[w][threadIdx.x] = run;
            run += c;
        }
    }
    __syncthreads();
    for (uint32_t s = 0; s < PP_WAVE_STEPS; ++s) {
        uint32_t cell = 0, digit = 0;
        const bool valid = pp_digit(src, label, base + s * 64, n3, shift, &cell, &digit);
        // the lanes of this step that hold the same digit
        unsigned long long m = __ballot(valid);
#pragma unroll
        for (uint32_t b = 0; b < 8; ++b) {
            const bool bit = (digit >> b) & 1u;
            const unsigned long long v = __ballot(bit);
            m &= bit ? v : ~v;
        }
        if (!valid) m = 1ull << lane;
        const uint32_t leader = (uint32_t)__ffsll((long long)m) - 1;
        uint32_t start = 0;
        if (valid && lane == leader) start = atomicAdd(&cur[wave][digit], (uint32_t)__popcll(m));
        start = __shfl(start, (int)leader);
        const uint32_t pos = start + (uint32_t)__popcll(m & ((1ull << lane) - 1));
        if (valid && pos < n3) dst[pos] = cell;
    }
}

// order: the cells sorted by (label, cell).  perm[c] = the next cell of c's run, or the run's first cell (its label).
__global__ __launch_bounds__(256) void pp_link_kernel(const uint32_t* order, const uint32_t* label, uint32_t n3, uint32_t* perm,
                                                      PairFlags* f) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool last = false;
    if (i < n3) {
        const uint32_t c = order[i], l = label[c];
        uint32_t next = l;
        last = true;
        if (i + 1 < n3) {
            const uint32_t d = order[i + 1];
            if (label[d] == l) {
                next = d;
                last = false;
            }
        }
        perm[c] = next;
    }
    const uint32_t k = __popcll(__ballot(last));
    if ((threadIdx.x & 63) == 0 && k) atomicAdd(&f->classes, (unsigned long long)k);
}

struct PairsArg {
    const uint32_t* pairs;
    size_t count;
    uint32_t log_n;
    uint64_t classes;
};

// The canonical permutation of `count` HOST pairs into d_perm (device, 3n; null: one of the sort's own arrays) and, where
// h_perm is given, on to the host.  Nothing is written to d_perm, h_perm or *classes unless every pair is inside the table.
int perm_from_pairs(typlonk_ctx* ctx, const uint32_t* pairs, size_t count, uint32_t log_n, uint32_t* d_perm, uint32_t* h_perm,
                    uint64_t* classes) {
    const uint32_t n3 = 3u << log_n;
    const uint32_t nblocks = (n3 + PP_TILE - 1) / PP_TILE, len = 256 * nblocks, nsums = (len + PP_SCAN_BLOCK - 1) / PP_SCAN_BLOCK;
    const uint32_t passes = (log_n + 2 + 7) / 8;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t words = (size_t)3 * n3 + len + nsums + 2 * count;
    char* ws = nullptr;
    HIPCHK(hipMalloc((void**)&ws, sizeof(PairFlags) + words * sizeof(uint32_t)));
    DevGuard guard;   // (never dismissed: the workspace goes when the call returns)
    guard.add(ws);
    PairFlags* d_flags = (PairFlags*)ws;
    uint32_t* parent = (uint32_t*)(ws + sizeof(PairFlags));
    uint32_t* ord[2] = {parent + n3, parent + 2 * (size_t)n3};
    uint32_t* hist = parent + 3 * (size_t)n3;
    uint32_t* sums = hist + len;
    uint32_t* d_pairs = sums + nsums;
    const PairFlags init{0, ~0ull, 0, 0};
    PairFlags res{};
    const dim3 cells((n3 + 255) / 256), blk(256);
    HIPCHK(hipMemcpyAsync(d_flags, &init, sizeof(init), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(pp_init_kernel, cells, blk, 0, s, parent, n3);
    HIPCHK(hipGetLastError());
    if (count) {
        const dim3 per_pair((unsigned)((count + 255) / 256));
        HIPCHK(hipMemcpyAsync(d_pairs, pairs, 2 * count * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(pp_validate_kernel, per_pair, blk, 0, s, (const uint32_t*)d_pairs, (uint64_t)count, n3, d_flags);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(pp_hook_kernel, per_pair, blk, 0, s, (const uint32_t*)d_pairs, (uint64_t)count, n3, parent, d_flags);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&res, d_flags, sizeof(res), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (res.bad)
            return fail(ctx, TYPLONK_ERR_INVALID_ARG,
                        std::to_string(res.bad) + " pairs name a cell that is not below 3n = " + std::to_string(n3) +
                            ", the lowest is pair " + std::to_string(res.first_bad >> 32) + " with cell " +
                            std::to_string((uint32_t)res.first_bad));
        if (res.over)
            return fail(ctx, TYPLONK_ERR_INTERNAL,
                        "union-find: " + std::to_string(res.over) + " pairs did not reach a root within 2 * 3n steps");
    }
    for (uint32_t r = 0; r < pp_jump_rounds(log_n); ++r) {
        hipLaunchKernelGGL(pp_jump_kernel, cells, blk, 0, s, parent, n3);
        HIPCHK(hipGetLastError());
    }
    const uint32_t* label = parent;
    const uint32_t* src = nullptr;
    for (uint32_t p = 0; p < passes; ++p) {
        uint32_t* dst = ord[p & 1];
        hipLaunchKernelGGL(pp_hist_kernel, dim3(nblocks), blk, 0, s, src, label, n3, 8 * p, hist);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(pp_scan_sums_kernel, dim3(nsums), blk, 0, s, (const uint32_t*)hist, len, sums);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(pp_scan_top_kernel, dim3(1), blk, 0, s, sums, nsums);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(pp_scan_finish_kernel, dim3(nsums), blk, 0, s, hist, len, (const uint32_t*)sums);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(pp_scatter_kernel, dim3(nblocks), blk, 0, s, src, label, n3, 8 * p, (const uint32_t*)hist, dst);
        HIPCHK(hipGetLastError());
        src = dst;
    }
    if (!d_perm) d_perm = ord[passes & 1];   // the array the last pass did not write
    hipLaunchKernelGGL(pp_link_kernel, cells, blk, 0, s, src, label, n3, d_perm, d_flags);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&res, d_flags, sizeof(res), hipMemcpyDeviceToHost, s));
    if (h_perm) HIPCHK(hipMemcpyAsync(h_perm, d_perm, (size_t)n3 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (classes) *classes = res.classes;
    return TYPLONK_OK;
}

// what every entry point refuses before a pair is read
int check_pairs_args(typlonk_ctx* ctx, const uint32_t* pairs, size_t count, uint32_t log_n) {
    if (log_n < 1 || log_n > TYPLONK_MAX_PROVER_LOG_N) return fail(ctx, TYPLONK_ERR_DOMAIN, "pairs need 1 <= log_n <= 24");
    if (!pairs && count) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null pairs with count != 0");
    if ((uint64_t)count > 0xFFFFFFFFull) return fail(ctx, TYPLONK_ERR_LENGTH, "more than 2^32 - 1 pairs");
    return TYPLONK_OK;
}

int fill_from_pairs(typlonk_ctx* ctx, uint32_t* d_perm, void* arg) {
    PairsArg* a = (PairsArg*)arg;
    return perm_from_pairs(ctx, a->pairs, a->count, a->log_n, d_perm, nullptr, &a->classes);
}

int compile_pairs_impl(typlonk_ctx* ctx, const ColumnsOf& in, const uint32_t* pairs, size_t count, const uint64_t cosets[3][4],
                       uint32_t log_n, uint32_t* circuit_id, uint64_t* classes) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    int rc = check_pairs_args(ctx, pairs, count, log_n);
    if (rc) return rc;
    PairsArg arg{pairs, count, log_n, 3ull << log_n};
    PermSource from{};
    if (count) {   // (no pairs: the identity, which the compile writes by itself)
        from.fill = fill_from_pairs;
        from.arg = &arg;
    }
    rc = circuit_compile_from(ctx, in, from, cosets, log_n, circuit_id, nullptr);
    if (rc) return rc;
    if (classes) *classes = arg.classes;
    return TYPLONK_OK;
}

}  // namespace

int typlonk_permutation_from_pairs(typlonk_ctx* ctx, const uint32_t* pairs, size_t count, uint32_t log_n, uint32_t* perm,
                                   uint64_t* classes) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    const int rc = check_pairs_args(ctx, pairs, count, log_n);
    if (rc) return rc;
    return perm_from_pairs(ctx, pairs, count, log_n, nullptr, perm, classes);
}

int typlonk_circuit_compile_pairs(typlonk_ctx* ctx, const typlonk_buf* const selector_evals[5], const uint32_t* pairs,
                                  size_t count, const uint64_t cosets[3][4], uint32_t log_n, uint32_t* circuit_id,
                                  uint64_t* classes) {
    return compile_pairs_impl(ctx, ColumnsOf(selector_evals, 1).selectors(), pairs, count, cosets, log_n, circuit_id, classes);
}

int typlonk_circuit_compile_pairs_host(typlonk_ctx* ctx, const uint64_t* const selector_evals[5], size_t rows,
                                       const uint32_t* pairs, size_t count, const uint64_t cosets[3][4], uint32_t log_n,
                                       uint32_t* circuit_id, uint64_t* classes) {
    return compile_pairs_impl(ctx, ColumnsOf(selector_evals, 1).selectors().with_rows(rows), pairs, count, cosets, log_n, circuit_id, classes);
}
