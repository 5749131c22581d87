// libtyplonk_hip.so -- typlonk_circuit_permutation, typlonk_witness_check: does a witness satisfy a loaded circuit, and if
// not, which gate rows and which copy constraints fail?  Exact (no challenge, no SRS, no collective), one pass over the columns.
// Part of the host driver of include/typlonk.h (see host.hpp for the shared state).
//
//   1. permutation recovery   typlonk_circuit_load only ever sees sigma as field values k_i w^j (permutation/src/lib.rs:101-128);
//                             the index map x -> y is a discrete logarithm in the order-2^log_n subgroup.  One thread per cell:
//                             u = v / k_i, u^n = 1 picks the coset, Pohlig-Hellman over the 2-group gives the row bit by bit
//                             (about log_n^2 / 2 + 4 log_n products per cell).  Once per (circuit, cosets), cached.
//   2. selector evaluations   a forward transform of CircuitEntry::coef[0..5), cached.
//   3. the check              one thread per row, the witness in blockIdx.y: the gate equation of proof.rs:317-320 and the three
//                             comparisons w[x] == w[perm[x]].  Flags -> wave ballots -> block counts -> one exclusive scan over
//                             the blocks -> the first `cap` failures written in ascending order.
//
// Arithmetic is fr30.hpp's (a * b / 2^270 mod r on 9 x 30-bit limbs): its operands may be ANY value below 2^256, so a cell that
// holds v + r is read as v, and every comparison is one of residues.  Data stay in arkworks' form x * 2^256; the constants
// below move between the two Montgomery radices:
//   recovery   u = fr30_mul(v, k^-1 * 2^284) = (v / k) * 2^270: the 2^270 domain, closed under fr30_mul; one there is 2^270 mod r
//   gate       fr30_mul(q, a) = q a * 2^242 for two data words, so every term is brought to the factor 2^242:
//              q_m a b = fr30_mul(fr30_mul(fr30_mul(a, b), 2^284), q_m),   q_c + PI -> fr30_mul(q_c + PI, 2^256)
//
// typlonk_circuit_compile is the way forward, for a front end that holds the permutation itself: sigma_from_perm_kernel writes
// sigma = k_col(perm[x]) * w^row(perm[x]) (sigma_cell.hpp, two products per cell), the indegree and defects kernels of step 1 lint
// the permutation, one batched inverse transform interpolates the eight columns, and the circuit keeps the permutation it was
// compiled from: step 1 never runs for it under the cosets it was compiled with.  typlonk_circuit_compile_pairs (perm_pairs.hip)
// enters the same code with a producer that writes the kept copy on the device, where the caller's array would be uploaded.
#include "host.hpp"
#include "host_checks.hpp"
#include "fr30.hpp"
#include "scan_ops.hpp"
#include "sigma_cell.hpp"

using namespace ty;
using namespace tyh;

namespace {

constexpr uint32_t CELL_NONE = TYPLONK_CELL_NONE;
constexpr uint32_t WC_BLOCK = 256;                  // rows per workgroup of the check: four waves, four mask words
constexpr uint32_t WC_WAVES = WC_BLOCK / 64;

struct PermArgs {
    const Fr* sig;      // 3n sigma evaluations (CircuitEntry::sig_ev)
    uint32_t* perm;     // 3n
    uint64_t n3;
    uint32_t log_n;
    Fr30 kinv[3];       // k_i^-1 * 2^284
    Fr30 wneg[TYPLONK_MAX_PROVER_LOG_N];   // w^(-2^b) * 2^270
};

// a witness of a batch as the check kernel reads it
struct WcWitness {
    const Fr* w[3];
    const Fr* pi;       // may be null when pi_len = 0
    uint64_t pi_len;
};

struct CheckArgs {
    const Fr* sel;          // 5n selector evaluations
    const uint32_t* perm;   // 3n
    const WcWitness* wit;
    uint64_t n;
    uint32_t log_n, nblocks, words;
    uint64_t* masks;        // [witness][4][words]: failure bits of the gate rows and of the cells of column 0, 1, 2
    uint32_t* bcnt;         // [witness][4 * nblocks]: failures per workgroup, the gate blocks, then the cells' in ascending order
    Fr30 c256, c284;        // 2^256 mod r, 2^284 mod r
};

struct ListArgs {
    const uint64_t* masks;
    const uint32_t* bcnt;   // after the scan: exclusive offsets
    const uint32_t* perm;
    uint64_t n;
    uint32_t nblocks, words, cap_gate, cap_copy;
    uint32_t* gate_rows;    // [witness][cap_gate]
    uint32_t* copy_cells;   // [witness][cap_copy][2]
};

__device__ __forceinline__ bool fr30_is(const Fr30& x, const Fr& canonical) { return fr30_to_canonical(x) == canonical; }
// lazy value (fr30_reduce_lazy's contract) == 0 mod r
__device__ __forceinline__ bool fr30_is_zero_mod_r(const Fr30& x) { return fr30_to_canonical(fr30_reduce_lazy(x)).is_zero(); }

__global__ __launch_bounds__(256) void perm_recover_kernel(PermArgs a) {
    const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= a.n3) return;
    const Fr one = fr30_pack(fr30_const_one());
    const Fr30 v = fr30_unpack(p_ld(a.sig + x));
    uint32_t out = CELL_NONE;
    for (uint32_t i = 0; i < 3 && out == CELL_NONE; ++i) {
        const Fr30 u = fr30_mul(v, a.kinv[i]);
        Fr30 t = u;
        for (uint32_t s = 0; s < a.log_n; ++s) t = fr30_mul(t, t);
        if (!fr30_is(t, one)) continue;                       // v is not in k_i H
        // u = w^row: bit b of the row is set iff (u w^-(bits below b))^(2^(log_n - 1 - b)) != 1
        Fr30 h = u;
        uint32_t row = 0;
        for (uint32_t b = 0; b < a.log_n; ++b) {
            t = h;
            for (uint32_t s = b + 1; s < a.log_n; ++s) t = fr30_mul(t, t);
            if (!fr30_is(t, one)) {
                row |= 1u << b;
                h = fr30_mul(h, a.wneg[b]);
            }
        }
        out = (i << a.log_n) + row;
    }
    a.perm[x] = out;
}

__global__ __launch_bounds__(256) void perm_indegree_kernel(const uint32_t* perm, uint32_t* indeg, uint64_t n3) {
    const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= n3) return;
    const uint32_t y = perm[x];
    if (y != CELL_NONE) atomicAdd(indeg + y, 1u);             // y < 3n by construction
}
// out[0] += cells without an image + cells that are the image of != 1 cells; out[1] = the lowest such cell
__global__ __launch_bounds__(256) void perm_defects_kernel(const uint32_t* perm, const uint32_t* indeg, uint64_t n3,
                                                           unsigned long long* out) {
    const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool none = x < n3 && perm[x] == CELL_NONE, deg = x < n3 && indeg[x] != 1u;
    const uint32_t c = __popcll(__ballot(none)) + __popcll(__ballot(deg));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, (unsigned long long)c);
    if (none || deg) atomicMin(out + 1, (unsigned long long)x);
}

// The forward direction of perm_recover_kernel.  One thread per cell x, cells in memory order: perm[x] is read (null: the
// identity), sig[x] = k_col(y) * w^row(y) written, and the kept copy perm[x] set to TYPLONK_CELL_NONE where y is no cell (sig[x]
// is then zero; such a permutation is refused before anything reads it).
__global__ __launch_bounds__(256) void sigma_from_perm_kernel(SigmaTables t, const uint32_t* perm_in, uint32_t* perm, Fr* sig,
                                                              uint64_t n3) {
    const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= n3) return;
    const uint32_t y = perm_in ? perm_in[x] : (uint32_t)x;
    Fr v = Fr::zero();
    const bool cell = sigma_cell(t, y, &v);
    perm[x] = cell ? y : CELL_NONE;
    p_st(sig + x, v);
}

__global__ __launch_bounds__(WC_BLOCK) void witness_flags_kernel(CheckArgs a) {
    __shared__ uint32_t cnt[4][WC_WAVES];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, k = blockIdx.y;
    const uint64_t j = (uint64_t)blockIdx.x * WC_BLOCK + threadIdx.x, n = a.n;
    bool f[4] = {false, false, false, false};
    if (j < n) {
        const WcWitness wt = a.wit[k];
        const Fr30 w0 = fr30_unpack(p_ld(wt.w[0] + j)), w1 = fr30_unpack(p_ld(wt.w[1] + j)), w2 = fr30_unpack(p_ld(wt.w[2] + j));
        // q_l a + q_r b - q_o c + q_m a b + q_c + PI (proof.rs:317-320), every term with the factor 2^242
        Fr30 pos = fr30_mul(fr30_unpack(p_ld(a.sel + j)), w0);
        pos = fr30_add(pos, fr30_mul(fr30_unpack(p_ld(a.sel + n + j)), w1));
        const Fr30 ab = fr30_mul(fr30_mul(w0, w1), a.c284);
        pos = fr30_add(pos, fr30_mul(ab, fr30_unpack(p_ld(a.sel + 3 * n + j))));
        Fr30 cst = fr30_unpack(p_ld(a.sel + 4 * n + j));
        if (j < wt.pi_len) cst = fr30_add(cst, fr30_unpack(p_ld(wt.pi + j)));
        pos = fr30_add(pos, fr30_mul(cst, a.c256));
        const Fr30 neg = fr30_mul(fr30_unpack(p_ld(a.sel + 2 * n + j)), w2);
        f[0] = !fr30_is_zero_mod_r(fr30_sub(pos, neg));
        // the copy constraints of the row's three cells
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const uint32_t y = a.perm[(uint64_t)i * n + j], col = y >> a.log_n;
            const Fr* src = col == 0 ? wt.w[0] : (col == 1 ? wt.w[1] : wt.w[2]);
            const Fr30 other = fr30_unpack(p_ld(src + (y & (n - 1))));
            f[1 + i] = !fr30_is_zero_mod_r(fr30_sub(i == 0 ? w0 : (i == 1 ? w1 : w2), other));
        }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const unsigned long long m = __ballot(f[s]);
        if (lane == 0) {
            cnt[s][wave] = __popcll(m);
            if ((j >> 6) < a.words) a.masks[((uint64_t)k * 4 + s) * a.words + (j >> 6)] = m;
        }
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        uint32_t c = 0;
#pragma unroll
        for (uint32_t w = 0; w < WC_WAVES; ++w) c += cnt[threadIdx.x][w];
        a.bcnt[((uint64_t)k * 4 + threadIdx.x) * a.nblocks + blockIdx.x] = c;
    }
}

// blockIdx.x = 0: the gate blocks, 1: the 3 * nblocks cell blocks; blockIdx.y = witness.  Exclusive scan in place, the total to
// totals[2 * witness + kind].  One workgroup: a thread sums a contiguous piece, the 256 sums are scanned in the LDS.
__global__ __launch_bounds__(256) void witness_scan_kernel(uint32_t* bcnt, uint32_t nblocks, uint64_t* totals) {
    __shared__ uint32_t part[256];
    const uint32_t kind = blockIdx.x, k = blockIdx.y, t = threadIdx.x;
    uint32_t* v = bcnt + (uint64_t)k * 4 * nblocks + (kind ? nblocks : 0);
    const uint32_t len = kind ? 3 * nblocks : nblocks, per = (len + 255) / 256;
    const uint32_t lo = min(t * per, len), hi = min(lo + per, len);
    uint32_t s = 0;
    for (uint32_t i = lo; i < hi; ++i) s += v[i];
    part[t] = s;
    __syncthreads();
    for (uint32_t off = 1; off < 256; off <<= 1) {
        const uint32_t add = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    uint32_t run = part[t] - s;
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t c = v[i];
        v[i] = run;
        run += c;
    }
    if (t == 255) totals[2 * k + kind] = part[255];
}

// a thread per mask word: its failures have ranks [block offset + bits of the block's earlier words, ...) in the witness's list
__global__ __launch_bounds__(256) void witness_list_kernel(ListArgs a) {
    const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= 4ull * a.words) return;
    const uint32_t k = blockIdx.y, s = (uint32_t)(idx / a.words), wd = (uint32_t)(idx % a.words);
    const uint64_t* masks = a.masks + ((uint64_t)k * 4 + s) * a.words;
    unsigned long long m = masks[wd];
    if (!m) return;
    const uint32_t blk = wd / WC_WAVES, cap = s ? a.cap_copy : a.cap_gate;
    uint32_t rank = a.bcnt[((uint64_t)k * 4 + s) * a.nblocks + blk];
    for (uint32_t w = blk * WC_WAVES; w < wd; ++w) rank += __popcll(masks[w]);
    for (; m && rank < cap; ++rank) {
        const uint32_t row = wd * 64 + (uint32_t)__ffsll((long long)m) - 1;
        m &= m - 1;
        if (s == 0) {
            a.gate_rows[(uint64_t)k * a.cap_gate + rank] = row;
        } else {
            const uint64_t x = (uint64_t)(s - 1) * a.n + row;
            uint32_t* o = a.copy_cells + ((uint64_t)k * a.cap_copy + rank) * 2;
            o[0] = (uint32_t)x;
            o[1] = a.perm[x];
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// words of a canonical residue -> 9 exact limbs (fr30_unpack on the host)
Fr30 to_limbs30(const Fr& x) {
    Fr30 r;
    for (int i = 0; i < 9; ++i) {
        const int bit = 30 * i, wi = bit >> 5, sh = bit & 31;
        uint64_t t = x.v[wi];
        if (wi + 1 < 8) t |= (uint64_t)x.v[wi + 1] << 32;
        r.v[i] = (uint32_t)(t >> sh) & FR30_MASK;
    }
    return r;
}

void free_check_cache(CircuitEntry& e) {
    (void)hipFree(e.perm);
    (void)hipFree(e.sel_ev);
    e.perm = nullptr;
    e.sel_ev = nullptr;
}

// Is the 3n-entry map `perm` (device; TYPLONK_CELL_NONE or a cell below 3n in every entry) a bijection of the cells?  ws: 3n
// uint32 of indegrees and 16 bytes behind them.  *defects = cells without an image + cells that are the image of != 1 cells,
// *first_bad = the lowest such cell (TYPLONK_CELL_NONE when there is none).  Blocks for the answer.
int perm_lint(typlonk_ctx* ctx, const uint32_t* perm, uint32_t* ws, uint64_t n3, uint64_t* defects, uint32_t* first_bad) {
    uint32_t* indeg = ws;
    unsigned long long* d_out = (unsigned long long*)(indeg + n3);
    const unsigned long long init[2] = {0, ~0ull};
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemsetAsync(indeg, 0, n3 * sizeof(uint32_t), s));
    HIPCHK(hipMemcpyAsync(d_out, init, sizeof(init), hipMemcpyHostToDevice, s));
    const dim3 grid((unsigned)((n3 + 255) / 256));
    hipLaunchKernelGGL(perm_indegree_kernel, grid, dim3(256), 0, s, perm, indeg, n3);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(perm_defects_kernel, grid, dim3(256), 0, s, perm, (const uint32_t*)indeg, n3, d_out);
    HIPCHK(hipGetLastError());
    unsigned long long res[2];
    HIPCHK(hipMemcpyAsync(res, d_out, sizeof(res), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *defects = res[0];
    *first_bad = res[0] ? (uint32_t)res[1] : CELL_NONE;
    return TYPLONK_OK;
}

// CircuitEntry::perm for these cosets: recovered on first use and again when the cosets change
int ensure_perm(typlonk_ctx* ctx, CircuitEntry& e, const uint64_t cosets[3][4]) {
    if (e.perm && e.perm_ready && memcmp(e.perm_cosets, cosets, sizeof(e.perm_cosets)) == 0) return TYPLONK_OK;
    const uint32_t log_n = e.log_n;
    const uint64_t n3 = 3ull << log_n;
    PermArgs a{};
    for (int i = 0; i < 3; ++i) {
        Fr k;
        memcpy(k.v, cosets[i], sizeof(k.v));
        if (!fr_canonical(cosets[i])) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "coset is not a canonical residue");
        a.kinv[i] = to_limbs30(fe_mul(fe_inv(k), fr_from_u64(1u << 28)));
    }
    const Fr c14 = fr_from_u64(1u << 14);
    Fr w = fr_domain_root_inv(log_n);
    for (uint32_t b = 0; b < log_n; ++b) {
        a.wneg[b] = to_limbs30(fe_mul(w, c14));
        w = fe_sqr(w);
    }
    e.perm_ready = false;
    if (!e.perm) HIPCHK(hipMalloc((void**)&e.perm, n3 * sizeof(uint32_t)));
    const int rc = ensure(ctx, ctx->wc_ws, n3 * sizeof(uint32_t) + 16);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    a.sig = e.sig_ev;
    a.perm = e.perm;
    a.n3 = n3;
    a.log_n = log_n;
    const dim3 grid((unsigned)((n3 + 255) / 256));
    hipLaunchKernelGGL(perm_recover_kernel, grid, dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
    const int lrc = perm_lint(ctx, e.perm, (uint32_t*)ctx->wc_ws.p, n3, &e.perm_defects, &e.perm_first_bad);
    if (lrc) return lrc;
    memcpy(e.perm_cosets, cosets, sizeof(e.perm_cosets));
    e.perm_ready = true;
    return TYPLONK_OK;
}

// CircuitEntry::sel_ev: q_l q_r q_o q_m q_c over the domain (builder.rs:84-88 interpolates them; this is the way back)
int ensure_selectors(typlonk_ctx* ctx, CircuitEntry& e) {
    if (e.sel_ev) return TYPLONK_OK;
    const uint64_t n = 1ull << e.log_n;
    Fr* ev = nullptr;
    HIPCHK(hipMalloc((void**)&ev, 5 * n * sizeof(Fr)));
    DevGuard guard;
    guard.add(ev);
    HIPCHK(hipMemcpyAsync(ev, e.coef, 5 * n * sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
    Fr* dst[5];
    for (int k = 0; k < 5; ++k) dst[k] = ev + (uint64_t)k * n;
    const int rc = ntt_run_batch(ctx, dst, 5, e.log_n, 0, nullptr, /*sync=*/false);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    guard.dismiss();
    e.sel_ev = ev;
    return TYPLONK_OK;
}

struct Outputs {
    uint32_t cap;
    typlonk_witness_report* reports;
    uint32_t* gate_rows;
    uint32_t* copy_cells;
};

// `g` witnesses whose device table entries are tab[0..g): flags, scan, lists, and the reports of witnesses first.. on the host
int check_chunk(typlonk_ctx* ctx, const CircuitEntry& e, const std::vector<WcWitness>& tab, size_t first, const Outputs& o) {
    const uint32_t log_n = e.log_n, g = (uint32_t)tab.size();
    const uint64_t n = 1ull << log_n;
    const uint32_t nblocks = (uint32_t)((n + WC_BLOCK - 1) / WC_BLOCK), words = (uint32_t)((n + 63) / 64);
    const uint32_t cap_gate = (uint32_t)std::min<uint64_t>(o.cap, n), cap_copy = (uint32_t)std::min<uint64_t>(o.cap, 3 * n);
    // workspace: masks | totals | table | block counts | gate list | copy list  (8-byte aligned parts first)
    const size_t b_masks = (size_t)g * 4 * words * 8, b_tot = (size_t)g * 2 * 8, b_tab = (size_t)g * sizeof(WcWitness);
    const size_t b_cnt = (size_t)g * 4 * nblocks * 4, b_gate = (size_t)g * cap_gate * 4, b_copy = (size_t)g * cap_copy * 8;
    const int rc = ensure(ctx, ctx->wc_ws, b_masks + b_tot + b_tab + b_cnt + b_gate + b_copy);
    if (rc) return rc;
    char* p = (char*)ctx->wc_ws.p;
    uint64_t* d_masks = (uint64_t*)p;
    uint64_t* d_tot = (uint64_t*)(p + b_masks);
    WcWitness* d_tab = (WcWitness*)(p + b_masks + b_tot);
    uint32_t* d_cnt = (uint32_t*)(p + b_masks + b_tot + b_tab);
    uint32_t* d_gate = d_cnt + (size_t)g * 4 * nblocks;
    uint32_t* d_copy = d_gate + (size_t)g * cap_gate;
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(d_tab, tab.data(), b_tab, hipMemcpyHostToDevice, s));
    CheckArgs a{};
    a.sel = e.sel_ev;
    a.perm = e.perm;
    a.wit = d_tab;
    a.n = n;
    a.log_n = log_n;
    a.nblocks = nblocks;
    a.words = words;
    a.masks = d_masks;
    a.bcnt = d_cnt;
    a.c256 = to_limbs30(Fr::one());
    a.c284 = to_limbs30(fr_from_u64(1u << 28));
    hipLaunchKernelGGL(witness_flags_kernel, dim3(nblocks, g), dim3(WC_BLOCK), 0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(witness_scan_kernel, dim3(2, g), dim3(256), 0, s, d_cnt, nblocks, d_tot);
    HIPCHK(hipGetLastError());
    std::vector<uint64_t> tot((size_t)g * 2);
    std::vector<uint32_t> gate, copy;
    if (o.cap) {
        ListArgs l{};
        l.masks = d_masks;
        l.bcnt = d_cnt;
        l.perm = e.perm;
        l.n = n;
        l.nblocks = nblocks;
        l.words = words;
        l.cap_gate = cap_gate;
        l.cap_copy = cap_copy;
        l.gate_rows = d_gate;
        l.copy_cells = d_copy;
        hipLaunchKernelGGL(witness_list_kernel, dim3((unsigned)((4ull * words + 255) / 256), g), dim3(256), 0, s, l);
        HIPCHK(hipGetLastError());
        gate.resize((size_t)g * cap_gate);
        copy.resize((size_t)g * cap_copy * 2);
        HIPCHK(hipMemcpyAsync(gate.data(), d_gate, b_gate, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(copy.data(), d_copy, b_copy, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipMemcpyAsync(tot.data(), d_tot, b_tot, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (uint32_t k = 0; k < g; ++k) {
        typlonk_witness_report& r = o.reports[first + k];
        r.gate_failures = tot[2 * k];
        r.copy_failures = tot[2 * k + 1];
        r.gate_listed = (uint32_t)std::min<uint64_t>(r.gate_failures, cap_gate);
        r.copy_listed = (uint32_t)std::min<uint64_t>(r.copy_failures, cap_copy);
        if (r.gate_listed) memcpy(o.gate_rows + (first + k) * (size_t)o.cap, gate.data() + (size_t)k * cap_gate, (size_t)r.gate_listed * 4);
        if (r.copy_listed)
            memcpy(o.copy_cells + (first + k) * (size_t)o.cap * 2, copy.data() + (size_t)k * cap_copy * 2, (size_t)r.copy_listed * 8);
    }
    return TYPLONK_OK;
}

int witness_check_impl(typlonk_ctx* ctx, uint32_t circuit_id, const ColumnsOf& in, const uint64_t cosets[3][4], const Outputs& o) {
    const size_t count = in.count;
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    if (count == 0) return TYPLONK_OK;
    if (!cosets || !o.reports || !in.given() || (o.cap && (!o.gate_rows || !o.copy_cells)))
        return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    auto ci = ctx->circuits.find(circuit_id);
    if (ci == ctx->circuits.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown circuit id");
    CircuitEntry& e = ci->second;
    const uint64_t n = 1ull << e.log_n;
    int rc = admit_columns(ctx, in, n);
    if (!rc) rc = admit_rows(ctx, in, n);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    ProfilingOff prof_off(ctx);
    rc = circuit_check_prepare(ctx, e, cosets);
    if (rc) return rc;
    // witnesses per launch: bounded by the workspace (masks, counts, lists) and, for the host form, by the staged columns
    const uint32_t cap_copy = (uint32_t)std::min<uint64_t>(o.cap, 3 * n);
    const uint64_t per = n / 2 + n / 16 + 64 + 12ull * cap_copy + (in.on_device() ? 0 : 4 * n * sizeof(Fr));
    const size_t G = (size_t)std::min<uint64_t>({(uint64_t)count, 1024, std::max<uint64_t>(1, ((uint64_t)512 << 20) / per)});
    std::vector<WcWitness> tab;
    for (size_t first = 0; first < count; first += G) {
        const size_t g = std::min(G, count - first);
        tab.assign(g, WcWitness{});
        Fr* d = nullptr;
        if (!in.on_device()) {
            // the chunk is staged: three columns per witness, then its public values (only the rows that are read)
            size_t elems = 0;
            for (size_t k = 0; k < g; ++k) elems += 3 * n + in.pi_rows(first + k, n);
            rc = ensure(ctx, ctx->wc_stage, elems * sizeof(Fr));
            if (rc) return rc;
            d = (Fr*)ctx->wc_stage.p;
        }
        // a column where the kernels read it: in its buffer, or copied into the next `rows` elements of the stage
        auto place = [&](const ColumnSrc& c, const Fr** at) -> hipError_t {
            *at = c.dev;
            if (!c.host) return hipSuccess;   // in its buffer already, or absent
            *at = d;
            d += c.rows;
            return column_to_device(d - c.rows, c, c.rows, ctx->stream);
        };
        for (size_t k = 0; k < g; ++k) {
            for (int i = 0; i < 3; ++i) HIPCHK(place(in.column(first + k, i, n), &tab[k].w[i]));
            tab[k].pi_len = in.pi_rows(first + k, n);
            HIPCHK(place(in.pi(first + k, n), &tab[k].pi));
        }
        rc = check_chunk(ctx, e, tab, first, o);
        if (rc) return rc;
    }
    return TYPLONK_OK;
}

// ---- typlonk_circuit_compile ---------------------------------------------------------------------------------------------
// k_0 H, k_1 H, k_2 H are cosets of the domain H, pairwise disjoint: canonical, non-zero, (k_i / k_j)^n != 1
int check_cosets(typlonk_ctx* ctx, const uint64_t cosets[3][4], uint32_t log_n, Fr (&k)[3]) {
    for (int i = 0; i < 3; ++i) {
        if (!fr_canonical(cosets[i])) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "coset is not a canonical residue");
        memcpy(k[i].v, cosets[i], sizeof(k[i].v));
        if (k[i].is_zero()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "coset is zero");
    }
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j) {
            Fr t = fe_mul(k[i], fe_inv(k[j]));
            for (uint32_t s = 0; s < log_n; ++s) t = fe_sqr(t);
            if (t == Fr::one())
                return fail(ctx, TYPLONK_ERR_INVALID_ARG,
                            "cosets " + std::to_string(i) + " and " + std::to_string(j) + " are not disjoint: (k_i / k_j)^n = 1");
        }
    return TYPLONK_OK;
}

int circuit_compile_impl(typlonk_ctx* ctx, const ColumnsOf& in, const PermSource& from, const uint64_t cosets[3][4], uint32_t log_n,
                         uint32_t* circuit_id, uint64_t* defects) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    if (!in.given() || !cosets || !circuit_id) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    if (log_n < 1 || log_n > TYPLONK_MAX_PROVER_LOG_N) return fail(ctx, TYPLONK_ERR_DOMAIN, "quotient needs 1 <= log_n <= 24");
    const uint64_t n = 1ull << log_n, n3 = 3 * n;
    int rc = admit_columns(ctx, in, n);
    if (!rc) rc = admit_rows(ctx, in, n);
    if (rc) return rc;
    SigmaTables t{};
    rc = check_cosets(ctx, cosets, log_n, t.k);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    ProfilingOff prof_off(ctx);
    rc = domain_twiddles(ctx, log_n, &t.lo, &t.hi, &t.h);
    if (rc) return rc;
    t.log_n = log_n;

    CircuitEntry e;
    e.log_n = log_n;
    DevGuard guard;
    HIPCHK(hipMalloc((void**)&e.ext, 36 * n * sizeof(Fr)));
    guard.add(e.ext);
    HIPCHK(hipMalloc((void**)&e.coef, 8 * n * sizeof(Fr)));
    guard.add(e.coef);
    HIPCHK(hipMalloc((void**)&e.sig_ev, n3 * sizeof(Fr)));
    guard.add(e.sig_ev);
    HIPCHK(hipMalloc((void**)&e.perm, n3 * sizeof(uint32_t)));
    guard.add(e.perm);
    hipStream_t s = ctx->stream;
    {
        // the lint's indegrees live for this block only
        uint32_t* indeg = nullptr;
        HIPCHK(hipMalloc((void**)&indeg, n3 * sizeof(uint32_t) + 16));
        DevGuard transient;
        transient.add(indeg);
        // the permutation goes into the kept copy, from the caller's array or from a producer on the device; the kernel reads
        // it there and rewrites an entry that is no cell
        const bool given = from.host || from.fill;
        if (from.host) HIPCHK(hipMemcpyAsync(e.perm, from.host, n3 * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        if (from.fill) {
            rc = from.fill(ctx, e.perm, from.arg);
            if (rc) return rc;
        }
        hipLaunchKernelGGL(sigma_from_perm_kernel, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, s, t,
                           given ? (const uint32_t*)e.perm : (const uint32_t*)nullptr, e.perm, e.sig_ev, n3);
        HIPCHK(hipGetLastError());
        rc = perm_lint(ctx, e.perm, indeg, n3, &e.perm_defects, &e.perm_first_bad);
        if (rc) return rc;
    }
    if (defects) *defects = e.perm_defects;
    if (e.perm_defects)
        return fail(ctx, TYPLONK_ERR_INVALID_ARG,
                    "perm is not a permutation of the cells (" + std::to_string(e.perm_defects) + " defects, the lowest at cell " +
                        std::to_string(e.perm_first_bad) + ")");
    // the eight columns as evaluations in `coef`, interpolated there in one batch (builder.rs:84-88, proof.rs:334-338)
    for (int k = 0; k < 5; ++k) HIPCHK(column_to_device(e.coef + (uint64_t)k * n, in.column(0, k, n), n, s));
    HIPCHK(hipMemcpyAsync(e.coef + 5 * n, e.sig_ev, n3 * sizeof(Fr), hipMemcpyDeviceToDevice, s));
    Fr* co[8];
    for (int k = 0; k < 8; ++k) co[k] = e.coef + (uint64_t)k * n;
    rc = ntt_run_batch(ctx, co, 8, log_n, 1, nullptr, /*sync=*/false);
    if (rc) return rc;
    memcpy(e.perm_cosets, cosets, sizeof(e.perm_cosets));
    e.perm_ready = true;
    rc = circuit_finish(ctx, e, co, /*sigma_forward=*/false, circuit_id);
    if (rc) return rc;
    guard.dismiss();
    return TYPLONK_OK;
}

}  // namespace

namespace tyh {
void circuit_check_release(CircuitEntry& e) {
    free_check_cache(e);
    circuit_solve_release(e);
}
int circuit_check_prepare(typlonk_ctx* ctx, CircuitEntry& e, const uint64_t cosets[3][4]) {
    const int rc = ensure_perm(ctx, e, cosets);
    if (rc) return rc;
    if (e.perm_defects)
        return fail(ctx, TYPLONK_ERR_INVALID_ARG,
                    "malformed circuit: sigma is not a permutation of the cells (" + std::to_string(e.perm_defects) +
                        " defects, the lowest at cell " + std::to_string(e.perm_first_bad) + "; see typlonk_circuit_permutation)");
    return ensure_selectors(ctx, e);
}
int circuit_compile_from(typlonk_ctx* ctx, const ColumnsOf& in, const PermSource& from, const uint64_t cosets[3][4], uint32_t log_n,
                         uint32_t* circuit_id, uint64_t* defects) {
    return circuit_compile_impl(ctx, in, from, cosets, log_n, circuit_id, defects);
}
}  // namespace tyh

int typlonk_circuit_permutation(typlonk_ctx* ctx, uint32_t circuit_id, const uint64_t cosets[3][4], uint32_t* perm,
                                uint64_t* defects) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    if (!cosets || !defects) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    auto ci = ctx->circuits.find(circuit_id);
    if (ci == ctx->circuits.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown circuit id");
    HIPCHK(hipSetDevice(ctx->device));
    ProfilingOff prof_off(ctx);
    CircuitEntry& e = ci->second;
    const int rc = ensure_perm(ctx, e, cosets);
    if (rc) return rc;
    if (perm) {
        HIPCHK(hipMemcpyAsync(perm, e.perm, (3ull << e.log_n) * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    *defects = e.perm_defects;
    return TYPLONK_OK;
}

int typlonk_witness_check(typlonk_ctx* ctx, uint32_t circuit_id, const typlonk_buf* const* wire_evals,
                          const typlonk_buf* const* pi, const size_t* pi_len, size_t count, const uint64_t cosets[3][4],
                          uint32_t cap, typlonk_witness_report* reports, uint32_t* gate_rows, uint32_t* copy_cells) {
    return witness_check_impl(ctx, circuit_id, ColumnsOf(wire_evals, count, ColumnsOf::PI_FIRST, pi, pi_len), cosets,
                              Outputs{cap, reports, gate_rows, copy_cells});
}

int typlonk_witness_check_host(typlonk_ctx* ctx, uint32_t circuit_id, const uint64_t* const* wire_evals, size_t rows,
                               const uint64_t* const* pi, const size_t* pi_len, size_t count, const uint64_t cosets[3][4],
                               uint32_t cap, typlonk_witness_report* reports, uint32_t* gate_rows, uint32_t* copy_cells) {
    return witness_check_impl(ctx, circuit_id, ColumnsOf(wire_evals, count, ColumnsOf::PI_FIRST, pi, pi_len).with_rows(rows),
                              cosets, Outputs{cap, reports, gate_rows, copy_cells});
}

int typlonk_circuit_compile(typlonk_ctx* ctx, const typlonk_buf* const selector_evals[5], const uint32_t* perm,
                            const uint64_t cosets[3][4], uint32_t log_n, uint32_t* circuit_id, uint64_t* defects) {
    PermSource from{};
    from.host = perm;
    return circuit_compile_impl(ctx, ColumnsOf(selector_evals, 1).selectors(), from, cosets, log_n, circuit_id, defects);
}

int typlonk_circuit_compile_host(typlonk_ctx* ctx, const uint64_t* const selector_evals[5], size_t rows, const uint32_t* perm,
                                 const uint64_t cosets[3][4], uint32_t log_n, uint32_t* circuit_id, uint64_t* defects) {
    PermSource from{};
    from.host = perm;
    return circuit_compile_impl(ctx, ColumnsOf(selector_evals, 1).selectors().with_rows(rows), from, cosets, log_n, circuit_id,
                                defects);
}
