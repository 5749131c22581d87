// The kernels of typlonk_recover_chunks (host: recover_chunks_host.hip; every shape: recover_chunks_plan.hpp): between the four
// transforms of a call, what recovers `count` polynomials from K of the r cosets of their domain.  n = 2^log_n, l = 2^log_l,
// r = n / l, w the generator of the size-n domain, a_k = w^(k l), g the quotient's coset generator.  The cosets the call does
// not name are the MISSING ones, Z'(Y) = prod over them of (Y - a_j), and Z(X) = Z'(X^l) vanishes on them:
//     Zd[k] = Z'(a_k)      = Z on every point of coset k                   (zero exactly on the missing cosets)
//     Zc[i] = Z'(g^l a_i)  = Z at g w^i' for every i' = i mod r            (never zero: g^n != 1)
//   recover_vanish_kernel / recover_vanish_combine_kernel   Zd and Zc, 2r plain products of `missing` factors each
//   recover_invert_kernel    Zc <- 1 / Zc
//   recover_scatter_kernel   V[p][k + r t] = E_p[pos[k]][t] Zd[k], zero on the missing cosets: h_p Z on the whole domain
//   recover_scale_kernel     V[p][i] *= ZcInv[i mod r], between the coset transforms: (h_p Z) / Z on g H
//   recover_excess_kernel / recover_finish_kernel   the lowest nonzero coefficient of [m, K l), the verdict, and the m low
//                            coefficients -- or zeros -- to their destinations
// Every barrier is a __syncthreads() that the whole workgroup meets the same number of times: the trip counts of the loops around
// them are launch arguments (or blockIdx alone), never data.
#include "launch.hpp"
#include "fr_inv.hpp"
#include "recover_chunks_plan.hpp"

namespace ty {

// ---- the vanishing products ---------------------------------------------------------------------------------------------------
// Thread x < 2r takes the point a_x (x < r) or g^l a_(x - r); workgroup (bx, s) the slice s of the missing set, `tiles` tiles of
// RECOVER_TILE factors: thread t of the workgroup stages a_(missing[base + t]) in the LDS, and after the barrier every lane walks
// the tile at the same address -- a broadcast, no bank conflict --  acc <- acc (x - a_j).  partial[s 2r + x] = the slice's product.
__global__ __launch_bounds__(256) void recover_vanish_kernel(const Fr* pw, const uint32_t* missing_idx, uint64_t missing, uint64_t r, Fr gl,
                                                             uint64_t per_slice, uint32_t tiles, Fr* partial) {
    __shared__ Fr tile[RECOVER_TILE];
    const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = x < 2 * r;
    Fr pt = Fr::zero();
    if (in) pt = x < r ? pw[x] : fe_mul(gl, pw[x - r]);
    const uint64_t lo = (uint64_t)blockIdx.y * per_slice;
    const uint64_t hi = lo + per_slice < missing ? lo + per_slice : missing;   // (lo >= missing only when missing = 0)
    Fr acc = Fr::one();
    for (uint32_t ti = 0; ti < tiles; ++ti) {
        const uint64_t base = lo + (uint64_t)ti * RECOVER_TILE;
        if (base + threadIdx.x < hi) tile[threadIdx.x] = pw[missing_idx[base + threadIdx.x]];
        __syncthreads();
        const uint32_t cnt = base < hi ? (uint32_t)(hi - base < RECOVER_TILE ? hi - base : RECOVER_TILE) : 0u;
#pragma unroll 1
        for (uint32_t j = 0; j < cnt; ++j) acc = fe_mul(acc, fe_sub(pt, tile[j]));
        __syncthreads();
    }
    if (in) partial[(uint64_t)blockIdx.y * 2 * r + x] = acc;
}
// z[x] = prod_{s < slices} partial[s 2r + x], in slice order
__global__ __launch_bounds__(256) void recover_vanish_combine_kernel(const Fr* partial, uint64_t r2, uint32_t slices, Fr* z) {
    const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= r2) return;
    Fr acc = partial[x];
    for (uint32_t s = 1; s < slices; ++s) acc = fe_mul(acc, partial[(uint64_t)s * r2 + x]);
    z[x] = acc;
}
void launch_recover_vanish(const Fr* pw, const uint32_t* missing_idx, const Fr& gl, const RecoverChunksPlan& pl, Fr* partial, Fr* z, hipStream_t st) {
    hipLaunchKernelGGL(recover_vanish_kernel, dim3(pl.vanish_xblocks, pl.slices), dim3(256), 0, st, pw, missing_idx, pl.missing, pl.r, gl,
                       pl.per_slice, pl.tiles, partial);
    hipLaunchKernelGGL(recover_vanish_combine_kernel, dim3(pl.vanish_xblocks), dim3(256), 0, st, partial, 2 * pl.r, pl.slices, z);
}

// z[i] <- 1 / z[i], i < cnt: one divsteps inversion a thread (0 -> 0)
__global__ __launch_bounds__(256) void recover_invert_kernel(Fr* z, uint64_t cnt) {
    const uint64_t i0 = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t i = i0 < cnt ? i0 : cnt - 1;   // spare lanes shadow the last value: fr_inv_divsteps votes across the wavefront
    const Fr inv = fr_inv_divsteps(z[i]);
    if (i0 < cnt) z[i0] = inv;
}
void launch_recover_invert(Fr* z, uint64_t cnt, hipStream_t st) {
    if (cnt == 0) return;
    hipLaunchKernelGGL(recover_invert_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, z, cnt);
}

// ---- the scatter ----------------------------------------------------------------------------------------------------------------
// Workgroup tile + tiles p (the grid's y stops at 65535 and a call may hold more polynomials): cosets [k0, k0 + TK) x points
// [t0, t0 + TT) of polynomial p, TK TT <= 256.  In: thread q reads the cell of coset k0 + q / TT at point t0 + q % TT -- runs of TT
// elements, contiguous in t -- or zero where pos names no cell.  Out: thread q writes index (k0 + q % TK) + r (t0 + q / TK) -- runs
// of TK elements, contiguous in k -- times Zd.  Every element of the n count is written, the zeros included.  A row of the tile
// (one coset's TT points) is padded by one element where TT > 1: on the way out the lanes of a run read a COLUMN, and with rows of
// 16 elements (512 bytes) sixteen lanes would meet in the same banks; with rows of 17 consecutive lanes are 8 words apart.
// TK (TT + 1) <= 256 + 128 elements.
__global__ __launch_bounds__(256) void recover_scatter_kernel(const Fr* cells, const uint32_t* pos, const Fr* zd, uint64_t K, uint32_t log_r,
                                                              uint32_t log_l, uint32_t log_tk, uint32_t log_tt, Fr* v) {
    __shared__ Fr tile[RECOVER_SCATTER_LDS];
    const uint32_t q = threadIdx.x, live = 1u << (log_tk + log_tt), row = (1u << log_tt) | 1u;   // TT + 1, or 1 at TT = 1
    const uint32_t log_tiles = log_r + log_l - log_tk - log_tt;
    const uint64_t p = (uint64_t)blockIdx.x >> log_tiles, tl = (uint64_t)blockIdx.x & ((1ull << log_tiles) - 1);
    const uint64_t tiles_t = 1ull << (log_l - log_tt);
    const uint64_t k0 = (tl / tiles_t) << log_tk, t0 = (tl % tiles_t) << log_tt;
    if (q < live) {
        const uint64_t k = k0 + (q >> log_tt), t = t0 + (q & ((1u << log_tt) - 1));
        const uint32_t c = pos[k];
        tile[(q >> log_tt) * row + (q & ((1u << log_tt) - 1))] = c == RECOVER_NO_CELL ? Fr::zero() : cells[((p * K + c) << log_l) + t];
    }
    __syncthreads();
    if (q < live) {
        const uint32_t ki = q & ((1u << log_tk) - 1), ti = q >> log_tk;
        const uint64_t k = k0 + ki, t = t0 + ti;
        v[(p << (log_r + log_l)) + k + (t << log_r)] = fe_mul(tile[ki * row + ti], zd[k]);
    }
}
void launch_recover_scatter(const Fr* cells, const uint32_t* pos, const Fr* zd, uint64_t K, uint32_t log_n, uint32_t log_l, uint64_t count,
                            const RecoverChunksPlan& pl, Fr* v, hipStream_t st) {
    hipLaunchKernelGGL(recover_scatter_kernel, dim3((unsigned)(pl.scatter_tiles * count)), dim3(256), 0, st, cells, pos, zd, K,
                       log_n - log_l, log_l, pl.log_tk, pl.log_tt, v);
}

// v[i] *= zc_inv[i & (r - 1)], i < total = count n (the vectors lie one behind the other, n a multiple of r)
__global__ __launch_bounds__(256) void recover_scale_kernel(Fr* v, const Fr* zc_inv, uint64_t r, uint64_t total) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    v[i] = fe_mul(v[i], zc_inv[i & (r - 1)]);
}
void launch_recover_scale(Fr* v, const Fr* zc_inv, uint64_t r, uint64_t total, hipStream_t st) {
    hipLaunchKernelGGL(recover_scale_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, v, zc_inv, r, total);
}

// ---- the finish -----------------------------------------------------------------------------------------------------------------
// Workgroup b + blocks p: the lowest j of [m + b span, min(m + (b + 1) span, m + len)) with v[p n + j] != 0, or all ones: each thread
// strides over the span `iters` times, a tree over the 256 minima in the LDS.  mins[p blocks + b].
__global__ __launch_bounds__(256) void recover_excess_kernel(const Fr* v, uint64_t n, uint64_t m, uint64_t len, uint64_t span, uint32_t iters, uint32_t blocks,
                                                             unsigned long long* mins) {
    __shared__ unsigned long long red[256];
    const uint64_t p = blockIdx.x / blocks, b = blockIdx.x % blocks;
    const uint64_t lo = m + b * span;
    const uint64_t hi = lo + span < m + len ? lo + span : m + len;
    unsigned long long best = ~0ull;
    for (uint32_t it = 0; it < iters; ++it) {
        const uint64_t j = lo + (uint64_t)it * 256 + threadIdx.x;
        if (j < hi && best == ~0ull && !v[p * n + j].is_zero()) best = j;   // (ascending in `it`: the first hit is the thread's lowest)
    }
    red[threadIdx.x] = best;
    for (uint32_t h = 128; h >= 1; h >>= 1) {
        __syncthreads();
        if (threadIdx.x < h && red[threadIdx.x + h] < red[threadIdx.x]) red[threadIdx.x] = red[threadIdx.x + h];
    }
    if (threadIdx.x == 0) mins[blockIdx.x] = red[0];
}
// Workgroup c + ceil(m / 256) p: the minimum of p's `blocks` partial minima in workgroup order (every thread reads the same words), the verdict
// -- fixed[p] != 0: that status stands; else INCONSISTENT when a coefficient was found, else OK -- and then coefficients
// [256 c, 256 c + 256) of the m: v's for an OK polynomial, zeros for any other, to dst[p] (NULL: none) and out + p m (out NULL: none).
// Workgroup c = 0 writes verdict[p] = first_excess (all ones unless INCONSISTENT) and verdict[count + p] = the status.
struct RecoverFinishArgs {
    const Fr* v;
    uint64_t n, m, count;
    uint32_t mblocks;   // ceil(m / 256)
    const unsigned long long* mins;
    uint32_t blocks;
    const uint8_t* fixed;
    Fr* const* dst;
    Fr* out;
    unsigned long long* verdict;
};
__global__ __launch_bounds__(256) void recover_finish_kernel(RecoverFinishArgs a) {
    const uint64_t p = blockIdx.x / a.mblocks, c0 = blockIdx.x % a.mblocks;
    unsigned long long first = ~0ull;
    for (uint32_t b = 0; b < a.blocks; ++b) {
        const unsigned long long x = a.mins[p * a.blocks + b];
        first = x < first ? x : first;
    }
    uint32_t status = a.fixed[p];
    if (status != 0)
        first = ~0ull;
    else if (first != ~0ull)
        status = 2;   // TYPLONK_RECOVER_INCONSISTENT
    if (c0 == 0 && threadIdx.x == 0) {
        a.verdict[p] = first;
        a.verdict[a.count + p] = status;
    }
    const uint64_t j = c0 * 256 + threadIdx.x;
    if (j >= a.m) return;
    const Fr c = status == 0 ? a.v[p * a.n + j] : Fr::zero();
    Fr* d = a.dst ? a.dst[p] : nullptr;
    if (d) d[j] = c;
    if (a.out) a.out[p * a.m + j] = c;
}
void launch_recover_finish(const Fr* v, uint64_t n, uint64_t m, uint64_t count, const RecoverChunksPlan& pl, const uint8_t* fixed,
                           Fr* const* dst, Fr* out, unsigned long long* mins, unsigned long long* verdict, hipStream_t st) {
    hipLaunchKernelGGL(recover_excess_kernel, dim3((unsigned)(pl.excess_blocks * count)), dim3(256), 0, st, v, n, m, pl.excess_len, pl.excess_span,
                       pl.excess_iters, pl.excess_blocks, mins);
    const uint32_t mblocks = (uint32_t)((m + 255) / 256);
    RecoverFinishArgs a{v, n, m, count, mblocks, mins, pl.excess_blocks, fixed, dst, out, verdict};
    hipLaunchKernelGGL(recover_finish_kernel, dim3((unsigned)(mblocks * count)), dim3(256), 0, st, a);
}

}  // namespace ty
