// The kernels of typlonk_verify_chunks (host: verify_chunks_host.hip; the fold's launch shape: verify_chunks_plan.hpp): the
// membership of a batch's points, one flag per point, the weights of one fold, and the fold of the cells' interpolants into one
// polynomial of l coefficients.  n = 2^log_n, l = 2^log_l, r = n / l, w the generator of the size-n domain, mu = w^r that of
// the size-l domain.  Cell i carries a coset index k_i < r and l evaluations E_i[t] = f(w^(k_i + r t)); its interpolant is
//     I_i = sum_{j<l} X^j w^(-k_i j) (1/l) sum_t E_i[t] mu^(-j t)
// and a fold over the live cells of [lo, hi) with the weights rho_i = rho^i needs, beside two MSMs over the proofs and the
// commitments,  A_j = sum_i rho_i w^(-k_i j) (1/l) sum_t E_i[t] mu^(-j t),  the coefficients of sum_i rho_i I_i.
#include "launch.hpp"
#include "g1_ladder.hpp"
#include "point_codec.hpp"
#include "verify_chunks_plan.hpp"

namespace ty {

// ---- membership, one flag per point --------------------------------------------------------------------------------------------
// flags[i] = g1_record_class of record i (point_codec.hpp: PC_OK, PC_NOT_ON_CURVE or PC_NOT_IN_SUBGROUP), the test of
// srs_membership_kernel, which reports only the lowest failing index.  clear: a record that fails is overwritten with the
// identity, so that nothing that is not a group element is ever summed.  One thread per point, each on its own record.
__global__ __launch_bounds__(64) void chunks_membership_kernel(uint32_t* pts, uint64_t n, uint8_t* flags, uint32_t clear) {
    const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint32_t st = g1_record_class(ld_affine(pts, i));
    flags[i] = (uint8_t)st;
    if (st != PC_OK && clear) {
        uint4* q = reinterpret_cast<uint4*>(pts + i * PT_WORDS);
#pragma unroll
        for (int w = 0; w < PT_WORDS / 4; ++w) q[w] = make_uint4(0, 0, 0, 0);
    }
}
void launch_chunks_membership(uint32_t* pts, uint64_t n, uint8_t* flags, bool clear, hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(chunks_membership_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, pts, n, flags, clear ? 1u : 0u);
}

// ---- the weights of one fold -----------------------------------------------------------------------------------------------------
// b^ex for ex < 2^bits, most significant bit first
__device__ __forceinline__ Fr fr_pow_bits(const Fr& b, uint32_t ex, int bits) {
    Fr e = Fr::one();
#pragma unroll 1
    for (int bit = bits - 1; bit >= 0; --bit) {
        e = fe_sqr(e);
        if ((ex >> bit) & 1u) e = fe_mul(e, b);
    }
    return e;
}

// What a cell's coset index gives, once per call: coset_a[i] = a_(k_i) = (w^l)^(k_i) and twist[i] = w^(-k_i); one thread a cell
__global__ __launch_bounds__(256) void chunks_cosets_kernel(const uint32_t* cell_coset, uint64_t N, Fr root_r, Fr w_inv, Fr* coset_a, Fr* twist) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const uint64_t k = cell_coset[i];
    coset_a[i] = fr_pow_u64(root_r, k);
    twist[i] = fr_pow_u64(w_inv, k);
}
void launch_chunks_cosets(const uint32_t* cell_coset, uint64_t N, const Fr& root_r, const Fr& w_inv, Fr* coset_a, Fr* twist, hipStream_t st) {
    if (N == 0) return;
    hipLaunchKernelGGL(chunks_cosets_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, cell_coset, N, root_r, w_inv, coset_a, twist);
}

// For the fold over [lo, hi): cell i is IN when lo <= i < hi and live[i].  The first cell_blocks workgroups take one cell a
// thread and write
//     s_pi[i] = rho_i, s_all[i] = rho_i coset_a[i], scale[i] = rho_i / l   for a cell that is in, zero otherwise
// with rho_i = pw[i] the powers of launch_fr_powers.  Each of the M workgroups behind them takes one commitment c.  The cells
// come sorted by commitment: order[first[c] .. first[c + 1]) are the cells with c_i = c in ascending order (the host's counting
// sort), so a workgroup reads its own cells only, N indices a launch in all.  Its threads stride over them, each summing the
// rho_i of the cells that are in, and a tree over the workgroup's 256 sums in the LDS gives w_c: s_pi[N + c] = 0,
// s_all[N + c] = w_c.  The order of the additions is fixed by the call's cells alone: no atomics.
struct ChunksWeightsArgs {
    const Fr* pw;
    const Fr* coset_a;
    const uint32_t* order;
    const uint32_t* first;
    const uint8_t* live;
    uint64_t N, M, lo, hi;
    uint32_t cell_blocks;
    Fr l_inv;
    Fr *s_pi, *s_all, *scale;
};
__global__ __launch_bounds__(256) void chunks_weights_kernel(ChunksWeightsArgs a) {
    __shared__ Fr red[256];
    if (blockIdx.x < a.cell_blocks) {   // (uniform over the workgroup; this half meets no barrier)
        const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
        if (i >= a.N) return;
        const bool in = i >= a.lo && i < a.hi && a.live[i];
        const Fr rho = in ? a.pw[i] : Fr::zero();
        a.s_pi[i] = rho;
        a.s_all[i] = in ? fe_mul(rho, a.coset_a[i]) : Fr::zero();
        a.scale[i] = in ? fe_mul(rho, a.l_inv) : Fr::zero();
        return;
    }
    const uint64_t c = blockIdx.x - a.cell_blocks;
    const uint32_t end = a.first[c + 1];
    Fr s = Fr::zero();
    for (uint32_t t = a.first[c] + threadIdx.x; t < end; t += 256) {
        const uint64_t i = a.order[t];
        if (i >= a.lo && i < a.hi && a.live[i]) s = fe_add(s, a.pw[i]);
    }
    red[threadIdx.x] = s;
    for (uint32_t h = 128; h >= 1; h >>= 1) {
        __syncthreads();
        if (threadIdx.x < h) red[threadIdx.x] = fe_add(red[threadIdx.x], red[threadIdx.x + h]);
    }
    if (threadIdx.x == 0) {
        a.s_pi[a.N + c] = Fr::zero();
        a.s_all[a.N + c] = red[0];
    }
}
void launch_chunks_weights(const Fr* pw, const Fr* coset_a, const uint32_t* order, const uint32_t* first, const uint8_t* live, uint64_t N,
                           uint64_t M, uint64_t lo, uint64_t hi, const Fr& l_inv, Fr* s_pi, Fr* s_all, Fr* scale, hipStream_t st) {
    ChunksWeightsArgs a;
    a.pw = pw;
    a.coset_a = coset_a;
    a.order = order;
    a.first = first;
    a.live = live;
    a.N = N;
    a.M = M;
    a.lo = lo;
    a.hi = hi;
    a.cell_blocks = (uint32_t)((N + 255) / 256);
    a.l_inv = l_inv;
    a.s_pi = s_pi;
    a.s_all = s_all;
    a.scale = scale;
    hipLaunchKernelGGL(chunks_weights_kernel, dim3((unsigned)(a.cell_blocks + M)), dim3(256), 0, st, a);
}

// ---- the fold ------------------------------------------------------------------------------------------------------------------------
// Workgroup b takes the cells lo + [b strip, min((b + 1) strip, cells)) (verify_chunks_plan.hpp); group g of its threads takes
// every groups-th of them, one after the other.  Per cell: the l evaluations times scale[cell] = rho / l into the group's l
// elements of the LDS; a radix-2 decimation-in-frequency transform in place with the inverse twiddles tw[j] = mu^(-j), j < l / 2,
// which leaves X_j = sum_t x_t mu^(-j t) at the bit-reversed index of j; then thread q adds twist[cell]^j X_j into its accumulator
// of coefficient j = q + p group, p < PER.  A group past the end of its strip runs along on zeros: every barrier is met by the
// whole workgroup the same number of times (iters and l are uniform over the launch).  After the strip the groups' accumulators
// are added in group order and the workgroup writes partial[b l + j], j < l.  Every value is a canonical residue throughout.
struct ChunksFoldArgs {
    const Fr* evals;    // cell i at evals + i l
    const Fr* scale;
    const Fr* twist;
    const Fr* tw;       // max(l / 2, 1) inverse twiddles
    Fr* partial;        // blocks * l
    uint64_t lo, cells, strip;
    uint32_t log_l, group, iters;
};
template <int PER>
__global__ __launch_bounds__(256) void chunks_fold_kernel(ChunksFoldArgs a) {
    extern __shared__ uint4 chunks_lds[];
    const uint32_t l = 1u << a.log_l, half_l = l >> 1;
    const uint32_t T = a.group, G = VERIFY_CHUNKS_THREADS / T;
    const uint32_t g = threadIdx.x / T, q = threadIdx.x % T;
    Fr* buf = reinterpret_cast<Fr*>(chunks_lds);
    Fr* tw = buf + (size_t)G * l;
    Fr* x = buf + (size_t)g * l;
    for (uint32_t j = threadIdx.x; j < (half_l ? half_l : 1u); j += VERIFY_CHUNKS_THREADS) tw[j] = a.tw[j];
    const uint64_t first = (uint64_t)blockIdx.x * a.strip;
    const uint64_t last = first + a.strip < a.cells ? first + a.strip : a.cells;
    Fr acc[PER];
#pragma unroll
    for (int p = 0; p < PER; ++p) acc[p] = Fr::zero();
#pragma unroll 1
    for (uint32_t it = 0; it < a.iters; ++it) {
        const uint64_t local = first + (uint64_t)it * G + g;
        const bool have = local < last;
        const uint64_t cell = a.lo + (have ? local : first);   // (first < cells: an address that exists)
        __syncthreads();   // the table is in place; the last cell's elements have been read
        const Fr k = have ? a.scale[cell] : Fr::zero();
        for (uint32_t e = q; e < l; e += T) x[e] = have ? fe_mul(a.evals[cell * l + e], k) : Fr::zero();
        uint32_t sh = 0;
#pragma unroll 1
        for (uint32_t half = half_l; half >= 1; half >>= 1, ++sh) {
            __syncthreads();
            for (uint32_t b = q; b < half_l; b += T) {
                const uint32_t pos = b & (half - 1), i0 = ((b - pos) << 1) + pos, i1 = i0 + half;
                const Fr u = x[i0], v = x[i1];
                x[i0] = fe_add(u, v);
                x[i1] = fe_mul(fe_sub(u, v), tw[pos << sh]);
            }
        }
        __syncthreads();
        const Fr base = a.twist[cell];
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const uint32_t j = q + (uint32_t)p * T;
            if (j < l) {
                const uint32_t rev = a.log_l ? __brev(j) >> (32 - a.log_l) : 0u;
                acc[p] = fe_add(acc[p], fe_mul(fr_pow_bits(base, j, (int)a.log_l), x[rev]));
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < PER; ++p) {
        const uint32_t j = q + (uint32_t)p * T;
        if (j < l) x[j] = acc[p];
    }
    __syncthreads();
    if (g != 0) return;   // (behind the last barrier)
#pragma unroll
    for (int p = 0; p < PER; ++p) {
        const uint32_t j = q + (uint32_t)p * T;
        if (j < l) {
            Fr s = buf[j];
            for (uint32_t o = 1; o < G; ++o) s = fe_add(s, buf[(size_t)o * l + j]);
            a.partial[(uint64_t)blockIdx.x * l + j] = s;
        }
    }
}
// cells >= 1 cells from lo on; pl = verify_chunks_plan(cells, log_l[, strip]); partial: pl.blocks * l elements
void launch_chunks_fold(const Fr* evals, const Fr* scale, const Fr* twist, const Fr* tw, uint64_t lo, uint64_t cells, uint32_t log_l,
                        const VerifyChunksPlan& pl, Fr* partial, hipStream_t st) {
    ChunksFoldArgs a;
    a.evals = evals;
    a.scale = scale;
    a.twist = twist;
    a.tw = tw;
    a.partial = partial;
    a.lo = lo;
    a.cells = cells;
    a.strip = pl.strip;
    a.log_l = log_l;
    a.group = pl.group;
    a.iters = pl.iters;
    const dim3 grid((unsigned)pl.blocks), block(VERIFY_CHUNKS_THREADS);
    if (pl.per == 1) hipLaunchKernelGGL(chunks_fold_kernel<1>, grid, block, pl.lds_bytes, st, a);
    else if (pl.per == 2) hipLaunchKernelGGL(chunks_fold_kernel<2>, grid, block, pl.lds_bytes, st, a);
    else hipLaunchKernelGGL(chunks_fold_kernel<4>, grid, block, pl.lds_bytes, st, a);
}

// A[j] = sum over the workgroups b < blocks, in that order, of partial[b l + j]; one thread per coefficient.  The sum is a field
// element in canonical form, so every strip size gives the same words.
__global__ __launch_bounds__(256) void chunks_fold_sum_kernel(const Fr* partial, uint64_t blocks, uint32_t l, Fr* out) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= l) return;
    Fr s = Fr::zero();
    for (uint64_t b = 0; b < blocks; ++b) s = fe_add(s, partial[b * l + j]);
    out[j] = s;
}
void launch_chunks_fold_sum(const Fr* partial, uint64_t blocks, uint32_t l, Fr* out, hipStream_t st) {
    hipLaunchKernelGGL(chunks_fold_sum_kernel, dim3((l + 255) / 256), dim3(256), 0, st, partial, blocks, l, out);
}

}  // namespace ty
