// O(n) prover steps that sit between the NTT / MSM kernels of prove(), kept on the device so that
// polynomials never cross PCIe inside a proof:
//
//   grand product   permutation::CompiledPermutation::prove   /root/reference/permutation/src/proving.rs:7-31
//   open            kzg::KzgScheme::open (Horner + division)   /root/reference/kzg/src/lib.rs:55-61
//   lincomb         the axpy combinations of linearisation_poly /root/reference/plonk/src/proof.rs:376-439
//
// All three are scans over Fr.  The grand product avoids the reference's one field division per cell:
//   Z_j = prod_{k<j} num_k / prod_{k<j} den_k = N_j * S_j * S_0^-1,
// N = exclusive prefix products of the numerators, S_j = prod_{k>=j} den_k (suffix products), so one
// inversion (of S_0, on the device: fr_inv_kernel) serves the whole column.  Field arithmetic is exact, so every Z_j is
// the same field element the reference computes.
#include "fr_inv.hpp"
#include "launch.hpp"
#include "scan_ops.hpp"

namespace ty {

// num_j, den_j of every row (gp_term, scan_ops.hpp)
__global__ __launch_bounds__(256) void gp_terms_kernel(GrandProductArgs a) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= a.n) return;
    const Fr x = fe_mul(p_ld(a.w_lo + (j & ((1ull << a.w_h) - 1))), p_ld(a.w_hi + (j >> a.w_h)));
    Fr num = Fr::one(), den = Fr::one();
#pragma unroll
    for (int i = 0; i < 3; ++i) gp_term(a.wires[i] + j, a.sigma[i] + j, x, a.beta, a.gamma, a.kbeta[i], num, den);
    p_st(a.num + j, num);
    p_st(a.den + j, den);
}

// ---- product scan over Fr: three launches, 2048 elements per workgroup (8 per thread); the bodies are in scan_ops.hpp
__global__ __launch_bounds__(256) void pscan_block_kernel(const Fr* in, uint64_t n, int reverse, Fr* block_prod) {
    pscan_block(in, n, reverse, block_prod, blockIdx.x);
}
__global__ __launch_bounds__(256) void pscan_top_kernel(Fr* block_prod, uint32_t nblocks) { pscan_top(block_prod, nblocks); }
__global__ __launch_bounds__(256) void pscan_finish_kernel(const Fr* in, uint64_t n, int reverse, const Fr* block_excl,
                                                           Fr* out) {
    pscan_finish(in, n, reverse, block_excl, out, blockIdx.x);
}

// out[0] = in[0]^-1 (0 -> 0): one wavefront, every lane the same value -- the ONE inversion of a proof's grand product
// (fr_inv.hpp: divsteps, ~20 rounds of 30), on the device so that round 2 never drains the stream for it
__global__ __launch_bounds__(64) void fr_inv_kernel(const Fr* in, Fr* out) {
    const Fr x = fr_inv_divsteps(p_ld(in));
    if (threadIdx.x == 0) p_st(out, x);
}
// Z_j = N_j * S_j * inv_total
__global__ __launch_bounds__(256) void gp_finish_kernel(const Fr* nprefix, const Fr* dsuffix, const Fr* inv_total, uint64_t n, Fr* z) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    p_st(z + j, gp_finish(p_ld(nprefix + j), p_ld(dsuffix + j), p_ld(inv_total)));
}

// ---- open(): H_j = c_j + z H_{j+1} (H_m = 0) for all j at once; the three stages are bodies of scan_ops.hpp -------------

struct OpenArgs {
    const Fr* c;
    uint64_t m;
    Fr* q;          // m - 1 coefficients, may be null (evaluation only)
    Fr* blocks;     // per-workgroup values / carries
    Fr* y;          // device scalar: p(z)
    Fr zpow[32];    // z^(2^k)
};
__device__ __forceinline__ OpenItem open_item(const OpenArgs& a) { return OpenItem{a.c, a.q, a.y, a.zpow, a.blocks}; }

__global__ __launch_bounds__(256) void open_block_kernel(OpenArgs a) {
    __shared__ Fr lds[256];
    open_block_stage(open_item(a), a.m, lds);
}
// (always stores the carries: an evaluation too goes through the second sweep, which writes only y)
__global__ __launch_bounds__(256) void open_top_kernel(OpenArgs a, uint32_t nblk) {
    __shared__ Fr lds[256];
    open_top_stage(open_item(a), nblk, true, lds);
}
__global__ __launch_bounds__(256) void open_finish_kernel(OpenArgs a) {
    __shared__ Fr lds[256];
    open_finish_stage(open_item(a), a.m, lds);
}

// ---- up to 8 openings / evaluations of polynomials of the same length at one of two points: three launches in all ----
// (round 3 of the prover: a, b, c, Z, sigma_0, sigma_1, PI at zeta and Z at zeta * w were seventeen launches of
// 25-55 us each on the context's stream before anything else of the round could start)
struct OpenMultiArgs {
    const Fr* c[8];
    Fr* q[8];        // m - 1 quotient coefficients, or null: evaluation only
    Fr* y[8];        // device scalars
    uint8_t zsel[8]; // which of the two points
    uint64_t m;
    Fr* blocks;      // 8 * nblk per-workgroup values / carries
    uint32_t nblk;
    Fr zpow[2][32];
};
__device__ __forceinline__ OpenItem open_item(const OpenMultiArgs& a, uint32_t k) {
    return OpenItem{a.c[k], a.q[k], a.y[k], a.zpow[a.zsel[k]], a.blocks + (uint64_t)k * a.nblk};
}
__global__ __launch_bounds__(256) void open_multi_block_kernel(OpenMultiArgs a) {
    __shared__ Fr lds[256];
    open_block_stage(open_item(a, blockIdx.y), a.m, lds);
}
__global__ __launch_bounds__(256) void open_multi_top_kernel(OpenMultiArgs a) {
    __shared__ Fr lds[256];
    const OpenItem it = open_item(a, blockIdx.x);
    open_top_stage(it, a.nblk, it.q != nullptr, lds);
}
__global__ __launch_bounds__(256) void open_multi_finish_kernel(OpenMultiArgs a) {
    __shared__ Fr lds[256];
    const OpenItem it = open_item(a, blockIdx.y);
    if (!it.q) return;  // an evaluation was complete at the top stage (whole workgroup: no barrier is skipped by part of it)
    open_finish_stage(it, a.m, lds);
}
void launch_open_multi(const Fr* const* polys, Fr* const* quotients, Fr* const* ys, const uint8_t* zsel, uint32_t count,
                       uint64_t m, const Fr& z0, const Fr& z1, Fr* blocks, hipStream_t s) {
    OpenMultiArgs a;
    for (uint32_t k = 0; k < 8; ++k) {
        const uint32_t j = k < count ? k : 0;
        a.c[k] = polys[j];
        a.q[k] = quotients[j];
        a.y[k] = ys[j];
        a.zsel[k] = zsel[j];
    }
    a.m = m;
    a.blocks = blocks;
    a.nblk = (uint32_t)((m + 2047) / 2048);
    a.zpow[0][0] = z0;
    a.zpow[1][0] = z1;
    for (int k = 1; k < 32; ++k) {
        a.zpow[0][k] = fe_sqr(a.zpow[0][k - 1]);
        a.zpow[1][k] = fe_sqr(a.zpow[1][k - 1]);
    }
    hipLaunchKernelGGL(open_multi_block_kernel, dim3(a.nblk, count), dim3(256), 0, s, a);
    hipLaunchKernelGGL(open_multi_top_kernel, dim3(count), dim3(256), 0, s, a);
    hipLaunchKernelGGL(open_multi_finish_kernel, dim3(a.nblk, count), dim3(256), 0, s, a);
}

// ---- out[i] = sum_k scalar_k * poly_k[i]  (+ constant on coefficient 0) ---------------------------------
__global__ __launch_bounds__(256) void lincomb_kernel(LincombArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    Fr acc = (i == 0) ? a.constant : Fr::zero();
    for (uint32_t k = 0; k < a.terms; ++k) acc = fe_add(acc, fe_mul(a.scalar[k], p_ld(a.poly[k] + i)));
    p_st(a.out + i, acc);
}

void launch_lincomb(const LincombArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(lincomb_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a);
}

void launch_open(const Fr* c, uint64_t m, const Fr& z, Fr* q, Fr* blocks, Fr* y, hipStream_t s) {
    OpenArgs a;
    a.c = c;
    a.m = m;
    a.q = q;
    a.blocks = blocks;
    a.y = y;
    a.zpow[0] = z;
    for (int k = 1; k < 32; ++k) a.zpow[k] = fe_sqr(a.zpow[k - 1]);
    const uint32_t nblk = (uint32_t)((m + 2047) / 2048);
    hipLaunchKernelGGL(open_block_kernel, dim3(nblk), dim3(256), 0, s, a);
    hipLaunchKernelGGL(open_top_kernel, dim3(1), dim3(256), 0, s, a, nblk);
    hipLaunchKernelGGL(open_finish_kernel, dim3(nblk), dim3(256), 0, s, a);
}

void launch_gp_terms(const GrandProductArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(gp_terms_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a);
}
void launch_product_scan(const Fr* in, uint64_t n, int reverse, Fr* block_scratch, Fr* out, hipStream_t s) {
    const uint32_t nblk = (uint32_t)((n + PSCAN_PER_BLOCK - 1) / PSCAN_PER_BLOCK);
    hipLaunchKernelGGL(pscan_block_kernel, dim3(nblk), dim3(256), 0, s, in, n, reverse, block_scratch);
    hipLaunchKernelGGL(pscan_top_kernel, dim3(1), dim3(256), 0, s, block_scratch, nblk);
    hipLaunchKernelGGL(pscan_finish_kernel, dim3(nblk), dim3(256), 0, s, in, n, reverse, block_scratch, out);
}
void launch_fr_inv(const Fr* in, Fr* out, hipStream_t s) { hipLaunchKernelGGL(fr_inv_kernel, dim3(1), dim3(64), 0, s, in, out); }
void launch_gp_finish(const Fr* nprefix, const Fr* dsuffix, const Fr* inv_total, uint64_t n, Fr* z, hipStream_t s) {
    hipLaunchKernelGGL(gp_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, nprefix, dsuffix, inv_total, n, z);
}

}  // namespace ty
