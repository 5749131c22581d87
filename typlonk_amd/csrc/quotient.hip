// Quotient polynomial t(X) of the PLONK prover on the 4n coset domain -- replaces the 12 schoolbook
// `naive_mul` products + divide_by_vanishing_poly of plonk::proof::quotient_polynomial
// (/root/reference/plonk/src/proof.rs:292-375) by pointwise arithmetic on coset evaluations:
//
//   t = [ q_l a + q_r b - q_o c + q_m a b + q_c + PI
//         + alpha ( (a + beta k0 X + gamma)(b + beta k1 X + gamma)(c + beta k2 X + gamma) Z
//                 - (a + beta s0 + gamma)(b + beta s1 + gamma)(c + beta s2 + gamma) Z(wX) )
//         + alpha^2 (Z - 1) L0 ] / (X^n - 1)
//
// evaluated at x_i = g w_{4n}^i, i < 4n.  deg(numerator) <= 4n - 4 < 4n, so the inverse coset NTT of the
// pointwise quotient is exactly t whenever the numerator vanishes on H (any valid witness; the
// reference discards the remainder otherwise).  On this domain Z(w x_i) is the evaluation at index
// i + 4 (w = w_{4n}^4) and X^n - 1 takes only four values g^n i^k - 1, whose inverses come as arguments.
// The formula itself is quotient_point (scan_ops.hpp), shared with the wave's kernel (prove_batch.hip).
#include "launch.hpp"
#include "scan_ops.hpp"

namespace ty {

__global__ __launch_bounds__(256) void fr_fill_kernel(Fr* out, uint64_t n, Fr value) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p_st(out + i, value);
}

__global__ __launch_bounds__(256) void quotient_pointwise_kernel(QuotientArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n4) return;
    const Fr wa = p_ld(a.wires[0] + i), wb = p_ld(a.wires[1] + i), wc = p_ld(a.wires[2] + i);
    const Fr z = p_ld(a.z + i), zw = p_ld(a.z + ((i + 4) & (a.n4 - 1)));
    Fr sel[5], sig[3];
#pragma unroll
    for (int k = 0; k < 5; ++k) sel[k] = p_ld(a.sel[k] + i);
#pragma unroll
    for (int k = 0; k < 3; ++k) sig[k] = p_ld(a.sigma[k] + i);
    // beta * x_i, x_i = g * w_{4n}^i: the two-level power table of w_{4n} with beta * g folded into its upper level
    const Fr bx = fe_mul(p_ld(a.w_lo + (i & ((1ull << a.w_h) - 1))), p_ld(a.bx_hi + (i >> a.w_h)));
    // (no public-input polynomial = the zero polynomial)
    const Fr t = quotient_point(wa, wb, wc, z, zw, a.pi ? a.pi + i : nullptr, sel, sig, p_ld(a.l0 + i), bx, a.k, a.k0_is_one,
                                a.beta, a.gamma, a.alpha, a.alpha2, a.zh_inv[i & 3]);
    p_st(a.out + i, t);
}

__global__ __launch_bounds__(256) void fr_scale_kernel(const Fr* in, uint64_t n, Fr factor, Fr* out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p_st(out + i, fe_mul(p_ld(in + i), factor));
}

void launch_fr_scale(const Fr* in, uint64_t n, const Fr& factor, Fr* out, hipStream_t s) {
    hipLaunchKernelGGL(fr_scale_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, n, factor, out);
}
void launch_fr_fill(Fr* out, uint64_t n, const Fr& value, hipStream_t s) {
    hipLaunchKernelGGL(fr_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out, n, value);
}
void launch_quotient_pointwise(const QuotientArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(quotient_pointwise_kernel, dim3((unsigned)((a.n4 + 255) / 256)), dim3(256), 0, s, a);
}

}  // namespace ty
