// Device bodies shared by the prover's kernels for one proof (plonk_ops.hip, quotient.hip) and for a wave of proofs
// (prove_batch.hip, the proof index in blockIdx.y): 32-byte loads / stores, the product scan over Fr, the grand product's
// row term, the three stages of open() and the quotient's formula at one coset point.  The kernels around them differ only
// in where their operands come from: by-value arguments for one proof, device tables for a wave.
#pragma once
#include "launch.hpp"

namespace ty {

__device__ __forceinline__ Fr p_ld(const Fr* p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    const uint4 a = q[0], b = q[1];
    Fr r;
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
    r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
    return r;
}
__device__ __forceinline__ void p_st(Fr* p, const Fr& r) {
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(r.v[0], r.v[1], r.v[2], r.v[3]);
    q[1] = make_uint4(r.v[4], r.v[5], r.v[6], r.v[7]);
}

// ---- product scan over Fr: three launches, 2048 elements per workgroup (8 per thread) ----------------
// reverse = 0: out[j] = prod_{k<j} in[k] (exclusive prefix);  reverse = 1: out[j] = prod_{k>=j} in[k]
constexpr int PSCAN_PER_BLOCK = 2048;

__device__ __forceinline__ uint64_t pscan_index(uint64_t pos, uint64_t n, int reverse) { return reverse ? n - 1 - pos : pos; }

__device__ __forceinline__ void pscan_block(const Fr* in, uint64_t n, int reverse, Fr* block_prod, uint32_t blk) {
    __shared__ Fr red[256];
    const uint64_t base = (uint64_t)blk * PSCAN_PER_BLOCK + threadIdx.x * 8;
    Fr p = Fr::one();
    for (int e = 0; e < 8; ++e)
        if (base + e < n) p = fe_mul(p, p_ld(in + pscan_index(base + e, n, reverse)));
    red[threadIdx.x] = p;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] = fe_mul(red[threadIdx.x], red[threadIdx.x + off]);
        __syncthreads();
    }
    if (threadIdx.x == 0) p_st(block_prod + blk, red[0]);
}
// single workgroup: exclusive scan of the block products in place (sequential over chunks of 256)
__device__ __forceinline__ void pscan_top(Fr* block_prod, uint32_t nblocks) {
    __shared__ Fr buf[256];
    __shared__ Fr running;
    if (threadIdx.x == 0) running = Fr::one();
    __syncthreads();
    for (uint32_t base = 0; base < nblocks; base += 256) {
        const uint32_t i = base + threadIdx.x;
        const Fr v = i < nblocks ? p_ld(block_prod + i) : Fr::one();
        buf[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            Fr t = Fr::one();
            if ((int)threadIdx.x >= off) t = buf[threadIdx.x - off];
            __syncthreads();
            buf[threadIdx.x] = fe_mul(buf[threadIdx.x], t);
            __syncthreads();
        }
        // exclusive value = running * (inclusive of the previous lane)
        Fr excl = running;
        if (threadIdx.x > 0) excl = fe_mul(running, buf[threadIdx.x - 1]);
        const Fr total = fe_mul(running, buf[255]);
        if (i < nblocks) p_st(block_prod + i, excl);
        __syncthreads();
        if (threadIdx.x == 0) running = total;
        __syncthreads();
    }
}
__device__ __forceinline__ void pscan_finish(const Fr* in, uint64_t n, int reverse, const Fr* block_excl, Fr* out, uint32_t blk) {
    __shared__ Fr buf[256];
    const uint64_t base = (uint64_t)blk * PSCAN_PER_BLOCK + threadIdx.x * 8;
    Fr v[8];
    Fr p = Fr::one();
    for (int e = 0; e < 8; ++e) {
        v[e] = base + e < n ? p_ld(in + pscan_index(base + e, n, reverse)) : Fr::one();
        p = fe_mul(p, v[e]);
    }
    buf[threadIdx.x] = p;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        Fr t = Fr::one();
        if ((int)threadIdx.x >= off) t = buf[threadIdx.x - off];
        __syncthreads();
        buf[threadIdx.x] = fe_mul(buf[threadIdx.x], t);
        __syncthreads();
    }
    Fr run = p_ld(block_excl + blk);
    if (threadIdx.x > 0) run = fe_mul(run, buf[threadIdx.x - 1]);
    for (int e = 0; e < 8; ++e) {
        if (base + e < n) {
            if (reverse) {
                run = fe_mul(run, v[e]);  // inclusive in scan order = product of in[k], k >= index
                p_st(out + pscan_index(base + e, n, 1), run);
            } else {
                p_st(out + base + e, run);  // exclusive prefix
                run = fe_mul(run, v[e]);
            }
        }
    }
}

// ---- open(): H_j = c_j + z H_{j+1} (H_m = 0) for all j at once ------------------------------------------
// y = p(z) = H_0 and (p - y) / (X - z) has coefficients q_{j-1} = H_j: Horner evaluation and synthetic
// division are the same suffix recurrence.  A thread owns 8 consecutive coefficients, a workgroup
// 2048; inside the workgroup the per-thread values are combined by a Hillis-Steele suffix scan with
// ratio z^8 (multipliers z^(8*2^k) come precomputed as zpow[3+k]).  `seed` is the value of H at the END
// of the workgroup's range (0 in the first sweep, the scanned carry in the second).
__device__ __forceinline__ Fr horner_block(const Fr* c, uint64_t m, uint64_t base, const Fr& seed, const Fr* zpow,
                                           int pow0, Fr* lds, Fr (&loc)[8], Fr* carry_in) {
    // local Horner over [base + 8t, base + 8t + 8); the last thread starts from the seed
    const uint64_t s0 = base + (uint64_t)threadIdx.x * 8;
    Fr h = (threadIdx.x == 255) ? seed : Fr::zero();
    const Fr z = zpow[pow0];
    for (int e = 7; e >= 0; --e) {
        loc[e] = (s0 + e < m) ? p_ld(c + s0 + e) : Fr::zero();
        h = fe_add(loc[e], fe_mul(z, h));
    }
    lds[threadIdx.x] = h;
    __syncthreads();
    // G_t = sum_{t' >= t} h_t' (z^8)^(t' - t)
    for (int k = 0; k < 8; ++k) {
        const int off = 1 << k;
        Fr add = Fr::zero();
        if ((int)threadIdx.x + off < 256) add = fe_mul(zpow[pow0 + 3 + k], lds[threadIdx.x + off]);
        __syncthreads();
        lds[threadIdx.x] = fe_add(lds[threadIdx.x], add);
        __syncthreads();
    }
    // value of H just after this thread's range
    *carry_in = (threadIdx.x == 255) ? seed : lds[threadIdx.x + 1];
    return lds[0];
}

// single workgroup: carries between workgroups, C_b = A_b + z^2048 C_{b+1}; blocks[b] <- C_{b+1} (the value of H at the
// end of workgroup b); returns C_0 = p(z).  Rounds of 2048 entries from the high end, each seeded with the C its upper
// neighbour ended on: horner_block then carries the seed across the round with (z^2048)^2048 = z^(2^22), so any number of
// workgroups is one launch of the same kernel (m <= 2^22: one round from a zero seed, as before).  A third scan level
// would cost two more launches at every size for at most 8 serial rounds of ~3 us at m = 2^25.
__device__ __forceinline__ Fr open_top_rounds(Fr* blocks, uint32_t nblk, const Fr* zpow, bool store, Fr* lds) {
    Fr loc[8], ci;
    Fr run = Fr::zero();
    const Fr zb = zpow[11];
    for (uint32_t r = (nblk + 2047) / 2048; r-- > 0;) {
        const uint64_t base = (uint64_t)r * 2048;
        const Fr c0 = horner_block(blocks, nblk, base, run, zpow, 11, lds, loc, &ci);
        if (store) {
            // recompute the local chain from the true carry-in and store, for every entry, H of the NEXT entry
            Fr h = ci;
            const uint64_t s0 = base + (uint64_t)threadIdx.x * 8;
            for (int e = 7; e >= 0; --e) {
                if (s0 + e < nblk) p_st(blocks + s0 + e, h);
                h = fe_add(loc[e], fe_mul(zb, h));
            }
        }
        run = c0;
        __syncthreads();   // the next round's horner_block overwrites the LDS this one's lds[0] / carries came from
    }
    return run;
}

// One opening (q != null: y = p(z) and the m - 1 coefficients of (p - y) / (X - z)) or evaluation (q == null) of an
// m-coefficient polynomial: zpow = the 32 powers z^(2^k), carries = one Fr per 2048-coefficient workgroup.
struct OpenItem {
    const Fr* c;
    Fr* q;
    Fr* y;
    const Fr* zpow;
    Fr* carries;
};
// sweep 1 (one workgroup per 2048 coefficients): H at the start of every workgroup assuming a zero carry
__device__ __forceinline__ void open_block_stage(const OpenItem& it, uint64_t m, Fr* lds) {
    Fr loc[8], ci;
    const Fr g0 = horner_block(it.c, m, (uint64_t)blockIdx.x * 2048, Fr::zero(), it.zpow, 0, lds, loc, &ci);
    if (threadIdx.x == 0) p_st(it.carries + blockIdx.x, g0);
}
// top stage (one workgroup): the true carries when a second sweep follows (store); otherwise p(z) = sum_b A_b (z^2048)^b
// is complete here and goes to y
__device__ __forceinline__ void open_top_stage(const OpenItem& it, uint32_t nblk, bool store, Fr* lds) {
    const Fr y = open_top_rounds(it.carries, nblk, it.zpow, store, lds);
    if (!store && threadIdx.x == 0) p_st(it.y, y);
}
// sweep 2: seeded with the true carry; writes y and, where there is one, q
__device__ __forceinline__ void open_finish_stage(const OpenItem& it, uint64_t m, Fr* lds) {
    Fr loc[8], ci;
    const uint64_t base = (uint64_t)blockIdx.x * 2048;
    const Fr seed = p_ld(it.carries + blockIdx.x);
    horner_block(it.c, m, base, seed, it.zpow, 0, lds, loc, &ci);
    const Fr z = it.zpow[0];
    Fr h = ci;
    const uint64_t s0 = base + (uint64_t)threadIdx.x * 8;
    for (int e = 7; e >= 0; --e) {
        const uint64_t i = s0 + e;
        h = fe_add(loc[e], fe_mul(z, h));  // H_i
        if (i < m) {
            if (i == 0) p_st(it.y, h);
            else if (it.q) p_st(it.q + i - 1, h);
        }
    }
}

// ---- grand product: row j's term and the finish -------------------------------------------------------------------
// num_j = prod_i (w_ij + beta k_i x_j + gamma),  den_j = prod_i (w_ij + beta sigma_ij + gamma),  x_j = w^j: wire i's factors of
// both, multiplied into num and den (which start at one).  w, sigma: where w_ij and sigma_ij lie; kbeta = k_i * beta.
__device__ __forceinline__ void gp_term(const Fr* w, const Fr* sigma, const Fr& x, const Fr& beta, const Fr& gamma, const Fr& kbeta,
                                        Fr& num, Fr& den) {
    const Fr wg = fe_add(p_ld(w), gamma);
    num = fe_mul(num, fe_add(wg, fe_mul(kbeta, x)));
    den = fe_mul(den, fe_add(wg, fe_mul(beta, p_ld(sigma))));
}
// Z_j = N_j * S_j * S_0^-1 (N: exclusive prefix products of the numerators, S: suffix products of the denominators)
__device__ __forceinline__ Fr gp_finish(const Fr& nprefix, const Fr& dsuffix, const Fr& inv_total) {
    return fe_mul(fe_mul(nprefix, dsuffix), inv_total);
}

// ---- the quotient at one point x of the 4n coset (the formula is in quotient.hip's header) -------------------------
// Everything is the value AT the point: the wires, Z and Z(w x), the selectors q_l q_r q_o q_m q_c, the sigmas, L0;
// pi: where PI's value lies, null for the zero polynomial; bx = beta * x; zh_inv = 1 / (x^n - 1).
__device__ __forceinline__ Fr quotient_point(const Fr& wa, const Fr& wb, const Fr& wc, const Fr& z, const Fr& zw, const Fr* pi,
                                             const Fr (&sel)[5], const Fr (&sigma)[3], const Fr& l0, const Fr& bx, const Fr* k,
                                             bool k0_is_one, const Fr& beta, const Fr& gamma, const Fr& alpha, const Fr& alpha2,
                                             const Fr& zh_inv) {
    // gate constraint
    Fr line1 = fe_mul(sel[0], wa);
    line1 = fe_add(line1, fe_mul(sel[1], wb));
    line1 = fe_sub(line1, fe_mul(sel[2], wc));
    line1 = fe_add(line1, fe_mul(fe_mul(sel[3], wa), wb));
    line1 = fe_add(line1, sel[4]);
    if (pi) line1 = fe_add(line1, p_ld(pi));
    Fr l2 = fe_add(fe_add(wa, k0_is_one ? bx : fe_mul(k[0], bx)), gamma);
    l2 = fe_mul(l2, fe_add(fe_add(wb, fe_mul(k[1], bx)), gamma));
    l2 = fe_mul(l2, fe_add(fe_add(wc, fe_mul(k[2], bx)), gamma));
    l2 = fe_mul(l2, z);
    Fr l3 = fe_add(fe_add(wa, fe_mul(beta, sigma[0])), gamma);
    l3 = fe_mul(l3, fe_add(fe_add(wb, fe_mul(beta, sigma[1])), gamma));
    l3 = fe_mul(l3, fe_add(fe_add(wc, fe_mul(beta, sigma[2])), gamma));
    l3 = fe_mul(l3, zw);
    const Fr l4 = fe_mul(fe_sub(z, Fr::one()), l0);
    Fr t = fe_add(line1, fe_mul(alpha, fe_sub(l2, l3)));
    t = fe_add(t, fe_mul(alpha2, l4));
    return fe_mul(t, zh_inv);
}
}  // namespace ty
