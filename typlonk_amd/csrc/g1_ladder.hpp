// The 255-step scalar multiplication of the set-up kernels, stated once for srs_gen.hip (the contribution) and g1_fft.hip (the
// group transform and the openings): a power in Fr, [k]P, and [k]P as a stored record.  Device code only.
#pragma once
#include "msm_common.hpp"

namespace ty {

// b^ex by the 64-step ladder of srs_generate_kernel
__device__ __forceinline__ Fr fr_pow_u64(const Fr& b, uint64_t ex) {
    Fr e = Fr::one();
#pragma unroll 1
    for (int bit = 63; bit >= 0; --bit) {
        e = fe_sqr(e);
        if ((ex >> bit) & 1) e = fe_mul(e, b);
    }
    return e;
}

// [k] p for a canonical k < 2^255 and an affine p: 255 steps of doubling and mixed addition, most significant bit first
__device__ __forceinline__ G1Xyzz g1_ladder(const Fr& k, const G1Affine& p) {
    G1Xyzz acc = G1Xyzz::inf();
#pragma unroll 1
    for (int bit = 254; bit >= 0; --bit) {
        acc = g1_dbl(acc);
        uint32_t word = 0;   // (a select over the eight words: no indexed private array, no scratch)
#pragma unroll
        for (int w = 0; w < 8; ++w) word = (bit >> 5) == w ? k.v[w] : word;
        if ((word >> (bit & 31)) & 1u) g1_madd(acc, p, false);
    }
    return acc;
}

// dst[o] = [k] src[i] as a canonical affine record, the body of srs_contribute_kernel and srs_g1_scale_kernel.  The base is
// whatever the record holds: g1_madd_xy's equal and opposite branches make the result [k]P by the group law for every curve
// point, those of small order included; k = 0 and an identity record both give the all-zero record (the ladder never leaves
// the identity).  A spare lane (live = false) runs along on a record of its wavefront's -- the inversion's exit test is
// wave-uniform -- and skips only the store.
__device__ __forceinline__ void g1_ladder_record(const Fr& k, const uint32_t* src, uint64_t i, uint32_t* dst, uint64_t o, bool live) {
    const G1Affine r = g1_to_affine(g1_ladder(k, ld_affine(src, i)));
    if (!live) return;
    uint32_t* q = dst + o * PT_WORDS;
    st_fq(q, r.x);
    st_fq(q + 12, r.y);
}

}  // namespace ty
