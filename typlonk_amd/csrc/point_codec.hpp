// Compressed G1 points: the 48-byte ZCash / IETF BLS12-381 form (include/typlonk.h, "wire format").
//
// One source for the host path (ctx = NULL) and the kernels of point_codec.hip: decoding a point is one Fq square root
// (a 379-bit power ladder, 606 products) and one subgroup test (128 doublings + 10 additions, ~1150 products).
//
//   byte 0, bit 7  compressed (must be set)      bit 6  infinity (every other bit must then be 0)
//           bit 5  y > (p - 1) / 2               the remaining 381 bits: x, big-endian, canonical (< p)
//
// Subgroup test: phi(P) = -[z^2] P with phi(x, y) = (beta x, y), z = 0xd201000000010000 and beta the cube root of unity for
// which the identity holds on G.  -z^2 is a root of X^2 + X + 1 mod r (z^4 - z^2 + 1 = r), i.e. the eigenvalue of phi on
// the r-torsion of E(Fq), so every point of G passes; that no other point of E(Fq) does is M. Scott, "A note on group
// membership tests for G1, G2 and GT on BLS pairing-friendly curves" (ePrint 2021/1130), section 4.  The tests probe it with
// points of cofactor order and sums of such points with multiples of G against a plain [r]P.
#pragma once
#include "g1.hpp"

namespace ty {

// reject classes (TYPLONK_POINT_* of include/typlonk.h; the first failing check in this order decides)
constexpr uint32_t PC_OK = 0, PC_ENCODING = 1, PC_X_RANGE = 2, PC_NOT_ON_CURVE = 3, PC_NOT_IN_SUBGROUP = 4;

// R^2 mod p (R = 2^390): one Montgomery product with it brings a canonical integer into the internal form
TY_HD constexpr uint32_t pc_r2_limb(int i) {
    constexpr uint32_t t[13] = {0x0510070fu, 0x3b19070du, 0x0132243au, 0x299bb0e8u, 0x3507af6eu, 0x3b81ec77u, 0x21b145efu,
                                0x0a487bb4u, 0x370a4144u, 0x05dcb4cbu, 0x18c97900u, 0x3812b364u, 0x000f696eu};
    return t[i];
}
// beta = 0x5f19672fdf76ce51ba69c6076a0f77eaddb3a93be6f89688de17d813620a00022e01fffffffefffe in the internal form
TY_HD constexpr uint32_t pc_beta_limb(int i) {
    constexpr uint32_t t[13] = {0x229d39fcu, 0x11661b79u, 0x3a68a8f8u, 0x09dabbd8u, 0x12744b7eu, 0x22bc97d4u, 0x3c5ccd3eu,
                                0x1cf87540u, 0x0197e4f4u, 0x3433d1ecu, 0x0d20861fu, 0x33953662u, 0x000edc53u};
    return t[i];
}
// (p + 1) / 4 as 32-bit words, little endian (379 bits)
TY_HD constexpr uint32_t pc_sqrt_exp(int i) {
    constexpr uint32_t t[12] = {0xffffeaabu, 0xee7fbfffu, 0xac54ffffu, 0x07aaffffu, 0x3dac3d89u, 0xd9cc34a8u,
                                0x3ce144afu, 0xd91dd2e1u, 0x90d2eb35u, 0x92c6e9edu, 0x8e5ff9a6u, 0x0680447au};
    return t[i];
}
constexpr uint64_t PC_Z = 0xd201000000010000ull;

// a >= p for a normalised a
TY_HD bool pc_geq_p(const Fq30& a) {
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < 13; ++i) c = ((int32_t)a.v[i] + c - (int32_t)fq30_kp(1, i)) >> 30;
    return c >= 0;
}
// a == b mod p; a < 1.1 p, b < 6 p
TY_HD bool pc_eq_mod(const Fq30& a, const Fq30& b) { return fq30_is_zero_exact(fq30_canon(fq30_sub_lazy<6>(a, b))); }
// internal form -> canonical integer digits
TY_HD Fq30 pc_from_mont(const Fq30& a) {
    Fq30 one = fq30_zero();
    one.v[0] = 1;
    return fq30_canon(fq30_mul(a, one));
}
// canonical integer y > (p - 1) / 2  <=>  2 y >= p  (p is odd)
TY_HD bool pc_is_high(const Fq30& y_int) { return pc_geq_p(fq30_mulk_lazy<2>(y_int)); }

// a^((p + 1) / 4): the square root of a when a is a square (p = 3 mod 4).  a < 8p, result < 1.01 p.
TY_HD Fq30 pc_sqrt_candidate(const Fq30& a) {
    Fq30 acc = a;   // bit 378 of the exponent, the leading one
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int bit = 377; bit >= 0; --bit) {
        acc = fq30_sqr(acc);
        uint32_t word = 0;   // (a select over the constant words: no indexed private array, no scratch)
#pragma unroll
        for (int w = 0; w < 12; ++w) word = (bit >> 5) == w ? pc_sqrt_exp(w) : word;
        if ((word >> (bit & 31)) & 1u) acc = fq30_mul(acc, a);
    }
    return acc;
}

// [r] P = O for a finite curve point P = (x, y), canonical internal coordinates
TY_HD bool g1_in_subgroup(const Fq30& x, const Fq30& y) {
    // Q = [z] P (mixed additions), then Q2 = [z] Q
    G1Xyzz q = G1Xyzz::inf();
    g1_madd_xy(q, x, y);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int bit = 62; bit >= 0; --bit) {
        q = g1_dbl(q);
        if ((PC_Z >> bit) & 1ull) g1_madd_xy(q, x, y);
    }
    G1Xyzz q2 = q;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int bit = 62; bit >= 0; --bit) {
        q2 = g1_dbl(q2);
        if ((PC_Z >> bit) & 1ull) q2 = g1_add(q2, q);
    }
    if (q2.is_inf()) return false;   // phi(P) is finite
    // (beta x, y) == (X / ZZ, -Y / ZZZ)
    Fq30 beta;
#pragma unroll
    for (int i = 0; i < 13; ++i) beta.v[i] = pc_beta_limb(i);
    Fq30 bx, lx, ly;
    bx = fq30_mul(beta, x);                                            // < 1.01
    fq30_mul_pair(bx, q2.zz, fq30_neg_lazy<1>(y), q2.zzz, lx, ly);     // < 1.01 each
    return pc_eq_mod(lx, q2.x) && pc_eq_mod(ly, q2.y);                 // X < 5.1, Y < 3.2 <= 6
}

// The reject class of a stored record with canonical coordinates: PC_OK for an identity and for an element of the group of
// order r, else PC_NOT_ON_CURVE or PC_NOT_IN_SUBGROUP.  The body of srs_membership_kernel (srs_gen.hip) and of
// chunks_membership_kernel (verify_chunks.hip).
TY_HD uint32_t g1_record_class(const G1Affine& p) {
    if (p.is_inf()) return PC_OK;
    const Fq30 four = fq30_mulk_lazy<2>(fq30_mulk_lazy<2>(fq30_one()));                // < 4.1
    const Fq30 rhs = fq30_add_lazy(fq30_mul(fq30_sqr(p.x), p.x), four);                // x^3 + 4 < 5.2
    if (!pc_eq_mod(fq30_sqr(p.y), rhs)) return PC_NOT_ON_CURVE;
    return g1_in_subgroup(p.x, p.y) ? PC_OK : PC_NOT_IN_SUBGROUP;
}

// The 48 bytes as the twelve 32-bit words a little-endian load of them gives (raw[k] = bytes 4k .. 4k + 3) -> the point in
// the internal form, canonical, the identity as (0, 0).  A rejected encoding gives the identity and its class.
TY_HD uint32_t g1_decode(const uint32_t (&raw)[12], bool check_subgroup, G1Affine& out) {
    out = G1Affine::inf();
    uint32_t w[12];   // x as little-endian words
#pragma unroll
    for (int j = 0; j < 12; ++j) w[j] = __builtin_bswap32(raw[11 - j]);
    const uint32_t flags = w[11] >> 29;
    w[11] &= 0x1fffffffu;
    if (!(flags & 4u)) return PC_ENCODING;
    if (flags & 2u) {
        uint32_t any = flags & 1u;
#pragma unroll
        for (int j = 0; j < 12; ++j) any |= w[j];
        return any ? PC_ENCODING : PC_OK;
    }
    const Fq30 xi = fq30_unpack(w);
    if (pc_geq_p(xi)) return PC_X_RANGE;
    Fq30 r2;
#pragma unroll
    for (int i = 0; i < 13; ++i) r2.v[i] = pc_r2_limb(i);
    const Fq30 x = fq30_canon(fq30_mul(xi, r2));
    const Fq30 four = fq30_mulk_lazy<2>(fq30_mulk_lazy<2>(fq30_one()));        // < 4.1
    const Fq30 rhs = fq30_add_lazy(fq30_mul(fq30_sqr(x), x), four);            // x^3 + 4 < 5.2
    Fq30 y = fq30_canon(pc_sqrt_candidate(rhs));
    if (!pc_eq_mod(fq30_sqr(y), rhs)) return PC_NOT_ON_CURVE;
    if (pc_is_high(pc_from_mont(y)) != ((flags & 1u) != 0)) y = fq30_canon(fq30_neg_lazy<1>(y));
    if (check_subgroup && !g1_in_subgroup(x, y)) return PC_NOT_IN_SUBGROUP;
    out.x = x;
    out.y = y;
    return PC_OK;
}

// internal form (canonical; (0, 0) = identity) -> the 48 bytes as little-endian-loaded words
TY_HD void g1_encode(const G1Affine& p, uint32_t (&raw)[12]) {
    if (p.is_inf()) {
#pragma unroll
        for (int k = 0; k < 12; ++k) raw[k] = 0;
        raw[0] = 0xc0u;   // byte 0
        return;
    }
    uint32_t w[12];
    fq30_pack(pc_from_mont(p.x), w);
    w[11] |= 0x80000000u | (pc_is_high(pc_from_mont(p.y)) ? 0x20000000u : 0u);
#pragma unroll
    for (int k = 0; k < 12; ++k) raw[k] = __builtin_bswap32(w[11 - k]);
}

// the decoded point in the C ABI's form: 24 words (x then y, arkworks residues), the identity as (0, 1) with inf = 1
TY_HD uint32_t g1_decode_ark(const uint32_t (&raw)[12], bool check_subgroup, uint32_t (&xy)[24], uint8_t& inf) {
    G1Affine a;
    const uint32_t st = g1_decode(raw, check_subgroup, a);
    uint32_t w[12];
    if (a.is_inf()) {
#pragma unroll
        for (int i = 0; i < 12; ++i) xy[i] = 0;
        fq30_to_ark(fq30_one(), w);
        inf = 1;
    } else {
        fq30_to_ark(a.x, w);
#pragma unroll
        for (int i = 0; i < 12; ++i) xy[i] = w[i];
        fq30_to_ark(a.y, w);
        inf = 0;
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) xy[12 + i] = w[i];
    return st;
}

}  // namespace ty
