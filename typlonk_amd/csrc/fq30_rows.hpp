// Fq with ONE LIMB PER LANE: limb i of a field element on lane i of a 16-lane row of the wavefront -- the arithmetic of the
// bucket reduction's last levels (msm_reduce.hip), where a handful of additions are left, each waits for the one before it,
// and the chip's lanes are idle.  fq30.hpp's multiplication is 351 dependent multiply-adds on one lane; here it is 13 steps
// of ~10 wave-instructions, four of them (one per row of the wavefront) at once.
//
// Same field, same Montgomery domain (R = 2^390), same modulus digits and the same packed 12-word memory form as fq30.hpp:
// what either form stores the other reads.
//
// Representation.  x = sum l[i] 2^(30 i), i = 0..12, on lanes 0..12 of the row; lanes 13..15 hold 0.  Between operations a
// limb is LOOSE: 0 <= l[i] <= FQR_LOOSE = 2^30 + 3, so an operation ends with ONE carry hand-over (fqr_norm: every lane keeps
// its low 30 bits and takes the bits above from the lane below) and not with a 13-step ripple.  Values obey the bound
// contracts of fq30.hpp / g1.hpp (units of p); a limb vector is turned into the unique digits only where they are needed:
// before an exact zero test and before a store (fqr_full_norm).
//
// Column bounds of the multiplication.  Step i adds a_i b_j and m p_j to the 64-bit accumulator of lane j, then every lane
// keeps the bits above 30 and takes the low 30 bits of the lane above (a division by 2^30; lane 0's low bits are zero by the
// choice of m).  With limbs <= 2^30 + 3 and m, p_j < 2^30 a step adds at most (2^30 + 3)^2 + (2^30 - 1)^2 = 2^61 + 4 * 2^30 + 10
// to an accumulator that enters it below C = 3 * 2^30 + 8, and leaves ((C + 2^61 + 4 * 2^30 + 10) >> 30) + 2^30 - 1 =
// 3 * 2^30 + 6 < C: an accumulator never exceeds 2^62 inside a step nor C < 2^32 between steps, whatever the 13 products and
// 13 reduction products before it were.  The last hand-over turns limbs < 2^32 into limbs <= 2^30 - 1 + 3.
//
// The arithmetic is written once, over a small "wave of four rows" abstraction W:
//     W::U32, W::U64, W::Mask      a value per lane
//     W::limb(), W::role()         lane index in the row, 0..15, and the row, 0..3
//     W::bcast(x, k)               lane k of the own row, on every lane of the row
//     W::up1(x) / W::down1(x)      the lane below / above in the row (0 shifted in at the row's end)
//     W::xrow(x, m)                the same lane of row (role ^ m)
//     W::mad, W::lo, W::shr30_add  the 64-bit accumulator
//     W::any(m), W::row_all(m)     over the wavefront / the own row
//     W::load2, W::store           per-lane addressed words
// RowsDev implements it with DPP moves and __shfl, RowsHost with arrays of 64: the host compiles and runs the same text
// (tests/cpp/fq30_rows_host.cpp).
#pragma once
#include "g1.hpp"

namespace ty {

constexpr uint32_t FQR_LOOSE = (1u << 30) + 3u;

// ---- the wave abstraction -------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
struct RowsDev {
    using U32 = uint32_t;
    using U64 = uint64_t;
    using Mask = bool;
    static __device__ __forceinline__ U32 limb() { return threadIdx.x & 15u; }
    static __device__ __forceinline__ U32 role() { return (threadIdx.x >> 4) & 3u; }
    static __device__ __forceinline__ U32 splat(uint32_t v) { return v; }
    // row_newbcast:k (DPP control 0x150 + k)
    static __device__ __forceinline__ U32 bcast(U32 x, int k) {
    // (every lane has a source, so no value for lanes without one is set up: __builtin_amdgcn_mov_dpp)
#define FQR_BC(K) case K: return (U32)__builtin_amdgcn_mov_dpp((int)x, 0x150 + K, 0xf, 0xf, false)
        switch (k) {
            FQR_BC(0); FQR_BC(1); FQR_BC(2); FQR_BC(3); FQR_BC(4); FQR_BC(5); FQR_BC(6); FQR_BC(7);
            FQR_BC(8); FQR_BC(9); FQR_BC(10); FQR_BC(11); FQR_BC(12); FQR_BC(13); FQR_BC(14);
            default: FQR_BC(15);
        }
#undef FQR_BC
    }
    // row_shr:1 / row_shl:1, bound_ctrl: the lane without a source reads 0
    static __device__ __forceinline__ U32 up1(U32 x) { return (U32)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, true); }
    static __device__ __forceinline__ U32 down1(U32 x) { return (U32)__builtin_amdgcn_update_dpp(0, (int)x, 0x101, 0xf, 0xf, true); }
    static __device__ __forceinline__ U32 xrow(U32 x, int m) { return (U32)__shfl_xor((int)x, m << 4); }
    static __device__ __forceinline__ U64 zero64() { return 0; }
    static __device__ __forceinline__ U64 mad(U32 a, U32 b, U64 acc) { return acc + (uint64_t)a * b; }
    static __device__ __forceinline__ U32 lo(U64 a) { return (U32)a; }
    static __device__ __forceinline__ U64 shr30_add(U64 a, U32 x) { return (a >> 30) + x; }
    static __device__ __forceinline__ U32 sel(Mask c, U32 a, U32 b) { return c ? a : b; }
    static __device__ __forceinline__ bool any(Mask m) { return __any((int)m) != 0; }
    static __device__ __forceinline__ Mask row_all(Mask m) {
        const uint64_t b = __ballot((int)m);
        return ((b >> (threadIdx.x & 48u)) & 0xffffu) == 0xffffu;
    }
    static __device__ __forceinline__ U32 load2(const uint32_t* p0, const uint32_t* p1, Mask second, U32 idx) {
        return (second ? p1 : p0)[idx];
    }
    static __device__ __forceinline__ void store(uint32_t* p, U32 idx, U32 v, Mask m) {
        if (m) p[idx] = v;
    }
    // a per-lane constant from a table of 16
    static __device__ __forceinline__ U32 lane_table(const uint32_t (&t)[16]) {
        U32 r = 0;
        const U32 l = limb();
#pragma unroll
        for (int i = 0; i < 13; ++i) r = l == (U32)i ? t[i] : r;
        return r;
    }
};
#endif
#if !defined(__HIP_DEVICE_COMPILE__)
template <class T>
struct HV {
    T l[64];
};
#define FQR_HV_BIN(OP)                                                        \
    template <class T>                                                        \
    inline HV<T> operator OP(const HV<T>& a, const HV<T>& b) {                \
        HV<T> r;                                                              \
        for (int i = 0; i < 64; ++i) r.l[i] = (T)(a.l[i] OP b.l[i]);          \
        return r;                                                             \
    }                                                                         \
    template <class T>                                                        \
    inline HV<T> operator OP(const HV<T>& a, uint32_t b) {                    \
        HV<T> r;                                                              \
        for (int i = 0; i < 64; ++i) r.l[i] = (T)(a.l[i] OP (T)b);            \
        return r;                                                             \
    }
FQR_HV_BIN(+)
FQR_HV_BIN(-)
FQR_HV_BIN(*)
FQR_HV_BIN(&)
FQR_HV_BIN(|)
#undef FQR_HV_BIN
// shifts: a count of 32 or more never reaches the hardware shifter on the device path either (fqr_load guards it)
inline HV<uint32_t> operator>>(const HV<uint32_t>& a, const HV<uint32_t>& n) {
    HV<uint32_t> r;
    for (int i = 0; i < 64; ++i) r.l[i] = a.l[i] >> (n.l[i] & 31u);
    return r;
}
inline HV<uint32_t> operator<<(const HV<uint32_t>& a, const HV<uint32_t>& n) {
    HV<uint32_t> r;
    for (int i = 0; i < 64; ++i) r.l[i] = a.l[i] << (n.l[i] & 31u);
    return r;
}
inline HV<uint32_t> operator>>(const HV<uint32_t>& a, int n) {
    HV<uint32_t> r;
    for (int i = 0; i < 64; ++i) r.l[i] = a.l[i] >> n;
    return r;
}
#define FQR_HV_CMP(OP)                                                        \
    inline HV<bool> operator OP(const HV<uint32_t>& a, const HV<uint32_t>& b) { \
        HV<bool> r;                                                           \
        for (int i = 0; i < 64; ++i) r.l[i] = a.l[i] OP b.l[i];               \
        return r;                                                             \
    }                                                                         \
    inline HV<bool> operator OP(const HV<uint32_t>& a, uint32_t b) {          \
        HV<bool> r;                                                           \
        for (int i = 0; i < 64; ++i) r.l[i] = a.l[i] OP b;                    \
        return r;                                                             \
    }
FQR_HV_CMP(==)
FQR_HV_CMP(!=)
FQR_HV_CMP(<)
#undef FQR_HV_CMP
inline HV<bool> operator&&(const HV<bool>& a, const HV<bool>& b) {
    HV<bool> r;
    for (int i = 0; i < 64; ++i) r.l[i] = a.l[i] && b.l[i];
    return r;
}
inline HV<bool> operator||(const HV<bool>& a, const HV<bool>& b) {
    HV<bool> r;
    for (int i = 0; i < 64; ++i) r.l[i] = a.l[i] || b.l[i];
    return r;
}
inline HV<bool> operator!(const HV<bool>& a) {
    HV<bool> r;
    for (int i = 0; i < 64; ++i) r.l[i] = !a.l[i];
    return r;
}

struct RowsHost {
    using U32 = HV<uint32_t>;
    using U64 = HV<uint64_t>;
    using Mask = HV<bool>;
    static U32 limb() {
        U32 r;
        for (int i = 0; i < 64; ++i) r.l[i] = (uint32_t)i & 15u;
        return r;
    }
    static U32 role() {
        U32 r;
        for (int i = 0; i < 64; ++i) r.l[i] = (uint32_t)i >> 4;
        return r;
    }
    static U32 splat(uint32_t v) {
        U32 r;
        for (int i = 0; i < 64; ++i) r.l[i] = v;
        return r;
    }
    static U32 bcast(const U32& x, int k) {
        U32 r;
        for (int i = 0; i < 64; ++i) r.l[i] = x.l[(i & 48) | k];
        return r;
    }
    static U32 up1(const U32& x) {
        U32 r;
        for (int i = 0; i < 64; ++i) r.l[i] = (i & 15) ? x.l[i - 1] : 0u;
        return r;
    }
    static U32 down1(const U32& x) {
        U32 r;
        for (int i = 0; i < 64; ++i) r.l[i] = (i & 15) != 15 ? x.l[i + 1] : 0u;
        return r;
    }
    static U32 xrow(const U32& x, int m) {
        U32 r;
        for (int i = 0; i < 64; ++i) r.l[i] = x.l[i ^ (m << 4)];
        return r;
    }
    static U64 zero64() {
        U64 r;
        for (int i = 0; i < 64; ++i) r.l[i] = 0;
        return r;
    }
    static U64 mad(const U32& a, const U32& b, const U64& acc) {
        U64 r;
        for (int i = 0; i < 64; ++i) {
            const uint64_t t = (uint64_t)a.l[i] * b.l[i];
            r.l[i] = acc.l[i] + t;
            if (r.l[i] < t) overflow() = true;   // the column bound of the header, checked in every host run
        }
        return r;
    }
    static bool& overflow() {
        static bool f = false;
        return f;
    }
    static U32 lo(const U64& a) {
        U32 r;
        for (int i = 0; i < 64; ++i) r.l[i] = (uint32_t)a.l[i];
        return r;
    }
    static U64 shr30_add(const U64& a, const U32& x) {
        U64 r;
        for (int i = 0; i < 64; ++i) r.l[i] = (a.l[i] >> 30) + x.l[i];
        return r;
    }
    static U32 sel(const Mask& c, const U32& a, const U32& b) {
        U32 r;
        for (int i = 0; i < 64; ++i) r.l[i] = c.l[i] ? a.l[i] : b.l[i];
        return r;
    }
    static bool any(const Mask& m) {
        for (int i = 0; i < 64; ++i)
            if (m.l[i]) return true;
        return false;
    }
    static Mask row_all(const Mask& m) {
        Mask r;
        for (int row = 0; row < 4; ++row) {
            bool a = true;
            for (int i = 0; i < 16; ++i) a = a && m.l[row * 16 + i];
            for (int i = 0; i < 16; ++i) r.l[row * 16 + i] = a;
        }
        return r;
    }
    static U32 load2(const uint32_t* p0, const uint32_t* p1, const Mask& second, const U32& idx) {
        U32 r;
        for (int i = 0; i < 64; ++i) r.l[i] = (second.l[i] ? p1 : p0)[idx.l[i]];
        return r;
    }
    static void store(uint32_t* p, const U32& idx, const U32& v, const Mask& m) {
        for (int i = 0; i < 64; ++i)
            if (m.l[i]) p[idx.l[i]] = v.l[i];
    }
    static U32 lane_table(const uint32_t (&t)[16]) {
        U32 r;
        for (int i = 0; i < 64; ++i) r.l[i] = t[i & 15];
        return r;
    }
};
#endif

// ---- constants per lane -----------------------------------------------------------------------------------------------------
// the digits of p
template <class W>
TY_HD typename W::U32 fqr_p() {
    const uint32_t t[16] = {fq30_kp(1, 0), fq30_kp(1, 1), fq30_kp(1, 2), fq30_kp(1, 3), fq30_kp(1, 4), fq30_kp(1, 5), fq30_kp(1, 6),
                            fq30_kp(1, 7), fq30_kp(1, 8), fq30_kp(1, 9), fq30_kp(1, 10), fq30_kp(1, 11), fq30_kp(1, 12), 0, 0, 0};
    return W::lane_table(t);
}
// K p with 2^30 lent from every limb to the one below: d_0 + 2^30, d_j + 2^30 - 1 (0 < j < 12), d_12 - 1 -- the same value,
// and a + (this) - b is >= 0 in EVERY lane for loose a, b (d_j >= 4 for j < 12, checked below), so a subtraction needs no
// signed limbs.
TY_HD constexpr uint32_t fqr_kp_lent(int k, int j) {
    return j == 0 ? fq30_kp(k, 0) + (1u << 30) : j < 12 ? fq30_kp(k, j) + (1u << 30) - 1u : fq30_kp(k, 12) - 1u;
}
TY_HD constexpr bool fqr_kp_digits_ok() {
    for (int k = 1; k <= 8; ++k) {
        for (int j = 0; j < 12; ++j)
            if (fq30_kp(k, j) < 4u) return false;
        if (fq30_kp(k, 12) < 1u) return false;
    }
    return true;
}
static_assert(fqr_kp_digits_ok(), "a lent digit of K p could go negative against a loose limb");
template <class W, int K>
TY_HD typename W::U32 fqr_kp_lent_lanes() {
    const uint32_t t[16] = {fqr_kp_lent(K, 0), fqr_kp_lent(K, 1), fqr_kp_lent(K, 2), fqr_kp_lent(K, 3), fqr_kp_lent(K, 4),
                            fqr_kp_lent(K, 5), fqr_kp_lent(K, 6), fqr_kp_lent(K, 7), fqr_kp_lent(K, 8), fqr_kp_lent(K, 9),
                            fqr_kp_lent(K, 10), fqr_kp_lent(K, 11), fqr_kp_lent(K, 12), 0, 0, 0};
    return W::lane_table(t);
}

// ---- carries ------------------------------------------------------------------------------------------------------------------
// one hand-over: limbs < 2^32 -> limbs <= 2^30 - 1 + 3 = FQR_LOOSE, same value (lane 12 must hold no carry: value < 2^390)
template <class W>
TY_HD typename W::U32 fqr_norm(const typename W::U32& s) {
    return (s & FQ30_MASK) + W::up1(s >> 30);
}
// the unique digits (limbs < 2^30) of a value < 2^390: hand-overs until no lane of the wavefront holds a carry (one or two
// as a rule; a carry moves one lane per round, so 14 rounds settle any input)
template <class W>
TY_HD typename W::U32 fqr_full_norm(typename W::U32 s) {
    for (int it = 0; it < 14; ++it) {
        const typename W::U32 c = s >> 30;
        if (!W::any(c != 0u)) break;
        s = (s & FQ30_MASK) + W::up1(c);
    }
    return s;
}

// ---- multiplication -----------------------------------------------------------------------------------------------------------
// a*b*2^-390 mod p.  Loose limbs in, loose limbs out.  Contract of fq30_mul: a*b < (2^390 - p) 2^390, result < p + a*b / 2^390,
// i.e. < (1 + A*B/630) p for a < A p, b < B p.  Column bounds: the header's.
template <class W>
TY_HD typename W::U32 fqr_mul(const typename W::U32& a, const typename W::U32& b) {
    const typename W::U32 p = fqr_p<W>();
    typename W::U64 acc = W::zero64();
#pragma unroll
    for (int i = 0; i < 13; ++i) {
        acc = W::mad(W::bcast(a, i), b, acc);
        const typename W::U32 m = (W::lo(acc) * FQ30_NINV) & FQ30_MASK;   // lane 0's is the step's reduction digit
        acc = W::mad(W::bcast(m, 0), p, acc);
        acc = W::shr30_add(acc, W::down1(W::lo(acc)) & FQ30_MASK);
    }
    return fqr_norm<W>(W::lo(acc));
}

// ---- lazy additive operations (no modular reduction; callers track the value bounds, as in fq30.hpp) ---------------------------
// a + b; value < 2^390
template <class W>
TY_HD typename W::U32 fqr_add_lazy(const typename W::U32& a, const typename W::U32& b) {
    return fqr_norm<W>(a + b);                                            // <= 2^31 + 6 per lane
}
// K a, K = 2 or 3
template <class W, int K>
TY_HD typename W::U32 fqr_mulk_lazy(const typename W::U32& a) {
    return fqr_norm<W>(a * (uint32_t)K);                                  // <= 3 * 2^30 + 9 per lane
}
// a - b + K p.  Requires b <= K p - 2^361 (so that the top lane stays >= 0 with the lent digits) and a + K p < 2^390.
// Per lane: a_j + (d_j + 2^30) - b_j <= 2^30 + 3 + 2^30 - 1 + 2^30 < 2^32.
template <class W, int K>
TY_HD typename W::U32 fqr_sub_lazy(const typename W::U32& a, const typename W::U32& b) {
    return fqr_norm<W>(a + fqr_kp_lent_lanes<W, K>() - b);
}
// a - b - c + K p.  Requires b + c <= K p - 2^361.
template <class W, int K>
TY_HD typename W::U32 fqr_sub2_lazy(const typename W::U32& a, const typename W::U32& b, const typename W::U32& c) {
    return fqr_sub_lazy<W, K>(a, fqr_add_lazy<W>(b, c));
}
template <class W>
TY_HD typename W::U32 fqr_select(const typename W::Mask& c, const typename W::U32& a, const typename W::U32& b) {
    return W::sel(c, a, b);
}
// a == 0 mod p, exactly, for a value < 2p: the same answer on every lane of the row
template <class W>
TY_HD typename W::Mask fqr_is_zero_mod(const typename W::U32& a) {
    const typename W::U32 d = fqr_full_norm<W>(a);
    return W::row_all(d == 0u) || W::row_all(d == fqr_p<W>());
}
// the cheap form of the same test: "this value < 2p may be 0 mod p", read off the lowest limb alone (a loose limb 0 is
// congruent to the value mod 2^30).  True on lane 0 of a row whose value is 0 or p; true by accident once in 2^29.
template <class W>
TY_HD typename W::Mask fqr_maybe_zero_mod(const typename W::U32& a) {
    const typename W::U32 low = a & FQ30_MASK;
    return (W::limb() == 0u) && (low == 0u || low == fq30_kp(1, 0));
}

// ---- packed 12 x 32-bit memory form (fq30_pack / fq30_unpack) -------------------------------------------------------------------
// limb i of the packed words w[0..11], i = 0..15 (0 above 12): bits 30 i .. 30 i + 29 lie in words i - 1 and i
TY_HD uint32_t fqr_limb_of_words(const uint32_t* w, uint32_t i) {
    if (i > 12u) return 0u;
    const uint32_t cur = i < 12u ? w[i] : 0u;
    if (i == 0u) return cur & FQ30_MASK;
    return ((w[i - 1] >> (32u - 2u * i)) | (cur << (2u * i))) & FQ30_MASK;
}
// the row form of a packed element: lane i reads word i (lanes 0..11) and builds its limb from it and the word below
template <class W>
TY_HD typename W::U32 fqr_load(const uint32_t* w) {
    const typename W::U32 i = W::limb();
    const typename W::Mask has = i < 12u;
    const typename W::U32 cur = W::sel(has, W::load2(w, w, has, W::sel(has, i, W::splat(0))), W::splat(0));
    const typename W::U32 below = W::up1(cur);
    const typename W::U32 hi = W::sel(i == 0u, W::splat(0), below >> ((W::splat(32) - i * 2u) & 31u));
    return W::sel(i < 13u, (hi | (cur << (i * 2u))) & FQ30_MASK, W::splat(0));
}
// normalise fully and store: word j = digits j and j + 1 (value < 2^384).  All four rows store their own element:
// row r writes w + 12 r.
template <class W>
TY_HD void fqr_store_rows(uint32_t* w, const typename W::U32& a) {
    const typename W::U32 d = fqr_full_norm<W>(a);
    const typename W::U32 j = W::limb();
    const typename W::U32 word = (d >> (j * 2u)) | (W::down1(d) << (W::splat(30) - j * 2u));
    W::store(w, W::role() * 12u + j, word, j < 12u);
}

// ---- one XYZZ addition per wavefront --------------------------------------------------------------------------------------------
// A point in the "limb layout": 64 words, X, Y, ZZ, ZZZ as 16 lanes each, limbs loose (stored invariants of g1.hpp: X < 5.1,
// Y < 3.2, ZZ, ZZZ < 1.1 in units of p).
constexpr uint32_t FQR_POINT_WORDS = 64;

// the digits of a limb-layout element
TY_HD Fq30 fqr_to_fq30(const uint32_t* l) {
    Fq30 r;
    uint32_t c = 0;
    for (int i = 0; i < 13; ++i) {
        const uint32_t s = l[i] + c;
        r.v[i] = s & FQ30_MASK;
        c = s >> 30;
    }
    return r;
}
TY_HD G1Xyzz fqr_to_xyzz(const uint32_t* pt) {
    G1Xyzz r;
    r.x = fqr_to_fq30(pt);
    r.y = fqr_to_fq30(pt + 16);
    r.zz = fqr_to_fq30(pt + 32);
    r.zzz = fqr_to_fq30(pt + 48);
    return r;
}

// out = A + B (add-2008-s), the four rows in the roles q0..q3 of butterfly_add4's four rounds (msm_common.hpp):
//   round 1   q0: U1 = X_A ZZ_B    q1: S1 = Y_A ZZZ_B    q2: U2 = X_B ZZ_A     q3: S2 = Y_B ZZZ_A
//   round 2   q0: ZZ12             q1: ZZZ12             q2: PP = P^2          q3: RR = R^2       (P = U2 - U1, R = S2 - S1)
//   round 3   q0: Q = U1 PP        q1: --                q2: PPP = P PP        q3: --
//   round 4   q0: ZZ3 = ZZ12 PP    q1: R (Q - X3)        q2: ZZZ3 = ZZZ12 PPP  q3: S1 PPP
// A row exchange is one cross-lane move.  Bounds: g1_add's.  An identity operand, equal points and opposite points are seen
// by the cheap test on the lowest limbs of ZZ_A, ZZ_B and PP (each < 2p); then -- for the whole wavefront, which holds this
// one addition -- the operands are converted and g1_add settles the case, exactly as for one-thread-per-point callers.
// `out` must not overlap A or B.  Returns true when the slow path ran (tests).
template <class W>
TY_HD bool g1_add_rows(const uint32_t* A, const uint32_t* B, uint32_t* out) {
    using U32 = typename W::U32;
    using Mask = typename W::Mask;
    const U32 li = W::limb(), role = W::role();
    const Mask odd = (role & 1u) != 0u, bside = (role & 2u) != 0u;
    const U32 zoff = W::sel(odd, W::splat(48), W::splat(32)) + li;
    const U32 own = W::load2(A, B, bside, W::sel(odd, W::splat(16), W::splat(0)) + li);   // X_A | Y_A | X_B | Y_B
    const U32 oz = W::load2(A, B, !bside, zoff);                                          // ZZ_B | ZZZ_B | ZZ_A | ZZZ_A
    const U32 mz = W::load2(A, B, bside, zoff);                                           // ZZ_A | ZZZ_A | ZZ_B | ZZZ_B
    // round 1
    const U32 m1 = fqr_mul<W>(own, oz);                                                   // U1 | S1 | U2 | S2   < 1.01
    // round 2
    const U32 x1 = W::xrow(m1, 2);                                                        // U2 | S2 | U1 | S1
    const U32 d = fqr_sub_lazy<W, 2>(W::sel(bside, m1, x1), W::sel(bside, x1, m1));       // P (even rows) | R (odd rows)  < 3.1
    const U32 m2 = fqr_mul<W>(W::sel(bside, d, mz), W::sel(bside, d, oz));                // ZZ12 | ZZZ12 | PP | RR   < 1.02
    const Mask maybe = (!odd && fqr_maybe_zero_mod<W>(mz)) || (bside && !odd && fqr_maybe_zero_mod<W>(m2));
    if (W::any(maybe)) {
        const G1Xyzz s = g1_add(fqr_to_xyzz(A), fqr_to_xyzz(B));
        const uint32_t tx[16] = {s.x.v[0], s.x.v[1], s.x.v[2], s.x.v[3], s.x.v[4], s.x.v[5], s.x.v[6], s.x.v[7], s.x.v[8], s.x.v[9],
                                 s.x.v[10], s.x.v[11], s.x.v[12], 0, 0, 0};
        const uint32_t ty[16] = {s.y.v[0], s.y.v[1], s.y.v[2], s.y.v[3], s.y.v[4], s.y.v[5], s.y.v[6], s.y.v[7], s.y.v[8], s.y.v[9],
                                 s.y.v[10], s.y.v[11], s.y.v[12], 0, 0, 0};
        const uint32_t tz[16] = {s.zz.v[0], s.zz.v[1], s.zz.v[2], s.zz.v[3], s.zz.v[4], s.zz.v[5], s.zz.v[6], s.zz.v[7], s.zz.v[8],
                                 s.zz.v[9], s.zz.v[10], s.zz.v[11], s.zz.v[12], 0, 0, 0};
        const uint32_t tw[16] = {s.zzz.v[0], s.zzz.v[1], s.zzz.v[2], s.zzz.v[3], s.zzz.v[4], s.zzz.v[5], s.zzz.v[6], s.zzz.v[7],
                                 s.zzz.v[8], s.zzz.v[9], s.zzz.v[10], s.zzz.v[11], s.zzz.v[12], 0, 0, 0};
        // row r writes coordinate r
        const U32 v = W::sel(bside, W::sel(odd, W::lane_table(tw), W::lane_table(tz)), W::sel(odd, W::lane_table(ty), W::lane_table(tx)));
        W::store(out, role * 16u + li, v, li < 16u);
        return true;
    }
    // round 3
    const U32 x2 = W::xrow(m2, 2);                                                        // PP | RR | ZZ12 | ZZZ12
    const U32 m3 = fqr_mul<W>(W::sel(bside, d, m1), W::sel(bside, m2, x2));               // Q | -- | PPP | --   < 1.01
    // round 4
    const U32 qa = W::xrow(m3, 1);                                                        // -- | Q | -- | PPP
    const U32 qb = W::xrow(m3, 3);                                                        // -- | PPP | -- | Q
    const U32 qc = W::xrow(m2, 3);                                                        // (q2 takes ZZZ12 from q1)
    const U32 x3 = fqr_sub2_lazy<W, 4>(x2, qb, fqr_mulk_lazy<W, 2>(qa));                  // q1: RR - PPP - 2Q  < 5.1
    const U32 t = fqr_sub_lazy<W, 6>(qa, x3);                                             // q1: Q - X3  < 7.1
    // q0: ZZ12 PP = m2 x2;  q1: R T = d t;  q2: ZZZ12 PPP = qc m3;  q3: S1 PPP = x1 qa
    const U32 opa = W::sel(bside, W::sel(odd, x1, qc), W::sel(odd, d, m2));
    const U32 opb = W::sel(bside, W::sel(odd, qa, m3), W::sel(odd, t, x2));
    const U32 m4 = fqr_mul<W>(opa, opb);                                                  // ZZ3 | R T | ZZZ3 | S1 PPP   < 1.04
    const U32 y3 = fqr_sub_lazy<W, 2>(m4, W::xrow(m4, 2));                                // q1: R T - S1 PPP  < 3.1
    W::store(out, li, x3, role == 1u);
    W::store(out, li + 16u, y3, role == 1u);
    W::store(out, li + 32u, m4, role == 0u);
    W::store(out, li + 48u, m4, role == 2u);
    return false;
}

}  // namespace ty
