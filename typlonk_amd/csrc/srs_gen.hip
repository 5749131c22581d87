// Device-side SRS generation: g1[i] = [s^(start+i)] G, canonical affine -- the vector
// Srs::from_secret builds (/root/reference/kzg/src/srs.rs:15-24, 30-34), one thread per power.
// Setup-time only (not on the prove() path); it exists so that benchmarks and large parity tests
// can create 2^20..2^22-point SRS shards directly in HBM.
#include "launch.hpp"
#include "msm_common.hpp"
#include "point_codec.hpp"

namespace ty {

// ---- fixed-base comb for G ----------------------------------------------------------------------------------------------
// comb[w * 256 + j] = [j * 2^(8 w)] G, affine, w < 32, 1 <= j < 256 (entry 0 of a row is unused): a power of the secret
// then costs 32 mixed additions and one inversion instead of the 255 doublings + ~128 additions + 551-multiplication
// Fermat inversion of rounds 1-4 (69 ms per 2^20 points -> profiles/r05_*).  Built once per context (1 MiB).
constexpr uint32_t COMB_WINDOWS = 32, COMB_ROW = 256;

__device__ __forceinline__ void g1_generator(Fq30& gx, Fq30& gy) {
    // G1 generator in the internal form (x * 2^390 mod p as 30-bit digits)
    constexpr uint32_t x[13] = {0x14d1b01cu, 0x143790fdu, 0x34ffd633u, 0x1bc687f8u, 0x3e2228c0u, 0x04f86aa1u, 0x298df978u,
                                0x2e28c656u, 0x1b36e719u, 0x3ed397edu, 0x2f68adadu, 0x096840ceu, 0x00082ebcu};
    constexpr uint32_t y[13] = {0x39d1f18cu, 0x0d03d50cu, 0x10f63b65u, 0x3231b0b8u, 0x2e87afadu, 0x02eceb19u, 0x258480d0u,
                                0x31f25b61u, 0x08856e09u, 0x1fef8f3eu, 0x1a3501cbu, 0x1d6e0ad8u, 0x0016f1c9u};
#pragma unroll
    for (int i = 0; i < 13; ++i) {
        gx.v[i] = x[i];
        gy.v[i] = y[i];
    }
}

__global__ __launch_bounds__(64) void srs_comb_kernel(uint32_t* comb) {
    const uint32_t t = blockIdx.x * 64 + threadIdx.x;   // (w, j)
    const uint32_t w = t / COMB_ROW, j = t % COMB_ROW;
    if (w >= COMB_WINDOWS) return;
    G1Affine g;
    g1_generator(g.x, g.y);
    // B = 2^(8w) G, then j B by an 8-step double-and-add
    G1Jac b = G1Jac::from_affine(g);
    for (uint32_t d = 0; d < 8 * w; ++d) b = g1_jac_dbl(b);
    const G1Xyzz bx = g1_jac_to_xyzz(b);
    G1Xyzz acc = G1Xyzz::inf();
    for (int bit = 7; bit >= 0; --bit) {
        acc = g1_dbl(acc);
        if ((j >> bit) & 1) acc = g1_add(acc, bx);
    }
    const G1Affine r = g1_to_affine(acc);   // j = 0: the identity, (0, 0)
    uint32_t* p = comb + (uint64_t)t * PT_WORDS;
    st_fq(p, r.x);
    st_fq(p + 12, r.y);
}

struct SrsGenArgs {
    Fr s;
    uint64_t start, n;
    const uint32_t* comb;
    uint32_t* pts;
};

__global__ __launch_bounds__(64) void srs_generate_kernel(SrsGenArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    // (lanes past the end run along on the last power: the inversion's exit test is wave-uniform)
    const uint64_t ex = a.start + (i < a.n ? i : a.n - 1);
    // e = s^(start+i)
    Fr e = Fr::one();
    for (int b = 63; b >= 0; --b) {
        e = fe_sqr(e);
        if ((ex >> b) & 1) e = fe_mul(e, a.s);
    }
    const Fr k = fe_from_mont(e);
    G1Xyzz acc = G1Xyzz::inf();
    for (uint32_t w = 0; w < COMB_WINDOWS; ++w) {
        const uint32_t j = (k.v[w >> 2] >> (8 * (w & 3))) & 255u;
        if (j) {
            const G1Affine q = ld_affine(a.comb, (uint64_t)w * COMB_ROW + j);
            g1_madd_xy(acc, q.x, q.y);
        }
    }
    const G1Affine r = g1_to_affine(acc);
    if (i >= a.n) return;
    uint32_t* p = a.pts + i * PT_WORDS;
    st_fq(p, r.x);
    st_fq(p + 12, r.y);
}

// ---- fixed-base window tables -------------------------------------------------------------------------------------------
// Table t holds 2^(c*t) * P_i (affine, canonical) at point index t*len + i, table 0 being the SRS itself.  Setup-time
// only; it trades HBM capacity (T x the SRS) for the whole cross-window recombination of every later MSM over this SRS.
//
// One thread per base walks its column of T - 1 entries as ONE Jacobian doubling chain -- c doublings per entry, never
// normalised on the way -- parks (X_t, Y_t) in the entry's own slot and Z_t in a scratch vector, and keeps the running
// products Z_1 ... Z_(t-1) in the LDS; then one inversion (divsteps, fq30.hpp) of the full product and a walk back up
// the column (Montgomery's trick) turn every entry into its canonical affine form.  Per entry: c * 6.0 + 7
// multiplication times, and 1/(T-1) of an inversion, where rounds 1-4 paid c * 8.0 + 5 + a 551-multiplication Fermat
// ladder: 115 ms -> profiles/r05_* per 2^20-point SRS at c = 20.  Same points, bit for bit (canonical affine).
// LDS: (T - 1) x 13 words per thread, [t][limb][thread].
__global__ __launch_bounds__(64) void srs_tables_kernel(uint32_t* pts, uint32_t* zbuf, uint64_t len, uint32_t c, uint32_t T) {
    extern __shared__ uint32_t prefix[];
    const uint64_t i0 = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = i0 < len;
    const uint64_t i = live ? i0 : len - 1;            // spare lanes shadow the last base (wave-uniform inversion loop)
    const G1Affine p = ld_affine(pts, i);
    const bool inf = p.is_inf();
    G1Jac a;
    a.x = p.x;
    a.y = p.y;
    a.z = fq30_one();                                   // the identity walks along as a harmless non-point
    Fq30 run = fq30_one();
    uint32_t dead_from = inf ? 1u : T;                  // first table whose entry is the identity (T: none)
    for (uint32_t t = 1; t < T; ++t) {
        for (uint32_t d = 0; d < c; ++d) a = g1_jac_dbl(a);
        // a denominator that vanishes (an input that is not a point of odd order -- only typlonk_srs_load can bring one,
        // it does not validate) is taken out of the product; 2^k * identity = identity, so that entry AND every later one
        // of the column are the identity (the chain itself walks on from a harmless non-point)
        const bool zero = fq30_is_zero_mod(a.z);
        if (zero) {
            a.z = fq30_one();
            dead_from = min(dead_from, t);
        }
        if (live) {
            uint32_t* dst = pts + (t * len + i) * PT_WORDS;
            st_fq(dst, zero ? fq30_zero() : a.x);
            st_fq(dst + 12, zero ? fq30_zero() : a.y);
            st_fq(zbuf + ((uint64_t)(t - 1) * len + i) * 12, a.z);
        }
#pragma unroll
        for (int l = 0; l < 13; ++l) prefix[((t - 1) * 13 + l) * 64 + threadIdx.x] = run.v[l];
        run = fq30_mul(run, a.z);                       // < 1.01
    }
    Fq30 inv = fq30_inv(run);                           // 1 / (Z_1 ... Z_(T-1))
    if (!live) return;
    for (uint32_t t = T - 1; t >= 1; --t) {
        uint32_t* dst = pts + (t * len + i) * PT_WORDS;
        Fq30 before;
#pragma unroll
        for (int l = 0; l < 13; ++l) before.v[l] = prefix[((t - 1) * 13 + l) * 64 + threadIdx.x];
        const Fq30 z = ld_fq(zbuf + ((uint64_t)(t - 1) * len + i) * 12);
        const Fq30 zinv = fq30_mul(inv, before);        // 1 / Z_t
        inv = fq30_mul(inv, z);
        G1Jac e;
        e.x = ld_fq(dst);
        e.y = ld_fq(dst + 12);
        G1Affine r = g1_jac_to_affine_with(e, zinv);
        if (t >= dead_from) r = G1Affine::inf();
        st_fq(dst, r.x);
        st_fq(dst + 12, r.y);
    }
}
// scratch of the walk: one denominator (48 B) per entry of tables 1 .. T-1.  The LDS holds (T - 1) x 13 words per thread:
// 59.9 KiB for the largest table count the ABI accepts (c = 14: 19 tables), inside the 64 KiB a launch gets by default.
size_t srs_tables_scratch_bytes(uint64_t len, uint32_t T) { return T > 1 ? (size_t)(T - 1) * len * 48 : 0; }
static_assert((19 - 1) * 13 * 64 * 4 <= 64 * 1024, "the running products of the largest table count must fit the default LDS");
void launch_srs_tables(uint32_t* pts, uint32_t* zbuf, uint64_t len, uint32_t c, uint32_t T, hipStream_t s) {
    if (T <= 1 || len == 0) return;
    hipLaunchKernelGGL(srs_tables_kernel, dim3((unsigned)((len + 63) / 64)), dim3(64), (size_t)(T - 1) * 13 * 64 * 4, s, pts, zbuf, len, c, T);
}

// ---- self-test of the SIMT inversion (typlonk_selftest_fq_inv) --------------------------------------------------------------
// Every thread draws `per_thread` residues (xorshift; every 16th slot an edge value: 0, 1, 2, p - 1, p - 2, a one-limb
// value), lifts them by 0..7 multiples of p (the contract of fq30_inv: any normalised value < 8p), and compares
// fq30_inv_divsteps with the Fermat ladder a^(p-2) digit for digit after canonicalisation, plus x * x^-1 = 1.
// out[0] = mismatches, out[1] = largest number of 30-divstep rounds a call ran, out[2] = calls.
__global__ __launch_bounds__(64) void fq_inv_selftest_kernel(uint64_t seed, uint32_t per_thread, uint32_t* out) {
    const uint32_t tid = blockIdx.x * 64 + threadIdx.x;
    uint64_t st = (seed + tid) * 0x9E3779B97F4A7C15ull + 1;
    uint32_t bad = 0;
    int maxr = 0;
    for (uint32_t it = 0; it < per_thread; ++it) {
        Fq30 x;
#pragma unroll
        for (int i = 0; i < 13; ++i) {
            st ^= st << 13;
            st ^= st >> 7;
            st ^= st << 17;
            x.v[i] = (uint32_t)st & FQ30_MASK;
        }
        x.v[12] &= 0x000fffffu;   // < 2^380 < p
        const uint32_t cls = (it * 64u + threadIdx.x) & 255u;
        if (cls < 6) {
            const Fq30 keep = x;
            x = fq30_zero();
            if (cls == 1) x.v[0] = 1;
            if (cls == 2) x.v[0] = 2;
            if (cls == 3 || cls == 4) {
#pragma unroll
                for (int i = 0; i < 13; ++i) x.v[i] = fq30_kp(1, i);
                x.v[0] -= cls == 3 ? 1u : 2u;
            }
            if (cls == 5) x.v[0] = keep.v[0];
        }
        Fq30 xl = x;
        const uint32_t lift = (uint32_t)(st >> 40) & 7u;
        for (uint32_t l = 0; l < lift; ++l) {
            Fq30 pp;
#pragma unroll
            for (int i = 0; i < 13; ++i) pp.v[i] = fq30_kp(1, i);
            xl = fq30_add_lazy(xl, pp);
        }
        int rounds = 0;
        const Fq30 d = fq30_canon(fq30_inv_divsteps(xl, &rounds));
        const Fq30 f = fq30_canon(fq30_inv_fermat(x));
        bool ok = true;
#pragma unroll
        for (int i = 0; i < 13; ++i) ok = ok && d.v[i] == f.v[i];
        if (!fq30_is_zero_exact(x)) {
            const Fq30 one = fq30_canon(fq30_mul(xl, d)), r1 = fq30_one();
#pragma unroll
            for (int i = 0; i < 13; ++i) ok = ok && one.v[i] == r1.v[i];
        } else {
            ok = ok && fq30_is_zero_exact(d);
        }
        bad += ok ? 0u : 1u;
        maxr = rounds > maxr ? rounds : maxr;
    }
    if (bad) atomicAdd(&out[0], bad);
    atomicMax(&out[1], (uint32_t)maxr);
    atomicAdd(&out[2], per_thread);
}
void launch_fq_inv_selftest(uint64_t seed, uint32_t threads, uint32_t per_thread, uint32_t* out, hipStream_t st) {
    hipLaunchKernelGGL(fq_inv_selftest_kernel, dim3((threads + 63) / 64), dim3(64), 0, st, seed, per_thread, out);
}

void launch_srs_comb(uint32_t* comb, hipStream_t st) {
    hipLaunchKernelGGL(srs_comb_kernel, dim3(COMB_WINDOWS * COMB_ROW / 64), dim3(64), 0, st, comb);
}
size_t srs_comb_bytes() { return (size_t)COMB_WINDOWS * COMB_ROW * PT_WORDS * 4; }

void launch_srs_generate(const Fr& s, uint64_t start, uint64_t n, const uint32_t* comb, uint32_t* pts, hipStream_t st) {
    if (n == 0) return;
    SrsGenArgs a;
    a.s = s;
    a.start = start;
    a.n = n;
    a.comb = comb;
    a.pts = pts;
    hipLaunchKernelGGL(srs_generate_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, a);
}

// ---- typlonk_srs_check / typlonk_srs_contribute (srs_check.hip) -------------------------------------------------------------
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

// Membership of every record of an SRS entry, one thread per point: on y^2 = x^3 + 4 (else
// PC_NOT_ON_CURVE) and in the subgroup of order r (g1_in_subgroup, point_codec.hpp; else PC_NOT_IN_SUBGROUP).  An identity
// record passes.  out[0] <- min over the failing points of (index << 8 | class) (the caller sets it to all ones),
// out[1] += the number of failing points (one ballot per wavefront, one atomic add), out[2] <- 1 when record 0 is not the
// fixed generator word for word (the caller clears both).  No lane leaves before the ballot.
__global__ __launch_bounds__(64) void srs_membership_kernel(const uint32_t* pts, uint64_t n, unsigned long long* out) {
    const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = i < n;
    const G1Affine p = ld_affine(pts, live ? i : n - 1);
    uint32_t st = PC_OK;
    if (live && !p.is_inf()) {
        // (coordinates are canonical in every record: the generator, the decoder and the contribution write them so, and
        // typlonk_srs_load reduces what it is given -- fq30_from_ark, msm_convert_points_kernel)
        const Fq30 four = fq30_mulk_lazy<2>(fq30_mulk_lazy<2>(fq30_one()));                // < 4.1
        const Fq30 rhs = fq30_add_lazy(fq30_mul(fq30_sqr(p.x), p.x), four);                // x^3 + 4 < 5.2
        if (!pc_eq_mod(fq30_sqr(p.y), rhs)) st = PC_NOT_ON_CURVE;
        else if (!g1_in_subgroup(p.x, p.y)) st = PC_NOT_IN_SUBGROUP;
    }
    if (i == 0) {
        Fq30 gx, gy;
        g1_generator(gx, gy);
        bool same = true;
#pragma unroll
        for (int l = 0; l < 13; ++l) same = same && p.x.v[l] == gx.v[l] && p.y.v[l] == gy.v[l];
        if (!same) out[2] = 1ull;
    }
    const unsigned long long bad = __ballot(st != PC_OK);
    if (st != PC_OK) atomicMin(&out[0], (unsigned long long)((i << 8) | st));
    if (threadIdx.x == 0 && bad) atomicAdd(&out[1], (unsigned long long)__popcll(bad));
}
void launch_srs_membership(const uint32_t* pts, uint64_t n, unsigned long long* out, hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(srs_membership_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, pts, n, out);
}

// The weights of the ratio test: pw[i] = rho^i and pw_shift[i] = rho^(i - 1), pw_shift[0] = 0 (n elements each), so that
// the first k entries of pw weigh P_0 .. P_(k-1) and the first k + 1 entries of pw_shift weigh P_1 .. P_k alike.
__global__ __launch_bounds__(256) void fr_powers_kernel(Fr rho, uint64_t n, Fr* pw, Fr* pw_shift) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Fr e = fr_pow_u64(rho, i);
    pw[i] = e;
    if (i == 0) pw_shift[0] = Fr::zero();
    if (i + 1 < n) pw_shift[i + 1] = e;
}
void launch_fr_powers(const Fr& rho, uint64_t n, Fr* pw, Fr* pw_shift, hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(fr_powers_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, rho, n, pw, pw_shift);
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

// dst[i] = [t^i] src[i], canonical affine, one thread per point: t^i by fr_pow_u64, then g1_ladder (r < 2^255).  The base is
// whatever the record holds: g1_madd_xy's equal and opposite branches make the result [k]P by the group law for every curve
// point, those of small order included; an identity stays one.  Spare lanes shadow the last point and skip only the store
// (srs_generate_kernel: the inversion's exit test is wave-uniform).
struct SrsContributeArgs {
    Fr t;
    uint64_t n;
    const uint32_t* src;
    uint32_t* dst;
};
__global__ __launch_bounds__(64) void srs_contribute_kernel(SrsContributeArgs a) {
    const uint64_t i0 = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    const uint64_t i = i0 < a.n ? i0 : a.n - 1;
    const Fr k = fe_from_mont(fr_pow_u64(a.t, i));
    const G1Affine r = g1_to_affine(g1_ladder(k, ld_affine(a.src, i)));
    if (i0 >= a.n) return;
    uint32_t* q = a.dst + i0 * PT_WORDS;
    st_fq(q, r.x);
    st_fq(q + 12, r.y);
}
void launch_srs_contribute(const Fr& t, uint64_t n, const uint32_t* src, uint32_t* dst, hipStream_t st) {
    if (n == 0) return;
    SrsContributeArgs a;
    a.t = t;
    a.n = n;
    a.src = src;
    a.dst = dst;
    hipLaunchKernelGGL(srs_contribute_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, a);
}

// ---- typlonk_srs_g1_ntt (srs_check.hip): a radix-2 NTT whose elements are G1 points ----------------------------------------
// Decimation in time over the bit-reversed first n = 2^log_n records, one launch per stage, one thread per butterfly, the
// points canonical affine records between the stages.  Butterfly j of a block of 2^stage points:
//     (P, Q) -> (P + [w]Q, P - [w]Q),   w = root^j,   root = the generator of the domain of size 2^stage (or its inverse).
// [w]Q is g1_ladder; j = 0 (all of stage 1) skips it.  Both sums go through g1_madd, so P = +-[w]Q and an identity on either
// side are g1_madd_xy's own branches; the two results share one inversion.  Stage 1 reads `src` -- the source entry --
// through the bit reversal and every later stage works in place on `dst`: a butterfly reads and writes its own two records
// only.  Spare lanes (n / 2 < 64) shadow the last butterfly of their own wavefront and skip only the stores.
struct SrsNttStageArgs {
    Fr root;
    const uint32_t* src;
    uint32_t* dst;
    uint32_t log_n, stage;
};
// both of a butterfly's results as canonical affine records with ONE inversion, of ZZ ZZZ of the one times ZZ ZZZ of the
// other (an identity contributes 1, so every lane inverts)
__device__ __forceinline__ void g1_pair_to_affine(const G1Xyzz& a, const G1Xyzz& b, G1Affine& ra, G1Affine& rb) {
    const bool ia = a.is_inf(), ib = b.is_inf();
    const Fq30 ta = ia ? fq30_one() : fq30_mul(a.zz, a.zzz), tb = ib ? fq30_one() : fq30_mul(b.zz, b.zzz);   // < 1.01
    const Fq30 inv = fq30_inv(fq30_mul(ta, tb));                       // < 1.01
    const Fq30 va = fq30_mul(inv, tb), vb = fq30_mul(inv, ta);         // 1 / (ZZ ZZZ) of a, of b
    ra.x = fq30_canon(fq30_mul(a.x, fq30_mul(va, a.zzz)));             // X / ZZ
    ra.y = fq30_canon(fq30_mul(a.y, fq30_mul(va, a.zz)));              // Y / ZZZ
    rb.x = fq30_canon(fq30_mul(b.x, fq30_mul(vb, b.zzz)));
    rb.y = fq30_canon(fq30_mul(b.y, fq30_mul(vb, b.zz)));
    if (ia) ra = G1Affine::inf();
    if (ib) rb = G1Affine::inf();
}
// One butterfly, stated once for the stage kernel below and the batched one (srs_g1_ntt_batch_stage_kernel): w = root^j,
// (P, Q) = records rp, rq of `in`, the results to records ip, iq of `out` unless the lane is a spare one.
// (P is loaded behind the ladder: across it the kernel holds what srs_contribute_kernel holds, and no more)
__device__ __forceinline__ void g1_ntt_butterfly(const Fr& root, uint32_t j, const uint32_t* in, uint64_t rp, uint64_t rq, uint32_t* out,
                                                 uint64_t ip, uint64_t iq, bool live) {
    const G1Affine q = ld_affine(in, rq);
    G1Xyzz wq = G1Xyzz::from_affine(q);
    if (j != 0) wq = g1_ladder(fe_from_mont(fr_pow_u64(root, j)), q);
    const G1Affine p = ld_affine(in, rp);
    G1Xyzz sum = wq, dif = wq;
    dif.y = fq30_neg_lazy<4>(wq.y);                                    // -[w]Q: 4p - Y <= 4p, the bound g1_madd_xy needs of Y1
    g1_madd(sum, p, false);
    g1_madd(dif, p, false);
    G1Affine rs, rd;
    g1_pair_to_affine(sum, dif, rs, rd);
    if (!live) return;
    uint32_t* o = out + ip * PT_WORDS;
    st_fq(o, rs.x);
    st_fq(o + 12, rs.y);
    o = out + iq * PT_WORDS;
    st_fq(o, rd.x);
    st_fq(o + 12, rd.y);
}
__global__ __launch_bounds__(64) void srs_g1_ntt_stage_kernel(SrsNttStageArgs a) {
    const uint32_t t0 = blockIdx.x * 64 + threadIdx.x, nb = 1u << (a.log_n - 1);
    const uint32_t t = t0 < nb ? t0 : nb - 1;
    const uint32_t half = 1u << (a.stage - 1), j = t & (half - 1);
    const uint32_t ip = ((t - j) << 1) + j, iq = ip + half;            // < 2^log_n
    const uint32_t sh = 32 - a.log_n;                                  // stage 1: src through the bit reversal
    const bool first = a.stage == 1;
    g1_ntt_butterfly(a.root, j, first ? a.src : a.dst, first ? __brev(ip) >> sh : ip, first ? __brev(iq) >> sh : iq, a.dst, ip, iq, t0 < nb);
}
// stage 1 <= stage <= log_n of the transform of 2^log_n points, log_n >= 1; root: see above
void launch_srs_g1_ntt_stage(const Fr& root, uint32_t log_n, uint32_t stage, const uint32_t* src, uint32_t* dst, hipStream_t st) {
    SrsNttStageArgs a;
    a.root = root;
    a.src = src;
    a.dst = dst;
    a.log_n = log_n;
    a.stage = stage;
    const uint32_t nb = 1u << (log_n - 1);
    hipLaunchKernelGGL(srs_g1_ntt_stage_kernel, dim3((nb + 63) / 64), dim3(64), 0, st, a);
}

// pts[i] <- [k] pts[i], i < n, in place (the transform's 1/n): srs_contribute_kernel with one scalar for every point
struct SrsScaleArgs {
    Fr k;
    uint64_t n;
    uint32_t* pts;
};
__global__ __launch_bounds__(64) void srs_g1_scale_kernel(SrsScaleArgs a) {
    const uint64_t i0 = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    const uint64_t i = i0 < a.n ? i0 : a.n - 1;
    const G1Affine r = g1_to_affine(g1_ladder(fe_from_mont(a.k), ld_affine(a.pts, i)));
    if (i0 >= a.n) return;
    uint32_t* q = a.pts + i0 * PT_WORDS;
    st_fq(q, r.x);
    st_fq(q + 12, r.y);
}
void launch_srs_g1_scale(const Fr& k, uint64_t n, uint32_t* pts, hipStream_t st) {
    if (n == 0) return;
    SrsScaleArgs a;
    a.k = k;
    a.n = n;
    a.pts = pts;
    hipLaunchKernelGGL(srs_g1_scale_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, a);
}

// ---- typlonk_open_all_* (open_all.hip): every opening of a polynomial over its domain ---------------------------------------
// dst[i] = [k_i] src[i], canonical affine, one thread per record: srs_contribute_kernel with the scalar read from a device
// vector of Montgomery residues instead of computed.  k_i = 0 and an identity record both give the all-zero record (the
// ladder never leaves the identity).  Spare lanes shadow the last point and skip only the store.
struct G1PointwiseArgs {
    const Fr* k;
    uint64_t n;
    const uint32_t* src;
    uint32_t* dst;
};
__global__ __launch_bounds__(64) void g1_pointwise_mul_kernel(G1PointwiseArgs a) {
    const uint64_t i0 = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    const uint64_t i = i0 < a.n ? i0 : a.n - 1;
    const Fr k = fe_from_mont(a.k[i]);
    const G1Affine r = g1_to_affine(g1_ladder(k, ld_affine(a.src, i)));
    if (i0 >= a.n) return;
    uint32_t* q = a.dst + i0 * PT_WORDS;
    st_fq(q, r.x);
    st_fq(q + 12, r.y);
}
void launch_g1_pointwise_mul(const Fr* k, uint64_t n, const uint32_t* src, uint32_t* dst, hipStream_t st) {
    if (n == 0) return;
    G1PointwiseArgs a;
    a.k = k;
    a.n = n;
    a.src = src;
    a.dst = dst;
    hipLaunchKernelGGL(g1_pointwise_mul_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, a);
}

// The first operand of the circular product, 2n records: dst = (src[n-2], src[n-3], ..., src[0], identity x (n + 1)).  One
// thread per 16 bytes of a record's 128 (the stride's padding is copied along: it is never read).
__global__ __launch_bounds__(256) void open_all_gather_kernel(const uint4* src, uint4* dst, uint64_t n) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    constexpr uint64_t Q = PT_WORDS / 4;
    const uint64_t i = t / Q, q = t % Q;
    if (i >= 2 * n) return;
    dst[t] = i + 1 < n ? src[(n - 2 - i) * Q + q] : make_uint4(0, 0, 0, 0);
}
void launch_open_all_gather(const uint32_t* src, uint32_t* dst, uint64_t n, hipStream_t st) {
    const uint64_t threads = 2 * n * (PT_WORDS / 4);
    hipLaunchKernelGGL(open_all_gather_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, (const uint4*)src, (uint4*)dst, n);
}

// The second operand, 2n elements, with the 1/(2n) of the inverse group transform folded in (the Fr transform is linear):
// c[0] = k f[n-1], c[1 .. n] = 0, c[n+1+j] = k f[j] for j < n - 1; f holds m <= n coefficients, zero above.
__global__ __launch_bounds__(256) void open_all_coeffs_kernel(const Fr* f, uint64_t m, uint64_t n, Fr k, Fr* c) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * n) return;
    const uint64_t j = i == 0 ? n - 1 : i - n - 1;      // (1 <= i <= n wraps around: >= m, zero)
    c[i] = (i == 0 || i > n) && j < m ? fe_mul(f[j], k) : Fr::zero();
}
void launch_open_all_coeffs(const Fr* f, uint64_t m, uint64_t n, const Fr& k, Fr* c, hipStream_t st) {
    hipLaunchKernelGGL(open_all_coeffs_kernel, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0, st, f, m, n, k, c);
}

// ---- typlonk_open_chunks_* (open_chunks.hip): a polynomial's openings on every coset of its domain ----------------------------
// srs_g1_ntt_stage_kernel over `blocks` transforms of 2^l records in one launch, one thread per butterfly of one block:
// thread t works on block t / 2^(l-1).  Block b is records [b * src_stride, + 2^l) of src -- read by stage 1 through the bit
// reversal over the low l bits -- and [b * dst_stride, + 2^l) of dst, where every later stage works in place.  The strides are
// in records and at least 2^l; src and dst must not overlap.  Spare lanes shadow the last butterfly and skip only the stores.
struct G1NttBatchStageArgs {
    Fr root;
    const uint32_t* src;
    uint32_t* dst;
    uint64_t blocks, src_stride, dst_stride;
    uint32_t l, stage;
};
__global__ __launch_bounds__(64) void srs_g1_ntt_batch_stage_kernel(G1NttBatchStageArgs a) {
    const uint64_t t0 = (uint64_t)blockIdx.x * 64 + threadIdx.x, nb = a.blocks << (a.l - 1);
    const uint64_t t = t0 < nb ? t0 : nb - 1;
    const uint64_t b = t >> (a.l - 1);                                 // < blocks
    const uint32_t tb = (uint32_t)(t - (b << (a.l - 1)));              // the butterfly within the block, < 2^(l-1)
    const uint32_t half = 1u << (a.stage - 1), j = tb & (half - 1);
    const uint32_t ip = ((tb - j) << 1) + j, iq = ip + half;           // < 2^l
    const uint32_t sh = 32 - a.l;
    const bool first = a.stage == 1;
    const uint64_t ob = b * a.dst_stride, sb = first ? b * a.src_stride : ob;
    g1_ntt_butterfly(a.root, j, first ? a.src : a.dst, sb + (first ? __brev(ip) >> sh : ip), sb + (first ? __brev(iq) >> sh : iq), a.dst,
                     ob + ip, ob + iq, t0 < nb);
}
void launch_srs_g1_ntt_batch_stage(const Fr& root, uint32_t l, uint32_t stage, uint64_t blocks, const uint32_t* src, uint64_t src_stride,
                                   uint32_t* dst, uint64_t dst_stride, hipStream_t st) {
    if (blocks == 0) return;
    G1NttBatchStageArgs a;
    a.root = root;
    a.src = src;
    a.dst = dst;
    a.blocks = blocks;
    a.src_stride = src_stride;
    a.dst_stride = dst_stride;
    a.l = l;
    a.stage = stage;
    const uint64_t nb = blocks << (l - 1);
    hipLaunchKernelGGL(srs_g1_ntt_batch_stage_kernel, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, st, a);
}

// The pointwise pass: dst[o] = sum_{j < l} [k_(o,j)] y_(o,j), canonical affine, for o < outputs.  With p = o / period and
// i = o % period, term j of output o is the scalar k[(p l + j) period + i] -- CANONICAL words, not Montgomery residues -- and
// the record tab[j period + i]: `outputs / period` polynomials over one table of l blocks of `period` records.
// One thread per (output, slice): thread t takes slice t % g of output t / g, the l / g terms from (t % g) l / g on, as ONE
// doubling chain, most significant bit first -- per bit one g1_dbl, then one g1_madd for every term of the slice whose bit is
// set.  That shares the 255 doublings among the slice's terms; the additions are not shared, and since 64 lanes never agree on
// a bit, a wavefront runs the g1_madd of nearly every (bit, term), as it does in g1_ladder.  The scalar's word is read from
// memory per (bit, term): a slice's scalars do not fit in registers, and there is no indexed private array.
// g > 1: the g partial sums of an output lie in g neighbouring lanes of one wavefront (g divides 64); they go through the LDS
// ([word][lane]) and EVERY lane of the group adds all g of them in the same order with g1_add and converts the sum, so that
// the inversion's exit test stays wave-uniform; the group's first lane stores.  The sum is a group element and the record
// its canonical form, so every g gives the same words.  k = 0, identity records and P = +-Q are g1_madd_xy's and g1_add's own
// branches.  Spare lanes (whole groups: g divides the thread count) shadow the last output and skip only the store.
struct G1PointwiseMsmArgs {
    const Fr* k;
    const uint32_t* tab;
    uint32_t* dst;
    uint64_t outputs, period;
    uint32_t l, g;
};
__global__ __launch_bounds__(64) void g1_pointwise_msm_kernel(G1PointwiseMsmArgs a) {
    __shared__ uint32_t part[52 * 64];
    const uint64_t t = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    const uint64_t o0 = t / a.g, o = o0 < a.outputs ? o0 : a.outputs - 1;
    const uint32_t s = (uint32_t)(t % a.g), per = a.l / a.g;
    const uint64_t p = o / a.period, i = o - p * a.period;
    const uint32_t* kw = reinterpret_cast<const uint32_t*>(a.k + (p * a.l + (uint64_t)s * per) * a.period + i);   // term j0 = s per
    const uint64_t r0 = (uint64_t)s * per * a.period + i;
    const uint64_t kstep = a.period * (sizeof(Fr) / 4);                // words from one term's scalar to the next
    G1Xyzz acc = G1Xyzz::inf();
#pragma unroll 1
    for (int bit = 254; bit >= 0; --bit) {
        acc = g1_dbl(acc);
        const uint32_t* w = kw + (bit >> 5);
#pragma unroll 1
        for (uint32_t j = 0; j < per; ++j) {
            if ((w[j * kstep] >> (bit & 31)) & 1u) g1_madd(acc, ld_affine(a.tab, r0 + j * a.period), false);
        }
    }
    if (a.g > 1) {
        const uint32_t lane = threadIdx.x, base = lane - s;
#pragma unroll
        for (int l = 0; l < 13; ++l) {
            part[l * 64 + lane] = acc.x.v[l];
            part[(13 + l) * 64 + lane] = acc.y.v[l];
            part[(26 + l) * 64 + lane] = acc.zz.v[l];
            part[(39 + l) * 64 + lane] = acc.zzz.v[l];
        }
        __syncthreads();
        acc = G1Xyzz::inf();
#pragma unroll 1
        for (uint32_t q = 0; q < a.g; ++q) {
            G1Xyzz b;
#pragma unroll
            for (int l = 0; l < 13; ++l) {
                b.x.v[l] = part[l * 64 + base + q];
                b.y.v[l] = part[(13 + l) * 64 + base + q];
                b.zz.v[l] = part[(26 + l) * 64 + base + q];
                b.zzz.v[l] = part[(39 + l) * 64 + base + q];
            }
            acc = g1_add(acc, b);
        }
    }
    const G1Affine r = g1_to_affine(acc);
    if (o0 >= a.outputs || s != 0) return;
    uint32_t* q = a.dst + o0 * PT_WORDS;
    st_fq(q, r.x);
    st_fq(q + 12, r.y);
}
// l, g powers of two, g <= min(l, 64); outputs a multiple of period >= 1; dst must not overlap k or tab
void launch_g1_pointwise_msm(const Fr* k, const uint32_t* tab, uint32_t* dst, uint64_t outputs, uint64_t period, uint32_t l, uint32_t g,
                             hipStream_t st) {
    if (outputs == 0) return;
    G1PointwiseMsmArgs a;
    a.k = k;
    a.tab = tab;
    a.dst = dst;
    a.outputs = outputs;
    a.period = period;
    a.l = l;
    a.g = g;
    hipLaunchKernelGGL(g1_pointwise_msm_kernel, dim3((unsigned)((outputs * g + 63) / 64)), dim3(64), 0, st, a);
}

// The first operand of the l circular products of size 2r, 2n = l * 2r records in l blocks: block j is open_all_gather_kernel's
// sequence of the decimated points S_(a l + j), dst[j 2r + i] = src[(r - 2 - i) l + j] for i + 1 < r and the identity above.
// It reads src[0, n - l).
__global__ __launch_bounds__(256) void open_chunks_gather_kernel(const uint4* src, uint4* dst, uint64_t r, uint64_t l) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    constexpr uint64_t Q = PT_WORDS / 4;
    const uint64_t rec = t / Q, q = t % Q;
    if (rec >= 2 * r * l) return;
    const uint64_t j = rec / (2 * r), i = rec % (2 * r);
    dst[t] = i + 1 < r ? src[((r - 2 - i) * l + j) * Q + q] : make_uint4(0, 0, 0, 0);
}
void launch_open_chunks_gather(const uint32_t* src, uint32_t* dst, uint64_t r, uint64_t l, hipStream_t st) {
    const uint64_t threads = 2 * r * l * (PT_WORDS / 4);
    hipLaunchKernelGGL(open_chunks_gather_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, (const uint4*)src, (uint4*)dst, r, l);
}

// The second operands, count * l vectors of 2r elements: vector p l + j is open_all_coeffs_kernel's sequence of the decimated
// coefficients f_(a l + j) of polynomial p, times k:  c[0] = k f_((r-1) l + j), c[1 .. r] = 0, c[r+1+a] = k f_(a l + j), a < r - 1.
// f[p] holds m coefficients, zero above.
__global__ __launch_bounds__(256) void open_chunks_coeffs_kernel(const Fr* const* f, uint64_t m, uint64_t r, uint64_t l, uint64_t count, Fr k, Fr* c) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= count * l * 2 * r) return;
    const uint64_t i = t % (2 * r), v = t / (2 * r), j = v % l, p = v / l;
    const uint64_t a = i == 0 ? r - 1 : i - r - 1;      // (1 <= i <= r wraps around: not read)
    const uint64_t idx = a * l + j;
    c[t] = (i == 0 || i > r) && idx < m ? fe_mul(f[p][idx], k) : Fr::zero();
}
void launch_open_chunks_coeffs(const Fr* const* f, uint64_t m, uint64_t r, uint64_t l, uint64_t count, const Fr& k, Fr* c, hipStream_t st) {
    const uint64_t threads = count * l * 2 * r;
    hipLaunchKernelGGL(open_chunks_coeffs_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, f, m, r, l, count, k, c);
}

// e[p n + i] = f[p][i] for i < m and zero above, n = r l: the polynomials padded to the domain, for the evaluations' transform
__global__ __launch_bounds__(256) void open_chunks_pad_kernel(const Fr* const* f, uint64_t m, uint64_t n, uint64_t count, Fr* e) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= count * n) return;
    const uint64_t i = t % n;
    e[t] = i < m ? f[t / n][i] : Fr::zero();
}
void launch_open_chunks_pad(const Fr* const* f, uint64_t m, uint64_t n, uint64_t count, Fr* e, hipStream_t st) {
    hipLaunchKernelGGL(open_chunks_pad_kernel, dim3((unsigned)((count * n + 255) / 256)), dim3(256), 0, st, f, m, n, count, e);
}

// The evaluations chunk-major: out[p n + k l + t] = ev[p n + k + r t], the l values on coset k contiguous.  One thread per
// element written; src and dst must not overlap.
__global__ __launch_bounds__(256) void open_chunks_evals_kernel(const Fr* ev, uint64_t r, uint64_t l, uint64_t count, Fr* out) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t n = r * l;
    if (t >= count * n) return;
    const uint64_t w = t % n, k = w / l, u = w % l;
    out[t] = ev[t - w + k + r * u];
}
void launch_open_chunks_evals(const Fr* ev, uint64_t r, uint64_t l, uint64_t count, Fr* out, hipStream_t st) {
    hipLaunchKernelGGL(open_chunks_evals_kernel, dim3((unsigned)((count * r * l + 255) / 256)), dim3(256), 0, st, ev, r, l, count, out);
}

}  // namespace ty
