// The transform over G1 points and what is built on it: the kernels of typlonk_srs_g1_ntt (host: srs_check.hip) and of the FK20
// openings typlonk_open_chunks_* / typlonk_open_all_* (host: open_chunks.hip).  Set-up and opening time only, nothing of the
// prove() path.  The scalar multiplication they share with the contribution of srs_gen.hip is g1_ladder.hpp.
#include "launch.hpp"
#include "g1_ladder.hpp"

namespace ty {

// ---- a radix-2 NTT whose elements are G1 points (typlonk_srs_g1_ntt, and the three transforms of an opening) -----------------
// Decimation in time over the bit-reversed 2^l records of a block, one launch per stage, one thread per butterfly, the
// points canonical affine records between the stages.  Butterfly j of a group of 2^stage points:
//     (P, Q) -> (P + [w]Q, P - [w]Q),   w = root^j,   root = the generator of the domain of size 2^stage (or its inverse).
// [w]Q is g1_ladder; j = 0 (all of stage 1) skips it.  Both sums go through g1_madd, so P = +-[w]Q and an identity on either
// side are g1_madd_xy's own branches; the two results share one inversion.  Stage 1 reads `src` through the bit reversal and
// every later stage works in place on `dst`: a butterfly reads and writes its own two records only.  Spare lanes (a launch of
// fewer than 64 butterflies) shadow the last butterfly of their own wavefront and skip only the stores.
//
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
// One butterfly: w = root^j,
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

// One stage of ONE transform of 2^log_n records, one thread per butterfly; src, dst and the spare lanes as above.  It is the
// kernel below at blocks = 1 with 32-bit indices throughout, kept because it measures faster there by 0.13 to 0.14 ms a launch
// (profiles/r32_open_one_path.txt): g1_ntt_stages (srs_check.hip) picks it for a single block.
struct SrsNttStageArgs {
    Fr root;
    const uint32_t* src;
    uint32_t* dst;
    uint32_t log_n, stage;
};
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

// One stage of `blocks` transforms of 2^l records in one launch, one thread per butterfly of one block: thread t works on
// block t / 2^(l-1).  Block b is records [b * src_stride, + 2^l) of src -- read by stage 1 through the bit reversal over the
// low l bits -- and [b * dst_stride, + 2^l) of dst, where every later stage works in place.  The strides are in records and
// at least 2^l; src and dst must not overlap.  Spare lanes shadow the last butterfly and skip only the stores.
// The indices within a block are 32-bit: l <= 25 (typlonk_srs_g1_ntt's cap, and log_n + 1 of a table) gives tb < 2^24 and
// ip, iq < 2^25, a shift of 32 - l >= 7, and with blocks = 1 a grid of 2^18 workgroups.
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

// pts[i] <- [k] pts[i], i < n, in place (the transform's 1/n): g1_ladder_record with one scalar for every point.  Spare lanes
// shadow the last point.
struct SrsScaleArgs {
    Fr k;
    uint64_t n;
    uint32_t* pts;
};
__global__ __launch_bounds__(64) void srs_g1_scale_kernel(SrsScaleArgs a) {
    const uint64_t i0 = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    const uint64_t i = i0 < a.n ? i0 : a.n - 1;
    g1_ladder_record(fe_from_mont(a.k), a.pts, i, a.pts, i0, i0 < a.n);
}
void launch_srs_g1_scale(const Fr& k, uint64_t n, uint32_t* pts, hipStream_t st) {
    if (n == 0) return;
    SrsScaleArgs a;
    a.k = k;
    a.n = n;
    a.pts = pts;
    hipLaunchKernelGGL(srs_g1_scale_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, a);
}

// ---- typlonk_open_chunks_* and typlonk_open_all_* (open_chunks.hip): a polynomial's openings on every coset of its domain ------------
// The pointwise pass: dst[o] = sum_{j < l} [k_(o,j)] y_(o,j), canonical affine, for o < outputs.  With p = o / period and
// i = o % period, term j of output o is the scalar k[(p l + j) period + i] -- CANONICAL words, not Montgomery residues -- and
// the record tab[j period + i]: `outputs / period` polynomials over one table of l blocks of `period` records.
// One thread per (output, slice): thread t takes slice t % g of output t / g, the l / g terms from (t % g) l / g on, as ONE
// doubling chain, most significant bit first -- per bit one g1_dbl, then one g1_madd for every term of the slice whose bit is
// set.  That shares the 255 doublings among the slice's terms; the additions are not shared, and since 64 lanes never agree on
// a bit, a wavefront runs the g1_madd of nearly every (bit, term), as it does in g1_ladder.  The scalar's word is read from
// memory per (bit, term): a slice's scalars do not fit in registers, and there is no indexed private array.  l = 1, g = 1 is
// one ladder per record, u_i = [v_i] y_i: the pointwise pass of the one-point opening.
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

// The first operand of the l circular products of size 2r, 2n = l * 2r records in l blocks: block j is the decimated points
// S_(a l + j) reversed and padded, dst[j 2r + i] = src[(r - 2 - i) l + j] for i + 1 < r and the identity above.  It reads
// src[0, n - l).  One thread per 16 bytes of a record's 128 (the stride's padding is copied along: it is never read).
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

// The second operands, count * l vectors of 2r elements: vector p l + j is the decimated coefficients f_(a l + j) of polynomial
// p, times k (the Fr transform is linear):  c[0] = k f_((r-1) l + j), c[1 .. r] = 0, c[r+1+a] = k f_(a l + j), a < r - 1.
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
