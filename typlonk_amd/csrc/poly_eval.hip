// libtyplonk_hip.so -- polynomials evaluated at many points: typlonk_poly_eval_dev
//   DensePolynomial::evaluate (ark-poly), reached from permutation/src/lib.rs:165-176 and plonk/src/proof.rs:205-210: the
//   verifier's sigma(zeta) and PI(zeta) of every proof of a batch (verify.hip).
//
// count x n_points x m Fr multiply-adds.  A workgroup stages one PE_S-coefficient chunk of one polynomial in the LDS once
// and evaluates it at a tile of P points (P = 1, 2, 4, .. 256): thread t takes point t mod P and runs Horner over segment
// t / P of the chunk (256 / P segments of L = PE_S P / 256 coefficients), the segments are joined by a tree with ratios
// x^L, x^2L, .., and the chunk's value is scaled by x^(PE_S j) (a short ladder per point and chunk).  A second kernel
// sums the chunk partials of every (polynomial, point).  Field arithmetic is exact, so the result is the same element
// whatever the chunking: Horner's value, bit for bit.
#include "host.hpp"
#include "host_checks.hpp"

using namespace ty;
using namespace tyh;

namespace {

constexpr uint32_t PE_S = 1024;         // coefficients per chunk (32 KiB of LDS)
constexpr uint32_t PE_LOG_S = 10;
constexpr uint32_t PE_MAX_POLYS = 16;
constexpr size_t PE_PART_MAX = (size_t)1 << 22;   // partials resident at once (128 MiB): points are processed in tiles

__device__ __forceinline__ Fr pe_ld(const Fr* p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    const uint4 a = q[0], b = q[1];
    Fr r;
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
    r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
    return r;
}
__device__ __forceinline__ void pe_st(Fr* p, const Fr& r) {
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(r.v[0], r.v[1], r.v[2], r.v[3]);
    q[1] = make_uint4(r.v[4], r.v[5], r.v[6], r.v[7]);
}

struct PolyEvalArgs {
    const Fr* poly[PE_MAX_POLYS];
    uint64_t m;
    const Fr* pts;     // the n_pts points of this tile
    uint32_t n_pts;
    uint32_t log_p;    // P = 2^log_p points per workgroup
    uint32_t nchunk;
    Fr* part;          // [count][n_pts][nchunk]
};

// grid (nchunk, ceil(n_pts / P), count)
__global__ __launch_bounds__(256) void poly_eval_chunk_kernel(PolyEvalArgs a) {
    __shared__ Fr cf[PE_S];
    __shared__ Fr hs[256];
    const uint32_t j = blockIdx.x, p = blockIdx.z;
    const uint32_t P = 1u << a.log_p, G = 256u >> a.log_p, L = PE_S / G;
    const uint64_t base = (uint64_t)j * PE_S;
    const Fr* c = a.poly[p];
    for (uint32_t i = threadIdx.x; i < PE_S; i += 256) cf[i] = base + i < a.m ? pe_ld(c + base + i) : Fr::zero();
    __syncthreads();
    const uint32_t lp = threadIdx.x & (P - 1), seg = threadIdx.x >> a.log_p;
    const uint32_t k = blockIdx.y * P + lp;
    const Fr x = k < a.n_pts ? pe_ld(a.pts + k) : Fr::zero();
    // Horner over [seg L, seg L + L)
    Fr h = Fr::zero();
    const uint32_t s0 = seg * L;
    for (int i = (int)L - 1; i >= 0; --i) h = fe_add(cf[s0 + i], fe_mul(x, h));
    hs[threadIdx.x] = h;
    Fr xl = x;   // x^L (L is a power of two)
    for (uint32_t t = L; t > 1; t >>= 1) xl = fe_sqr(xl);
    __syncthreads();
    // segments g and g + s joined as h_g + x^(L s) h_{g+s}, s = 1, 2, 4, ..: the same P lanes of every segment hold one point
    for (uint32_t s = 1; s < G; s <<= 1) {
        const bool act = (seg & (2 * s - 1)) == 0;
        Fr v;
        if (act) v = fe_add(hs[threadIdx.x], fe_mul(xl, hs[threadIdx.x + s * P]));
        __syncthreads();
        if (act) hs[threadIdx.x] = v;
        __syncthreads();
        xl = fe_sqr(xl);
    }
    if (seg == 0 && k < a.n_pts) {
        // x^(PE_S j): x^PE_S by squaring, then a ladder over the bits of j
        Fr xs = x;
        for (uint32_t t = 0; t < PE_LOG_S; ++t) xs = fe_sqr(xs);
        Fr sc = Fr::one();
        for (int b = 31 - __clz(j | 1); b >= 0; --b) {
            sc = fe_sqr(sc);
            if ((j >> b) & 1u) sc = fe_mul(sc, xs);
        }
        pe_st(a.part + ((uint64_t)p * a.n_pts + k) * a.nchunk + j, fe_mul(hs[threadIdx.x], sc));
    }
}

// grid (n_pts, count): out[p * out_stride + k] = sum_j part[p][k][j]
__global__ __launch_bounds__(256) void poly_eval_sum_kernel(const Fr* part, uint32_t n_pts, uint32_t nchunk, Fr* out,
                                                            uint64_t out_stride) {
    __shared__ Fr red[256];
    const uint32_t k = blockIdx.x, p = blockIdx.y;
    const Fr* src = part + ((uint64_t)p * n_pts + k) * nchunk;
    Fr acc = Fr::zero();
    for (uint32_t j = threadIdx.x; j < nchunk; j += 256) acc = fe_add(acc, pe_ld(src + j));
    red[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] = fe_add(red[threadIdx.x], red[threadIdx.x + off]);
        __syncthreads();
    }
    if (threadIdx.x == 0) pe_st(out + (uint64_t)p * out_stride + k, red[0]);
}

}  // namespace

namespace tyh {

int poly_eval_run(typlonk_ctx* ctx, const Fr* const* polys, size_t count, uint64_t m, const uint64_t* points, size_t n_points,
                  uint64_t* out) {
    const uint32_t nchunk = (uint32_t)((m + PE_S - 1) / PE_S);
    // points per tile: every tile's partials fit PE_PART_MAX; a multiple of the 256-point workgroup tile when it is larger
    size_t tile = std::max<size_t>(1, PE_PART_MAX / ((size_t)count * nchunk));
    if (tile > 256) tile &= ~(size_t)255;
    tile = std::min(tile, n_points);
    const size_t pts_bytes = n_points * sizeof(Fr), out_bytes = count * n_points * sizeof(Fr);
    const size_t part_bytes = count * tile * nchunk * sizeof(Fr);
    int rc = ensure(ctx, ctx->eval_ws, pts_bytes + out_bytes + part_bytes);
    if (rc) return rc;
    Fr* d_pts = (Fr*)ctx->eval_ws.p;
    Fr* d_out = d_pts + n_points;
    Fr* d_part = d_out + count * n_points;
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(d_pts, points, pts_bytes, hipMemcpyHostToDevice, s));
    PolyEvalArgs a{};
    for (size_t p = 0; p < PE_MAX_POLYS; ++p) a.poly[p] = polys[p < count ? p : 0];
    a.m = m;
    a.nchunk = nchunk;
    a.part = d_part;
    for (size_t k0 = 0; k0 < n_points; k0 += tile) {
        const uint32_t nt = (uint32_t)std::min(tile, n_points - k0);
        uint32_t log_p = 0;
        while ((1u << log_p) < nt && log_p < 8) ++log_p;
        a.pts = d_pts + k0;
        a.n_pts = nt;
        a.log_p = log_p;
        const uint32_t gy = (nt + (1u << log_p) - 1) >> log_p;
        hipLaunchKernelGGL(poly_eval_chunk_kernel, dim3(nchunk, gy, (uint32_t)count), dim3(256), 0, s, a);
        hipLaunchKernelGGL(poly_eval_sum_kernel, dim3(nt, (uint32_t)count), dim3(256), 0, s, (const Fr*)d_part, nt, nchunk,
                           d_out + k0, (uint64_t)n_points);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return TYPLONK_OK;
}

}  // namespace tyh

int typlonk_poly_eval_dev(typlonk_ctx* ctx, const typlonk_buf* const* polys, size_t count, size_t offset, size_t m,
                          const uint64_t (*points)[4], size_t n_points, uint64_t* out) {
    if (!ctx || !polys || !points || !out) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    if (count < 1 || count > PE_MAX_POLYS) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "1 <= count <= 16 polynomials");
    if (n_points < 1 || n_points > 0xffffffffull) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "n_points must be >= 1");
    if (m < 1 || m > ((size_t)1 << (TYPLONK_MAX_PROVER_LOG_N + 1)))
        return fail(ctx, TYPLONK_ERR_LENGTH, "poly_eval takes 1 <= m <= 2^25 coefficients");
    const Fr* ptrs[PE_MAX_POLYS];
    for (size_t p = 0; p < count; ++p) {
        if (!polys[p]) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null polynomial");
        if (offset > polys[p]->n || m > polys[p]->n - offset) return fail(ctx, TYPLONK_ERR_RANGE, "range outside buffer");
        ptrs[p] = polys[p]->d + offset;
    }
    for (size_t k = 0; k < n_points; ++k)
        if (!fr_canonical(points[k])) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "point is not a canonical Fr residue");
    HIPCHK(hipSetDevice(ctx->device));
    return poly_eval_run(ctx, ptrs, count, m, &points[0][0], n_points, out);
}
