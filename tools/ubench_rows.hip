// Latency of the one-limb-per-lane Fq multiplication (csrc/fq30_rows.hpp) against the single-lane fq30_mul, and of one
// g1_add_rows level against one butterfly_add4 level, each as a dependent chain at one wavefront per SIMD -- the regime of the
// bucket reduction's last levels.  Prints microseconds per operation and checks that the two multiplication chains agree.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ubench_rows.hip -o tools/ubench_rows && tools/ubench_rows
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "../typlonk_amd/csrc/fq30_rows.hpp"
#include "../typlonk_amd/csrc/msm_common.hpp"

using namespace ty;

#define CK(x)                                                              \
    do {                                                                   \
        hipError_t e_ = (x);                                               \
        if (e_ != hipSuccess) {                                            \
            printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

// x <- x * y, n times, in the row form: every row of every wavefront runs the same chain; row 0 of wave 0 stores
__global__ __launch_bounds__(256) void mul_chain_rows(const uint32_t* __restrict__ xy, int n, uint32_t* out) {
    using W = RowsDev;
    uint32_t x = fqr_load<W>(xy);
    const uint32_t y = fqr_load<W>(xy + 12);
#pragma unroll 1
    for (int i = 0; i < n; ++i) x = fqr_mul<W>(x, y);
    if (blockIdx.x == 0 && threadIdx.x < 64) fqr_store_rows<W>(out, x);
}
__global__ __launch_bounds__(256) void mul_chain_lane(const uint32_t* __restrict__ xy, int n, uint32_t* out) {
    Fq30 x = ld_fq(xy);
    const Fq30 y = ld_fq(xy + 12);
#pragma unroll 1
    for (int i = 0; i < n; ++i) x = fq30_mul(x, y);
    if (blockIdx.x == 0 && threadIdx.x == 0) st_fq(out, fq30_canon(x));
}
// S <- S + D, n times (D fixed), one addition per wavefront through the LDS in the limb layout; wave 0 of block 0 stores
__global__ __launch_bounds__(256) void add_chain_rows(const uint32_t* __restrict__ pts, int n, uint32_t* out) {
    using W = RowsDev;
    __shared__ uint32_t buf[4][3][FQR_POINT_WORDS];
    uint32_t(*b)[FQR_POINT_WORDS] = buf[threadIdx.x >> 6];
    const uint32_t lane = threadIdx.x & 63u, c = lane >> 4, i = lane & 15u;
    b[0][lane] = fqr_limb_of_words(pts + c * 12, i);
    b[2][lane] = fqr_limb_of_words(pts + 48 + c * 12, i);
    int cur = 0;
#pragma unroll 1
    for (int k = 0; k < n; ++k) {
        __syncthreads();
        g1_add_rows<W>(b[cur], b[2], b[cur ^ 1]);
        cur ^= 1;
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x < 64) fqr_store_rows<W>(out, b[cur][lane]);
}
// the same chain as butterfly_add4 levels: lanes {0, 1} hold S, lanes {2, 3} hold D; after a level all four hold S + D and
// lanes 2, 3 take D again
__global__ __launch_bounds__(256) void add_chain_bfly(const uint32_t* __restrict__ pts, int n, uint32_t* out) {
    const bool dside = (threadIdx.x & 2u) != 0;
    const G1Xyzz d = ld_xyzz(pts, 1);
    G1Xyzz v = dside ? d : ld_xyzz(pts, 0);
#pragma unroll 1
    for (int k = 0; k < n; ++k) {
        v = butterfly_add4(v, 2);
        if (dside) v = d;
    }
    v = butterfly_add4(v, 2);
    if (blockIdx.x == 0 && threadIdx.x == 0) st_xyzz(out, 0, v);
}

int main() {
    // eight pseudo-random field elements < 2^376: x, y for the multiplication chains, and two "points" whose words the group
    // law treats as bounded values (they need not lie on the curve to time a level)
    std::vector<uint32_t> h(96);
    uint32_t seed = 12345;
    for (auto& w : h) w = (seed = seed * 1664525u + 1013904223u);
    for (int e = 0; e < 8; ++e) h[e * 12 + 11] &= 0x00ffffffu;   // < 2^376 < p
    uint32_t *d_in, *d_out;
    CK(hipMalloc(&d_in, 96 * 4));
    CK(hipMalloc(&d_out, 4 * 48 * 4));
    CK(hipMemcpy(d_in, h.data(), 96 * 4, hipMemcpyHostToDevice));
    CK(hipMemset(d_out, 0, 4 * 48 * 4));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    const int blocks = 256, n = 2000;
    float ms;
    for (int rep = 0; rep < 2; ++rep) {
        CK(hipEventRecord(e0));
        hipLaunchKernelGGL(mul_chain_rows, dim3(blocks), dim3(256), 0, 0, d_in, n, d_out);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (rep) printf("fqr_mul   (rows)  %.3f us per multiplication\n", ms * 1e3 / n);
        CK(hipEventRecord(e0));
        hipLaunchKernelGGL(mul_chain_lane, dim3(blocks), dim3(256), 0, 0, d_in, n, d_out + 48);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (rep) printf("fq30_mul  (lane)  %.3f us per multiplication\n", ms * 1e3 / n);
    }
    const int na = 200;
    for (int rep = 0; rep < 2; ++rep) {
        CK(hipEventRecord(e0));
        hipLaunchKernelGGL(add_chain_rows, dim3(blocks), dim3(256), 0, 0, d_in, na, d_out + 96);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (rep) printf("g1_add_rows level       %.3f us\n", ms * 1e3 / na);
        CK(hipEventRecord(e0));
        hipLaunchKernelGGL(add_chain_bfly, dim3(blocks), dim3(256), 0, 0, d_in, na, d_out + 144);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (rep) printf("butterfly_add4 level    %.3f us\n", ms * 1e3 / (na + 1));
    }
    std::vector<uint32_t> o(4 * 48);
    CK(hipMemcpy(o.data(), d_out, 4 * 48 * 4, hipMemcpyDeviceToHost));
    // the row chain stores a value < 2p, the lane chain the canonical one: compare after the same canonicalisation
    uint32_t wr[12], wl[12];
    for (int j = 0; j < 12; ++j) {
        wr[j] = o[j];
        wl[j] = o[48 + j];
    }
    uint32_t cr[12];
    fq30_pack(fq30_canon(fq30_unpack(wr)), cr);
    bool same = true;
    for (int j = 0; j < 12; ++j) same = same && cr[j] == wl[j];
    printf("multiplication chains agree: %s\n", same ? "yes" : "NO");
    return same ? 0 : 1;
}
