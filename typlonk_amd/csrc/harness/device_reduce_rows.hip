// Test-only device harness over the row form of the bucket reduction (tests/test_gpu_reduce_rows.py): g1_add_rows
// (csrc/fq30_rows.hpp) on caller-made point pairs, and the four-launch reduction of msm_reduce.hip -- compiled here as a
// unit, as the library compiles it -- with its bit planes summed either way on the same buckets: one addition per wavefront
// (what launch_msm_rc_reduce runs) or one thread per point (msm_rc2_planes_kernel, the form before it).  Not linked into
// libtyplonk_hip.so; device_reduce.hip beside it keeps its own interface.
#include "../msm_reduce.hip"

#include <algorithm>

using namespace ty;

namespace {

struct Bufs {
    void* p[8] = {};
    int used = 0;
    hipError_t err = hipSuccess;
    uint32_t* zeros(uint64_t points) {   // zero words: ZZ = 0, the identity
        void* d = nullptr;
        const size_t bytes = (size_t)std::max<uint64_t>(points, 1) * 192;
        if (err == hipSuccess) err = hipMalloc(&d, bytes);
        if (err == hipSuccess) p[used++] = d;
        if (err == hipSuccess) err = hipMemset(d, 0, bytes);
        return static_cast<uint32_t*>(d);
    }
    ~Bufs() {
        for (int i = 0; i < used; ++i) (void)hipFree(p[i]);
    }
};

// the shapes the planes kernels of either form take (device_reduce.hip's check, and cl, ch >= 6)
bool shape_ok(const RcShape& sh) {
    if (sh.nsets < 1 || sh.nsets > 32 || sh.c1 != sh.cl + sh.ch || sh.c1 > 19) return false;
    if (sh.cl < 6 || sh.ch < 6 || sh.cl > 12 || sh.ch > 12 || sh.lhc > sh.ch || sh.llc > sh.cl) return false;
    if (sh.cl - sh.llc > 7 || sh.ch - sh.lhc > 7) return false;
    for (uint32_t set = 0; set < sh.nsets; ++set) {
        uint32_t nbr, nbc, shift;
        rc_bits(sh, set, &nbr, &nbc, &shift);
        if (nbr > RC_NB || nbc > RC_NB) return false;
    }
    return true;
}

// pair w of a launch: wavefront w reads a[w], b[w] into the LDS in the limb layout, adds them as one wavefront and packs the
// sum; lane 0 also adds them alone (g1_add)
__global__ __launch_bounds__(256) void add_pairs_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t npairs,
                                                        uint32_t* rows_out, uint32_t* lane_out, uint32_t* slow) {
    __shared__ uint32_t buf[4][3][FQR_POINT_WORDS];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, w = blockIdx.x * 4 + wave;
    if (w >= npairs) return;   // whole wavefronts; no barrier below
    const uint32_t c = lane >> 4, i = lane & 15u;
    buf[wave][0][lane] = fqr_limb_of_words(a + (uint64_t)w * 48 + c * 12, i);
    buf[wave][1][lane] = fqr_limb_of_words(b + (uint64_t)w * 48 + c * 12, i);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const bool s = g1_add_rows<RowsDev>(buf[wave][0], buf[wave][1], buf[wave][2]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    fqr_store_rows<RowsDev>(rows_out + (uint64_t)w * 48, buf[wave][2][lane]);
    if (lane == 0) {
        slow[w] = s ? 1u : 0u;
        st_xyzz(lane_out, w, g1_add(ld_xyzz(a, w), ld_xyzz(b, w)));
    }
}

}  // namespace

// a, b: npairs stored XYZZ points each (48 packed words a point); rows_out: a[w] + b[w] by g1_add_rows, lane_out: by g1_add,
// slow[w]: 1 where g1_add_rows took its slow path.  npairs <= 4096.  Returns the HIP error code.
extern "C" int drr_add_pairs(const uint32_t* a, const uint32_t* b, uint32_t npairs, uint32_t* rows_out, uint32_t* lane_out,
                             uint32_t* slow) {
    if (npairs < 1 || npairs > 4096) return (int)hipErrorInvalidValue;
    Bufs m;
    uint32_t* d_a = m.zeros(npairs);
    uint32_t* d_b = m.zeros(npairs);
    uint32_t* d_r = m.zeros(npairs);
    uint32_t* d_l = m.zeros(npairs);
    uint32_t* d_s = m.zeros((npairs + 47) / 48);
    if (m.err == hipSuccess) m.err = hipMemcpy(d_a, a, (size_t)npairs * 192, hipMemcpyHostToDevice);
    if (m.err == hipSuccess) m.err = hipMemcpy(d_b, b, (size_t)npairs * 192, hipMemcpyHostToDevice);
    if (m.err == hipSuccess) {
        hipLaunchKernelGGL(add_pairs_kernel, dim3((npairs + 3) / 4), dim3(256), 0, 0, d_a, d_b, npairs, d_r, d_l, d_s);
        m.err = hipGetLastError();
    }
    if (m.err == hipSuccess) m.err = hipDeviceSynchronize();
    if (m.err == hipSuccess) m.err = hipMemcpy(rows_out, d_r, (size_t)npairs * 192, hipMemcpyDeviceToHost);
    if (m.err == hipSuccess) m.err = hipMemcpy(lane_out, d_l, (size_t)npairs * 192, hipMemcpyDeviceToHost);
    if (m.err == hipSuccess) m.err = hipMemcpy(slow, d_s, (size_t)npairs * 4, hipMemcpyDeviceToHost);
    return (int)m.err;
}

// shape: {nsets, c1, ch, cl, lhc, llc, top_v}, cl, ch >= 6; buckets: (nsets << c1) * 48 words.
// form 0: the planes one addition per wavefront (launch_msm_rc_reduce); form 1: one thread per point (msm_rc2_planes_kernel).
// planes: nsets * 2 * RC_NB * 48 words (planes the shape does not have stay zero words).
// Returns the HIP error code, hipErrorInvalidValue for a shape the kernels do not take.
extern "C" int drr_reduce(int form, const uint32_t* shape, const uint32_t* buckets, uint32_t* planes) {
    RcShape sh;
    sh.nsets = shape[0];
    sh.c1 = shape[1];
    sh.ch = shape[2];
    sh.cl = shape[3];
    sh.lhc = shape[4];
    sh.llc = shape[5];
    sh.top_v = shape[6];
    if ((form != 0 && form != 1) || !shape_ok(sh) || !msm_rows_ok(sh)) return (int)hipErrorInvalidValue;
    const uint64_t nb = (uint64_t)sh.nsets << sh.c1;
    const uint64_t nrow = (uint64_t)sh.nsets << (sh.c1 - sh.llc), ncol = (uint64_t)sh.nsets << (sh.c1 - sh.lhc);
    const uint64_t nplanes = (uint64_t)sh.nsets * 2 * RC_NB;
    Bufs m;
    uint32_t* d_buckets = m.zeros(nb);
    uint32_t* part_b = m.zeros(nrow);
    uint32_t* part_a = m.zeros(ncol);
    uint32_t* sums = m.zeros(((uint64_t)sh.nsets << sh.ch) + ((uint64_t)sh.nsets << sh.cl));
    uint32_t* bitsum = m.zeros(nplanes * 64);
    uint32_t* d_planes = m.zeros(nplanes);
    if (m.err == hipSuccess) m.err = hipMemcpy(d_buckets, buckets, (size_t)nb * 192, hipMemcpyHostToDevice);
    if (m.err == hipSuccess) {
        launch_msm_rc_reduce_form(d_buckets, sh, part_b, part_a, sums, bitsum, d_planes, form == 0, 0);
        m.err = hipGetLastError();
    }
    if (m.err == hipSuccess) m.err = hipDeviceSynchronize();
    if (m.err == hipSuccess) m.err = hipMemcpy(planes, d_planes, (size_t)nplanes * 192, hipMemcpyDeviceToHost);
    return (int)m.err;
}
