// Test-only device harness over the MSM's bucket reduction (tests/test_gpu_reduce.py).
//
// msm_reduce.hip is compiled here as a unit, exactly as the library compiles it (same flags, no extra defines), and its three
// launchers run on a bucket array the caller chose: nsets << c1 XYZZ points in the packed HBM form (4 x 12 words, st_xyzz).
// The scratch buffers are sized as msm_host.hip sizes them.  Not linked into libtyplonk_hip.so.  It lives beside the unit it
// wraps, not under tests/cpp: the build recipe then depends on nothing in the test tree but the directory its output goes to.
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

// the shapes the kernels' index arithmetic and the fixed-size scratch arrays admit
bool shape_ok(const RcShape& sh, int form) {
    if (sh.nsets < 1 || sh.nsets > 32 || sh.c1 != sh.cl + sh.ch || sh.c1 > 19) return false;
    if (sh.cl < 1 || sh.ch < 1 || sh.cl > 12 || sh.ch > 12 || sh.lhc > sh.ch || sh.llc > sh.cl) return false;
    // msm_fold_seq_kernel folds 2^(cl - llc) row partials (2^(ch - lhc) column partials) with two per lane of ONE wavefront
    if (sh.cl - sh.llc > 7 || sh.ch - sh.lhc > 7) return false;
    for (uint32_t set = 0; set < sh.nsets; ++set) {
        uint32_t nbr, nbc, shift;
        rc_bits(sh, set, &nbr, &nbc, &shift);
        if (nbr > RC_NB || nbc > RC_NB) return false;
    }
    return form != 0 || msm_rc2_ok(sh);
}

}  // namespace

// shape: {nsets, c1, ch, cl, lhc, llc, top_v}; buckets: (nsets << c1) * 48 words.
// form 0: launch_msm_rc2_reduce (needs cl, ch >= 6); form 1: launch_msm_rc_reduce (msm_rc2_planes_kernel for cl, ch >= 6,
// msm_rc_bits_kernel + msm_rc_final_kernel below that).
// planes: nsets * 2 * RC_NB * 48 words, the bit planes (planes the shape does not have stay zero words);
// set_sums: NULL, or nsets * 48 words filled by launch_msm_rc_combine from those planes.
// Returns the HIP error code, hipErrorInvalidValue for a shape the kernels do not take.
extern "C" int dr_reduce(int form, const uint32_t* shape, const uint32_t* buckets, uint32_t* planes, uint32_t* set_sums) {
    RcShape sh;
    sh.nsets = shape[0];
    sh.c1 = shape[1];
    sh.ch = shape[2];
    sh.cl = shape[3];
    sh.lhc = shape[4];
    sh.llc = shape[5];
    sh.top_v = shape[6];
    if ((form != 0 && form != 1) || !shape_ok(sh, form)) return (int)hipErrorInvalidValue;
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
    uint32_t* d_sets = m.zeros(sh.nsets);
    if (m.err == hipSuccess) m.err = hipMemcpy(d_buckets, buckets, (size_t)nb * 192, hipMemcpyHostToDevice);
    if (m.err == hipSuccess) {
        if (form == 0) launch_msm_rc2_reduce(d_buckets, sh, part_b, part_a, d_planes, 0);
        else launch_msm_rc_reduce(d_buckets, sh, part_b, part_a, sums, bitsum, d_planes, 0);
        if (set_sums) launch_msm_rc_combine(d_planes, sh, d_sets, 0);
        m.err = hipGetLastError();
    }
    if (m.err == hipSuccess) m.err = hipDeviceSynchronize();
    if (m.err == hipSuccess) m.err = hipMemcpy(planes, d_planes, (size_t)nplanes * 192, hipMemcpyDeviceToHost);
    if (m.err == hipSuccess && set_sums) m.err = hipMemcpy(set_sums, d_sets, (size_t)sh.nsets * 192, hipMemcpyDeviceToHost);
    return (int)m.err;
}

extern "C" int dr_rc_nb() { return (int)RC_NB; }
