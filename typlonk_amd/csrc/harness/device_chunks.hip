// Test-only device harness over the kernels of typlonk_open_chunks_* (tests/test_gpu_pointwise_msm.py).
//
// g1_fft.hip is compiled here as a unit, exactly as the library compiles it (same flags, no extra defines).  dc_pointwise_msm runs
// launch_g1_pointwise_msm with the number of slices the caller names -- through the library a small shape only ever reaches the
// largest -- and dc_ntt_stages runs the stages of launch_srs_g1_ntt_batch_stage over blocks at the strides the caller names, with
// the roots the caller hands in.  Points come and go in the SRS's internal form (PT_WORDS words a record).  Every output buffer
// is allocated at exactly the size the launcher may write, followed by a guard band.
// Nothing is launched on a shape a kernel could leave its buffers with: the checks run on the host before the first HIP call.
// Not linked into libtyplonk_hip.so.  It lives beside the unit it wraps, as device_reduce.hip and device_accum.hip do.
#include "../g1_fft.hip"

#include <vector>

using namespace ty;

namespace {

constexpr size_t GUARD_BYTES = 4096;
constexpr int GUARD_FILL = 0xA5;   // every allocation starts out as this byte, body and band

struct Buf {
    void* p = nullptr;
    size_t bytes = 0;
    uint32_t* u32() const { return static_cast<uint32_t*>(p); }
    // n bytes copied from src (or left as the fill), then the band
    hipError_t make(const void* src, size_t n) {
        bytes = n;
        hipError_t e = hipMalloc(&p, n + GUARD_BYTES);
        if (e == hipSuccess) e = hipMemset(p, GUARD_FILL, n + GUARD_BYTES);
        if (e == hipSuccess && src && n) e = hipMemcpy(p, src, n, hipMemcpyHostToDevice);
        return e;
    }
    bool intact(hipError_t& e) const {
        std::vector<unsigned char> band(GUARD_BYTES);
        if (e == hipSuccess) e = hipMemcpy(band.data(), static_cast<char*>(p) + bytes, GUARD_BYTES, hipMemcpyDeviceToHost);
        bool ok = e == hipSuccess;
        for (size_t i = 0; ok && i < GUARD_BYTES; ++i) ok = band[i] == GUARD_FILL;
        return ok;
    }
    ~Buf() {
        if (p) (void)hipFree(p);
    }
};

bool pow2(uint64_t x) { return x && !(x & (x - 1)); }

}  // namespace

extern "C" int dc_guard_bytes() { return (int)GUARD_BYTES; }

// k: (outputs / period) * l * period scalars of 8 CANONICAL words; tab: l * period records; out: outputs records.
// *guard = 1: the band behind the outputs is still the fill.  Returns the HIP error code, hipErrorInvalidValue -- before anything
// touches the device -- for a shape outside the launcher's contract.
extern "C" int dc_pointwise_msm(const uint32_t* k, const uint32_t* tab, uint64_t outputs, uint64_t period, uint32_t l, uint32_t g,
                                uint32_t* out, uint32_t* guard) {
    if (!k || !tab || !out || !guard) return (int)hipErrorInvalidValue;
    if (!pow2(l) || !pow2(g) || g > l || g > 64 || l > (1u << 16)) return (int)hipErrorInvalidValue;
    if (period == 0 || outputs == 0 || outputs % period || outputs > (1u << 20)) return (int)hipErrorInvalidValue;
    Buf d_k, d_tab, d_out;
    hipError_t err = d_k.make(k, (size_t)outputs * l * sizeof(Fr));
    if (err == hipSuccess) err = d_tab.make(tab, (size_t)l * period * PT_WORDS * 4);
    if (err == hipSuccess) err = d_out.make(nullptr, (size_t)outputs * PT_WORDS * 4);
    if (err != hipSuccess) return (int)err;
    launch_g1_pointwise_msm(static_cast<const Fr*>(d_k.p), d_tab.u32(), d_out.u32(), outputs, period, l, g, 0);
    err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err != hipSuccess) return (int)err;
    err = hipMemcpy(out, d_out.p, d_out.bytes, hipMemcpyDeviceToHost);
    *guard = d_out.intact(err) ? 1u : 0u;
    return (int)err;
}

// The same launch `reps` times between events, after one untimed launch, for tools/open_chunks_time.py: msm_ms[reps] the
// milliseconds of launch_g1_pointwise_msm with g slices (g = 0: skipped), mul_ms[reps] (NULL: skipped) those of the same
// launcher at l = 1, g = 1 -- one ladder per record, as the one-point opening runs it -- over the same outputs * l (scalar,
// record) pairs one by one, one launch per polynomial over the whole table: the ladders the joint kernel's sums would cost as
// separate scalar multiplications, without the additions that sum them.
extern "C" int dc_time_pointwise(const uint32_t* k, const uint32_t* tab, uint64_t outputs, uint64_t period, uint32_t l, uint32_t g,
                                 uint32_t reps, float* msm_ms, float* mul_ms) {
    if (!k || !tab || (g && !msm_ms) || reps == 0 || reps > 100) return (int)hipErrorInvalidValue;
    if (!pow2(l) || (g && (!pow2(g) || g > l || g > 64)) || l > (1u << 16)) return (int)hipErrorInvalidValue;
    if (period == 0 || outputs == 0 || outputs % period || outputs * l > (1ull << 26)) return (int)hipErrorInvalidValue;
    const uint64_t polys = outputs / period;
    Buf d_k, d_tab, d_out, d_rec;
    hipError_t err = d_k.make(k, (size_t)outputs * l * sizeof(Fr));
    if (err == hipSuccess) err = d_tab.make(tab, (size_t)l * period * PT_WORDS * 4);
    if (err == hipSuccess) err = d_out.make(nullptr, (size_t)outputs * PT_WORDS * 4);
    if (err == hipSuccess && mul_ms) err = d_rec.make(nullptr, (size_t)l * period * PT_WORDS * 4);
    hipEvent_t a = nullptr, b = nullptr;
    if (err == hipSuccess) err = hipEventCreate(&a);
    if (err == hipSuccess) err = hipEventCreate(&b);
    for (uint32_t it = 0; it <= reps && err == hipSuccess && g; ++it) {
        err = hipEventRecord(a, 0);
        launch_g1_pointwise_msm(static_cast<const Fr*>(d_k.p), d_tab.u32(), d_out.u32(), outputs, period, l, g, 0);
        if (err == hipSuccess) err = hipEventRecord(b, 0);
        if (err == hipSuccess) err = hipEventSynchronize(b);
        if (err == hipSuccess && it) err = hipEventElapsedTime(&msm_ms[it - 1], a, b);
    }
    for (uint32_t it = 0; it <= reps && err == hipSuccess && mul_ms; ++it) {
        err = hipEventRecord(a, 0);
        for (uint64_t p = 0; p < polys; ++p)
            launch_g1_pointwise_msm(static_cast<const Fr*>(d_k.p) + p * l * period, d_tab.u32(), d_rec.u32(), l * period, l * period, 1, 1, 0);
        if (err == hipSuccess) err = hipEventRecord(b, 0);
        if (err == hipSuccess) err = hipEventSynchronize(b);
        if (err == hipSuccess && it) err = hipEventElapsedTime(&mul_ms[it - 1], a, b);
    }
    if (err == hipSuccess) err = hipGetLastError();
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    return (int)err;
}

// `blocks` transforms of 2^l records: block b is src[b * src_stride, + 2^l) and dst[b * dst_stride, + 2^l); roots: l Montgomery Fr
// (8 words each), roots[s - 1] the root stage s applies.  src: (blocks - 1) * src_stride + 2^l records; out: the whole of dst,
// (blocks - 1) * dst_stride + 2^l records, whatever lies between the blocks still the fill byte.
extern "C" int dc_ntt_stages(const uint32_t* src, const uint32_t* roots, uint32_t l, uint64_t blocks, uint64_t src_stride,
                             uint64_t dst_stride, uint32_t* out, uint32_t* guard) {
    if (!src || !roots || !out || !guard) return (int)hipErrorInvalidValue;
    if (l < 1 || l > 16 || blocks < 1 || blocks > 64) return (int)hipErrorInvalidValue;
    const uint64_t n = 1ull << l;
    if (src_stride < n || dst_stride < n || src_stride > (1u << 20) || dst_stride > (1u << 20)) return (int)hipErrorInvalidValue;
    Buf d_src, d_dst;
    hipError_t err = d_src.make(src, (size_t)((blocks - 1) * src_stride + n) * PT_WORDS * 4);
    if (err == hipSuccess) err = d_dst.make(nullptr, (size_t)((blocks - 1) * dst_stride + n) * PT_WORDS * 4);
    if (err != hipSuccess) return (int)err;
    for (uint32_t stage = 1; stage <= l; ++stage) {
        Fr root;
        for (int w = 0; w < 8; ++w) root.v[w] = roots[(stage - 1) * 8 + w];
        launch_srs_g1_ntt_batch_stage(root, l, stage, blocks, d_src.u32(), src_stride, d_dst.u32(), dst_stride, 0);
    }
    err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err != hipSuccess) return (int)err;
    err = hipMemcpy(out, d_dst.p, d_dst.bytes, hipMemcpyDeviceToHost);
    *guard = d_dst.intact(err) ? 1u : 0u;
    return (int)err;
}
