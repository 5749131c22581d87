// Test-only device harness of the paired Fq30 products (tests/test_gpu_fq30_pair.py): fq30_mul_pair, fq30_sqr_pair and
// fq30_mul2_add compiled for gfx950 with the library's flags, so what runs is the interleaved-chain code of fq30_pair.hpp
// that the group law runs.  One thread per case in 64-thread blocks.  Not linked into libtyplonk_hip.so.
#include <hip/hip_runtime.h>

#include "fq30_pair_harness.hpp"

namespace {

__global__ __launch_bounds__(64) void pair_kernel(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d,
                                                  uint32_t* out0, uint32_t* out1, int n) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n) return;
    fq30_pair_test::run_case(op, (size_t)t, a, b, c, d, out0, out1);
}

}  // namespace

// n cases, host arrays of n * 13 limbs; returns the HIP error code (0 on success)
extern "C" int fp_device(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out0, uint32_t* out1,
                         int n) {
    if (n <= 0) return 0;
    const size_t bytes = (size_t)n * 13 * sizeof(uint32_t);
    const uint32_t* host_in[4] = {a, b, c, d};
    uint32_t* dev[6] = {};
    hipError_t err = hipSuccess;
    for (int i = 0; i < 6 && err == hipSuccess; ++i) err = hipMalloc(reinterpret_cast<void**>(&dev[i]), bytes);
    for (int i = 0; i < 4 && err == hipSuccess; ++i) err = hipMemcpy(dev[i], host_in[i], bytes, hipMemcpyHostToDevice);
    for (int i = 4; i < 6 && err == hipSuccess; ++i) err = hipMemset(dev[i], 0, bytes);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(pair_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, op, dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], n);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err == hipSuccess) err = hipMemcpy(out0, dev[4], bytes, hipMemcpyDeviceToHost);
    if (err == hipSuccess) err = hipMemcpy(out1, dev[5], bytes, hipMemcpyDeviceToHost);
    for (int i = 0; i < 6; ++i)
        if (dev[i]) (void)hipFree(dev[i]);
    return (int)err;
}
