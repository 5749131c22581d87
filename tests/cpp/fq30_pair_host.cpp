// Test-only host build of the paired Fq30 products (tests/test_fq30_pair.py): fq30_mul_pair, fq30_sqr_pair and
// fq30_mul2_add as the host compiles them.  Not linked into libtyplonk_hip.so.
#include <cstddef>

#include "fq30_pair_harness.hpp"

// n cases, arrays of n * 13 limbs; returns 0
extern "C" int fp_host(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out0, uint32_t* out1,
                       int n) {
    for (int t = 0; t < n; ++t) fq30_pair_test::run_case(op, (size_t)t, a, b, c, d, out0, out1);
    return 0;
}
