// PermutationBuilder<3>::build of tests/cpp/circuit_host.hpp (the sequential union of cycles a caller wrote by hand before
// typlonk_circuit_compile_pairs) behind a C entry point, for tools/perm_pairs_time.py: pairs of flat cells in, the 3n-entry
// successor map out.  Built -O2 into tools/_ub/libperm_builder.so by that tool.
#include "../tests/cpp/circuit_host.hpp"

using namespace typlonk::plonk;

extern "C" int perm_builder_build(const uint32_t* pairs, size_t count, uint32_t log_n, uint32_t* perm) {
    const size_t n = (size_t)1 << log_n;
    auto b = PermutationBuilder<3>::with_rows(n);
    for (size_t i = 0; i < count; ++i) {
        const uint32_t l = pairs[2 * i], r = pairs[2 * i + 1];
        if (!b.add_constrain(Tag{l >> log_n, l & (n - 1)}, Tag{r >> log_n, r & (n - 1)})) return -1;
    }
    const Permutation<3> p = b.build(n);
    for (size_t x = 0; x < 3 * n; ++x) perm[x] = (uint32_t)p.perm[x];
    return 0;
}
