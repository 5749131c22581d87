// Test-only host build of sigma_cell (typlonk_amd/csrc/sigma_cell.hpp), the per-cell body of sigma_from_perm_kernel, as the
// host compiles it (tests/test_circuit_compile_host.py).  Not linked into libtyplonk_hip.so.
#include <cstddef>
#include <cstring>
#include <vector>

#include "../../typlonk_amd/csrc/sigma_cell.hpp"

using namespace ty;

// root: the generator of the size-2^log_n domain, cosets: k_0 k_1 k_2 (8 words each, canonical Montgomery residues); the two-level
// tables are built here as get_pow2l builds them.  perm: 3n entries.  out: 3n * 8 words, cell[x] = 1 where perm[x] is a cell
// (out[x] is left alone elsewhere).  Returns h.
extern "C" int sigma_cells_host(uint32_t log_n, const uint32_t* root, const uint32_t* cosets, const uint32_t* perm, uint32_t* out,
                                unsigned char* cell) {
    SigmaTables t{};
    t.log_n = log_n;
    t.h = (log_n + 1) / 2;
    Fr w;
    std::memcpy(w.v, root, sizeof(w.v));
    for (int i = 0; i < 3; ++i) std::memcpy(t.k[i].v, cosets + 8 * i, sizeof(t.k[i].v));
    std::vector<Fr> lo((size_t)1 << t.h), hi((size_t)1 << (log_n - t.h));
    Fr x = Fr::one();
    for (Fr& v : lo) {
        v = x;
        x = fe_mul(x, w);
    }
    const Fr step = x;   // w^(2^h)
    x = Fr::one();
    for (Fr& v : hi) {
        v = x;
        x = fe_mul(x, step);
    }
    t.lo = lo.data();
    t.hi = hi.data();
    const size_t n3 = (size_t)3 << log_n;
    for (size_t c = 0; c < n3; ++c) {
        Fr v;
        cell[c] = sigma_cell(t, perm[c], &v) ? 1 : 0;
        if (cell[c]) std::memcpy(out + 8 * c, v.v, sizeof(v.v));
    }
    return (int)t.h;
}
