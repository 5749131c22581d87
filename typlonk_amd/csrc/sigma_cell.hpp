// One cell of Permutation::compile (permutation/src/lib.rs:101-128): the sigma evaluation of a cell whose successor is the
// flat cell y = col * n + row, sigma = k_col * w^row.  Shared by sigma_from_perm_kernel (witness_check.hip) and the host
// (typlonk_amd/host, tests/cpp/sigma_cell_host.cpp), like the bodies of point_codec.hpp and scan_ops.hpp.
//
// w^row comes from the two-level tables get_pow2l builds for the domain root (h = (log_n + 1) / 2):
//   lo[j] = w^j for j < 2^h,   hi[j] = w^(j 2^h) for j < 2^(log_n - h),   w^row = hi[row >> h] * lo[row & (2^h - 1)]
// so a cell costs two field products.  fe_mul returns the canonical residue for canonical operands (its closing conditional
// subtraction), the tables and the cosets are canonical, and so is every value written: a circuit compiled from a
// permutation holds word for word what one loaded from the interpolated sigma columns holds.
#pragma once
#include "ff.hpp"

namespace ty {

struct SigmaTables {
    const Fr* lo;      // 2^h entries
    const Fr* hi;      // 2^(log_n - h) entries
    uint32_t h, log_n;
    Fr k[3];           // the cosets k_0 k_1 k_2, canonical Montgomery residues
};

// false (and *out untouched) when y is no cell: y >= 3n
TY_HD bool sigma_cell(const SigmaTables& t, uint32_t y, Fr* out) {
    const uint32_t col = y >> t.log_n;
    if (col >= 3) return false;
    const uint32_t row = y & ((1u << t.log_n) - 1);
    // (16 bytes: what both hipMalloc and the host allocator guarantee; the device reads an element as two 16-byte loads)
    const Fr* lo = static_cast<const Fr*>(__builtin_assume_aligned(t.lo, 16));
    const Fr* hi = static_cast<const Fr*>(__builtin_assume_aligned(t.hi, 16));
    const Fr w = fe_mul(hi[row >> t.h], lo[row & ((1u << t.h) - 1)]);
    *out = fe_mul(col == 0 ? t.k[0] : (col == 1 ? t.k[1] : t.k[2]), w);
    return true;
}

}  // namespace ty
