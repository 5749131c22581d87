// Test-only: the paired Fq30 products (fq30.hpp: fq30_mul_pair, fq30_sqr_pair, fq30_mul2_add) over arrays of 13-limb
// operands, shared by the host build (fq30_pair_host.cpp, g++) and the device build (device_pair.hip, hipcc gfx950).
// One case per index; the headers are included exactly as the library's units include them.
#pragma once
#include "../../typlonk_amd/csrc/fq30.hpp"

namespace fq30_pair_test {

using ty::Fq30;

enum { OP_MUL_PAIR = 0, OP_SQR_PAIR = 1, OP_MUL2_ADD = 2 };

TY_HD Fq30 ld(const uint32_t* p) {
    Fq30 r;
    for (int i = 0; i < 13; ++i) r.v[i] = p[i];
    return r;
}
TY_HD void st(uint32_t* p, const Fq30& x) {
    for (int i = 0; i < 13; ++i) p[i] = x.v[i];
}

// case t: operands a, b, c, d (13 limbs each); results: out0 (a*b, a*a, or a*b + c*d reduced), out1 (c*d, c*c, unused)
TY_HD void run_case(int op, size_t t, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out0,
                           uint32_t* out1) {
    const size_t o = t * 13;
    const Fq30 x = ld(a + o), y = ld(b + o), z = ld(c + o), w = ld(d + o);
    Fq30 r0 = ty::fq30_zero(), r1 = ty::fq30_zero();
    switch (op) {
        case OP_MUL_PAIR: ty::fq30_mul_pair(x, y, z, w, r0, r1); break;
        case OP_SQR_PAIR: ty::fq30_sqr_pair(x, z, r0, r1); break;
        case OP_MUL2_ADD: r0 = ty::fq30_mul2_add(x, y, z, w); break;
        default: break;
    }
    st(out0 + o, r0);
    st(out1 + o, r1);
}

}  // namespace fq30_pair_test
