// Which scalars and points the host driver admits, stated once (host code only): a canonical Fr / Fq residue, a G1 point on
// the curve, [s]G2 on the twist.  Everything is in the C ABI's form (include/typlonk.h): little-endian 64-bit limbs of
// arkworks' Montgomery residues.  Used by verify.hip, point_codec.hip, poly_eval.hip and witness_check.hip.
#pragma once
#include <stdint.h>
#include <string.h>

#include "g1_host64.hpp"
#include "../host/pairing_host.hpp"

namespace tyh {

inline bool fr_canonical(const uint64_t* l) {
    static const uint64_t R[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
    for (int i = 3; i >= 0; --i)
        if (l[i] != R[i]) return l[i] < R[i];
    return false;
}
inline bool fq_canonical(const uint64_t* l) {
    for (int i = 5; i >= 0; --i)
        if (l[i] != ty::h64::P[i]) return l[i] < ty::h64::P[i];
    return false;
}
// y^2 = x^3 + 4 with canonical coordinates (the identity is on the curve)
inline bool g1_on_curve(const uint64_t xy[12], uint8_t inf) {
    namespace h64 = ty::h64;
    if (inf) return true;
    if (!fq_canonical(xy) || !fq_canonical(xy + 6)) return false;
    h64::Fq x, y;
    memcpy(x.v, xy, 48);
    memcpy(y.v, xy + 6, 48);
    const h64::Fq four = typlonk::pairing::q64(typlonk::pairing::fq_from_u64(4));
    return h64::eq(h64::mul(y, y), h64::add(h64::mul(h64::mul(x, x), x), four));
}
// a finite G2 point from its 24 limbs (x.c0 x.c1 y.c0 y.c1): canonical coordinates on the twist
inline bool g2_from_limbs(const uint64_t xy[24], typlonk::pairing::G2Affine* q) {
    for (int i = 0; i < 24; i += 6)
        if (!fq_canonical(xy + i)) return false;
    memcpy(q->x.a.v, xy, 48);
    memcpy(q->x.b.v, xy + 6, 48);
    memcpy(q->y.a.v, xy + 12, 48);
    memcpy(q->y.b.v, xy + 18, 48);
    q->infinity = false;
    return typlonk::pairing::g2_is_on_curve(*q);
}

}  // namespace tyh
