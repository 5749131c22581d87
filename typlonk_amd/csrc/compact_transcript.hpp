// Fiat-Shamir transcript of the compact proof shape (include/typlonk.h, typlonk_prove_compact), host side.  Shared by the
// prover (prover.hip), the verifier and typlonk_compact_challenges (verify.hip); restated in Python by tests/compact_ref.py.
//   d0 = Blake2b-512("typlonk/compact/v1" || vk_bytes || u64 pi_len || pi), T = d0, then T ||= points / evaluations and
//   challenge = H(T || label), H = Blake2b-512 read as a little-endian integer mod r.
// Unlike transcript.hpp (the reference's ChallengeGenerator) every value the verifier uses is hashed before the challenge
// that depends on it, the quotient commitments and the statement included.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/typlonk.h"
#include "transcript.hpp"

namespace ty {

// the 64-byte digest as a little-endian integer mod r
inline Fr fr_from_digest(const uint8_t h[64]) {
    auto from_u64 = [](uint64_t x) {
        Fr c = Fr::zero();
        c.v[0] = (uint32_t)x;
        c.v[1] = (uint32_t)(x >> 32);
        return fe_to_mont(c);
    };
    const Fr two32 = from_u64(1ull << 32), two64 = fe_mul(two32, two32);
    Fr acc = Fr::zero();
    for (int w = 7; w >= 0; --w) {
        uint64_t d = 0;
        for (int b = 7; b >= 0; --b) d = (d << 8) | h[8 * w + b];
        acc = fe_add(fe_mul(acc, two64), fe_add(fe_mul(from_u64(d >> 32), two32), from_u64(d & 0xffffffffull)));
    }
    return acc;
}

inline void compact_put_u64(std::vector<uint8_t>& b, uint64_t v, int bytes = 8) {
    for (int i = 0; i < bytes; ++i) b.push_back((uint8_t)(v >> (8 * i)));
}
// an Fr given as 4 Montgomery limbs -> 32 bytes of its canonical integer
inline void compact_put_fr(std::vector<uint8_t>& b, const uint64_t l[4]) {
    Fr m;
    memcpy(m.v, l, 32);
    const Fr c = fe_from_mont(m);
    const uint8_t* p = (const uint8_t*)c.v;   // little-endian host
    b.insert(b.end(), p, p + 32);
}
inline void compact_put_point(std::vector<uint8_t>& b, const uint64_t xy[12], uint8_t inf) {
    uint8_t rec[96];
    serialize_unchecked_g1(xy, inf, rec);
    b.insert(b.end(), rec, rec + 96);
}

// vk_bytes = u32 log_n || k_0 || k_1 || k_2 || the eight commitments || P0   (g2s is not part of the statement)
inline void compact_vk_bytes(const typlonk_vk& vk, std::vector<uint8_t>& b) {
    compact_put_u64(b, vk.log_n, 4);
    for (int i = 0; i < 3; ++i) compact_put_fr(b, vk.cosets[i]);
    for (int i = 0; i < 8; ++i) compact_put_point(b, vk.commit_xy[i], vk.commit_inf[i]);
    compact_put_point(b, vk.srs0_xy, vk.srs0_inf);
}

inline void compact_statement_digest(const typlonk_vk& vk, const uint64_t* pi, size_t pi_len, uint8_t d0[64]) {
    static const char tag[] = "typlonk/compact/v1";
    std::vector<uint8_t> b(tag, tag + sizeof(tag) - 1);
    b.reserve(b.size() + 4 + 3 * 32 + 9 * 96 + 8 + 32 * pi_len);
    compact_vk_bytes(vk, b);
    compact_put_u64(b, pi_len);
    for (size_t i = 0; i < pi_len; ++i) compact_put_fr(b, pi + 4 * i);
    blake2b_512(b.data(), b.size(), d0);
}

struct CompactTranscript {
    std::vector<uint8_t> t;
    explicit CompactTranscript(const uint8_t d0[64]) : t(d0, d0 + 64) {}
    void point(const uint64_t xy[12], uint8_t inf) { compact_put_point(t, xy, inf); }
    void scalar(const uint64_t l[4]) { compact_put_fr(t, l); }
    Fr squeeze(char label) {
        t.push_back((uint8_t)label);
        uint8_t h[64];
        blake2b_512(t.data(), t.size(), h);
        t.pop_back();
        return fr_from_digest(h);
    }
};

// the five challenges of a proof, in the order beta, gamma, alpha, zeta, v
inline void compact_challenges(const uint8_t d0[64], const typlonk_proof_compact& pr, Fr out[5]) {
    CompactTranscript tr(d0);
    for (int i = 0; i < 3; ++i) tr.point(pr.commit_xy[i], pr.commit_inf[i]);
    out[0] = tr.squeeze('b');
    out[1] = tr.squeeze('g');
    tr.point(pr.z_xy, pr.z_inf);
    out[2] = tr.squeeze('a');
    for (int i = 0; i < 3; ++i) tr.point(pr.t_xy[i], pr.t_inf[i]);
    out[3] = tr.squeeze('z');
    for (int i = 0; i < 7; ++i) tr.scalar(pr.evals[i]);
    out[4] = tr.squeeze('v');
}

}  // namespace ty
