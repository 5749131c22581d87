// The verifier's linearisation commitment [r] (plonk/src/proof.rs:441-503) as scalars on its eleven bases, stated once for
// both proof shapes (verify.hip).  Host arithmetic over Fr alone: no HIP, no C ABI, so the g++ test shim compiles it too.
//   [r] = a [q_l] + b [q_r] - c [q_o] + a b [q_m] + [q_c] + (l2 alpha + L0 alpha^2) [Z] - l3 alpha beta Z(zeta w) [sigma_3]
//         - constant P0 - Z_H(zeta) ([t_lo] + zeta^n [t_mid] + zeta^2n [t_hi])
//   l2 = prod_{i<3} (w_i + beta k_i zeta + gamma),   l3 = (a + beta sigma_1 + gamma) (b + beta sigma_2 + gamma),
//   constant = alpha l3 (c + gamma) Z(zeta w) + L0 alpha^2 + pi_signed
// with w = (a, b, c), every evaluation at zeta unless marked, and L0(zeta) = (zeta^n - 1) / (n (zeta - 1)), 1 at zeta = 1.
// pi_signed is PI(zeta) as the shape's prover counted it: + PI(zeta) for the reference, - PI(zeta) for a prover that subtracts
// it (TYPLONK_VERIFY_PI_AS_PROVER, and the compact shape always).
#pragma once
#include "ff.hpp"

namespace ty {

enum LinBase { LIN_QL, LIN_QR, LIN_QO, LIN_QM, LIN_QC, LIN_SIGMA3, LIN_P0, LIN_Z, LIN_T_LO, LIN_T_MID, LIN_T_HI, LIN_BASES };

struct LinCommitIn {
    Fr a, b, c, zw;         // a, b, c at zeta, Z at zeta w
    Fr sigma[2];            // sigma_1, sigma_2 at zeta
    Fr alpha, beta, gamma, zeta, zn;   // zn = zeta^n
    uint64_t n;
    Fr cosets[3];
    Fr pi_signed;
};

inline void lin_commit_scalars(const LinCommitIn& in, Fr (&out)[LIN_BASES]) {
    const Fr adv[3] = {in.a, in.b, in.c};
    Fr l2 = Fr::one();
    for (int i = 0; i < 3; ++i) l2 = fe_mul(l2, fe_add(fe_add(adv[i], fe_mul(fe_mul(in.beta, in.cosets[i]), in.zeta)), in.gamma));
    Fr l3 = Fr::one();
    for (int i = 0; i < 2; ++i) l3 = fe_mul(l3, fe_add(fe_add(adv[i], fe_mul(in.beta, in.sigma[i])), in.gamma));
    const Fr vanish = fe_sub(in.zn, Fr::one());
    Fr l0 = Fr::one();
    if (in.zeta != Fr::one()) {
        Fr nn = Fr::zero();
        nn.v[0] = (uint32_t)in.n;
        nn.v[1] = (uint32_t)(in.n >> 32);
        l0 = fe_mul(vanish, fe_inv(fe_mul(fe_to_mont(nn), fe_sub(in.zeta, Fr::one()))));
    }
    const Fr l0a2 = fe_mul(l0, fe_mul(in.alpha, in.alpha));
    const Fr constant = fe_add(fe_add(fe_mul(in.alpha, fe_mul(fe_mul(l3, fe_add(in.c, in.gamma)), in.zw)), l0a2), in.pi_signed);
    out[LIN_QL] = in.a;
    out[LIN_QR] = in.b;
    out[LIN_QO] = fe_neg(in.c);
    out[LIN_QM] = fe_mul(in.a, in.b);
    out[LIN_QC] = Fr::one();
    out[LIN_SIGMA3] = fe_neg(fe_mul(fe_mul(fe_mul(l3, in.alpha), in.beta), in.zw));
    out[LIN_P0] = fe_neg(constant);
    out[LIN_Z] = fe_add(fe_mul(l2, in.alpha), l0a2);
    out[LIN_T_LO] = fe_neg(vanish);
    out[LIN_T_MID] = fe_neg(fe_mul(vanish, in.zn));
    out[LIN_T_HI] = fe_neg(fe_mul(vanish, fe_mul(in.zn, in.zn)));
}

}  // namespace ty
