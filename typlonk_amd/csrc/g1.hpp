// BLS12-381 G1 group law for the MSM hot path (replaces ark-ec 0.3.0 `add_assign_mixed`,
// `double_in_place`, `From<GroupProjective> for GroupAffine`; reference call sites
// /root/reference/kzg/src/lib.rs:49-52).
//
// E: y^2 = x^3 + 4 (a = 0).  Accumulators use extended-Jacobian "XYZZ" coordinates
// (x = X/ZZ, y = Y/ZZZ, ZZ^3 = ZZZ^2): a mixed add is 8M+2S with no field inversion and bucket
// accumulation is made of nothing else.  The result of an MSM is a group element, and the library
// returns its unique canonical affine form, so the choice of coordinates cannot change a single
// output bit -- provided every exceptional case (identity operand, P+P, P+(-P)) is handled, which
// the functions below do explicitly.
//
// Field values are lazily reduced (fq30.hpp).  Invariants of a stored XYZZ point, in units of p:
//     X < 5.1    Y < 3.2    ZZ, ZZZ < 1.1      (all < 8p < 2^384, so they pack into 12 words)
// Affine points have canonical coordinates (< p).  Each line below carries the bound of its
// result; "m(A,B)" = 1 + A*B/630 is the bound of a Montgomery product of inputs < A p and < B p.
#pragma once
#include "fq30.hpp"

namespace ty {

// Affine point; identity is encoded (0, 0), which is not on the curve (0 != 0 + 4).  The C-ABI's
// separate `inf` flag byte is folded into this form at upload.
struct G1Affine {
    Fq30 x, y;  // canonical, Montgomery R = 2^390
    TY_HD bool is_inf() const { return fq30_is_zero_exact(x) && fq30_is_zero_exact(y); }
    static TY_HD G1Affine inf() {
        G1Affine r;
        r.x = fq30_zero();
        r.y = fq30_zero();
        return r;
    }
};

struct G1Xyzz {
    Fq30 x, y, zz, zzz;
    TY_HD bool is_inf() const { return fq30_is_zero_mod(zz); }
    static TY_HD G1Xyzz inf() {
        G1Xyzz r;
        r.x = fq30_one();
        r.y = fq30_one();
        r.zz = fq30_zero();
        r.zzz = fq30_zero();
        return r;
    }
    static TY_HD G1Xyzz from_affine(const G1Affine& p) {
        if (p.is_inf()) return inf();
        G1Xyzz r;
        r.x = p.x;
        r.y = p.y;
        r.zz = fq30_one();
        r.zzz = fq30_one();
        return r;
    }
};

// r*t - y*w with ONE Montgomery reduction (fq30_mul2_add): r*t + (4p - y)*w.  Needs y <= 4p.
// Result < 1 + (R*T + 4*W)/630 in units of p for r < R, t < T, w < W.
// -DG1_SPLIT_Y3 keeps the two separately reduced products (A/B measurements, tools/ubench2.hip).
TY_HD Fq30 g1_y3(const Fq30& r, const Fq30& t, const Fq30& y, const Fq30& w) {
#if defined(G1_SPLIT_Y3)
    return fq30_sub_lazy<2>(fq30_mul(r, t), fq30_mul(y, w));
#else
    return fq30_mul2_add(r, t, fq30_neg_lazy<4>(y), w);
#endif
}

// 2*(x, y) for an affine non-identity point, x, y < 1.1  (dbl-2008-s-1 with ZZ = ZZZ = 1)
TY_HD G1Xyzz g1_dbl_affine(const Fq30& x, const Fq30& y) {
    G1Xyzz r;
    const Fq30 u = fq30_mulk_lazy<2>(y);                               // < 2.2
    Fq30 v, xx, w, s;
    fq30_sqr_pair(u, x, v, xx);                                        // v: m(2.2,2.2) < 1.01, xx: m(1.1,1.1) < 1.01
    if (fq30_is_zero_mod(v)) return G1Xyzz::inf();                     // y = 0: order-2 point (none on G1)
    fq30_mul_pair(u, v, x, v, w, s);                                   // w, s < 1.01
    const Fq30 m = fq30_mulk_lazy<3>(xx);                              // 3 * 1.01 < 3.1
    r.x = fq30_sub_lazy<3>(fq30_sqr(m), fq30_mulk_lazy<2>(s));         // m(3.1,3.1) + 3 < 4.1   (2s < 2.1 <= 3)
    const Fq30 t = fq30_sub_lazy<5>(s, r.x);                           // 1.01 + 5 < 6.1         (X3 < 4.1 <= 5)
    r.y = g1_y3(m, t, y, w);                                           // < 3.1   (split: m(3.1,6.1) + 2; merged: 1 + (3.1*6.1 + 4*1.01)/630)
    r.zz = v;
    r.zzz = w;
    return r;
}

// 2*P  (dbl-2008-s-1)
TY_HD G1Xyzz g1_dbl(const G1Xyzz& p) {
    if (p.is_inf()) return G1Xyzz::inf();
    G1Xyzz r;
    const Fq30 u = fq30_mulk_lazy<2>(p.y);                             // < 6.4
    Fq30 v, xx, w, s;
    fq30_sqr_pair(u, p.x, v, xx);                                      // v: m(6.4,6.4) < 1.07, xx: m(5.1,5.1) < 1.05
    if (fq30_is_zero_mod(v)) return G1Xyzz::inf();
    fq30_mul_pair(u, v, p.x, v, w, s);                                 // w: m(6.4,1.07) < 1.02, s: m(5.1,1.07) < 1.01
    const Fq30 m = fq30_mulk_lazy<3>(xx);                              // 3 * 1.05 < 3.2
    r.x = fq30_sub_lazy<3>(fq30_sqr(m), fq30_mulk_lazy<2>(s));         // m(3.2,3.2) + 3 < 4.1
    const Fq30 t = fq30_sub_lazy<5>(s, r.x);                           // < 6.1
    r.y = g1_y3(m, t, p.y, w);                                         // < 3.1   (Y < 3.2 <= 4)
    fq30_mul_pair(v, p.zz, w, p.zzz, r.zz, r.zzz);                     // < 1.01 each
    return r;
}

// acc += (qx, qy)   mixed addition, madd-2008-s; qx, qy < 1.1; the affine operand must not be the
// identity (callers test G1Affine::is_inf first).
TY_HD void g1_madd_xy(G1Xyzz& acc, const Fq30& qx, const Fq30& qy) {
    if (acc.is_inf()) {
        acc.x = qx;
        acc.y = qy;
        acc.zz = fq30_one();
        acc.zzz = fq30_one();
        return;
    }
    Fq30 u2, s2, pp, rr, ppp, q;
    fq30_mul_pair(qx, acc.zz, qy, acc.zzz, u2, s2);                    // < 1.01 each
    const Fq30 p = fq30_sub_lazy<6>(u2, acc.x);                        // 1.01 + 6 < 7.1   (X1 < 5.1 <= 6)
    const Fq30 r = fq30_sub_lazy<4>(s2, acc.y);                        // 1.01 + 4 < 5.1   (Y1 < 3.2 <= 4)
    fq30_sqr_pair(p, r, pp, rr);                                       // pp: m(7.1,7.1) < 1.09, rr: m(5.1,5.1) < 1.05
    if (fq30_is_zero_mod(pp)) {                                        // P = 0  <=>  same x
        if (fq30_is_zero_mod(rr)) {                                    // and same y: doubling
            acc = g1_dbl_affine(qx, qy);
        } else {
            acc = G1Xyzz::inf();
        }
        return;
    }
    fq30_mul_pair(p, pp, acc.x, pp, ppp, q);                           // ppp: m(7.1,1.09) < 1.02, q: m(5.1,1.09) < 1.01
    const Fq30 x3 = fq30_sub2_lazy<4>(rr, ppp, fq30_mulk_lazy<2>(q));  // 1.05 + 4 < 5.1  (ppp + 2q < 3.1 <= 4)
    const Fq30 t = fq30_sub_lazy<6>(q, x3);                            // 1.01 + 6 < 7.1
    acc.y = g1_y3(r, t, acc.y, ppp);                                   // < 3.1   (split: m(5.1,7.1) + 2; merged: 1 + (5.1*7.1 + 4*1.02)/630 < 1.07)
    acc.x = x3;
    fq30_mul_pair(acc.zz, pp, acc.zzz, ppp, acc.zz, acc.zzz);          // < 1.01 each
}

// acc += (neg ? -q : q)
TY_HD void g1_madd(G1Xyzz& acc, const G1Affine& q, bool neg) {
    if (q.is_inf()) return;
    const Fq30 qy = neg ? fq30_neg_lazy<1>(q.y) : q.y;                 // p - y <= p
    g1_madd_xy(acc, q.x, qy);
}

// ---- the mixed addition of the accumulation loops (msm_accum.hip) --------------------------------------------------
// g1_madd_xy spends four carry passes and three 26-word zero tests per addition on things the sum does not need.  An
// accumulator that is only ever fed by mixed additions can drop them by carrying two bits beside the point:
//   inf   the sum is the identity (the words of p are then meaningless): replaces ZZ == 0 mod p, tested every addition;
//   flip  the sum is -p, not p.  madd-2008-s ends in Y3 = R (Q - X3) - Y1 PPP, and the subtraction costs a 4p - Y1 pass
//         before the two-product reduction.  With R' = -R = Y1 - S2 instead, R' (Q - X3) + Y1 PPP = -Y3 has two positive
//         terms, and R'^2 = R^2, so X3, ZZ3 and ZZZ3 are those of the sum: the formulas yield -(p + q), which is
//         recorded by toggling flip, and the next point is added with the sign neg ^ flip.
// The sign of the incoming point is applied to S2 inside the R' pass (fq30_addsub_lazy) rather than to qy in a pass of
// its own, and the equal-x test runs in full only when some lane's lowest limb says it may hold.
// g1_acc_finish turns the pair back into a stored XYZZ point (invariants at the top of this file).
struct G1Acc {
    G1Xyzz p;
    uint32_t flags;
};
constexpr uint32_t G1_ACC_INF = 1u, G1_ACC_FLIP = 2u;

// `c` on any active lane of the wavefront (host: this one value)
#if defined(__HIP_DEVICE_COMPILE__)
#define G1_ANY_LANE(c) (__any((int)(c)) != 0)
#else
#define G1_ANY_LANE(c) (c)
#endif

TY_HD G1Acc g1_acc_empty() {
    G1Acc a;
    a.p = G1Xyzz::inf();
    a.flags = G1_ACC_INF;
    return a;
}
// continue from a stored point (flip = 0)
TY_HD G1Acc g1_acc_from(const G1Xyzz& p) {
    G1Acc a;
    a.p = p;
    a.flags = p.is_inf() ? G1_ACC_INF : 0u;
    return a;
}

// acc += (neg ? -q : q);  q canonical (x, y < p) or the identity (0, 0).  With s = neg ^ flip, p takes +-q:
TY_HD void g1_madd_acc(G1Acc& a, const G1Affine& q, bool neg) {
    if (G1_ANY_LANE(q.x.v[0] == 0u)) {                                 // (0, 0) in full only where a lowest limb allows it
        if (q.is_inf()) return;
    }
    if (a.flags & G1_ACC_INF) {                                        // the sum is +-q itself: p = q, flip = neg
        a.p.x = q.x;
        a.p.y = q.y;                                                   // < 1 (so is every Y held with flip set, see below)
        a.p.zz = fq30_one();
        a.p.zzz = fq30_one();
        a.flags = neg ? G1_ACC_FLIP : 0u;
        return;
    }
    const bool s = neg != ((a.flags & G1_ACC_FLIP) != 0);
    Fq30 u2, s2, pp, rr, ppp, qq;
    fq30_mul_pair(q.x, a.p.zz, q.y, a.p.zzz, u2, s2);                  // < 1.01 each
    const Fq30 p = fq30_sub_lazy<6>(u2, a.p.x);                        // 1.01 + 6 < 7.1   (X1 < 5.1 <= 6)
    // R' = Y1 - (s ? -S2 : S2):  s: Y1 + S2 < 3.2 + 1.01;  else Y1 - S2 + 2p < 3.2 + 2   (S2 < 1.01 <= 2)
    const Fq30 r = fq30_addsub_lazy<2>(a.p.y, s2, s);                  // < 5.2
    fq30_sqr_pair(p, r, pp, rr);                                       // pp: m(7.1,7.1) < 1.09, rr: m(5.2,5.2) < 1.05
    fq30_mul_pair(p, pp, a.p.x, pp, ppp, qq);                          // ppp: m(7.1,1.09) < 1.02, q: m(5.1,1.09) < 1.01
    const Fq30 x3 = fq30_sub2_lazy<4>(rr, ppp, fq30_mulk_lazy<2>(qq)); // 1.05 + 4 < 5.1  (ppp + 2q < 3.1 <= 4)
    const Fq30 t = fq30_sub_lazy<6>(qq, x3);                           // 1.01 + 6 < 7.1
    a.p.y = fq30_mul2_add(r, t, a.p.y, ppp);                           // -Y3 < 1 + (5.2*7.1 + 3.2*1.02)/630 < 1.07
    a.p.x = x3;
    fq30_mul_pair(a.p.zz, pp, a.p.zzz, ppp, a.p.zz, a.p.zzz);          // < 1.01 each
    a.flags ^= G1_ACC_FLIP;
    // Same x (P = 0 mod p): the formulas do not apply; they ran on bounded values, harmlessly, and the case shows in
    // their results, so nothing stays alive for it.  ZZ1 != 0, hence P = 0 <=> ZZ3 = ZZ1 P^2 = 0; and then PPP = Q = 0,
    // X3 = R'^2, -Y3 = -R'^3, which is 0 exactly when R' = 0: the same point (double) and not the opposite one (cancel).
    // Both tests are exact (values < 2p) and run only when some lane's lowest limb of ZZ3 says it may be 0 or p.
    if (G1_ANY_LANE(a.p.zz.v[0] == 0u || a.p.zz.v[0] == fq30_kp(1, 0))) {
        if (fq30_is_zero_mod(a.p.zz)) {
            if (fq30_is_zero_mod(a.p.y)) {                             // p was +-q as added: the sum is 2 (neg ? -q : q)
                const Fq30 ny = fq30_neg_lazy<1>(q.y);                 // p - y <= p
                Fq30 y;
#pragma unroll
                for (int i = 0; i < 13; ++i) y.v[i] = neg ? ny.v[i] : q.y.v[i];
                a.p = g1_dbl_affine(q.x, y);                           // Y < 3.1, held with flip = 0
                a.flags = 0u;                                          // (never the identity: #E(Fq) is odd, no point has y = 0)
            } else {
                a.flags = G1_ACC_INF;
            }
        }
    }
}

// The sum as a stored XYZZ point: X < 5.1, Y < 3.2, ZZ, ZZZ < 1.1.  flip is set only by the two paths above that leave
// Y < 1.07 (a stored point and a doubling are held with flip = 0), so 2p - Y < 2 restores the sign within the bound.
TY_HD G1Xyzz g1_acc_finish(const G1Acc& a) {
    const bool inf = (a.flags & G1_ACC_INF) != 0, flip = (a.flags & G1_ACC_FLIP) != 0;
    const Fq30 ny = fq30_neg_lazy<2>(a.p.y);                           // (of meaningless words when inf: not used)
    G1Xyzz r;                                                          // word by word: G1Xyzz::inf() or (X, +-Y, ZZ, ZZZ)
#pragma unroll
    for (int i = 0; i < 13; ++i) {
        r.x.v[i] = inf ? fq30_one_limb(i) : a.p.x.v[i];
        r.y.v[i] = inf ? fq30_one_limb(i) : flip ? ny.v[i] : a.p.y.v[i];
        r.zz.v[i] = inf ? 0u : a.p.zz.v[i];
        r.zzz.v[i] = inf ? 0u : a.p.zzz.v[i];
    }
    return r;
}

// a + b, both XYZZ  (add-2008-s)
TY_HD G1Xyzz g1_add(const G1Xyzz& a, const G1Xyzz& b) {
    if (a.is_inf()) return b;
    if (b.is_inf()) return a;
    Fq30 u1, u2, s1, s2, pp, rr, ppp, q, zz12, zzz12;
    fq30_mul_pair(a.x, b.zz, b.x, a.zz, u1, u2);                       // m(5.1,1.1) < 1.01 each
    fq30_mul_pair(a.y, b.zzz, b.y, a.zzz, s1, s2);                     // < 1.01 each
    const Fq30 p = fq30_sub_lazy<2>(u2, u1);                           // < 3.1
    const Fq30 r = fq30_sub_lazy<2>(s2, s1);                           // < 3.1
    fq30_sqr_pair(p, r, pp, rr);                                       // < 1.02 each
    if (fq30_is_zero_mod(pp)) {
        if (fq30_is_zero_mod(rr)) return g1_dbl(a);
        return G1Xyzz::inf();
    }
    fq30_mul_pair(p, pp, u1, pp, ppp, q);                              // < 1.01 each
    G1Xyzz o;
    o.x = fq30_sub2_lazy<4>(rr, ppp, fq30_mulk_lazy<2>(q));            // m(3.1,3.1) + 4 < 5.1
    const Fq30 t = fq30_sub_lazy<6>(q, o.x);                           // < 7.1
    o.y = g1_y3(r, t, s1, ppp);                                        // < 3.1   (s1 < 1.01 <= 4)
    fq30_mul_pair(a.zz, b.zz, a.zzz, b.zzz, zz12, zzz12);              // < 1.01 each
    fq30_mul_pair(zz12, pp, zzz12, ppp, o.zz, o.zzz);                  // < 1.01 each
    return o;
}

// Canonical affine form (one field inversion).  Identity -> (0, 0).
TY_HD G1Affine g1_to_affine(const G1Xyzz& p) {
    if (p.is_inf()) return G1Affine::inf();
    const Fq30 t = fq30_inv(fq30_mul(p.zz, p.zzz));
    G1Affine r;
    r.x = fq30_canon(fq30_mul(p.x, fq30_mul(t, p.zzz)));  // X / ZZ
    r.y = fq30_canon(fq30_mul(p.y, fq30_mul(t, p.zz)));   // Y / ZZZ
    return r;
}

// ---- Jacobian doubling chains (fixed-base table set-up, srs_gen.hip) ---------------------------------------------------
// (X, Y, Z): x = X/Z^2, y = Y/Z^3.  A run of doublings costs 3S + 2M + one two-product reduction each (~6.0
// multiplication times) against the 8.0 of g1_dbl, and carries ONE denominator, so that a whole column of table entries
// can be normalised with one shared inversion.  Invariants as for XYZZ: X < 5.1, Y < 3.2, Z < 1.1 (units of p).
// Z = 0 (mod p) is the identity.
struct G1Jac {
    Fq30 x, y, z;
    TY_HD bool is_inf() const { return fq30_is_zero_mod(z); }
    static TY_HD G1Jac from_affine(const G1Affine& p) {   // p must not be the identity
        G1Jac r;
        r.x = p.x;
        r.y = p.y;
        r.z = fq30_one();
        return r;
    }
};
// 2*P.  With B = Y^2, V = 4B, S = X V = 4XY^2, M = 3X^2:  X3 = M^2 - 2S,  Y3 = M (S - X3) - 8B^2,  Z3 = 2YZ.
// (The identity doubles to itself: Z3 = 0; the other coordinates are then meaningless but bounded.)
TY_HD G1Jac g1_jac_dbl(const G1Jac& p) {
    G1Jac r;
    const Fq30 b = fq30_sqr(p.y);                                      // m(3.2,3.2) < 1.02
    const Fq30 v = fq30_mulk_lazy<2>(fq30_mulk_lazy<2>(b));            // < 4.1
    const Fq30 s = fq30_mul(p.x, v);                                   // m(5.1,4.1) < 1.04
    const Fq30 m = fq30_mulk_lazy<3>(fq30_sqr(p.x));                   // 3 * m(5.1,5.1) < 3.2
    r.x = fq30_sub_lazy<3>(fq30_sqr(m), fq30_mulk_lazy<2>(s));         // m(3.2,3.2) + 3 < 4.1   (2s < 2.1 <= 3)
    const Fq30 t = fq30_sub_lazy<5>(s, r.x);                           // 1.04 + 5 < 6.1         (X3 < 4.1 <= 5)
    r.y = g1_y3(m, t, fq30_mulk_lazy<2>(b), v);                        // m t - 2b v = m t - 8 b^2:  1 + (3.2*6.1 + 4*4.1)/630 < 1.06   (2b < 2.1 <= 4)
    r.z = fq30_mul(fq30_mulk_lazy<2>(p.y), p.z);                       // m(6.4,1.1) < 1.02
    return r;
}
// the same point in XYZZ form (ZZ = Z^2, ZZZ = Z^3)
TY_HD G1Xyzz g1_jac_to_xyzz(const G1Jac& p) {
    if (p.is_inf()) return G1Xyzz::inf();
    G1Xyzz r;
    r.x = p.x;
    r.y = p.y;
    r.zz = fq30_sqr(p.z);                                              // < 1.01
    r.zzz = fq30_mul(r.zz, p.z);                                       // < 1.01
    return r;
}
// canonical affine form given zinv = 1/Z
TY_HD G1Affine g1_jac_to_affine_with(const G1Jac& p, const Fq30& zinv) {
    const Fq30 zi2 = fq30_sqr(zinv);                                   // < 1.01
    G1Affine r;
    r.x = fq30_canon(fq30_mul(p.x, zi2));
    r.y = fq30_canon(fq30_mul(p.y, fq30_mul(zi2, zinv)));
    return r;
}

// k * P for a small unsigned k, double-and-add.
TY_HD G1Xyzz g1_mul_small(const G1Xyzz& p, uint32_t k) {
    G1Xyzz acc = G1Xyzz::inf();
    for (int b = 31; b >= 0; --b) {
        acc = g1_dbl(acc);
        if ((k >> b) & 1) acc = g1_add(acc, p);
    }
    return acc;
}

}  // namespace ty
