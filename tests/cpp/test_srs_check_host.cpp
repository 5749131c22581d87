// kzg::Srs::check and kzg::Srs::contribute of the C++ host mirror (typlonk_amd/host/typlonk_host.hpp) -- needs a GPU.
//   a generated SRS checks against its own g2s; the contribution is the SRS of s t, point for point, carries [s t]G2, and
//   checks against it -- not against the old [s]G2; a KZG opening made on the contributed SRS verifies with its G2 pair;
//   an SRS loaded from points 2G, 2sG, .. is refused for its point 0; bad arguments throw.
#include <cstdio>
#include <cstdlib>

#include "../../typlonk_amd/host/typlonk_host.hpp"

using namespace typlonk;
using kzg::KzgScheme;
using kzg::Poly;
using kzg::Srs;

#define REQUIRE(c)                                                          \
    do {                                                                    \
        if (!(c)) {                                                         \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);      \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

int main() {
    Context ctx(0);
    uint8_t seed[32];
    for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(17 * i + 3);
    const Fr s = Fr(0x1234567) * Fr(0x89abcdef), t = Fr(0xfeedface) * Fr(0x0badc0de);
    const size_t gates = 127;   // 130 points

    Srs srs = Srs::from_secret(ctx, s, gates);
    typlonk_srs_report rep = srs.check(seed);
    REQUIRE(rep.verdict == TYPLONK_SRS_VALID && rep.folds == 1 && rep.bad_points == 0);
    std::puts("check ok");

    Srs mine = srs.contribute(t);
    REQUIRE(mine.len() == srs.len());
    Srs want = Srs::from_secret(ctx, s * t, gates);
    REQUIRE(mine.g1_ref() == want.g1_ref());
    REQUIRE(mine.g2s() == want.g2s() && mine.g2() == want.g2());
    REQUIRE(srs.g1_ref() == Srs::from_secret(ctx, s, gates).g1_ref());   // the old one is untouched
    rep = mine.check(seed);
    REQUIRE(rep.verdict == TYPLONK_SRS_VALID);
    mine.set_g2(srs.g2(), srs.g2s());                                      // the old [s]G2 beside the new points
    rep = mine.check(seed);
    REQUIRE(rep.verdict == TYPLONK_SRS_BAD_RATIO && rep.index == 0);
    mine.set_g2(want.g2(), want.g2s());
    {
        KzgScheme scheme(mine);
        Poly poly = Poly::from_coefficients_slice({Fr(5), Fr(7), Fr(11), Fr(13)});
        auto c = scheme.commit(poly);
        auto o = scheme.open(poly, Fr(99));
        REQUIRE(scheme.verify(c, o, Fr(99)));
    }
    std::puts("contribute ok");

    // [2 s^i] G: every link holds, point 0 is not the generator
    std::vector<kzg::G1Point> pts = srs.g1_ref();
    for (auto& p : pts) p = kzg::g1_mul(ctx, p, Fr(2));
    Srs doubled = Srs::from_points(ctx, pts);
    doubled.set_g2(srs.g2(), srs.g2s());
    rep = doubled.check(seed);
    REQUIRE(rep.verdict == TYPLONK_SRS_BAD_P0 && rep.folds == 0);
    // one bad link
    pts = srs.g1_ref();
    pts[64] = kzg::g1_add(pts[64], pts[0]);
    Srs broken = Srs::from_points(ctx, pts);
    broken.set_g2(srs.g2(), srs.g2s());
    rep = broken.check(seed);
    REQUIRE(rep.verdict == TYPLONK_SRS_BAD_RATIO && rep.index == 63 && rep.folds >= 2 && rep.folds <= 1 + 8);
    std::puts("verdicts ok");

    bool threw = false;
    try {
        srs.contribute(Fr(0));
    } catch (const std::runtime_error&) {
        threw = true;
    }
    REQUIRE(threw);
    threw = false;
    try {
        Srs::from_points(ctx, pts).check(seed);   // no G2 elements
    } catch (const std::runtime_error&) {
        threw = true;
    }
    REQUIRE(threw);
    std::puts("refusals ok");
    return 0;
}
