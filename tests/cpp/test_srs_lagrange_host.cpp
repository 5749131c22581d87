// kzg::Srs::lagrange / Srs::from_lagrange and kzg::KzgScheme::commit_evaluations of the C++ host mirror
// (typlonk_amd/host/typlonk_host.hpp) -- needs a GPU.
//   the Lagrange SRS has 2^log_n points, keeps the G2 pair and leaves the monomial SRS untouched; its points sum to G
//   (sum_i L_i = 1) and point i weighted by w^i sums to [s]G (sum_i w^i L_i(X) = X); from_lagrange gives the monomial
//   prefix back, point for point; commit_evaluations over the Lagrange SRS equals commit(interpolate) over the monomial
//   one; bad arguments throw.
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
    const Fr s = Fr(0x1234567) * Fr(0x89abcdef);
    const uint32_t log_n = 7;
    const size_t n = (size_t)1 << log_n;
    Srs srs = Srs::from_secret(ctx, s, n);   // n + 3 points
    const std::vector<kzg::G1Point> mono = srs.g1_ref();

    Srs lag = srs.lagrange(log_n);
    REQUIRE(lag.len() == n && lag.g1_ref().size() == n);
    REQUIRE(lag.g2s() == srs.g2s() && lag.g2() == srs.g2());
    REQUIRE(srs.g1_ref() == mono);                                         // the old one is untouched
    const poly::Radix2EvaluationDomain domain(ctx, n);
    {
        std::vector<Fr> ones(n, Fr::one()), roots(n);
        for (size_t i = 0; i < n; ++i) roots[i] = domain.element(i);
        KzgScheme scheme(lag);
        REQUIRE(scheme.commit_evaluations(ones).p == mono[0]);
        REQUIRE(scheme.commit_evaluations(roots).p == mono[1]);
    }
    std::puts("lagrange ok");

    Srs back = lag.from_lagrange(log_n);
    REQUIRE(back.len() == n);
    REQUIRE(back.g1_ref() == std::vector<kzg::G1Point>(mono.begin(), mono.begin() + n));
    REQUIRE(srs.lagrange(3).from_lagrange(3).g1_ref() == std::vector<kzg::G1Point>(mono.begin(), mono.begin() + 8));
    std::puts("from_lagrange ok");

    {
        std::vector<Fr> evals(n);
        Fr x = Fr(0xfeedface);
        for (size_t i = 0; i < n; ++i) {
            x = x * x + Fr((int64_t)i + 3);
            evals[i] = x;
        }
        const Poly p = poly::interpolate(evals, domain);
        REQUIRE(KzgScheme(lag).commit_evaluations(evals) == KzgScheme(srs).commit(p));
        evals.resize(n / 2 + 1);                                           // a short column: the rest is zero
        REQUIRE(KzgScheme(lag).commit_evaluations(evals) == KzgScheme(srs).commit(poly::interpolate(evals, domain)));
    }
    std::puts("commit_evaluations ok");

    int threw = 0;
    try {
        srs.lagrange(8);                    // 256 > 131 points
    } catch (const std::runtime_error&) {
        ++threw;
    }
    try {
        srs.lagrange(26);
    } catch (const std::runtime_error&) {
        ++threw;
    }
    try {
        KzgScheme(lag).commit_evaluations(std::vector<Fr>(n + 1, Fr::one()));
    } catch (const std::runtime_error&) {
        ++threw;
    }
    REQUIRE(threw == 3);
    std::puts("refusals ok");
    return 0;
}
