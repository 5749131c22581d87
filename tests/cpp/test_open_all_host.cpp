// kzg::Srs::open_all_table and kzg::KzgScheme::open_all of the C++ host mirror (typlonk_amd/host/typlonk_host.hpp) -- needs a
// GPU.
//   a polynomial of degree 63 opened at all 64 points of its domain in one call: opening k equals KzgScheme::open at w^k,
//   point and evaluation; two of them pass KzgScheme::verify against the commitment and a shifted evaluation does not; the
//   table reports 2n records and leaves the SRS untouched; a short polynomial is zero-padded; bad arguments throw.
#include <cstdio>
#include <cstdlib>

#include "../../typlonk_amd/host/typlonk_host.hpp"

using namespace typlonk;
using kzg::KzgOpening;
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
    const Fr s = Fr(0x7654321) * Fr(0x89abcdef);
    const uint32_t log_n = 6;
    const size_t n = (size_t)1 << log_n;
    Srs srs = Srs::from_secret(ctx, s, n);   // n + 3 points
    const std::vector<kzg::G1Point> mono = srs.g1_ref();
    Srs table = srs.open_all_table(log_n);
    REQUIRE(table.len() == 2 * n && table.g1_ref().size() == 2 * n);
    REQUIRE(srs.g1_ref() == mono);                                         // the SRS is untouched
    const poly::Radix2EvaluationDomain domain(ctx, n);
    KzgScheme scheme(srs);

    std::vector<Fr> co(n);
    Fr x = Fr(0xfeedface);
    for (size_t i = 0; i < n; ++i) {
        x = x * x + Fr((int64_t)i + 3);
        co[i] = x;
    }
    const Poly p = Poly::from_coefficients_vec(co);
    REQUIRE(p.degree() == n - 1);
    const std::vector<KzgOpening> all = scheme.open_all(table, p);
    REQUIRE(all.size() == n);
    for (size_t k = 0; k < n; ++k) {
        const KzgOpening one = scheme.open(p, domain.element(k));
        REQUIRE(all[k].p == one.p);
        REQUIRE(all[k].y == one.y);
    }
    {   // a short polynomial: the rest is zero
        co.resize(n / 2 + 1);
        const Poly q = Poly::from_coefficients_vec(co);
        const std::vector<KzgOpening> part = scheme.open_all(table, q);
        for (size_t k : {(size_t)0, (size_t)5, n - 1}) {
            const KzgOpening one = scheme.open(q, domain.element(k));
            REQUIRE(part[k].p == one.p && part[k].y == one.y);
        }
    }
    std::puts("open_all ok");

    const kzg::KzgCommitment c = scheme.commit(p);
    for (size_t k : {(size_t)1, n - 2}) REQUIRE(scheme.verify(c, all[k], domain.element(k)));
    KzgOpening wrong = all[1];
    wrong.y = wrong.y + Fr::one();
    REQUIRE(!scheme.verify(c, wrong, domain.element(1)));
    std::puts("verify ok");

    int threw = 0;
    try {
        srs.open_all_table(7);              // 127 > 67 points
    } catch (const std::runtime_error&) {
        ++threw;
    }
    try {
        srs.open_all_table(0);
    } catch (const std::runtime_error&) {
        ++threw;
    }
    try {
        table.open_all_table(2);            // a table is no source
    } catch (const std::runtime_error&) {
        ++threw;
    }
    try {
        scheme.open_all(srs, p);            // an SRS is no table
    } catch (const std::runtime_error&) {
        ++threw;
    }
    try {
        scheme.open_all(table, Poly::from_coefficients_vec(std::vector<Fr>(n + 1, Fr::one())));
    } catch (const std::runtime_error&) {
        ++threw;
    }
    REQUIRE(threw == 5);
    std::puts("refusals ok");
    return 0;
}
