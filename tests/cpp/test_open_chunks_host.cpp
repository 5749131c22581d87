// kzg::Srs::open_chunks_table and kzg::KzgScheme::open_chunks of the C++ host mirror (typlonk_amd/host/typlonk_host.hpp) -- needs
// a GPU.
//   two polynomials of degree 63 opened on all 8 cosets of 8 points of their domain in one call: proof k equals the commitment to
//   the quotient by X^l - w^(k l), divided out on the host, and the l evaluations are f at w^(k + r t) in that order; a table of
//   log_l = 0 gives KzgScheme::open_all's openings; the table reports 2n records and its log_l and leaves the SRS untouched; a
//   short polynomial is zero-padded; bad arguments throw.
#include <cstdio>
#include <cstdlib>

#include "../../typlonk_amd/host/typlonk_host.hpp"

using namespace typlonk;
using kzg::KzgChunkOpening;
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

// f = q (X^l - a) + I, deg I < l: the quotient, schoolbook from the top coefficient down
static Poly quotient(std::vector<Fr> f, size_t l, const Fr& a) {
    std::vector<Fr> q(f.size() > l ? f.size() - l : 0);
    for (size_t i = f.size(); i-- > l;) {
        q[i - l] = f[i];
        f[i - l] = f[i - l] + a * f[i];
    }
    return Poly::from_coefficients_vec(q);
}

static void check(const KzgScheme& scheme, const poly::Radix2EvaluationDomain& domain, const Poly& p, const std::vector<KzgChunkOpening>& got,
                  size_t l, size_t r) {
    REQUIRE(got.size() == r);
    for (size_t k = 0; k < r; ++k) {
        REQUIRE(got[k].p == scheme.commit(quotient(p.coeffs, l, domain.element(k * l))).p);
        REQUIRE(got[k].ys.size() == l);
        for (size_t t = 0; t < l; ++t) REQUIRE(got[k].ys[t] == p.evaluate(domain.element(k + r * t)));
    }
}

int main() {
    Context ctx(0);
    const Fr s = Fr(0x7654321) * Fr(0x89abcdef);
    const uint32_t log_n = 6, log_l = 3;
    const size_t n = (size_t)1 << log_n, l = (size_t)1 << log_l, r = n / l;
    Srs srs = Srs::from_secret(ctx, s, n);   // n + 3 points
    const std::vector<kzg::G1Point> mono = srs.g1_ref();
    Srs table = srs.open_chunks_table(log_n, log_l);
    REQUIRE(table.len() == 2 * n && table.g1_ref().size() == 2 * n && table.chunk_log_l() == log_l);
    REQUIRE(srs.g1_ref() == mono);                                         // the SRS is untouched
    const poly::Radix2EvaluationDomain domain(ctx, n);
    KzgScheme scheme(srs);

    std::vector<Poly> ps;
    Fr x = Fr(0xfeedface);
    for (int which = 0; which < 2; ++which) {
        std::vector<Fr> co(n);
        for (size_t i = 0; i < n; ++i) {
            x = x * x + Fr((int64_t)i + 3);
            co[i] = x;
        }
        ps.push_back(Poly::from_coefficients_vec(co));
    }
    const std::vector<std::vector<KzgChunkOpening>> all = scheme.open_chunks(table, ps);
    REQUIRE(all.size() == 2);
    for (int which = 0; which < 2; ++which) check(scheme, domain, ps[which], all[which], l, r);
    {   // a short polynomial: the rest is zero
        std::vector<Fr> co(ps[0].coeffs.begin(), ps[0].coeffs.begin() + (n / 2 + 1));
        const Poly q = Poly::from_coefficients_vec(co);
        check(scheme, domain, q, scheme.open_chunks(table, {q})[0], l, r);
    }
    {   // one point per coset: open_all's openings, from a table of either constructor
        const std::vector<KzgOpening> want = scheme.open_all(srs.open_all_table(log_n), ps[0]);
        const Srs t0 = srs.open_chunks_table(log_n, 0);
        REQUIRE(t0.g1_ref() == srs.open_all_table(log_n).g1_ref());
        const std::vector<KzgChunkOpening> got = scheme.open_chunks(t0, {ps[0]})[0];
        REQUIRE(got.size() == n);
        for (size_t k = 0; k < n; ++k) REQUIRE(got[k].p == want[k].p && got[k].ys.size() == 1 && got[k].ys[0] == want[k].y);
        const std::vector<KzgOpening> again = scheme.open_all(t0, ps[0]);
        for (size_t k = 0; k < n; ++k) REQUIRE(again[k].p == want[k].p && again[k].y == want[k].y);
    }
    std::puts("open_chunks ok");

    int threw = 0;
    try {
        srs.open_chunks_table(7, 2);        // 124 > 67 points
    } catch (const std::runtime_error&) {
        ++threw;
    }
    try {
        srs.open_chunks_table(6, 6);        // a single coset
    } catch (const std::runtime_error&) {
        ++threw;
    }
    try {
        table.open_chunks_table(2, 1);      // a table is no source
    } catch (const std::runtime_error&) {
        ++threw;
    }
    try {
        scheme.open_chunks(srs, ps);        // an SRS is no table
    } catch (const std::runtime_error&) {
        ++threw;
    }
    try {
        scheme.open_all(table, ps[0]);      // open_all takes the tables of one point per coset only
    } catch (const std::runtime_error&) {
        ++threw;
    }
    try {
        scheme.open_chunks(table, {Poly::from_coefficients_vec(std::vector<Fr>(n + 1, Fr::one()))});
    } catch (const std::runtime_error&) {
        ++threw;
    }
    try {
        scheme.open_chunks(table, {ps[0], Poly::from_coefficients_vec(std::vector<Fr>(n - 1, Fr::one()))});   // two lengths
    } catch (const std::runtime_error&) {
        ++threw;
    }
    REQUIRE(threw == 7);
    std::puts("refusals ok");
    return 0;
}
