// kzg::KzgScheme::recover_chunks of the C++ host mirror (typlonk_amd/host/typlonk_host.hpp) -- needs a GPU.
//   two polynomials of 128 coefficients over the domain of 256 points cut into 32 cosets of 8 (KzgScheme::open_chunks): from 20 of
//   their cells each, in no order, the coefficients come back exactly; opened again, the recovered polynomials give the proofs of the
//   originals on every coset, and the cells of the twelve cosets that were NOT given verify in one fold; one changed evaluation
//   makes that polynomial inconsistent and leaves the other exact; bad arguments throw.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../typlonk_amd/host/typlonk_host.hpp"

using namespace typlonk;
using kzg::KzgCell;
using kzg::KzgCellVerdicts;
using kzg::KzgChunkOpening;
using kzg::KzgCommitment;
using kzg::KzgRecovered;
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

static bool same(const Fr& a, const Fr& b) { return std::memcmp(a.limbs(), b.limbs(), 32) == 0; }

int main() {
    Context ctx(0);
    const Fr s = Fr(0x1234567) * Fr(0x89abcdef);
    const uint32_t log_n = 8, log_l = 3;
    const size_t n = (size_t)1 << log_n, l = (size_t)1 << log_l, r = n / l, m = 128, K = 20;
    Srs srs = Srs::from_secret(ctx, s, n);
    Srs table = srs.open_chunks_table(log_n, log_l);
    KzgScheme scheme(srs);
    Fr sl = s;
    for (uint32_t i = 0; i < log_l; ++i) sl = sl * sl;
    const pairing::G2Affine g2sl = pairing::g2_mul(pairing::g2_generator(), sl.v);
    uint8_t seed[32];
    for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(5 * i + 2);

    std::vector<Poly> ps;
    Fr x = Fr(0xdecafbad);
    for (int which = 0; which < 2; ++which) {
        std::vector<Fr> co(m);
        for (size_t i = 0; i < m; ++i) {
            x = x * x + Fr((int64_t)i + 5);
            co[i] = x;
        }
        ps.push_back(Poly::from_coefficients_vec(co));
    }
    const std::vector<KzgCommitment> commitments = {scheme.commit(ps[0]), scheme.commit(ps[1])};
    const std::vector<std::vector<KzgChunkOpening>> all = scheme.open_chunks(table, ps);

    // 20 of the 32 cosets, in no order: k = 7 i + 3 mod 32
    std::vector<uint32_t> cosets;
    std::vector<bool> known(r, false);
    for (size_t i = 0; i < K; ++i) {
        cosets.push_back((uint32_t)((7 * i + 3) % r));
        REQUIRE(!known[cosets.back()]);
        known[cosets.back()] = true;
    }
    std::vector<std::vector<std::vector<Fr>>> cells(2);
    for (size_t p = 0; p < 2; ++p)
        for (uint32_t k : cosets) cells[p].push_back(all[p][k].ys);

    KzgRecovered rec = scheme.recover_chunks(log_n, log_l, m, cosets, cells);
    REQUIRE(rec.all_ok() && rec.report.known == K && rec.report.missing == r - K && rec.status.size() == 2);
    for (size_t p = 0; p < 2; ++p) {
        REQUIRE(rec.first_excess[p] == UINT64_MAX && rec.coeffs[p].size() == m);
        for (size_t i = 0; i < m; ++i) REQUIRE(same(rec.coeffs[p][i], ps[p].coeffs[i]));
    }
    std::puts("recover ok");

    const std::vector<std::vector<KzgChunkOpening>> again = scheme.open_chunks(table, {rec.poly(0), rec.poly(1)});
    for (size_t p = 0; p < 2; ++p)
        for (size_t k = 0; k < r; ++k) {
            REQUIRE(std::memcmp(again[p][k].p.xy, all[p][k].p.xy, 96) == 0 && again[p][k].p.infinity == all[p][k].p.infinity);
            for (size_t t = 0; t < l; ++t) REQUIRE(same(again[p][k].ys[t], all[p][k].ys[t]));
        }
    std::puts("open ok");

    std::vector<KzgCell> lost;   // the cells the call was not given, as recovered
    for (size_t k = 0; k < r; ++k)
        if (!known[k])
            for (uint32_t p = 0; p < 2; ++p) lost.push_back(KzgCell{p, (uint32_t)k, again[p][k]});
    REQUIRE(lost.size() == 2 * (r - K));
    const KzgCellVerdicts v = scheme.verify_chunks(log_n, log_l, g2sl, seed, commitments, lost);
    REQUIRE(v.all_ok() && v.report.folds == 1);
    std::puts("verify ok");

    std::vector<std::vector<std::vector<Fr>>> bad = cells;
    bad[1][4][l - 1] = bad[1][4][l - 1] + Fr::one();
    rec = scheme.recover_chunks(log_n, log_l, m, cosets, bad);
    REQUIRE(!rec.all_ok() && rec.status[0] == TYPLONK_RECOVER_OK && rec.status[1] == TYPLONK_RECOVER_INCONSISTENT);
    REQUIRE(rec.first_excess[0] == UINT64_MAX && rec.first_excess[1] >= m && rec.first_excess[1] < K * l);
    REQUIRE(rec.report.count[TYPLONK_RECOVER_INCONSISTENT] == 1);
    for (size_t i = 0; i < m; ++i) REQUIRE(same(rec.coeffs[0][i], ps[0].coeffs[i]) && same(rec.coeffs[1][i], Fr()));
    rec = scheme.recover_chunks(log_n, log_l, K * l, cosets, bad);   // m = K l: an interpolation of the changed values
    REQUIRE(rec.all_ok());
    int threw = 0;
    try {
        scheme.recover_chunks(log_n, log_l, K * l + 1, cosets, cells);   // too few cells for this degree bound
    } catch (const std::runtime_error&) {
        ++threw;
    }
    try {
        std::vector<uint32_t> twice = cosets;
        twice[5] = twice[0];
        scheme.recover_chunks(log_n, log_l, m, twice, cells);
    } catch (const std::runtime_error&) {
        ++threw;
    }
    try {
        scheme.recover_chunks(log_n, log_n, m, cosets, cells);           // a single coset
    } catch (const std::runtime_error&) {
        ++threw;
    }
    try {
        std::vector<std::vector<std::vector<Fr>>> c2 = cells;
        c2[0][3].pop_back();                                              // l - 1 evaluations
        scheme.recover_chunks(log_n, log_l, m, cosets, c2);
    } catch (const std::runtime_error&) {
        ++threw;
    }
    REQUIRE(threw == 4);
    REQUIRE(scheme.recover_chunks(log_n, log_l, m, cosets, cells).all_ok());
    std::puts("verdicts ok");
    return 0;
}
