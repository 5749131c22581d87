// kzg::KzgScheme::verify_chunks of the C++ host mirror (typlonk_amd/host/typlonk_host.hpp) -- needs a GPU.
//   two polynomials of degree 63 opened on all 8 cosets of 8 points (KzgScheme::open_chunks): the 16 cells, interleaved, are all
//   accepted in one fold; a cell with one evaluation changed, one paired with its neighbour's coset and one claimed against the
//   other commitment are the only cells rejected, the others stay accepted; the wrong G2 element rejects every cell; bad arguments
//   throw and leave nothing behind.
#include <cstdio>
#include <cstdlib>

#include "../../typlonk_amd/host/typlonk_host.hpp"

using namespace typlonk;
using kzg::KzgCell;
using kzg::KzgCellVerdicts;
using kzg::KzgChunkOpening;
using kzg::KzgCommitment;
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
    const uint32_t log_n = 6, log_l = 3;
    const size_t n = (size_t)1 << log_n, l = (size_t)1 << log_l, r = n / l;
    Srs srs = Srs::from_secret(ctx, s, n);   // n + 3 points
    Srs table = srs.open_chunks_table(log_n, log_l);
    KzgScheme scheme(srs);
    Fr sl = s;
    for (uint32_t i = 0; i < log_l; ++i) sl = sl * sl;
    const pairing::G2Affine g2sl = pairing::g2_mul(pairing::g2_generator(), sl.v);
    uint8_t seed[32];
    for (int i = 0; i < 32; ++i) seed[i] = (uint8_t)(7 * i + 1);

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
    const std::vector<KzgCommitment> commitments = {scheme.commit(ps[0]), scheme.commit(ps[1])};
    const std::vector<std::vector<KzgChunkOpening>> all = scheme.open_chunks(table, ps);
    std::vector<KzgCell> cells;
    for (size_t k = 0; k < r; ++k)
        for (uint32_t p = 0; p < 2; ++p) cells.push_back(KzgCell{p, (uint32_t)k, all[p][k]});
    const size_t N = cells.size();

    KzgCellVerdicts v = scheme.verify_chunks(log_n, log_l, g2sl, seed, commitments, cells);
    REQUIRE(v.status.size() == N && v.all_ok() && v.report.folds == 1 && v.report.live == N);
    std::puts("accept ok");

    std::vector<KzgCell> bad = cells;
    bad[2].opening.ys[l - 1] = bad[2].opening.ys[l - 1] + Fr::one();   // one evaluation
    bad[7].coset = (bad[7].coset + 1) % (uint32_t)r;                    // a neighbour's coset
    bad[13].commitment ^= 1u;                                           // the other commitment
    v = scheme.verify_chunks(log_n, log_l, g2sl, seed, commitments, bad);
    for (size_t i = 0; i < N; ++i)
        REQUIRE(v.status[i] == (i == 2 || i == 7 || i == 13 ? TYPLONK_CELL_BAD_PROOF : TYPLONK_CELL_OK));
    REQUIRE(!v.all_ok() && v.report.count[TYPLONK_CELL_BAD_PROOF] == 3 && v.report.count[TYPLONK_CELL_OK] == N - 3);
    REQUIRE(v.report.folds > 1 && v.report.folds <= 2 * 3 * 4 + 1);    // 2 b ceil(log2 16) + 1
    v = scheme.verify_chunks(log_n, log_l, srs.g2s(), seed, commitments, cells);   // [s]G2 where [s^l]G2 belongs
    REQUIRE(v.report.count[TYPLONK_CELL_BAD_PROOF] == N);
    std::puts("reject ok");

    int threw = 0;
    try {
        scheme.verify_chunks(log_n, log_n, g2sl, seed, commitments, cells);   // a single coset
    } catch (const std::runtime_error&) {
        ++threw;
    }
    try {
        scheme.verify_chunks(log_n, log_l, g2sl, seed, commitments, {});      // no cell
    } catch (const std::runtime_error&) {
        ++threw;
    }
    try {
        KzgScheme(table).verify_chunks(log_n, log_l, g2sl, seed, commitments, cells);   // a table is no SRS
    } catch (const std::runtime_error&) {
        ++threw;
    }
    try {
        std::vector<KzgCell> c2 = cells;
        c2[3].commitment = 2;                                                 // past the commitments
        scheme.verify_chunks(log_n, log_l, g2sl, seed, commitments, c2);
    } catch (const std::runtime_error&) {
        ++threw;
    }
    try {
        std::vector<KzgCell> c2 = cells;
        c2[3].opening.ys.pop_back();                                          // l - 1 evaluations
        scheme.verify_chunks(log_n, log_l, g2sl, seed, commitments, c2);
    } catch (const std::runtime_error&) {
        ++threw;
    }
    REQUIRE(threw == 5);
    REQUIRE(scheme.verify_chunks(log_n, log_l, g2sl, seed, commitments, cells).all_ok());   // and a good call still succeeds
    std::puts("refusals ok");
    return 0;
}
