// plonk::CompiledCircuit::prove_batch_compact (typlonk_prove_batch_compact_host through the C ABI) against the mirror's
// prove_compact() on each witness -- needs a GPU.  The circuit is test_verify_host's squaring chain (x_{j+1} = x_j^2 + pi_j).
//   test_prove_batch_compact_host [log_n]   every proof is bytewise prove_compact's, with and without public values; an
//                                           unsatisfied witness is reported and the batch verifies except there, in a context
//                                           holding only the vk
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../typlonk_amd/host/typlonk_host.hpp"

using namespace typlonk;

#define REQUIRE(c)                                                          \
    do {                                                                    \
        if (!(c)) {                                                         \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);      \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

struct Chain {
    size_t n, gates;
    std::vector<Fr> sel[5], sigma[3];
    Fr cosets[3] = {Fr(2), Fr(3), Fr(4)};
    Chain(const Context& ctx, uint32_t log_n) : n((size_t)1 << log_n), gates(n - 3) {
        const poly::Radix2EvaluationDomain domain(ctx, n);
        for (auto& v : sel) v.assign(n, Fr::zero());
        for (size_t j = 0; j < gates; ++j) sel[2][j] = sel[3][j] = Fr::one();   // q_o, q_m
        std::vector<size_t> perm(3 * n);
        for (size_t i = 0; i < 3 * n; ++i) perm[i] = i;
        auto cyc = [&](std::vector<size_t> cells) {
            for (size_t u = 0; u < cells.size(); ++u) perm[cells[u]] = cells[(u + 1) % cells.size()];
        };
        cyc({0, n});
        for (size_t j = 0; j + 1 < gates; ++j) cyc({2 * n + j, j + 1, n + j + 1});
        const Fr w = domain.element(1);
        std::vector<Fr> roots(n);
        roots[0] = Fr::one();
        for (size_t j = 1; j < n; ++j) roots[j] = roots[j - 1] * w;
        for (int i = 0; i < 3; ++i) {
            sigma[i].resize(n);
            for (size_t j = 0; j < n; ++j) sigma[i][j] = cosets[perm[j + i * n] / n] * roots[perm[j + i * n] % n];
        }
    }
    // x_0 = 3 + variant, x_{j+1} = x_j^2 + pi_j, blinding rows by `variant`
    std::array<std::vector<Fr>, 3> witness(int variant, const std::vector<Fr>& pi) const {
        std::array<std::vector<Fr>, 3> adv;
        Fr x((int64_t)(3 + variant));
        for (size_t j = 0; j < gates; ++j) {
            adv[0].push_back(x);
            adv[1].push_back(x);
            x = x * x + (j < pi.size() ? pi[j] : Fr::zero());
            adv[2].push_back(x);
        }
        for (int i = 0; i < 3; ++i)
            for (int k = 0; k < 3; ++k) adv[i].push_back(Fr((int64_t)(1000 + 131 * variant + 17 * i + 5 * k)));
        return adv;
    }
};

int main(int argc, char** argv) {
    const uint32_t log_n = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 6;
    std::vector<typlonk_proof_compact> got;
    std::vector<std::vector<Fr>> pis;
    typlonk_vk vk;
    const size_t bad = 3;
    {
        Context ctx(0);
        const Chain ch(ctx, log_n);
        kzg::Srs srs = kzg::Srs::from_secret(ctx, Fr(0x5EC2E7), ch.gates);
        plonk::CompiledCircuit circuit(srs, log_n, ch.sel, ch.sigma, ch.cosets);
        vk = circuit.verifying_key();
        std::vector<std::array<std::vector<Fr>, 3>> adv;
        for (int v = 0; v < 5; ++v) {
            std::vector<Fr> pi;
            if (v == 1) pi = {Fr(5), Fr::zero(), Fr(-3)};
            if (v == 4) pi = {Fr(7)};
            adv.push_back(ch.witness(v, pi));
            pis.push_back(pi);
        }
        adv[bad][2][1] = adv[bad][2][1] + Fr::one();   // witness 3 violates a gate
        std::vector<int> status;
        got = circuit.prove_batch_compact(adv, pis, &status);
        REQUIRE(got.size() == adv.size() && status.size() == adv.size());
        for (size_t k = 0; k < adv.size(); ++k) {
            const std::vector<Fr> cols[3] = {adv[k][0], adv[k][1], adv[k][2]};
            if (k == bad) {   // prove_compact() throws for it; the batch reports it and fills its proof
                REQUIRE(status[k] == TYPLONK_ERR_UNSATISFIED);
                bool threw = false;
                try {
                    (void)circuit.prove_compact(cols, pis[k]);
                } catch (const std::exception&) {
                    threw = true;
                }
                REQUIRE(threw);
                continue;
            }
            REQUIRE(status[k] == TYPLONK_OK);
            const typlonk_proof_compact one = circuit.prove_compact(cols, pis[k]);
            REQUIRE(std::memcmp(&got[k], &one, sizeof(one)) == 0);
        }
        REQUIRE(circuit.prove_batch_compact({}, {}, &status).empty() && status.empty());
    }
    // a fresh context: no SRS, no circuit, only the verifying key
    Context fresh(0);
    std::vector<bool> want(got.size(), true);
    want[bad] = false;
    REQUIRE(plonk::verify_compact(fresh, vk, got, pis) == want);
    std::printf("prove_batch_compact agrees with prove_compact ok\n");
    return 0;
}
