// plonk::CompiledCircuit::prove_compact / verifying_key and plonk::verify_compact (typlonk_prove_compact_host,
// typlonk_circuit_vk, typlonk_verify_compact through the C ABI) -- needs a GPU.  The circuit is test_verify_host's squaring
// chain (x_{j+1} = x_j^2 + pi_j).
//   test_compact_host [log_n]   proofs with and without public values verify in a context holding only the vk; the
//                               challenges equal typlonk_compact_challenges; tampering and an unsatisfied witness fail
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
    std::vector<typlonk_proof_compact> proofs;
    std::vector<std::vector<Fr>> pis;
    typlonk_vk vk;
    {
        Context ctx(0);
        const Chain ch(ctx, log_n);
        kzg::Srs srs = kzg::Srs::from_secret(ctx, Fr(0x5EC2E7), ch.gates);
        plonk::CompiledCircuit circuit(srs, log_n, ch.sel, ch.sigma, ch.cosets);
        vk = circuit.verifying_key();
        REQUIRE(vk.log_n == log_n);
        for (int v = 0; v < 4; ++v) {
            std::vector<Fr> pi;
            if (v & 1) pi = {Fr(5), Fr::zero(), Fr(-3)};
            const std::array<std::vector<Fr>, 3> adv = ch.witness(v, pi);
            const std::vector<Fr> cols[3] = {adv[0], adv[1], adv[2]};
            proofs.push_back(circuit.prove_compact(cols, pi));
            pis.push_back(pi);
            // the challenges the prover drew are the transcript's
            uint64_t chal[5][4];
            REQUIRE(typlonk_compact_challenges(&vk, &proofs.back(), pi.empty() ? nullptr : pi[0].limbs(), pi.size(), chal) == 0);
            REQUIRE(std::memcmp(chal[0], proofs.back().beta, 32) == 0 && std::memcmp(chal[4], proofs.back().v, 32) == 0);
        }
        REQUIRE(plonk::verify_compact(ctx, vk, proofs, pis) == std::vector<bool>(4, true));
        // a witness that violates a gate throws, as prove() does
        std::array<std::vector<Fr>, 3> adv = ch.witness(7, {});
        adv[2][1] = adv[2][1] + Fr::one();
        const std::vector<Fr> cols[3] = {adv[0], adv[1], adv[2]};
        bool threw = false;
        try {
            (void)circuit.prove_compact(cols);
        } catch (const std::exception&) {
            threw = true;
        }
        REQUIRE(threw);
    }
    // a fresh context: no SRS, no circuit, only the verifying key
    Context fresh(0);
    REQUIRE(plonk::verify_compact(fresh, vk, proofs, pis) == std::vector<bool>(4, true));
    std::vector<typlonk_proof_compact> bad = proofs;
    bad[1].evals[2][0] ^= 1;                 // c(zeta) changed
    std::vector<std::vector<Fr>> other = pis;
    other[2] = {Fr(1)};                      // proof 2 under another statement
    REQUIRE(plonk::verify_compact(fresh, vk, bad, other) == std::vector<bool>({true, false, false, true}));
    REQUIRE(plonk::verify_compact(fresh, vk, {}, {}).empty());
    std::printf("compact mirror ok\n");
    return 0;
}
