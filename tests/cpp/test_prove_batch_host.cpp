// plonk::CompiledCircuit::prove_batch (typlonk_prove_batch_host through the C ABI) against the mirror's prove() on each
// witness -- needs a GPU.  The circuit is test_verify_host's squaring chain (x_{j+1} = x_j^2 + pi_j).
//   test_prove_batch_host [log_n]   equality of every proof and status, public inputs, an unsatisfied witness
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

static bool same_point(const kzg::G1Point& a, const kzg::G1Point& b) {
    return a.infinity == b.infinity && std::memcmp(a.xy, b.xy, 96) == 0;
}
static bool same_fr(const Fr& a, const Fr& b) { return std::memcmp(a.limbs(), b.limbs(), 32) == 0; }
static bool same_proof(const plonk::Proof& a, const plonk::Proof& b) {
    const kzg::KzgOpening* oa[6] = {&a.a, &a.b, &a.c, &a.permutation.z, &a.permutation.zw, &a.r};
    const kzg::KzgOpening* ob[6] = {&b.a, &b.b, &b.c, &b.permutation.z, &b.permutation.zw, &b.r};
    for (int i = 0; i < 6; ++i)
        if (!same_point(oa[i]->p, ob[i]->p) || !same_fr(oa[i]->y, ob[i]->y)) return false;
    for (int i = 0; i < 3; ++i)
        if (!same_point(a.t[i].p, b.t[i].p)) return false;
    return same_point(a.a_commit.p, b.a_commit.p) && same_point(a.b_commit.p, b.b_commit.p) && same_point(a.c_commit.p, b.c_commit.p) &&
           same_point(a.permutation.commitment.p, b.permutation.commitment.p) && same_fr(a.evaluation_point, b.evaluation_point) &&
           same_fr(a.beta, b.beta) && same_fr(a.gamma, b.gamma) && same_fr(a.alpha, b.alpha);
}

int main(int argc, char** argv) {
    const uint32_t log_n = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 6;
    Context ctx(0);
    const Chain ch(ctx, log_n);
    kzg::Srs srs = kzg::Srs::from_secret(ctx, Fr(0x5EC2E7), ch.gates);
    plonk::CompiledCircuit circuit(srs, log_n, ch.sel, ch.sigma, ch.cosets);
    std::vector<Fr> pi(ch.n);
    pi[0] = Fr(5);
    pi[3] = Fr(-3);
    pi[ch.gates - 1] = Fr(1234567);
    std::vector<std::array<std::vector<Fr>, 3>> adv;
    std::vector<std::vector<Fr>> pis;
    for (int v = 0; v < 5; ++v) {
        adv.push_back(ch.witness(v, v == 1 ? pi : std::vector<Fr>{}));
        pis.push_back(v == 1 ? pi : std::vector<Fr>{});
    }
    adv[3][2][1] = adv[3][2][1] + Fr::one();   // witness 3 violates a gate
    std::vector<int> status;
    const std::vector<plonk::Proof> got = circuit.prove_batch(adv, pis, &status);
    REQUIRE(got.size() == adv.size() && status.size() == adv.size());
    for (size_t k = 0; k < adv.size(); ++k) {
        std::vector<Fr> cols[3] = {adv[k][0], adv[k][1], adv[k][2]};
        if (k == 3) {   // prove() throws for it; the batch reports it and fills its proof, which does not verify
            REQUIRE(status[k] == TYPLONK_ERR_UNSATISFIED);
            bool threw = false;
            try {
                (void)circuit.prove(cols);
            } catch (const std::exception&) {
                threw = true;
            }
            REQUIRE(threw);
            REQUIRE(!circuit.verify(got[k]));
            continue;
        }
        REQUIRE(status[k] == TYPLONK_OK);
        REQUIRE(same_proof(got[k], circuit.prove(cols, pis[k])));
        REQUIRE(circuit.verify(got[k], pis[k], plonk::CompiledCircuit::PublicInputSign::AsProver));
    }
    REQUIRE(circuit.prove_batch({}, {}, &status).empty() && status.empty());
    std::printf("prove_batch agrees with prove ok\n");
    return 0;
}
