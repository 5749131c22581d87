// plonk::CompiledCircuit::verify_batch (typlonk_verify through the C ABI) against the mirror's own verify, which stays the
// independent per-proof check (host pairings, host Horner) -- needs a GPU.  The circuit is test_plonk_host's squaring chain.
//   test_verify_host [log_n]                   agreement: valid proofs, a tampered one, public inputs under both signs
//   test_verify_host bench log_n c1 [c2 ...]   timing: verify_batch of c proofs (16 distinct proofs repeated), with the
//                                              stage split of typlonk_profile_get, and the mirror's verify of one proof
#include <chrono>
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

static double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

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
    // x_{j+1} = x_j^2 + pi_j, blinding rows by `variant`
    void witness(int variant, const std::vector<Fr>& pi, std::vector<Fr> (&adv)[3]) const {
        Fr x(3);
        for (auto& a : adv) a.clear();
        for (size_t j = 0; j < gates; ++j) {
            adv[0].push_back(x);
            adv[1].push_back(x);
            x = x * x + (j < pi.size() ? pi[j] : Fr::zero());
            adv[2].push_back(x);
        }
        for (int i = 0; i < 3; ++i)
            for (int k = 0; k < 3; ++k) adv[i].push_back(Fr((int64_t)(1000 + 131 * variant + 17 * i + 5 * k)));
    }
};

int main(int argc, char** argv) {
    const bool bench = argc > 1 && std::strcmp(argv[1], "bench") == 0;
    const uint32_t log_n = bench ? (uint32_t)std::atoi(argv[2]) : (argc > 1 ? (uint32_t)std::atoi(argv[1]) : 6);
    Context ctx(0);
    const Chain ch(ctx, log_n);
    const Fr s(0x5EC2E7);
    kzg::Srs srs = kzg::Srs::from_secret(ctx, s, ch.gates);
    plonk::CompiledCircuit circuit(srs, log_n, ch.sel, ch.sigma, ch.cosets);
    using Sign = plonk::CompiledCircuit::PublicInputSign;
    std::vector<Fr> adv[3];
    if (!bench) {
        std::vector<plonk::Proof> proofs;
        for (int v = 0; v < 5; ++v) {
            ch.witness(v, {}, adv);
            proofs.push_back(circuit.prove(adv));
        }
        for (const auto& p : proofs) REQUIRE(circuit.verify(p));
        std::vector<bool> got = circuit.verify_batch(proofs);
        for (bool b : got) REQUIRE(b);
        // one tampered proof: both verifiers reject it, and only it
        plonk::Proof bad = proofs[2];
        bad.b.y = bad.b.y + Fr::one();
        REQUIRE(!circuit.verify(bad));
        proofs[2] = bad;
        got = circuit.verify_batch(proofs);
        for (size_t k = 0; k < proofs.size(); ++k) REQUIRE(got[k] == (k != 2));
        // public inputs: the two signs of the mirror's verify, proof by proof
        std::vector<Fr> pi(ch.n);
        pi[0] = Fr(5);
        pi[3] = Fr(-3);
        pi[ch.gates - 1] = Fr(1234567);
        ch.witness(0, pi, adv);
        const plonk::Proof pp = circuit.prove(adv, pi);
        for (Sign sg : {Sign::AsReference, Sign::AsProver}) {
            const bool want = circuit.verify(pp, pi, sg);
            REQUIRE(want == (sg == Sign::AsProver));
            const std::vector<bool> b = circuit.verify_batch({pp, proofs[0]}, {pi, {}}, sg);
            REQUIRE(b[0] == want && b[1]);
            REQUIRE(!circuit.verify_batch({pp}, {}, sg)[0]);
        }
        std::printf("verify_batch agrees with verify ok\n");
        return 0;
    }
    // ---- timing ----
    std::vector<plonk::Proof> distinct;
    for (int v = 0; v < 16; ++v) {
        ch.witness(v, {}, adv);
        distinct.push_back(circuit.prove(adv));
    }
    typlonk_ctx* c = ctx.raw();
    (void)circuit.verify_batch({distinct[0]});   // warm: the circuit's commitments are computed once and cached
    double t0 = now_ms();
    const bool mirror_ok = circuit.verify(distinct[0]);
    const double mirror_ms = now_ms() - t0;
    REQUIRE(mirror_ok);
    std::printf("MIRROR log_n=%u ms=%.2f\n", log_n, mirror_ms);
    for (int a = 3; a < argc; ++a) {
        const size_t count = (size_t)std::atol(argv[a]);
        std::vector<plonk::Proof> batch;
        for (size_t k = 0; k < count; ++k) batch.push_back(distinct[k % distinct.size()]);
        double best = 1e30;
        float split[5] = {0, 0, 0, 0, 0};
        for (int rep = 0; rep < 2; ++rep) {
            typlonk_set_profiling(c, 1);
            t0 = now_ms();
            const std::vector<bool> ok = circuit.verify_batch(batch);
            const double ms = now_ms() - t0;
            typlonk_set_profiling(c, 0);
            for (bool b : ok) REQUIRE(b);
            if (ms < best) {
                best = ms;
                const char* names[8];
                float v[8];
                const int ns = typlonk_profile_get(c, names, v, 8);
                for (int i = 0; i < ns && i < 5; ++i) split[i] = v[i];
            }
        }
        std::printf("BATCH log_n=%u count=%zu ms=%.2f per_proof_ms=%.3f host=%.2f eval=%.2f msm=%.2f pairing=%.2f folds=%.0f\n", log_n,
                    count, best, best / (double)count, split[0], split[1], split[2], split[3], split[4]);
    }
    return 0;
}
