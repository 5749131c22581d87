// The wire format through the C++ mirror (plonk::proof_to_bytes / proofs_from_bytes / vk_to_bytes / vk_from_bytes /
// verify_compact_bytes) -- needs a GPU.  The circuit is test_verify_host's squaring chain (x_{j+1} = x_j^2 + pi_j).
//   test_wire_host [log_n]   a batch of proofs and its key round-trip through their bytes; the bytes verify in a context that
//                            holds only the decoded key; a proof with a flipped sign bit decodes and fails, one with an
//                            evaluation equal to r does not decode, and neither changes the verdict of the others
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
    std::vector<uint8_t> vk_bytes;
    typlonk_vk vk;
    {
        Context ctx(0);
        const Chain ch(ctx, log_n);
        kzg::Srs srs = kzg::Srs::from_secret(ctx, Fr(0x5EC2E7), ch.gates);
        plonk::CompiledCircuit circuit(srs, log_n, ch.sel, ch.sigma, ch.cosets);
        vk = circuit.verifying_key();
        vk_bytes = plonk::vk_to_bytes(vk);
        std::vector<std::array<std::vector<Fr>, 3>> adv;
        for (int v = 0; v < 5; ++v) {
            std::vector<Fr> pi;
            if (v == 1) pi = {Fr(5), Fr::zero(), Fr(-3)};
            if (v == 4) pi = {Fr(7)};
            adv.push_back(ch.witness(v, pi));
            pis.push_back(pi);
        }
        std::vector<int> status;
        got = circuit.prove_batch_compact(adv, pis, &status);
        for (int st : status) REQUIRE(st == TYPLONK_OK);
    }
    REQUIRE(vk_bytes.size() == TYPLONK_VK_WIRE_BYTES);
    const typlonk_vk vk2 = plonk::vk_from_bytes(vk_bytes);
    REQUIRE(plonk::vk_to_bytes(vk2) == vk_bytes);
    REQUIRE(vk2.log_n == vk.log_n && std::memcmp(vk2.commit_xy, vk.commit_xy, sizeof(vk.commit_xy)) == 0 &&
            std::memcmp(vk2.g2s_xy, vk.g2s_xy, sizeof(vk.g2s_xy)) == 0 && std::memcmp(vk2.srs0_xy, vk.srs0_xy, 96) == 0);
    std::vector<uint8_t> bytes;
    for (const auto& p : got) {
        const std::vector<uint8_t> b = plonk::proof_to_bytes(p);
        REQUIRE(b.size() == TYPLONK_PROOF_COMPACT_BYTES);
        bytes.insert(bytes.end(), b.begin(), b.end());
    }
    // a fresh context: no SRS, no circuit, only the key that came in as bytes
    Context fresh(0);
    std::vector<uint32_t> st_dev, st_host;
    const std::vector<typlonk_proof_compact> dev = plonk::proofs_from_bytes(&fresh, bytes, &st_dev);
    const std::vector<typlonk_proof_compact> host = plonk::proofs_from_bytes(nullptr, bytes, &st_host);
    REQUIRE(dev.size() == got.size() && st_dev == st_host);
    for (size_t k = 0; k < got.size(); ++k) {
        REQUIRE(st_dev[k] == 0);
        REQUIRE(std::memcmp(&dev[k], &host[k], sizeof(dev[k])) == 0);
        REQUIRE(plonk::proof_to_bytes(dev[k]) == plonk::proof_to_bytes(got[k]));
        REQUIRE(std::memcmp(dev[k].commit_xy, got[k].commit_xy, sizeof(got[k].commit_xy)) == 0 &&
                std::memcmp(dev[k].evals, got[k].evals, sizeof(got[k].evals)) == 0);
    }
    REQUIRE(plonk::verify_compact_bytes(fresh, vk2, bytes, pis) == std::vector<bool>(got.size(), true));
    std::vector<uint8_t> bad = bytes;
    bad[1 * TYPLONK_PROOF_COMPACT_BYTES + 7 * 48] ^= 0x20;                     // proof 1: the sign bit of W_z
    static const uint8_t R_LE[32] = {0x01, 0x00, 0x00, 0x00, 0xff, 0xff, 0xff, 0xff, 0xfe, 0x5b, 0xfe, 0xff, 0x02, 0xa4, 0xbd, 0x53,
                                     0x05, 0xd8, 0xa1, 0x09, 0x08, 0xd8, 0x39, 0x33, 0x48, 0x7d, 0x9d, 0x29, 0x53, 0xa7, 0xed, 0x73};
    std::memcpy(&bad[3 * TYPLONK_PROOF_COMPACT_BYTES + 9 * 48 + 2 * 32], R_LE, 32);   // proof 3: c(z) = r
    std::vector<bool> want(got.size(), true);
    want[1] = want[3] = false;
    REQUIRE(plonk::verify_compact_bytes(fresh, vk2, bad, pis) == want);
    std::vector<uint32_t> st;
    (void)plonk::proofs_from_bytes(&fresh, bad, &st);
    REQUIRE(st[1] == 0 && st[3] == TYPLONK_DECODE_STATUS(TYPLONK_SCALAR_RANGE, 11) && st[0] == 0 && st[2] == 0 && st[4] == 0);
    std::printf("wire format round trip ok\n");
    return 0;
}
