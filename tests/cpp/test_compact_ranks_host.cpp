// The compact proof shape on a sharded SRS from plain C++ processes -- no Python, no PyTorch -- through the host mirror
// (typlonk_amd/host/typlonk_host.hpp).  `test_compact_ranks_host <world> <scratch dir>` starts <world> fresh copies of itself
// BEFORE it touches the GPU; every copy is one rank on GPU 0: own context, own SRS shard (kzg::Srs::from_secret_shard), own
// communicator (TYPLONK_RCCL_LIB = tests/cpp/libfake_rccl.so carries the all-gather: RCCL refuses several ranks per device).
// Each rank also holds the whole SRS under a second circuit object and checks that on the shard
//   * plonk::CompiledCircuit's commitments and verifying_key() are the whole-SRS ones (through typlonk_vk_to_bytes),
//   * prove_compact() returns the whole-SRS proof, byte for byte, with and without public values,
//   * plonk::verify_compact accepts it under the key the rank produced,
//   * an unsatisfied witness throws on every rank, and more public values than rows on rank 1 throw TYPLONK_ERR_LENGTH there
//     and TYPLONK_ERR_COMM naming rank 1 on its peers; the next proof succeeds each time.
#include <sys/wait.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../typlonk_amd/host/typlonk_host.hpp"

using namespace typlonk;

static int g_rank = -1;
#define REQUIRE(c)                                                                       \
    do {                                                                                 \
        if (!(c)) {                                                                      \
            std::printf("rank %d FAILED %s:%d: %s\n", g_rank, __FILE__, __LINE__, #c);   \
            std::exit(1);                                                                \
        }                                                                                \
    } while (0)

// test_compact_host's squaring chain (x_{j+1} = x_j^2 + pi_j)
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

static bool same_vk(const typlonk_vk& a, const typlonk_vk& b) {
    uint8_t x[TYPLONK_VK_WIRE_BYTES], y[TYPLONK_VK_WIRE_BYTES];
    return typlonk_vk_to_bytes(&a, x) == 0 && typlonk_vk_to_bytes(&b, y) == 0 && std::memcmp(x, y, sizeof(x)) == 0;
}

static int run_rank(int rank, int world, const std::string& dir) {
    g_rank = rank;
    const uint32_t log_n = 10;
    Context ctx(0);
    REQUIRE(typlonk_comm_available() == 1);
    // rendezvous id: rank 0 writes it, the others wait for the file
    std::array<uint8_t, TYPLONK_COMM_ID_BYTES> id{};
    const std::string path = dir + "/uid.bin", tmp = path + ".tmp";
    if (rank == 0) {
        id = Context::comm_unique_id();
        FILE* f = std::fopen(tmp.c_str(), "wb");
        REQUIRE(f && std::fwrite(id.data(), 1, id.size(), f) == id.size());
        std::fclose(f);
        REQUIRE(std::rename(tmp.c_str(), path.c_str()) == 0);
    } else {
        FILE* f = nullptr;
        for (int i = 0; i < 12000 && !(f = std::fopen(path.c_str(), "rb")); ++i) usleep(10000);
        REQUIRE(f && std::fread(id.data(), 1, id.size(), f) == id.size());
        std::fclose(f);
    }
    ctx.comm_init(id, rank, world);

    const Chain ch(ctx, log_n);
    const size_t total = ch.gates + 3;
    const size_t lo = (size_t)rank * total / world, hi = (size_t)(rank + 1) * total / world;
    const Fr secret(0x5EC2E7);
    kzg::Srs whole = kzg::Srs::from_secret(ctx, secret, ch.gates);
    kzg::Srs shard = kzg::Srs::from_secret_shard(ctx, secret, ch.gates, lo, hi - lo);
    REQUIRE(shard.sharded() && shard.len() == total && shard.g1_ref().size() == hi - lo);
    plonk::CompiledCircuit ref(whole, log_n, ch.sel, ch.sigma, ch.cosets);
    plonk::CompiledCircuit circuit(shard, log_n, ch.sel, ch.sigma, ch.cosets);   // a collective: the folded commitments
    for (int k = 0; k < 5; ++k) REQUIRE(!(circuit.fixed_commitments[k].p != ref.fixed_commitments[k].p));
    for (int k = 0; k < 3; ++k) REQUIRE(!(circuit.sigma_commitments[k].p != ref.sigma_commitments[k].p));
    const typlonk_vk want_vk = ref.verifying_key();
    const typlonk_vk vk = circuit.verifying_key();                               // a collective: 9 records
    REQUIRE(same_vk(vk, want_vk));

    std::vector<typlonk_proof_compact> proofs;
    std::vector<std::vector<Fr>> pis;
    for (int v = 0; v < 3; ++v) {
        std::vector<Fr> pi;
        if (v == 1) pi = {Fr(5), Fr::zero(), Fr(-3)};
        if (v == 2) pi.assign(ch.n, Fr::zero()), pi[0] = Fr(7), pi[ch.gates - 1] = Fr(11);   // pi_len = n
        const std::array<std::vector<Fr>, 3> adv = ch.witness(v, pi);
        const std::vector<Fr> cols[3] = {adv[0], adv[1], adv[2]};
        const typlonk_proof_compact want = ref.prove_compact(cols, pi);
        const typlonk_proof_compact got = circuit.prove_compact(cols, pi);      // a collective: 12, 1, 3 and 2 records
        REQUIRE(std::memcmp(&got, &want, sizeof(got)) == 0);
        proofs.push_back(got);
        pis.push_back(pi);
    }
    REQUIRE(plonk::verify_compact(ctx, vk, proofs, pis) == std::vector<bool>(3, true));
    // an unsatisfied witness throws on EVERY rank (all four folds complete); the next proof is the whole-SRS one again
    {
        std::array<std::vector<Fr>, 3> adv = ch.witness(7, {});
        adv[2][1] = adv[2][1] + Fr::one();
        const std::vector<Fr> cols[3] = {adv[0], adv[1], adv[2]};
        bool threw = false;
        try {
            (void)circuit.prove_compact(cols);
        } catch (const std::exception& e) {
            threw = std::strstr(e.what(), typlonk_strerror(TYPLONK_ERR_UNSATISFIED)) != nullptr;
        }
        REQUIRE(threw);
        const std::array<std::vector<Fr>, 3> good = ch.witness(0, {});
        const std::vector<Fr> gc[3] = {good[0], good[1], good[2]};
        const typlonk_proof_compact again = circuit.prove_compact(gc);
        REQUIRE(std::memcmp(&again, &proofs[0], sizeof(again)) == 0);
    }
    // more public values than rows on rank 1: ITS call throws TYPLONK_ERR_LENGTH, its peers' TYPLONK_ERR_COMM naming it
    {
        const std::array<std::vector<Fr>, 3> good = ch.witness(0, {});
        const std::vector<Fr> gc[3] = {good[0], good[1], good[2]};
        const std::vector<Fr> too_many(rank == 1 ? ch.n + 1 : 0, Fr::zero());
        std::string what;
        try {
            (void)circuit.prove_compact(gc, too_many);
        } catch (const std::exception& e) {
            what = e.what();
        }
        if (rank == 1) {
            REQUIRE(what.find(typlonk_strerror(TYPLONK_ERR_LENGTH)) != std::string::npos);
        } else {
            REQUIRE(what.find(typlonk_strerror(TYPLONK_ERR_COMM)) != std::string::npos && what.find("rank 1") != std::string::npos);
        }
        const typlonk_proof_compact again = circuit.prove_compact(gc);
        REQUIRE(std::memcmp(&again, &proofs[0], sizeof(again)) == 0);
    }
    ctx.comm_destroy();
    std::printf("rank %d of %d ok\n", rank, world);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 5 && std::strcmp(argv[1], "rank") == 0) {
        try {
            return run_rank(std::atoi(argv[2]), std::atoi(argv[3]), argv[4]);
        } catch (const std::exception& e) {
            std::printf("rank %d FAILED: %s\n", g_rank, e.what());
            return 1;
        }
    }
    if (argc != 3) {
        std::printf("usage: %s <world> <scratch dir>\n", argv[0]);
        return 2;
    }
    // the launcher: nothing here touches the GPU; the ranks are fresh processes (fork + exec of this binary)
    const int world = std::atoi(argv[1]);
    std::vector<pid_t> kids;
    for (int r = 0; r < world; ++r) {
        const pid_t pid = fork();
        if (pid == 0) {
            const std::string rs = std::to_string(r), ws = std::to_string(world);
            execl(argv[0], argv[0], "rank", rs.c_str(), ws.c_str(), argv[2], (char*)nullptr);
            _exit(127);
        }
        kids.push_back(pid);
    }
    int bad = 0;
    for (pid_t k : kids) {
        int st = 0;
        waitpid(k, &st, 0);
        if (!WIFEXITED(st) || WEXITSTATUS(st) != 0) ++bad;
    }
    std::printf(bad ? "%d rank(s) failed\n" : "all %d ranks ok\n", bad ? bad : world);
    return bad ? 1 : 0;
}
