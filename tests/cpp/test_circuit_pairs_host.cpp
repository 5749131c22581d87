// CompiledCircuit's constructor from selector evaluations and copy constraints given as cell pairs (typlonk_host.hpp ->
// typlonk_circuit_compile_pairs_host) on the README circuit a*a + b*b == c*c (/root/reference/README.md:16-27): the pairs are
// the front end's own permutation read as (x, perm[x]); the circuit proves and verifies, its kept permutation is the one
// CellPermutation::from_pairs returns, and both are printed for tests/test_gpu_perm_pairs.py to hold against its reference.
// Needs a GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "circuit_host.hpp"

using namespace typlonk;

#define REQUIRE(c)                                                          \
    do {                                                                    \
        if (!(c)) {                                                         \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);      \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

struct Circuit2 : plonk::CircuitDescription<3, Circuit2> {
    template <class V>
    static void run(std::array<V, 3> in) {
        V a = in[0].clone() * in[0];
        V b = in[1].clone() * in[1];
        V c = in[2].clone() * in[2];
        V d = a + b;
        d.assert_eq(c);
    }
};

// the columns ComputeVar records for inputs x, y, z (gates Mul, Mul, Mul, Add), padded to n - 3 = 5 rows, then three blinding rows
static void columns(uint64_t x, uint64_t y, uint64_t z, std::vector<Fr> (&advice)[3]) {
    const Fr X(x), Y(y), Z(z);
    advice[0] = {X, Y, Z, X * X, Fr(0)};
    advice[1] = {X, Y, Z, Y * Y, Fr(0)};
    advice[2] = {X * X, Y * Y, Z * Z, X * X + Y * Y, Fr(0)};
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) advice[i].push_back(Fr(100 + 10 * i + k));
}

static void print(const char* name, const std::vector<uint32_t>& v) {
    std::printf("%s:", name);
    for (uint32_t x : v) std::printf(" %u", x);
    std::printf("\n");
}

int main() {
    Context ctx(0);
    auto circuit = Circuit2::build(ctx);
    REQUIRE(circuit.rows == 8);
    const plonk::CircuitTables& t = circuit.tables();
    std::vector<plonk::CellPair> pairs;
    std::vector<uint32_t> flat;
    for (size_t x = 0; x < t.permutation.perm.size(); ++x)
        if (t.permutation.perm[x] != x) {
            pairs.push_back({(uint32_t)x, (uint32_t)t.permutation.perm[x]});
            flat.push_back((uint32_t)x);
            flat.push_back((uint32_t)t.permutation.perm[x]);
        }
    REQUIRE(!pairs.empty());
    Fr cosets[3];
    for (int i = 0; i < 3; ++i) cosets[i] = t.copy_constrains.cosets[i];
    const auto canonical = plonk::CellPermutation::from_pairs(ctx, t.log_rows, pairs);
    REQUIRE(canonical.perm.size() == 3 * circuit.rows);
    const plonk::CompiledCircuit from_pairs(circuit.srs(), t.log_rows, t.selector_evals, pairs, cosets);
    const plonk::CompiledCircuit from_perm(circuit.srs(), t.log_rows, t.selector_evals, canonical.perm, cosets);
    REQUIRE(from_pairs.classes() == canonical.classes);
    for (int k = 0; k < 5; ++k) REQUIRE(from_pairs.fixed_commitments[k] == from_perm.fixed_commitments[k]);
    for (int k = 0; k < 3; ++k) REQUIRE(from_pairs.sigma_commitments[k] == from_perm.sigma_commitments[k]);
    std::printf("commitments ok\n");
    std::vector<Fr> advice[3];
    columns(3, 4, 5, advice);
    const auto p1 = from_pairs.prove(advice), p2 = circuit.compiled().prove(advice);
    REQUIRE(p1.r.eval().is_zero());
    // the front end's permutation has the same classes in another order: each circuit accepts its own proofs only
    REQUIRE(from_pairs.verify(p1) && from_perm.verify(p1) && circuit.compiled().verify(p2));
    std::printf("proofs ok\n");
    REQUIRE(from_pairs.check_witness(advice).satisfied());
    columns(3, 4, 6, advice);   // 9 + 16 != 36: the copy constraint d == c fails
    REQUIRE(!from_pairs.check_witness(advice).satisfied());
    std::printf("check ok\n");
    {   // a pair outside the table: refused, the lowest bad pair named
        std::vector<plonk::CellPair> bad(pairs);
        bad.push_back({0, (uint32_t)(3 * circuit.rows)});
        bool threw = false;
        try {
            const plonk::CompiledCircuit refused(circuit.srs(), t.log_rows, t.selector_evals, bad, cosets);
        } catch (const std::exception& e) {
            threw = true;
            const std::string lowest = "pair " + std::to_string(bad.size() - 1);
            REQUIRE(std::strstr(e.what(), lowest.c_str()));
        }
        REQUIRE(threw);
        std::printf("refusal ok\n");
    }
    print("pairs", flat);
    print("perm", canonical.perm);
    std::printf("classes: %llu\n", (unsigned long long)canonical.classes);
    std::printf("all ok\n");
    return 0;
}
