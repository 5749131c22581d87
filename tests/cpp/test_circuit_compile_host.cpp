// CompiledCircuit's constructor from selector evaluations and a permutation (typlonk_host.hpp -> typlonk_circuit_compile_host)
// on the README circuit a*a + b*b == c*c (/root/reference/README.md:16-27), against the constructor that takes ready-made
// sigma evaluations: the same eight commitments, a proof of either verifies under the other, check_witness gives the same
// reports, and a permutation with two cells on one target is refused with the cell named.  Needs a GPU.
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

int main() {
    Context ctx(0);
    auto circuit = Circuit2::build(ctx);
    REQUIRE(circuit.rows == 8);
    const plonk::CircuitTables& t = circuit.tables();
    std::vector<uint32_t> perm(t.permutation.perm.begin(), t.permutation.perm.end());
    REQUIRE(perm.size() == 3 * circuit.rows);
    Fr cosets[3];
    for (int i = 0; i < 3; ++i) cosets[i] = t.copy_constrains.cosets[i];
    const plonk::CompiledCircuit& loaded = circuit.compiled();
    {
        const plonk::CompiledCircuit compiled(circuit.srs(), t.log_rows, t.selector_evals, perm, cosets);
        for (int k = 0; k < 5; ++k) REQUIRE(compiled.fixed_commitments[k] == loaded.fixed_commitments[k]);
        for (int k = 0; k < 3; ++k) REQUIRE(compiled.sigma_commitments[k] == loaded.sigma_commitments[k]);
        std::printf("commitments ok\n");
        std::vector<Fr> advice[3];
        columns(3, 4, 5, advice);
        const auto p1 = compiled.prove(advice), p2 = loaded.prove(advice);
        REQUIRE(p1.r.eval().is_zero() && p2.r.eval().is_zero());
        REQUIRE(loaded.verify(p1) && compiled.verify(p2) && compiled.verify(p1));
        std::printf("proofs ok\n");
        REQUIRE(compiled.check_witness(advice).satisfied());
        columns(3, 4, 6, advice);   // 9 + 16 != 36: the copy constraint d == c fails
        const auto a = compiled.check_witness(advice), b = loaded.check_witness(advice);
        REQUIRE(!a.satisfied() && a.gate_failures == b.gate_failures && a.copy_failures == b.copy_failures);
        REQUIRE(a.gate_rows == b.gate_rows && a.copy_cells == b.copy_cells && a.copy_cells.size() == 2);
        std::printf("check ok\n");
    }
    {   // no copy constraints at all: the identity
        const plonk::CompiledCircuit open(circuit.srs(), t.log_rows, t.selector_evals, std::vector<uint32_t>(), cosets);
        std::vector<uint32_t> id(perm.size());
        for (size_t x = 0; x < id.size(); ++x) id[x] = (uint32_t)x;
        const plonk::CompiledCircuit same(circuit.srs(), t.log_rows, t.selector_evals, id, cosets);
        for (int k = 0; k < 3; ++k) REQUIRE(open.sigma_commitments[k] == same.sigma_commitments[k]);
        REQUIRE(!(open.sigma_commitments[0] == loaded.sigma_commitments[0]));
        std::printf("identity ok\n");
    }
    {   // cell 1 sent where cell 0 goes already: that target is the image of two cells, cell 1's old target of none
        std::vector<uint32_t> bad(perm);
        const uint32_t orphan = bad[1];
        bad[1] = bad[0];
        bool threw = false;
        try {
            const plonk::CompiledCircuit refused(circuit.srs(), t.log_rows, t.selector_evals, bad, cosets);
        } catch (const std::exception& e) {
            threw = true;
            const std::string lowest = "cell " + std::to_string(std::min(orphan, bad[0]));
            REQUIRE(std::strstr(e.what(), "2 defects") && std::strstr(e.what(), lowest.c_str()));
        }
        REQUIRE(threw);
        std::printf("lint ok\n");
    }
    std::printf("all ok\n");
    return 0;
}
