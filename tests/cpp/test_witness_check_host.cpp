// CompiledCircuit::check_witness (typlonk_host.hpp -> typlonk_witness_check_host) on the README circuit a*a + b*b == c*c
// (/root/reference/README.md:16-27): the honest witness has no failure; a wrong input names the gate row and the copy
// constraints it breaks, and is the witness prove() refuses.  Needs a GPU.
#include <cstdio>
#include <cstdlib>

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
    const size_t n = circuit.rows;
    std::vector<Fr> advice[3];
    {   // honest: 9 + 16 == 25
        columns(3, 4, 5, advice);
        const auto rep = circuit.compiled().check_witness(advice);
        REQUIRE(rep.satisfied() && rep.gate_rows.empty() && rep.copy_cells.empty());
        const auto proof = circuit.compiled().prove(advice);
        REQUIRE(proof.r.eval().is_zero());
        std::printf("honest ok\n");
    }
    {   // 9 + 16 != 36: every gate holds (the columns are computed), the copy constraint d == c does not
        columns(3, 4, 6, advice);
        const auto rep = circuit.compiled().check_witness(advice);
        REQUIRE(!rep.satisfied() && rep.gate_failures == 0 && rep.copy_failures == 2 && rep.copy_cells.size() == 2);
        // the cycle (c_2 c_3): flat cells 2 n + 2 and 2 n + 3, each listed with its successor
        REQUIRE(rep.copy_cells[0][0] == 2 * n + 2 && rep.copy_cells[0][1] == 2 * n + 3);
        REQUIRE(rep.copy_cells[1][0] == 2 * n + 3 && rep.copy_cells[1][1] == 2 * n + 2);
        bool threw = false;
        try {
            circuit.compiled().prove(advice);
        } catch (const std::exception&) {
            threw = true;
        }
        REQUIRE(threw);
        std::printf("wrong input ok\n");
    }
    {   // one cell of a gate changed: the gate row and the cell's copy constraints, lowest first, cap = 1 truncates the lists only
        columns(3, 4, 5, advice);
        advice[2][0] = advice[2][0] + Fr::one();   // c_0 = x^2 + 1: gate 0 fails; c_0 ~ a_3 fails both ways round the cycle
        const auto rep = circuit.compiled().check_witness(advice);
        REQUIRE(rep.gate_failures == 1 && rep.gate_rows.size() == 1 && rep.gate_rows[0] == 0);
        REQUIRE(rep.copy_failures == 2 && rep.copy_cells[0][0] == 3 && rep.copy_cells[0][1] == 2 * n && rep.copy_cells[1][0] == 2 * n);
        const auto cut = circuit.compiled().check_witness(advice, {}, 1);
        REQUIRE(cut.copy_failures == 2 && cut.copy_cells.size() == 1 && cut.copy_cells[0][0] == 3);
        const auto none = circuit.compiled().check_witness(advice, {}, 0);
        REQUIRE(none.gate_failures == 1 && none.copy_failures == 2 && none.gate_rows.empty() && none.copy_cells.empty());
        std::printf("corrupted cell ok\n");
    }
    std::printf("all ok\n");
    return 0;
}
