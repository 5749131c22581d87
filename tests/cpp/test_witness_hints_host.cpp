// CompiledCircuit::set_hints (typlonk_host.hpp -> typlonk_circuit_set_hints) on the README circuit a*a + b*b == c*c: the two free
// cells of the padding row take the inverse and the low three bits of the computed sum a*a + b*b, the check finds no failure and
// prove() accepts the columns; an empty set removes the hints; a refused set leaves the installed one in force.  Needs a GPU.
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

int main() {
    Context ctx(0);
    auto circuit = Circuit2::build(ctx);
    REQUIRE(circuit.rows == 8);
    const uint32_t n = 8;
    const std::vector<uint32_t> cells = {0, 1, 2};
    const std::vector<Fr> values = {Fr(3), Fr(4), Fr(5)};
    const Fr sum(25);
    // a_4 = 1 / c_3, b_4 = bits [0, 3) of c_3: row 4 is the padding row, its cells are free
    const std::vector<typlonk_hint> hints = {{TYPLONK_HINT_INV0, 4, 2 * n + 3, 0, 0}, {TYPLONK_HINT_BITS, n + 4, 2 * n + 3, 0, 3}};
    std::vector<Fr> plain[3], got[3];
    circuit.compiled().solve_witness(cells, values, plain);
    REQUIRE(plain[0][4] == Fr(0) && plain[1][4] == Fr(0) && plain[2][3] == sum);
    {
        circuit.compiled().set_hints(hints);
        const auto info = circuit.compiled().solve_info();
        REQUIRE(info.driven_rows == 4 && info.depth == 3);   // the squarings, their sum, the two hints
        circuit.compiled().solve_witness(cells, values, got);
        REQUIRE(got[0][4] == sum.inverse() && got[0][4] * sum == Fr(1) && got[1][4] == Fr(25 & 7));
        for (int i = 0; i < 3; ++i)
            for (uint32_t j = 0; j < n; ++j) REQUIRE((i < 2 && j == 4) || got[i][j] == plain[i][j]);
        REQUIRE(circuit.compiled().check_witness(got).satisfied());
        const auto proof = circuit.compiled().prove(got);
        REQUIRE(proof.r.eval().is_zero());
        std::printf("hinted ok\n");
    }
    {   // a hinted cell cannot be assigned; a hint into a driven class is refused, and the installed set stays
        bool threw = false;
        try {
            circuit.compiled().solve_witness({0, 1, 2, 4}, {Fr(3), Fr(4), Fr(5), Fr(9)}, got);
        } catch (const std::exception&) {
            threw = true;
        }
        REQUIRE(threw);
        threw = false;
        try {
            circuit.compiled().set_hints({{TYPLONK_HINT_INV0, 3, 0, 0, 0}});   // a_3 is c_0's copy
        } catch (const std::exception&) {
            threw = true;
        }
        REQUIRE(threw);
        circuit.compiled().solve_witness(cells, values, got);
        REQUIRE(got[0][4] == sum.inverse() && got[1][4] == Fr(1));
        std::printf("refusals ok\n");
    }
    {
        circuit.compiled().set_hints({});
        circuit.compiled().solve_witness(cells, values, got);
        for (int i = 0; i < 3; ++i)
            for (uint32_t j = 0; j < n; ++j) REQUIRE(got[i][j] == plain[i][j]);
        REQUIRE(circuit.compiled().solve_info().depth == 2);
        std::printf("removed ok\n");
    }
    std::printf("all ok\n");
    return 0;
}
