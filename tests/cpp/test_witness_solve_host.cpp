// CompiledCircuit::solve_witness (typlonk_host.hpp -> typlonk_witness_solve) on the README circuit a*a + b*b == c*c: from the
// inputs [3, 4, 5] and the blinding rows the device fills the columns ComputeVar would push (builder.rs:381-396), the check finds
// no failure and prove() accepts them; the inputs [3, 4, 6] give two computed values tied by assert_eq that differ, and the
// check names that copy constraint.  Needs a GPU.
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

static bool same(const std::vector<Fr> (&a)[3], const std::vector<Fr> (&b)[3]) {
    for (int i = 0; i < 3; ++i) {
        if (a[i].size() != b[i].size()) return false;
        for (size_t j = 0; j < a[i].size(); ++j)
            if (!(a[i][j] == b[i][j])) return false;
    }
    return true;
}

int main() {
    Context ctx(0);
    auto circuit = Circuit2::build(ctx);
    REQUIRE(circuit.rows == 8);
    const uint32_t n = 8;
    // the inputs are the a cells of the three squarings; the blinding rows are free cells like any other
    std::vector<uint32_t> cells = {0, 1, 2};
    for (uint32_t i = 0; i < 3; ++i)
        for (uint32_t k = 0; k < 3; ++k) cells.push_back(i * n + 5 + k);
    auto values = [](uint64_t x, uint64_t y, uint64_t z) {
        std::vector<Fr> v = {Fr(x), Fr(y), Fr(z)};
        for (int i = 0; i < 3; ++i)
            for (int k = 0; k < 3; ++k) v.push_back(Fr(100 + 10 * i + k));
        return v;
    };
    const auto info = circuit.compiled().solve_info();
    REQUIRE(info.driven_rows == 4 && info.depth == 2 && info.launches == 2);   // three squarings, then their sum: one narrow run + the fill
    std::vector<Fr> want[3], got[3];
    {   // honest: 9 + 16 == 25
        columns(3, 4, 5, want);
        circuit.compiled().solve_witness(cells, values(3, 4, 5), got);
        REQUIRE(same(got, want));
        REQUIRE(circuit.compiled().check_witness(got).satisfied());
        const auto proof = circuit.compiled().prove(got);
        REQUIRE(proof.r.eval().is_zero());
        std::printf("honest ok\n");
    }
    {   // 9 + 16 != 36: both tied cells keep their own computed value, and the check names the copy constraint
        columns(3, 4, 6, want);
        circuit.compiled().solve_witness(cells, values(3, 4, 6), got);
        REQUIRE(same(got, want));
        const auto rep = circuit.compiled().check_witness(got);
        REQUIRE(rep.gate_failures == 0 && rep.copy_failures == 2);
        REQUIRE(rep.copy_cells[0][0] == 2 * n + 2 && rep.copy_cells[0][1] == 2 * n + 3);
        std::printf("wrong input ok\n");
    }
    {   // a computed cell cannot be assigned, and two cells of one class cannot both be
        bool threw = false;
        try {
            circuit.compiled().solve_witness({0, 1, 2, 3}, {Fr(3), Fr(4), Fr(5), Fr(9)}, got);   // a_3 is c_0's copy
        } catch (const std::exception&) {
            threw = true;
        }
        REQUIRE(threw);
        threw = false;
        try {
            circuit.compiled().solve_witness({0, n}, {Fr(3), Fr(3)}, got);                        // a_0 and b_0 are one variable
        } catch (const std::exception&) {
            threw = true;
        }
        REQUIRE(threw);
        std::printf("refusals ok\n");
    }
    std::printf("all ok\n");
    return 0;
}
