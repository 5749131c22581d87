// The CPU side of tools/witness_solve_time.py: the fill typlonk_witness_solve replaces, by the C++ front end's computing run
// (ComputeVar, tests/cpp/circuit_host.hpp: one field operation and three pushes per gate), single thread, host wall time.
//   witness_fill_cpu LOG_N [REPS]
// prints one line of JSON: the median of REPS (default 20) fills of n - 3 gates as the squaring chain (every gate waits for the
// one before it) and as a layered circuit of 32 levels (gate i of a level takes outputs i and i + 1 of the level before,
// multiplications and additions in turn).  Host arithmetic only; linked to the library for the header's sake.
//   g++ -O2 -std=c++17 tools/witness_fill_cpu.cpp -o tools/witness_fill_cpu -L typlonk_amd -ltyplonk_hip -Wl,-rpath,$PWD/typlonk_amd
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "../tests/cpp/circuit_host.hpp"

using namespace typlonk;
using plonk::Advice;
using plonk::ComputeVar;

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

static double chain(size_t gates, Fr* last) {
    const auto t0 = std::chrono::steady_clock::now();
    auto adv = std::make_shared<Advice>();
    ComputeVar x(Fr(3), adv);
    for (size_t j = 0; j < gates; ++j) x = x.clone() * x;
    *last = adv->col[2].back();
    return ms_since(t0);
}

static double layered(size_t gates, size_t levels, Fr* last) {
    const auto t0 = std::chrono::steady_clock::now();
    auto adv = std::make_shared<Advice>();
    const size_t width = gates / levels;
    std::vector<ComputeVar> prev(width, ComputeVar(Fr(3), adv)), next;
    for (size_t i = 0; i < width; ++i) prev[i] = ComputeVar(Fr(3 + i), adv);
    size_t done = 0;
    for (size_t k = 0; done < gates; ++k) {
        next.clear();
        for (size_t i = 0; i < width && done < gates; ++i, ++done)
            next.push_back((i + k) & 1 ? prev[i] + prev[(i + 1) % width] : prev[i] * prev[(i + 1) % width]);
        prev.swap(next);
        prev.resize(width, ComputeVar(Fr(1), adv));
    }
    *last = adv->col[2].back();
    return ms_since(t0);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const unsigned log_n = (unsigned)std::atoi(argv[1]);
    const int reps = argc > 2 ? std::atoi(argv[2]) : 20;
    if (log_n < 3 || log_n > 24 || reps < 1) return 2;
    const size_t gates = ((size_t)1 << log_n) - 3;
    std::vector<double> a, b;
    Fr sink_a, sink_b;
    for (int r = 0; r < reps; ++r) {
        a.push_back(chain(gates, &sink_a));
        b.push_back(layered(gates, 32, &sink_b));
    }
    std::sort(a.begin(), a.end());
    std::sort(b.begin(), b.end());
    std::printf("{\"log_n\":%u,\"reps\":%d,\"chain_fill_ms\":%.4f,\"layered_fill_ms\":%.4f,\"check\":%llu}\n", log_n, reps, a[a.size() / 2],
                b[b.size() / 2], (unsigned long long)(sink_a.limbs()[0] ^ sink_b.limbs()[0]));
    return 0;
}
