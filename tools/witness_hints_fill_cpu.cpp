// The CPU side of tools/witness_hints_time.py: the fill a solve under hints replaces, on one thread, host wall time.
//   witness_hints_fill_cpu LOG_N K [REPS]
// prints one line of JSON: the median of REPS (default 5) fills of the three columns of a circuit of (n - 3) / 2K range-check
// blocks (tests/witness_hints_ref.py, range_check): per block s = x + y, the K bits of s out of Montgomery form (what the BITS
// hints compute), and the K - 1 recomposition rows acc + 2^i b_i, one product and one sum each.  Host arithmetic only; linked to
// the library for the header's sake.
//   g++ -O2 -std=c++17 tools/witness_hints_fill_cpu.cpp -o tools/witness_hints_fill_cpu -L typlonk_amd -ltyplonk_hip -Wl,-rpath,$PWD/typlonk_amd
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../tests/cpp/circuit_host.hpp"

using namespace typlonk;

static double fill(size_t n, size_t k, std::vector<Fr> (&col)[3]) {
    const auto t0 = std::chrono::steady_clock::now();
    for (auto& c : col) c.assign(n, Fr());
    std::vector<Fr> pow2(k);
    pow2[0] = Fr::one();
    for (size_t i = 1; i < k; ++i) pow2[i] = pow2[i - 1] + pow2[i - 1];
    const Fr one = Fr::one(), zero = Fr::zero();
    for (size_t base = 0; base + 2 * k <= n - 3; base += 2 * k) {
        const Fr x((int64_t)(3 + base % 30000)), y((int64_t)(5 + (7 * base) % 30000));
        const Fr s = x + y;
        col[0][base] = x;
        col[1][base] = y;
        col[2][base] = s;
        ty::Fr m;
        std::memcpy(m.v, s.limbs(), 32);
        const ty::Fr plain = ty::fe_from_mont(m);
        const uint64_t word = (uint64_t)plain.v[0] | ((uint64_t)plain.v[1] << 32);
        Fr acc = zero;
        for (size_t i = 0; i < k; ++i) {
            const Fr bit = (word >> i) & 1 ? one : zero;
            col[0][base + 1 + i] = col[1][base + 1 + i] = bit;
            if (i == 0) {
                acc = bit;
                continue;
            }
            const size_t j = base + k + i;
            col[0][j] = acc;
            col[1][j] = bit;
            acc = acc + pow2[i] * bit;
            col[2][j] = acc;
        }
    }
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const unsigned log_n = (unsigned)std::atoi(argv[1]);
    const size_t k = (size_t)std::atoi(argv[2]);
    const int reps = argc > 3 ? std::atoi(argv[3]) : 5;
    if (log_n < 6 || log_n > 24 || k < 2 || k > 32 || reps < 1) return 2;
    std::vector<Fr> col[3];
    std::vector<double> t;
    for (int r = 0; r < reps; ++r) t.push_back(fill((size_t)1 << log_n, k, col));
    std::sort(t.begin(), t.end());
    uint64_t sink = 0;
    for (const Fr& v : col[2]) sink ^= v.limbs()[0];
    std::printf("{\"log_n\":%u,\"k\":%zu,\"reps\":%d,\"fill_ms\":%.4f,\"check\":%llu}\n", log_n, k, reps, t[t.size() / 2], (unsigned long long)sink);
    return 0;
}
