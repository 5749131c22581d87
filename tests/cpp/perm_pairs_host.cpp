// Test-only host build of the union-find of typlonk_permutation_from_pairs (typlonk_amd/csrc/perm_pairs.hpp): the find, hook and
// pointer-jumping bodies of pp_hook_kernel and pp_jump_kernel as the host compiles them, their atomics relaxed __atomic
// builtins, run by real threads (tests/test_perm_pairs_host.py).  Not linked into libtyplonk_hip.so.
//
//   perm_pairs_host <log_n> < pairs      pairs: whitespace-separated cells, two per pair
//
// prints the 3 * 2^log_n labels after the hooks ran on 1 thread, then (second line) after they ran on 16 threads, thread t
// taking the pairs t, t + 16, ... so that neighbours in the list meet in time.  The jumps run on the same thread count.
// Exit status 2: a cell outside the table; 3: a walk reached its bound.
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../../typlonk_amd/csrc/perm_pairs.hpp"

using namespace ty;

static bool run(uint32_t log_n, const std::vector<uint32_t>& pairs, unsigned threads, std::vector<uint32_t>* label) {
    const uint32_t n3 = 3u << log_n;
    const size_t count = pairs.size() / 2;
    std::vector<uint32_t>& parent = *label;
    parent.resize(n3);
    for (uint32_t x = 0; x < n3; ++x) parent[x] = x;
    std::vector<char> ok(threads, 1);
    auto each = [&](auto body) {
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < threads; ++t) pool.emplace_back(body, t);
        body(0u);
        for (auto& th : pool) th.join();
    };
    each([&](unsigned t) {
        for (size_t i = t; i < count; i += threads)
            if (!pp_union(parent.data(), pairs[2 * i], pairs[2 * i + 1], 2 * n3)) ok[t] = 0;
    });
    for (uint32_t r = 0; r < pp_jump_rounds(log_n); ++r)
        each([&](unsigned t) {
            for (uint32_t x = t; x < n3; x += threads) pp_jump(parent.data(), x, PP_JUMP_HOPS);
        });
    for (char k : ok)
        if (!k) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) return 1;
    const uint32_t log_n = (uint32_t)std::atoi(argv[1]);
    if (log_n < 1 || log_n > 24) return 1;
    const uint32_t n3 = 3u << log_n;
    std::vector<uint32_t> pairs;
    unsigned long long v;
    while (std::scanf("%llu", &v) == 1) {
        if (v >= n3) return 2;
        pairs.push_back((uint32_t)v);
    }
    if (pairs.size() % 2) return 1;
    for (unsigned threads : {1u, 16u}) {
        std::vector<uint32_t> label;
        if (!run(log_n, pairs, threads, &label)) return 3;
        for (uint32_t x = 0; x < n3; ++x) std::printf(x + 1 < n3 ? "%u " : "%u\n", label[x]);
    }
    return 0;
}
