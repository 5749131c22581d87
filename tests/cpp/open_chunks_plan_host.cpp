// open_chunks_plan (csrc/open_chunks_plan.hpp) as the host compiles it, without any HIP header: reads cases
//   count r l
// from stdin or from the file named by the first argument and prints the plan of each as one line of JSON, and beside it the
// result of walking the launch the kernel's way -- thread t takes slice t % g of output t / g, terms [s per, (s + 1) per) -- over
// every thread of every block: "covered" is 1 when each (output, term) was taken exactly once by a thread inside the launch and
// no thread below `threads` fell outside it (tests/test_open_chunks_plan_host.py).
#include <cstdio>
#include <vector>

#include "../../typlonk_amd/csrc/open_chunks_plan.hpp"

using namespace ty;

int main(int argc, char** argv) {
    FILE* in = argc > 1 ? fopen(argv[1], "r") : stdin;
    if (!in) return 2;
    long long v[3];
    for (;;) {
        for (int i = 0; i < 3; ++i)
            if (fscanf(in, "%lld", &v[i]) != 1) return i == 0 ? 0 : 2;   // a case cut short is an error
        const uint64_t count = (uint64_t)v[0], r = (uint64_t)v[1], l = (uint64_t)v[2];
        const OpenChunksPlan p = open_chunks_plan(count, r, l);
        int covered = -1;   // (not walked: too large)
        if (p.outputs * l <= (1ull << 24) && p.g) {
            std::vector<unsigned char> seen(p.outputs * l, 0);
            bool ok = p.blocks * 64 >= p.threads && (p.blocks - 1) * 64 < p.threads;
            for (uint64_t t = 0; t < p.blocks * 64 && ok; ++t) {
                const uint64_t o = t / p.g, s = t % p.g;
                if (o >= p.outputs) continue;   // a spare lane: shadows, stores nothing
                for (uint64_t j = s * p.per; j < (s + 1) * p.per && ok; ++j) {
                    ok = j < l && !seen[o * l + j];
                    if (ok) seen[o * l + j] = 1;
                }
            }
            for (uint64_t i = 0; i < seen.size() && ok; ++i) ok = seen[i] != 0;
            covered = ok ? 1 : 0;
        }
        printf("{\"count\":%llu,\"r\":%llu,\"l\":%llu,\"g\":%u,\"per\":%u,\"outputs\":%llu,\"threads\":%llu,\"blocks\":%llu,\"covered\":%d}\n",
               (unsigned long long)count, (unsigned long long)r, (unsigned long long)l, p.g, p.per, (unsigned long long)p.outputs,
               (unsigned long long)p.threads, (unsigned long long)p.blocks, covered);
    }
}
