// solve_plan with hints (csrc/solve_plan.hpp) as the host compiles it, without any HIP header: reads circuits
//   n narrow run_cut n_hints   then 3n successors   then n driven flags   then n_hints times  kind dst src shift width
// from stdin or from the file named by the first argument and prints the full plan of each as one line of JSON
// (tests/test_solve_hints_host.py).
#include <cstdio>
#include <vector>

#include "../../typlonk_amd/csrc/solve_plan.hpp"

using namespace ty;

static void print_list(const char* name, const std::vector<uint32_t>& v) {
    printf(",\"%s\":[", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s%u", i ? "," : "", v[i]);
    printf("]");
}

int main(int argc, char** argv) {
    FILE* in = argc > 1 ? fopen(argv[1], "r") : stdin;
    if (!in) return 2;
    for (;;) {
        long long n, narrow, cut, nh;
        if (fscanf(in, "%lld", &n) != 1) return 0;
        if (fscanf(in, "%lld %lld %lld", &narrow, &cut, &nh) != 3 || n < 1 || narrow < 1 || cut < 1 || nh < 0) return 2;
        std::vector<uint32_t> perm(3 * (size_t)n);
        std::vector<uint8_t> driven((size_t)n);
        std::vector<SolveHint> hints((size_t)nh);
        for (auto& x : perm) {
            long long v;
            if (fscanf(in, "%lld", &v) != 1) return 2;   // a circuit cut short is an error
            x = (uint32_t)v;
        }
        for (auto& x : driven) {
            long long v;
            if (fscanf(in, "%lld", &v) != 1) return 2;
            x = v != 0;
        }
        for (auto& h : hints) {
            long long v[5];
            for (auto& x : v)
                if (fscanf(in, "%lld", &x) != 1) return 2;
            h = SolveHint{(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint16_t)v[3], (uint16_t)v[4]};
        }
        const SolvePlan p = solve_plan(perm.data(), driven.data(), (uint64_t)n, hints.data(), hints.size(), (uint32_t)narrow, (uint32_t)cut);
        printf("{\"status\":%d,\"bad\":%u,\"other\":%u", (int)p.status, p.bad, p.other);
        if (p.status == SOLVE_OK) {
            printf(",\"driven_rows\":%llu,\"free_classes\":%llu,\"depth\":%u,\"launches\":%u", (unsigned long long)p.driven_rows,
                   (unsigned long long)p.free_classes, p.depth, p.launches());
            print_list("src", p.src);
            print_list("level", p.level);
            print_list("hint_level", p.hint_level);
            print_list("order", p.order);
            print_list("level_off", p.level_off);
            printf(",\"schedule\":[");
            for (size_t i = 0; i < p.schedule.size(); ++i)
                printf("%s[%u,%u,%d]", i ? "," : "", p.schedule[i].first, p.schedule[i].levels, (int)p.schedule[i].wide);
            printf("]");
        }
        printf("}\n");
    }
}
