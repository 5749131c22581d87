// verify_chunks_plan (csrc/verify_chunks_plan.hpp) as the host compiles it, without any HIP header: reads cases
//   cells log_l strip        (strip = 0: the plan's own)
// from stdin or from the file named by the first argument and prints the plan of each as one line of JSON, and beside it the
// result of walking the launch the kernel's way -- workgroup b, iteration it, group g takes cell b strip + it groups + g when that
// lies below min((b + 1) strip, cells); thread q of a group takes the coefficients q + p group, p < per, that lie below l --:
// "covered" is 1 when every cell was taken exactly once and every coefficient of a cell by exactly one thread of its group
// (tests/test_verify_chunks_plan_host.py).  "sub_max_blocks" is the most workgroups any sub-range of 1 .. cells cells gets when
// it is planned with THIS plan's strip -- the way a bisection's folds are planned, into a buffer of `blocks` partial vectors --
// and "own_sub_max_blocks" the most a sub-range's own plan would ask for, which may be more: the count is not monotone in the
// cells (-1 each: not walked).
#include <cstdio>
#include <vector>

#include "../../typlonk_amd/csrc/verify_chunks_plan.hpp"

using namespace ty;

int main(int argc, char** argv) {
    FILE* in = argc > 1 ? fopen(argv[1], "r") : stdin;
    if (!in) return 2;
    long long v[3];
    for (;;) {
        for (int i = 0; i < 3; ++i)
            if (fscanf(in, "%lld", &v[i]) != 1) return i == 0 ? 0 : 2;   // a case cut short is an error
        const uint64_t cells = (uint64_t)v[0], strip = (uint64_t)v[2];
        const uint32_t log_l = (uint32_t)v[1], l = 1u << log_l;
        const VerifyChunksPlan p = verify_chunks_plan(cells, log_l, strip);
        int covered = -1;   // (not walked: too large)
        if (cells <= (1ull << 22) && p.blocks <= (1ull << 22)) {
            std::vector<unsigned char> seen(cells, 0);
            bool ok = true;
            for (uint64_t b = 0; b < p.blocks && ok; ++b) {
                const uint64_t first = b * p.strip, last = first + p.strip < cells ? first + p.strip : cells;
                ok = first < cells;   // no workgroup without a cell
                for (uint32_t it = 0; it < p.iters && ok; ++it)
                    for (uint32_t g = 0; g < p.groups && ok; ++g) {
                        const uint64_t c = first + (uint64_t)it * p.groups + g;
                        if (c >= last) continue;   // a group past the end of its strip: runs along on zeros
                        ok = !seen[c];
                        seen[c] = 1;
                    }
            }
            for (uint64_t c = 0; c < cells && ok; ++c) ok = seen[c] != 0;
            std::vector<unsigned char> coef(l, 0);
            for (uint32_t q = 0; q < p.group && ok; ++q)
                for (uint32_t k = 0; k < p.per && ok; ++k) {
                    const uint32_t j = q + k * p.group;
                    if (j >= l) continue;
                    ok = !coef[j];
                    coef[j] = 1;
                }
            for (uint32_t j = 0; j < l && ok; ++j) ok = coef[j] != 0;
            covered = ok ? 1 : 0;
        }
        long long sub_max = -1, own_sub_max = -1;
        if (cells <= (1ull << 22)) {
            for (uint64_t c = 1; c <= cells; ++c) {
                const long long with_strip = (long long)verify_chunks_plan(c, log_l, p.strip).blocks;
                const long long own = (long long)verify_chunks_plan(c, log_l).blocks;
                if (with_strip > sub_max) sub_max = with_strip;
                if (own > own_sub_max) own_sub_max = own;
            }
        }
        printf("{\"cells\":%llu,\"log_l\":%u,\"named\":%llu,\"group\":%u,\"groups\":%u,\"per\":%u,\"iters\":%u,\"strip\":%llu,\"blocks\":%llu,"
               "\"tw\":%u,\"lds_cells\":%u,\"lds_bytes\":%u,\"covered\":%d,\"sub_max_blocks\":%lld,\"own_sub_max_blocks\":%lld}\n",
               (unsigned long long)cells, log_l, (unsigned long long)strip, p.group, p.groups, p.per, p.iters, (unsigned long long)p.strip,
               (unsigned long long)p.blocks, p.tw, p.lds_cells, p.lds_bytes, covered, sub_max, own_sub_max);
    }
}
