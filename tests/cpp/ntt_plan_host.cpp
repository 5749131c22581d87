// ntt_plan (csrc/ntt_plan.hpp) as the host compiles it, without any HIP header: reads cases
//   log_n inverse shift count short_in ntt_fr30 ntt_big prover_rounds_active big_tiles_available
// (shift: the coset shift's 64 hex digits as they stand in a cache key, or - for no coset) from stdin or from the file named
// by the first argument and prints the full plan of each as one line of JSON (tests/test_ntt_plan_host.py).
#include <cstdio>
#include <cstring>

#include "../../typlonk_amd/csrc/ntt_plan.hpp"

using namespace ty;

int main(int argc, char** argv) {
    FILE* in = argc > 1 ? fopen(argv[1], "r") : stdin;
    if (!in) return 2;
    for (;;) {
        long long v[9] = {};
        char shift[80] = "";
        for (int i = 0; i < 9; ++i)
            if ((i == 2 ? fscanf(in, "%79s", shift) : fscanf(in, "%lld", &v[i])) != 1) return i == 0 ? 0 : 2;   // a case cut short is an error
        const bool coset = strcmp(shift, "-") != 0;
        NttFacts facts;
        facts.ntt_fr30 = (int)v[5];
        facts.ntt_big = (int)v[6];
        facts.prover_rounds_active = v[7] != 0;
        facts.big_tiles_available = v[8] != 0;
        const NttPlan p = ntt_plan((uint32_t)v[0], v[1] != 0, coset, (size_t)v[3], v[4] != 0, facts);
        printf("{\"status\":%d,\"group\":%zu,\"P\":%u,\"ks\":[%u,%u,%u,%u],\"big\":%d,\"want30\":%d,\"try30\":%d,\"f30_eligible\":%d,\"scratch_bytes\":%zu,"
               "\"passes\":[",
               (int)p.status, p.group, p.P, p.ks[0], p.ks[1], p.ks[2], p.ks[3], (int)p.big, (int)p.want30, (int)p.try30, (int)p.f30_eligible,
               p.scratch_bytes);
        for (uint32_t i = 0; i < p.P; ++i) {
            const NttPassPlan& ps = p.pass[i];
            const NttPassArgs& a = ps.a;
            printf("%s{\"k\":%u,\"last\":%u,\"logT\":%u,\"tw_h\":%u,\"pre_h\":%u,\"post_h\":%u,\"blocks_per_vec\":%u,\"threads\":%u,\"S\":%llu,"
                   "\"row_len\":%llu,\"N1\":%llu,\"Q\":%llu,\"N2\":%llu,\"N3\":%llu,\"out_stride\":%llu,\"short_in\":%d,\"lds\":[%zu,%zu]}",
                   i ? "," : "", a.k, a.last, a.logT, a.tw_h, a.pre_h, a.post_h, a.blocks_per_vec, ps.threads, (unsigned long long)a.S,
                   (unsigned long long)a.row_len, (unsigned long long)a.N1, (unsigned long long)a.Q, (unsigned long long)a.N2,
                   (unsigned long long)a.N3, (unsigned long long)a.out_stride, (int)ps.short_in, ps.lds[NTT_F32], ps.lds[NTT_F30]);
        }
        printf("],\"tables\":[");
        for (size_t i = 0; i < p.tables.size(); ++i) {
            const NttTableReq& r = p.tables[i];
            printf("%s{\"form\":%d,\"role\":%d,\"kind\":%d,\"pass\":%u,\"n\":%llu,\"base\":%d,\"base_log\":%u,\"base_sqr\":%u,\"scale\":%d,\"lo\":%u,"
                   "\"hi\":%u,\"h\":%u,\"S\":%llu,\"unless30\":%d,\"key\":\"%s\",\"group\":\"%s\"}",
                   i ? "," : "", (int)r.form, (int)r.role, (int)r.kind, r.pass, (unsigned long long)r.n, (int)r.base, r.base_log, r.base_sqr,
                   (int)r.scale, r.lo, r.hi, r.h, (unsigned long long)r.S, (int)r.unless30, ntt_key(r, shift).c_str(),
                   ntt_coset_group_of(ntt_key(r, shift)).c_str());
        }
        printf("]}\n");
    }
}
