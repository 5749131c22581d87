// prove_plan (csrc/prove_plan.hpp) as the host compiles it, without any HIP header: reads cases
//   log_n proofs mode cached
// (mode 0: a prover session, 1: a wave of a batch call; cached 0: the stand-alone quotient without a circuit id) from stdin or
// from the file named by the first argument and prints the plan of each, with the layouts and constants it was made from, as
// one line of JSON (tests/test_prove_plan_host.py).
#include <cstdio>

#include "../../typlonk_amd/csrc/prove_plan.hpp"

using namespace ty;

static void print_gp(const char* name, const GpScratch& g) {
    printf("\"%s\":{\"num\":%llu,\"den\":%llu,\"npre\":%llu,\"dsuf\":%llu,\"carries\":%llu,\"runs\":%llu,\"inv\":%llu,\"end\":%llu},", name,
           (unsigned long long)g.num, (unsigned long long)g.den, (unsigned long long)g.npre, (unsigned long long)g.dsuf,
           (unsigned long long)g.carries, (unsigned long long)g.runs, (unsigned long long)g.inv, (unsigned long long)g.end);
}
static void print_slots(const char* name, const Round3Slots& s) {
    printf("\"%s\":{\"wire\":%d,\"z\":%d,\"sig0\":%d,\"sig1\":%d,\"pi\":%d,\"zw\":%d,\"count\":%d,\"r\":%d,\"f\":%d},", name, s.wire, s.z, s.sig0,
           s.sig1, s.pi, s.zw, s.count, s.r, s.f);
}

int main(int argc, char** argv) {
    FILE* in = argc > 1 ? fopen(argv[1], "r") : stdin;
    if (!in) return 2;
    for (;;) {
        long long v[4];
        for (int i = 0; i < 4; ++i)
            if (fscanf(in, "%lld", &v[i]) != 1) return i == 0 ? 0 : 2;   // a case cut short is an error
        if (v[0] < 0 || v[0] > 24 || v[1] < 1 || v[2] < 0 || v[2] > 1) return 2;
        const ProvePlan p = prove_plan((uint32_t)v[0], (uint64_t)v[1], (ProveMode)v[2], v[3] != 0);
        const uint64_t n = p.n;
        printf("{\"log_n\":%u,\"n\":%llu,\"G\":%u,\"stride\":%u,\"prover_mem\":%zu,\"ops_tmp\":%zu,\"quot_ext\":%zu,\"quot_tab\":%zu,"
               "\"batch_tab\":%zu,\"slots\":%zu,\"need_gp\":%llu,\"need_open\":%llu,\"fr\":%zu,",
               p.log_n, (unsigned long long)n, p.G, p.stride, p.prover_mem, p.ops_tmp, p.quot_ext, p.quot_tab, p.batch_tab, p.slots,
               (unsigned long long)p.need_gp, (unsigned long long)p.need_open, sizeof(Fr));
        // the arena: each region's offset and length in Fr, and where the accessor puts vector 0 of each region of the LAST proof
        const char* names[8] = {"ev", "co", "pi", "z", "t", "q", "r", "ext"};
        const ProveArena a{nullptr, n, p.stride};
        printf("\"regions\":{");
        for (int i = 0; i < (p.stride == PROVE_STRIDE_WAVE ? 8 : 7); ++i)
            printf("%s\"%s\":[%llu,%llu,%llu]", i ? "," : "", names[i], (unsigned long long)(PROVE_REGIONS[i].off * n),
                   (unsigned long long)(PROVE_REGIONS[i].len * n), (unsigned long long)a.index(p.G - 1, PROVE_REGIONS[i]));
        printf("},\"stride_elems\":%llu,", (unsigned long long)a.stride_elems());
        printf("\"q\":{\"wit_a\":%u,\"wit_b\":%u,\"wit_c\":%u,\"wit_z\":%u,\"wit_zw\":%u,\"wit_r\":%u,\"batched_f\":%u,\"batched_wit\":%u,"
               "\"compact_f\":%u,\"compact_wit\":%u},",
               Q_WIT_A, Q_WIT_B, Q_WIT_C, Q_WIT_Z, Q_WIT_ZW, Q_WIT_R, Q_BATCHED_F, Q_BATCHED_WIT, Q_COMPACT_F, Q_COMPACT_WIT);
        print_gp("gp", gp_scratch(n));
        print_gp("gp_wave", gp_scratch_wave(n));
        const OpenDevScratch od = open_dev_scratch(n);
        printf("\"open_dev\":{\"carries\":%llu,\"y\":%llu,\"end\":%llu},", (unsigned long long)od.carries, (unsigned long long)od.y,
               (unsigned long long)od.end);
        // the opening launches of the mode, in carries: round 3's items, then r's (the compact shape: F's and r's)
        const uint64_t G = p.G;
        if (v[2] == PROVE_WAVE)
            printf("\"open_launches\":[%llu,%llu,%llu],", (unsigned long long)open_carries(G * PB_ITEMS, n),
                   (unsigned long long)open_carries(G, n), (unsigned long long)open_carries(2 * G, n));
        else
            printf("\"open_launches\":[%llu,%llu],", (unsigned long long)open_carries(PB_ITEMS, n), (unsigned long long)open_carries(1, n));
        print_slots("ref_slots", REF_SLOTS);
        print_slots("compact_slots", COMPACT_SLOTS);
        printf("\"slots_per_proof\":%d,\"items\":%u,\"tables\":%zu}\n", PROVE_SLOTS, PB_ITEMS, sizeof(PbTables));
    }
}
