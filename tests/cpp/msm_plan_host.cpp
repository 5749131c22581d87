// msm_plan (csrc/msm_plan.hpp) as the host compiles it, without any HIP header: reads cases
//   m mode len table_c table_T table_centred msm_chunks msm_lanes msm_scatter_staged msm_rc4 msm_chain
// (mode 0 stand-alone over device scalars, 1 stand-alone over host scalars, 2 queued) from stdin or from the file named by
// the first argument and prints the full plan of each as one line of JSON (tests/test_msm_plan_host.py).
#include <cstdio>

#include "../../typlonk_amd/csrc/msm_plan.hpp"

using namespace ty;

int main(int argc, char** argv) {
    FILE* in = argc > 1 ? fopen(argv[1], "r") : stdin;
    if (!in) return 2;
    long long v[11];
    for (;;) {
        for (int i = 0; i < 11; ++i)
            if (fscanf(in, "%lld", &v[i]) != 1) return i == 0 ? 0 : 2;   // a case cut short is an error
        MsmSrsFacts srs;
        srs.len = (size_t)v[2];
        srs.table_c = (uint32_t)v[3];
        srs.table_T = (uint32_t)v[4];
        srs.table_centred = v[5] != 0;
        MsmOverrides ov;
        ov.msm_chunks = (int)v[6];
        ov.msm_lanes = (int)v[7];
        ov.msm_scatter_staged = v[8] != 0;
        ov.msm_rc4 = v[9] != 0;
        ov.msm_chain = (int)v[10];
        const MsmPlan p = msm_plan(srs, (size_t)v[0], v[1] != 2, v[1] == 1, ov);
        printf("{\"status\":%d,\"tables\":%d,\"centred\":%d,\"c\":%u,\"W\":%u,\"nsets\":%u,\"digit_v\":%u,\"nb\":%llu,\"nch\":%u,"
               "\"overlap\":%d,\"chain\":%d,\"scatter_staged\":%d,\"chunks\":[",
               (int)p.status, (int)p.tables, (int)p.centred, p.c, p.W, p.nsets, p.digit_v, (unsigned long long)p.nb, p.nch, (int)p.overlap,
               (int)p.chain, (int)p.scatter_staged);
        for (size_t k = 0; k < p.chunk.size(); ++k) {
            const MsmChunkPlan& c = p.chunk[k];
            const MsmShape& s = c.sh;
            printf("%s{\"off\":%zu,\"mk\":%zu,\"beside\":%d,\"segsort\":%d,\"sh\":[%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u,%u],\"cap\":%u,"
                   "\"max_tasks\":%llu,\"lanes\":%u,\"split\":%u}",
                   k ? "," : "", c.off, c.mk, (int)c.beside, (int)c.segsort, s.c, s.W, s.top_v, s.hb, s.lb, s.nseg, s.nblk, s.chunk, s.ibits,
                   s.jbits, s.tlen, s.nsets, s.centred, s.prio, c.cap, (unsigned long long)c.max_tasks, c.lanes, c.split);
        }
        const RcShape& r = p.rcs;
        printf("],\"rcs\":[%u,%u,%u,%u,%u,%u,%u],\"rc2\":%d,\"sort\":[", r.nsets, r.c1, r.ch, r.cl, r.lhc, r.llc, r.top_v, (int)p.rc2);
        for (int set = 0; set < 2; ++set) {
            const MsmSortBytes& z = p.sort[set];
            printf("%s[%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu]", set ? "," : "", z.keys, z.sorted, z.counts, z.offsets,
                   z.cursor, z.blocksums, z.order, z.ohist, z.heavy, z.tasks, z.hpart, z.blk_hist, z.blk_base, z.blk_cnt, z.seg_start);
        }
        printf("],\"ws\":[%zu,%zu,%zu,%zu,%zu,%zu]}\n", p.buckets, p.part_a, p.part_b, p.rc_sums, p.rc_bits, p.rc_out);
    }
}
