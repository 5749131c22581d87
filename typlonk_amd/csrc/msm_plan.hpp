// Every decision of an MSM that does not need the device: windows, table or plain mode, the chunk cuts, the shape of each
// chunk's bucket sort, the heavy-bucket threshold, lanes per bucket, the reduction's shape and form -- and the byte size of
// every workspace buffer the call needs.  msm_plan() states them once; msm_enqueue (msm_host.hip) sizes the workspace from
// the plan and queues what it says, and the sort kernels (msm_sort.hip) index by the very MsmShape the buffers were sized
// from.  MSM policy is edited HERE.  No HIP include: the host compiles this header on its own
// (tests/cpp/msm_plan_host.cpp prints the plan, tests/test_msm_plan_host.py holds it against tests/golden/msm_plans.json),
// like sigma_cell.hpp and perm_pairs.hpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "ff.hpp"   // TY_HD

namespace ty {

constexpr int SCAN_PER_BLOCK = 2048;  // 256 threads x 8
// a heavy bucket of `count` entries (more than `cap`, msm_sort.hip) is cut into tasks of this many entries, one wavefront
// each: 4 entries per lane before the six butterfly steps, 16 for the very large buckets (where the tasks are many and
// the butterfly is the cost: 2^20 equal scalars 20 -> 5.4 ms; with a few thousand heavy entries the short tasks win)
TY_HD uint32_t msm_task_len(uint32_t count) { return count >= 65536u ? 1024u : 256u; }
constexpr uint32_t MSM_TASK_LEN_MIN = 256;
// smallest heavy-bucket threshold (entries one accumulation thread may sum; msm_plan)
constexpr uint32_t MSM_CAP_MIN = 32;
constexpr int MSM_MAX_CHUNKS = 8;
constexpr size_t MSM_CHAIN_MIN_TERMS = (size_t)1 << 17;   // typlonk_ctx::msm_chain

// windows of the signed c-bit digit decomposition.  Scalars are canonical (< r < 2^255): the top window holds
// t = bits - c (W0 - 1) bits, W0 = ceil(bits / c), and a digit <= 2^t cannot exceed 2^(c-1) (no carry out of it) unless
// t = c.  Centred scalars (|k| <= (r - 1)/2 < 2^254) have one bit less: c = 17 -> 15 windows instead of 16.
TY_HD uint32_t msm_windows(uint32_t c, bool centred) {
    const uint32_t bits = centred ? 254u : 255u;
    const uint32_t w0 = (bits + c - 1) / c;
    return w0 + ((bits - c * (w0 - 1)) == c ? 1u : 0u);
}
// window of a plain m-term MSM
inline void msm_shape(size_t m, uint32_t* c_out, uint32_t* w_out) {
    uint32_t lg = 0;  // ceil(log2 m)
    while (((size_t)1 << lg) < m) ++lg;
    // measured on MI355X in round 1 (a sweep over forced windows): the best window is c ~ ceil(log2 m) clamped to [8, 16];
    // the bucket reduction is a fixed ~50-operation dependent chain whatever c is, so small MSMs want
    // many small buckets (short accumulate chains) rather than few windows
    int c = (int)lg;
    if (c < 8) c = 8;
    if (c > 16) c = 16;
    *c_out = (uint32_t)c;
    *w_out = msm_windows((uint32_t)c, false);
}

// Row/column bucket reduction (msm_reduce.hip).  A bucket set of B = 2^c1 buckets is read as a grid of
// R = 2^ch rows x C = 2^cl columns, k = hi * C + lo.  Every bucket weight splits as w(k) = wr(hi) + wc(lo):
//   v <= cl : wr = hi << (cl - v),            wc = (lo >> v) + 1
//   v >  cl : wr = (hi >> (v - cl)) + 1,      wc = 0
// (v = virtual-copy bits of the set: top_v for the last set of a plain MSM, else 0), so
// sum_k w(k) B_k = sum_hi wr(hi) Rsum_hi + sum_lo wc(lo) Csum_lo needs only PLAIN sums of buckets plus two
// weighted sums of R + C points.  Those are returned as bit planes -- out[(set*2 + kind)*RC_NB + b] =
// sum of the row (kind 0) / column (kind 1) sums whose weight has bit b set, rows WITHOUT their common
// factor 2^shift -- and the host finishes with one Horner pass over powers of two.
constexpr uint32_t RC_NB = 16;
struct RcShape {
    uint32_t nsets, c1, ch, cl;
    uint32_t lhc, llc;  // log2 rows per column partial / columns per row partial
    uint32_t top_v;
};
TY_HD uint32_t rc_set_v(const RcShape& sh, uint32_t set) { return set + 1 == sh.nsets ? sh.top_v : 0u; }
// bits of the row / column weights of a set and the rows' common shift
TY_HD void rc_bits(const RcShape& sh, uint32_t set, uint32_t* nbr, uint32_t* nbc, uint32_t* shift) {
    const uint32_t v = rc_set_v(sh, set);
    if (v <= sh.cl) {
        *nbr = sh.ch;
        *nbc = sh.cl - v + 1;
        *shift = sh.cl - v;
    } else {
        const uint32_t d = v - sh.cl;
        *nbr = (d <= sh.ch ? sh.ch - d : 0u) + 1;
        *nbc = 0;
        *shift = 0;
    }
}
TY_HD uint32_t rc_weight(const RcShape& sh, uint32_t set, uint32_t kind, uint32_t idx) {
    const uint32_t v = rc_set_v(sh, set);
    if (v <= sh.cl) return kind == 0 ? idx : (idx >> v) + 1;
    return kind == 0 ? (idx >> (v - sh.cl)) + 1 : 0u;
}
// the same bit planes in two launches (msm_reduce.hip, launch_msm_rc2_reduce) need cl, ch >= 6
inline bool msm_rc2_ok(const RcShape& sh) { return sh.cl >= 6 && sh.ch >= 6; }

// ---- segmented counting sort: its shape, for the host that sizes its buffers and the kernels that index them ----
// scalars per workgroup: 2048 (8 per thread) up to 2^20 terms, growing with m beyond that so the
// workgroup x segment matrix (nblk * nseg counters) stays bounded instead of growing like m^2
// threads per workgroup of the level-1 passes (512 and 1024 were measured: no gain)
inline uint32_t msm_seg1_threads() { return 256; }
// scalars per thread of the level-1 passes: 8 from 2^20 terms on; a short MSM (an index shard) gets fewer, so that its
// level-1 launches still have 512 workgroups -- at 2^17 terms 8 per thread is 64 workgroups and 34 + 39 us for the
// histogram and the scatter, 1 per thread 512 workgroups (profiles/r03_shard_timeline.txt)
inline uint32_t msm_seg1_per_thread(uint64_t m) {
    // (2^19-term chunks keep 8: their scatter, 4096 segments wide, wants long runs per workgroup and segment)
    return m <= (1u << 17) ? 1u : (m <= (1u << 18) ? 2u : 8u);
}
inline uint32_t msm_chunk_for(uint64_t m) {
    uint32_t chunk = msm_seg1_per_thread(m) * msm_seg1_threads();
    while (((uint64_t)chunk << 9) < m) chunk <<= 1;  // at most 512 workgroups
    return chunk;
}

// nblk = workgroups of the level-1 passes, `chunk` scalars each
struct MsmShape {
    uint32_t c, W, top_v, hb, lb, nseg, nblk, chunk;
    // level-1 entry layout: [i : ibits][j : jbits][sign : 1][low bucket bits : lb]
    uint32_t ibits, jbits;
    // fixed-base table mode (tlen != 0): base (j, i) lives at gather index j * tlen + i and all windows
    // share one bucket set (nsets = 1; 0 in plain mode, where every window has its own)
    uint32_t tlen, nsets;
    // centred scalars: k > (r - 1)/2 is replaced by r - k with every digit's sign flipped, so |k| < 2^254 and
    // c = 17 needs 15 windows instead of 16, c = 15 17 instead of 18 (msm_windows)
    uint32_t centred;
    // > 0: the kernels of this sort raise their wavefronts' issue priority (s_setprio).  Set for a sort that runs BESIDE an
    // accumulation (an overlapped chunk, a queued MSM): its few, short wavefronts then get the issue slots they ask for
    // instead of the ones two accumulation wavefronts per SIMD leave over.
    uint32_t prio;
};
// Shape of the two-level (segmented) counting sort for an m-term MSM (or chunk) with c-bit windows: hb high bucket bits pick
// the segment, the low lb <= 8 bits are sorted in LDS; a level-1 entry packs [i : ibits][j : 4 in table mode][sign][low : lb]
// into 32 bits.  Fills what follows from (m, c, W, nsets, tables) -- the caller adds top_v, tlen, centred and prio -- and
// returns whether the segmented sort can handle it (otherwise: plain MSMs use the atomic sort, table mode is not available).
inline bool msm_seg_shape(uint64_t m, uint32_t c, uint32_t W, uint32_t nsets, bool tables, MsmShape* sh) {
    *sh = MsmShape{};
    uint32_t lgm = 0;
    while (((uint64_t)1 << lgm) < m) ++lgm;
    sh->c = c;
    sh->W = W;
    sh->nsets = tables ? nsets : 0u;
    sh->ibits = tables ? std::max<uint32_t>(lgm, 1) : 23;
    sh->jbits = tables ? (W > 16 ? 5 : 4) : 0;   // table mode: the window index travels in the level-1 entry
    const int lb_max = tables ? std::min<int>(8, 32 - (int)sh->ibits - (int)sh->jbits - 1) : 8;
    const int hb = std::max<int>((int)c - 1 - lb_max, tables ? 0 : (int)lgm - 13);
    sh->hb = (uint32_t)std::max(0, std::min<int>(hb, (int)c - 1));
    sh->lb = c - 1 - sh->hb;
    const uint64_t nseg = (uint64_t)nsets << sh->hb;   // segments keyed by (bucket set, b >> lb)
    sh->nseg = (uint32_t)nseg;
    sh->chunk = msm_chunk_for(m);
    sh->nblk = (uint32_t)((m + sh->chunk - 1) / sh->chunk);
    const uint64_t nmat = nseg * sh->nblk;             // the workgroup x segment matrix
    return m <= (1u << 23) && lb_max >= 1 && nseg * 4 <= 64 * 1024 && nmat < (1ull << 31) && (!tables || W <= 32) &&
           (uint64_t)W * m < (1ull << 31);
}

// Schedule counters of the segmented sort.  Words [0, 516) keep the layout of the atomic sort's hist514 ([512] heavy buckets,
// [513] tasks -- msm_heavy_kernel reads those); the size histogram and the claim cursors of the SEGMENTED sort are kept in
// MSM_SCHED_REPLICAS copies behind them, replica r = segment mod R at word 1024 + 512 r (256 bins + 256 cursors, a KiB apart).
// Why: ~25 size bins are hot, adjacent words of ONE cache line, and every one of the 2048-4096 level-2 workgroups adds
// to each of them -- 51 K atomics on one line, which the L2 retires one per clock: ~24 us per launch, the whole run time of
// order_fused_kernel in rounds 1-5 and most of msm_seg_count / msm_seg_place.  Sixteen lines take them sixteen at a time.
constexpr uint32_t MSM_SCHED_REPLICAS = 16;
constexpr uint32_t MSM_SCHED_WORDS = 1024 + 512 * MSM_SCHED_REPLICAS;

// ---- chunks ----
// Chunks of an m-term MSM (msm_chunks): chunk k = terms [cut(k), cut(k + 1)), equal shares, or (first != 0) a first chunk
// of that many terms and equal shares of the rest
struct MsmChunks {
    uint32_t nch = 1;
    size_t first = 0;
    size_t cut(size_t m, uint32_t k) const {
        if (k == 0) return 0;
        const size_t step = first ? (m - first + nch - 2) / (nch - 1) : (m + nch - 1) / nch;
        return std::min(m, first ? first + (size_t)(k - 1) * step : (size_t)k * step);
    }
    size_t largest(size_t m) const {
        size_t big = 0;
        for (uint32_t k = 0; k < nch; ++k) big = std::max(big, cut(m, k + 1) - cut(m, k));
        return big;
    }
};
// a queued table-mode MSM of more than 2^20 terms runs in chunks of <= 2^20 terms (see msm_chunks)
inline uint32_t queued_table_chunks(size_t m) { return m > ((size_t)1 << 20) ? (uint32_t)((m + ((size_t)1 << 20) - 1) >> 20) : 1u; }
// Can MSMs over a len-point SRS run in table mode with c-bit windows and T tables?  Every gather index j * len + i
// (j < T, i < len) must leave bit 31 free for the sign (msm_sort.hip), and the shortest table-mode MSM -- len / 4 terms,
// in the chunks a queued MSM of that length takes -- must have a sort shape.
inline bool msm_table_srs_ok(size_t len, uint32_t c, uint32_t T) {
    if ((uint64_t)T * len > (1ull << 31)) return false;
    const size_t m = std::max<size_t>(len / 4, 1);
    MsmChunks ch;
    ch.nch = queued_table_chunks(m);
    MsmShape sh;
    return msm_seg_shape(ch.largest(m), c, T, 1, true, &sh);
}

// what a plan depends on besides the length: the SRS, and the context's overrides (host.hpp, typlonk_ctx)
struct MsmSrsFacts {
    size_t len = 0;
    uint32_t table_c = 0, table_T = 0;
    bool table_centred = false;
};
struct MsmOverrides {
    int msm_chunks = 0, msm_lanes = 0;
    bool msm_scatter_staged = true, msm_rc4 = false;
    int msm_chain = -1;
};

// stand-alone MSM over host scalars with the default chunking: a short first chunk (see msm_chunks)
inline bool overlap_host_first(const MsmOverrides& ov, bool standalone, bool host_scalars, uint32_t nch, size_t m) {
    // (two default chunks only, i.e. 2^20 <= m < 3 * 2^19: at 2^22, eight chunks, the short first chunk costs 0.07 ms instead)
    return standalone && host_scalars && nch == 2 && !ov.msm_chunks && m >= ((size_t)1 << 20);
}

inline MsmChunks msm_chunks(const MsmOverrides& ov, size_t m, bool tables, bool standalone, bool host_scalars) {
    // Chunks of terms.  A stand-alone MSM (nothing else in flight to hide behind) is cut into chunks that all add into
    // the SAME buckets: while chunk k is accumulated on the MSM's stream, chunk k + 1 is sorted on the workspace's side
    // stream, so only the first chunk's sort (and the last one's reduction) stay exposed.  Later chunks start from the
    // stored buckets (192 B read + written per bucket and chunk -- noise next to the additions).  Bit-identical
    // results: group addition is commutative and the output is the canonical affine point.
    MsmChunks ch;
    if (standalone) {
        // measured (tools/msm_chunks.py, profiles/r02_msm_chunks.jsonl): the overlapped sort is not free -- it competes
        // with the accumulation for issue slots -- and chunks of ~2^19 terms are the best grain: 2 chunks at 2^20
        // (2.76 -> 2.68 ms), 4 at 2^21 (5.09 -> 4.81), 8 at 2^22 (9.92 -> 8.99); below 2^20 one chunk wins
        // (scalars still on the host: two chunks from 2^19 terms on, so that half of the copy hides -- 1.68 -> 1.57 ms at 2^19;
        // neutral at 2^18, a loss at 2^17: profiles/r06_ab_host_scalar_path.txt, call W)
        ch.nch = ov.msm_chunks ? (uint32_t)ov.msm_chunks
                               : (m >= (1u << 20) ? (uint32_t)std::min<size_t>(m >> 19, MSM_MAX_CHUNKS)
                                                  : (host_scalars && m >= (1u << 19) ? 2u : 1u));
        while (ch.nch > 1 && m / ch.nch < 4096) --ch.nch;
    } else if (tables) {
        // A queued MSM (a batch, a prover round) of more than 2^20 terms: chunks of <= 2^20 terms one after the other on the
        // MSM's own stream, all adding into the same buckets.  Not for overlap (the other lanes provide that) but for the
        // sort's shape: above 2^20 terms a level-1 entry has too few bits left for the low bucket bits, the segment count
        // passes 8192 and the sort falls back to the three-launch scan and the direct scatter (rounds 1-5: every
        // commitment of a 2^22-row proof).  Not capped at MSM_MAX_CHUNKS (which sizes the overlap events of a stand-alone
        // MSM): these chunks run in stream order, so a 2^24-term commitment is 16 chunks of the same shape as at 2^20.
        ch.nch = queued_table_chunks(m);
    }
    // chunk k = terms [cut(k), cut(k + 1)): equal shares, or a first chunk of its own size and equal shares of the rest:
    //  * scalars in HOST memory (typlonk_msm_g1): the first chunk's copy over PCIe is the exposed one, so it is 2^18 terms (8 MB)
    //    instead of 2^19 and there is one chunk more -- 2.73-2.75 -> 2.59-2.65 ms per 2^20-term commitment
    //    (profiles/r06_ab_host_scalar_path.txt, calls U and V); device-resident scalars keep equal chunks (an unequal first
    //    chunk loses there: profiles/r06_ab_first_chunk_and_rc2.txt).
    if (overlap_host_first(ov, standalone, host_scalars, ch.nch, m)) {
        ch.first = (size_t)1 << 18;
        ch.nch = std::min<uint32_t>(ch.nch + 1, MSM_MAX_CHUNKS);
    }
    return ch;
}

// ---- the plan ----
// byte sizes of one set of sort outputs (host.hpp, SortBufs: the same names)
struct MsmSortBytes {
    size_t keys = 0, sorted = 0, counts = 0, offsets = 0, cursor = 0, blocksums = 0, order = 0, ohist = 0, blk_hist = 0, blk_base = 0,
           blk_cnt = 0, seg_start = 0, heavy = 0, tasks = 0, hpart = 0;
};
struct MsmChunkPlan {
    size_t off = 0, mk = 0;    // terms [off, off + mk)
    bool beside = false;       // sorted on the side stream, beside the previous chunk's accumulation
    // the segmented sort with this shape, or (shapes it cannot take -- more than 2^23 terms) the atomic counting sort
    bool segsort = false;
    MsmShape sh{};
    uint32_t cap = 0;          // entries one accumulation thread may sum; a bucket above it is heavy
    uint64_t max_tasks = 0;    // bound on the heavy-bucket tasks
    uint32_t lanes = 1, split = 0;
};
enum MsmPlanStatus { MSM_PLAN_OK = 0, MSM_PLAN_TOO_LARGE, MSM_PLAN_NO_TABLE_SORT };
struct MsmPlan {
    MsmPlanStatus status = MSM_PLAN_OK;
    bool tables = false, centred = false;
    uint32_t c = 0, W = 0;
    uint32_t nsets = 0, digit_v = 0;   // bucket sets; virtual-copy bits of the top window's digits
    uint64_t nb = 0;                   // buckets
    uint32_t nch = 1;                  // chunk cuts (every one of them non-empty: chunk.size() == nch)
    bool overlap = false;              // chunk k + 1 sorted on the side stream while chunk k accumulates
    bool chain = false;                // the accumulations of queued MSMs run one after the other (typlonk_ctx::accum_chain)
    std::vector<MsmChunkPlan> chunk;
    RcShape rcs{};
    bool rc2 = false;                  // the two-launch form of the row/column reduction (else four launches)
    bool scatter_staged = true;        // level 1 of the segmented sort stages its runs in the LDS where that fits (else: direct)
    // workspace bytes, each the maximum over the chunks that use the buffer: chunk k sorts into set k & 1 (host.hpp, MsmWs::sb)
    MsmSortBytes sort[2];
    size_t buckets = 0, part_a = 0, part_b = 0, rc_sums = 0, rc_bits = 0, rc_out = 0;
};

inline MsmPlan msm_plan(const MsmSrsFacts& srs, size_t m, bool standalone, bool host_scalars, const MsmOverrides& ov) {
    MsmPlan p;
    msm_shape(m, &p.c, &p.W);
    // fixed-base tables: every window reads its own pre-shifted copy of the base, so all windows share
    // one bucket set (plus a separate set for a thin top window) and no cross-window doublings remain.  The sort sees one
    // chunk at a time, with chunk-local term indices, so the shape of the LARGEST chunk decides (typlonk_srs_precompute
    // refuses SRS shapes the table-mode sort cannot handle; the check here keeps a plain MSM possible should one slip through)
    MsmChunks chunks;
    MsmShape probe;
    if (srs.table_T != 0 && m >= srs.len / 4 && (uint64_t)srs.table_T * srs.len <= (1ull << 31)) {
        chunks = msm_chunks(ov, m, true, standalone, host_scalars);
        p.tables = msm_seg_shape(chunks.largest(m), srs.table_c, srs.table_T, 1, true, &probe);
    }
    if (!p.tables) chunks = msm_chunks(ov, m, false, standalone, host_scalars);
    if (p.tables) {
        p.c = srs.table_c;
        p.W = srs.table_T;
    }
    const uint32_t c = p.c, W = p.W;
    p.centred = p.tables && srs.table_centred;
    const uint32_t B = 1u << (c - 1);
    // top window: t scalar bits -> 2^t digits, spread over 2^top_v virtual bucket copies
    const uint32_t t_bits = (p.centred ? 254u : 255u) - c * (W - 1);
    const uint32_t top_v = (t_bits >= c - 1) ? 0u : (c - 1 - t_bits);
    // table mode: ONE bucket set for all windows -- the top window's digits d <= 2^t go to the shared
    // buckets d - 1 with their true weight (no virtual copies).  Balanced when t is large (c = 20: t = 15);
    // for a thin top window the heavy-bucket tasks keep it correct, just slower.
    p.nsets = p.tables ? 1u : W;
    p.digit_v = p.tables ? 0u : top_v;
    const uint64_t nb = p.nb = (uint64_t)p.nsets * B;
    if ((uint64_t)W * m >= (1ull << 31)) {
        p.status = MSM_PLAN_TOO_LARGE;   // 32-bit entry indices
        return p;
    }
    const uint32_t scan_blocks = (uint32_t)((nb + SCAN_PER_BLOCK - 1) / SCAN_PER_BLOCK);
    p.nch = chunks.nch;
    p.overlap = p.nch > 1 && standalone;
    p.chain = !standalone && (ov.msm_chain < 0 ? m >= MSM_CHAIN_MIN_TERMS : ov.msm_chain != 0);
    p.scatter_staged = ov.msm_scatter_staged;
    p.buckets = nb * 192;

    auto grow = [](size_t& have, uint64_t want) { have = std::max(have, (size_t)want); };
    for (uint32_t k = 0; k < p.nch; ++k) {
        MsmChunkPlan ck;
        ck.off = chunks.cut(m, k);
        if (ck.off >= m) break;
        ck.mk = chunks.cut(m, k + 1) - ck.off;
        ck.beside = p.overlap && k > 0;   // the first sort has nothing to overlap with
        MsmSortBytes& sz = p.sort[k & 1];
        const uint64_t total = (uint64_t)W * ck.mk;
        grow(sz.keys, total * 4);
        grow(sz.sorted, total * 4);
        grow(sz.counts, nb * 4);
        grow(sz.offsets, (nb + 1) * 4);
        grow(sz.cursor, nb * 4);
        grow(sz.blocksums, (uint64_t)scan_blocks * 4);
        grow(sz.order, nb * 4);
        grow(sz.ohist, (uint64_t)MSM_SCHED_WORDS * 4);
        // heavy-bucket splitting: cap = entries one thread may sum; at most total/cap heavy buckets/tasks
        // 8 x the mean, at least 32 (round 2: 4 x the mean, at least 512).  The accumulate kernel's thread walks a bucket's
        // first cap entries one after the other -- 6.7 us each when it is the last one running -- so a few buckets of 500
        // were a 3.4-ms tail; and the factor is 8 because table mode is not uniform: the top window's 2^t digits land
        // on the first 2^t buckets of the shared set (c = 20: 2.2 x the mean there), which 4 x the mean would already
        // turn into heavy buckets now and then (measured: +0.3 ms per 2^20 MSM for the extra launch's work)
        ck.cap = (uint32_t)std::max<uint64_t>(MSM_CAP_MIN, 8 * ((total + nb - 1) / nb));
        ck.max_tasks = total / MSM_TASK_LEN_MIN + total / ck.cap + 2;   // sum of ceil(count / task length) over buckets > cap
        grow(sz.heavy, ck.max_tasks * 16);
        grow(sz.tasks, ck.max_tasks * 12);
        grow(sz.hpart, ck.max_tasks * 192);
        // segmented sort shape: hb high bucket bits pick the segment, lb <= 8 low bits are sorted in LDS;
        // the level-1 entry packs [i : ibits][j : 4 in table mode][sign][low : lb] into 32 bits
        ck.segsort = msm_seg_shape(ck.mk, c, W, p.nsets, p.tables, &ck.sh);
        if (p.tables && !ck.segsort) {   // unreachable: the largest chunk had a shape
            p.status = MSM_PLAN_NO_TABLE_SORT;
            return p;
        }
        if (ck.segsort) {
            ck.sh.top_v = p.digit_v;
            ck.sh.tlen = p.tables ? (uint32_t)srs.len : 0u;
            ck.sh.centred = p.centred ? 1u : 0u;
            // The sort of an OVERLAPPED chunk (side stream, beside the previous chunk's accumulation) takes 256-thread level-1
            // workgroups -- one 70-register wavefront per SIMD fits next to two 200-register accumulation wavefronts; two
            // do not, and the kernel then waits for the accumulation to drain -- and a raised wavefront priority: its five
            // kernels finish in 0.14 ms instead of trailing the whole accumulation (0.95 ms), and the next accumulation
            // starts 6 us after the previous one instead of 56 (profiles/r06_ab_sort_prio.txt).  The exposed first sort has
            // the chip to itself and takes 512.  NOT for the queued MSMs of a batch: there it is neutral to slightly
            // negative (the sorts steal from another MSM's accumulation what they gain).
            ck.sh.prio = ck.beside ? 1u : 0u;
            const uint64_t nmat = (uint64_t)ck.sh.nseg * ck.sh.nblk;
            grow(sz.blk_hist, nmat * 4);
            grow(sz.blk_base, (nmat + 1) * 4);
            grow(sz.blk_cnt, nmat * 4);
            grow(sz.seg_start, (uint64_t)ck.sh.nseg * 8);
            grow(sz.blocksums, ((nmat + SCAN_PER_BLOCK - 1) / SCAN_PER_BLOCK + scan_blocks + ck.sh.nseg) * 4);
        }
        // lanes per bucket: a short MSM over a small bucket set has few, long buckets -- spread each over L lanes so
        // that the launch fills the chip twice over (>= 2^18 threads: two rounds of two wavefronts per SIMD balance the
        // size-sorted schedule; one round leaves the SIMDs with the largest buckets 30 % behind), while a lane keeps >= 4 terms
        if (ov.msm_lanes) {
            ck.lanes = (uint32_t)ov.msm_lanes;
        } else {
            const uint64_t mean = total / nb;
            while (ck.lanes < 16 && nb * ck.lanes < (1u << 18)) ck.lanes *= 2;
            while (ck.lanes > 1 && mean / ck.lanes < 4) ck.lanes /= 2;
        }
        // two size classes (the larger half of the buckets: `lanes`, the smaller half: lanes / 2) when lanes were
        // chosen from the load; TYPLONK_MSM_LANES forces one class
        ck.split = (ck.lanes >= 2 && !ov.msm_lanes) ? (uint32_t)(nb / 2) : (uint32_t)nb;
        p.chunk.push_back(ck);
    }
    // row/column bucket reduction (RcShape above): c is in 8..20 and a plain MSM has at most 32 windows, so it always applies
    RcShape& sh = p.rcs;
    sh.nsets = p.nsets;
    sh.c1 = c - 1;
    sh.cl = (c - 1 + 1) / 2;
    sh.ch = c - 1 - sh.cl;
    sh.lhc = std::min<uint32_t>(3, sh.ch);
    sh.llc = std::min<uint32_t>(3, sh.cl);
    sh.top_v = p.digit_v;
    const uint64_t nrow = (uint64_t)p.nsets << (sh.c1 - sh.llc), ncol = (uint64_t)p.nsets << (sh.c1 - sh.lhc);
    p.part_a = ncol * 192;
    p.part_b = nrow * 192;
    p.rc_sums = (((uint64_t)p.nsets << sh.ch) + ((uint64_t)p.nsets << sh.cl)) * 192;
    p.rc_bits = (uint64_t)p.nsets * 2 * RC_NB * 64 * 192;
    p.rc_out = (uint64_t)p.nsets * 2 * RC_NB * 192;
    // two launches for small bucket sets, where the reduction is a latency chain; big sets are work-bound and the
    // four-launch form wastes fewer lanes (2^19 buckets: 0.39 ms against 0.49, profiles/r03_shard_variants.jsonl)
    p.rc2 = !ov.msm_rc4 && msm_rc2_ok(sh) && nb <= (1u << 17);
    return p;
}

}  // namespace ty
