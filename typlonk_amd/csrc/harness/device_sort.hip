// Test-only device harness over the MSM's bucket sorts (tests/test_gpu_msm_sort.py).
//
// msm_sort.hip is compiled here as a unit, exactly as the library compiles it (same flags, no extra defines).  ds_sort plans an
// MSM with msm_plan() as msm_enqueue does, allocates ONE chunk's sort buffers at exactly the byte sizes of the plan, each
// followed by a guard band, runs that chunk's sort as msm_queue runs it (msm_host.hip) -- the segmented sort in the shape the
// plan gave the chunk, or the atomic counting sort -- and hands back everything the sort passes on to the accumulation:
// counts, offsets, sorted, order, the schedule counters, the heavy-bucket lists, and whether every guard band is intact.
// force_atomic takes the atomic counting sort where the plan says segmented: its launchers take (m, c, W, digit_v, nb, cap) and
// no MsmShape, so every length is within their contract; a segmented shape the plan did not produce is never run.
// Not linked into libtyplonk_hip.so.  It lives beside the unit it wraps, as device_reduce.hip does.
#include "../msm_sort.hip"

#include <cstring>
#include <vector>

using namespace ty;

namespace {

constexpr size_t GUARD_BYTES = 4096;
constexpr int GUARD_FILL = 0xA5;   // every allocation starts out as this byte, body and band: the sort gets no zeroed memory

// the buffers of one SortBufs set the sort touches, in the order of the guard bits ds_sort reports
enum { B_KEYS, B_SORTED, B_COUNTS, B_OFFSETS, B_CURSOR, B_BLOCKSUMS, B_ORDER, B_OHIST, B_BLK_HIST, B_BLK_BASE, B_BLK_CNT, B_SEG_START,
       B_HEAVY, B_TASKS, B_SCALARS, N_BUFS };

struct Bufs {
    void* p[N_BUFS] = {};
    size_t bytes[N_BUFS] = {};
    hipError_t err = hipSuccess;
    void alloc(int which, size_t n) {
        bytes[which] = n;
        if (err == hipSuccess) err = hipMalloc(&p[which], n + GUARD_BYTES);
        if (err == hipSuccess) err = hipMemset(p[which], GUARD_FILL, n + GUARD_BYTES);
    }
    uint32_t* u32(int which) const { return static_cast<uint32_t*>(p[which]); }
    // bit b set: the band behind buffer b still holds the fill
    uint32_t intact() {
        uint32_t bits = 0;
        std::vector<unsigned char> band(GUARD_BYTES);
        for (int b = 0; b < N_BUFS; ++b) {
            if (err == hipSuccess) err = hipMemcpy(band.data(), static_cast<char*>(p[b]) + bytes[b], GUARD_BYTES, hipMemcpyDeviceToHost);
            bool ok = err == hipSuccess;
            for (size_t i = 0; ok && i < GUARD_BYTES; ++i) ok = band[i] == GUARD_FILL;
            bits |= ok ? 1u << b : 0u;
        }
        return bits;
    }
    ~Bufs() {
        for (void* q : p)
            if (q) (void)hipFree(q);
    }
};

// the plan of the caller's MSM as msm_enqueue makes it; T and centred from the window as typlonk_srs_precompute derives them
bool plan_of(uint64_t m, int mode, uint64_t srs_len, uint32_t table_c, int ov_chunks, int ov_staged, MsmPlan* plan) {
    if (m == 0 || m > srs_len || (mode != 0 && mode != 2) || ov_chunks < 0 || ov_chunks > MSM_MAX_CHUNKS) return false;
    MsmSrsFacts facts;
    facts.len = (size_t)srs_len;
    if (table_c) {
        if (table_c < 14 || table_c > 20 || srs_len > ((uint64_t)1 << 25)) return false;
        const bool centred = msm_windows(table_c, true) < msm_windows(table_c, false);
        const uint32_t T = msm_windows(table_c, centred);
        if (!msm_table_srs_ok((size_t)srs_len, table_c, T)) return false;
        facts.table_c = table_c;
        facts.table_T = T;
        facts.table_centred = centred;
    }
    MsmOverrides ov;
    ov.msm_chunks = ov_chunks;
    ov.msm_scatter_staged = ov_staged != 0;
    *plan = msm_plan(facts, (size_t)m, mode != 2, false, ov);
    return plan->status == MSM_PLAN_OK;
}

constexpr int INFO_WORDS = 32;
enum { I_C, I_W, I_DIGIT_V, I_NB, I_CAP, I_SEGSORT, I_SHAPE /* 14 words */, I_STAGED = I_SHAPE + 14, I_NCH, I_OFF, I_MK, I_MAX_TASKS,
       I_TABLES, I_CENTRED, I_ATOMIC, I_GUARDS, I_HEAVY, I_NTASKS, I_END };
static_assert(I_END <= INFO_WORDS, "info words");

void plan_info(const MsmPlan& plan, uint32_t k, uint32_t* info) {
    const MsmChunkPlan& ck = plan.chunk[k];
    const MsmShape& s = ck.sh;
    const uint32_t shape[14] = {s.c, s.W, s.top_v, s.hb, s.lb, s.nseg, s.nblk, s.chunk, s.ibits, s.jbits, s.tlen, s.nsets, s.centred, s.prio};
    memset(info, 0, INFO_WORDS * sizeof(uint32_t));
    info[I_C] = plan.c;
    info[I_W] = plan.W;
    info[I_DIGIT_V] = plan.digit_v;
    info[I_NB] = (uint32_t)plan.nb;
    info[I_CAP] = ck.cap;
    info[I_SEGSORT] = ck.segsort ? 1u : 0u;
    memcpy(info + I_SHAPE, shape, sizeof(shape));
    info[I_NCH] = (uint32_t)plan.chunk.size();
    info[I_OFF] = (uint32_t)ck.off;
    info[I_MK] = (uint32_t)ck.mk;
    info[I_MAX_TASKS] = (uint32_t)ck.max_tasks;
    info[I_TABLES] = plan.tables ? 1u : 0u;
    info[I_CENTRED] = plan.centred ? 1u : 0u;
}

// whether launch_msm_segsort_c<C> takes the LDS-staged level-1 scatter for this shape (its own condition, restated)
template <uint32_t C>
bool staged_taken(const MsmShape& sh, bool staged_mode) {
    const size_t lds = msm_staged_lds(sh);
    return staged_mode && sh.nseg <= 8192 && lds <= 160 * 1024 && (lds <= 64 * 1024 || msm_staged_raise_lds<C>());
}

}  // namespace

extern "C" int ds_info_words() { return INFO_WORDS; }

// the plan's numbers for chunk k, without touching the device: info[] as ds_sort fills it, up to I_CENTRED
extern "C" int ds_plan(uint64_t m, int mode, uint64_t srs_len, uint32_t table_c, int ov_chunks, int ov_staged, uint32_t k, uint32_t* info) {
    MsmPlan plan;
    if (!info || !plan_of(m, mode, srs_len, table_c, ov_chunks, ov_staged, &plan) || k >= plan.chunk.size()) return (int)hipErrorInvalidValue;
    plan_info(plan, k, info);
    return 0;
}

// scalars: m Montgomery residues (8 words each); mode 0 stand-alone, 2 queued; (srs_len, table_c): the SRS, table_c = 0 plain;
// ov_chunks / ov_staged: the overrides msm_chunks (0 = the plan's own) and msm_scatter_staged; k: the chunk.
// Out (sizes from ds_plan): info[ds_info_words()], counts[nb], offsets[nb + 1], sorted[W * mk], order[nb], sched[514] (the schedule
// words 0..513), heavy[4 * max_tasks], tasks[3 * max_tasks]; sorted is filled up to offsets[nb], heavy and tasks up to the
// counters in sched[512] and sched[513] (each no further than the size above).
// Returns the HIP error code, hipErrorInvalidValue for what the plan refuses and for a chunk the plan does not have.
extern "C" int ds_sort(const uint32_t* scalars, uint64_t m, int mode, uint64_t srs_len, uint32_t table_c, int ov_chunks, int ov_staged,
                       uint32_t k, int force_atomic, uint32_t* info, uint32_t* counts, uint32_t* offsets, uint32_t* sorted, uint32_t* order,
                       uint32_t* sched, uint32_t* heavy, uint32_t* tasks) {
    MsmPlan plan;
    if (!scalars || !info || !plan_of(m, mode, srs_len, table_c, ov_chunks, ov_staged, &plan) || k >= plan.chunk.size())
        return (int)hipErrorInvalidValue;
    // the atomic sort knows neither tables nor centred scalars (a table-mode plan without a segmented shape is refused by the plan)
    if (force_atomic && plan.tables) return (int)hipErrorInvalidValue;
    const MsmChunkPlan& ck = plan.chunk[k];
    const MsmSortBytes& z = plan.sort[k & 1];
    const uint32_t nb = (uint32_t)plan.nb;
    const uint64_t total = (uint64_t)plan.W * ck.mk;
    plan_info(plan, k, info);
    const bool atomic = force_atomic != 0 || !ck.segsort;
    info[I_ATOMIC] = atomic ? 1u : 0u;

    Bufs b;
    const size_t want[N_BUFS] = {z.keys, z.sorted, z.counts, z.offsets, z.cursor, z.blocksums, z.order, z.ohist, z.blk_hist, z.blk_base,
                                 z.blk_cnt, z.seg_start, z.heavy, z.tasks, (size_t)m * sizeof(Fr)};
    for (int i = 0; i < N_BUFS; ++i) b.alloc(i, want[i]);
    if (b.err == hipSuccess) b.err = hipMemcpy(b.p[B_SCALARS], scalars, (size_t)m * sizeof(Fr), hipMemcpyHostToDevice);
    if (b.err != hipSuccess) return (int)b.err;

    const Fr* sc = static_cast<const Fr*>(b.p[B_SCALARS]) + ck.off;
    hipStream_t s = 0;
    if (!atomic) {
        const MsmSortPtrs p = {b.u32(B_BLK_HIST), b.u32(B_BLK_BASE), b.u32(B_BLOCKSUMS), b.u32(B_BLK_CNT), b.u32(B_SEG_START), b.u32(B_KEYS),
                               b.u32(B_COUNTS), b.u32(B_OFFSETS), b.u32(B_SORTED), b.u32(B_OHIST), b.u32(B_HEAVY), b.u32(B_TASKS),
                               b.u32(B_ORDER)};
        const MsmShape& sh = ck.sh;
        info[I_STAGED] = sh.c == 20 ? staged_taken<20>(sh, plan.scatter_staged) : sh.c == 17 ? staged_taken<17>(sh, plan.scatter_staged)
                         : sh.c == 15 ? staged_taken<15>(sh, plan.scatter_staged) : staged_taken<0>(sh, plan.scatter_staged);
        launch_msm_segsort(sc, (uint64_t)ck.mk, sh, p, ck.cap, plan.scatter_staged ? 1 : 0, s);
    } else {
        b.err = hipMemsetAsync(b.p[B_COUNTS], 0, plan.nb * 4, s);
        launch_msm_digits(sc, (uint64_t)ck.mk, plan.c, plan.W, plan.digit_v, b.u32(B_KEYS), b.u32(B_COUNTS), s);
        launch_scan(b.u32(B_COUNTS), plan.nb, b.u32(B_BLOCKSUMS), b.u32(B_OFFSETS), b.u32(B_CURSOR), s);
        launch_msm_scatter(b.u32(B_KEYS), (uint64_t)ck.mk, total, b.u32(B_CURSOR), b.u32(B_SORTED), s);
        launch_bucket_order(b.u32(B_COUNTS), b.u32(B_OFFSETS), nb, ck.cap, b.u32(B_OHIST), b.u32(B_ORDER), b.u32(B_HEAVY), b.u32(B_TASKS), s);
    }
    if (b.err == hipSuccess) b.err = hipGetLastError();
    if (b.err == hipSuccess) b.err = hipDeviceSynchronize();
    if (b.err != hipSuccess) return (int)b.err;

    auto back = [&](void* dst, int which, size_t bytes) {
        if (dst && bytes && b.err == hipSuccess) b.err = hipMemcpy(dst, b.p[which], bytes, hipMemcpyDeviceToHost);
    };
    back(counts, B_COUNTS, (size_t)nb * 4);
    back(offsets, B_OFFSETS, ((size_t)nb + 1) * 4);
    back(order, B_ORDER, (size_t)nb * 4);
    uint32_t words[514] = {};
    back(words, B_OHIST, sizeof(words));
    if (sched) memcpy(sched, words, sizeof(words));
    uint32_t emitted = 0;
    if (b.err == hipSuccess) b.err = hipMemcpy(&emitted, b.u32(B_OFFSETS) + nb, 4, hipMemcpyDeviceToHost);
    back(sorted, B_SORTED, (size_t)std::min<uint64_t>(emitted, total) * 4);
    back(heavy, B_HEAVY, (size_t)std::min<uint64_t>(words[512], ck.max_tasks) * 16);
    back(tasks, B_TASKS, (size_t)std::min<uint64_t>(words[513], ck.max_tasks) * 12);
    info[I_HEAVY] = words[512];
    info[I_NTASKS] = words[513];
    info[I_GUARDS] = b.intact();
    return (int)b.err;
}

extern "C" int ds_guard_buffers() { return N_BUFS; }
