// Test-only device harness over the MSM's bucket accumulation (tests/test_gpu_accum.py).
//
// msm_accum.hip is compiled here as a unit, exactly as the library compiles it (same flags, no extra defines).  da_accum takes
// what the bucket sorts hand on -- offsets, sorted, order, and optionally the schedule counters, the heavy-bucket records and the
// task list -- as arrays the caller chose, together with a point array in the SRS's internal form and a bucket array to continue
// from, and runs launch_msm_accum and then launch_msm_heavy on one stream, as msm_queue queues them (msm_host.hip).  It hands back
// every bucket, every task partial and the heavy records with their done counters.  The bucket array and the partials are
// allocated at exactly nb and ntasks points, each followed by a guard band.
// Nothing is launched on arrays a kernel could leave its buffers with: admit() runs on the host before the first HIP call.
// Not linked into libtyplonk_hip.so.  It lives beside the unit it wraps, as device_reduce.hip and device_sort.hip do.
#include "../msm_accum.hip"

#include <vector>

using namespace ty;

namespace {

constexpr size_t GUARD_BYTES = 4096;
constexpr int GUARD_FILL = 0xA5;   // every allocation starts out as this byte, body and band

struct Buf {
    void* p = nullptr;
    size_t bytes = 0;
    uint32_t* u32() const { return static_cast<uint32_t*>(p); }
    // n bytes copied from src (or left as the fill), then the band
    hipError_t make(const void* src, size_t n) {
        bytes = n;
        hipError_t e = hipMalloc(&p, n + GUARD_BYTES);
        if (e == hipSuccess) e = hipMemset(p, GUARD_FILL, n + GUARD_BYTES);
        if (e == hipSuccess && src && n) e = hipMemcpy(p, src, n, hipMemcpyHostToDevice);
        return e;
    }
    bool intact(hipError_t& e) const {
        std::vector<unsigned char> band(GUARD_BYTES);
        if (e == hipSuccess) e = hipMemcpy(band.data(), static_cast<char*>(p) + bytes, GUARD_BYTES, hipMemcpyDeviceToHost);
        bool ok = e == hipSuccess;
        for (size_t i = 0; ok && i < GUARD_BYTES; ++i) ok = band[i] == GUARD_FILL;
        return ok;
    }
    ~Buf() {
        if (p) (void)hipFree(p);
    }
};

struct Args {
    const uint32_t *points, *offsets, *sorted, *order, *buckets_in, *sched, *heavy, *tasks;
    uint64_t npoints, total, max_tasks;
    uint32_t nb, cap, init, lanes, split;
};

// what the kernels' index arithmetic takes for granted
bool admit(const Args& a) {
    if (!a.points || !a.offsets || !a.sorted || !a.order || a.npoints == 0 || a.npoints > (1u << 31)) return false;
    if (a.nb == 0 || a.nb > (1u << 24) || a.total > 0xffffffffull || a.init > 1 || (a.init && !a.buckets_in)) return false;
    if (a.lanes != 1 && a.lanes != 2 && a.lanes != 4 && a.lanes != 8 && a.lanes != 16) return false;
    for (uint32_t g = 0; g < a.nb; ++g)
        if (a.offsets[g] > a.offsets[g + 1]) return false;
    if (a.offsets[a.nb] != a.total) return false;
    for (uint64_t i = 0; i < a.total; ++i)
        if ((a.sorted[i] & 0x7fffffffu) >= a.npoints) return false;
    std::vector<bool> seen(a.nb, false);
    for (uint32_t t = 0; t < a.nb; ++t) {
        if (a.order[t] >= a.nb || seen[a.order[t]]) return false;
        seen[a.order[t]] = true;
    }
    if (!a.sched) return !a.heavy && !a.tasks;
    if (!a.heavy || !a.tasks) return false;
    const uint64_t nheavy = a.sched[512], ntasks = a.sched[513];
    if (nheavy > a.max_tasks || ntasks > a.max_tasks) return false;
    for (uint64_t t = 0; t < ntasks; ++t) {
        const uint32_t lo = a.tasks[3 * t], hi = a.tasks[3 * t + 1], h = a.tasks[3 * t + 2];
        if (lo >= hi || hi > a.total || h >= nheavy) return false;
    }
    for (uint64_t h = 0; h < nheavy; ++h) {
        const uint32_t b = a.heavy[4 * h], t0 = a.heavy[4 * h + 1], k = a.heavy[4 * h + 2], done = a.heavy[4 * h + 3];
        if (b >= a.nb || k == 0 || (uint64_t)t0 + k > ntasks || done != 0) return false;
    }
    return true;
}

}  // namespace

extern "C" int da_guard_bytes() { return (int)GUARD_BYTES; }

// points: npoints records of PT_WORDS words; offsets[nb + 1], sorted[total], order[nb]: one chunk's sort, total = offsets[nb];
// buckets_in: nb * 48 words, the stored buckets (may be NULL with init = 0: the array then starts out as the fill byte);
// sched: NULL, or the 516 schedule words ([512] heavy buckets, [513] tasks) with heavy[4 * max_tasks] and tasks[3 * max_tasks].
// Out: buckets_out[nb * 48]; with sched also partial_out[sched[513] * 48] and heavy_out[4 * sched[512]] (the records, done counters
// included); guards: bit 0 the band behind the buckets, bit 1 the band behind the partials (set: still the fill).
// Returns the HIP error code, hipErrorInvalidValue -- before anything touches the device -- for what admit() refuses.
extern "C" int da_accum(const uint32_t* points, uint64_t npoints, const uint32_t* offsets, const uint32_t* sorted, uint64_t total,
                        const uint32_t* order, uint32_t nb, uint32_t cap, uint32_t init, uint32_t lanes, uint32_t split,
                        const uint32_t* buckets_in, const uint32_t* sched, const uint32_t* heavy, const uint32_t* tasks, uint64_t max_tasks,
                        uint32_t* buckets_out, uint32_t* partial_out, uint32_t* heavy_out, uint32_t* guards) {
    const Args a = {points, offsets, sorted, order, buckets_in, sched, heavy, tasks, npoints, total, max_tasks, nb, cap, init, lanes, split};
    if (!buckets_out || !guards || (sched && (!partial_out || !heavy_out)) || !admit(a)) return (int)hipErrorInvalidValue;
    const uint64_t nheavy = sched ? sched[512] : 0, ntasks = sched ? sched[513] : 0;

    Buf d_points, d_offsets, d_sorted, d_order, d_buckets, d_sched, d_heavy, d_tasks, d_partial;
    hipError_t err = d_points.make(points, (size_t)npoints * PT_WORDS * 4);
    if (err == hipSuccess) err = d_offsets.make(offsets, ((size_t)nb + 1) * 4);
    if (err == hipSuccess) err = d_sorted.make(sorted, (size_t)total * 4);
    if (err == hipSuccess) err = d_order.make(order, (size_t)nb * 4);
    if (err == hipSuccess) err = d_buckets.make(buckets_in, (size_t)nb * 192);
    if (err == hipSuccess && sched) err = d_sched.make(sched, 516 * 4);
    if (err == hipSuccess && sched) err = d_heavy.make(heavy, (size_t)nheavy * 16);
    if (err == hipSuccess && sched) err = d_tasks.make(tasks, (size_t)ntasks * 12);
    if (err == hipSuccess && sched) err = d_partial.make(nullptr, (size_t)ntasks * 192);
    if (err != hipSuccess) return (int)err;

    hipStream_t s = 0;
    launch_msm_accum(d_points.u32(), d_offsets.u32(), d_sorted.u32(), d_order.u32(), nb, cap, init != 0, lanes, split, d_buckets.u32(), s);
    if (sched)
        launch_msm_heavy(d_points.u32(), d_sorted.u32(), d_sched.u32(), d_heavy.u32(), d_tasks.u32(), d_partial.u32(), d_buckets.u32(), s);
    err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err != hipSuccess) return (int)err;

    err = hipMemcpy(buckets_out, d_buckets.p, (size_t)nb * 192, hipMemcpyDeviceToHost);
    if (err == hipSuccess && ntasks) err = hipMemcpy(partial_out, d_partial.p, (size_t)ntasks * 192, hipMemcpyDeviceToHost);
    if (err == hipSuccess && nheavy) err = hipMemcpy(heavy_out, d_heavy.p, (size_t)nheavy * 16, hipMemcpyDeviceToHost);
    const bool g0 = d_buckets.intact(err);
    const bool g1 = sched ? d_partial.intact(err) : true;
    *guards = (g0 ? 1u : 0u) | (g1 ? 2u : 0u);
    return (int)err;
}
