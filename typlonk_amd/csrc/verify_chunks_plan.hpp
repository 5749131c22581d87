// The launch shape of typlonk_verify_chunks's fold (chunks_fold_kernel and chunks_fold_sum_kernel, verify_chunks.hip), decided on
// the host before anything is queued, in the manner of open_chunks_plan: a pure function of (cells, log_l[, strip]) with no HIP
// include, so that a host program can walk it over a grid (tests/cpp/verify_chunks_plan_host.cpp).
//
// The fold takes `cells` cells of l = 2^log_l evaluations each and gives l coefficients.  A workgroup of 256 threads takes a STRIP
// of consecutive cells; within it a GROUP of threads works on one cell at a time: a wavefront (64 threads, 4 groups a workgroup)
// for l <= 64, the whole workgroup above.  A group holds its cell's l elements in the LDS for the radix-2 inverse transform, and
// thread q of the group keeps the accumulators of the coefficients q, q + group, ... (`per` of them, in registers).  After its
// strip a workgroup writes ONE vector of l partial coefficients, and chunks_fold_sum_kernel adds the `blocks` vectors in
// workgroup order.  The strip is the smallest that keeps the partial vectors at or below VERIFY_CHUNKS_MAX_BLOCKS -- the sum
// kernel's thread walks them one by one -- and never below one cell per group; a caller (the test harness) may name another.
// The number of workgroups is NOT monotone in the cells (4097 cells of l = 128: strips of 3, 1366 workgroups; 2048 cells: strips of
// 1, 2048 workgroups), so a caller that folds sub-ranges into a buffer sized for the whole call -- the bisection of
// verify_chunks_host.hip -- plans every sub-range with the whole call's strip: ceil(c / strip) <= ceil(cells / strip) for c <= cells.
// LDS: groups * l elements of 32 bytes (at most 32 KiB, at l = 1024) and the table of the l / 2 inverse twiddles (at most 16 KiB).
#pragma once
#include <cstdint>

namespace ty {

constexpr uint32_t VERIFY_CHUNKS_MAX_LOG_L = 10;        // one cell's elements fill 32 KiB of LDS
constexpr uint32_t VERIFY_CHUNKS_THREADS = 256;
constexpr uint32_t VERIFY_CHUNKS_WAVE = 64;
constexpr uint64_t VERIFY_CHUNKS_MAX_BLOCKS = 2048;     // 256 CUs x 8 workgroups: the device is filled well before
constexpr uint32_t VERIFY_CHUNKS_FR_BYTES = 32;
constexpr uint32_t VERIFY_CHUNKS_LDS_CELLS_MAX = 32u << 10;   // the bound on the cells' share of the LDS

struct VerifyChunksPlan {
    uint32_t group;      // threads that work on one cell: 64 for l <= 64, else 256
    uint32_t groups;     // cells a workgroup works on at once: 256 / group
    uint32_t per;        // coefficients (and accumulators) per thread: max(1, l / group)
    uint32_t iters;      // cells a group takes one after the other: ceil(strip / groups), the same in every workgroup
    uint64_t strip;      // cells per workgroup; workgroup b takes cells [b * strip, min((b + 1) * strip, cells))
    uint64_t blocks;     // workgroups = partial vectors of l coefficients
    uint32_t tw;         // entries of the twiddle table: max(l / 2, 1)
    uint32_t lds_cells;  // bytes: groups * l * 32
    uint32_t lds_bytes;  // lds_cells + tw * 32
};

// cells >= 1, log_l <= VERIFY_CHUNKS_MAX_LOG_L; strip = 0: the plan's own
inline VerifyChunksPlan verify_chunks_plan(uint64_t cells, uint32_t log_l, uint64_t strip = 0) {
    VerifyChunksPlan p;
    const uint32_t l = 1u << log_l;
    p.group = l <= VERIFY_CHUNKS_WAVE ? VERIFY_CHUNKS_WAVE : VERIFY_CHUNKS_THREADS;
    p.groups = VERIFY_CHUNKS_THREADS / p.group;
    p.per = l > p.group ? l / p.group : 1;
    if (!strip) {
        strip = (cells + VERIFY_CHUNKS_MAX_BLOCKS - 1) / VERIFY_CHUNKS_MAX_BLOCKS;
        if (strip < p.groups) strip = p.groups;
    }
    p.strip = strip;
    p.iters = (uint32_t)((strip + p.groups - 1) / p.groups);
    p.blocks = (cells + strip - 1) / strip;
    p.tw = l >= 2 ? l / 2 : 1;
    p.lds_cells = p.groups * l * VERIFY_CHUNKS_FR_BYTES;
    p.lds_bytes = p.lds_cells + p.tw * VERIFY_CHUNKS_FR_BYTES;
    return p;
}

}  // namespace ty
