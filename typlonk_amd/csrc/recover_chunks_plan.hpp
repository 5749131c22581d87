// Every decision of a typlonk_recover_chunks call (include/typlonk.h; kernels: recover_chunks.hip; host: recover_chunks_host.hip),
// made on the host before anything is queued, in the manner of verify_chunks_plan: pure functions of the call's arguments with
// no HIP include, so that a host program can walk them over a table of cases (tests/cpp/recover_chunks_plan_host.cpp).
//
//   recover_chunks_refusal  the refusals of the call in the order the header states them: the first that applies, or none
//   recover_chunks_plan     the sizes of the temporaries and the launch shapes
//
// The vanishing products.  2r values -- Zd[k] = Z'(a_k), then Zc[i] = Z'(g^l a_i), Z'(Y) = prod over the `missing` a_j of (Y - a_j)
// -- one thread each, 256 a workgroup, `missing` factors a thread.  With r = 128 that is ONE workgroup, so the missing set is
// cut into `slices` runs of `per_slice` factors (blockIdx.y), each writing a partial product, and a second kernel multiplies
// the partials in slice order: as many slices as bring the launch to RECOVER_TARGET_BLOCKS workgroups, none shorter than
// RECOVER_MIN_SLICE factors, at most RECOVER_MAX_SLICES.  With r = 2^16 the 512 workgroups of one slice fill the device and
// nothing is split.  A workgroup stages its slice through the LDS RECOVER_TILE values at a time, `tiles` times.
//
// The scatter.  V[p][k + r t] = E_p[pos[k]][t] Zd[k]: the read runs along t, the write along k, so a workgroup moves a tile of
// 2^log_tk cosets x 2^log_tt points (256 elements, fewer only when n < 256) through the LDS; the tile is as square as r and l
// allow (16 x 16: 512-byte runs on both sides) and degenerates to 256 x 1 at l = 1 and 2 x 128 at r = 2.  In the LDS a coset's row
// is padded by one element (not at l = 1), so that the column a run reads on the way out does not fall into one set of banks.
//
// The finish.  The lowest nonzero index of [m, K l) per polynomial: `excess_blocks` workgroups a polynomial, each over a span of
// `excess_span` indices in `excess_iters` steps of 256, then a minimum over the workgroups in their order.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

namespace ty {

constexpr uint32_t RECOVER_MAX_LOG_N = 24;
constexpr uint32_t RECOVER_MAX_LOG_R = 16;            // the products are quadratic in r: at most 2^17 values x 2^16 factors
constexpr uint64_t RECOVER_MAX_ELEMS = 1ull << 26;    // count * n
constexpr uint32_t RECOVER_THREADS = 256;
constexpr uint32_t RECOVER_TILE = 256;                // missing a_j staged in the LDS at a time: 8 KiB
constexpr uint32_t RECOVER_TARGET_BLOCKS = 512;       // 256 CUs x 2
constexpr uint32_t RECOVER_MIN_SLICE = 8;
constexpr uint32_t RECOVER_MAX_SLICES = 64;
constexpr uint32_t RECOVER_EXCESS_SPAN = 4096;        // indices a workgroup scans at least (16 a thread)
constexpr uint32_t RECOVER_EXCESS_MAX_BLOCKS = 256;
constexpr uint32_t RECOVER_FR_BYTES = 32;
constexpr uint32_t RECOVER_SCATTER_LDS = 384;        // elements of the scatter's tile: rows of TT + 1 for TT > 1, at most 128 (17/16 of 256 < 384)
constexpr uint32_t RECOVER_NO_CELL = 0xffffffffu;     // pos[k] of a coset the call does not name

// the codes of include/typlonk.h a refusal maps to (recover_chunks_host.hip asserts the equalities)
enum RecoverRefusal : int {
    RECOVER_ADMITTED = 0,
    RECOVER_INVALID_ARG = -1,
    RECOVER_LENGTH = -2,
    RECOVER_DOMAIN = -3,
    RECOVER_RANGE = -7,
};

// The arguments of a call as the refusals see them.  A device buffer is its identity and its length in elements.
struct RecoverChunksArgs {
    bool ctx, evals, status, report;          // non-null
    uint32_t log_n, log_l;
    uint64_t m;
    const uint32_t* cosets;
    uint64_t K, count;
    bool want_dev, want_coeffs, want_evals;   // coeffs_dev, coeffs, evals_out non-null
    const void* const* buf_id;                // want_dev: `count` entries, NULL = a null entry of coeffs_dev
    const uint64_t* buf_len;                  // want_dev: the elements each holds
    const uint64_t* offsets;                  // NULL: all zero
};

struct RecoverVerdict {
    int code;
    const char* text;
};

inline RecoverVerdict recover_chunks_refusal(const RecoverChunksArgs& a) {
    if (!a.ctx || !a.cosets || !a.evals || !a.status || !a.report) return {RECOVER_INVALID_ARG, "null argument"};
    if (!a.want_dev && !a.want_coeffs && !a.want_evals) return {RECOVER_INVALID_ARG, "no output: coeffs_dev, coeffs and evals_out are all null"};
    if (a.want_dev) {
        if (!a.buf_id || !a.buf_len) return {RECOVER_INVALID_ARG, "null argument"};
        // (count = 0 is refused below: no entry is read for it)
        for (uint64_t p = 0; p < a.count; ++p)
            if (!a.buf_id[p]) return {RECOVER_INVALID_ARG, "null entry of coeffs_dev"};
    }
    if (a.log_n < 1 || a.log_n > RECOVER_MAX_LOG_N) return {RECOVER_DOMAIN, "log_n outside 1..24"};
    if (a.log_l >= a.log_n) return {RECOVER_DOMAIN, "log_l >= log_n: the domain is cut into at least two cosets"};
    if (a.log_n - a.log_l > RECOVER_MAX_LOG_R) return {RECOVER_DOMAIN, "log_n - log_l > 16: the vanishing products are quadratic in the number of cosets"};
    const uint64_t n = 1ull << a.log_n, l = 1ull << a.log_l, r = n >> a.log_l;
    if (a.K == 0) return {RECOVER_LENGTH, "a call takes at least one cell per polynomial"};
    if (a.K > r) return {RECOVER_LENGTH, "more cells than cosets"};
    if (a.count == 0) return {RECOVER_LENGTH, "a call takes at least one polynomial"};
    if (a.m == 0) return {RECOVER_LENGTH, "a degree bound of at least one coefficient"};
    if (a.m > a.K * l) return {RECOVER_LENGTH, "too few cells for this degree bound"};
    if (a.count > RECOVER_MAX_ELEMS / n) return {RECOVER_LENGTH, "count * n > 2^26 elements"};
    for (uint64_t i = 0; i < a.K; ++i)
        if (a.cosets[i] >= r) return {RECOVER_RANGE, "a coset >= r"};
    if (a.want_dev)
        for (uint64_t p = 0; p < a.count; ++p) {
            const uint64_t off = a.offsets ? a.offsets[p] : 0;
            if (off > a.buf_len[p] || a.m > a.buf_len[p] - off) return {RECOVER_RANGE, "range outside buffer"};
        }
    // r <= 2^16 here: a mark per coset, no allocation
    {
        uint64_t seen[(1u << RECOVER_MAX_LOG_R) / 64] = {};
        for (uint64_t i = 0; i < a.K; ++i) {
            const uint32_t k = a.cosets[i];
            if (seen[k >> 6] >> (k & 63) & 1) return {RECOVER_INVALID_ARG, "a coset named twice"};
            seen[k >> 6] |= 1ull << (k & 63);
        }
    }
    if (a.want_dev && a.count > 1) {   // sorted by (buffer, offset), two ranges of one buffer overlap iff two neighbours do
        std::vector<uint64_t> by(a.count);
        for (uint64_t p = 0; p < a.count; ++p) by[p] = p;
        auto off = [&](uint64_t p) { return a.offsets ? a.offsets[p] : 0; };
        std::sort(by.begin(), by.end(), [&](uint64_t p, uint64_t q) {
            return a.buf_id[p] != a.buf_id[q] ? std::less<const void*>()(a.buf_id[p], a.buf_id[q]) : off(p) < off(q);
        });
        for (uint64_t i = 1; i < a.count; ++i)
            if (a.buf_id[by[i]] == a.buf_id[by[i - 1]] && off(by[i]) - off(by[i - 1]) < a.m)
                return {RECOVER_INVALID_ARG, "the same range of one buffer given for two polynomials"};
    }
    return {RECOVER_ADMITTED, ""};
}

struct RecoverChunksPlan {
    uint64_t n, l, r, known, missing;
    // the vanishing products
    uint32_t tile;            // RECOVER_TILE
    uint32_t vanish_xblocks;  // ceil(2r / 256)
    uint32_t slices;          // blockIdx.y of recover_vanish_kernel; partial products per value
    uint64_t per_slice;       // factors a slice takes: slice s has [s per_slice, min((s + 1) per_slice, missing))
    uint32_t tiles;           // ceil(per_slice / tile), the same in every workgroup
    // the scatter
    uint32_t log_tk, log_tt;  // a tile: 2^log_tk cosets x 2^log_tt points, at most 256 elements
    uint64_t scatter_tiles;   // per polynomial: n >> (log_tk + log_tt)
    // the finish
    uint64_t excess_len;      // K l - m
    uint32_t excess_blocks;   // workgroups a polynomial, at least one
    uint64_t excess_span;     // indices each takes
    uint32_t excess_iters;    // ceil(excess_span / 256)
    // bytes of the temporaries
    uint64_t bytes_consts;    // a_k, the shifted powers beside them, Zd, Zc: 4 r elements
    uint64_t bytes_partial;   // slices * 2 r elements
    uint64_t bytes_index;     // pos (r) and the missing list (max(missing, 1)), 32-bit words
    uint64_t bytes_cells;     // count * K * l elements
    uint64_t bytes_work;      // count * n elements
    uint64_t bytes_out;       // count * m elements when coeffs or evals_out is given, else 0
    uint64_t bytes_evals;     // count * n elements when evals_out is given, else 0
    uint64_t bytes_verdict;   // per polynomial: first_excess and status (two 64-bit words), the fixed flag (a byte), the
                              // destination (a pointer), and excess_blocks 64-bit partial minima
    uint64_t bytes_total;
};

// an admitted call's shape (recover_chunks_refusal gave RECOVER_ADMITTED); named_slices = 0: the plan's own
inline RecoverChunksPlan recover_chunks_plan(uint32_t log_n, uint32_t log_l, uint64_t m, uint64_t K, uint64_t count, bool want_out, bool want_evals,
                                             uint32_t named_slices = 0) {
    RecoverChunksPlan p;
    const uint32_t log_r = log_n - log_l;
    p.n = 1ull << log_n;
    p.l = 1ull << log_l;
    p.r = 1ull << log_r;
    p.known = K;
    p.missing = p.r - K;
    p.tile = RECOVER_TILE;
    p.vanish_xblocks = (uint32_t)((2 * p.r + RECOVER_THREADS - 1) / RECOVER_THREADS);
    uint64_t s = RECOVER_TARGET_BLOCKS / p.vanish_xblocks;
    const uint64_t by_len = p.missing / RECOVER_MIN_SLICE;
    if (s > by_len) s = by_len;
    if (s > RECOVER_MAX_SLICES) s = RECOVER_MAX_SLICES;
    if (s < 1) s = 1;
    if (named_slices) s = named_slices;   // (the test harness: every slicing gives the same words)
    p.per_slice = (p.missing + s - 1) / s;
    if (p.per_slice < 1) p.per_slice = 1;                           // (missing = 0: one slice of no factor)
    p.slices = p.missing ? (uint32_t)((p.missing + p.per_slice - 1) / p.per_slice) : 1;   // no slice without a factor
    p.tiles = (uint32_t)((p.per_slice + p.tile - 1) / p.tile);
    uint32_t tt = log_l < 4 ? log_l : 4;
    p.log_tk = log_r < 8 - tt ? log_r : 8 - tt;
    p.log_tt = log_l < 8 - p.log_tk ? log_l : 8 - p.log_tk;
    p.scatter_tiles = p.n >> (p.log_tk + p.log_tt);
    p.excess_len = K * p.l - m;
    uint64_t eb = (p.excess_len + RECOVER_EXCESS_SPAN - 1) / RECOVER_EXCESS_SPAN;
    if (eb > RECOVER_EXCESS_MAX_BLOCKS) eb = RECOVER_EXCESS_MAX_BLOCKS;
    if (eb < 1) eb = 1;
    p.excess_span = (p.excess_len + eb - 1) / eb;
    p.excess_blocks = p.excess_span ? (uint32_t)((p.excess_len + p.excess_span - 1) / p.excess_span) : 1;
    p.excess_iters = (uint32_t)((p.excess_span + RECOVER_THREADS - 1) / RECOVER_THREADS);
    p.bytes_consts = 4 * p.r * RECOVER_FR_BYTES;
    p.bytes_partial = (uint64_t)p.slices * 2 * p.r * RECOVER_FR_BYTES;
    p.bytes_index = (p.r + (p.missing ? p.missing : 1)) * 4;
    p.bytes_cells = count * K * p.l * RECOVER_FR_BYTES;
    p.bytes_work = count * p.n * RECOVER_FR_BYTES;
    p.bytes_out = want_out || want_evals ? count * m * RECOVER_FR_BYTES : 0;
    p.bytes_evals = want_evals ? count * p.n * RECOVER_FR_BYTES : 0;
    p.bytes_verdict = count * (16 + 1 + 8 + 8ull * p.excess_blocks);
    p.bytes_total = p.bytes_consts + p.bytes_partial + p.bytes_index + p.bytes_cells + p.bytes_work + p.bytes_out + p.bytes_evals + p.bytes_verdict;
    return p;
}

}  // namespace ty
