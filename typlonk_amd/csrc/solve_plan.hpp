// Every decision of typlonk_witness_solve that does not need the device: where each cell's value comes from, in which order
// the driven rows can be computed, and which launches compute them.  solve_plan() states them once per (circuit, cosets);
// witness_solve.hip uploads the tables and queues what the plan lists.  No HIP include: the host compiles this header on its
// own (tests/cpp/solve_plan_host.cpp prints the plan, tests/test_solve_plan_host.py holds it against the Python statement of
// the contract, tests/witness_solve_ref.py), like msm_plan.hpp, ntt_plan.hpp and prove_plan.hpp.
//
// The contract (include/typlonk.h has it in full).  Cells are flat indices x = col * n + row; a class is a cycle of the
// permutation.  Row j is DRIVEN iff q_o[j] != 0 mod r; a class is driven iff it holds the c cell 2n + j of a driven row, and its
// driver is the lowest such row; every other class is free and takes an assigned value or 0.  A driven row's c cell gets
//   c_j = (q_l a + q_r b + q_m a b + q_c + PI_j) / q_o      a, b = the values of the classes of cells j and n + j,
// every other cell gets its class's value: src[x] says where that is --
//   src[x] = d                  the c column at row d (a driven row: the class's driver, or x's own row for x = 2n + j, j driven)
//   src[x] = SOLVE_FREE | s     free slot s (slots are numbered by the lowest cell of their class, ascending)
// Row j depends on the rows src[j] and src[n + j] name: level(j) = 1 + the larger of their levels, a free source being level 0.
// A dependency cycle has no levels: SOLVE_CYCLE, with the lowest row that could not be scheduled.
//
// Schedule.  One launch per level wider than `narrow` rows (a thread per row and witness); a maximal run of consecutive levels
// of at most `narrow` rows each is ONE launch of one workgroup per witness, which steps through the levels with a workgroup
// fence and barrier between them -- cut every `run_cut` levels, so that no launch runs unboundedly long.  No launch waits for
// another workgroup: order across workgroups is stream order between launches, nothing else.  One fill launch for the cells of
// the undriven rows ends the call.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace ty {

constexpr uint32_t SOLVE_FREE = 0x80000000u;   // tag of a free source in src[]
constexpr uint32_t SOLVE_NARROW = 256;         // rows per level a run's single workgroup takes (= its threads)
constexpr uint32_t SOLVE_RUN_CUT = 65536;      // levels per run launch at most

enum SolveStatus {
    SOLVE_OK = 0,
    SOLVE_BAD_PERM = 1,   // perm is no bijection of the 3n cells (bad = the lowest cell that shows it)
    SOLVE_CYCLE = 2,      // the rows' dependencies have a cycle (bad = the lowest row that could not be scheduled)
};

// levels [first, first + levels) of the plan (0-based: level l holds order[level_off[l] .. level_off[l + 1]))
struct SolveLaunch {
    uint32_t first, levels;
    bool wide;   // one level, a thread per row; else a run: one workgroup per witness
};

struct SolvePlan {
    SolveStatus status = SOLVE_OK;
    uint32_t bad = 0;
    std::vector<uint32_t> src;         // 3n
    std::vector<uint32_t> level;       // n: 1.. for a driven row, 0 for an undriven one
    std::vector<uint32_t> order;       // the driven rows by level, ascending within a level
    std::vector<uint32_t> level_off;   // depth + 1
    std::vector<SolveLaunch> schedule; // the level launches; the fill launch follows them
    uint64_t driven_rows = 0, free_classes = 0;
    uint32_t depth = 0;
    uint32_t launches() const { return (uint32_t)schedule.size() + 1; }
};

// perm: 3n successors; driven: n flags (q_o != 0 mod r)
inline SolvePlan solve_plan(const uint32_t* perm, const uint8_t* driven, uint64_t n, uint32_t narrow = SOLVE_NARROW,
                            uint32_t run_cut = SOLVE_RUN_CUT) {
    SolvePlan p;
    const uint64_t n3 = 3 * n;
    // a bijection: every entry a cell, every cell the image of one
    {
        std::vector<uint8_t> hit(n3, 0);
        for (uint64_t x = 0; x < n3; ++x) {
            if (perm[x] >= n3 || hit[perm[x]]) {
                p.status = SOLVE_BAD_PERM;
                p.bad = (uint32_t)x;
                return p;
            }
            hit[perm[x]] = 1;
        }
    }
    // classes: walk each cycle from its lowest cell, once for the driver and once to write src
    p.src.assign(n3, 0);
    {
        std::vector<uint8_t> seen(n3, 0);
        for (uint64_t x0 = 0; x0 < n3; ++x0) {
            if (seen[x0]) continue;
            uint32_t driver = SOLVE_FREE;
            uint64_t x = x0;
            do {
                seen[x] = 1;
                if (x >= 2 * n && driven[x - 2 * n] && (uint32_t)(x - 2 * n) < driver) driver = (uint32_t)(x - 2 * n);
                x = perm[x];
            } while (x != x0);
            const uint32_t s = driver != SOLVE_FREE ? driver : SOLVE_FREE | (uint32_t)p.free_classes++;
            do {
                p.src[x] = s;
                x = perm[x];
            } while (x != x0);
        }
    }
    for (uint64_t j = 0; j < n; ++j)
        if (driven[j]) {
            p.src[2 * n + j] = (uint32_t)j;   // a driven row's c cell is its own computed value, driver or not
            ++p.driven_rows;
        }
    // levels: Kahn's pass over the rows; users of row d in CSR form
    p.level.assign(n, 0);
    std::vector<uint32_t> waits(n, 0), ucnt(n + 1, 0);
    auto deps = [&](uint64_t j, uint32_t (&d)[2]) {
        int k = 0;
        for (int i = 0; i < 2; ++i) {
            const uint32_t s = p.src[(uint64_t)i * n + j];
            if (!(s & SOLVE_FREE)) d[k++] = s;
        }
        return k;
    };
    uint32_t d[2];
    for (uint64_t j = 0; j < n; ++j)
        if (driven[j]) {
            const int k = deps(j, d);
            waits[j] = (uint32_t)k;
            for (int i = 0; i < k; ++i) ++ucnt[d[i] + 1];
        }
    for (uint64_t j = 0; j < n; ++j) ucnt[j + 1] += ucnt[j];
    std::vector<uint32_t> users(ucnt[n]), fill(ucnt.begin(), ucnt.end() - 1);
    for (uint64_t j = 0; j < n; ++j)
        if (driven[j]) {
            const int k = deps(j, d);
            for (int i = 0; i < k; ++i) users[fill[d[i]]++] = (uint32_t)j;
        }
    std::vector<uint32_t> queue;
    queue.reserve(p.driven_rows);
    for (uint64_t j = 0; j < n; ++j)
        if (driven[j] && !waits[j]) {
            p.level[j] = 1;
            queue.push_back((uint32_t)j);
        }
    for (size_t h = 0; h < queue.size(); ++h) {
        const uint32_t r = queue[h];
        for (uint32_t u = ucnt[r]; u < ucnt[r + 1]; ++u) {
            const uint32_t j = users[u];
            if (p.level[j] < p.level[r] + 1) p.level[j] = p.level[r] + 1;
            if (--waits[j] == 0) queue.push_back(j);
        }
    }
    if (queue.size() != p.driven_rows) {
        p.status = SOLVE_CYCLE;
        for (uint64_t j = 0; j < n; ++j)
            if (driven[j] && waits[j]) {
                p.bad = (uint32_t)j;
                break;
            }
        return p;
    }
    for (uint32_t r : queue) p.depth = p.level[r] > p.depth ? p.level[r] : p.depth;
    // the rows by level, ascending within a level
    p.level_off.assign((size_t)p.depth + 1, 0);
    for (uint32_t r : queue) ++p.level_off[p.level[r]];
    for (uint32_t l = 0; l < p.depth; ++l) p.level_off[l + 1] += p.level_off[l];
    p.order.resize(p.driven_rows);
    {
        std::vector<uint32_t> at(p.level_off.begin(), p.level_off.end());
        for (uint64_t j = 0; j < n; ++j)
            if (driven[j]) p.order[at[p.level[j] - 1]++] = (uint32_t)j;
    }
    // the launches
    for (uint32_t l = 0; l < p.depth; ++l) {
        const uint32_t width = p.level_off[l + 1] - p.level_off[l];
        if (width > narrow) {
            p.schedule.push_back({l, 1, true});
        } else if (!p.schedule.empty() && !p.schedule.back().wide && p.schedule.back().levels < run_cut) {
            ++p.schedule.back().levels;
        } else {
            p.schedule.push_back({l, 1, false});
        }
    }
    return p;
}

}  // namespace ty
