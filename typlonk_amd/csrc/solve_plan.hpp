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
// Hints (typlonk_circuit_set_hints).  Hint h says: the free class of cell dst takes f(the value the solve writes to cell src).
//   src[x] = SOLVE_HINT | h     hint h's value, for every cell x of the class of hints[h].dst
// It is one more node of the dependency graph: level(h) = 1 + the level of src[hints[h].src], and a row that reads a hinted class
// counts the hint's level.  The level lists carry both: within a level the rows, ascending, then the hints (SOLVE_HINT | h),
// ascending, so a wavefront of a level is all rows or all hints except at one boundary; a level's width is rows + hints.  A
// cycle through hints names the lowest unschedulable row, or the lowest such hint if every row could be scheduled.
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
constexpr uint32_t SOLVE_HINT = 0xc0000000u;   // tag of a hinted source in src[] (a free class a hint computes), and of a hint in order[]
constexpr uint32_t SOLVE_NARROW = 256;         // entries per level a run's single workgroup takes (= its threads)
constexpr uint32_t SOLVE_RUN_CUT = 65536;      // levels per run launch at most
constexpr uint32_t SOLVE_HINT_INV0 = 1, SOLVE_HINT_BITS = 2;   // TYPLONK_HINT_*

constexpr bool solve_is_hint(uint32_t s) { return (s & SOLVE_HINT) == SOLVE_HINT; }

// typlonk_hint (include/typlonk.h), field for field
struct SolveHint {
    uint32_t kind, dst, src;
    uint16_t shift, width;
};

enum SolveStatus {
    SOLVE_OK = 0,
    SOLVE_BAD_PERM = 1,   // perm is no bijection of the 3n cells (bad = the lowest cell that shows it)
    SOLVE_CYCLE = 2,      // the dependencies have a cycle (bad = the lowest row that could not be scheduled)
    // the hints' refusals: bad = the lowest offending hint
    SOLVE_HINT_KIND = 3,    // an unknown kind
    SOLVE_HINT_CELL = 4,    // dst or src is no cell
    SOLVE_HINT_RANGE = 5,   // width outside 1..64 or shift > 254
    SOLVE_HINT_DRIVEN = 6,  // dst lies in a driven class
    SOLVE_HINT_CLASH = 7,   // dst lies in the class hint `other` (a lower one) writes
    SOLVE_HINT_CYCLE = 8,   // a cycle that every row escapes: bad = the lowest hint that could not be scheduled
};

// levels [first, first + levels) of the plan (0-based: level l holds order[level_off[l] .. level_off[l + 1]))
struct SolveLaunch {
    uint32_t first, levels;
    bool wide;   // one level, a thread per entry; else a run: one workgroup per witness
};

struct SolvePlan {
    SolveStatus status = SOLVE_OK;
    uint32_t bad = 0, other = 0;
    std::vector<uint32_t> src;         // 3n
    std::vector<uint32_t> level;       // n: 1.. for a driven row, 0 for an undriven one
    std::vector<uint32_t> hint_level;  // one per hint, 1..
    std::vector<uint32_t> order;       // the driven rows and the hints (SOLVE_HINT | h) by level: rows ascending, then hints ascending
    std::vector<uint32_t> level_off;   // depth + 1
    std::vector<SolveLaunch> schedule; // the level launches; the fill launch follows them
    uint64_t driven_rows = 0, free_classes = 0;
    uint32_t depth = 0;
    uint32_t launches() const { return (uint32_t)schedule.size() + 1; }
};

// perm: 3n successors; driven: n flags (q_o != 0 mod r); hints: n_hints of them (may be null when there is none)
inline SolvePlan solve_plan(const uint32_t* perm, const uint8_t* driven, uint64_t n, const SolveHint* hints, size_t n_hints,
                            uint32_t narrow = SOLVE_NARROW, uint32_t run_cut = SOLVE_RUN_CUT) {
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
    // hints: each takes over the free class of its dst (the class keeps its slot number, which no cell names any more)
    for (size_t h = 0; h < n_hints; ++h) {
        const SolveHint& t = hints[h];
        p.bad = (uint32_t)h;
        if (t.kind != SOLVE_HINT_INV0 && t.kind != SOLVE_HINT_BITS) p.status = SOLVE_HINT_KIND;
        else if (t.dst >= n3 || t.src >= n3) p.status = SOLVE_HINT_CELL;
        else if (t.kind == SOLVE_HINT_BITS && (t.width < 1 || t.width > 64 || t.shift > 254)) p.status = SOLVE_HINT_RANGE;
        else if (!(p.src[t.dst] & SOLVE_FREE)) p.status = SOLVE_HINT_DRIVEN;
        else if (solve_is_hint(p.src[t.dst])) {
            p.status = SOLVE_HINT_CLASH;
            p.other = p.src[t.dst] & ~SOLVE_HINT;
        }
        if (p.status != SOLVE_OK) return p;
        uint64_t x = t.dst;
        do {
            p.src[x] = SOLVE_HINT | (uint32_t)h;
            x = perm[x];
        } while (x != t.dst);
    }
    p.bad = 0;
    for (uint64_t j = 0; j < n; ++j)
        if (driven[j]) {
            p.src[2 * n + j] = (uint32_t)j;   // a driven row's c cell is its own computed value, driver or not
            ++p.driven_rows;
        }
    // levels: Kahn's pass over the rows (nodes 0 .. n - 1) and the hints (nodes n ..) together; users of a node in CSR form
    const uint64_t nodes = n + n_hints;
    std::vector<uint32_t> lv(nodes, 0), waits(nodes, 0), ucnt(nodes + 1, 0);
    auto deps = [&](uint64_t v, uint32_t (&d)[2]) {   // the nodes v reads
        int k = 0;
        const int cells = v < n ? 2 : 1;
        for (int i = 0; i < cells; ++i) {
            const uint32_t s = p.src[v < n ? (uint64_t)i * n + v : hints[v - n].src];
            if (!(s & SOLVE_FREE)) d[k++] = s;
            else if (solve_is_hint(s)) d[k++] = (uint32_t)n + (s & ~SOLVE_HINT);
        }
        return k;
    };
    auto live = [&](uint64_t v) { return v >= n || driven[v]; };
    uint32_t d[2];
    for (uint64_t v = 0; v < nodes; ++v)
        if (live(v)) {
            const int k = deps(v, d);
            waits[v] = (uint32_t)k;
            for (int i = 0; i < k; ++i) ++ucnt[d[i] + 1];
        }
    for (uint64_t v = 0; v < nodes; ++v) ucnt[v + 1] += ucnt[v];
    std::vector<uint32_t> users(ucnt[nodes]), fill(ucnt.begin(), ucnt.end() - 1);
    for (uint64_t v = 0; v < nodes; ++v)
        if (live(v)) {
            const int k = deps(v, d);
            for (int i = 0; i < k; ++i) users[fill[d[i]]++] = (uint32_t)v;
        }
    std::vector<uint32_t> queue;
    queue.reserve(p.driven_rows + n_hints);
    for (uint64_t v = 0; v < nodes; ++v)
        if (live(v) && !waits[v]) {
            lv[v] = 1;
            queue.push_back((uint32_t)v);
        }
    for (size_t h = 0; h < queue.size(); ++h) {
        const uint32_t r = queue[h];
        for (uint32_t u = ucnt[r]; u < ucnt[r + 1]; ++u) {
            const uint32_t j = users[u];
            if (lv[j] < lv[r] + 1) lv[j] = lv[r] + 1;
            if (--waits[j] == 0) queue.push_back(j);
        }
    }
    if (queue.size() != p.driven_rows + n_hints) {
        for (uint64_t v = 0; v < nodes; ++v)
            if (live(v) && waits[v]) {   // rows come first: a hint is named only when every row could be scheduled
                p.status = v < n ? SOLVE_CYCLE : SOLVE_HINT_CYCLE;
                p.bad = (uint32_t)(v < n ? v : v - n);
                break;
            }
        return p;
    }
    for (uint32_t r : queue) p.depth = lv[r] > p.depth ? lv[r] : p.depth;
    // the entries by level: rows ascending, then hints ascending
    p.level_off.assign((size_t)p.depth + 1, 0);
    for (uint32_t r : queue) ++p.level_off[lv[r]];
    for (uint32_t l = 0; l < p.depth; ++l) p.level_off[l + 1] += p.level_off[l];
    p.order.resize(queue.size());
    {
        std::vector<uint32_t> at(p.level_off.begin(), p.level_off.end());
        for (uint64_t v = 0; v < nodes; ++v)
            if (live(v)) p.order[at[lv[v] - 1]++] = v < n ? (uint32_t)v : SOLVE_HINT | (uint32_t)(v - n);
    }
    p.hint_level.assign(lv.begin() + (ptrdiff_t)n, lv.end());
    lv.resize(n);
    p.level = std::move(lv);
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

// a circuit without hints
inline SolvePlan solve_plan(const uint32_t* perm, const uint8_t* driven, uint64_t n, uint32_t narrow = SOLVE_NARROW,
                            uint32_t run_cut = SOLVE_RUN_CUT) {
    return solve_plan(perm, driven, n, nullptr, 0, narrow, run_cut);
}

}  // namespace ty
