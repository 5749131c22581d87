// The class structure of typlonk_permutation_from_pairs (perm_pairs.hip): a union-find over parent[3n] in which every thread
// joins one pair of cells, and the pointer jumping that flattens it.  Shared by the kernels and by the host
// (tests/cpp/perm_pairs_host.cpp runs the same bodies on 1 and on 16 threads), like sigma_cell.hpp.
//
// Invariant: parent[x] <= x, with equality exactly for a root.  So no cycle can form, a root is the lowest cell of its tree,
// and once every pair is joined the root of a class is its lowest cell: the label the canonical permutation is defined by.
//
// Every access to parent[] in a phase that also hooks is a relaxed atomic of agent scope (the host: relaxed __atomic
// builtins): a plain load may be served from a stale line of another XCD's L2 for as long as the line stays resident.  No
// loop waits for another thread: a failed compare-and-swap goes on from the value it returned, which is strictly lower than
// the root it tried, and every loop carries a bound (2 * 3n covers any walk: a walk only ever descends).
#pragma once
#include "ff.hpp"

namespace ty {

TY_HD uint32_t pp_load(const uint32_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return __atomic_load_n(p, __ATOMIC_RELAXED);
#endif
}
TY_HD void pp_store(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    __atomic_store_n(p, v, __ATOMIC_RELAXED);
#endif
}
// the value found at p: `expected` exactly when `desired` was written
TY_HD uint32_t pp_cas(uint32_t* p, uint32_t expected, uint32_t desired) {
#if defined(__HIP_DEVICE_COMPILE__)
    __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    __atomic_compare_exchange_n(p, &expected, desired, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
#endif
    return expected;
}

// The root above x, with path halving: every second cell of the walk is pointed at its grandparent.  Such a store only ever
// hits a cell already seen with a parent below it (never a root, so it cannot undo or race a hook) and writes an ancestor,
// so the invariant holds whatever the interleaving.  *over is set when `bound` steps did not reach a root.
TY_HD uint32_t pp_find(uint32_t* parent, uint32_t x, uint32_t bound, bool* over) {
    for (uint32_t it = 0; it < bound; ++it) {
        const uint32_t p = pp_load(parent + x);
        if (p == x) return x;
        const uint32_t g = pp_load(parent + p);
        if (g == p) return p;
        pp_store(parent + x, g);
        x = g;
    }
    *over = true;
    return x;
}

// Join the classes of a and b: the larger root is hooked under the smaller one.  false when a bound was reached.
TY_HD bool pp_union(uint32_t* parent, uint32_t a, uint32_t b, uint32_t bound) {
    if (a == b) return true;
    bool over = false;
    uint32_t ra = pp_find(parent, a, bound, &over), rb = pp_find(parent, b, bound, &over);
    for (uint32_t it = 0; ra != rb && !over; ++it) {
        if (it >= bound) return false;
        const uint32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        const uint32_t seen = pp_cas(parent + hi, hi, lo);
        if (seen == hi) break;
        // hi has been hooked by someone else: seen < hi is an ancestor of it, and the walk goes on from there (lo stays an
        // ancestor of the other cell whether or not it is still a root)
        ra = pp_find(parent, seen, bound, &over);
        rb = lo;
    }
    return !over;
}

// One round of pointer jumping for cell x, after the hooks: up to `hops` steps towards the root, then parent[x] is pointed at
// the cell reached.  A round divides every depth by hops + 1 at least (other cells' concurrent jumps only shorten the walk),
// so ceil(log(3n) / log(hops + 1)) rounds leave parent[x] = root(x) everywhere.
TY_HD void pp_jump(uint32_t* parent, uint32_t x, uint32_t hops) {
    const uint32_t first = pp_load(parent + x);
    uint32_t p = first;
    for (uint32_t h = 0; h < hops; ++h) {
        const uint32_t g = pp_load(parent + p);
        if (g == p) break;
        p = g;
    }
    if (p != first) pp_store(parent + x, p);
}
constexpr uint32_t PP_JUMP_HOPS = 7;
// rounds of pp_jump that flatten any forest over 3 * 2^log_n cells: depth < 2^(log_n + 2), three bits per round
TY_HD uint32_t pp_jump_rounds(uint32_t log_n) { return (log_n + 2 + 2) / 3; }

}  // namespace ty
