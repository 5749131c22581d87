// Every decision of a batch of NTTs that does not need the device: vectors per launch sequence, the pass split, the two-pass
// 2^20 form, the 30-bit or 8 x 32 kernel, tile widths, grids and LDS bytes of every pass, the scratch size -- and the ordered
// list of tables the call looks up, each with its cache key and with its base and scale named, not computed.  ntt_plan()
// states them once; ntt_run_batch (ntt_host.hip) sizes the scratch from the plan, acquires the tables it lists and queues
// the passes it describes.  NTT policy is edited HERE.  No HIP include and no field arithmetic: the host compiles this header
// on its own (tests/cpp/ntt_plan_host.cpp prints the plan, tests/test_ntt_plan_host.py holds it against
// tests/golden/ntt_plans.json), like msm_plan.hpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "fr30.hpp"       // FR30_MAX_STAGES
#include "ntt_args.hpp"   // NTT_BATCH_MAX

namespace ty {

// full (one-multiplication) twiddle / coset tables are built up to this many entries (512 MB); above, two-level tables
constexpr uint32_t NTT_FULL_MAX_LOG = 24;
// default policy (TYPLONK_NTT_FR30 = 1): forward transforms take the 9 x 30-bit kernel up to this size, inverse ones always
// (their closing factor is free); set from the same-box A/B of the two kernels (ntt_plan, want30)
constexpr uint32_t NTT_FR30_FWD_MAX_LOG = 32;
// a multi-pass transform keeps one scratch vector per batch member: at most 2^25 elements = 1 GiB of scratch in all
constexpr uint32_t NTT_SCRATCH_MAX_LOG = 25;

// what a plan depends on besides the call's arguments: the context's switches (host.hpp, typlonk_ctx) and the device
struct NttFacts {
    int ntt_fr30 = 1, ntt_big = 1;
    bool prover_rounds_active = false, big_tiles_available = false;
};

// big = 4096-element tiles (1024 threads, 128 KiB of LDS): sub-transforms of 2^10 points with 4 adjacent columns, so a
// 2^20 transform needs two passes instead of three -- one load/store round and one inter-pass twiddle fewer.  Only 2^20:
// that is 256 tiles, one per CU; 2^17..2^19 would leave most of the chip idle (measured: 2^19 0.097 -> 0.132 ms) and
// 2^21.. do not fit (2^11-point sub-transforms x 4 columns = 256 KiB).
inline void ntt_split_log(uint32_t L, uint32_t ks[4], uint32_t* P, bool big) {
    uint32_t p = L <= 10 ? 1 : (L <= 16 ? 2 : (L <= 24 ? 3 : 4));
    if (big && L == 20) p = 2;
    *P = p;
    for (uint32_t i = 0; i < p; ++i) ks[i] = L / p + (i < L % p ? 1 : 0);
}

inline uint32_t ntt_ilog2(uint64_t x) {
    uint32_t r = 0;
    while ((1ull << (r + 1)) <= x) ++r;
    return r;
}

// ---- table requests ----
enum NttForm { NTT_F32 = 0, NTT_F30 = 1 };                            // the 8 x 32-bit kernel's table, the 9 x 30-bit kernel's
enum NttRole { NTT_SUB = 0, NTT_TW, NTT_PRE, NTT_POST, NTT_SCALE };   // which factor of a pass (NttPassArgs) the table holds
// out[j] = scale * base^j;  the same re-cut into nine 30-bit limbs on a 12-word stride;  the two halves of a two-level pair
// covering exponents < 2^log_len: lo[j] = base^j (j < 2^h), hi[j] = scale * base^(j 2^h) (j < 2^(log_len - h)),
// h = (log_len + 1) / 2;  the product table built on the device from such a pair, full[i] = pair(i-th exponent, stride S)
enum NttKind { NTT_POW = 0, NTT_POW30, NTT_PAIR_LO, NTT_PAIR_HI, NTT_FULL };
enum NttBase { NTT_B_ONE = 0, NTT_B_ROOT, NTT_B_ROOT_INV, NTT_B_SHIFT, NTT_B_SHIFT_INV };   // root: of the 2^base_log domain
enum NttScale { NTT_S_ONE = 0, NTT_S_NINV, NTT_S_C14, NTT_S_NINV_C14 };   // n^-1 of the transform; 2^14: the 30-bit kernel's R'/R

struct NttTableReq {
    NttForm form = NTT_F32;
    NttRole role = NTT_SUB;
    NttKind kind = NTT_POW;
    bool inverse = false;
    uint32_t pass = 0;
    uint64_t n = 0;                        // entries
    NttBase base = NTT_B_ONE;
    uint32_t base_log = 0, base_sqr = 0;   // the named base, squared base_sqr times
    NttScale scale = NTT_S_ONE;
    uint32_t lo = 0, hi = 0, h = 0;        // NTT_FULL: its pair (positions in the plan's list), the pair's split
    uint64_t S = 0;                        // NTT_FULL: stride of the exponent's row digit (0: the exponent is the index)
    uint32_t key_log = 0, key_k = 0;       // the key's numbers: transform / row / sub-transform size, and the pass size of a tw full table
    // an 8 x 32 full table that only a transform NOT run by the 30-bit kernel looks up
    bool unless30 = false;
};

// The cache keys, spelled here and nowhere else:
//   sub[30]:<dir>:<k>                          sub-transform twiddles of 2^k points
//   tw[30]:<dir>:<lrow>:lo|:hi|:full:<k>       inter-pass twiddles inside rows of 2^lrow, the full table per pass size 2^k
//   ninv[30]:<log_n>                           n^-1
//   cs:<dir>:<log_n>:<shift, 64 hex digits>[:30]:lo|:hi|:full      coset powers of a caller-chosen shift
// <dir> = f | i; "30" marks the 30-bit kernel's tables.  "cs:<dir>:<log_n>:<shift>" is the key's COSET GROUP, the unit of
// eviction: every key of the group is the group followed by ':...'.
inline std::string ntt_coset_group(bool inverse, uint32_t log_n, const std::string& shift_hex) {
    return std::string(inverse ? "cs:i:" : "cs:f:") + std::to_string(log_n) + ":" + shift_hex;
}
// the coset group of a key (empty: not a coset table)
inline std::string ntt_coset_group_of(const std::string& key) {
    if (key.compare(0, 3, "cs:") != 0) return std::string();
    return key.substr(0, key.find(':', 5) + 1 + 64);   // "cs:f:" <log_n> ':' and the shift's 64 digits
}
inline std::string ntt_key(const NttTableReq& r, const std::string& shift_hex) {
    const char* f30 = r.form == NTT_F30 ? "30" : "";
    const char* dir = r.inverse ? ":i:" : ":f:";
    const char* part = r.kind == NTT_PAIR_LO ? ":lo" : (r.kind == NTT_PAIR_HI ? ":hi" : (r.kind == NTT_FULL ? ":full" : ""));
    switch (r.role) {
        case NTT_SUB: return std::string("sub") + f30 + dir + std::to_string(r.key_log);
        case NTT_SCALE: return std::string("ninv") + f30 + ":" + std::to_string(r.key_log);
        case NTT_TW: {
            std::string k = std::string("tw") + f30 + dir + std::to_string(r.key_log) + part;
            return r.kind == NTT_FULL ? k + ":" + std::to_string(r.key_k) : k;
        }
        default: return ntt_coset_group(r.inverse, r.key_log, shift_hex) + (r.form == NTT_F30 ? ":30" : "") + part;
    }
}

// the two halves of a two-level pair over exponents < 2^log_len (r: everything but kind, n, base_sqr and the lo half's scale)
// (the split: the lo half holds 2^h entries, the hi half 2^(log_len - h))
constexpr uint32_t ntt_pair_lo_log(uint32_t log_len) { return (log_len + 1) / 2; }
inline void ntt_push_pair(std::vector<NttTableReq>& t, NttTableReq r, uint32_t log_len) {
    const uint32_t h = ntt_pair_lo_log(log_len);
    NttTableReq lo = r, hi = r;
    lo.kind = NTT_PAIR_LO;
    lo.n = 1ull << h;
    lo.scale = NTT_S_ONE;
    hi.kind = NTT_PAIR_HI;
    hi.n = 1ull << (log_len - h);
    hi.base_sqr = h;
    t.push_back(lo);
    t.push_back(hi);
}
// the full table of the pair pushed last: n entries, or nothing and false above the limit
inline bool ntt_push_full(std::vector<NttTableReq>& t, uint64_t S, uint64_t n, uint32_t key_k, bool unless30) {
    if (n > (1ull << NTT_FULL_MAX_LOG)) return false;
    NttTableReq f = t.back();
    f.kind = NTT_FULL;
    f.n = n;
    f.lo = (uint32_t)t.size() - 2;
    f.hi = (uint32_t)t.size() - 1;
    f.h = f.base_sqr;
    f.S = S;
    f.key_k = key_k;
    f.unless30 = unless30;
    t.push_back(f);
    return true;
}
// the domain's forward two-level twiddles w^j, w the generator of the 2^log_len domain: the pair the transform's inter-pass
// twiddles of that row length are, under the same keys
inline void ntt_push_domain_twiddles(std::vector<NttTableReq>& t, bool inverse, NttForm form, uint32_t pass, uint32_t log_len) {
    NttTableReq r;
    r.form = form;
    r.role = NTT_TW;
    r.inverse = inverse;
    r.pass = pass;
    r.base = inverse ? NTT_B_ROOT_INV : NTT_B_ROOT;
    r.base_log = r.key_log = log_len;
    r.scale = form == NTT_F30 ? NTT_S_C14 : NTT_S_ONE;
    ntt_push_pair(t, r, log_len);
}

// ---- the plan ----
// one pass: NttPassArgs with every scalar set (both kernel forms read the same ones; n_valid = ~0, the pointers null: the
// executor's), the launch, the LDS bytes of each form
struct NttPassPlan {
    NttPassArgs a{};
    uint32_t threads = 0;
    bool short_in = false;   // reads the caller's zero-padded source: n_valid is the caller's
    size_t lds[2] = {0, 0};  // [NTT_F32], [NTT_F30]
};
enum NttPlanStatus { NTT_PLAN_OK = 0, NTT_PLAN_DOMAIN, NTT_PLAN_EMPTY, NTT_PLAN_IDENTITY };
struct NttPlan {
    NttPlanStatus status = NTT_PLAN_OK;   // DOMAIN: log_n > 32 (Fr two-adicity); EMPTY: no vectors; IDENTITY: size 1
    size_t group = 0;        // vectors per launch sequence: the call runs vectors [g0, g0 + group) for g0 = 0, group, ...
    uint32_t P = 0, ks[4] = {0, 0, 0, 0};
    bool big = false;
    bool want30 = false;     // policy asks for the 30-bit kernel
    bool try30 = false;      // ... and every pass is within its bounds: its tables are looked up
    bool f30_eligible = false;   // ... and every full table it needs is within NTT_FULL_MAX_LOG: only an allocation failure can
                                 // still send the transform to the 8 x 32 kernel
    size_t scratch_bytes = 0;    // of a full group
    NttPassPlan pass[4];
    // In the order they are looked up (and, the first time, built).  The 30-bit list ends behind the pair whose full table
    // would pass the limit.  A 30-bit run also looks up the 8 x 32 sub: and tw: tables and reads none of them.
    std::vector<NttTableReq> tables;
};

inline NttPlan ntt_plan(uint32_t log_n, bool inverse, bool has_coset, size_t count, bool has_short_in, const NttFacts& facts) {
    NttPlan pl;
    if (log_n > 32) {
        pl.status = NTT_PLAN_DOMAIN;
        return pl;
    }
    if (count == 0) {
        pl.status = NTT_PLAN_EMPTY;
        return pl;
    }
    // vectors per launch: at most NTT_BATCH_MAX, and a multi-pass transform keeps one scratch vector per batch member
    // (<= 2^25 elements = 1 GiB of scratch in all: the 2^24-point coset extensions of a 2^22-row proof go two at a time)
    pl.group = std::min<size_t>(count, NTT_BATCH_MAX);
    while (pl.group > 1 && (((uint64_t)pl.group) << log_n) > (1ull << NTT_SCRATCH_MAX_LOG)) --pl.group;
    if (log_n == 0) {
        pl.status = NTT_PLAN_IDENTITY;   // size-1 transform is the identity (g^0 = 1, n^-1 = 1)
        return pl;
    }
    const uint64_t N = 1ull << log_n;
    // (not inside a prover round: there the 144 KiB workgroups crowd out the LDS of the MSM lanes' sort kernels running
    // beside them -- prove() 38.1 -> 38.3 ms in the same-box A/B)
    // (forward only: an inverse 2^20 transform is 4 % faster in three passes of the 30-bit kernel, 0.148 against 0.153 ms)
    // (round 4: the 30-bit kernel reads its sub-transform twiddles from global memory, so 4096 of its 36-byte elements fit
    // the LDS -- 144 KiB -- and it can take the two-pass form too)
    pl.big = log_n == 20 && facts.ntt_big != 0 && !facts.prover_rounds_active && facts.big_tiles_available;
    // log2 of the tile capacity: 4096-element tiles in the first pass of the two-pass 2^20 transform (strided: four columns
    // make 128-byte runs) and 2048 in the last (rows are contiguous, and two workgroups per CU overlap each other's
    // load / compute / store phases: 0.0775 -> 0.070 ms, profiles/r03_ntt_2_20_tiles.txt)
    const uint32_t cap_first = pl.big ? 12u : 10u;
    const uint32_t cap_last = pl.big ? 11u : 10u;
    ntt_split_log(log_n, pl.ks, &pl.P, pl.big);
    const uint32_t P = pl.P;
    if (P >= 2) pl.scratch_bytes = pl.group * (size_t)N * sizeof(Fr);

    // measured (HISTORY.md section 5): the 9 x 30-bit kernel is 9-12 % faster up to 2^19; at 2^20 the two-pass 4096-element
    // tiles of the 8 x 32 kernel win, and from 2^21 on the 36-B LDS elements cost a workgroup per CU (3 instead of 4)
    // and a forward transform pays one extra reducing multiplication per element: mode 1 (default) stops at 2^19
    // Round 3 (radix-4 groups in both kernels, profiles/r03_ntt_fr30_modes.txt): an INVERSE transform is 4-9 % faster on the
    // 30-bit kernel at every size (its n^-1 / coset factor closes the last pass for free), a forward one from 2^21 on is
    // not; at 2^20 a forward transform takes the two-pass big tiles when they are allowed, the 30-bit kernel otherwise
    // Round 4 (profiles/r04_ntt_fr30_global_twiddles.txt): with its twiddles in global memory the 30-bit kernel runs four
    // 1024-element workgroups per CU and takes the two-pass 2^20 form: 2^20 0.141 -> 0.129 ms in both directions, 2^21
    // forward 0.268 -> 0.252; mode 1 (default) = the 30-bit kernel for every inverse transform and for forward ones up to
    // 2^NTT_FR30_FWD_MAX_LOG points
    pl.want30 = facts.ntt_fr30 == 2 || (facts.ntt_fr30 == 1 && (inverse || log_n <= NTT_FR30_FWD_MAX_LOG));
    // The 9 x 30-bit kernel (fr30.hpp) multiplies with R' = 2^270: its tables carry an extra factor 2^14 and every one
    // of them must exist as a full table; if one cannot be built (size, memory) the transform runs on the 8 x 32 kernel.
    pl.try30 = pl.want30;
    for (uint32_t p = 0; p < P; ++p) pl.try30 = pl.try30 && pl.ks[p] <= FR30_MAX_STAGES;   // the bounds of fr30.hpp hold for k <= 10

    // ---- the passes: one walk of the shape ----
    uint64_t row_len = N;  // length of the rows the current pass works inside
    uint64_t rows = 1;
    for (uint32_t p = 0; p < P; ++p) {
        NttPassPlan& ps = pl.pass[p];
        NttPassArgs& a = ps.a;
        a.k = pl.ks[p];
        const uint64_t M = 1ull << a.k;
        a.last = (p + 1 == P) ? 1 : 0;
        a.S = row_len / M;
        a.row_len = row_len;
        if (!a.last) {
            a.tw_h = (ntt_ilog2(row_len) + 1) / 2;
            a.logT = std::min<uint32_t>(cap_first - a.k, ntt_ilog2(a.S));
        } else {
            const uint64_t N1 = 1ull << pl.ks[0];
            a.N1 = (P == 1) ? 1 : N1;
            a.Q = (P <= 2) ? 1 : rows / N1;
            a.N2 = (P >= 3) ? (1ull << pl.ks[1]) : 1;
            a.N3 = (P == 4) ? (1ull << pl.ks[2]) : 1;
            a.out_stride = N / M;
            a.logT = (P == 1) ? 0 : std::min<uint32_t>(cap_last - a.k, pl.ks[0]);
            if (has_coset && inverse) a.post_h = (log_n + 1) / 2;
        }
        if (p == 0 && has_coset && !inverse) a.pre_h = (log_n + 1) / 2;
        a.n_valid = ~0ull;
        ps.short_in = p == 0 && has_short_in;
        const uint64_t E = M << a.logT;
        a.blocks_per_vec = (uint32_t)(N / E);
        ps.threads = pl.big ? (unsigned)std::max<uint64_t>(E / 4, 64) : 256u;
        // LDS: the tile, and (8 x 32 kernel) the sub-transform's twiddles behind it
        ps.lds[NTT_F32] = (size_t)(E + std::max<uint64_t>(M / 2, 1)) * sizeof(Fr);
        ps.lds[NTT_F30] = (size_t)E * 36;
        rows *= M;
        row_len /= M;
    }

    // ---- the tables ----
    std::vector<NttTableReq>& t = pl.tables;
    t.reserve(24);
    // coset / scaling tables (the full tables of the 8 x 32 kernel are not built when the other kernel is asked for)
    NttTableReq cs;
    cs.inverse = inverse;
    cs.key_log = log_n;
    cs.role = inverse ? NTT_POST : NTT_PRE;
    cs.pass = inverse ? P - 1 : 0;
    cs.base = inverse ? NTT_B_SHIFT_INV : NTT_B_SHIFT;
    NttTableReq sc = cs;   // n^-1 of a plain inverse transform, one entry
    sc.role = NTT_SCALE;
    sc.base = NTT_B_ONE;
    sc.n = 1;
    if (has_coset) {
        cs.scale = inverse ? NTT_S_NINV : NTT_S_ONE;
        ntt_push_pair(t, cs, log_n);
        if (!pl.want30) ntt_push_full(t, 0, N, 0, false);
    } else if (inverse) {
        sc.scale = NTT_S_NINV;
        t.push_back(sc);
    }
    bool more30 = pl.try30;   // false behind the first full table past the limit
    if (more30) {
        cs.form = sc.form = NTT_F30;
        if (has_coset) {
            cs.scale = inverse ? NTT_S_NINV_C14 : NTT_S_C14;
            ntt_push_pair(t, cs, log_n);
            more30 = ntt_push_full(t, 0, N, 0, false);
        } else if (inverse) {
            sc.scale = NTT_S_NINV_C14;
            t.push_back(sc);
        }
    }
    for (int form = NTT_F30; form >= NTT_F32; --form) {
        for (uint32_t p = 0; p < P && (form == NTT_F32 || more30); ++p) {
            const NttPassArgs& a = pl.pass[p].a;
            NttTableReq sub;   // sub-transform twiddles w_M^e, e < M / 2
            sub.form = (NttForm)form;
            sub.kind = form == NTT_F30 ? NTT_POW30 : NTT_POW;
            sub.inverse = inverse;
            sub.pass = p;
            sub.n = std::max<uint64_t>((1ull << a.k) / 2, 1);
            sub.base = inverse ? NTT_B_ROOT_INV : NTT_B_ROOT;
            sub.base_log = sub.key_log = a.k;
            sub.scale = form == NTT_F30 ? NTT_S_C14 : NTT_S_ONE;
            t.push_back(sub);
            if (a.last) continue;
            ntt_push_domain_twiddles(t, inverse, (NttForm)form, p, ntt_ilog2(a.row_len));
            const bool full = ntt_push_full(t, a.S, a.row_len, a.k, form == NTT_F32);
            if (form == NTT_F30) more30 = full;
        }
        if (form == NTT_F30) pl.f30_eligible = more30;
    }
    return pl;
}

}  // namespace ty
