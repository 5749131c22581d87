// Every decision about a proof's device memory that does not need the device: the per-proof arena and its regions, which of
// the six q vectors plays which part in each proof shape, the wave size, the scratch layouts of the grand product and the
// openings, the pinned result slots, and -- prove_plan() -- the size of every workspace a prover call touches, each the
// maximum over the steps that use it.  A session (typlonk_prover_round1) and a batch call (prove_batch_impl) make the plan and
// size everything from it before anything is queued (prover_workspaces, prover.hip); the steps inside take their pointers from
// what was sized and never allocate.  The stand-alone entry points (typlonk_grand_product_dev, typlonk_open_dev,
// typlonk_quotient_dev) size for themselves from the same layouts.  Prover memory policy is edited HERE.  No HIP include: the
// host compiles this header on its own (tests/cpp/prove_plan_host.cpp prints the plan, tests/test_prove_plan_host.py holds it
// against tests/golden/prove_plans.json), like msm_plan.hpp and ntt_plan.hpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "ntt_plan.hpp"   // Fr; the two-level split of a domain's twiddles (ntt_pair_lo_log)

namespace ty {

// ---- the per-proof arena (typlonk_ctx::prover_mem), in units of n Fr ----
// ev: the three columns' evaluations (round 2 reads them), co: a, b, c, pi, z: PI and Z, t: the quotient (4n; t_lo t_mid t_hi
// are its first 3n coefficients), q: six witness / work vectors (roles below), r: the linearisation; and, in a wave only,
// ext: the 4n-point coset evaluations of a, b, c, Z, PI (a session keeps those in typlonk_ctx::quot_ext)
struct ProveRegion {
    uint32_t off, len;
};
constexpr ProveRegion PR_EV{0, 3}, PR_CO{3, 3}, PR_PI{6, 1}, PR_Z{7, 1}, PR_T{8, 4}, PR_Q{12, 6}, PR_R{18, 1}, PR_EXT{19, 20};
constexpr ProveRegion PROVE_REGIONS[] = {PR_EV, PR_CO, PR_PI, PR_Z, PR_T, PR_Q, PR_R, PR_EXT};
constexpr uint32_t PROVE_STRIDE = PR_R.off + PR_R.len, PROVE_STRIDE_WAVE = PR_EXT.off + PR_EXT.len;   // per proof, without and with ext
constexpr bool prove_regions_tile() {   // each region starts where the one before ends: no overlap, no hole
    uint32_t end = 0;
    for (const ProveRegion& r : PROVE_REGIONS) {
        if (r.off != end) return false;
        end += r.len;
    }
    return end == PROVE_STRIDE_WAVE;
}
static_assert(prove_regions_tile() && PROVE_STRIDE == 19 && PROVE_STRIDE_WAVE == 39, "the regions tile the arena; ext comes last");
struct ProveArena {
    Fr* mem = nullptr;
    uint64_t n = 0;
    uint32_t stride = PROVE_STRIDE;
    // vector i of region r of proof p (ext: i counts n, so its k-th 4n extension is i = 4 k)
    uint64_t index(uint32_t p, ProveRegion r, uint64_t i = 0) const { return ((uint64_t)p * stride + r.off + i) * n; }
    Fr* at(uint32_t p, ProveRegion r, uint64_t i = 0) const { return mem + index(p, r, i); }
    uint64_t stride_elems() const { return (uint64_t)stride * n; }   // what a wave's kernels add per proof
};

// ---- the roles of q, per proof shape (indices into PR_Q) ----
enum ProveQ : uint32_t {
    Q_WIT_A = 0, Q_WIT_B = 1, Q_WIT_C = 2, Q_WIT_Z = 3,   // the reference shape: the witnesses of a, b, c, Z at zeta,
    Q_WIT_ZW = 4,                                         // of Z at zeta w (every shape),
    Q_WIT_R = 5,                                          // of r at zeta
    Q_BATCHED_F = 5, Q_BATCHED_WIT = 0,   // batched openings (round4_batched): F = a + v b + v^2 c + v^3 Z + v^4 r, its witness
    Q_COMPACT_F = 1, Q_COMPACT_WIT = 0,   // the compact shape: F (+ v^5 sigma_1 + v^6 sigma_2) and its witness
};
// round3_openings (host.hpp) steps from Q_WIT_A through b and c, and a reference proof lists its six witnesses as q[0..5]
static_assert(Q_WIT_A == 0 && Q_WIT_B == 1 && Q_WIT_C == 2 && Q_WIT_Z == 3 && Q_WIT_ZW == 4 && Q_WIT_R == 5 && PR_Q.len == 6,
              "the reference shape's witnesses in q's order");
static_assert(Q_BATCHED_F != Q_BATCHED_WIT && Q_BATCHED_F != Q_WIT_ZW && Q_BATCHED_WIT != Q_WIT_ZW, "batched openings: F, W_F, W_zw apart");
static_assert(Q_COMPACT_F != Q_COMPACT_WIT && Q_COMPACT_F != Q_WIT_ZW && Q_COMPACT_WIT != Q_WIT_ZW, "compact: F, W_F, W_zw apart");

// ---- the pinned result slots (typlonk_ctx::eval_slots_host), PROVE_SLOTS per proof in flight ----
// Where round 3's evaluations land depends on the proof shape: the compact shape keeps its seven evaluations in the proof's
// order.  (sig0, sig1: CircuitEntry::coef's sigma_0 and sigma_1, which the compact shape's documents count from 1.)  r(zeta)
// and F(zeta) are written after the first `count` slots have been fetched.
struct Round3Slots {
    int wire;   // a, b, c at zeta: wire + i
    int z, sig0, sig1;
    int pi;     // PI(zeta), for the linearisation only
    int zw;     // Z at zeta w
    int count;  // slots to fetch
    int r, f;   // r(zeta) (the status of the proof) and F(zeta) (never read)
};
constexpr int PROVE_SLOTS = 16;
constexpr Round3Slots REF_SLOTS{0, 3, 4, 5, 6, 8, 9, 9, 10};
constexpr Round3Slots COMPACT_SLOTS{0, 3, 5, 6, 7, 4, 8, 9, 8};
constexpr bool prove_slots_ok(const Round3Slots& s) {
    const int v[8] = {s.wire, s.wire + 1, s.wire + 2, s.z, s.sig0, s.sig1, s.pi, s.zw};
    for (int i = 0; i < 8; ++i) {
        if (v[i] < 0 || v[i] >= s.count) return false;
        for (int j = 0; j < i; ++j)
            if (v[i] == v[j]) return false;
    }
    return s.r >= s.count && s.f >= s.count && s.r != s.f && s.r < PROVE_SLOTS && s.f < PROVE_SLOTS;
}
static_assert(prove_slots_ok(REF_SLOTS) && prove_slots_ok(COMPACT_SLOTS), "distinct slots, r and F behind the fetched ones");

// ---- a wave ----
constexpr uint32_t PB_MAX = 64;              // proofs per wave (the cap of typlonk.h)
constexpr uint64_t PB_ROWS = 1ull << 22;     // and at most this many rows of all proofs of a wave together
constexpr uint32_t PB_ITEMS = 8;             // round 3's openings / evaluations per proof and launch (launch_open_multi's 8 too)
inline uint32_t prove_wave_size(uint64_t count, uint32_t log_n) {
    return (uint32_t)std::min<uint64_t>({count, PB_MAX, std::max<uint64_t>(1, PB_ROWS >> log_n)});
}

// every table of a wave, staged in pinned memory (ctx->batch_host) and copied to ctx->batch_tab; each part is written once per
// wave and copied once, so no host write can overtake a copy still in flight
constexpr int LIN_TERMS = 10;   // the linearisation's polynomials (lin_polys, host.hpp)
struct PbGp {          // round 2
    Fr beta, gamma, kbeta[3];
};
struct PbQuot {        // round 3, quotient
    Fr alpha, alpha2, beta, gamma;
    uint32_t has_pi, pad[7];
};
struct PbLin {         // round 3, linearisation
    Fr scalar[LIN_TERMS];
    Fr constant;
};
struct PbFold {        // round 3 of the compact shape: r's terms, then F = a + v b + ... with vpow[j] = v^(j + 1)
    PbLin lin;
    Fr vpow[6];
};
struct PbItem {        // one opening (q != null) or evaluation at zpow[zi]
    const Fr* c;
    Fr* q;
    Fr* y;
    uint64_t zi;
};
struct PbTables {
    PbGp gp[PB_MAX];
    PbQuot quot[PB_MAX];
    PbLin lin[PB_MAX];
    PbItem item[PB_MAX * PB_ITEMS];
    PbItem ritem[2 * PB_MAX];   // r's opening; the compact shape: F's opening and r's evaluation
    PbFold fold[PB_MAX];
    Fr zpow[2 * PB_MAX][32];   // zeta_p^(2^k) at 2p, (zeta_p w)^(2^k) at 2p + 1
};

// ---- scratch layouts, in Fr ----
constexpr uint64_t PROVE_SCAN_BLOCK = 2048;   // elements per workgroup of the product scans and of the openings' suffix scans
constexpr uint64_t prove_nblk(uint64_t m) { return (m + PROVE_SCAN_BLOCK - 1) / PROVE_SCAN_BLOCK; }

// The grand product: numerators, denominators, their prefix / suffix products (n each), `runs` runs of nblk scan carries
// and, right behind them, the inverse of the denominators' total.
struct GpScratch {
    uint64_t num, den, npre, dsuf, carries, runs, inv, end;   // offsets from the layout's base; end: first element past it
};
// stand-alone and in a session, over ops_tmp: the two scans run one after the other and share one run of carries
inline GpScratch gp_scratch(uint64_t n) {
    const uint64_t nblk = prove_nblk(n);
    return GpScratch{0, n, 2 * n, 3 * n, 4 * n, 1, 4 * n + nblk, 4 * n + nblk + 8};
}
// in a wave, from a proof's arena base: the four vectors are t (not written before round 3), the carries the head of q; both
// scans of a proof run in one launch, so each has its run.  The wave's kernels (pb_pscan_*, pb_gp_*) take the two bases and
// index {0, 1, 2, 3} n and {0, 1} nblk, 2 nblk from them.
inline GpScratch gp_scratch_wave(uint64_t n) {
    const uint64_t t = PR_T.off * n, q = PR_Q.off * n, nblk = prove_nblk(n);
    return GpScratch{t, t + n, t + 2 * n, t + 3 * n, q, 2, q + 2 * nblk, q + 2 * nblk + 1};
}
constexpr bool gp_wave_carries_fit() {   // 2 nblk + 1 <= 6 n at every size a prover takes
    for (uint32_t lg = 0; lg <= 24; ++lg)
        if (2 * prove_nblk(1ull << lg) + 1 > ((uint64_t)PR_Q.len << lg)) return false;
    return PR_T.len == 4;
}
static_assert(gp_wave_carries_fit(), "a wave's grand product: four vectors in t, two carry runs and the inverse in q");

// the openings' carries: nblk per item of a launch, item k's run at k nblk (launch_open_multi, pb_launch_open)
inline uint64_t open_carries(uint64_t items, uint64_t m) { return items * prove_nblk(m); }
// a session's openings: launches of up to PB_ITEMS items (at least 2048 carries per item: the layout of n <= 2^22)
inline uint64_t session_open_carries(uint64_t n) { return PB_ITEMS * std::max<uint64_t>(PROVE_SCAN_BLOCK, prove_nblk(n)); }
// typlonk_open_dev: one item's carries (the same floor), then the result
struct OpenDevScratch {
    uint64_t carries, y, end;
};
inline OpenDevScratch open_dev_scratch(uint64_t m) {
    const uint64_t nb = std::max<uint64_t>(prove_nblk(m), PROVE_SCAN_BLOCK);
    return OpenDevScratch{0, nb, nb + 8};
}

// ---- the quotient's workspaces ----
// quot_ext: the 4n coset evaluations of a, b, c, Z, PI, and without a cached circuit of its nine vectors behind them
inline uint64_t quot_ext_vectors(bool cached) { return cached ? 5 : 14; }
// quot_tab: a scaled copy of the upper level of the 4n domain's two-level twiddles (domain_twiddles' hi table)
constexpr uint64_t quot_tab_entries(uint32_t log_n) { return 1ull << (log_n + 2 - ntt_pair_lo_log(log_n + 2)); }

// ---- the plan ----
enum ProveMode { PROVE_SESSION = 0, PROVE_WAVE = 1 };
struct ProvePlan {
    uint32_t log_n = 0, G = 1;   // G: proofs in flight
    uint64_t n = 0;
    uint32_t stride = PROVE_STRIDE;
    // what each step asks of ops_tmp, in Fr: the grand product (a wave's lives in the arena), the largest opening launch
    uint64_t need_gp = 0, need_open = 0;
    // bytes of each device workspace (0: the call does not touch it), and the pinned slots in Fr
    size_t prover_mem = 0, ops_tmp = 0, quot_ext = 0, quot_tab = 0, batch_tab = 0;
    size_t slots = 0;
};
// proofs: of the call (a session has one in flight whatever it says); cached: the circuit's coset evaluations are in the
// circuit cache -- always so for a prover, the stand-alone quotient without a circuit id brings its own
inline ProvePlan prove_plan(uint32_t log_n, uint64_t proofs, ProveMode mode, bool cached) {
    ProvePlan pl;
    pl.log_n = log_n;
    const uint64_t n = pl.n = 1ull << log_n;
    const bool wave = mode == PROVE_WAVE;
    pl.G = wave ? prove_wave_size(proofs, log_n) : 1;
    pl.stride = wave ? PROVE_STRIDE_WAVE : PROVE_STRIDE;
    pl.prover_mem = (size_t)pl.G * pl.stride * n * sizeof(Fr);
    pl.need_gp = wave ? 0 : gp_scratch(n).end;
    // a wave: round 3's items of every proof in one launch; r's (F's and r's) openings, 2G at most, fit the same runs
    pl.need_open = wave ? open_carries((uint64_t)pl.G * PB_ITEMS, n) : session_open_carries(n);
    pl.ops_tmp = (size_t)std::max(pl.need_gp, pl.need_open) * sizeof(Fr);
    pl.quot_ext = wave ? 0 : (size_t)quot_ext_vectors(cached) * 4 * n * sizeof(Fr);
    pl.quot_tab = (size_t)quot_tab_entries(log_n) * sizeof(Fr);
    pl.batch_tab = wave ? sizeof(PbTables) : 0;
    pl.slots = (size_t)pl.G * PROVE_SLOTS;
    return pl;
}

}  // namespace ty
