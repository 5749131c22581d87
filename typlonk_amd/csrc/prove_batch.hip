// libtyplonk_hip.so -- typlonk_prove_batch: many witnesses of one circuit per call, batched across proofs.
//
// The proofs run in waves of G (include/typlonk.h).  A wave goes round by round like typlonk_prove (prover.hip), but every
// stage is one launch sequence for the whole wave instead of one per proof: the transforms through ntt_run_batch, the grand
// product, the openings, the quotient's pointwise kernel and the linearisation through the kernels below (the proof index in
// blockIdx.y, per-proof scalars in a small device table), and each round's commitments in one MsmQueue.  The host waits
// three times per wave -- after round 1's and round 2's commitments (the transcripts need them) and for round 3's
// evaluations -- plus the final read, never once per proof.  Every proof keeps its own Fiat-Shamir transcript, and every
// field operation is exact, so proof k is bit for bit what typlonk_prove returns for witness k.
//
// typlonk_prove_batch_compact runs the same waves in the compact shape (typlonk_prove_compact): rounds 1 and 2 are shared
// (wave_rounds12, with the shape's transcript), round 3 goes in the compact transcript's order -- the 3G quotient commitments
// before any zeta is drawn (a fourth host wait per wave), then the evaluations, then r and F of every proof from one fused
// kernel (pb_fold_kernel) and the 2G opening commitments.
#include "fr_inv.hpp"
#include "host.hpp"
#include "proof_script.hpp"
#include "scan_ops.hpp"

#include <cstddef>

using namespace ty;
using namespace tyh;

namespace {

// (the wave size, the item count per proof and every table of a wave: prove_plan.hpp)
constexpr uint32_t PB_QGROUP = 4;            // proofs one thread of the quotient kernel evaluates per point
constexpr uint32_t PB_FGROUP = 4;            // proofs one thread of the compact shape's fold kernel combines per coefficient
static_assert(PSCAN_PER_BLOCK == PROVE_SCAN_BLOCK, "the plan sizes the scans' carries");

// ---- round 2: the grand product of every proof of the wave (plonk_ops.hip's kernels with a proof index) ---------------------
struct PbGpArgs {
    const Fr* ev;        // proof p's three columns: ev + p * stride + i * n
    const Fr* sigma;     // the circuit's sigma evaluations (3 n), shared
    const Fr* w_lo;
    const Fr* w_hi;
    Fr* tmp;             // num, den, nprefix, dsuffix of proof p: tmp + p * stride + {0, 1, 2, 3} n
    Fr* blk;             // carries of the two scans (2 nblk) and the inverse of proof p: blk + p * stride
    Fr* z;
    const PbGp* gp;
    uint64_t n, stride;
    uint32_t w_h, nblk;
};

__global__ __launch_bounds__(256) void pb_gp_terms_kernel(PbGpArgs a) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= a.n) return;
    const uint32_t p = blockIdx.y;
    const PbGp& g = a.gp[p];
    const Fr x = fe_mul(p_ld(a.w_lo + (j & ((1ull << a.w_h) - 1))), p_ld(a.w_hi + (j >> a.w_h)));
    const Fr* ev = a.ev + p * a.stride;
    Fr num = Fr::one(), den = Fr::one();
#pragma unroll
    for (int i = 0; i < 3; ++i) gp_term(ev + i * a.n + j, a.sigma + i * a.n + j, x, g.beta, g.gamma, g.kbeta[i], num, den);
    Fr* t = a.tmp + p * a.stride;
    p_st(t + j, num);
    p_st(t + a.n + j, den);
}
// scan s = 2 p + d of the wave: d = 0 the exclusive prefix products of proof p's numerators, d = 1 the suffix products of
// its denominators
__global__ __launch_bounds__(256) void pb_pscan_block_kernel(PbGpArgs a) {
    const uint32_t p = blockIdx.y >> 1, d = blockIdx.y & 1;
    pscan_block(a.tmp + p * a.stride + d * a.n, a.n, (int)d, a.blk + p * a.stride + d * a.nblk, blockIdx.x);
}
__global__ __launch_bounds__(256) void pb_pscan_top_kernel(PbGpArgs a) {
    const uint32_t p = blockIdx.x >> 1, d = blockIdx.x & 1;
    pscan_top(a.blk + p * a.stride + d * a.nblk, a.nblk);
}
__global__ __launch_bounds__(256) void pb_pscan_finish_kernel(PbGpArgs a) {
    const uint32_t p = blockIdx.y >> 1, d = blockIdx.y & 1;
    Fr* t = a.tmp + p * a.stride;
    pscan_finish(t + d * a.n, a.n, (int)d, a.blk + p * a.stride + d * a.nblk, t + (2 + d) * a.n, blockIdx.x);
}
// the one inversion of every proof: S_0 = dsuffix[0]
__global__ __launch_bounds__(64) void pb_fr_inv_kernel(PbGpArgs a) {
    const uint32_t p = blockIdx.x;
    const Fr x = fr_inv_divsteps(p_ld(a.tmp + p * a.stride + 3 * a.n));
    if (threadIdx.x == 0) p_st(a.blk + p * a.stride + 2 * a.nblk, x);
}
__global__ __launch_bounds__(256) void pb_gp_finish_kernel(PbGpArgs a) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= a.n) return;
    const uint32_t p = blockIdx.y;
    const Fr* t = a.tmp + p * a.stride;
    p_st(a.z + p * a.stride + j,
         gp_finish(p_ld(t + 2 * a.n + j), p_ld(t + 3 * a.n + j), p_ld(a.blk + p * a.stride + 2 * a.nblk)));
}

// ---- openings / evaluations of many polynomials of m coefficients, each at its own point (launch_open_multi for a wave) -----
struct PbOpenArgs {
    const PbItem* items;
    const Fr* zpow;      // 32 powers z^(2^k) per point
    Fr* blocks;          // nblk carries per item
    uint64_t m;
    uint32_t nblk;
};
__device__ __forceinline__ OpenItem open_item(const PbOpenArgs& a, uint32_t k) {
    const PbItem it = a.items[k];
    return OpenItem{it.c, it.q, it.y, a.zpow + it.zi * 32, a.blocks + (uint64_t)k * a.nblk};
}
__global__ __launch_bounds__(256) void pb_open_block_kernel(PbOpenArgs a) {
    __shared__ Fr lds[256];
    open_block_stage(open_item(a, blockIdx.y), a.m, lds);
}
__global__ __launch_bounds__(256) void pb_open_top_kernel(PbOpenArgs a) {
    __shared__ Fr lds[256];
    const OpenItem it = open_item(a, blockIdx.x);
    open_top_stage(it, a.nblk, it.q != nullptr, lds);
}
__global__ __launch_bounds__(256) void pb_open_finish_kernel(PbOpenArgs a) {
    __shared__ Fr lds[256];
    const OpenItem it = open_item(a, blockIdx.y);
    if (!it.q) return;  // whole workgroup
    open_finish_stage(it, a.m, lds);
}
void pb_launch_open(const PbItem* items, uint32_t count, const Fr* zpow, uint64_t m, Fr* blocks, hipStream_t s) {
    PbOpenArgs a{items, zpow, blocks, m, (uint32_t)((m + 2047) / 2048)};
    hipLaunchKernelGGL(pb_open_block_kernel, dim3(a.nblk, count), dim3(256), 0, s, a);
    hipLaunchKernelGGL(pb_open_top_kernel, dim3(count), dim3(256), 0, s, a);
    hipLaunchKernelGGL(pb_open_finish_kernel, dim3(a.nblk, count), dim3(256), 0, s, a);
}

// ---- round 3: the quotient's pointwise kernel for a wave (quotient_point, scan_ops.hpp) -----------------------------------
// One thread owns one point of the 4n coset and PB_QGROUP proofs: the circuit's nine coset constants and x_i are loaded once
// and serve every proof of the group (each proof alone re-read them at all 4n points).
struct PbQuotArgs {
    const Fr* ext;       // proof p's coset evaluations of a, b, c, Z, PI: ext + p * stride + k * n4
    const Fr* cext;      // the circuit's: q_l q_r q_o q_m q_c sigma_0..2 L0 (9 x n4)
    const Fr* w_lo;      // x_i = g w_{4n}^i = w_lo[i & mask] * gx_hi[i >> w_h]
    const Fr* gx_hi;
    Fr* t;               // proof p's pointwise quotient: t + p * stride
    const PbQuot* pq;
    uint64_t n4, stride;
    uint32_t w_h, count, k0_is_one;
    Fr k[3];
    Fr zh_inv[4];
};
__global__ __launch_bounds__(256) void pb_quotient_kernel(PbQuotArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n4) return;
    const uint64_t iw = (i + 4) & (a.n4 - 1);
    Fr sel[5], sig[3];
#pragma unroll
    for (int k = 0; k < 5; ++k) sel[k] = p_ld(a.cext + k * a.n4 + i);
#pragma unroll
    for (int k = 0; k < 3; ++k) sig[k] = p_ld(a.cext + (5 + k) * a.n4 + i);
    const Fr l0 = p_ld(a.cext + 8 * a.n4 + i);
    const Fr x = fe_mul(p_ld(a.w_lo + (i & ((1ull << a.w_h) - 1))), p_ld(a.gx_hi + (i >> a.w_h)));
    const Fr zhi = a.zh_inv[i & 3];
    const uint32_t p0 = blockIdx.y * PB_QGROUP, p1 = min(a.count, p0 + PB_QGROUP);
    for (uint32_t p = p0; p < p1; ++p) {
        const PbQuot& q = a.pq[p];
        const Fr* e = a.ext + p * a.stride;
        const Fr wa = p_ld(e + i), wb = p_ld(e + a.n4 + i), wc = p_ld(e + 2 * a.n4 + i);
        const Fr z = p_ld(e + 3 * a.n4 + i), zw = p_ld(e + 3 * a.n4 + iw);
        const Fr t = quotient_point(wa, wb, wc, z, zw, q.has_pi ? e + 4 * a.n4 + i : nullptr, sel, sig, l0, fe_mul(q.beta, x), a.k,
                                    a.k0_is_one, q.beta, q.gamma, q.alpha, q.alpha2, zhi);
        p_st(a.t + p * a.stride + i, t);
    }
}

// ---- round 3: r = sum_k scalar_k poly_k + constant for every proof (lincomb_kernel with per-proof terms) -------------------
struct PbLinArgs {
    const Fr* coef;      // the circuit's coefficient copies (8 n)
    const Fr* z;         // proof p's Z: z + p * stride, its t: t + p * stride, its r: r + p * stride
    const Fr* t;
    Fr* r;
    const PbLin* lin;
    uint64_t n, stride;
};
__global__ __launch_bounds__(256) void pb_lincomb_kernel(PbLinArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t p = blockIdx.y;
    const PbLin& l = a.lin[p];
    const Fr* t = a.t + p * a.stride;
    const Fr* polys[LIN_TERMS];
    lin_polys(a.coef, a.z + p * a.stride, t, a.n, polys);
    Fr acc = (i == 0) ? l.constant : Fr::zero();
#pragma unroll
    for (int k = 0; k < LIN_TERMS; ++k) acc = fe_add(acc, fe_mul(l.scalar[k], p_ld(polys[k] + i)));
    p_st(a.r + p * a.stride + i, acc);
}

// ---- round 3 of the compact shape: r and F = a + v b + v^2 c + v^3 Z + v^4 r + v^5 sigma_1 + v^6 sigma_2 in one pass ----------
// One thread owns coefficient i and PB_FGROUP proofs: the circuit's eight coefficients at i are loaded once and serve every proof
// of the group.  A single proof runs lincomb_kernel twice (17 n Fr read, r written and read back); here a proof reads its own
// seven vectors and writes r and F.  r's ten terms are lin_polys' (host.hpp), in its order: coefficients 0..4 and 7 of the
// circuit, Z, t_lo t_mid t_hi.  Every value is a canonical residue of an exact field expression, so the order of the sums
// does not show in the result.
struct PbFoldArgs {
    const Fr* coef;      // the circuit's coefficient copies (8 n): q_l q_r q_o q_m q_c sigma_0 sigma_1 sigma_2
    const Fr* co;        // proof p's a, b, c: co + p * stride + k * n; its Z, t, r, F at z / t / r / f + p * stride
    const Fr* z;
    const Fr* t;
    Fr* r;
    Fr* f;
    const PbFold* fold;
    uint64_t n, stride;
    uint32_t count;
};
__global__ __launch_bounds__(256) void pb_fold_kernel(PbFoldArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    Fr cc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) cc[k] = p_ld(a.coef + k * a.n + i);
    const uint32_t p0 = blockIdx.y * PB_FGROUP, p1 = min(a.count, p0 + PB_FGROUP);
    for (uint32_t p = p0; p < p1; ++p) {
        const PbFold& s = a.fold[p];
        const uint64_t at = p * a.stride + i;
        Fr r = (i == 0) ? s.lin.constant : Fr::zero();
#pragma unroll
        for (int k = 0; k < 5; ++k) r = fe_add(r, fe_mul(s.lin.scalar[k], cc[k]));
        const Fr z = p_ld(a.z + at);
        r = fe_add(r, fe_mul(s.lin.scalar[5], z));
        r = fe_add(r, fe_mul(s.lin.scalar[6], cc[7]));
#pragma unroll
        for (int k = 0; k < 3; ++k) r = fe_add(r, fe_mul(s.lin.scalar[7 + k], p_ld(a.t + at + k * a.n)));
        p_st(a.r + at, r);
        Fr f = p_ld(a.co + at);
        f = fe_add(f, fe_mul(s.vpow[0], p_ld(a.co + at + a.n)));
        f = fe_add(f, fe_mul(s.vpow[1], p_ld(a.co + at + 2 * a.n)));
        f = fe_add(f, fe_mul(s.vpow[2], z));
        f = fe_add(f, fe_mul(s.vpow[3], r));
        f = fe_add(f, fe_mul(s.vpow[4], cc[5]));
        f = fe_add(f, fe_mul(s.vpow[5], cc[6]));
        p_st(a.f + at, f);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
struct Wave {
    typlonk_ctx* ctx;
    const SrsEntry* srs;
    const CircuitEntry* ce;
    uint32_t log_n;
    uint64_t n;
    ProveArena mem;   // proof p's arena: regions, stride and the roles of q in prove_plan.hpp
    PbTables* host;   // pinned staging
    PbTables* dev;
    Fr* slots;        // PROVE_SLOTS per proof
    Fr* carries;      // of the openings: nblk per item of a launch (ops_tmp, sized for PB_ITEMS items per proof)
    Fr k[3];
    bool has_pi[PB_MAX];   // of the running wave (wave_rounds12)
    const typlonk_vk* vk = nullptr;   // the compact shape's statement (without [s]G2)
    Fr* at(uint32_t p, ProveRegion r, uint64_t i = 0) const { return mem.at(p, r, i); }
    Fr* slot(uint32_t p, int i = 0) const { return slots + (uint64_t)p * PROVE_SLOTS + i; }
};

// copy one part of the staged tables to the device, stream-ordered
int upload(const Wave& w, const void* host_part, size_t bytes) {
    const size_t off = (const char*)host_part - (const char*)w.host;
    return hip_rc(w.ctx, hipMemcpyAsync((char*)w.dev + off, host_part, bytes, hipMemcpyHostToDevice, w.ctx->stream));
}

// Rounds 1 and 2 of a wave in either shape: [a] [b] [c] and [Z] of every proof, beta / gamma / alpha in out[], the coset
// extensions of a, b, c, Z (and PI) queued, and the quotient's per-proof table (w.host->quot) filled.  Script: the shape's
// Fiat-Shamir script (proof_script.hpp), one per proof.
template <class Script>
int wave_rounds12(Wave& w, const ColumnsOf& in, size_t first, uint32_t G, typename Script::Proof* out, std::vector<Script>& tr) {
    typlonk_ctx* ctx = w.ctx;
    hipStream_t s = ctx->stream;
    const uint64_t n = w.n;
    const uint32_t log_n = w.log_n, log4 = log_n + 2;
    const uint64_t stride = w.mem.stride_elems();
    const uint64_t* g_limbs = coset_g();
    int rc = TYPLONK_OK;
    bool* has_pi = w.has_pi;
    for (uint32_t p = 0; p < G; ++p) has_pi[p] = in.pi_rows(first + p, n) != 0;
    auto lasterr = [&]() { return hip_rc(ctx, hipGetLastError()); };

    // ---- round 1: columns into the arena, a, b, c (and PI) by one batched inverse transform, 3G commitments ----
    std::vector<Fr*> co, ext;
    std::vector<const Fr*> ext_src;
    for (uint32_t p = 0; p < G && !rc; ++p) {
        for (int i = 0; i < 3 && !rc; ++i) {
            rc = hip_rc(ctx, column_to_device(w.at(p, PR_EV, i), in.column(first + p, i, n), n, s));
            if (!rc) rc = hip_rc(ctx, hipMemcpyAsync(w.at(p, PR_CO, i), w.at(p, PR_EV, i), n * sizeof(Fr), hipMemcpyDeviceToDevice, s));
            co.push_back(w.at(p, PR_CO, i));
        }
        if (!rc && has_pi[p]) {   // (the compact shape reads pi_len rows; the rest are zero)
            rc = hip_rc(ctx, column_to_device(w.at(p, PR_PI), in.pi(first + p, n), n, s));
            co.push_back(w.at(p, PR_PI));
        }
    }
    if (!rc) rc = ntt_run_batch(ctx, co.data(), co.size(), log_n, 1, nullptr, /*sync=*/false);   // proof.rs:50, 105-106
    if (rc) return rc;
    // the commitments wait for this mark only: the coset extensions queued behind it run beside them
    if (!ctx->batch_fence) HIPCHK(hipEventCreateWithFlags(&ctx->batch_fence, hipEventDisableTiming));
    HIPCHK(hipEventRecord(ctx->batch_fence, s));
    for (uint32_t p = 0; p < G; ++p)
        for (int k = 0; k < 5; ++k) {
            if (k == 3 || (k == 4 && !has_pi[p])) continue;   // (Z is extended in round 2)
            ext.push_back(w.at(p, PR_EXT, 4 * k));
            ext_src.push_back(k < 3 ? w.at(p, PR_CO, k) : w.at(p, PR_PI));
        }
    rc = ntt_run_batch(ctx, ext.data(), ext.size(), log4, 0, g_limbs, /*sync=*/false, ext_src.data(), n);
    {
        MsmQueue q(ctx, w.srs, /*first_lane=*/1);
        q.fence = ctx->batch_fence;
        for (uint32_t p = 0; p < G && !rc; ++p)
            for (int i = 0; i < 3 && !rc; ++i)
                rc = q.submit(w.at(p, PR_CO, i), n, out[first + p].commit_xy[i], out[first + p].commit_inf + i);   // :107-110
        const int r = q.wait_all();
        if (!rc) rc = r;
    }
    if (rc) return rc;
    for (uint32_t p = 0; p < G; ++p) {
        auto& o = out[first + p];
        tr[p].after_round1(o);
        PbGp& g = w.host->gp[p];
        memcpy(g.beta.v, o.beta, 32);
        memcpy(g.gamma.v, o.gamma, 32);
        for (int i = 0; i < 3; ++i) g.kbeta[i] = fe_mul(w.k[i], g.beta);
    }

    // ---- round 2: the grand products (:119-120), one batched inverse transform (:127-128), G commitments of [Z] (:129) ----
    if ((rc = upload(w, w.host->gp, G * sizeof(PbGp)))) return rc;
    {
        PbGpArgs a{};
        a.ev = w.at(0, PR_EV);
        a.sigma = w.ce->sig_ev;
        // the scratch is laid over t and the head of q, not written before round 3 (gp_scratch_wave; the kernels index the
        // four vectors from a.tmp and the two carry runs and the inverse from a.blk)
        const GpScratch L = gp_scratch_wave(n);
        a.tmp = w.mem.mem + L.num;
        a.blk = w.mem.mem + L.carries;
        a.z = w.at(0, PR_Z);
        a.gp = w.dev->gp;
        a.n = n;
        a.stride = stride;
        a.nblk = (uint32_t)prove_nblk(n);
        if ((rc = domain_twiddles(ctx, std::max<uint32_t>(log_n, 1), &a.w_lo, &a.w_hi, &a.w_h))) return rc;
        const unsigned gx = (unsigned)((n + 255) / 256);
        hipLaunchKernelGGL(pb_gp_terms_kernel, dim3(gx, G), dim3(256), 0, s, a);
        hipLaunchKernelGGL(pb_pscan_block_kernel, dim3(a.nblk, 2 * G), dim3(256), 0, s, a);
        hipLaunchKernelGGL(pb_pscan_top_kernel, dim3(2 * G), dim3(256), 0, s, a);
        hipLaunchKernelGGL(pb_pscan_finish_kernel, dim3(a.nblk, 2 * G), dim3(256), 0, s, a);
        hipLaunchKernelGGL(pb_fr_inv_kernel, dim3(G), dim3(64), 0, s, a);
        hipLaunchKernelGGL(pb_gp_finish_kernel, dim3(gx, G), dim3(256), 0, s, a);
        if ((rc = lasterr())) return rc;
    }
    {
        std::vector<Fr*> zs(G), zext(G);
        std::vector<const Fr*> zsrc(G);
        for (uint32_t p = 0; p < G; ++p) {
            zs[p] = w.at(p, PR_Z);
            zsrc[p] = zs[p];
            zext[p] = w.at(p, PR_EXT, 4 * 3);
        }
        if ((rc = ntt_run_batch(ctx, zs.data(), G, log_n, 1, nullptr, /*sync=*/false))) return rc;
        HIPCHK(hipEventRecord(ctx->batch_fence, s));
        rc = ntt_run_batch(ctx, zext.data(), G, log4, 0, g_limbs, /*sync=*/false, zsrc.data(), n);   // beside the commitments
        MsmQueue q(ctx, w.srs, /*first_lane=*/1);
        q.fence = ctx->batch_fence;
        for (uint32_t p = 0; p < G && !rc; ++p) rc = q.submit(w.at(p, PR_Z), n, out[first + p].z_xy, &out[first + p].z_inf);
        const int r = q.wait_all();
        if (!rc) rc = r;
    }
    if (rc) return rc;
    for (uint32_t p = 0; p < G; ++p) {
        auto& o = out[first + p];
        tr[p].after_round2(o);
        PbQuot& q = w.host->quot[p];
        memcpy(q.alpha.v, o.alpha, 32);
        q.alpha2 = fe_sqr(q.alpha);
        q.beta = w.host->gp[p].beta;
        q.gamma = w.host->gp[p].gamma;
        q.has_pi = has_pi[p];
    }
    return TYPLONK_OK;
}

// round 3's openings and evaluations of every proof of the wave (round3_openings) into the staged item table; returns how many
uint32_t stage_round3_items(Wave& w, uint32_t G, const Round3Slots& slots, bool with_quotients) {
    uint32_t nitems = 0;
    for (uint32_t p = 0; p < G; ++p) {
        const Round3Polys polys{w.at(p, PR_CO), w.at(p, PR_Z), w.has_pi[p] ? w.at(p, PR_PI) : nullptr, w.at(p, PR_Q), w.ce->coef, w.n};
        round3_openings(slots, with_quotients, polys, [&](const Fr* c, Fr* quot, int slot, uint32_t point) {
            w.host->item[nitems++] = PbItem{c, quot, w.slot(p, slot), 2ull * p + point};
        });
    }
    return nitems;
}

// zeta_p^(2^k) and (zeta_p w)^(2^k) of proof p into the staged table
void stage_zpow(Wave& w, uint32_t p, const Fr& zeta) {
    Fr* zp0 = w.host->zpow[2 * p];
    Fr* zp1 = w.host->zpow[2 * p + 1];
    zp0[0] = zeta;
    zp1[0] = fe_mul(zeta, fr_domain_root(w.log_n));
    for (int k = 1; k < 32; ++k) {
        zp0[k] = fe_sqr(zp0[k - 1]);
        zp1[k] = fe_sqr(zp1[k - 1]);
    }
}

// The quotient of every proof of the wave (proof.rs:139-145): the staged table w.host->quot to the device, the pointwise kernel
// and one batched inverse 4n transform; t_lo, t_mid, t_hi of proof p are then the first 3n coefficients of its t.
int wave_quotient(Wave& w, uint32_t G) {
    typlonk_ctx* ctx = w.ctx;
    hipStream_t s = ctx->stream;
    const uint64_t n = w.n, n4 = 4 * n;
    const uint32_t log_n = w.log_n, log4 = log_n + 2;
    int rc;
    if ((rc = upload(w, w.host->quot, G * sizeof(PbQuot)))) return rc;
    PbQuotArgs a{};
    QuotientDomain d;
    if ((rc = quotient_domain(ctx, log_n, &d))) return rc;
    const uint64_t* g_limbs = d.g_limbs;
    a.ext = w.at(0, PR_EXT);
    a.cext = w.ce->ext;
    a.t = w.at(0, PR_T);
    a.pq = w.dev->quot;
    a.n4 = n4;
    a.stride = w.mem.stride_elems();
    a.count = G;
    a.w_lo = d.w_lo;
    a.w_h = d.w_h;
    if (d.n_hi * sizeof(Fr) > ctx->quot_tab.cap) return fail(ctx, TYPLONK_ERR_INTERNAL, "quot_tab is smaller than the 4n domain's upper level");
    launch_fr_scale(d.w_hi, d.n_hi, d.g, (Fr*)ctx->quot_tab.p, s);   // (beta is per proof: the kernel multiplies)
    a.gx_hi = (const Fr*)ctx->quot_tab.p;
    for (int k = 0; k < 4; ++k) a.zh_inv[k] = d.zh_inv[k];
    for (int k = 0; k < 3; ++k) a.k[k] = w.k[k];
    a.k0_is_one = w.k[0] == Fr::one();
    hipLaunchKernelGGL(pb_quotient_kernel, dim3((unsigned)((n4 + 255) / 256), (G + PB_QGROUP - 1) / PB_QGROUP), dim3(256), 0, s, a);
    if ((rc = hip_rc(ctx, hipGetLastError()))) return rc;
    std::vector<Fr*> ts(G);
    for (uint32_t p = 0; p < G; ++p) ts[p] = w.at(p, PR_T);
    return ntt_run_batch(ctx, ts.data(), G, log4, 1, g_limbs, /*sync=*/false);
}

int run_wave(Wave& w, const ColumnsOf& in, size_t first, uint32_t G, typlonk_proof* out, int* status) {
    typlonk_ctx* ctx = w.ctx;
    hipStream_t s = ctx->stream;
    const uint64_t n = w.n, stride = w.mem.stride_elems();
    const uint32_t log_n = w.log_n;
    const bool* has_pi = w.has_pi;
    auto lasterr = [&]() { return hip_rc(ctx, hipGetLastError()); };
    std::vector<RefScript> tr(G);
    int rc = wave_rounds12(w, in, first, G, out, tr);
    if (rc) return rc;
    std::vector<Fr> zeta(G), alpha(G);
    for (uint32_t p = 0; p < G; ++p) {
        memcpy(alpha[p].v, out[first + p].alpha, 32);
        memcpy(zeta[p].v, out[first + p].zeta, 32);
        stage_zpow(w, p, zeta[p]);
    }

    // ---- round 3: openings (:147-163), quotient (:139-145), linearisation (:165-175), nine commitments per proof (:181) ----
    Fr* blocks = w.carries;
    const uint32_t nitems = stage_round3_items(w, G, REF_SLOTS, /*with_quotients=*/true);
    if ((rc = upload(w, w.host->item, nitems * sizeof(PbItem)))) return rc;
    if ((rc = upload(w, w.host->zpow, 2 * G * sizeof(w.host->zpow[0])))) return rc;
    pb_launch_open(w.dev->item, nitems, &w.dev->zpow[0][0], n, blocks, s);
    if ((rc = lasterr())) return rc;
    if ((rc = wave_quotient(w, G))) return rc;
    // what the linearisation needs of zeta alone, while the kernels run; then ONE wait for every evaluation of the wave
    std::vector<Fr> zn(G), zh(G), l0z(G);
    for (uint32_t p = 0; p < G; ++p) lin_zeta_terms(zeta[p], log_n, &zn[p], &zh[p], &l0z[p]);
    HIPCHK(hipStreamSynchronize(s));
    for (uint32_t p = 0; p < G; ++p) {
        const Fr* y = w.slot(p);
        constexpr Round3Slots S = REF_SLOTS;
        const Fr ev[5] = {y[S.wire], y[S.wire + 1], y[S.wire + 2], y[S.z], y[S.zw]};
        const Fr pi_z = has_pi[p] ? y[S.pi] : Fr::zero();
        PbLin& l = w.host->lin[p];
        lin_scalars(ev, y[S.sig0], y[S.sig1], pi_z, w.host->gp[p].beta, w.host->gp[p].gamma, w.k, alpha[p], zeta[p], zn[p], zh[p],
                    l0z[p], l.scalar, &l.constant);
        typlonk_proof_tail& t = out[first + p].tail;
        for (int i = 0; i < 5; ++i) memcpy(t.evals[i], ev[i].v, 32);
        w.host->ritem[p] = PbItem{w.at(p, PR_R), w.at(p, PR_Q, Q_WIT_R), w.slot(p, S.r), 2ull * p};
    }
    if ((rc = upload(w, w.host->lin, G * sizeof(PbLin)))) return rc;
    if ((rc = upload(w, w.host->ritem, G * sizeof(PbItem)))) return rc;
    {
        PbLinArgs a{w.ce->coef, w.at(0, PR_Z), w.at(0, PR_T), w.at(0, PR_R), w.dev->lin, n, stride};
        hipLaunchKernelGGL(pb_lincomb_kernel, dim3((unsigned)((n + 255) / 256), G), dim3(256), 0, s, a);
        if ((rc = lasterr())) return rc;
    }
    pb_launch_open(w.dev->ritem, G, &w.dev->zpow[0][0], n, blocks, s);   // r(zeta) and its witness (:175)
    if ((rc = lasterr())) return rc;
    {
        HIPCHK(hipEventRecord(ctx->batch_fence, s));
        MsmQueue q(ctx, w.srs, /*first_lane=*/0);
        q.fence = ctx->batch_fence;
        const size_t m[9] = {n - 1, n - 1, n - 1, n - 1, n - 1, n - 1, n, n, n > 3 ? n - 3 : 0};
        for (uint32_t p = 0; p < G && !rc; ++p) {
            typlonk_proof_tail& t = out[first + p].tail;
            // (the six witnesses in q's order, Q_WIT_A .. Q_WIT_R, as the proof lists them)
            const Fr* polys[9] = {w.at(p, PR_Q, 0), w.at(p, PR_Q, 1), w.at(p, PR_Q, 2), w.at(p, PR_Q, 3), w.at(p, PR_Q, 4),
                                  w.at(p, PR_Q, 5), w.at(p, PR_T), w.at(p, PR_T, 1), w.at(p, PR_T, 2)};
            for (int k = 0; k < 9 && !rc; ++k)
                rc = k < 6 ? q.submit(polys[k], m[k], t.w_xy[k], t.w_inf + k) : q.submit(polys[k], m[k], t.t_xy[k - 6], t.t_inf + k - 6);
        }
        const int r = q.wait_all();
        if (!rc) rc = r;
    }
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(s));
    for (uint32_t p = 0; p < G; ++p) {
        const Fr rz = *w.slot(p, REF_SLOTS.r);
        memcpy(out[first + p].tail.evals[5], rz.v, 32);
        // r(zeta) != 0: the witness does not satisfy the circuit (proof.rs:234-235), as typlonk_prove reports it
        status[first + p] = rz.is_zero() ? TYPLONK_OK : TYPLONK_ERR_UNSATISFIED;
    }
    return TYPLONK_OK;
}

// A wave in the compact shape (typlonk_prove_compact's order, prover.hip prover_round3_compact).  The host waits four times --
// round 1's, round 2's and the quotient's commitments, round 3's evaluations -- plus the final read.
int run_wave(Wave& w, const ColumnsOf& in, size_t first, uint32_t G, typlonk_proof_compact* out, int* status) {
    typlonk_ctx* ctx = w.ctx;
    hipStream_t s = ctx->stream;
    const uint64_t n = w.n, stride = w.mem.stride_elems();
    const uint32_t log_n = w.log_n;
    const bool* has_pi = w.has_pi;
    auto lasterr = [&]() { return hip_rc(ctx, hipGetLastError()); };
    int rc;
    // ---- the statements: d0 of every proof from the shared vk and its own public values; the device form brings the values
    // of the whole wave to the host behind ONE synchronisation ----
    std::vector<CompactScript> tr;
    tr.reserve(G);
    {
        std::vector<std::vector<uint64_t>> fetched(in.on_device() ? G : 0);
        bool any = false;
        for (uint32_t p = 0; p < G && in.on_device(); ++p) {
            const ColumnSrc pi = in.pi(first + p, n);
            if (!pi.rows) continue;
            fetched[p].resize(4 * pi.rows);
            HIPCHK(hipMemcpyAsync(fetched[p].data(), pi.dev, pi.rows * sizeof(Fr), hipMemcpyDeviceToHost, s));
            any = true;
        }
        if (any) HIPCHK(hipStreamSynchronize(s));
        for (uint32_t p = 0; p < G; ++p) {
            const uint64_t rows = in.pi_rows(first + p, n);
            const uint64_t* vals = !rows ? nullptr : in.on_device() ? fetched[p].data() : in.pi(first + p, n).host;
            uint8_t d0[64];
            compact_statement_digest(*w.vk, vals, rows, d0);
            tr.emplace_back(d0);
        }
    }
    if ((rc = wave_rounds12(w, in, first, G, out, tr))) return rc;

    // ---- round 3: the quotient as soon as every alpha is known, its 3G commitments behind one fence; zeta binds them ----
    if ((rc = wave_quotient(w, G))) return rc;
    {
        HIPCHK(hipEventRecord(ctx->batch_fence, s));
        MsmQueue q(ctx, w.srs, /*first_lane=*/0);
        q.fence = ctx->batch_fence;
        const size_t m[3] = {n, n, n > 3 ? n - 3 : 0};
        for (uint32_t p = 0; p < G && !rc; ++p)
            for (int k = 0; k < 3 && !rc; ++k)
                rc = q.submit(w.at(p, PR_T, k), m[k], out[first + p].t_xy[k], out[first + p].t_inf + k);
        const int r = q.wait_all();
        if (!rc) rc = r;
    }
    if (rc) return rc;
    std::vector<Fr> zeta(G);
    for (uint32_t p = 0; p < G; ++p) {
        zeta[p] = tr[p].after_quotient(out[first + p]);
        stage_zpow(w, p, zeta[p]);
    }
    // ---- a, b, c, Z, sigma_1, sigma_2 (and PI) at zeta_p, Z at zeta_p w with its quotient (COMPACT_SLOTS: the first seven slots
    // are the proof's evaluations in order); one wait for the whole wave ----
    Fr* blocks = w.carries;
    const uint32_t nitems = stage_round3_items(w, G, COMPACT_SLOTS, /*with_quotients=*/false);
    if ((rc = upload(w, w.host->item, nitems * sizeof(PbItem)))) return rc;
    if ((rc = upload(w, w.host->zpow, 2 * G * sizeof(w.host->zpow[0])))) return rc;
    pb_launch_open(w.dev->item, nitems, &w.dev->zpow[0][0], n, blocks, s);
    if ((rc = lasterr())) return rc;
    std::vector<Fr> zn(G), zh(G), l0z(G);
    for (uint32_t p = 0; p < G; ++p) lin_zeta_terms(zeta[p], log_n, &zn[p], &zh[p], &l0z[p]);   // while the kernels run
    HIPCHK(hipStreamSynchronize(s));
    for (uint32_t p = 0; p < G; ++p) {
        Fr* y = w.slot(p);
        typlonk_proof_compact& o = out[first + p];
        constexpr Round3Slots S = COMPACT_SLOTS;
        for (int i = 0; i < 7; ++i) memcpy(o.evals[i], y[i].v, 32);
        const Fr v = tr[p].after_evals(o);
        const Fr pi_z = has_pi[p] ? y[S.pi] : Fr::zero();
        Fr alpha;
        memcpy(alpha.v, o.alpha, 32);
        PbFold& f = w.host->fold[p];
        static_assert(S.wire == 0 && S.z == 3 && S.zw == 4, "lin_scalars reads a, b, c, Z, Z(zeta w) as ev[0..4]");
        lin_scalars(y, y[S.sig0], y[S.sig1], pi_z, w.host->gp[p].beta, w.host->gp[p].gamma, w.k, alpha, zeta[p], zn[p], zh[p],
                    l0z[p], f.lin.scalar, &f.lin.constant);
        f.vpow[0] = v;
        for (int j = 1; j < 6; ++j) f.vpow[j] = fe_mul(f.vpow[j - 1], v);
        // F opened at zeta with its witness (their places in q: ProveQ); r evaluated there for the status
        w.host->ritem[2 * p] = PbItem{w.at(p, PR_Q, Q_COMPACT_F), w.at(p, PR_Q, Q_COMPACT_WIT), y + S.f, 2ull * p};
        w.host->ritem[2 * p + 1] = PbItem{w.at(p, PR_R), nullptr, y + S.r, 2ull * p};
    }
    if ((rc = upload(w, w.host->fold, G * sizeof(PbFold)))) return rc;
    if ((rc = upload(w, w.host->ritem, 2 * G * sizeof(PbItem)))) return rc;
    {
        PbFoldArgs a{w.ce->coef, w.at(0, PR_CO), w.at(0, PR_Z), w.at(0, PR_T), w.at(0, PR_R), w.at(0, PR_Q, Q_COMPACT_F), w.dev->fold,
                     n, stride, G};
        hipLaunchKernelGGL(pb_fold_kernel, dim3((unsigned)((n + 255) / 256), (G + PB_FGROUP - 1) / PB_FGROUP), dim3(256), 0, s, a);
        if ((rc = lasterr())) return rc;
    }
    pb_launch_open(w.dev->ritem, 2 * G, &w.dev->zpow[0][0], n, blocks, s);
    if ((rc = lasterr())) return rc;
    // ---- W_zeta and W_zeta_w of every proof in one queue ----
    {
        HIPCHK(hipEventRecord(ctx->batch_fence, s));
        MsmQueue q(ctx, w.srs, /*first_lane=*/0);
        q.fence = ctx->batch_fence;
        for (uint32_t p = 0; p < G && !rc; ++p) {
            typlonk_proof_compact& o = out[first + p];
            rc = q.submit(w.at(p, PR_Q, Q_COMPACT_WIT), n - 1, o.w_xy[0], o.w_inf + 0);
            if (!rc) rc = q.submit(w.at(p, PR_Q, Q_WIT_ZW), n - 1, o.w_xy[1], o.w_inf + 1);
        }
        const int r = q.wait_all();
        if (!rc) rc = r;
    }
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(s));
    for (uint32_t p = 0; p < G; ++p)   // r(zeta) != 0: the witness does not satisfy the circuit, as typlonk_prove_compact reports it
        status[first + p] = w.slot(p, COMPACT_SLOTS.r)->is_zero() ? TYPLONK_OK : TYPLONK_ERR_UNSATISFIED;
    return TYPLONK_OK;
}

struct BusyGuard {
    typlonk_ctx* ctx;
    ~BusyGuard() {
        (void)hipStreamSynchronize(ctx->stream);
        ctx->prover_busy = false;
    }
};

template <class Proof>
int prove_batch_impl(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const ColumnsOf& in, const uint64_t cosets[3][4],
                     Proof* out, int* status) {
    const size_t count = in.count;
    const bool compact = in.rule == ColumnsOf::PI_FIRST;
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    if (count == 0) return TYPLONK_OK;
    if (!cosets || !out || !status || !in.given()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    auto ci = ctx->circuits.find(circuit_id);
    if (ci == ctx->circuits.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown circuit id");
    const uint32_t log_n = ci->second.log_n;
    if (compact && log_n > TYPLONK_MAX_PROVER_LOG_N) return fail(ctx, TYPLONK_ERR_DOMAIN, "prover supports up to 2^24 rows");
    const uint64_t n = 1ull << log_n;
    if (const int arc = admit_columns(ctx, in, n)) return arc;
    auto si = ctx->srs.find(srs_id);
    if (si == ctx->srs.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown srs id");
    if (si->second.total_len || comm_folds(ctx, srs_id))
        // sharding buys latency for ONE large proof (typlonk_prove, typlonk_prove_compact); a batch of small proofs belongs on
        // one GPU per proof, and from 2^22 rows on a wave holds a single proof anyway (4 at 2^20)
        return fail(ctx, TYPLONK_ERR_INVALID_ARG,
                    "batched proving needs a whole SRS on one GPU, not a shard (shard single large proofs with "
                    "typlonk_prove / typlonk_prove_compact; give each GPU its own batch)");
    if (si->second.len < n) return fail(ctx, TYPLONK_ERR_LENGTH, "SRS shorter than the circuit's n");
    if (const int arc = admit_rows(ctx, in, n)) return arc;
    if (ctx->prover_busy) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "a proof is already in flight on this context");
    HIPCHK(hipSetDevice(ctx->device));
    typlonk_vk vk;
    if (compact) {
        // the statement's shared part: the circuit's commitments (one batch of eight MSMs the first time per circuit and SRS,
        // then cached) and P0 -- once per call, not per proof or wave
        memset((void*)out, 0, count * sizeof(Proof));
        const int vrc = circuit_vk_fill(ctx, srs_id, circuit_id, cosets, &vk);
        if (vrc) return vrc;
    }
    // the wave's workspaces: the per-proof arenas, the openings' carries, the quotient's table, the result slots, the tables
    const ProvePlan plan = prove_plan(log_n, count, PROVE_WAVE, /*cached=*/true);
    const uint32_t G = plan.G;
    int rc = prover_workspaces(ctx, plan);
    if (rc) return rc;
    ctx->prover_busy = true;
    BusyGuard busy{ctx};
    ProfilingOff prof_off(ctx);
    ProverRound in_round(ctx);
    Wave w;
    w.ctx = ctx;
    w.srs = &si->second;
    w.ce = &ci->second;
    w.log_n = log_n;
    w.n = n;
    w.mem = ProveArena{(Fr*)ctx->prover_mem.p, n, plan.stride};
    w.carries = (Fr*)ctx->ops_tmp.p;
    w.host = (PbTables*)ctx->batch_host;
    w.dev = (PbTables*)ctx->batch_tab.p;
    w.slots = ctx->eval_slots_host;
    w.vk = compact ? &vk : nullptr;
    for (int i = 0; i < 3; ++i) memcpy(w.k[i].v, cosets[i], 32);
    for (size_t first = 0; first < count && !rc; first += G) {
        const uint32_t g = (uint32_t)std::min<size_t>(G, count - first);
        rc = run_wave(w, in, first, g, out, status);
    }
    return rc;
}

}  // namespace

int typlonk_prove_batch(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const typlonk_buf* const* wire_evals,
                        const typlonk_buf* const* pi_evals, size_t count, const uint64_t cosets[3][4], typlonk_proof* out,
                        int* status) {
    return prove_batch_impl(ctx, srs_id, circuit_id, ColumnsOf(wire_evals, count, ColumnsOf::PI_FULL, pi_evals), cosets, out, status);
}

int typlonk_prove_batch_host(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const uint64_t* const* wire_evals,
                             const uint64_t* const* pi_evals, size_t count, const uint64_t cosets[3][4], typlonk_proof* out,
                             int* status) {
    return prove_batch_impl(ctx, srs_id, circuit_id, ColumnsOf(wire_evals, count, ColumnsOf::PI_FULL, pi_evals), cosets, out, status);
}

int typlonk_prove_batch_compact(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const typlonk_buf* const* wire_evals,
                                const typlonk_buf* const* pi, const size_t* pi_len, size_t count, const uint64_t cosets[3][4],
                                typlonk_proof_compact* out, int* status) {
    return prove_batch_impl(ctx, srs_id, circuit_id, ColumnsOf(wire_evals, count, ColumnsOf::PI_FIRST, pi, pi_len), cosets, out,
                            status);
}

int typlonk_prove_batch_compact_host(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const uint64_t* const* wire_evals,
                                     size_t rows, const uint64_t* const* pi, const size_t* pi_len, size_t count,
                                     const uint64_t cosets[3][4], typlonk_proof_compact* out, int* status) {
    return prove_batch_impl(ctx, srs_id, circuit_id, ColumnsOf(wire_evals, count, ColumnsOf::PI_FIRST, pi, pi_len).with_rows(rows),
                            cosets, out, status);
}
