// libtyplonk_hip.so -- a powers-of-tau step (include/typlonk.h): typlonk_srs_check, typlonk_srs_check_challenge,
// typlonk_srs_contribute -- and typlonk_srs_g1_ntt, the Lagrange form of an SRS (at the end).  Host side only; the kernels
// (srs_membership_kernel, fr_powers_kernel, srs_contribute_kernel) are in srs_gen.hip, beside the generator they share the
// fixed base with, and the transform's (srs_g1_ntt_stage_kernel, srs_g1_ntt_batch_stage_kernel, srs_g1_scale_kernel) in g1_fft.hip.
//
// The check: g1[i+1] = [s] g1[i] for every i is  e(g1[i], [s]G2) = e(g1[i+1], G2)  for every i; weighted with rho^i and
// summed on the G1 side -- both pairings are linear there -- the len - 1 equations become ONE product
//   e(sum rho^i g1[i], [s]G2) * e(-sum rho^i g1[i+1], G2) = 1,
// two MSMs over the entry itself and one host pairing product.  The prefix sums of the same weights localise a failure.
#include "host.hpp"
#include "host_checks.hpp"
#include "compact_transcript.hpp"

using namespace ty;
using namespace tyh;

namespace {

namespace P = typlonk::pairing;

// rho of the ratio test, as a Montgomery residue
Fr check_challenge(const uint8_t seed[32], uint64_t len, const uint64_t g2s_xy[24]) {
    static const char tag[] = "typlonk/srs/check/v1";
    std::vector<uint8_t> b(tag, tag + sizeof(tag) - 1);
    b.insert(b.end(), seed, seed + 32);
    compact_put_u64(b, len);
    for (int i = 0; i < 24; ++i) compact_put_u64(b, g2s_xy[i]);
    uint8_t h[64];
    blake2b_512(b.data(), b.size(), h);
    return fr_from_digest(h);
}

// the entry a call works on, or the refusal: unknown ids and shards
int whole_srs(typlonk_ctx* ctx, uint32_t srs_id, const SrsEntry** out) {
    auto it = ctx->srs.find(srs_id);
    if (it == ctx->srs.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown srs id");
    if (it->second.total_len)
        return fail(ctx, TYPLONK_ERR_INVALID_ARG, "this call needs a whole SRS, not a shard (with or without a communicator)");
    *out = &it->second;
    return TYPLONK_OK;
}

// the prefix tests of one call: the weights on the device, the folds counted
struct RatioTest {
    typlonk_ctx* ctx;
    uint32_t srs_id;
    const Fr *pw, *pw_shift;
    P::G2Affine g2s;
    uint32_t folds = 0;

    // *pass: e(A_k, [s]G2) * e(-B_k, G2) = 1, for 1 <= k <= len - 1
    int prefix(uint64_t k, bool* pass) {
        const void* ptrs[2] = {pw, pw_shift};
        const size_t ms[2] = {(size_t)k, (size_t)k + 1};
        uint64_t xy[2][12];
        uint8_t inf[2];
        const int rc = msm_batch(ctx, srs_id, ptrs, ms, 2, &xy[0][0], inf);
        if (rc) return rc;
        P::G1Aff ps[2];
        for (int i = 0; i < 2; ++i) {
            memcpy(ps[i].x.v, xy[i], 48);
            memcpy(ps[i].y.v, xy[i] + 6, 48);
            ps[i].infinity = inf[i] != 0;
        }
        if (!ps[1].infinity) ps[1].y = P::qneg(ps[1].y);
        const P::G2Affine qs[2] = {g2s, P::g2_generator()};
        *pass = P::pairing_product_is_one(ps, qs, 2);
        ++folds;
        return TYPLONK_OK;
    }
};

}  // namespace

int typlonk_srs_check_challenge(const uint8_t seed[32], uint64_t len, const uint64_t g2s_xy[24], uint64_t rho[4]) {
    if (!seed || !g2s_xy || !rho) return TYPLONK_ERR_INVALID_ARG;
    const Fr r = check_challenge(seed, len, g2s_xy);
    memcpy(rho, r.v, 32);
    return TYPLONK_OK;
}

int typlonk_srs_check(typlonk_ctx* ctx, uint32_t srs_id, const uint64_t g2s_xy[24], const uint8_t seed[32],
                      typlonk_srs_report* report) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    if (!g2s_xy || !seed || !report) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    const SrsEntry* e = nullptr;
    int rc = whole_srs(ctx, srs_id, &e);
    if (rc) return rc;
    P::G2Affine g2s;
    if (!g2_from_limbs(g2s_xy, &g2s)) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "g2s is not a point of the twist");
    const uint64_t len = e->len;
    if (!len) return fail(ctx, TYPLONK_ERR_LENGTH, "an empty SRS has nothing to check");
    HIPCHK(hipSetDevice(ctx->device));
    typlonk_srs_report rep;
    memset(&rep, 0, sizeof(rep));

    // ---- membership and point 0: one launch ----
    DevGuard guard;
    unsigned long long* d_out = nullptr;
    HIPCHK(hipMalloc((void**)&d_out, 3 * sizeof(unsigned long long)));
    guard.add(d_out);
    unsigned long long h_out[3] = {~0ull, 0, 0};
    HIPCHK(hipMemcpyAsync(d_out, h_out, sizeof(h_out), hipMemcpyHostToDevice, ctx->stream));
    launch_srs_membership(e->d_points, len, d_out, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_out, d_out, sizeof(h_out), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (h_out[1]) {
        rep.verdict = TYPLONK_SRS_BAD_POINT;
        rep.point_class = (uint32_t)(h_out[0] & 0xff);
        rep.index = h_out[0] >> 8;
        rep.bad_points = h_out[1];
        *report = rep;
        return TYPLONK_OK;
    }
    if (h_out[2]) {
        rep.verdict = TYPLONK_SRS_BAD_P0;
        *report = rep;
        return TYPLONK_OK;
    }
    if (len == 1) {   // no link to test
        *report = rep;
        return TYPLONK_OK;
    }

    // ---- the ratio: the weights, the whole-SRS fold, and a bisection when it fails ----
    Fr* d_pw = nullptr;   // pw, then pw_shift
    HIPCHK(hipMalloc((void**)&d_pw, 2 * len * sizeof(Fr)));
    guard.add(d_pw);
    launch_fr_powers(check_challenge(seed, len, g2s_xy), len, d_pw, d_pw + len, ctx->stream);
    HIPCHK(hipGetLastError());
    ProfilingOff prof_off(ctx);   // the MSMs of a fold are not a call of their own
    RatioTest t{ctx, srs_id, d_pw, d_pw + len, g2s};
    // every return below leaves the lanes drained (msm_batch waits for its MSMs), so the guard may free the weights
    bool pass = false;
    if ((rc = t.prefix(len - 1, &pass))) return rc;
    if (!pass) {
        // prefix 0 holds (empty sums) and prefix hi fails: the least failing prefix lies in (lo, hi]
        uint64_t lo = 0, hi = len - 1;
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if ((rc = t.prefix(mid, &pass))) return rc;
            if (pass) lo = mid;
            else hi = mid;
        }
        rep.verdict = TYPLONK_SRS_BAD_RATIO;
        rep.index = hi - 1;
    }
    rep.folds = t.folds;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *report = rep;
    return TYPLONK_OK;
}

int typlonk_srs_contribute(typlonk_ctx* ctx, uint32_t srs_id, const uint64_t t[4], const uint64_t g2s_in[24],
                           uint32_t* new_srs_id, uint64_t g2s_out[24]) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    if (!t || !g2s_in || !new_srs_id || !g2s_out) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    const SrsEntry* src = nullptr;
    int rc = whole_srs(ctx, srs_id, &src);
    if (rc) return rc;
    if (!fr_canonical(t)) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "t is not a canonical residue");
    if (!(t[0] | t[1] | t[2] | t[3])) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "t = 0 contributes nothing: every power but the first would be the identity");
    P::G2Affine g2s;
    if (!g2_from_limbs(g2s_in, &g2s)) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "g2s is not a point of the twist");
    Fr tm;
    memcpy(tm.v, t, 32);
    const P::G2Affine q = P::g2_mul(g2s, tm);
    if (q.infinity) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "[t] g2s is the identity: g2s is not of order r");
    HIPCHK(hipSetDevice(ctx->device));
    SrsEntry e;
    e.len = src->len;
    DevGuard guard;
    HIPCHK(hipMalloc((void**)&e.d_points, std::max<size_t>(e.len, 1) * PT_WORDS * 4));
    guard.add(e.d_points);
    launch_srs_contribute(tm, (uint64_t)e.len, src->d_points, e.d_points, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    guard.dismiss();
    const uint32_t id = ctx->next_srs++;
    ctx->srs[id] = e;
    *new_srs_id = id;
    memcpy(g2s_out, q.x.a.v, 48);
    memcpy(g2s_out + 6, q.x.b.v, 48);
    memcpy(g2s_out + 12, q.y.a.v, 48);
    memcpy(g2s_out + 18, q.y.b.v, 48);
    return TYPLONK_OK;
}

// One launch per stage (g1_fft.hip); typlonk_srs_g1_ntt below, one block, and the transforms of the openings (open_chunks.hip).
// A single block goes to srs_g1_ntt_stage_kernel, which measures faster there, several to the batched kernel.
int tyh::g1_ntt_stages(typlonk_ctx* ctx, uint32_t l, uint64_t blocks, const uint32_t* src, uint64_t src_stride, uint32_t* dst,
                       uint64_t dst_stride, bool inverse) {
    for (uint32_t stage = 1; stage <= l; ++stage) {
        const Fr root = inverse ? fr_domain_root_inv(stage) : fr_domain_root(stage);
        if (blocks == 1) launch_srs_g1_ntt_stage(root, l, stage, src, dst, ctx->stream);
        else launch_srs_g1_ntt_batch_stage(root, l, stage, blocks, src, src_stride, dst, dst_stride, ctx->stream);
        HIPCHK(hipGetLastError());
    }
    return TYPLONK_OK;
}

// The Lagrange form of a monomial SRS and back: an NTT over the first 2^log_n points of the entry, in the group.  Stage by
// stage on the new entry's own records (g1_ntt_stages at one block; log_n <= 25: the stage kernels' indices within a block are
// 32-bit, g1_fft.hip); the inverse direction's 1/n is a pass of its own behind the last stage (srs_g1_scale_kernel).
int typlonk_srs_g1_ntt(typlonk_ctx* ctx, uint32_t srs_id, uint32_t log_n, uint32_t direction, uint32_t* new_srs_id) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    if (!new_srs_id) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    const SrsEntry* src = nullptr;
    int rc = whole_srs(ctx, srs_id, &src);
    if (rc) return rc;
    if (direction != TYPLONK_SRS_TO_LAGRANGE && direction != TYPLONK_SRS_FROM_LAGRANGE)
        return fail(ctx, TYPLONK_ERR_INVALID_ARG, "direction is neither TYPLONK_SRS_TO_LAGRANGE nor TYPLONK_SRS_FROM_LAGRANGE");
    if (log_n > 25) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "log_n > 25: an SRS holds at most 2^25 points");
    const size_t n = (size_t)1 << log_n;
    if (n > src->len) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "the entry holds fewer than 2^log_n points");
    HIPCHK(hipSetDevice(ctx->device));
    SrsEntry e;
    e.len = n;
    DevGuard guard;
    HIPCHK(hipMalloc((void**)&e.d_points, n * PT_WORDS * 4));
    guard.add(e.d_points);
    const bool inverse = direction == TYPLONK_SRS_TO_LAGRANGE;
    if (log_n == 0) HIPCHK(hipMemcpyAsync(e.d_points, src->d_points, PT_WORDS * 4, hipMemcpyDeviceToDevice, ctx->stream));
    if (log_n && (rc = g1_ntt_stages(ctx, log_n, 1, src->d_points, n, e.d_points, n, inverse))) return rc;
    if (inverse && log_n) {
        launch_srs_g1_scale(fr_inv_pow2(log_n), (uint64_t)n, e.d_points, ctx->stream);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    guard.dismiss();
    const uint32_t id = ctx->next_srs++;
    ctx->srs[id] = e;
    *new_srs_id = id;
    return TYPLONK_OK;
}
