// libtyplonk_hip.so -- typlonk_verify_chunks and typlonk_verify_chunks_challenge (include/typlonk.h): the KZG multi-proofs of
// typlonk_open_chunks_*, a batch of cells per call.  Host side only; the kernels (chunks_membership_kernel, chunks_weights_kernel,
// chunks_fold_kernel, chunks_fold_sum_kernel) are in verify_chunks.hip and the fold's launch shape in verify_chunks_plan.hpp.
//
// Cell i = (c_i, k_i, E_i, pi_i) is valid iff  e(C_(c_i) - [I_i(s)]G + [a_(k_i)] pi_i, G2) = e(pi_i, [s^l]G2).  Weighted with
// rho_i = rho^i and summed on the G1 side the live cells of [lo, hi) become ONE product
//     e(sum rho_i pi_i, [s^l]G2) * e(-(sum_c w_c C_c + sum rho_i a_(k_i) pi_i - [A(s)]G), G2) = 1:
// two MSMs over a temporary entry (the N proofs, then the M commitments), one l-term MSM of A over the caller's SRS, one G1
// addition and two Miller loops on the host.  A failing fold is bisected over the live cells as FoldBisect::decide (verify.hip)
// bisects proofs.
#include "host.hpp"
#include "host_checks.hpp"
#include "compact_transcript.hpp"
#include "verify_chunks_plan.hpp"

#include <chrono>

using namespace ty;
using namespace tyh;

namespace {

namespace P = typlonk::pairing;

constexpr uint32_t CHUNKS_MAX_LOG_N = 24;
constexpr uint64_t CHUNKS_MAX_ELEMS = 1ull << 25;   // N * l evaluations, and N + M records (the SRS length cap)

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// rho of the fold, as a Montgomery residue
Fr chunks_challenge(const uint8_t seed[32], uint32_t log_n, uint32_t log_l, uint64_t N, uint64_t M, const uint64_t g2sl_xy[24]) {
    static const char tag[] = "typlonk/chunks/verify/v1";
    std::vector<uint8_t> b(tag, tag + sizeof(tag) - 1);
    b.insert(b.end(), seed, seed + 32);
    compact_put_u64(b, log_n);
    compact_put_u64(b, log_l);
    compact_put_u64(b, N);
    compact_put_u64(b, M);
    for (int i = 0; i < 24; ++i) compact_put_u64(b, g2sl_xy[i]);
    uint8_t h[64];
    blake2b_512(b.data(), b.size(), h);
    return fr_from_digest(h);
}

// the temporary entry leaves the context on every path out of the call
struct TempSrs {
    typlonk_ctx* ctx;
    uint32_t id = 0;
    ~TempSrs() {
        if (id) (void)typlonk_srs_free(ctx, id);
    }
};

// One call's folds: everything on the device, the folds counted and timed
struct ChunksFold {
    typlonk_ctx* ctx;
    uint32_t srs_id, tmp_id, log_l;
    uint64_t N, M;
    const std::vector<uint8_t>& live;
    uint64_t strip;   // of the whole call's plan: a sub-range planned with it never has more workgroups than the call
    Fr l_inv;
    const Fr *pw, *coset_a;
    const uint32_t *order, *first;
    const uint8_t* d_live;
    const Fr *evals, *tw;
    Fr *s_pi, *s_all, *scale, *twist, *partial, *coef;
    P::G2Affine g2sl;
    bool timed;
    uint32_t folds = 0;
    double t_kernels = 0, t_msm = 0, t_pair = 0;

    // *pass: the product over the live cells of [lo, hi) is one; hi > lo
    int fold(uint64_t lo, uint64_t hi, bool* pass) {
        auto t0 = std::chrono::steady_clock::now();
        const uint32_t l = 1u << log_l;
        launch_chunks_weights(pw, coset_a, order, first, d_live, N, M, lo, hi, l_inv, s_pi, s_all, scale, ctx->stream);
        HIPCHK(hipGetLastError());
        // `partial` holds the whole call's blocks: ceil((hi - lo) / strip) <= ceil(N / strip).  (A sub-range's OWN plan may have
        // more: its strip can be shorter.)
        const VerifyChunksPlan pl = verify_chunks_plan(hi - lo, log_l, strip);
        launch_chunks_fold(evals, scale, twist, tw, lo, hi - lo, log_l, pl, partial, ctx->stream);
        HIPCHK(hipGetLastError());
        launch_chunks_fold_sum(partial, pl.blocks, l, coef, ctx->stream);
        HIPCHK(hipGetLastError());
        if (timed) {
            HIPCHK(hipStreamSynchronize(ctx->stream));
            t_kernels += ms_since(t0);
            t0 = std::chrono::steady_clock::now();
        }
        // [0] = sum rho_i pi_i, [1] = sum_c w_c C_c + sum rho_i a_k pi_i, [2] = [A(s)] G
        uint64_t xy[3][12];
        uint8_t inf[3];
        const void* ptrs[2] = {s_pi, s_all};
        const size_t ms[2] = {(size_t)N, (size_t)(N + M)};
        int rc = msm_batch(ctx, tmp_id, ptrs, ms, 2, &xy[0][0], inf);
        if (!rc) rc = msm_run(ctx, srs_id, coef, l, xy[2], &inf[2]);
        if (rc) return rc;
        t_msm += ms_since(t0);
        t0 = std::chrono::steady_clock::now();
        // the second pair's G1 point: -([1] - [2]) = [2] - [1]
        h64::Fq y1;
        memcpy(y1.v, xy[1] + 6, 48);
        y1 = h64::sub(h64::Fq{}, y1);
        memcpy(xy[1] + 6, y1.v, 48);
        uint64_t sum_xy[12];
        uint8_t sum_inf = 0;
        if (typlonk_g1_sum_host(&xy[1][0], &inf[1], 2, sum_xy, &sum_inf)) return fail(ctx, TYPLONK_ERR_INTERNAL, "g1 sum failed");
        P::G1Aff ps[2];
        memcpy(ps[0].x.v, xy[0], 48);
        memcpy(ps[0].y.v, xy[0] + 6, 48);
        ps[0].infinity = inf[0] != 0;
        memcpy(ps[1].x.v, sum_xy, 48);
        memcpy(ps[1].y.v, sum_xy + 6, 48);
        ps[1].infinity = sum_inf != 0;
        const P::G2Affine qs[2] = {g2sl, P::g2_generator()};
        *pass = P::pairing_product_is_one(ps, qs, 2);
        t_pair += ms_since(t0);
        ++folds;
        return TYPLONK_OK;
    }
    // the verdicts of the live cells of [lo, hi), as FoldBisect::decide: accept all when their fold holds, else split the LIVE
    // cells of the range in half; a single live cell whose fold fails is the bad one
    int decide(uint64_t lo, uint64_t hi, uint8_t* status) {
        uint64_t n_live = 0;
        for (uint64_t i = lo; i < hi; ++i) n_live += live[i];
        if (!n_live) return TYPLONK_OK;
        bool pass = false;
        int rc = fold(lo, hi, &pass);
        if (rc) return rc;
        if (pass) return TYPLONK_OK;   // (a live cell's status starts out as TYPLONK_CELL_OK)
        if (n_live == 1) {
            for (uint64_t i = lo; i < hi; ++i)
                if (live[i]) status[i] = TYPLONK_CELL_BAD_PROOF;
            return TYPLONK_OK;
        }
        uint64_t seen = 0, mid = lo;
        for (; mid < hi; ++mid) {
            if (live[mid] && seen == n_live / 2) break;
            seen += live[mid];
        }
        rc = decide(lo, mid, status);
        if (!rc) rc = decide(mid, hi, status);
        return rc;
    }
};

}  // namespace

int typlonk_verify_chunks_challenge(const uint8_t seed[32], uint32_t log_n, uint32_t log_l, uint64_t N, uint64_t M,
                                    const uint64_t g2sl_xy[24], uint64_t rho[4]) {
    if (!seed || !g2sl_xy || !rho) return TYPLONK_ERR_INVALID_ARG;
    const Fr r = chunks_challenge(seed, log_n, log_l, N, M, g2sl_xy);
    memcpy(rho, r.v, 32);
    return TYPLONK_OK;
}

int typlonk_verify_chunks(typlonk_ctx* ctx, uint32_t srs_id, uint32_t log_n, uint32_t log_l, const uint64_t g2sl_xy[24],
                          const uint8_t seed[32], const uint64_t* commits_xy, const uint8_t* commits_inf, size_t M,
                          const uint32_t* cell_commit, const uint32_t* cell_coset, const uint64_t* evals, const uint64_t* proofs_xy,
                          const uint8_t* proofs_inf, size_t N, uint8_t* status, typlonk_chunks_report* report) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    if (!g2sl_xy || !seed || !commits_xy || !commits_inf || !cell_commit || !cell_coset || !evals || !proofs_xy || !proofs_inf ||
        !status || !report)
        return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    if (log_n < 1 || log_n > CHUNKS_MAX_LOG_N) return fail(ctx, TYPLONK_ERR_DOMAIN, "log_n outside 1..24");
    if (log_l >= log_n) return fail(ctx, TYPLONK_ERR_DOMAIN, "log_l >= log_n: the domain is cut into at least two cosets");
    if (log_l > VERIFY_CHUNKS_MAX_LOG_L) return fail(ctx, TYPLONK_ERR_DOMAIN, "log_l > 10: a cell's evaluations are transformed in the LDS");
    const uint64_t l = 1ull << log_l, r = 1ull << (log_n - log_l);
    if (N == 0 || M == 0) return fail(ctx, TYPLONK_ERR_LENGTH, "a call takes at least one cell and one commitment");
    if (N > CHUNKS_MAX_ELEMS / l) return fail(ctx, TYPLONK_ERR_LENGTH, "N * l > 2^25 evaluations");
    if (M > CHUNKS_MAX_ELEMS || N > CHUNKS_MAX_ELEMS - M) return fail(ctx, TYPLONK_ERR_LENGTH, "N + M > 2^25 points");
    auto it = ctx->srs.find(srs_id);
    if (it == ctx->srs.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown srs id");
    if (it->second.total_len) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "this call needs a whole SRS, not a shard (with or without a communicator)");
    if (it->second.open_all_log_n) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "srs_id names a table of typlonk_srs_open_chunks_table or typlonk_srs_open_all_table, not an SRS");
    if (it->second.len < l) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "the entry holds fewer than 2^log_l points");
    P::G2Affine g2sl;
    if (!g2_from_limbs(g2sl_xy, &g2sl)) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "g2sl is not a point of the twist");
    for (size_t i = 0; i < N; ++i)
        if (cell_commit[i] >= M || cell_coset[i] >= r) return fail(ctx, TYPLONK_ERR_RANGE, "a cell names a commitment >= M or a coset >= r");
    HIPCHK(hipSetDevice(ctx->device));
    ProfilingOff prof_off(ctx);   // the MSMs of a fold are not calls of their own
    const bool timed = prof_off.saved;
    auto t0 = std::chrono::steady_clock::now();

    // ---- the host's share of the per-cell checks, and the upload ----
    std::vector<uint8_t> st(N, TYPLONK_CELL_OK), live(N, 0);
    for (size_t i = 0; i < N; ++i)
        for (uint64_t t = 0; t < l; ++t)
            if (!fr_canonical(evals + (i * l + t) * 4)) {
                st[i] = TYPLONK_CELL_BAD_EVAL;
                break;
            }
    DevGuard guard;
    auto dev = [&](void** p, size_t bytes) {
        const hipError_t e = hipMalloc(p, bytes);
        if (e == hipSuccess) guard.add(*p);
        return e;
    };
    // the temporary entry: the proofs, then the commitments (as typlonk_srs_load makes one)
    const size_t NM = N + M;
    SrsEntry e;
    e.len = NM;
    uint8_t *d_inf = nullptr, *d_flags = nullptr, *d_live = nullptr;
    uint32_t* d_idx = nullptr;   // the cells sorted by commitment (N), cell_coset (N), each commitment's first position (M + 1)
    Fr *d_evals = nullptr, *d_w = nullptr, *d_small = nullptr, *d_partial = nullptr;
    HIPCHK(hipMalloc((void**)&e.d_points, NM * PT_WORDS * 4));
    DevGuard points_guard;
    points_guard.add(e.d_points);
    HIPCHK(dev((void**)&d_inf, 2 * NM + N));
    d_flags = d_inf + NM;
    d_live = d_flags + NM;
    HIPCHK(dev((void**)&d_idx, (2 * N + M + 1) * sizeof(uint32_t)));
    HIPCHK(dev((void**)&d_evals, N * l * sizeof(Fr)));
    // pw, the shifted powers launch_fr_powers writes beside them (unused: coset_a takes their place), s_pi, s_all, scale, twist
    HIPCHK(dev((void**)&d_w, (4 * N + 2 * NM) * sizeof(Fr)));
    const VerifyChunksPlan whole = verify_chunks_plan(N, log_l);   // every fold is planned with ITS strip (ChunksFold::strip)
    HIPCHK(dev((void**)&d_partial, whole.blocks * l * sizeof(Fr)));
    HIPCHK(dev((void**)&d_small, (l + whole.tw) * sizeof(Fr)));    // A, then the twiddles
    HIPCHK(hipMemcpy2DAsync(e.d_points, PT_WORDS * 4, proofs_xy, 96, 96, N, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpy2DAsync(e.d_points + N * PT_WORDS, PT_WORDS * 4, commits_xy, 96, 96, M, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_inf, proofs_inf, N, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_inf + N, commits_inf, M, hipMemcpyHostToDevice, ctx->stream));
    launch_convert_points(e.d_points, d_inf, (uint64_t)NM, ctx->stream);   // arkworks -> internal form
    HIPCHK(hipGetLastError());
    // a counting sort of the cells by commitment, ascending within one: w_c's workgroup reads its own cells only
    std::vector<uint32_t> first(M + 1, 0), order(N);
    for (size_t i = 0; i < N; ++i) ++first[cell_commit[i] + 1];
    for (size_t c = 0; c < M; ++c) first[c + 1] += first[c];
    {
        std::vector<uint32_t> next(first.begin(), first.end() - 1);
        for (size_t i = 0; i < N; ++i) order[next[cell_commit[i]]++] = (uint32_t)i;
    }
    HIPCHK(hipMemcpyAsync(d_idx, order.data(), N * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_idx + 2 * N, first.data(), (M + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_idx + N, cell_coset, N * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_evals, evals, N * l * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    std::vector<Fr> tw(whole.tw);
    tw[0] = Fr::one();
    const Fr mu_inv = log_l ? fr_domain_root_inv(log_l) : Fr::one();
    for (size_t j = 1; j < tw.size(); ++j) tw[j] = fe_mul(tw[j - 1], mu_inv);
    HIPCHK(hipMemcpyAsync(d_small + l, tw.data(), tw.size() * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const double t_upload = ms_since(t0);
    t0 = std::chrono::steady_clock::now();

    // ---- membership: one flag per point; a point that fails becomes the identity ----
    launch_chunks_membership(e.d_points, (uint64_t)NM, d_flags, /*clear=*/true, ctx->stream);
    HIPCHK(hipGetLastError());
    std::vector<uint8_t> flags(NM);
    HIPCHK(hipMemcpyAsync(flags.data(), d_flags, NM, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    uint64_t n_live = 0;
    for (size_t i = 0; i < N; ++i) {
        if (st[i] == TYPLONK_CELL_OK && flags[i]) st[i] = TYPLONK_CELL_BAD_POINT;
        if (st[i] == TYPLONK_CELL_OK && flags[N + cell_commit[i]]) st[i] = TYPLONK_CELL_BAD_COMMITMENT;
        live[i] = st[i] == TYPLONK_CELL_OK;
        n_live += live[i];
    }
    HIPCHK(hipMemcpyAsync(d_live, live.data(), N, hipMemcpyHostToDevice, ctx->stream));
    const double t_member = ms_since(t0);

    // ---- the weights' powers, the fold over all live cells, and the bisection when it fails ----
    launch_fr_powers(chunks_challenge(seed, log_n, log_l, N, M, g2sl_xy), (uint64_t)N, d_w, d_w + N, ctx->stream);
    HIPCHK(hipGetLastError());
    Fr* s_pi = d_w + 2 * N;
    Fr* s_all = s_pi + NM;
    Fr* scale = s_all + NM;
    // what depends on a cell's coset alone, once per call (behind the powers on the same stream: over the shifted ones)
    launch_chunks_cosets(d_idx + N, (uint64_t)N, fr_domain_root(log_n - log_l), fr_domain_root_inv(log_n), d_w + N, scale + N, ctx->stream);
    HIPCHK(hipGetLastError());
    const uint32_t tmp_id = ctx->next_srs++;
    ctx->srs[tmp_id] = e;
    points_guard.dismiss();   // the entry owns its records now
    TempSrs tmp{ctx, tmp_id};
    ChunksFold f{ctx, srs_id, tmp_id, log_l, (uint64_t)N, (uint64_t)M, live, whole.strip, fr_inv_pow2(log_l), d_w, d_w + N, d_idx,
                 d_idx + 2 * N, d_live, d_evals, d_small + l, s_pi, s_all, scale, scale + N, d_partial, d_small, g2sl, timed};
    // every return below leaves the lanes drained (the MSMs of a fold are waited for), so the guards may free
    if (int rc = f.decide(0, N, st.data())) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    typlonk_chunks_report rep;
    memset(&rep, 0, sizeof(rep));
    rep.folds = f.folds;
    rep.live = n_live;
    for (size_t i = 0; i < N; ++i) ++rep.count[st[i]];
    memcpy(status, st.data(), N);
    *report = rep;
    if (!timed) return TYPLONK_OK;
    prof_begin(ctx);
    ctx->prof_result.clear();
    ctx->prof_result.push_back({"chunks_upload", (float)t_upload});
    ctx->prof_result.push_back({"chunks_membership", (float)t_member});
    ctx->prof_result.push_back({"chunks_kernels", (float)f.t_kernels});
    ctx->prof_result.push_back({"chunks_msm", (float)f.t_msm});
    ctx->prof_result.push_back({"chunks_pairing", (float)f.t_pair});
    ctx->prof_result.push_back({"chunks_folds", (float)f.folds});
    return TYPLONK_OK;
}
