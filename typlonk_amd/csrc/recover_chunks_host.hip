// libtyplonk_hip.so -- typlonk_recover_chunks (include/typlonk.h): `count` polynomials from K of the r cosets of their domain.
// Host side only; the kernels are in recover_chunks.hip and every decision of a call -- the refusals, the sizes, the launch
// shapes -- in recover_chunks_plan.hpp.
//
// M = the r - K cosets the call does not name, Z'(Y) = prod_{j in M} (Y - a_j), Z(X) = Z'(X^l):
//   1. Zd[k] = Z'(a_k) and Zc[i] = Z'(g^l a_i), i, k < r: Z on coset k of the domain and at g w^i' for i' = i mod r
//   2. V_p[k + r t] = E_p[i][t] Zd[k_i] on the known cosets, zero on the missing ones: h_p Z on the whole domain
//   3. P_p = iNTT_n(V_p) = h_p Z exactly (deg < K l + (r - K) l = n)
//   4. coset NTT_n (shift g), times 1 / Zc[i mod r], coset iNTT_n (shift g): h_p; coefficients [K l, n) are zero whatever the input
//   5. the verdict from [m, K l), the outputs after it -- on the device: the copy is queued before the host sees a status
#include "host.hpp"
#include "host_checks.hpp"
#include "recover_chunks_plan.hpp"

#include <chrono>

using namespace ty;
using namespace tyh;

static_assert(RECOVER_INVALID_ARG == TYPLONK_ERR_INVALID_ARG && RECOVER_LENGTH == TYPLONK_ERR_LENGTH && RECOVER_DOMAIN == TYPLONK_ERR_DOMAIN &&
                  RECOVER_RANGE == TYPLONK_ERR_RANGE,
              "recover_chunks_plan.hpp states the codes of typlonk.h");
static_assert(sizeof(size_t) == sizeof(uint64_t), "offsets are read as 64-bit words");

int typlonk_recover_chunks(typlonk_ctx* ctx, uint32_t log_n, uint32_t log_l, size_t m, const uint32_t* cosets, size_t K, const uint64_t* evals,
                           size_t count, typlonk_buf* const* coeffs_dev, const size_t* offsets, uint64_t* coeffs, uint64_t* evals_out,
                           uint8_t* status, uint64_t* first_excess, typlonk_recover_report* report) {
    // ---- the refusals, as the plan states them ----
    std::vector<const void*> buf_id;
    std::vector<uint64_t> buf_len;
    // The refusals are a pure function of plain arguments, so the lengths of the `count` destination buffers are gathered first --
    // on purpose before anything is judged: "a null entry of coeffs_dev" comes before the DOMAIN and LENGTH refusals in the header's
    // order, and reading coeffs_dev[p]->n is all this walk does.  (A count of zero or past the cap is refused before an entry matters.)
    if (ctx && coeffs_dev && count && count <= RECOVER_MAX_ELEMS) {
        buf_id.resize(count);
        buf_len.resize(count);
        for (size_t p = 0; p < count; ++p) {
            buf_id[p] = coeffs_dev[p];
            buf_len[p] = coeffs_dev[p] ? coeffs_dev[p]->n : 0;
        }
    }
    RecoverChunksArgs a;
    a.ctx = ctx != nullptr;
    a.evals = evals != nullptr;
    a.status = status != nullptr;
    a.report = report != nullptr;
    a.log_n = log_n;
    a.log_l = log_l;
    a.m = m;
    a.cosets = cosets;
    a.K = K;
    a.count = count;
    a.want_dev = coeffs_dev != nullptr;
    a.want_coeffs = coeffs != nullptr;
    a.want_evals = evals_out != nullptr;
    a.buf_id = buf_id.data();
    a.buf_len = buf_len.data();
    a.offsets = reinterpret_cast<const uint64_t*>(offsets);
    if (a.want_dev && buf_id.empty()) {   // count = 0 or past the cap: LENGTH unless something earlier applies; no entry is read
        a.want_dev = false;
        a.want_coeffs = true;
    }
    const RecoverVerdict verdict = recover_chunks_refusal(a);
    if (verdict.code != RECOVER_ADMITTED) return ctx ? fail(ctx, verdict.code, verdict.text) : verdict.code;
    const RecoverChunksPlan pl = recover_chunks_plan(log_n, log_l, m, K, count, coeffs != nullptr, evals_out != nullptr);
    const size_t n = pl.n, l = pl.l, r = pl.r, Kl = K * l;
    HIPCHK(hipSetDevice(ctx->device));
    ProfilingOff prof_off(ctx);   // the transforms inside are not calls of their own
    const bool timed = prof_off.saved;

    // ---- the host's share: the canonical check, the map from coset to cell, the list of the missing ----
    std::vector<uint8_t> fixed(count, TYPLONK_RECOVER_OK);
    for (size_t p = 0; p < count; ++p)
        for (size_t e = 0; e < Kl; ++e)
            if (!fr_canonical(evals + (p * Kl + e) * 4)) {
                fixed[p] = TYPLONK_RECOVER_BAD_EVAL;
                break;
            }
    std::vector<uint32_t> index(r + (pl.missing ? pl.missing : 1), 0);   // pos, then the missing cosets ascending
    for (size_t k = 0; k < r; ++k) index[k] = RECOVER_NO_CELL;
    for (size_t i = 0; i < K; ++i) index[cosets[i]] = (uint32_t)i;
    for (size_t k = 0, j = 0; k < r; ++k)
        if (index[k] == RECOVER_NO_CELL) index[r + j++] = (uint32_t)k;
    std::vector<Fr*> dst(count, nullptr), vecs(count);
    if (coeffs_dev)
        for (size_t p = 0; p < count; ++p) dst[p] = coeffs_dev[p]->d + (offsets ? offsets[p] : 0);

    // ---- the temporaries (recover_chunks_plan's bytes_*), all of them before anything is queued ----
    DevGuard guard;
    auto dev = [&](void** p, size_t bytes) {
        const hipError_t e = hipMalloc(p, bytes);
        if (e == hipSuccess) guard.add(*p);
        return e;
    };
    Fr *d_consts = nullptr, *d_partial = nullptr, *d_cells = nullptr, *d_work = nullptr, *d_out = nullptr, *d_ev = nullptr;
    uint32_t* d_index = nullptr;
    unsigned long long* d_verdict = nullptr;   // mins (count B), first_excess and status (2 count), dst (count), fixed (count bytes)
    HIPCHK(dev((void**)&d_consts, pl.bytes_consts));
    HIPCHK(dev((void**)&d_partial, pl.bytes_partial));
    HIPCHK(dev((void**)&d_index, pl.bytes_index));
    HIPCHK(dev((void**)&d_cells, pl.bytes_cells));
    HIPCHK(dev((void**)&d_work, pl.bytes_work));
    if (pl.bytes_out) HIPCHK(dev((void**)&d_out, pl.bytes_out));
    if (pl.bytes_evals) HIPCHK(dev((void**)&d_ev, pl.bytes_evals));
    HIPCHK(dev((void**)&d_verdict, pl.bytes_verdict));
    unsigned long long* d_mins = d_verdict;
    unsigned long long* d_res = d_mins + count * pl.excess_blocks;
    Fr** d_dst = reinterpret_cast<Fr**>(d_res + 2 * count);
    uint8_t* d_fixed = reinterpret_cast<uint8_t*>(d_dst + count);
    Fr *pw = d_consts, *z = d_consts + 2 * r;   // a_k, the shifted powers launch_fr_powers writes beside them (unused), Zd, Zc

    auto t0 = std::chrono::steady_clock::now();
    std::vector<std::pair<const char*, float>> stages;
    // a stage's end under profiling: the device drained, its wall time noted
    auto stage_end = [&](const char* name) -> hipError_t {
        if (!timed) return hipSuccess;
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        const auto t1 = std::chrono::steady_clock::now();
        stages.push_back({name, std::chrono::duration<float, std::milli>(t1 - t0).count()});
        t0 = std::chrono::steady_clock::now();
        return e;
    };

    // ---- 1: the vanishing values ----
    HIPCHK(hipMemcpyAsync(d_index, index.data(), pl.bytes_index, hipMemcpyHostToDevice, ctx->stream));
    launch_fr_powers(fr_domain_root(log_n - log_l), (uint64_t)r, pw, pw + r, ctx->stream);
    HIPCHK(hipGetLastError());
    Fr gl;
    const uint64_t* g_limbs = coset_g(&gl);
    for (uint32_t s = 0; s < log_l; ++s) gl = fe_sqr(gl);
    launch_recover_vanish(pw, d_index + r, gl, pl, d_partial, z, ctx->stream);
    HIPCHK(hipGetLastError());
    launch_recover_invert(z + r, (uint64_t)r, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(stage_end("recover_vanish"));

    // ---- 2: the cells up (a BAD_EVAL polynomial's as zeros), and onto the domain ----
    for (size_t p = 0; p < count;) {   // runs of polynomials with the same flag: one copy or one fill each
        size_t q = p + 1;
        while (q < count && (fixed[q] != 0) == (fixed[p] != 0)) ++q;
        if (fixed[p])
            HIPCHK(hipMemsetAsync(d_cells + p * Kl, 0, (q - p) * Kl * sizeof(Fr), ctx->stream));
        else
            HIPCHK(hipMemcpyAsync(d_cells + p * Kl, evals + p * Kl * 4, (q - p) * Kl * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
        p = q;
    }
    HIPCHK(hipMemcpyAsync(d_fixed, fixed.data(), count, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_dst, dst.data(), count * sizeof(Fr*), hipMemcpyHostToDevice, ctx->stream));
    launch_recover_scatter(d_cells, d_index, z, (uint64_t)K, log_n, log_l, (uint64_t)count, pl, d_work, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(stage_end("recover_scatter"));

    // ---- 3 and 4: h Z, then the division on the shifted domain ----
    for (size_t p = 0; p < count; ++p) vecs[p] = d_work + p * n;
    int rc;
    if ((rc = ntt_run_batch(ctx, vecs.data(), count, log_n, /*inverse=*/1, nullptr, /*sync=*/false))) return rc;
    HIPCHK(stage_end("recover_interp"));
    if ((rc = ntt_run_batch(ctx, vecs.data(), count, log_n, /*inverse=*/0, g_limbs, /*sync=*/false))) return rc;
    launch_recover_scale(d_work, z + r, (uint64_t)r, (uint64_t)count * n, ctx->stream);
    HIPCHK(hipGetLastError());
    if ((rc = ntt_run_batch(ctx, vecs.data(), count, log_n, /*inverse=*/1, g_limbs, /*sync=*/false))) return rc;
    HIPCHK(stage_end("recover_divide"));

    // ---- 5: the verdicts and the coefficients ----
    launch_recover_finish(d_work, (uint64_t)n, (uint64_t)m, (uint64_t)count, pl, d_fixed, coeffs_dev ? d_dst : nullptr, d_out, d_mins, d_res,
                          ctx->stream);
    HIPCHK(hipGetLastError());
    std::vector<unsigned long long> res(2 * count);
    HIPCHK(hipMemcpyAsync(res.data(), d_res, 2 * count * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    if (coeffs) HIPCHK(hipMemcpyAsync(coeffs, d_out, count * m * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(stage_end("recover_finish"));
    if (evals_out) {   // one more forward transform, of the finished coefficients (zeros for a polynomial that is not OK) padded to n
        std::vector<const Fr*> src(count);
        for (size_t p = 0; p < count; ++p) src[p] = d_out + p * m;
        if ((rc = ntt_run_batch(ctx, vecs.data(), count, log_n, /*inverse=*/0, nullptr, /*sync=*/false, src.data(), (uint64_t)m))) return rc;
        launch_open_chunks_evals(d_work, (uint64_t)r, (uint64_t)l, (uint64_t)count, d_ev, ctx->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(evals_out, d_ev, count * n * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(stage_end("recover_evals"));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));

    typlonk_recover_report rep;
    memset(&rep, 0, sizeof(rep));
    rep.known = (uint32_t)K;
    rep.missing = (uint32_t)pl.missing;
    for (size_t p = 0; p < count; ++p) {
        status[p] = (uint8_t)res[count + p];
        ++rep.count[status[p]];
        if (first_excess) first_excess[p] = res[p];
    }
    *report = rep;
    if (!timed) return TYPLONK_OK;
    prof_begin(ctx);
    ctx->prof_result.clear();
    for (const auto& s : stages) ctx->prof_result.push_back(s);
    return TYPLONK_OK;
}
