// libtyplonk_hip.so -- typlonk_srs_open_all_table and typlonk_open_all_* (include/typlonk.h): the KZG openings of one
// polynomial at EVERY point of its evaluation domain in one call (Feist-Khovratovich).  Host side only; the kernels
// (g1_pointwise_mul_kernel, open_all_gather_kernel, open_all_coeffs_kernel, srs_g1_ntt_stage_kernel) are in srs_gen.hip.
//
// n = 2^log_n, w the generator of the size-n domain, S_m the source entry's points, f_0 .. f_(n-1) the coefficients:
//     h_i  = sum_{m=0}^{n-2-i} f_(m+i+1) S_m   (i <= n - 2),   h_(n-1) = O
//     pi_k = sum_{i<n} [w^(ik)] h_i              the opening at w^k
// h is a correlation, computed as a circular product of size 2n:
//   once per (SRS, log_n), the TABLE   y = DFT_2n(S_(n-2), S_(n-3), ..., S_0, O x (n + 1))   in the group, no scaling
//   per polynomial   v = NTT_2n(c) / 2n,  c = (f_(n-1), 0 x n, f_0, ..., f_(n-2))            over Fr
//                    u_i = [v_i] y_i                                                          the pointwise ladder
//                    h^ = DFT_2n^-1(u) without scaling: h_i = h^_i for i < n (h^_(n-1) comes out as the identity)
//                    pi = DFT_n(h)
// and the evaluations f(w^k) are one forward Fr transform of the padded f.
#include "host.hpp"

using namespace ty;
using namespace tyh;

namespace {

constexpr uint32_t OPEN_ALL_MAX_LOG_N = 24;   // 2n <= 2^25 records, the SRS length cap

// the table a call works on, or the refusal
int table_entry(typlonk_ctx* ctx, uint32_t table_id, const SrsEntry** out) {
    auto it = ctx->srs.find(table_id);
    if (it == ctx->srs.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown table id");
    if (!it->second.open_all_log_n) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "this SRS entry is not a table of typlonk_srs_open_all_table");
    if (it->second.open_chunks_log_l)
        return fail(ctx, TYPLONK_ERR_INVALID_ARG, "this table's cosets hold more than one point (typlonk_srs_open_chunks_table, log_l > 0): typlonk_open_chunks_* takes it");
    *out = &it->second;
    return TYPLONK_OK;
}

// The call behind both entry points, every argument admitted.  f: the m coefficients on the device, or h_f: on the host --
// those are staged in the first record buffer, which nothing else needs before the pointwise pass.
int open_all_run(typlonk_ctx* ctx, const SrsEntry& tab, const Fr* f, const uint64_t* h_f, size_t m, uint64_t* proofs_xy,
                 uint8_t* proofs_inf, uint64_t* evals) {
    const uint32_t log_n = tab.open_all_log_n;
    const size_t n = (size_t)1 << log_n;
    HIPCHK(hipSetDevice(ctx->device));
    DevGuard guard;   // the temporaries of the call: two buffers of 2n records, one of 2n Fr
    uint32_t *ra = nullptr, *rb = nullptr;
    Fr* c = nullptr;
    HIPCHK(hipMalloc((void**)&ra, 2 * n * PT_WORDS * 4));
    guard.add(ra);
    HIPCHK(hipMalloc((void**)&rb, 2 * n * PT_WORDS * 4));
    guard.add(rb);
    HIPCHK(hipMalloc((void**)&c, 2 * n * sizeof(Fr)));
    guard.add(c);
    ProfilingOff prof_off(ctx);   // the transforms inside are not calls of their own
    if (h_f) {
        HIPCHK(hipMemcpyAsync(ra, h_f, m * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
        f = (const Fr*)ra;
    }
    int rc;
    if (evals) {
        ColumnSrc col;
        col.dev = f;
        col.rows = m;
        HIPCHK(column_to_device(c, col, n, ctx->stream));
        if ((rc = ntt_run(ctx, c, log_n, /*inverse=*/0, nullptr, /*sync=*/false))) return rc;
        HIPCHK(hipMemcpyAsync(evals, c, n * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    }
    launch_open_all_coeffs(f, m, n, fr_inv_pow2(log_n + 1), c, ctx->stream);
    HIPCHK(hipGetLastError());
    if ((rc = ntt_run(ctx, c, log_n + 1, /*inverse=*/0, nullptr, /*sync=*/false))) return rc;
    launch_g1_pointwise_mul(c, 2 * n, tab.d_points, ra, ctx->stream);
    HIPCHK(hipGetLastError());
    if ((rc = g1_ntt_stages(ctx, ra, rb, log_n + 1, /*inverse=*/true))) return rc;
    if ((rc = g1_ntt_stages(ctx, rb, ra, log_n, /*inverse=*/false))) return rc;
    return points_to_host(ctx, ra, n, proofs_xy, proofs_inf);   // (waits for the evaluations' copy too)
}

}  // namespace

int typlonk_srs_open_all_table(typlonk_ctx* ctx, uint32_t srs_id, uint32_t log_n, uint32_t* table_id) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    if (!table_id) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    if (log_n < 1 || log_n > OPEN_ALL_MAX_LOG_N) return fail(ctx, TYPLONK_ERR_DOMAIN, "log_n outside 1..24: the table holds 2^(log_n + 1) <= 2^25 records");
    auto it = ctx->srs.find(srs_id);
    if (it == ctx->srs.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown srs id");
    const SrsEntry& src = it->second;
    if (src.total_len) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "this call needs a whole SRS, not a shard (with or without a communicator)");
    if (src.open_all_log_n) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "the source is itself a table of typlonk_srs_open_all_table");
    const size_t n = (size_t)1 << log_n;
    if (src.len < n - 1) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "the entry holds fewer than 2^log_n - 1 points");
    HIPCHK(hipSetDevice(ctx->device));
    SrsEntry e;
    e.len = 2 * n;
    e.open_all_log_n = log_n;
    DevGuard guard;
    HIPCHK(hipMalloc((void**)&e.d_points, 2 * n * PT_WORDS * 4));
    guard.add(e.d_points);
    uint32_t* rev = nullptr;   // the reversed, padded points: stage 1 reads them through the bit reversal
    DevGuard tmp;              // (freed when the call returns)
    HIPCHK(hipMalloc((void**)&rev, 2 * n * PT_WORDS * 4));
    tmp.add(rev);
    launch_open_all_gather(src.d_points, rev, (uint64_t)n, ctx->stream);
    HIPCHK(hipGetLastError());
    if (int rc = g1_ntt_stages(ctx, rev, e.d_points, log_n + 1, /*inverse=*/false)) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    guard.dismiss();
    const uint32_t id = ctx->next_srs++;
    ctx->srs[id] = e;
    *table_id = id;
    return TYPLONK_OK;
}

int typlonk_open_all_dev(typlonk_ctx* ctx, uint32_t table_id, const typlonk_buf* poly, size_t offset, size_t m, uint64_t* proofs_xy,
                         uint8_t* proofs_inf, uint64_t* evals) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    if (!poly || !proofs_xy || !proofs_inf) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    const SrsEntry* tab = nullptr;
    if (int rc = table_entry(ctx, table_id, &tab)) return rc;
    if (m < 1 || m > ((size_t)1 << tab->open_all_log_n)) return fail(ctx, TYPLONK_ERR_LENGTH, "open_all takes 1 <= m <= 2^log_n coefficients");
    if (offset > poly->n || m > poly->n - offset) return fail(ctx, TYPLONK_ERR_RANGE, "range outside buffer");
    return open_all_run(ctx, *tab, poly->d + offset, nullptr, m, proofs_xy, proofs_inf, evals);
}

int typlonk_open_all_host(typlonk_ctx* ctx, uint32_t table_id, const uint64_t* coeffs, size_t m, uint64_t* proofs_xy,
                          uint8_t* proofs_inf, uint64_t* evals) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    if (!coeffs || !proofs_xy || !proofs_inf) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    const SrsEntry* tab = nullptr;
    if (int rc = table_entry(ctx, table_id, &tab)) return rc;
    if (m < 1 || m > ((size_t)1 << tab->open_all_log_n)) return fail(ctx, TYPLONK_ERR_LENGTH, "open_all takes 1 <= m <= 2^log_n coefficients");
    return open_all_run(ctx, *tab, nullptr, coeffs, m, proofs_xy, proofs_inf, evals);
}
