// libtyplonk_hip.so -- typlonk_srs_open_chunks_table and typlonk_open_chunks_* (include/typlonk.h): the KZG multi-proofs of
// `count` polynomials on EVERY coset of their evaluation domain in one call (Feist-Khovratovich, the chunked form) -- and
// typlonk_srs_open_all_table and typlonk_open_all_*, the same with one point per coset and one polynomial (at the end).  Host
// side only; the kernels (g1_pointwise_msm_kernel, the two stage kernels, open_chunks_*_kernel) are in g1_fft.hip, the
// stage loop (g1_ntt_stages) in srs_check.hip and the pointwise pass's launch shape in open_chunks_plan.hpp.
//
// n = 2^log_n, l = 2^log_l, r = n / l >= 2, w the generator of the size-n domain (w^l that of the size-r domain), S_m the
// source entry's points, f_0 .. f_(n-1) the coefficients.  Coset k < r is {w^(k + r t) : t < l}, the roots of X^l - a_k,
// a_k = w^(k l):
//     f    = q_k (X^l - a_k) + I_k,  deg I_k < l,  I_k = f on coset k
//     pi_k = [q_k(s)] G = sum_{i<r} [w^(l i k)] h_i
//     h_i  = sum_{m=0}^{n-1-(i+1)l} f_(m+(i+1)l) S_m   (i <= r - 2),   h_(r-1) = O
// With f^(j)_a = f_(a l + j) and S^(j)_a = S_(a l + j), j < l, a < r:  h_i = sum_j h^(j)_i, each h^(j) a correlation of the
// decimated sequences, computed as a circular product of size 2r, and the l of them are summed in the Fourier domain:
//   once per (SRS, log_n, log_l), the TABLE   y^(j) = DFT_2r(S^(j)_(r-2), ..., S^(j)_0, O x (r + 1)),  y^(j)_i at record j 2r + i
//   per polynomial   v^(j) = NTT_2r(c^(j)) / 2r,  c^(j) = (f^(j)_(r-1), 0 x r, f^(j)_0, ..., f^(j)_(r-2))      over Fr
//                    u_i = sum_{j<l} [v^(j)_i] y^(j)_i,  i < 2r                                      the pointwise pass
//                    h^ = DFT_2r^-1(u) without scaling: h_i = h^_i for i < r (h^_(r-1) comes out as the identity)
//                    pi = DFT_r(h), root w^l
// and the evaluations are one forward Fr transform of the padded f, stored chunk-major: evals[k l + t] = f(w^(k + r t)).
// l = 1 is the opening at every point of the domain: r = n, pi_k the proof at w^k, u_i = [v_i] y_i one ladder per record.
#include "host.hpp"
#include "open_chunks_plan.hpp"

using namespace ty;
using namespace tyh;

namespace {

constexpr uint32_t OPEN_CHUNKS_MAX_LOG_N = 24;              // 2n <= 2^25 records, the SRS length cap
constexpr size_t OPEN_CHUNKS_MAX_RECORDS = (size_t)1 << 25;   // count * 2r, the records of one temporary buffer

// the table a call works on, or the refusal; one_point: the call is typlonk_open_all_*, which takes a table of log_l = 0 only
int table_entry(typlonk_ctx* ctx, uint32_t table_id, bool one_point, const SrsEntry** out) {
    auto it = ctx->srs.find(table_id);
    if (it == ctx->srs.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown table id");
    if (!it->second.open_all_log_n)
        return fail(ctx, TYPLONK_ERR_INVALID_ARG, "this SRS entry is not a table of typlonk_srs_open_chunks_table or typlonk_srs_open_all_table");
    if (one_point && it->second.open_chunks_log_l)
        return fail(ctx, TYPLONK_ERR_INVALID_ARG, "this table's cosets hold more than one point (typlonk_srs_open_chunks_table, log_l > 0): typlonk_open_chunks_* takes it");
    *out = &it->second;
    return TYPLONK_OK;
}

// what the four opening calls refuse alike (typlonk_open_all_*: count = 1)
int admit(typlonk_ctx* ctx, const SrsEntry& tab, size_t m, size_t count) {
    const size_t n = (size_t)1 << tab.open_all_log_n;
    if (m < 1 || m > n) return fail(ctx, TYPLONK_ERR_LENGTH, "an opening takes 1 <= m <= 2^log_n coefficients");
    if (count < 1) return fail(ctx, TYPLONK_ERR_LENGTH, "an opening takes at least one polynomial");
    const size_t r2 = (2 * n) >> tab.open_chunks_log_l;
    if (count > OPEN_CHUNKS_MAX_RECORDS / r2) return fail(ctx, TYPLONK_ERR_LENGTH, "count * 2r > 2^25 records");
    return TYPLONK_OK;
}

// The call behind the four opening entry points, every argument admitted.  f: `count` device pointers to m coefficients each, or h_f: host
// pointers -- those are staged in a buffer of their own.
int open_chunks_run(typlonk_ctx* ctx, const SrsEntry& tab, std::vector<const Fr*>& f, const uint64_t* const* h_f, size_t m, size_t count,
                    uint64_t* proofs_xy, uint8_t* proofs_inf, uint64_t* evals) {
    const uint32_t log_n = tab.open_all_log_n, log_l = tab.open_chunks_log_l, log_r = log_n - log_l;
    const size_t n = (size_t)1 << log_n, l = (size_t)1 << log_l, r = (size_t)1 << log_r;
    HIPCHK(hipSetDevice(ctx->device));
    // the temporaries of the call: two buffers of count * 2r records, one of count * 2n Fr, `count` pointers, and in the host
    // form count * m Fr
    DevGuard guard;
    uint32_t *ra = nullptr, *rb = nullptr;
    Fr *c = nullptr, *stage = nullptr;
    const Fr** d_f = nullptr;
    HIPCHK(hipMalloc((void**)&ra, count * 2 * r * PT_WORDS * 4));
    guard.add(ra);
    HIPCHK(hipMalloc((void**)&rb, count * 2 * r * PT_WORDS * 4));
    guard.add(rb);
    HIPCHK(hipMalloc((void**)&c, count * 2 * n * sizeof(Fr)));
    guard.add(c);
    HIPCHK(hipMalloc((void**)&d_f, count * sizeof(Fr*)));
    guard.add(d_f);
    ProfilingOff prof_off(ctx);   // the transforms inside are not calls of their own
    if (h_f) {
        HIPCHK(hipMalloc((void**)&stage, count * m * sizeof(Fr)));
        guard.add(stage);
        for (size_t p = 0; p < count; ++p) {
            HIPCHK(hipMemcpyAsync(stage + p * m, h_f[p], m * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
            f[p] = stage + p * m;
        }
    }
    HIPCHK(hipMemcpyAsync(d_f, f.data(), count * sizeof(Fr*), hipMemcpyHostToDevice, ctx->stream));
    int rc;
    std::vector<Fr*> vecs;
    if (evals) {   // in the two halves of c: the padded polynomials and their transforms, then the chunk-major copy
        launch_open_chunks_pad(d_f, m, n, count, c, ctx->stream);
        HIPCHK(hipGetLastError());
        vecs.resize(count);
        for (size_t p = 0; p < count; ++p) vecs[p] = c + p * n;
        if ((rc = ntt_run_batch(ctx, vecs.data(), count, log_n, /*inverse=*/0, nullptr, /*sync=*/false))) return rc;
        launch_open_chunks_evals(c, r, l, count, c + count * n, ctx->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(evals, c + count * n, count * n * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    }
    // 1/(2r) of the inverse group transform and the step out of Montgomery form folded into the coefficients (the Fr transform
    // is linear): the words of v are then the canonical scalars the pointwise pass reads bit by bit
    launch_open_chunks_coeffs(d_f, m, r, l, count, fe_from_mont(fr_inv_pow2(log_r + 1)), c, ctx->stream);
    HIPCHK(hipGetLastError());
    vecs.resize(count * l);
    for (size_t v = 0; v < count * l; ++v) vecs[v] = c + v * 2 * r;
    if ((rc = ntt_run_batch(ctx, vecs.data(), count * l, log_r + 1, /*inverse=*/0, nullptr, /*sync=*/false))) return rc;
    const OpenChunksPlan pl = open_chunks_plan(count, r, l);
    launch_g1_pointwise_msm(c, tab.d_points, ra, pl.outputs, 2 * r, (uint32_t)l, pl.g, ctx->stream);
    HIPCHK(hipGetLastError());
    if ((rc = g1_ntt_stages(ctx, log_r + 1, count, ra, 2 * r, rb, 2 * r, /*inverse=*/true))) return rc;
    if ((rc = g1_ntt_stages(ctx, log_r, count, rb, 2 * r, ra, r, /*inverse=*/false))) return rc;   // h^[0, r) of each block
    return points_to_host(ctx, ra, count * r, proofs_xy, proofs_inf);   // (waits for the evaluations' copy too)
}

// An opening call from its first refusal on.  polys: `count` device buffers, read from offsets[p] (NULL: from 0) -- or, with
// polys NULL, coeffs: `count` host pointers.  one_point: table_entry.
int open_call(typlonk_ctx* ctx, uint32_t table_id, bool one_point, const typlonk_buf* const* polys, const size_t* offsets,
              const uint64_t* const* coeffs, size_t m, size_t count, uint64_t* proofs_xy, uint8_t* proofs_inf, uint64_t* evals) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    if ((!polys && !coeffs) || !proofs_xy || !proofs_inf) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    const SrsEntry* tab = nullptr;
    if (int rc = table_entry(ctx, table_id, one_point, &tab)) return rc;
    if (int rc = admit(ctx, *tab, m, count)) return rc;
    std::vector<const Fr*> f(count);
    for (size_t p = 0; p < count; ++p) {
        if (polys ? !polys[p] : !coeffs[p]) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null polynomial");
        if (!polys) continue;
        const size_t off = offsets ? offsets[p] : 0;
        if (off > polys[p]->n || m > polys[p]->n - off) return fail(ctx, TYPLONK_ERR_RANGE, "range outside buffer");
        f[p] = polys[p]->d + off;
    }
    return open_chunks_run(ctx, *tab, f, polys ? nullptr : coeffs, m, count, proofs_xy, proofs_inf, evals);
}

}  // namespace

int typlonk_srs_open_chunks_table(typlonk_ctx* ctx, uint32_t srs_id, uint32_t log_n, uint32_t log_l, uint32_t* table_id) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    if (!table_id) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    if (log_n < 1 || log_n > OPEN_CHUNKS_MAX_LOG_N) return fail(ctx, TYPLONK_ERR_DOMAIN, "log_n outside 1..24: the table holds 2^(log_n + 1) <= 2^25 records");
    if (log_l >= log_n) return fail(ctx, TYPLONK_ERR_DOMAIN, "log_l >= log_n: the domain is cut into at least two cosets");
    auto it = ctx->srs.find(srs_id);
    if (it == ctx->srs.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown srs id");
    const SrsEntry& src = it->second;
    if (src.total_len) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "this call needs a whole SRS, not a shard (with or without a communicator)");
    if (src.open_all_log_n) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "the source is itself a table of typlonk_srs_open_chunks_table or typlonk_srs_open_all_table");
    const size_t n = (size_t)1 << log_n, l = (size_t)1 << log_l, r = n / l;
    if (src.len < n - l) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "the entry holds fewer than 2^log_n - 2^log_l points");
    HIPCHK(hipSetDevice(ctx->device));
    SrsEntry e;
    e.len = 2 * n;
    e.open_all_log_n = log_n;
    e.open_chunks_log_l = log_l;
    DevGuard guard;
    HIPCHK(hipMalloc((void**)&e.d_points, 2 * n * PT_WORDS * 4));
    guard.add(e.d_points);
    uint32_t* rev = nullptr;   // the decimated, reversed, padded points: stage 1 reads them through the bit reversal
    DevGuard tmp;              // (freed when the call returns)
    HIPCHK(hipMalloc((void**)&rev, 2 * n * PT_WORDS * 4));
    tmp.add(rev);
    launch_open_chunks_gather(src.d_points, rev, (uint64_t)r, (uint64_t)l, ctx->stream);
    HIPCHK(hipGetLastError());
    if (int rc = g1_ntt_stages(ctx, log_n - log_l + 1, l, rev, 2 * r, e.d_points, 2 * r, /*inverse=*/false)) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    guard.dismiss();
    const uint32_t id = ctx->next_srs++;
    ctx->srs[id] = e;
    *table_id = id;
    return TYPLONK_OK;
}


int typlonk_open_chunks_dev(typlonk_ctx* ctx, uint32_t table_id, const typlonk_buf* const* polys, const size_t* offsets, size_t m,
                            size_t count, uint64_t* proofs_xy, uint8_t* proofs_inf, uint64_t* evals) {
    return open_call(ctx, table_id, /*one_point=*/false, polys, offsets, nullptr, m, count, proofs_xy, proofs_inf, evals);
}

int typlonk_open_chunks_host(typlonk_ctx* ctx, uint32_t table_id, const uint64_t* const* coeffs, size_t m, size_t count,
                             uint64_t* proofs_xy, uint8_t* proofs_inf, uint64_t* evals) {
    return open_call(ctx, table_id, /*one_point=*/false, nullptr, nullptr, coeffs, m, count, proofs_xy, proofs_inf, evals);
}

// ---- one point per coset: log_l = 0, one polynomial -------------------------------------------------------------------------
int typlonk_srs_open_all_table(typlonk_ctx* ctx, uint32_t srs_id, uint32_t log_n, uint32_t* table_id) {
    return typlonk_srs_open_chunks_table(ctx, srs_id, log_n, 0, table_id);
}

int typlonk_open_all_dev(typlonk_ctx* ctx, uint32_t table_id, const typlonk_buf* poly, size_t offset, size_t m, uint64_t* proofs_xy,
                         uint8_t* proofs_inf, uint64_t* evals) {
    if (ctx && !poly) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    return open_call(ctx, table_id, /*one_point=*/true, &poly, &offset, nullptr, m, 1, proofs_xy, proofs_inf, evals);
}

int typlonk_open_all_host(typlonk_ctx* ctx, uint32_t table_id, const uint64_t* coeffs, size_t m, uint64_t* proofs_xy,
                          uint8_t* proofs_inf, uint64_t* evals) {
    if (ctx && !coeffs) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    return open_call(ctx, table_id, /*one_point=*/true, nullptr, nullptr, &coeffs, m, 1, proofs_xy, proofs_inf, evals);
}
