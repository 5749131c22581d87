// libtyplonk_hip.so -- the prover's device-side flow: quotient, grand product, openings, the three rounds, typlonk_prove
// Part of the host driver of include/typlonk.h (see host.hpp for the shared state).  There is deliberately no CPU compute
// fallback: without a HIP device typlonk_init fails with TYPLONK_ERR_NO_DEVICE.
#include "host.hpp"
#include "proof_script.hpp"

using namespace ty;
using namespace tyh;

// (entry points: C linkage comes from their declarations in include/typlonk.h)

namespace tyh {
const uint64_t* coset_g(Fr* g_out) {
    static uint64_t limbs[4];
    const Fr g = fr_from_u64(7);
    memcpy(limbs, g.v, sizeof(limbs));
    if (g_out) *g_out = g;
    return limbs;
}
int prover_workspaces(typlonk_ctx* ctx, const ProvePlan& plan) {
    const std::pair<DevBuf*, size_t> bufs[] = {{&ctx->prover_mem, plan.prover_mem}, {&ctx->ops_tmp, plan.ops_tmp},
                                               {&ctx->quot_ext, plan.quot_ext}, {&ctx->quot_tab, plan.quot_tab},
                                               {&ctx->batch_tab, plan.batch_tab}};
    for (const auto& b : bufs)
        if (const int rc = ensure(ctx, *b.first, b.second)) return rc;
    if (ctx->eval_slots_cap < plan.slots) {
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (ctx->eval_slots_host) HIPCHK(hipHostFree(ctx->eval_slots_host));
        ctx->eval_slots_host = nullptr;
        ctx->eval_slots_cap = 0;
        HIPCHK(hipHostMalloc((void**)&ctx->eval_slots_host, plan.slots * sizeof(Fr)));
        ctx->eval_slots_cap = plan.slots;
    }
    if (plan.batch_tab && !ctx->batch_host) HIPCHK(hipHostMalloc(&ctx->batch_host, plan.batch_tab));
    return TYPLONK_OK;
}
int quotient_domain(typlonk_ctx* ctx, uint32_t log_n, QuotientDomain* d) {
    const uint32_t log4 = log_n + 2;
    const Fr w4 = fr_domain_root(log4);
    const int rc = domain_twiddles(ctx, log4, &d->w_lo, &d->w_hi, &d->w_h);
    if (rc) return rc;
    d->n_hi = 1ull << (log4 - d->w_h);
    d->g_limbs = coset_g(&d->g);
    Fr gn = d->g, iota = w4;   // g^n; iota = w_{4n}^n, a primitive 4th root of unity
    for (uint32_t i = 0; i < log_n; ++i) {
        gn = fe_sqr(gn);
        iota = fe_sqr(iota);
    }
    Fr cur = gn;
    for (int k = 0; k < 4; ++k) {
        d->zh_inv[k] = fe_inv(fe_sub(cur, Fr::one()));
        cur = fe_mul(cur, iota);
    }
    return TYPLONK_OK;
}
}  // namespace tyh

namespace {
// zero-extend an n-coefficient vector (or the constant-coefficient polynomial `fill`) to 4n and
// evaluate it on the coset g*H_4n, in place in `e`
int quotient_extend(typlonk_ctx* ctx, Fr* e, const Fr* src, const Fr* fill, uint64_t n, uint32_t log4) {
    hipStream_t s = ctx->stream;
    // the coefficients are read in place, zero-padded to 4n by the first pass itself (no copy + 3n-element memset + reads
    // of the zeros: 160 MB of traffic and two launches per extension at n = 2^20)
    if (src) return ntt_run(ctx, e, log4, 0, coset_g(), /*sync=*/false, src, n);
    launch_fr_fill(e, n, *fill, s);
    HIPCHK(hipMemsetAsync(e + n, 0, 3 * n * sizeof(Fr), s));
    return ntt_run(ctx, e, log4, 0, coset_g(), /*sync=*/false);
}
// the same for `count` coefficient vectors at once (one launch per pass for the whole group)
int quotient_extend_batch(typlonk_ctx* ctx, Fr* const* e, const Fr* const* src, size_t count, uint64_t n, uint32_t log4) {
    return ntt_run_batch(ctx, e, count, log4, 0, coset_g(), /*sync=*/false, src, n);
}
}  // namespace

namespace tyh {
int circuit_finish(typlonk_ctx* ctx, CircuitEntry& e, const Fr* const src[8], bool sigma_forward, uint32_t* circuit_id) {
    const uint32_t log_n = e.log_n;
    const uint64_t n = 1ull << log_n, n4 = 4 * n;
    ProfilingOff prof_off(ctx);  // stage events are per call
    int rc = TYPLONK_OK;
    const Fr ninv = fe_inv(fr_from_u64(n));
    {
        // the eight coefficient vectors (builder.rs:84-88's five selectors, the three sigmas) as one batch, then L0
        Fr* dst[8];
        for (int k = 0; k < 8; ++k) dst[k] = e.ext + (uint64_t)k * n4;
        rc = quotient_extend_batch(ctx, dst, src, 8, n, log_n + 2);
        if (!rc) rc = quotient_extend(ctx, e.ext + 8 * n4, nullptr, &ninv, n, log_n + 2);
        Fr* sig[3] = {e.sig_ev, e.sig_ev + n, e.sig_ev + 2 * n};
        if (!rc && sigma_forward) rc = ntt_run_batch(ctx, sig, 3, log_n, 0, nullptr, /*sync=*/false);   // proof.rs:334-338
    }
    if (!rc) {
        rc = hip_rc(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (rc) return rc;
    const uint32_t id = ctx->next_circuit++;
    ctx->circuits[id] = e;
    *circuit_id = id;
    return TYPLONK_OK;
}
}  // namespace tyh

int typlonk_circuit_load(typlonk_ctx* ctx, const typlonk_buf* const selectors[5], const typlonk_buf* const sigma[3],
                         uint32_t log_n, uint32_t* circuit_id) {
    if (!ctx || !selectors || !sigma || !circuit_id) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    if (log_n < 1 || log_n > TYPLONK_MAX_PROVER_LOG_N) return fail(ctx, TYPLONK_ERR_DOMAIN, "quotient needs 1 <= log_n <= 24");
    HIPCHK(hipSetDevice(ctx->device));
    const uint64_t n = 1ull << log_n, n4 = 4 * n;
    const typlonk_buf* in[8] = {selectors[0], selectors[1], selectors[2], selectors[3], selectors[4],
                                sigma[0], sigma[1], sigma[2]};
    for (const typlonk_buf* b : in)
        if (!b || b->n < n) return fail(ctx, TYPLONK_ERR_RANGE, "circuit polynomial shorter than n");
    CircuitEntry e;
    e.log_n = log_n;
    DevGuard guard;
    HIPCHK(hipMalloc((void**)&e.ext, 9 * n4 * sizeof(Fr)));
    guard.add(e.ext);
    HIPCHK(hipMalloc((void**)&e.coef, 8 * n * sizeof(Fr)));
    guard.add(e.coef);
    HIPCHK(hipMalloc((void**)&e.sig_ev, 3 * n * sizeof(Fr)));
    guard.add(e.sig_ev);
    for (int k = 0; k < 8; ++k)
        HIPCHK(hipMemcpyAsync(e.coef + (uint64_t)k * n, in[k]->d, n * sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(e.sig_ev, e.coef + 5 * n, 3 * n * sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
    const Fr* src[8];
    for (int k = 0; k < 8; ++k) src[k] = in[k]->d;
    const int rc = circuit_finish(ctx, e, src, /*sigma_forward=*/true, circuit_id);
    if (rc) return rc;
    guard.dismiss();
    return TYPLONK_OK;
}

int typlonk_circuit_free(typlonk_ctx* ctx, uint32_t circuit_id) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    auto it = ctx->circuits.find(circuit_id);
    if (it == ctx->circuits.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown circuit id");
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipFree(it->second.ext));
    HIPCHK(hipFree(it->second.coef));
    HIPCHK(hipFree(it->second.sig_ev));
    circuit_check_release(it->second);
    ctx->circuits.erase(it);
    return TYPLONK_OK;
}

namespace {
// per-proof inputs first, then (without a cached circuit) the per-circuit ones
struct QuotientInputs {
    const typlonk_buf* in[13];
    const Fr* cached = nullptr;   // the circuit's coset evaluations from the circuit cache
    bool has_pi = false;          // NULL = zero polynomial (public inputs [0])
};
// what the quotient refuses, in this order, before it sizes or queues anything
int quotient_check(typlonk_ctx* ctx, const typlonk_quotient_args* args, uint32_t log_n, const typlonk_buf* t_out, QuotientInputs* qi) {
    if (log_n < 1 || log_n > TYPLONK_MAX_PROVER_LOG_N) return fail(ctx, TYPLONK_ERR_DOMAIN, "quotient needs 1 <= log_n <= 24");
    HIPCHK(hipSetDevice(ctx->device));
    const uint64_t n = 1ull << log_n;
    const typlonk_buf* in[13] = {args->wires[0], args->wires[1], args->wires[2], args->z, args->public_inputs,
                                 args->selectors[0], args->selectors[1], args->selectors[2], args->selectors[3],
                                 args->selectors[4], args->sigma[0], args->sigma[1], args->sigma[2]};
    std::copy(in, in + 13, qi->in);
    if (args->circuit) {
        auto it = ctx->circuits.find(args->circuit);
        if (it == ctx->circuits.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown circuit id");
        if (it->second.log_n != log_n) return fail(ctx, TYPLONK_ERR_DOMAIN, "circuit was loaded for another domain size");
        qi->cached = it->second.ext;
    }
    qi->has_pi = args->public_inputs != nullptr;
    for (int k = 0; k < (qi->cached ? 5 : 13); ++k) {
        if (k == 4 && !qi->has_pi) continue;
        if (!in[k] || in[k]->n < n) return fail(ctx, TYPLONK_ERR_RANGE, "quotient input shorter than n");
    }
    if (t_out->n < 4 * n) return fail(ctx, TYPLONK_ERR_RANGE, "t_out must hold 4n elements");
    return TYPLONK_OK;
}
// The quotient of checked inputs over ctx->quot_ext and ctx->quot_tab AS SIZED by the caller (prove_plan: quot_ext, quot_tab),
// stream-ordered.  Bit k of `extended`: ext[k] (k = 0..4: a, b, c, Z, PI) already holds that polynomial's coset evaluations
// -- the prover session extends them in rounds 1 and 2, beside the commitments
int quotient_queue(typlonk_ctx* ctx, const typlonk_quotient_args* args, uint32_t log_n, typlonk_buf* t_out, const QuotientInputs& qi,
                   uint32_t extended);
}  // namespace

int typlonk_quotient_dev(typlonk_ctx* ctx, const typlonk_quotient_args* args, uint32_t log_n, typlonk_buf* t_out) {
    if (!ctx || !args || !t_out) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    // a prover session keeps coset evaluations in the context's quotient workspace between its rounds
    if (ctx->prover_busy) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "a proof is in flight on this context");
    QuotientInputs qi;
    int rc = quotient_check(ctx, args, log_n, t_out, &qi);
    if (rc) return rc;
    const ProvePlan plan = prove_plan(log_n, 1, PROVE_SESSION, qi.cached != nullptr);
    if ((rc = ensure(ctx, ctx->quot_ext, plan.quot_ext))) return rc;
    if ((rc = ensure(ctx, ctx->quot_tab, plan.quot_tab))) return rc;
    return quotient_queue(ctx, args, log_n, t_out, qi, 0);
}

namespace {
int quotient_queue(typlonk_ctx* ctx, const typlonk_quotient_args* args, uint32_t log_n, typlonk_buf* t_out, const QuotientInputs& qi,
                   uint32_t extended) {
    const uint64_t n = 1ull << log_n, n4 = 4 * n;
    const uint32_t log4 = log_n + 2;
    const Fr* cached = qi.cached;
    const bool has_pi = qi.has_pi;
    const typlonk_buf* const* in = qi.in;
    int rc = TYPLONK_OK;
    Fr* ext = (Fr*)ctx->quot_ext.p;
    hipStream_t s = ctx->stream;
    ProfilingOff prof_off(ctx);  // stage events are per call
    const Fr ninv = fe_inv(fr_from_u64(n));
    {
        // every input that is not extended yet, as batched coset transforms (one launch per pass and group, ntt_run_batch);
        // L0 (k = 13, a constant-coefficient polynomial) is built in place
        Fr* dst[13];
        const Fr* src[13];
        size_t cnt = 0;
        for (int k = 0; k < (cached ? 5 : 13); ++k) {
            if (k == 4 && !has_pi) continue;
            if (k < 5 && ((extended >> k) & 1u)) continue;
            dst[cnt] = ext + (uint64_t)k * n4;
            src[cnt++] = in[k]->d;
        }
        if (cnt) rc = quotient_extend_batch(ctx, dst, src, cnt, n, log4);
        if (!rc && !cached) rc = quotient_extend(ctx, ext + (uint64_t)13 * n4, nullptr, &ninv, n, log4);
    }
    if (rc) {
        return rc;
    }
    QuotientArgs qa{};
    for (int k = 0; k < 3; ++k) qa.wires[k] = ext + (uint64_t)k * n4;
    qa.z = ext + 3 * n4;
    qa.pi = has_pi ? ext + 4 * n4 : nullptr;
    const Fr* cbase = cached ? cached : ext + 5 * n4;
    for (int k = 0; k < 5; ++k) qa.sel[k] = cbase + (uint64_t)k * n4;
    for (int k = 0; k < 3; ++k) qa.sigma[k] = cbase + (uint64_t)(5 + k) * n4;
    qa.l0 = cbase + 8 * n4;
    qa.out = t_out->d;
    qa.n4 = n4;
    QuotientDomain d;
    if ((rc = quotient_domain(ctx, log_n, &d))) return rc;
    qa.w_lo = d.w_lo;
    qa.w_h = d.w_h;
    memcpy(qa.beta.v, args->beta, 32);
    if (d.n_hi * sizeof(Fr) > ctx->quot_tab.cap) return fail(ctx, TYPLONK_ERR_INTERNAL, "quot_tab is smaller than the 4n domain's upper level");
    launch_fr_scale(d.w_hi, d.n_hi, fe_mul(qa.beta, d.g), (Fr*)ctx->quot_tab.p, s);   // beta * g folded into the upper level
    qa.bx_hi = (const Fr*)ctx->quot_tab.p;
    for (int k = 0; k < 4; ++k) qa.zh_inv[k] = d.zh_inv[k];
    memcpy(qa.alpha.v, args->alpha, 32);
    memcpy(qa.gamma.v, args->gamma, 32);
    qa.alpha2 = fe_sqr(qa.alpha);
    for (int k = 0; k < 3; ++k) memcpy(qa.k[k].v, args->cosets[k], 32);
    qa.k0_is_one = qa.k[0] == Fr::one();
    launch_quotient_pointwise(qa, s);
    HIPCHK(hipGetLastError());
    rc = ntt_run(ctx, t_out->d, log4, 1, d.g_limbs, /*sync=*/false);
    return rc;
}
}  // namespace

int typlonk_grand_product_dev(typlonk_ctx* ctx, const typlonk_buf* const wires[3], const typlonk_buf* const sigma[3],
                              const uint64_t beta[4], const uint64_t gamma[4], const uint64_t cosets[3][4],
                              uint32_t log_n, typlonk_buf* z_evals_out) {
    if (!ctx || !wires || !sigma || !beta || !gamma || !cosets || !z_evals_out)
        return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    if (log_n > TYPLONK_MAX_PROVER_LOG_N) return fail(ctx, TYPLONK_ERR_DOMAIN, "grand product needs log_n <= 24");
    HIPCHK(hipSetDevice(ctx->device));
    const uint64_t n = 1ull << log_n;
    for (int i = 0; i < 3; ++i)
        if (!wires[i] || !sigma[i] || wires[i]->n < n || sigma[i]->n < n)
            return fail(ctx, TYPLONK_ERR_RANGE, "grand product input shorter than n");
    if (z_evals_out->n < n) return fail(ctx, TYPLONK_ERR_RANGE, "z_evals_out shorter than n");
    const GpScratch L = gp_scratch(n);
    int rc = ensure(ctx, ctx->ops_tmp, L.end * sizeof(Fr));   // (inside a session: sized in round 1, nothing to grow)
    if (rc) return rc;
    Fr* const base = (Fr*)ctx->ops_tmp.p;
    Fr *num = base + L.num, *den = base + L.den, *npre = base + L.npre, *dsuf = base + L.dsuf, *blk = base + L.carries;
    hipStream_t s = ctx->stream;
    GrandProductArgs a{};
    for (int i = 0; i < 3; ++i) {
        a.wires[i] = wires[i]->d;
        a.sigma[i] = sigma[i]->d;
    }
    a.num = num;
    a.den = den;
    a.n = n;
    memcpy(a.beta.v, beta, 32);
    memcpy(a.gamma.v, gamma, 32);
    for (int i = 0; i < 3; ++i) {
        Fr k;
        memcpy(k.v, cosets[i], 32);
        a.kbeta[i] = fe_mul(k, a.beta);
    }
    rc = domain_twiddles(ctx, std::max<uint32_t>(log_n, 1), &a.w_lo, &a.w_hi, &a.w_h);  // a two-level table needs at least one bit
    if (rc) return rc;
    launch_gp_terms(a, s);
    launch_product_scan(num, n, 0, blk, npre, s);
    launch_product_scan(den, n, 1, blk, dsuf, s);
    HIPCHK(hipGetLastError());
    // S_0 = dsuf[0] = the product of all denominators: inverted ON THE DEVICE (fr_inv.hpp) into the slot behind the carries
    // -- no copy, no wait, no host inversion between the scans and the finish (rounds 1-5 drained the stream here)
    Fr* inv_total = base + L.inv;
    launch_fr_inv(dsuf, inv_total, s);
    launch_gp_finish(npre, dsuf, inv_total, n, z_evals_out->d, s);
    HIPCHK(hipGetLastError());
    return TYPLONK_OK;
}

int typlonk_open_dev(typlonk_ctx* ctx, const typlonk_buf* poly, size_t offset, size_t m, const uint64_t z[4],
                     typlonk_buf* q_out, uint64_t y_out[4]) {
    if (!ctx || !poly || !z || !y_out) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    if (m < 1) return fail(ctx, TYPLONK_ERR_LENGTH, "open needs at least 1 coefficient (kzg/src/lib.rs:58)");
    if (m > ((size_t)1 << (TYPLONK_MAX_PROVER_LOG_N + 1))) return fail(ctx, TYPLONK_ERR_LENGTH, "open supports up to 2^25 coefficients");
    if (offset > poly->n || m > poly->n - offset) return fail(ctx, TYPLONK_ERR_RANGE, "range outside buffer");
    if (q_out && q_out->n < m - 1) return fail(ctx, TYPLONK_ERR_RANGE, "q_out shorter than m - 1");
    if (q_out && q_out->d == poly->d) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "q_out must not alias poly");
    HIPCHK(hipSetDevice(ctx->device));
    const OpenDevScratch L = open_dev_scratch(m);   // one carry per 2048-coefficient workgroup, then the result
    int rc = ensure(ctx, ctx->ops_tmp, L.end * sizeof(Fr));
    if (rc) return rc;
    Fr* blocks = (Fr*)ctx->ops_tmp.p + L.carries;
    Fr* y_dev = (Fr*)ctx->ops_tmp.p + L.y;
    Fr zz;
    memcpy(zz.v, z, 32);
    launch_open(poly->d + offset, m, zz, q_out ? q_out->d : nullptr, blocks, y_dev, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(y_out, y_dev, sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return TYPLONK_OK;
}

int typlonk_lincomb_dev(typlonk_ctx* ctx, const typlonk_buf* const* polys, const uint64_t (*scalars)[4], size_t terms,
                        const uint64_t* constant, size_t n, typlonk_buf* out) {
    if (!ctx || !out || (terms && (!polys || !scalars))) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    if (terms > 12) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "at most 12 terms");
    if (out->n < n) return fail(ctx, TYPLONK_ERR_RANGE, "out shorter than n");
    HIPCHK(hipSetDevice(ctx->device));
    LincombArgs a{};
    for (size_t k = 0; k < terms; ++k) {
        if (!polys[k] || polys[k]->n < n) return fail(ctx, TYPLONK_ERR_RANGE, "term shorter than n");
        if (polys[k]->d == out->d) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "out must not alias a term");
        a.poly[k] = polys[k]->d;
        memcpy(a.scalar[k].v, scalars[k], 32);
    }
    a.constant = Fr::zero();
    if (constant) memcpy(a.constant.v, constant, 32);
    a.out = out->d;
    a.n = n;
    a.terms = (uint32_t)terms;
    if (n) launch_lincomb(a, ctx->stream);
    HIPCHK(hipGetLastError());
    return TYPLONK_OK;
}

// ================================================================================================
// The prover's device-side flow: plonk::proof::prove (/root/reference/plonk/src/proof.rs:26-57, 96-194)
// as three rounds around the two Fiat-Shamir squeezes.  Every polynomial stays in HBM from the
// witness upload to the last commitment; the host only handles the few scalars of the linearisation.
struct typlonk_prover {
    typlonk_ctx* ctx = nullptr;
    uint32_t srs_id = 0, circuit = 0, log_n = 0;
    uint64_t n = 0;
    ProveArena mem;     // the proof's arena in ctx->prover_mem (regions and the roles of q: prove_plan.hpp)
    Fr* at(ProveRegion r, uint64_t i = 0) const { return mem.at(0, r, i); }
    Fr beta, gamma, k[3];
    bool has_pi = true;
    int round = 0;
    uint32_t extended = 0;  // bit k: coset evaluations of a, b, c, Z, PI already sit in the quotient workspace
    // batched-opening flow (round3_evals / round4_batched)
    bool evals_only = false;
    Fr zeta;
};

namespace {
int prover_commit_batch(typlonk_prover* p, const Fr* const* polys, const size_t* m, size_t count, uint64_t* xy, uint8_t* inf) {
    std::vector<const void*> ptrs(count);
    for (size_t i = 0; i < count; ++i) ptrs[i] = polys[i];
    return msm_batch(p->ctx, p->srs_id, ptrs.data(), m, count, xy, inf);
}
// Coset evaluations of one per-proof quotient input (k = 0..4: a, b, c, Z, PI), queued on the context's stream as soon
// as its coefficients exist.  Rounds 1 and 2 commit on the other lanes at that time, so these transforms fill the
// latency-bound stretches of the MSMs (sort, bucket reduction) instead of sitting on round 3's critical path.
int prover_extend(typlonk_prover* p, int k, const Fr* coeffs) {
    typlonk_ctx* ctx = p->ctx;
    const Fr ninv = Fr::one();  // unused: src is never null here
    const int rc = quotient_extend(ctx, (Fr*)ctx->quot_ext.p + (uint64_t)k * 4 * p->n, coeffs, &ninv, p->n, p->log_n + 2);
    if (!rc) p->extended |= 1u << k;
    return rc;
}
// Scratch of the prover's openings: the carries in ops_tmp (session_open_carries) and the result slots, both sized in round 1.
// The slots are only ever WRITTEN by kernels (p(z) of an opening) and read by the host, so they live in pinned host memory the
// kernels store into directly: a fetch is one stream synchronisation, no copy.  (Device slots + hipMemcpyAsync into a stack
// array -- pageable, so staged by the runtime -- left the GPU idle for ~170 us before the linearisation and ~120 us before
// round 3's commitments, profiles/r06_prove_timeline.txt 15.50-15.67 and 15.89-16.02 ms.)
// open() without waiting: p(z) lands in result slot `slot`, the quotient (if q) in q; stream-ordered
int prover_open_async(typlonk_prover* p, const Fr* poly, uint64_t m, const Fr& z, Fr* q, int slot) {
    typlonk_ctx* ctx = p->ctx;
    launch_open(poly, m, z, q, (Fr*)ctx->ops_tmp.p, ctx->eval_slots_host + slot, ctx->stream);
    HIPCHK(hipGetLastError());
    return TYPLONK_OK;
}
// one synchronisation for the `count` result slots from `first` on
int prover_fetch(typlonk_prover* p, Fr* out, int first, int count) {
    typlonk_ctx* ctx = p->ctx;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    memcpy((void*)out, (const void*)(ctx->eval_slots_host + first), (size_t)count * sizeof(Fr));
    return TYPLONK_OK;
}
// round 3's openings and evaluations (round3_openings) at ze and zw = ze * w in three launches, the results into `slots`' places
int prover_open_round3(typlonk_prover* p, const CircuitEntry& ce, const Round3Slots& slots, bool with_quotients, const Fr& ze,
                       const Fr& zw) {
    const Fr* polys[PB_ITEMS];
    Fr* quots[PB_ITEMS];
    Fr* ys[PB_ITEMS];
    uint8_t zsel[PB_ITEMS];
    uint32_t cnt = 0;
    const Round3Polys in{p->at(PR_CO), p->at(PR_Z), p->has_pi ? p->at(PR_PI) : nullptr, p->at(PR_Q), ce.coef, p->n};
    round3_openings(slots, with_quotients, in, [&](const Fr* poly, Fr* quot, int slot, uint8_t point) {
        polys[cnt] = poly;
        quots[cnt] = quot;
        ys[cnt] = p->ctx->eval_slots_host + slot;
        zsel[cnt++] = point;
    });
    launch_open_multi(polys, quots, ys, zsel, cnt, p->n, ze, zw, (Fr*)p->ctx->ops_tmp.p, p->ctx->stream);
    return hip_rc(p->ctx, hipGetLastError());
}
// r = sum_k scalar[k] * lin_polys[k] + constant into the arena's r, stream-ordered
int prover_linearise(typlonk_prover* p, const CircuitEntry& ce, const Fr* scalar /* LIN_TERMS */, const Fr& constant) {
    LincombArgs la{};
    lin_polys(ce.coef, p->at(PR_Z), p->at(PR_T), p->n, la.poly);
    for (int k = 0; k < LIN_TERMS; ++k) la.scalar[k] = scalar[k];
    la.constant = constant;
    la.terms = LIN_TERMS;
    la.out = p->at(PR_R);
    la.n = p->n;
    launch_lincomb(la, p->ctx->stream);
    return hip_rc(p->ctx, hipGetLastError());
}
// typlonk_prover_round1, typlonk_prove and typlonk_prove_compact answer a null wire HANDLE with TYPLONK_ERR_RANGE, as a column
// of no rows (the other entry points: admit_columns' TYPLONK_ERR_INVALID_ARG); a null host column they refuse first of all
int null_handle_is_short(typlonk_ctx* ctx, const ColumnsOf& in) {
    for (int i = 0; i < 3 && in.bufs; ++i)
        if (!in.bufs[i]) return fail(ctx, TYPLONK_ERR_RANGE, "wire column shorter than n");
    return TYPLONK_OK;
}
int null_host_column(typlonk_ctx* ctx, const uint64_t* const wire_evals[3]) {
    for (int i = 0; i < 3; ++i)
        if (!wire_evals[i]) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null wire column");
    return TYPLONK_OK;
}
// wires, pi_src: n evaluations each on the device (a typlonk_buf) or still on the HOST (typlonk_prove_host: the reference's
// prove() holds its padded, blinded columns as Vec<Fr>, plonk/src/proof.rs:43-49); pi_src may be absent
int prover_round1_impl(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const ColumnSrc (&wires)[3], const ColumnSrc& pi_src,
                       typlonk_prover** out, uint64_t commit_xy[3][12], uint8_t commit_inf[3]) {
    HIPCHK(hipSetDevice(ctx->device));
    auto ci = ctx->circuits.find(circuit_id);
    if (ci == ctx->circuits.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown circuit id");
    const SrsEntry* srs = nullptr;
    const uint32_t log_n = ci->second.log_n;
    const uint64_t n = 1ull << log_n;
    int rc = msm_validate(ctx, srs_id, n, &srs);  // every committed polynomial has <= n coefficients
    if (rc) return rc;
    if (log_n > TYPLONK_MAX_PROVER_LOG_N) return fail(ctx, TYPLONK_ERR_LENGTH, "prover supports up to 2^24 rows");
    if (ctx->prover_busy) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "a proof is already in flight on this context");
    // everything the three (four) rounds touch, sized before anything is queued; kept across proofs
    const ProvePlan plan = prove_plan(log_n, 1, PROVE_SESSION, /*cached=*/true);
    if ((rc = prover_workspaces(ctx, plan))) return rc;
    typlonk_prover* p = new typlonk_prover();
    p->ctx = ctx;
    p->srs_id = srs_id;
    p->circuit = circuit_id;
    p->log_n = log_n;
    p->n = n;
    p->mem = ProveArena{(Fr*)ctx->prover_mem.p, n, plan.stride};
    hipStream_t s = ctx->stream;
    ProfilingOff prof_off(ctx);  // stage events are per call
    ProverRound in_round(ctx);
    // a, b, c = interpolate(columns) (proof.rs:50); the column values themselves are kept for round 2
    // (proof.rs:113-115 recomputes them with three forward FFTs).  Each commitment (round1, proof.rs:107-110) is
    // submitted to its own lane as soon as its polynomial exists, so the next interpolation and the coset transforms
    // of the quotient inputs run while it is being sorted and accumulated.  (Batched transforms, ntt_run_batch, LOSE
    // 0.3-0.5 ms per 2^20 proof here: they delay a commitment's start by the other columns' transforms, which were already
    // hidden beside the commitments' sorts, profiles/r06_ab_prover_ntt_batch.txt.)
    // Each column goes into its place (column_to_device: device -> device, or host -> device on the context's stream) right
    // before that column's transform and commitment are queued, so column i + 1 crosses PCIe while column i is being
    // transformed, sorted and accumulated
    MsmQueue q(ctx, srs, /*first_lane=*/1);
    p->has_pi = pi_src.present();  // absent: public inputs [0] -> the zero polynomial
    for (int i = 0; i < 3 && !rc; ++i) {
        if ((rc = hip_rc(ctx, column_to_device(p->at(PR_EV, i), wires[i], n, s)))) break;
        if ((rc = hip_rc(ctx, hipMemcpyAsync(p->at(PR_CO, i), p->at(PR_EV, i), n * sizeof(Fr), hipMemcpyDeviceToDevice, s)))) break;
        if ((rc = ntt_run(ctx, p->at(PR_CO, i), log_n, 1, nullptr, false))) break;
        rc = q.submit(p->at(PR_CO, i), n, commit_xy[i], commit_inf + i);
    }
    if (!rc && p->has_pi) {
        rc = hip_rc(ctx, column_to_device(p->at(PR_PI), pi_src, n, s));
        if (!rc) rc = ntt_run(ctx, p->at(PR_PI), log_n, 1, nullptr, false);  // proof.rs:105-106
    }
    // the coset transforms of the quotient's per-proof inputs run beside the commitments (measured: -1 % per proof;
    // submitting round 3's first opening MSMs before the quotient loses 1 %: profiles/r02_ab_prover_overlap.txt)
    for (int i = 0; i < 3 && !rc; ++i) rc = prover_extend(p, i, p->at(PR_CO, i));
    if (!rc && p->has_pi) rc = prover_extend(p, 4, p->at(PR_PI));
    {
        const int r = q.wait_all();
        if (!rc) rc = r;
    }
    if (rc) {
        delete p;
        return rc;
    }
    p->round = 1;
    ctx->prover_busy = true;
    *out = p;
    return TYPLONK_OK;
}

// round 1 of one proof from the caller's columns (the reference shape's rule for the public inputs)
int prover_round1_from(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const ColumnsOf& in, typlonk_prover** out,
                       uint64_t commit_xy[3][12], uint8_t commit_inf[3]) {
    auto ci = ctx->circuits.find(circuit_id);
    if (ci == ctx->circuits.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown circuit id");
    const uint64_t n = 1ull << ci->second.log_n;
    int rc = null_handle_is_short(ctx, in);
    if (!rc) rc = admit_columns(ctx, in, n);
    if (rc) return rc;
    const ColumnSrc w[3] = {in.column(0, 0, n), in.column(0, 1, n), in.column(0, 2, n)};
    return prover_round1_impl(ctx, srs_id, circuit_id, w, in.pi(0, n), out, commit_xy, commit_inf);
}
}  // namespace

int typlonk_prover_round1(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const typlonk_buf* const wire_evals[3],
                          const typlonk_buf* pi_evals, typlonk_prover** out, uint64_t commit_xy[3][12],
                          uint8_t commit_inf[3]) {
    if (!ctx || !wire_evals || !out || !commit_xy || !commit_inf) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    return prover_round1_from(ctx, srs_id, circuit_id, ColumnsOf(wire_evals, 1, ColumnsOf::PI_FULL, &pi_evals), out, commit_xy,
                              commit_inf);
}

int typlonk_prover_round2(typlonk_prover* p, const uint64_t beta[4], const uint64_t gamma[4], const uint64_t cosets[3][4],
                          uint64_t z_xy[12], uint8_t* z_inf) {
    if (!p || !beta || !gamma || !cosets || !z_xy || !z_inf) return TYPLONK_ERR_INVALID_ARG;
    typlonk_ctx* ctx = p->ctx;
    if (p->round != 1) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "round2 must follow round1");
    HIPCHK(hipSetDevice(ctx->device));
    auto cit = ctx->circuits.find(p->circuit);
    if (cit == ctx->circuits.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "circuit was freed during the proof");
    const CircuitEntry& ce = cit->second;
    const uint64_t n = p->n;
    memcpy(p->beta.v, beta, 32);
    memcpy(p->gamma.v, gamma, 32);
    for (int i = 0; i < 3; ++i) memcpy(p->k[i].v, cosets[i], 32);
    typlonk_buf wb[3] = {{p->at(PR_EV, 0), n}, {p->at(PR_EV, 1), n}, {p->at(PR_EV, 2), n}};
    typlonk_buf sb[3] = {{ce.sig_ev, n}, {ce.sig_ev + n, n}, {ce.sig_ev + 2 * n, n}};
    const typlonk_buf* wp[3] = {&wb[0], &wb[1], &wb[2]};
    const typlonk_buf* sp[3] = {&sb[0], &sb[1], &sb[2]};
    typlonk_buf zb{p->at(PR_Z), n};
    ProfilingOff prof_off(ctx);  // stage events are per call
    ProverRound in_round(ctx);
    int rc = typlonk_grand_product_dev(ctx, wp, sp, beta, gamma, cosets, p->log_n, &zb);  // proof.rs:119-120
    if (!rc) rc = ntt_run(ctx, p->at(PR_Z), p->log_n, 1, nullptr, false);                          // :127-128
    if (!rc) {
        const SrsEntry* srs = nullptr;
        rc = msm_validate(ctx, p->srs_id, n, &srs);
        if (!rc) {
            MsmQueue q(ctx, srs, /*first_lane=*/1);
            rc = q.submit(p->at(PR_Z), n, z_xy, z_inf, /*standalone=*/true);                       // :129
            if (!rc) rc = prover_extend(p, 3, p->at(PR_Z));  // Z's coset transform runs beside its commitment
            const int r = q.wait_all();
            if (!rc) rc = r;
        }
    }
    if (!rc) p->round = 2;
    return rc;
}

namespace {
// The quotient t (proof.rs:139-145) into the arena's t, stream-ordered.  a, b, c, Z (and PI) were transformed to the coset domain in
// rounds 1 and 2 (p->extended), so what is left is the pointwise kernel and one inverse transform.
int prover_quotient(typlonk_prover* p, const Fr& alpha) {
    const uint64_t n = p->n;
    typlonk_buf b[5] = {{p->at(PR_CO, 0), n}, {p->at(PR_CO, 1), n}, {p->at(PR_CO, 2), n}, {p->at(PR_Z), n}, {p->at(PR_PI), n}};
    typlonk_buf tb{p->at(PR_T), 4 * n};
    typlonk_quotient_args qa{};
    for (int i = 0; i < 3; ++i) qa.wires[i] = &b[i];
    qa.z = &b[3];
    qa.public_inputs = p->has_pi ? &b[4] : nullptr;
    memcpy(qa.alpha, alpha.v, 32);
    memcpy(qa.beta, p->beta.v, 32);
    memcpy(qa.gamma, p->gamma.v, 32);
    for (int i = 0; i < 3; ++i) memcpy(qa.cosets[i], p->k[i].v, 32);
    qa.circuit = p->circuit;
    // The session built every buffer itself, so the check is not here because these inputs can fail: it resolves the circuit's
    // cached evaluations, and it is kept whole so that this step refuses what it always refused, in the same order.
    QuotientInputs qi;
    if (const int rc = quotient_check(p->ctx, &qa, p->log_n, &tb, &qi)) return rc;
    return quotient_queue(p->ctx, &qa, p->log_n, &tb, qi, p->extended);   // (quot_ext, quot_tab: sized in round 1)
}

// Round 3 in both shapes.  tail != NULL: the reference's six separate openings (proof.rs:147-175).
// evals != NULL: evaluations only -- the quotients (p - p(zeta)) / (X - zeta) are not formed here; after
// the caller has squeezed v from the evaluations, round4_batched opens a + v b + v^2 c + v^3 Z + v^4 r once.
int prover_round3_core(typlonk_prover* p, const uint64_t alpha[4], const uint64_t zeta[4], typlonk_proof_tail* out,
                       typlonk_proof_evals* evals_out) {
    const bool batched = evals_out != nullptr;
    typlonk_ctx* ctx = p->ctx;
    if (p->round != 2) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "round3 must follow round2");
    HIPCHK(hipSetDevice(ctx->device));
    auto cit = ctx->circuits.find(p->circuit);
    if (cit == ctx->circuits.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "circuit was freed during the proof");
    const CircuitEntry& ce = cit->second;
    const uint64_t n = p->n;
    const uint32_t log_n = p->log_n;
    Fr al, ze;
    memcpy(al.v, alpha, 32);
    memcpy(ze.v, zeta, 32);
    ProfilingOff prof_off(ctx);  // stage events are per call
    ProverRound in_round(ctx);
    const SrsEntry* srs = nullptr;
    int rc = msm_validate(ctx, p->srs_id, n, &srs);
    if (rc) return rc;
    // commitments of this round: 6 opening witnesses + 3 quotient slices (:181).  The queue outlives every early
    // return (its destructor-side wait below), because the MSMs write into xy / inf.
    uint64_t xy[9][12];
    uint8_t inf[9];
    MsmQueue q(ctx, srs, /*first_lane=*/1);
    WaitAll wait_guard{q};
    // ---- openings of a, b, c at zeta; Z at zeta and zeta*w (proof.rs:147-163) ----
    Fr ev[6];
    const Fr w = fr_domain_root(log_n);
    const Fr zw = fe_mul(ze, w);
    Fr s0, s1, pi_z = Fr::zero();
    const Fr one = Fr::one();
    Fr zn = ze, zh = one, l0z = one;   // zeta^n, Z_H(zeta), L0(zeta): filled under the kernels, before the wait
    constexpr Round3Slots S = REF_SLOTS;
    {
        // ONE synchronisation for everything evaluated here (REF_SLOTS): a, b, c, Z at zeta (with their quotients unless
        // batched), sigma_0, sigma_1 and the public-input polynomial at zeta (for the linearisation, proof.rs:376-439, :138),
        // Z at zeta*w (always with its quotient) -- all of them in three launches (launch_open_multi)
        Fr host[S.count];
        rc = prover_open_round3(p, ce, S, /*with_quotients=*/!batched, ze, zw);
        // ---- quotient (proof.rs:139-145): queued behind the opening scans ----
        if (!rc) rc = prover_quotient(p, al);
        // what the linearisation needs of zeta alone (one host inversion among it): while the kernels above run
        lin_zeta_terms(ze, log_n, &zn, &zh, &l0z);
        if (!rc) rc = prover_fetch(p, host, 0, S.count);
        for (int i = 0; i < 3; ++i) ev[i] = host[S.wire + i];
        ev[3] = host[S.z];
        ev[4] = host[S.zw];
        s0 = host[S.sig0];
        s1 = host[S.sig1];
        if (p->has_pi) pi_z = host[S.pi];
    }
    if (!rc) {
        Fr scalar[LIN_TERMS], constant;
        lin_scalars(ev, s0, s1, pi_z, p->beta, p->gamma, p->k, al, ze, zn, zh, l0z, scalar, &constant);
        rc = prover_linearise(p, ce, scalar, constant);
    }
    // r(zeta) and its witness polynomial (proof.rs:175).  The reference shape does not wait for the value here: it is an
    // OUTPUT (and the r(zeta) != 0 check), nothing of this round's commitments depends on it -- it is read from its pinned slot
    // once the commitments have been waited for, and the first sort starts without a drain of the context's stream in between.
    if (!rc) rc = prover_open_async(p, p->at(PR_R), n, ze, batched ? nullptr : p->at(PR_Q, Q_WIT_R), S.r);
    if (!rc && batched) rc = prover_fetch(p, &ev[5], S.r, 1);
    if (!rc && batched) {
        // evaluations only: every commitment of this shape is issued by round4_batched in ONE five-MSM batch
        for (int i = 0; i < 6; ++i) memcpy(evals_out->evals[i], ev[i].v, 32);
        p->zeta = ze;
        p->evals_only = true;
    }
    // ---- the nine remaining commitments in one batch: 6 opening witnesses + 3 quotient slices (:181) ----
    if (!rc && !batched) {
        // (the six witnesses in q's order, Q_WIT_A .. Q_WIT_R, as the proof lists them: prove_plan.hpp asserts the order)
        const Fr* polys[9] = {p->at(PR_Q, 0), p->at(PR_Q, 1), p->at(PR_Q, 2), p->at(PR_Q, 3), p->at(PR_Q, 4), p->at(PR_Q, 5),
                              p->at(PR_T), p->at(PR_T, 1), p->at(PR_T, 2)};
        const size_t m[9] = {n - 1, n - 1, n - 1, n - 1, n - 1, n - 1, n, n, n > 3 ? n - 3 : 0};
        q.set_first_lane(0);  // the context's stream has nothing left to do but commit
        // All nine polynomials exist once what is queued on the context's stream NOW has run: the lanes wait for this
        // mark, not for "everything on the context's stream at submit time" -- which, with the context's stream itself a
        // lane, included the whole MSM submitted to it just before.  (Rounds 1-4: commitments 4 and 5 started their sorts
        // only when commitment 3 had finished, and 7 and 8 after 6: two stretches of 1.2 ms with no accumulation in
        // flight, profiles/r04_prove_timeline.txt 23.1-24.4 and 30.6-31.9 ms.)
        if (!ctx->batch_fence) HIPCHK(hipEventCreateWithFlags(&ctx->batch_fence, hipEventDisableTiming));
        HIPCHK(hipEventRecord(ctx->batch_fence, ctx->stream));
        q.fence = ctx->batch_fence;
        for (int k = 0; k < 9 && !rc; ++k) rc = q.submit(polys[k], m[k], xy[k], inf + k);
        {
            const int r = q.wait_all();
            if (!rc) rc = r;
        }
        if (!rc) rc = prover_fetch(p, &ev[5], S.r, 1);   // (every lane has been waited for: this returns at once)
        if (!rc) {
            memcpy(out->w_xy, xy, 6 * 96);
            memcpy(out->w_inf, inf, 6);
            memcpy(out->t_xy, xy[6], 3 * 96);
            memcpy(out->t_inf, inf + 6, 3);
            for (int i = 0; i < 6; ++i) memcpy(out->evals[i], ev[i].v, 32);
        }
    }
    if (!rc) {
        p->round = 3;
        // the verifier's check (proof.rs:234-235).  A witness that violates a gate makes the reference panic in
        // vanishes() (:321, :361); here the division by Z_H leaves a remainder the slices drop, and r(zeta) != 0
        // is how that shows.  Everything in `out` is filled; the caller learns the proof cannot verify.
        if (!ev[5].is_zero())
            return fail(ctx, TYPLONK_ERR_UNSATISFIED, "r(zeta) != 0: the witness does not satisfy the circuit (proof.rs:234-235)");
    }
    return rc;
}
}  // namespace

namespace tyh {
void lin_zeta_terms(const Fr& zeta, uint32_t log_n, Fr* zn, Fr* zh, Fr* l0z) {
    const Fr one = Fr::one();
    Fr x = zeta;
    for (uint32_t i = 0; i < log_n; ++i) x = fe_sqr(x);
    *zn = x;
    *zh = fe_sub(x, one);  // evaluate_vanishing_polynomial(zeta)
    // L0(zeta) = (zeta^n - 1) / (n (zeta - 1)); the polynomial (1/n) sum X^i evaluates to 1 at zeta = 1
    *l0z = one;
    const Fr zm1 = fe_sub(zeta, one);
    if (!zm1.is_zero()) *l0z = fe_mul(*zh, fe_inv(fe_mul(fr_from_u64(1ull << log_n), zm1)));
}
void lin_scalars(const Fr* ev, const Fr& s0, const Fr& s1, const Fr& pi_z, const Fr& beta, const Fr& gamma, const Fr (&k)[3],
                 const Fr& al, const Fr& zeta, const Fr& zn, const Fr& zh, const Fr& l0z, Fr* sc, Fr* constant) {
    const Fr one = Fr::one();
    const Fr &a = ev[0], &b = ev[1], &c = ev[2], &zwe = ev[4];
    const Fr bz = fe_mul(beta, zeta);
    Fr l2 = one;  // prod_i (w_i(zeta) + k_i beta zeta + gamma)
    for (int i = 0; i < 3; ++i) l2 = fe_mul(l2, fe_add(fe_add(ev[i], fe_mul(k[i], bz)), gamma));
    const Fr ab = fe_mul(fe_add(fe_add(a, fe_mul(beta, s0)), gamma), fe_add(fe_add(b, fe_mul(beta, s1)), gamma));
    const Fr abz = fe_mul(ab, zwe);          // copy_permutation_ab * Z(zeta w)
    const Fr al2 = fe_sqr(al);
    sc[0] = a;                                            // q_l a
    sc[1] = b;                                            // q_r b
    sc[2] = fe_neg(c);                                    // - q_o c
    sc[3] = fe_mul(a, b);                                 // q_m a b
    sc[4] = one;                                          // q_c
    sc[5] = fe_add(fe_mul(al, l2), fe_mul(al2, l0z));     // Z (alpha line2 + alpha^2 L0)
    sc[6] = fe_neg(fe_mul(al, fe_mul(beta, abz)));        // - alpha beta sigma_2 AB Z(zw)
    sc[7] = fe_neg(zh);                                   // - Z_H t_lo
    sc[8] = fe_neg(fe_mul(zh, zn));                       // - Z_H zeta^n t_mid
    sc[9] = fe_neg(fe_mul(zh, fe_sqr(zn)));               // - Z_H zeta^2n t_hi
    // constant: PI(zeta) - alpha (gamma + c) AB Z(zw) - alpha^2 L0
    *constant = fe_sub(fe_sub(pi_z, fe_mul(al, fe_mul(fe_add(gamma, c), abz))), fe_mul(al2, l0z));
}
}  // namespace tyh

int typlonk_prover_round3(typlonk_prover* p, const uint64_t alpha[4], const uint64_t zeta[4], typlonk_proof_tail* out) {
    if (!p || !alpha || !zeta || !out) return TYPLONK_ERR_INVALID_ARG;
    return prover_round3_core(p, alpha, zeta, out, nullptr);
}

int typlonk_prover_round3_evals(typlonk_prover* p, const uint64_t alpha[4], const uint64_t zeta[4],
                                typlonk_proof_evals* out) {
    if (!p || !alpha || !zeta || !out) return TYPLONK_ERR_INVALID_ARG;
    return prover_round3_core(p, alpha, zeta, nullptr, out);
}

int typlonk_prover_round4_batched(typlonk_prover* p, const uint64_t v[4], typlonk_proof_batched* out) {
    if (!p || !v || !out) return TYPLONK_ERR_INVALID_ARG;
    typlonk_ctx* ctx = p->ctx;
    if (p->round != 3 || !p->evals_only) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "round4_batched must follow round3_evals");
    HIPCHK(hipSetDevice(ctx->device));
    const uint64_t n = p->n;
    ProfilingOff prof_off(ctx);  // stage events are per call
    ProverRound in_round(ctx);
    // F = a + v b + v^2 c + v^3 Z + v^4 r; division by (X - zeta) is linear, so its witness is
    // sum_i v^i W_i of the six-opening proof
    LincombArgs la{};
    const Fr* polys[5] = {p->at(PR_CO, 0), p->at(PR_CO, 1), p->at(PR_CO, 2), p->at(PR_Z), p->at(PR_R)};
    Fr vv, pw = Fr::one();
    memcpy(vv.v, v, 32);
    for (int i = 0; i < 5; ++i) {
        la.poly[i] = polys[i];
        la.scalar[i] = pw;
        pw = fe_mul(pw, vv);
    }
    la.terms = 5;
    la.constant = Fr::zero();
    la.out = p->at(PR_Q, Q_BATCHED_F);
    la.n = n;
    launch_lincomb(la, ctx->stream);
    int rc = hip_rc(ctx, hipGetLastError());
    // (F(zeta) itself is not needed: stream-ordered)
    if (!rc) rc = prover_open_async(p, p->at(PR_Q, Q_BATCHED_F), n, p->zeta, p->at(PR_Q, Q_BATCHED_WIT), REF_SLOTS.f);
    if (!rc) {
        // one batch: [t_lo], [t_mid], [t_hi] (proof.rs:181), the witness of Z at zeta*w, the batched witness at zeta
        const Fr* ms[5] = {p->at(PR_T), p->at(PR_T, 1), p->at(PR_T, 2), p->at(PR_Q, Q_WIT_ZW), p->at(PR_Q, Q_BATCHED_WIT)};
        const size_t m[5] = {n, n, n > 3 ? n - 3 : 0, n - 1, n - 1};
        uint64_t xy[5][12];
        uint8_t inf[5];
        rc = prover_commit_batch(p, ms, m, 5, &xy[0][0], inf);
        if (!rc) {
            memcpy(out->t_xy, xy, 3 * 96);
            memcpy(out->t_inf, inf, 3);
            memcpy(out->w_xy[1], xy[3], 96);
            out->w_inf[1] = inf[3];
            memcpy(out->w_xy[0], xy[4], 96);
            out->w_inf[0] = inf[4];
            p->round = 4;
        }
    }
    return rc;
}

int typlonk_transcript_challenges(const uint64_t* xy, const uint8_t* inf, size_t count, size_t n_challenges, uint64_t* out) {
    if ((!xy && count) || (!out && n_challenges)) return TYPLONK_ERR_INVALID_ARG;
    ChallengeGenerator g;
    for (size_t i = 0; i < count; ++i) g.digest(xy + 12 * i, inf ? inf[i] : 0);
    g.generate(n_challenges, out);
    return TYPLONK_OK;
}

namespace {
int prove_impl(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const ColumnsOf& in, const uint64_t cosets[3][4],
               typlonk_proof* out) {
    typlonk_prover* p = nullptr;
    // An SRS shard on a context with a communicator: every round's partial commitments are folded over the ranks (one
    // all-gather per round), so all ranks hash the same points and end with the same proof.  A rank whose round fails
    // (an OOM, say) still joins that round's collective with flagged records, so its peers return TYPLONK_ERR_COMM
    // instead of waiting for ever (comm_fold).
    const bool folds = comm_folds(ctx, srs_id);
    // (columns on the host: each is uploaded right before its transform and commitment are queued)
    int rc = prover_round1_from(ctx, srs_id, circuit_id, in, &p, out->commit_xy, out->commit_inf);
    if (folds) rc = comm_fold(ctx, &out->commit_xy[0][0], out->commit_inf, 3, rc);
    if (rc) {
        if (p) typlonk_prover_free(p);
        return rc;
    }
    RefScript script;   // the challenges of this shape, in its order (proof_script.hpp)
    script.after_round1(*out);
    rc = typlonk_prover_round2(p, out->beta, out->gamma, cosets, out->z_xy, &out->z_inf);
    if (folds) rc = comm_fold(ctx, out->z_xy, &out->z_inf, 1, rc);
    if (!rc) {
        script.after_round2(*out);
        rc = typlonk_prover_round3(p, out->alpha, out->zeta, &out->tail);
        if (folds) {   // (an unsatisfied witness, r(zeta) != 0, is the same on every rank: the points are still folded)
            const int round_rc = rc;
            uint64_t xy[9][12];
            uint8_t inf[9];
            memcpy(xy, out->tail.t_xy, 3 * 96);
            memcpy(xy + 3, out->tail.w_xy, 6 * 96);
            memcpy(inf, out->tail.t_inf, 3);
            memcpy(inf + 3, out->tail.w_inf, 6);
            const int r2 = comm_fold(ctx, &xy[0][0], inf, 9, round_rc == TYPLONK_ERR_UNSATISFIED ? TYPLONK_OK : round_rc);
            memcpy(out->tail.t_xy, xy, 3 * 96);
            memcpy(out->tail.w_xy, xy + 3, 6 * 96);
            memcpy(out->tail.t_inf, inf, 3);
            memcpy(out->tail.w_inf, inf + 3, 6);
            if (r2) rc = r2;
            else rc = round_rc;
        }
    }
    typlonk_prover_free(p);
    return rc;
}
}  // namespace

int typlonk_prove(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const typlonk_buf* const wire_evals[3],
                  const typlonk_buf* pi_evals, const uint64_t cosets[3][4], typlonk_proof* out) {
    if (!ctx || !wire_evals || !cosets || !out) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    return prove_impl(ctx, srs_id, circuit_id, ColumnsOf(wire_evals, 1, ColumnsOf::PI_FULL, &pi_evals), cosets, out);
}

int typlonk_prove_host(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const uint64_t* const wire_evals[3],
                       const uint64_t* pi_evals, const uint64_t cosets[3][4], typlonk_proof* out) {
    if (!ctx || !wire_evals || !cosets || !out) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    if (const int rc = null_host_column(ctx, wire_evals)) return rc;
    return prove_impl(ctx, srs_id, circuit_id, ColumnsOf(wire_evals, 1, ColumnsOf::PI_FULL, &pi_evals), cosets, out);
}

// ================================================================================================
// The compact shape (include/typlonk.h, typlonk_prove_compact): rounds 1 and 2 as in typlonk_prove, then round 3 in the
// compact transcript's order -- the quotient is committed before zeta is drawn, sigma_1(zeta) and sigma_2(zeta) are sent, and
// every opening at zeta is one witness of F = a + v b + v^2 c + v^3 Z + v^4 r + v^5 sigma_1 + v^6 sigma_2.
namespace {
// folds (an SRS shard on a context with a communicator): the two groups of commitments are folded over the ranks where the
// host needs them -- [t_lo] [t_mid] [t_hi] before zeta (3 records), W_zeta and W_zeta_w at the end (2 records).  A rank that
// fails joins the NEXT of the two collectives with flagged records and returns there, as its peers do (comm_fold).
int prover_round3_compact(typlonk_prover* p, CompactScript& script, typlonk_proof_compact* out, bool folds) {
    typlonk_ctx* ctx = p->ctx;
    // every way out before zeta / after zeta: through that stage's collective when folding
    auto leave_t = [&](int rc) { return folds ? comm_fold(ctx, &out->t_xy[0][0], out->t_inf, 3, rc) : rc; };
    auto leave_w = [&](int rc) { return folds ? comm_fold(ctx, &out->w_xy[0][0], out->w_inf, 2, rc) : rc; };
    if (p->round != 2) return leave_t(fail(ctx, TYPLONK_ERR_INVALID_ARG, "round3 must follow round2"));
    int rc = hip_rc(ctx, hipSetDevice(ctx->device));
    if (rc) return leave_t(rc);
    auto cit = ctx->circuits.find(p->circuit);
    if (cit == ctx->circuits.end()) return leave_t(fail(ctx, TYPLONK_ERR_INVALID_ARG, "circuit was freed during the proof"));
    const CircuitEntry& ce = cit->second;
    const uint64_t n = p->n;
    const uint32_t log_n = p->log_n;
    ProfilingOff prof_off(ctx);  // stage events are per call
    ProverRound in_round(ctx);
    const SrsEntry* srs = nullptr;
    rc = msm_validate(ctx, p->srs_id, n, &srs);
    if (!rc && !ctx->batch_fence) rc = hip_rc(ctx, hipEventCreateWithFlags(&ctx->batch_fence, hipEventDisableTiming));
    if (rc) return leave_t(rc);
    // the queue outlives every early return (its destructor-side wait below): the MSMs write into `out`
    MsmQueue q(ctx, srs, /*first_lane=*/0);
    WaitAll wait_guard{q};
    auto record_fence = [&]() -> int {
        const int frc = hip_rc(ctx, hipEventRecord(ctx->batch_fence, ctx->stream));
        if (frc) return frc;
        q.fence = ctx->batch_fence;   // the lanes wait for what is queued NOW, not for later work on the context's stream
        return TYPLONK_OK;
    };
    // ---- the quotient (proof.rs:139-145) as soon as alpha is known; its three slices (:181) committed behind a fence ----
    Fr al;
    memcpy(al.v, out->alpha, 32);
    rc = prover_quotient(p, al);
    if (!rc) rc = record_fence();
    if (!rc) {
        const Fr* polys[3] = {p->at(PR_T), p->at(PR_T, 1), p->at(PR_T, 2)};
        const size_t m[3] = {n, n, n > 3 ? n - 3 : 0};
        for (int k = 0; k < 3 && !rc; ++k) rc = q.submit(polys[k], m[k], out->t_xy[k], out->t_inf + k);
    }
    {
        const int r = q.wait_all();
        if (!rc) rc = r;
    }
    rc = leave_t(rc);   // collective 3 of a sharded proof
    if (rc) return rc;
    // ---- zeta binds the quotient ----
    const Fr ze = script.after_quotient(*out);
    const Fr zw = fe_mul(ze, fr_domain_root(log_n));
    // ---- a, b, c, Z, sigma_1, sigma_2, PI at zeta and Z at zeta*w with its quotient: three launches, one fetch
    // (COMPACT_SLOTS: the first seven slots are the proof's evaluations in order) ----
    constexpr Round3Slots S = COMPACT_SLOTS;
    Fr host[S.count];
    Fr zn, zh, l0z;
    rc = prover_open_round3(p, ce, S, /*with_quotients=*/false, ze, zw);
    if (rc) return leave_w(rc);
    lin_zeta_terms(ze, log_n, &zn, &zh, &l0z);   // while the kernels run
    rc = prover_fetch(p, host, 0, S.count);
    if (rc) return leave_w(rc);
    const Fr pi_z = p->has_pi ? host[S.pi] : Fr::zero();
    for (int i = 0; i < 7; ++i) memcpy(out->evals[i], host[i].v, 32);
    const Fr v = script.after_evals(*out);
    // ---- r (proof.rs:376-439, with +PI(zeta) as typlonk_prove); r(zeta) lands in its slot and is read after the commitments ----
    {
        static_assert(S.wire == 0 && S.z == 3 && S.zw == 4, "lin_scalars reads a, b, c, Z, Z(zeta w) as ev[0..4]");
        Fr scalar[LIN_TERMS], constant;
        lin_scalars(host, host[S.sig0], host[S.sig1], pi_z, p->beta, p->gamma, p->k, al, ze, zn, zh, l0z, scalar, &constant);
        rc = prover_linearise(p, ce, scalar, constant);
        if (rc) return leave_w(rc);
    }
    rc = prover_open_async(p, p->at(PR_R), n, ze, nullptr, S.r);
    // ---- F as one 7-term combination and its witness polynomial, in the places of q this shape gives them (ProveQ) ----
    if (!rc) {
        LincombArgs fa{};
        const Fr* polys[7] = {p->at(PR_CO, 0), p->at(PR_CO, 1), p->at(PR_CO, 2), p->at(PR_Z), p->at(PR_R), ce.coef + 5 * n, ce.coef + 6 * n};
        Fr pw = Fr::one();
        for (int i = 0; i < 7; ++i) {
            fa.poly[i] = polys[i];
            fa.scalar[i] = pw;
            pw = fe_mul(pw, v);
        }
        fa.terms = 7;
        fa.constant = Fr::zero();
        fa.out = p->at(PR_Q, Q_COMPACT_F);
        fa.n = n;
        launch_lincomb(fa, ctx->stream);
        rc = hip_rc(ctx, hipGetLastError());
    }
    if (!rc) rc = prover_open_async(p, p->at(PR_Q, Q_COMPACT_F), n, ze, p->at(PR_Q, Q_COMPACT_WIT), S.f);   // F(zeta) itself is not needed
    // ---- W_zeta and W_zeta_w in one queue ----
    if (!rc) rc = record_fence();
    if (!rc) rc = q.submit(p->at(PR_Q, Q_COMPACT_WIT), n - 1, out->w_xy[0], out->w_inf + 0);
    if (!rc) rc = q.submit(p->at(PR_Q, Q_WIT_ZW), n - 1, out->w_xy[1], out->w_inf + 1);
    {
        const int r = q.wait_all();
        if (!rc) rc = r;
    }
    Fr rz;
    if (!rc) rc = prover_fetch(p, &rz, S.r, 1);   // (every lane has been waited for: this returns at once)
    // collective 4 of a sharded proof.  r(zeta) comes from replicated data: an unsatisfied witness is unsatisfied on every
    // rank, the points are folded all the same and `out` is filled as on one GPU
    rc = leave_w(rc);
    if (rc) return rc;
    p->round = 3;
    if (!rz.is_zero())
        return fail(ctx, TYPLONK_ERR_UNSATISFIED, "r(zeta) != 0: the witness does not satisfy the circuit");
    return TYPLONK_OK;
}

// what typlonk_prove_compact refuses before it queues anything, in this order; fills the column sources
int prove_compact_args(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const ColumnsOf& in, ColumnSrc (&w)[3], ColumnSrc& pi) {
    HIPCHK(hipSetDevice(ctx->device));
    if (ctx->prover_busy) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "a proof is already in flight on this context");
    auto ci = ctx->circuits.find(circuit_id);
    if (ci == ctx->circuits.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown circuit id");
    const uint32_t log_n = ci->second.log_n;
    if (log_n > TYPLONK_MAX_PROVER_LOG_N) return fail(ctx, TYPLONK_ERR_DOMAIN, "prover supports up to 2^24 rows");
    const uint64_t n = 1ull << log_n;
    auto si = ctx->srs.find(srs_id);
    if (si == ctx->srs.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown srs id");
    if (si->second.total_len && !ctx->comm.comm)
        return fail(ctx, TYPLONK_ERR_INVALID_ARG,
                    "a compact proof on an SRS shard needs a communicator on the context (typlonk_comm_init): its commitments are "
                    "folded over the ranks inside the call, before each challenge");
    if (si->second.total() < n) return fail(ctx, TYPLONK_ERR_LENGTH, "SRS shorter than the circuit's n");
    // (this entry point judges pi_len > n and the stated row count before it looks at the columns)
    if (in.pi_rows(0, n) > n) return fail(ctx, TYPLONK_ERR_LENGTH, "more public inputs than rows");
    int rc = admit_rows(ctx, in, n);
    if (!rc) rc = null_handle_is_short(ctx, in);
    if (!rc) rc = admit_columns(ctx, in, n);
    if (rc) return rc;
    for (int i = 0; i < 3; ++i) w[i] = in.column(0, i, n);
    pi = in.pi(0, n);
    return TYPLONK_OK;
}

// On an SRS shard with a communicator (folds) the call is a collective with a FIXED schedule of 12, 1, 3 and 2 records:
//   1. [a] [b] [c], this rank's eight partial circuit commitments (cached or not) and its P0 record -- before beta, gamma;
//      the statement digest d0 is formed from the folded key, after this fold (it is first hashed together with [a] [b] [c])
//   2. [Z] before alpha      3. [t_lo] [t_mid] [t_hi] before zeta      4. W_zeta, W_zeta_w
// The counts depend on nothing a rank could see differently from its peers: not on its cache, not on which argument it
// refuses.  From here on every path of a member ends in the next collective: a rank that fails joins it with flagged records
// and returns its own code there, its peers return TYPLONK_ERR_COMM there (comm_fold), the prover is freed on every path.
int prove_compact_impl(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const ColumnsOf& in, const uint64_t cosets[3][4],
                       typlonk_proof_compact* out) {
    const bool folds = comm_folds(ctx, srs_id);
    ColumnSrc w[3], pi;
    int rc = prove_compact_args(ctx, srs_id, circuit_id, in, w, pi);
    if (rc && !folds) return rc;
    if (!rc) memset(out, 0, sizeof(*out));
    // the statement: the circuit's commitments (one batch of eight MSMs the first time per circuit and SRS, then cached), P0,
    // and the pi_len public values -- brought to the host once in the device form
    typlonk_vk vk;
    uint64_t rec_xy[12][12];   // the first fold of a sharded proof: a b c | q_l .. sigma_3 | P0
    uint8_t rec_inf[12];
    if (!rc) rc = folds ? circuit_statement_partial(ctx, srs_id, circuit_id, rec_xy + 3, rec_inf + 3)
                        : circuit_vk_fill(ctx, srs_id, circuit_id, cosets, &vk);
    std::vector<uint64_t> pi_vals;
    const uint64_t* piv = pi.host;
    const size_t pi_len = pi.rows;
    if (!rc && pi.dev) {
        pi_vals.resize(4 * pi_len);
        hipError_t he = hipMemcpyAsync(pi_vals.data(), pi.dev, pi_len * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream);
        if (he == hipSuccess) he = hipStreamSynchronize(ctx->stream);
        rc = hip_rc(ctx, he);
        piv = pi_vals.data();
    }
    if (rc && !folds) return rc;
    uint8_t d0[64];
    if (!folds) compact_statement_digest(vk, piv, pi_len, d0);
    typlonk_prover* p = nullptr;
    if (!rc) rc = prover_round1_impl(ctx, srs_id, circuit_id, w, pi, &p, out->commit_xy, out->commit_inf);
    if (folds) {
        if (!rc) {
            memcpy(rec_xy, out->commit_xy, 3 * 96);
            memcpy(rec_inf, out->commit_inf, 3);
        }
        rc = comm_fold(ctx, &rec_xy[0][0], rec_inf, 12, rc);   // collective 1
        if (!rc) {
            memcpy(out->commit_xy, rec_xy, 3 * 96);
            memcpy(out->commit_inf, rec_inf, 3);
            vk_assemble(p->log_n, cosets, rec_xy + 3, rec_inf + 3, &vk);
            compact_statement_digest(vk, piv, pi_len, d0);
        }
    }
    if (rc) {
        if (p) typlonk_prover_free(p);
        return rc;
    }
    CompactScript script(d0);   // (a sharded proof has d0 only now, from the folded key)
    script.after_round1(*out);
    rc = typlonk_prover_round2(p, out->beta, out->gamma, cosets, out->z_xy, &out->z_inf);
    if (folds) rc = comm_fold(ctx, out->z_xy, &out->z_inf, 1, rc);   // collective 2
    if (!rc) {
        script.after_round2(*out);
        rc = prover_round3_compact(p, script, out, folds);   // collectives 3 and 4
    }
    typlonk_prover_free(p);
    return rc;
}
}  // namespace

int typlonk_prove_compact(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const typlonk_buf* const wire_evals[3],
                          const typlonk_buf* pi, size_t pi_len, const uint64_t cosets[3][4], typlonk_proof_compact* out) {
    if (!ctx || !wire_evals || !cosets || !out || (pi_len && !pi)) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    return prove_compact_impl(ctx, srs_id, circuit_id, ColumnsOf(wire_evals, 1, ColumnsOf::PI_FIRST, &pi, &pi_len), cosets, out);
}

int typlonk_prove_compact_host(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const uint64_t* const wire_evals[3],
                               size_t rows, const uint64_t* pi, size_t pi_len, const uint64_t cosets[3][4],
                               typlonk_proof_compact* out) {
    if (!ctx || !wire_evals || !cosets || !out || (pi_len && !pi)) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    if (const int rc = null_host_column(ctx, wire_evals)) return rc;
    return prove_compact_impl(ctx, srs_id, circuit_id, ColumnsOf(wire_evals, 1, ColumnsOf::PI_FIRST, &pi, &pi_len).with_rows(rows),
                              cosets, out);
}

void typlonk_prover_free(typlonk_prover* p) {
    if (!p) return;
    (void)hipStreamSynchronize(p->ctx->stream);
    p->ctx->prover_busy = false;
    delete p;
}

