// libtyplonk_hip.so -- MSM staging: sort / accumulate / reduce launches, the lanes of a batch, the host finish; SRS entry points
// Part of the host driver of include/typlonk.h (see host.hpp for the shared state).  There is deliberately no CPU compute
// fallback: without a HIP device typlonk_init fails with TYPLONK_ERR_NO_DEVICE.
#include "host.hpp"

using namespace ty;
using namespace tyh;

namespace tyh {

// ---- MSM: what to run is decided in msm_plan.hpp; here it is sized and queued ---------------------------------
void write_affine_out(const G1Affine& a, uint64_t out_xy[12], uint8_t* out_inf) {
    uint32_t w[12];
    if (a.is_inf()) {
        // ark-ec GroupAffine::zero(): x = 0, y = 1 (Montgomery one, R = 2^384), infinity = true
        memset(out_xy, 0, 6 * sizeof(uint64_t));
        fq30_to_ark(fq30_one(), w);
        memcpy(out_xy + 6, w, sizeof(w));
        *out_inf = 1;
    } else {
        fq30_to_ark(a.x, w);
        memcpy(out_xy, w, sizeof(w));
        fq30_to_ark(a.y, w);
        memcpy(out_xy + 6, w, sizeof(w));
        *out_inf = 0;
    }
}

// Every workspace buffer the planned MSM needs, before anything of it is queued: no allocation (hipFree + hipMalloc, a device
// synchronisation) falls between the copies and kernels of its chunks, and none can fail with a copy in flight.
static int msm_size(typlonk_ctx* ctx, MsmWs& ws, const MsmPlan& plan) {
    int rc;
    for (int set = 0; set < 2; ++set) {   // (a single chunk asks nothing of the second set)
        SortBufs& sb = ws.sb[set];
        const MsmSortBytes& z = plan.sort[set];
        const std::pair<DevBuf*, size_t> want[] = {
            {&sb.keys, z.keys}, {&sb.sorted, z.sorted}, {&sb.counts, z.counts}, {&sb.offsets, z.offsets}, {&sb.cursor, z.cursor},
            {&sb.blocksums, z.blocksums}, {&sb.order, z.order}, {&sb.ohist, z.ohist}, {&sb.blk_hist, z.blk_hist},
            {&sb.blk_base, z.blk_base}, {&sb.blk_cnt, z.blk_cnt}, {&sb.seg_start, z.seg_start}, {&sb.heavy, z.heavy},
            {&sb.tasks, z.tasks}, {&sb.hpart, z.hpart}};
        for (const auto& w : want)
            if ((rc = ensure(ctx, *w.first, w.second))) return rc;
    }
    const std::pair<DevBuf*, size_t> want[] = {{&ws.buckets, plan.buckets}, {&ws.part_a, plan.part_a}, {&ws.part_b, plan.part_b},
                                               {&ws.rc_sums, plan.rc_sums}, {&ws.rc_bits, plan.rc_bits}, {&ws.rc_out, plan.rc_out}};
    for (const auto& w : want)
        if ((rc = ensure(ctx, *w.first, w.second))) return rc;
    return TYPLONK_OK;
}

// Queue the planned MSM on ws.stream (and the sorts of overlapped chunks on ws.side): per chunk the copy of host scalars, the
// sort, the accumulation; then the reduction and the copy of its result into ws.host_wins.  Reads every size and shape from
// the plan and derives none.
static int msm_queue(typlonk_ctx* ctx, MsmWs& ws, const MsmPlan& plan, const SrsEntry& srs, const Fr* d_scalars,
                     const uint64_t* h_scalars) {
    hipStream_t s = ws.stream;
    const uint32_t nch = plan.nch, nb = (uint32_t)plan.nb;
    const bool overlap = plan.overlap;
    if (overlap) {
        // the side stream carries the sorts of the chunks after the first: short, latency-bound kernels beside an
        // accumulation that fills every wavefront slot (a high stream priority for it was measured: no effect)
        if (!ws.side) HIPCHK(hipStreamCreateWithFlags(&ws.side, hipStreamNonBlocking));
        if (!ws.ev_in) HIPCHK(hipEventCreateWithFlags(&ws.ev_in, hipEventDisableTiming));
        for (uint32_t k = 0; k < nch; ++k) {
            if (!ws.ev_sorted[k]) HIPCHK(hipEventCreateWithFlags(&ws.ev_sorted[k], hipEventDisableTiming));
            if (!ws.ev_acc[k]) HIPCHK(hipEventCreateWithFlags(&ws.ev_acc[k], hipEventDisableTiming));
        }
        HIPCHK(hipEventRecord(ws.ev_in, s));  // the scalars (and whatever produced them) are ordered on s
        HIPCHK(hipStreamWaitEvent(ws.side, ws.ev_in, 0));
    }
    uint32_t* buckets = (uint32_t*)ws.buckets.p;

    for (uint32_t k = 0; k < plan.chunk.size(); ++k) {
        const MsmChunkPlan& ck = plan.chunk[k];
        const Fr* sc = d_scalars + ck.off;
        const uint32_t* pts = srs.d_points + ck.off * PT_WORDS;  // chunk-local term index i -> base off + i (table t: + t*len)
        SortBufs& sb = ws.sb[k & 1];
        hipStream_t ss = ck.beside ? ws.side : s;
        if (overlap && k >= 2) HIPCHK(hipStreamWaitEvent(ss, ws.ev_acc[k - 2], 0));  // sb[k & 1] is free again
        // the first chunk's sort is the exposed one: the second chunk's sort starts behind it (it then has the whole first
        // accumulation to hide under) instead of beside it, where it doubled its time (profiles/r03_msm_2_20_timeline.txt)
        if (overlap && k == 1) HIPCHK(hipStreamWaitEvent(ss, ws.ev_sorted[0], 0));
        if (h_scalars)
            HIPCHK(hipMemcpyAsync(const_cast<Fr*>(sc), h_scalars + 4 * ck.off, ck.mk * sizeof(Fr), hipMemcpyHostToDevice, ss));
        uint32_t* keys = (uint32_t*)sb.keys.p;
        uint32_t* sorted = (uint32_t*)sb.sorted.p;
        uint32_t* counts = (uint32_t*)sb.counts.p;
        uint32_t* offsets = (uint32_t*)sb.offsets.p;
        uint32_t* blocksums = (uint32_t*)sb.blocksums.p;
        if (ck.segsort) {
            StageTimer st(ctx, ck.beside ? "msm_sort_overlapped" : "msm_sort", ss);
            const MsmSortPtrs p = {(uint32_t*)sb.blk_hist.p, (uint32_t*)sb.blk_base.p, blocksums, (uint32_t*)sb.blk_cnt.p,
                                   (uint32_t*)sb.seg_start.p, keys, counts, offsets, sorted, (uint32_t*)sb.ohist.p,
                                   (uint32_t*)sb.heavy.p, (uint32_t*)sb.tasks.p, (uint32_t*)sb.order.p};
            launch_msm_segsort(sc, (uint64_t)ck.mk, ck.sh, p, ck.cap, plan.scatter_staged ? 1 : 0, ss);
        } else {
            // The segmented sort ends with the bucket schedule (order[], msm_seg_place_kernel); only the atomic sort of the
            // shapes it cannot take needs the separate schedule launches.
            {
                StageTimer st(ctx, "msm_digits", ss);
                HIPCHK(hipMemsetAsync(counts, 0, plan.nb * 4, ss));
                launch_msm_digits(sc, (uint64_t)ck.mk, plan.c, plan.W, plan.digit_v, keys, counts, ss);
            }
            {
                StageTimer st(ctx, "msm_scan", ss);
                launch_scan(counts, plan.nb, blocksums, offsets, (uint32_t*)sb.cursor.p, ss);
            }
            {
                StageTimer st(ctx, "msm_scatter", ss);
                launch_msm_scatter(keys, (uint64_t)ck.mk, (uint64_t)plan.W * ck.mk, (uint32_t*)sb.cursor.p, sorted, ss);
            }
            StageTimer st(ctx, "msm_order", ss);
            launch_bucket_order(counts, offsets, nb, ck.cap, (uint32_t*)sb.ohist.p, (uint32_t*)sb.order.p, (uint32_t*)sb.heavy.p,
                                (uint32_t*)sb.tasks.p, ss);
        }
        if (ss != s) {   // an overlapped chunk: the accumulation on the MSM's stream waits for the side stream's sort
            HIPCHK(hipEventRecord(ws.ev_sorted[k], ss));
            HIPCHK(hipStreamWaitEvent(s, ws.ev_sorted[k], 0));
        } else if (overlap && k == 0) {
            HIPCHK(hipEventRecord(ws.ev_sorted[0], s));
        }
        {
            if (plan.chain && ctx->accum_chain_live) HIPCHK(hipStreamWaitEvent(s, ctx->accum_chain, 0));
            StageTimer st(ctx, "msm_accum", s);
            launch_msm_accum(pts, offsets, sorted, (const uint32_t*)sb.order.p, nb, ck.cap, /*init=*/k > 0, ck.lanes, ck.split, buckets, s);
            launch_msm_heavy(pts, sorted, (const uint32_t*)sb.ohist.p, (uint32_t*)sb.heavy.p,
                             (const uint32_t*)sb.tasks.p, (uint32_t*)sb.hpart.p, buckets, s);
            if (plan.chain) {
                if (!ctx->accum_chain) HIPCHK(hipEventCreateWithFlags(&ctx->accum_chain, hipEventDisableTiming));
                HIPCHK(hipEventRecord(ctx->accum_chain, s));
                ctx->accum_chain_live = true;
            }
        }
        if (overlap && k + 2 < nch) HIPCHK(hipEventRecord(ws.ev_acc[k], s));
    }
    // row/column bucket reduction (msm_plan.hpp, RcShape)
    const RcShape& sh = plan.rcs;
    // one shared bucket set (table mode): the last kernel of the reduction writes its <= 32 plane points straight into
    // the pinned host landing zone (device-visible) -- no copy kernel between it and the host's wait
    uint32_t* planes_out = sh.nsets == 1 ? ws.host_wins : (uint32_t*)ws.rc_out.p;
    StageTimer st(ctx, "msm_reduce", s);
    if (plan.rc2)
        launch_msm_rc2_reduce(buckets, sh, (uint32_t*)ws.part_b.p, (uint32_t*)ws.part_a.p, planes_out, s);
    else
        launch_msm_rc_reduce(buckets, sh, (uint32_t*)ws.part_b.p, (uint32_t*)ws.part_a.p, (uint32_t*)ws.rc_sums.p,
                             (uint32_t*)ws.rc_bits.p, planes_out, s);
    if (sh.nsets > 1) {
        // plain MSM: per-set powers of two on the device, the host keeps its Horner over the windows
        uint32_t* set_sums = (uint32_t*)ws.part_a.p;  // the column partials are consumed by now
        launch_msm_rc_combine((const uint32_t*)ws.rc_out.p, sh, set_sums, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(ws.host_wins, set_sums, (size_t)sh.nsets * 192, hipMemcpyDeviceToHost, s));
    } else {
        HIPCHK(hipGetLastError());
    }
    return TYPLONK_OK;
}

// Launch every kernel of one m-term MSM (m > 0, validated by the caller) on `stream` using workspace
// `ws`, ending with the asynchronous copy of the W window sums into ws.host_wins: plan, size, queue.
// h_scalars != NULL: the scalars are still on the HOST (typlonk_msm_g1: the reference's commit() hands over a Vec<Fr>); every
// chunk's slice is copied to d_scalars on the stream that sorts that chunk, so the copy of chunk k + 1 crosses PCIe while chunk k
// is sorted and accumulated instead of the whole vector crossing before the first kernel starts.
int msm_enqueue(typlonk_ctx* ctx, MsmWs& ws, hipStream_t stream, const SrsEntry& srs, const Fr* d_scalars, size_t m,
                uint64_t* out_xy, uint8_t* out_inf, bool standalone, const uint64_t* h_scalars) {
    ws.stream = stream;
    if (!ws.host_wins) HIPCHK(hipHostMalloc((void**)&ws.host_wins, HOST_WIN_POINTS * 192));
    const MsmSrsFacts facts = {srs.len, srs.table_c, srs.table_T, srs.table_centred};
    const MsmOverrides ov = {ctx->msm_chunks, ctx->msm_lanes, ctx->msm_scatter_staged, ctx->msm_rc4, ctx->msm_chain};
    const MsmPlan plan = msm_plan(facts, m, standalone, h_scalars != nullptr, ov);
    if (plan.status == MSM_PLAN_TOO_LARGE) return fail(ctx, TYPLONK_ERR_LENGTH, "MSM too large for 32-bit entry indices");
    if (plan.status != MSM_PLAN_OK) return fail(ctx, TYPLONK_ERR_LENGTH, "table-mode MSM shape not supported");  // unreachable
    int rc = msm_size(ctx, ws, plan);
    if (rc) return rc;
    if ((rc = msm_queue(ctx, ws, plan, srs, d_scalars, h_scalars))) {
        // a copy from the caller's host buffer may be in flight: it ends before the caller gets its buffer back
        if (h_scalars) {
            if (ws.side) (void)hipStreamSynchronize(ws.side);
            (void)hipStreamSynchronize(stream);
        }
        return rc;
    }
    ws.pending = true;
    ws.rc = plan.nsets == 1;   // one shared bucket set: host_wins holds the reduction's bit planes, else the per-set sums
    ws.rcs = plan.rcs;
    ws.W = plan.nsets;
    ws.c = plan.tables ? 0 : plan.c;  // table mode: the set sums are simply added
    ws.out_xy = out_xy;
    ws.out_inf = out_inf;
    return TYPLONK_OK;
}

// Wait for an enqueued MSM and finish it on the host: sum_j 2^(c*j) * window_j (Horner from the top
// window), then the canonical affine form.
int msm_finish(typlonk_ctx* ctx, MsmWs& ws) {
    if (!ws.pending) return TYPLONK_OK;
    ws.pending = false;
    HIPCHK(hipStreamSynchronize(ws.stream));
    // host arithmetic on 6 x 64-bit words (g1_host64.hpp): a third of the time of the 13 x 30-bit limb code here
    namespace H = h64;
    auto out = [&](const H::Xyzz& acc) {
        if (H::xyzz_to_affine(acc, ws.out_xy)) *ws.out_inf = 0;
        else write_affine_out(G1Affine::inf(), ws.out_xy, ws.out_inf);
    };
    if (ws.rc) {
        // bit planes -> points by power of two: set j (offset c*j; 0 in table mode), rows carry 2^shift
        const RcShape& sh = ws.rcs;
        std::vector<H::Xyzz> pe(ws.c * sh.nsets + 2 * RC_NB + sh.cl + 2, H::inf());
        int top = -1;
        for (uint32_t j = 0; j < sh.nsets; ++j) {
            uint32_t nbr, nbc, shift;
            rc_bits(sh, j, &nbr, &nbc, &shift);
            for (uint32_t kind = 0; kind < 2; ++kind)
                for (uint32_t b = 0; b < (kind ? nbc : nbr); ++b) {
                    const H::Xyzz pt = H::xyzz_from_device(ws.host_wins + (size_t)((j * 2 + kind) * RC_NB + b) * 48);
                    if (H::is_inf(pt)) continue;
                    const uint32_t e = ws.c * j + b + (kind ? 0u : shift);
                    pe[e] = H::xyzz_add(pe[e], pt);
                    top = std::max(top, (int)e);
                }
        }
        H::Xyzz acc = H::inf();
        for (int e = top; e >= 0; --e) {
            if (!H::is_inf(acc)) acc = H::xyzz_dbl(acc);
            if (!H::is_inf(pe[e])) acc = H::xyzz_add(acc, pe[e]);
        }
        out(acc);
        return TYPLONK_OK;
    }
    H::Xyzz acc = H::inf();
    for (int j = (int)ws.W - 1; j >= 0; --j) {
        if (!H::is_inf(acc))
            for (uint32_t d = 0; d < ws.c; ++d) acc = H::xyzz_dbl(acc);
        acc = H::xyzz_add(acc, H::xyzz_from_device(ws.host_wins + (size_t)j * 48));
    }
    out(acc);
    return TYPLONK_OK;
}

// the SRS entry of an id, or NULL with the context's error set (the caller returns TYPLONK_ERR_INVALID_ARG)
static SrsEntry* srs_lookup(typlonk_ctx* ctx, uint32_t srs_id) {
    auto it = ctx->srs.find(srs_id);
    if (it != ctx->srs.end()) return &it->second;
    (void)fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown srs id");
    return nullptr;
}

int msm_validate(typlonk_ctx* ctx, uint32_t srs_id, size_t m, const SrsEntry** srs) {
    const SrsEntry* e = srs_lookup(ctx, srs_id);
    if (!e) return TYPLONK_ERR_INVALID_ARG;
    if (m > e->total()) return fail(ctx, TYPLONK_ERR_LENGTH, "MSM length exceeds SRS length (kzg/src/lib.rs:43)");
    *srs = e;
    return TYPLONK_OK;
}

// d_scalars points at coefficient 0 of the m-term vector (ptr_is_local: at the first coefficient of this
// entry's share instead); an SRS shard sums only its own index range
int msm_run(typlonk_ctx* ctx, uint32_t srs_id, const Fr* d_scalars, size_t m, uint64_t out_xy[12], uint8_t* out_inf, bool ptr_is_local,
            const uint64_t* h_scalars) {
    if (!out_xy || !out_inf) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null output");
    const SrsEntry* srs = nullptr;
    int rc = msm_validate(ctx, srs_id, m, &srs);
    if (rc) return rc;
    prof_begin(ctx);
    size_t off, ml;
    srs->local_range(m, &off, &ml);
    if (ml == 0) {
        write_affine_out(G1Affine::inf(), out_xy, out_inf);
        prof_collect(ctx);
        return TYPLONK_OK;
    }
    if (!d_scalars) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null scalars");
    if (!ptr_is_local) d_scalars += off;
    m = ml;
    if ((rc = msm_enqueue(ctx, ctx->ws[0], ctx->stream, *srs, d_scalars, m, out_xy, out_inf, /*standalone=*/true, h_scalars))) return rc;
    if ((rc = msm_finish(ctx, ctx->ws[0]))) return rc;
    prof_collect(ctx);
    return TYPLONK_OK;
}

// ---- MsmQueue (host.hpp) --------------------------------------------------------------------------------------------
MsmQueue::MsmQueue(typlonk_ctx* c, const SrsEntry* s, int first_lane)
    : ctx(c), srs(s),
      lanes(std::max(1, std::min<int>(c->msm_inflight ? c->msm_inflight : (s->len < MSM_FOUR_LANES_BELOW ? 4 : 3), typlonk_ctx::MSM_LANES))),
      lane_lo(0), next(0) {
    set_first_lane(first_lane);
}
void MsmQueue::set_first_lane(int l) {
    lane_lo = (l < lanes) ? l : 0;
    if (next < lane_lo) next = lane_lo;
}
int MsmQueue::submit(const Fr* d_scalars, size_t m, uint64_t* out_xy, uint8_t* out_inf, bool standalone) {
    size_t off, ml;
    srs->local_range(m, &off, &ml);
    if (ml == 0) {
        write_affine_out(G1Affine::inf(), out_xy, out_inf);
        return TYPLONK_OK;
    }
    if (next >= lanes || next < lane_lo) next = lane_lo;
    const int l = next++;
    MsmWs& ws = ctx->ws[l];
    int rc = msm_finish(ctx, ws);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    if (l) {
        if (!ctx->lane[l]) HIPCHK(hipStreamCreateWithFlags(&ctx->lane[l], hipStreamNonBlocking));
        if (!ctx->lane_evt[l]) HIPCHK(hipEventCreateWithFlags(&ctx->lane_evt[l], hipEventDisableTiming));
        if (fence) {
            HIPCHK(hipStreamWaitEvent(ctx->lane[l], fence, 0));
        } else {
            HIPCHK(hipEventRecord(ctx->lane_evt[l], ctx->stream));
            HIPCHK(hipStreamWaitEvent(ctx->lane[l], ctx->lane_evt[l], 0));
        }
        st = ctx->lane[l];
    }
    return msm_enqueue(ctx, ws, st, *srs, d_scalars + off, ml, out_xy, out_inf, standalone, nullptr);
}
int MsmQueue::wait_all() {
    int rc = TYPLONK_OK;
    for (int l = 0; l < typlonk_ctx::MSM_LANES; ++l) {
        const int r = msm_finish(ctx, ctx->ws[l]);
        if (!rc) rc = r;
    }
    return rc;
}

// count independent MSMs over the same SRS, up to MSM_LANES in flight (separate workspaces/streams)
int msm_batch(typlonk_ctx* ctx, uint32_t srs_id, const void* const* d_scalars, const size_t* m, size_t count,
              uint64_t* out_xy, uint8_t* out_inf) {
    if (!out_xy || !out_inf || !m || (!d_scalars && count)) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    const SrsEntry* srs = nullptr;
    for (size_t k = 0; k < count; ++k) {
        int rc = msm_validate(ctx, srs_id, m[k], &srs);
        if (rc) return rc;
        if (m[k] && !d_scalars[k]) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null scalars");
    }
    if (!count) return TYPLONK_OK;
    prof_begin(ctx);
    ProfilingOff prof_off(ctx);  // stage events are per call
    MsmQueue q(ctx, srs);
    // all scalars exist when the call is made: the lanes wait for what is on the context's stream NOW, not for the
    // MSMs of this batch that lane 0 (the context's stream itself) receives in the meantime
    if (!ctx->batch_fence) HIPCHK(hipEventCreateWithFlags(&ctx->batch_fence, hipEventDisableTiming));
    HIPCHK(hipEventRecord(ctx->batch_fence, ctx->stream));
    q.fence = ctx->batch_fence;
    int rc = TYPLONK_OK;
    for (size_t k = 0; k < count && !rc; ++k)
        rc = q.submit((const Fr*)d_scalars[k], m[k], out_xy + 12 * k, out_inf + k, /*standalone=*/count == 1);
    const int r = q.wait_all();
    return rc ? rc : r;
}

}  // namespace tyh

// (entry points: C linkage comes from their declarations in include/typlonk.h)

int typlonk_srs_load(typlonk_ctx* ctx, const uint64_t* xy, const uint8_t* inf, size_t len, uint32_t* srs_id) {
    if (!ctx || !srs_id || (!xy && len)) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    HIPCHK(hipSetDevice(ctx->device));
    SrsEntry e;
    e.len = len;
    DevGuard guard;
    HIPCHK(hipMalloc((void**)&e.d_points, std::max<size_t>(len, 1) * PT_WORDS * 4));
    guard.add(e.d_points);
    if (len) {
        HIPCHK(hipMemcpy2DAsync(e.d_points, PT_WORDS * 4, xy, 96, 96, len, hipMemcpyHostToDevice, ctx->stream));
        DevGuard flags;  // freed on every path out of this block
        uint8_t* d_inf = nullptr;
        if (inf) {
            HIPCHK(hipMalloc((void**)&d_inf, len));
            flags.add(d_inf);
            HIPCHK(hipMemcpyAsync(d_inf, inf, len, hipMemcpyHostToDevice, ctx->stream));
        }
        launch_convert_points(e.d_points, d_inf, (uint64_t)len, ctx->stream);  // arkworks -> internal form
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    guard.dismiss();
    const uint32_t id = ctx->next_srs++;
    ctx->srs[id] = e;
    *srs_id = id;
    return TYPLONK_OK;
}

int typlonk_srs_free(typlonk_ctx* ctx, uint32_t srs_id) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    SrsEntry* e = srs_lookup(ctx, srs_id);
    if (!e) return TYPLONK_ERR_INVALID_ARG;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipFree(e->d_points));
    ctx->srs.erase(srs_id);
    return TYPLONK_OK;
}

int typlonk_srs_set_shard(typlonk_ctx* ctx, uint32_t srs_id, size_t first_index, size_t total_len) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    SrsEntry* e = srs_lookup(ctx, srs_id);
    if (!e) return TYPLONK_ERR_INVALID_ARG;
    if (first_index > total_len || e->len > total_len - first_index)
        return fail(ctx, TYPLONK_ERR_RANGE, "shard does not fit into total_len");
    e->shard_first = first_index;
    e->total_len = total_len;
    return TYPLONK_OK;
}

int typlonk_srs_len(typlonk_ctx* ctx, uint32_t srs_id, size_t* len) {
    if (!ctx || !len) return TYPLONK_ERR_INVALID_ARG;
    const SrsEntry* e = srs_lookup(ctx, srs_id);
    if (!e) return TYPLONK_ERR_INVALID_ARG;
    *len = e->len;
    return TYPLONK_OK;
}

int typlonk_srs_generate(typlonk_ctx* ctx, const uint64_t secret[4], uint64_t start, size_t len, uint32_t* srs_id) {
    if (!ctx || !secret || !srs_id) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    HIPCHK(hipSetDevice(ctx->device));
    SrsEntry e;
    e.len = len;
    DevGuard guard;
    HIPCHK(hipMalloc((void**)&e.d_points, std::max<size_t>(len, 1) * PT_WORDS * 4));
    guard.add(e.d_points);
    if (len) {
        Fr s;
        memcpy(s.v, secret, sizeof(s.v));
        const bool build_comb = !ctx->srs_comb_ready;   // [j 2^(8w)] G, once per context
        if (build_comb) {
            const int rc = ensure(ctx, ctx->srs_comb, srs_comb_bytes());
            if (rc != TYPLONK_OK) return rc;
            launch_srs_comb((uint32_t*)ctx->srs_comb.p, ctx->stream);
            HIPCHK(hipGetLastError());
        }
        launch_srs_generate(s, start, (uint64_t)len, (const uint32_t*)ctx->srs_comb.p, e.d_points, ctx->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(ctx->stream));
        ctx->srs_comb_ready = true;   // only now: a failed build is repeated by the next call, never read
    }
    guard.dismiss();
    const uint32_t id = ctx->next_srs++;
    ctx->srs[id] = e;
    *srs_id = id;
    return TYPLONK_OK;
}

int typlonk_selftest_fq_inv(typlonk_ctx* ctx, uint64_t seed, size_t count, uint64_t* mismatches, uint32_t* max_rounds) {
    if (!ctx || !mismatches) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    HIPCHK(hipSetDevice(ctx->device));
    uint32_t* d = nullptr;
    HIPCHK(hipMalloc((void**)&d, 16));
    DevGuard guard;
    guard.add(d);
    HIPCHK(hipMemsetAsync(d, 0, 16, ctx->stream));
    const uint32_t threads = 1u << 16;
    const uint32_t per = (uint32_t)((count + threads - 1) / threads);
    if (per) launch_fq_inv_selftest(seed, threads, per, d, ctx->stream);
    HIPCHK(hipGetLastError());
    uint32_t h[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(h, d, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *mismatches = h[0];
    if (max_rounds) *max_rounds = h[1];
    return TYPLONK_OK;
}

int typlonk_srs_precompute(typlonk_ctx* ctx, uint32_t srs_id, uint32_t window_bits) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    SrsEntry* found = srs_lookup(ctx, srs_id);
    if (!found) return TYPLONK_ERR_INVALID_ARG;
    SrsEntry& e = *found;
    if (window_bits == 0) {
        // auto: 15 below 2^16 points, 17 below 2^19, else 20 (measured best: HISTORY.md sections 4, 6;
        // profiles/r04_tables_small_sizes.txt) -- and nothing at all for an SRS shorter
        // than 2^14 points: 2^16 buckets (sort, reduction, heavy-bucket launch) for a handful of terms would be slower
        // than the plain path, whose window follows the length
        if (e.len < TYPLONK_TABLES_AUTO_MIN_LEN) return TYPLONK_OK;
        window_bits = e.len < (1u << 16) ? 15 : (e.len < (1u << 19) ? 17 : 20);
    }
    if (window_bits < 14 || window_bits > 20) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "window_bits must be 0 (auto) or 14..20");
    if (e.table_T) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "tables already built for this SRS");
    if (e.len == 0 || e.len > ((size_t)1 << 25)) return fail(ctx, TYPLONK_ERR_LENGTH, "tables need 1 <= len <= 2^25");
    HIPCHK(hipSetDevice(ctx->device));
    // centred scalars (|k| < 2^254) save a window -- and a table -- for c = 17 (15 instead of 16) and c = 15
    const bool centred = msm_windows(window_bits, true) < msm_windows(window_bits, false);
    const uint32_t T = msm_windows(window_bits, centred);
    // The sort sees one chunk at a time (msm_chunks), so MSMs of any length up to len run in table mode; one whose largest
    // chunk had no table-mode sort shape (more than 2^22 terms with 20-bit windows: 23 index bits leave too few low bucket
    // bits for the LDS level of the sort) would simply take the plain path over table 0, which IS the SRS (msm_enqueue) --
    // a set-up call that is supposed to be speed-only never turns a valid MSM into an error.  Refused: an SRS whose gather
    // indices would reach bit 31, and a window for which not even the shortest table-mode MSM (len / 4 terms) could be sorted.
    if (!msm_table_srs_ok(e.len, window_bits, T))
        return fail(ctx, TYPLONK_ERR_LENGTH, "fixed-base tables with this window are not supported for an SRS of this length");
    uint32_t* big = nullptr;
    HIPCHK(hipMalloc((void**)&big, (size_t)T * e.len * PT_WORDS * 4));
    DevGuard guard;
    guard.add(big);
    HIPCHK(hipMemcpyAsync(big, e.d_points, e.len * PT_WORDS * 4, hipMemcpyDeviceToDevice, ctx->stream));
    // scratch of the shared normalisation: one denominator per table entry, freed when the call returns
    uint32_t* zbuf = nullptr;
    HIPCHK(hipMalloc((void**)&zbuf, srs_tables_scratch_bytes(e.len, T)));
    DevGuard zguard;
    zguard.add(zbuf);
    launch_srs_tables(big, zbuf, (uint64_t)e.len, window_bits, T, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    guard.dismiss();
    HIPCHK(hipFree(e.d_points));
    e.d_points = big;
    e.table_c = window_bits;
    e.table_T = T;
    e.table_centred = centred;
    return TYPLONK_OK;
}

int typlonk_srs_download(typlonk_ctx* ctx, uint32_t srs_id, size_t offset, size_t count, uint64_t* xy, uint8_t* inf) {
    if (!ctx || (!xy && count)) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    const SrsEntry* e = srs_lookup(ctx, srs_id);
    if (!e) return TYPLONK_ERR_INVALID_ARG;
    if (offset > e->len || count > e->len - offset) return fail(ctx, TYPLONK_ERR_RANGE, "range outside SRS");
    if (!count) return TYPLONK_OK;
    return points_to_host(ctx, e->d_points + offset * PT_WORDS, count, xy, inf);
}

int tyh::points_to_host(typlonk_ctx* ctx, const uint32_t* d_points, size_t count, uint64_t* xy, uint8_t* inf) {
    HIPCHK(hipMemcpy2DAsync(xy, 96, d_points, PT_WORDS * 4, 96, count, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < count; ++i) {  // internal packed form -> arkworks; (0,0) -> ark-ec (0, 1, inf)
        G1Affine a;
        uint32_t w[12];
        memcpy(w, xy + i * 12, 48);
        a.x = fq30_unpack(w);
        memcpy(w, xy + i * 12 + 6, 48);
        a.y = fq30_unpack(w);
        uint8_t f = 0;
        write_affine_out(a, xy + i * 12, &f);
        if (inf) inf[i] = f;
    }
    return TYPLONK_OK;
}

int typlonk_msm_g1_devptr(typlonk_ctx* ctx, uint32_t srs_id, const void* d_scalars, size_t m, uint64_t out_xy[12],
                          uint8_t* out_inf) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return msm_run(ctx, srs_id, (const Fr*)d_scalars, m, out_xy, out_inf);
}

int typlonk_msm_g1_batch_devptr(typlonk_ctx* ctx, uint32_t srs_id, const void* const* d_scalars, const size_t* m,
                                size_t count, uint64_t* out_xy, uint8_t* out_inf) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return msm_batch(ctx, srs_id, d_scalars, m, count, out_xy, out_inf);
}


int typlonk_msm_g1_dev(typlonk_ctx* ctx, uint32_t srs_id, const typlonk_buf* scalars, size_t offset, size_t m,
                       uint64_t out_xy[12], uint8_t* out_inf) {
    if (!ctx || !scalars) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    if (offset > scalars->n || m > scalars->n - offset) return fail(ctx, TYPLONK_ERR_RANGE, "range outside buffer");
    HIPCHK(hipSetDevice(ctx->device));
    return msm_run(ctx, srs_id, scalars->d + offset, m, out_xy, out_inf);
}

int typlonk_msm_g1(typlonk_ctx* ctx, uint32_t srs_id, const uint64_t* scalars, size_t m, uint64_t out_xy[12],
                   uint8_t* out_inf) {
    if (!ctx || (!scalars && m)) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    HIPCHK(hipSetDevice(ctx->device));
    // validate the length before touching the device so the error matches the reference's assert
    const SrsEntry* srs = nullptr;
    int rc = msm_validate(ctx, srs_id, m, &srs);
    if (rc) return rc;
    size_t off, ml;
    srs->local_range(m, &off, &ml);
    if (ml) {  // only this entry's share of the coefficients crosses PCIe -- chunk by chunk, beside the kernels (msm_enqueue)
        if ((rc = ensure(ctx, ctx->scal, ml * sizeof(Fr)))) return rc;
    }
    return msm_run(ctx, srs_id, (const Fr*)ctx->scal.p, m, out_xy, out_inf, /*ptr_is_local=*/true, ml ? scalars + 4 * off : nullptr);
}

int typlonk_g1_sum_host(const uint64_t* xy, const uint8_t* inf, size_t count, uint64_t out_xy[12], uint8_t* out_inf) {
    if ((!xy && count) || !out_xy || !out_inf) return TYPLONK_ERR_INVALID_ARG;
    // arkworks' words ARE the 6 x 64-bit Montgomery form of g1_host64.hpp: no conversion in or out
    namespace H = h64;
    const H::Fq one = {{0x760900000002fffdull, 0xebf4000bc40c0002ull, 0x5f48985753c758baull, 0x77ce585370525745ull,
                        0x5c071a97a256ec6dull, 0x15f65ec3fa80e493ull}};  // 2^384 mod p
    H::Xyzz acc = H::inf();
    for (size_t i = 0; i < count; ++i) {
        if (inf && inf[i]) continue;
        H::Xyzz p;
        memcpy(p.x.v, xy + i * 12, 48);
        memcpy(p.y.v, xy + i * 12 + 6, 48);
        p.zz = one;
        p.zzz = one;
        acc = H::xyzz_add(acc, p);
    }
    if (H::xyzz_to_affine(acc, out_xy)) *out_inf = 0;
    else write_affine_out(G1Affine::inf(), out_xy, out_inf);
    return TYPLONK_OK;
}

int typlonk_g1_fold_records_host(const uint64_t* records, size_t world, size_t count, uint64_t* out_xy, uint8_t* out_inf,
                                 int* failed_rank) {
    static_assert(COMM_REC == TYPLONK_COMM_RECORD_WORDS, "record layout");
    if (!records || !world || ((!out_xy || !out_inf) && count)) return TYPLONK_ERR_INVALID_ARG;
    for (size_t r = 0; r < world; ++r)
        for (size_t i = 0; i < count; ++i)
            if (records[(r * count + i) * COMM_REC + 12] >> 32) {
                if (failed_rank) *failed_rank = (int)r;
                return TYPLONK_ERR_COMM;
            }
    // every point: the ranks' partial sums added in rank order (mixed additions: the records are affine), then ONE
    // inversion for all `count` results -- 97 -> 40 us for nine points from eight ranks, the same canonical points
    namespace H = h64;
    const H::Fq one = {{0x760900000002fffdull, 0xebf4000bc40c0002ull, 0x5f48985753c758baull, 0x77ce585370525745ull,
                        0x5c071a97a256ec6dull, 0x15f65ec3fa80e493ull}};  // 2^384 mod p
    std::vector<H::Xyzz> sums(count, H::inf());
    for (size_t i = 0; i < count; ++i) {
        for (size_t r = 0; r < world; ++r) {   // all-gather layout: rank-major, `count` records per rank
            const uint64_t* rec = records + (r * count + i) * COMM_REC;
            if (rec[12] & 1u) continue;
            H::Fq x, y;
            memcpy(x.v, rec, 48);
            memcpy(y.v, rec + 6, 48);
            sums[i] = H::xyzz_madd(sums[i], x, y, one);
        }
    }
    std::vector<char> ok(count ? count : 1);
    H::xyzz_to_affine_batch(sums.data(), count, out_xy, ok.data());
    for (size_t i = 0; i < count; ++i) {
        if (ok[i]) out_inf[i] = 0;
        else write_affine_out(G1Affine::inf(), out_xy + 12 * i, out_inf + i);
    }
    return TYPLONK_OK;
}

int typlonk_msm_plan(typlonk_ctx* ctx, size_t m, uint32_t* window_bits, uint32_t* n_windows, uint64_t* group_ops) {
    (void)ctx;   // the plan of a plain MSM depends on the length only
    uint32_t c, W;
    msm_shape(m ? m : 1, &c, &W);
    if (window_bits) *window_bits = c;
    if (n_windows) *n_windows = W;
    // Pippenger operation count for this shape: one mixed add per (term, window), two adds per
    // bucket in the running-sum reduction, c doublings per window in the final combine.
    if (group_ops) *group_ops = (uint64_t)W * m + 2ull * W * (1ull << (c - 1)) + (uint64_t)c * (W - 1);
    return TYPLONK_OK;
}

