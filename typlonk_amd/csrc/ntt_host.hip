// libtyplonk_hip.so -- NTT host side: the table cache, the executor of ntt_plan (ntt_plan.hpp), the typlonk_ntt_* entry points
// Part of the host driver of include/typlonk.h (see host.hpp for the shared state).  There is deliberately no CPU compute
// fallback: without a HIP device typlonk_init fails with TYPLONK_ERR_NO_DEVICE.
#include "host.hpp"
#include "fr30.hpp"

using namespace ty;
using namespace tyh;

namespace tyh {

// ---- host Fr helpers ---------------------------------------------------------------------------
Fr fr_root_of_unity_2_32() {
    // ark-bls12-381 FrParameters::TWO_ADIC_ROOT_OF_UNITY = 7^((r-1)/2^32), canonical value
    Fr c;
    const uint32_t limbs[8] = {0x439f0d2bu, 0x3829971fu, 0x8c2280b9u, 0xb6368350u,
                               0x22c813b4u, 0xd09b6819u, 0xdfe81f20u, 0x16a2a19eu};
    for (int i = 0; i < 8; ++i) c.v[i] = limbs[i];
    return fe_to_mont(c);
}

// generator of the size-2^log_n domain (ark-poly Radix2EvaluationDomain::group_gen)
Fr fr_domain_root(uint32_t log_n) {
    Fr w = fr_root_of_unity_2_32();
    for (uint32_t i = log_n; i < 32; ++i) w = fe_sqr(w);
    return w;
}
// its inverse (group_gen_inv) from the inverse of the 2^32-th root: squarings instead of a field inversion per call
Fr fr_domain_root_inv(uint32_t log_n) {
    Fr c;
    const uint32_t limbs[8] = {0x3cf19a78u, 0x0fb4d6e1u, 0xb566f833u, 0x6f67d4a2u, 0xa35d0168u, 0xed4f2f74u, 0x6e19c653u, 0x0538a6f6u};
    for (int i = 0; i < 8; ++i) c.v[i] = limbs[i];
    Fr w = fe_to_mont(c);
    for (uint32_t i = log_n; i < 32; ++i) w = fe_sqr(w);
    return w;
}
// (2^log_n)^-1 = ((r + 1) / 2)^log_n  (size_inv)
Fr fr_inv_pow2(uint32_t log_n) {
    Fr c;
    const uint32_t limbs[8] = {0x80000001u, 0x7fffffffu, 0x7fff2dffu, 0xa9ded201u, 0x04d0ec02u, 0x199cec04u, 0x94cebea4u, 0x39f6d3a9u};
    for (int i = 0; i < 8; ++i) c.v[i] = limbs[i];
    const Fr half = fe_to_mont(c);
    Fr x = Fr::one();
    for (uint32_t i = 0; i < log_n; ++i) x = fe_mul(x, half);
    return x;
}

Fr fr_from_u64(uint64_t x) {
    Fr c = Fr::zero();
    c.v[0] = (uint32_t)x;
    c.v[1] = (uint32_t)(x >> 32);
    return fe_to_mont(c);
}

int upload_table(typlonk_ctx* ctx, const std::string& key, const std::vector<Fr>& h, Table* out) {
    Table t;
    t.n = h.size();
    t.last_use = ++ctx->table_tick;
    HIPCHK(hipMalloc((void**)&t.d, h.size() * sizeof(Fr)));
    DevGuard g;
    g.add(t.d);
    HIPCHK(hipMemcpyAsync(t.d, h.data(), h.size() * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));  // h goes out of scope
    g.dismiss();
    ctx->tables[key] = t;
    *out = t;
    return TYPLONK_OK;
}

std::string fr_hex(const Fr& f) {
    char buf[80];
    snprintf(buf, sizeof(buf), "%08x%08x%08x%08x%08x%08x%08x%08x", f.v[7], f.v[6], f.v[5], f.v[4], f.v[3], f.v[2],
             f.v[1], f.v[0]);
    return buf;
}

// Full one-multiplication table built on the device from a two-level pair (launch_ntt_full_table); kept per
// context like every other table.  No room: *out stays empty and the kernel composes the factor from the two-level
// tables instead (sizes above 2^NTT_FULL_MAX_LOG entries -- 2^24 = 512 MB -- are not even asked for: ntt_plan.hpp).
int build_full_table(typlonk_ctx* ctx, const std::string& key, const NttTableReq& r, const Table& lo, const Table& hi, Table* out) {
    Table t;
    t.n = r.n;
    t.last_use = ++ctx->table_tick;
    hipError_t e = hipMalloc((void**)&t.d, r.n * sizeof(Fr));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return TYPLONK_OK;  // fall back to the two-level tables
    }
    launch_ntt_full_table(lo.d, hi.d, r.h, r.S, r.n, t.d, ctx->stream);
    {
        DevGuard g;
        g.add(t.d);
        HIPCHK(hipGetLastError());
        // built once per context: complete before it enters the cache, so that a later lookup from another stream
        // (typlonk_set_stream, the prover's extension lane) needs no ordering against the build
        HIPCHK(hipStreamSynchronize(ctx->stream));
        g.dismiss();
    }
    ctx->tables[key] = t;
    *out = t;
    return TYPLONK_OK;
}

// what the named bases and scales of a call's table requests (ntt_plan.hpp) stand for
struct NttValues {
    uint32_t log_n = 0;
    const uint64_t* shift = nullptr;
    std::string shift_hex;
    bool have_inv = false;
    Fr shift_inv;   // computed when the first table that needs it is BUILT: a resident coset group costs no field inversion
    NttValues(uint32_t lg, const uint64_t* g) : log_n(lg), shift(g) {
        if (g) shift_hex = fr_hex(shift_fr());
    }
    Fr shift_fr() const {
        Fr g;
        memcpy(g.v, shift, sizeof(g.v));
        return g;
    }
    Fr base(const NttTableReq& r) {
        Fr b = Fr::one();
        if (r.base == NTT_B_ROOT) b = fr_domain_root(r.base_log);
        if (r.base == NTT_B_ROOT_INV) b = fr_domain_root_inv(r.base_log);
        if (r.base == NTT_B_SHIFT) b = shift_fr();
        if (r.base == NTT_B_SHIFT_INV) {
            if (!have_inv) shift_inv = fe_inv(shift_fr());
            have_inv = true;
            b = shift_inv;
        }
        for (uint32_t i = 0; i < r.base_sqr; ++i) b = fe_sqr(b);
        return b;
    }
    Fr scale(const NttTableReq& r) const {
        const Fr c14 = fr_from_u64(1u << 14);
        if (r.scale == NTT_S_NINV) return fr_inv_pow2(log_n);
        if (r.scale == NTT_S_C14) return c14;
        if (r.scale == NTT_S_NINV_C14) return fe_mul(fr_inv_pow2(log_n), c14);
        return Fr::one();
    }
};

// THE table lookup: the cached table of a request, built first if the context does not hold it yet.  got = the tables of
// the requests before it in the same list (a full table is made from its pair).  An empty *out with TYPLONK_OK: a full
// table there was no room for.
int get_table(typlonk_ctx* ctx, const NttTableReq& r, NttValues& val, const Table* got, Table* out) {
    *out = Table{};
    const std::string key = ntt_key(r, val.shift_hex);
    auto it = ctx->tables.find(key);
    if (it != ctx->tables.end()) {
        it->second.last_use = ++ctx->table_tick;
        *out = it->second;
        return TYPLONK_OK;
    }
    if (r.kind == NTT_FULL) return build_full_table(ctx, key, r, got[r.lo], got[r.hi], out);
    const Fr base = val.base(r);
    Fr x = val.scale(r);
    std::vector<Fr> h;
    if (r.kind != NTT_POW30) {   // out[j] = scale * base^j
        h.resize(r.n);
        for (size_t j = 0; j < r.n; ++j) {
            h[j] = x;
            x = fe_mul(x, base);
        }
    } else {   // the same re-cut into nine 30-bit limbs on a 12-word (48-byte) stride -- what NttArith30::ldtw (ntt_kernels.hip) reads
        h.assign((12 * r.n + 7) / 8, Fr::zero());
        uint32_t* w = reinterpret_cast<uint32_t*>(h.data());
        for (size_t j = 0; j < r.n; ++j) {
            for (int i = 0; i < 9; ++i) {   // fr30_unpack (fr30.hpp) on the host
                const int bit = 30 * i, wi = bit >> 5, sh = bit & 31;
                uint32_t t = x.v[wi] >> sh;
                if (sh > 2 && wi + 1 < 8) t |= x.v[wi + 1] << (32 - sh);
                w[12 * j + i] = t & 0x3fffffffu;
            }
            x = fe_mul(x, base);
        }
    }
    return upload_table(ctx, key, h, out);
}

int domain_twiddles(typlonk_ctx* ctx, uint32_t log_n, const Fr** lo, const Fr** hi, uint32_t* h) {
    std::vector<NttTableReq> req;
    ntt_push_domain_twiddles(req, false, NTT_F32, 0, log_n);
    NttValues val(log_n, nullptr);
    Table t[2];
    for (int i = 0; i < 2; ++i)
        if (int rc = get_table(ctx, req[i], val, t, &t[i])) return rc;
    *lo = t[0].d;
    *hi = t[1].d;
    *h = req[1].base_sqr;
    return TYPLONK_OK;
}

// Coset tables are keyed by the caller's shift (ntt_plan.hpp, ntt_coset_group): a caller that varies the shift
// would otherwise grow HBM without bound.  Before a new group is built, drop least-recently-used groups until the
// cache is inside its limits (the quotient's generator 7 is looked up on every proof and therefore stays).
int evict_coset_tables(typlonk_ctx* ctx, const std::string& incoming_group, size_t incoming_bytes) {
    if (ctx->tables.count(incoming_group + ":lo")) return TYPLONK_OK;  // resident (the per-proof case)
    for (;;) {
        std::map<std::string, std::pair<uint64_t, size_t>> groups;  // group -> (last use, bytes)
        size_t bytes = 0;
        for (const auto& kv : ctx->tables) {
            const std::string grp = ntt_coset_group_of(kv.first);
            if (grp.empty()) continue;
            auto& g = groups[grp];
            g.first = std::max(g.first, kv.second.last_use);
            g.second += kv.second.n * sizeof(Fr);
            bytes += kv.second.n * sizeof(Fr);
        }
        if (groups.count(incoming_group)) return TYPLONK_OK;  // already resident: nothing new is built
        if (groups.size() < typlonk_ctx::COSET_GROUPS_MAX && bytes + incoming_bytes <= typlonk_ctx::COSET_BYTES_MAX)
            return TYPLONK_OK;
        if (groups.empty()) return TYPLONK_OK;
        std::string victim;
        uint64_t oldest = ~0ull;
        for (const auto& g : groups)
            if (g.second.first < oldest) {
                oldest = g.second.first;
                victim = g.first;
            }
        // kernels still reading the victim's tables: they may sit on a stream the context has since been moved away
        // from (typlonk_set_stream) or come from an un-synchronised *_devptr call, so the rare eviction waits for the
        // whole device rather than for the current stream only
        HIPCHK(hipDeviceSynchronize());
        for (auto it = ctx->tables.begin(); it != ctx->tables.end();) {
            if (ntt_coset_group_of(it->first) == victim) {
                (void)hipFree(it->second.d);
                it = ctx->tables.erase(it);
            } else {
                ++it;
            }
        }
    }
}

int ntt_run(typlonk_ctx* ctx, Fr* d_data, uint32_t log_n, int inverse, const uint64_t* coset_shift, bool sync, const Fr* short_in,
            uint64_t n_valid) {
    if (!d_data) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null data");
    return ntt_run_batch(ctx, &d_data, 1, log_n, inverse, coset_shift, sync, short_in ? &short_in : nullptr, n_valid);
}

// the pointer of NttPassArgs a table feeds.  The 30-bit kernel reads full tables only: the halves of its pairs feed nothing.
static void wire_table(NttPassArgs& a, const NttTableReq& r, const Table& t) {
    const bool lo = r.kind == NTT_PAIR_LO, hi = r.kind == NTT_PAIR_HI;
    if (r.form == NTT_F30 && (lo || hi)) return;
    switch (r.role) {
        case NTT_SUB:
            if (r.form == NTT_F30) a.sub_tw30 = reinterpret_cast<const uint32_t*>(t.d);
            else a.sub_tw = t.d;
            break;
        case NTT_TW: (lo ? a.tw_lo : hi ? a.tw_hi : a.tw_full) = t.d; break;
        case NTT_PRE: (lo ? a.pre_lo : hi ? a.pre_hi : a.pre_full) = t.d; break;
        case NTT_POST: (lo ? a.post_lo : hi ? a.post_hi : a.post_full) = t.d; break;
        case NTT_SCALE: a.scale = t.d; break;
    }
}

// `count` transforms of the same size, direction and coset in ONE sequence of pass launches: pass p of every vector is
// one launch whose grid is count x the tiles of one vector (NttPassArgs::in / out / blocks_per_vec), the tables are shared.
// The reference always transforms in groups -- the three wire columns (plonk/src/proof.rs:50), their re-evaluation
// (:113-115), the three sigmas (:334-338, :412-418), the five selectors (plonk/src/builder.rs:84-88) -- and a 2^20
// transform alone is one round of tiles on the chip (every CU loads, computes and stores in step); a launch with 3 x
// the tiles lets rounds overlap.  Bit-identical to `count` single calls (the same kernels on the same tiles).
// More vectors than the plan's group go through in groups.  Every decision is ntt_plan's (ntt_plan.hpp).
int ntt_run_batch(typlonk_ctx* ctx, Fr* const* d_data, size_t count, uint32_t log_n, int inverse, const uint64_t* coset_shift,
                  bool sync, const Fr* const* short_in, uint64_t n_valid) {
    // (the device is asked for its 144 KiB of LDS only by a transform that could use them)
    const bool rounds = ctx->prover_rounds_active != 0;
    const NttFacts facts{ctx->ntt_fr30, ctx->ntt_big, rounds, log_n == 20 && ctx->ntt_big != 0 && !rounds && ntt_big_tiles_available()};
    const NttPlan pl = ntt_plan(log_n, inverse != 0, coset_shift != nullptr, count, short_in != nullptr, facts);
    if (pl.status == NTT_PLAN_DOMAIN) return fail(ctx, TYPLONK_ERR_DOMAIN, "log_n > 32 (Fr two-adicity)");
    if (!d_data && count) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null data");
    for (size_t v = 0; v < count; ++v)
        if (!d_data[v]) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null data");
    if (pl.status == NTT_PLAN_EMPTY) return TYPLONK_OK;
    const uint64_t N = 1ull << log_n;
    if (int rc = ensure(ctx, ctx->ntt_scratch, pl.scratch_bytes)) return rc;
    Fr* const scratch = pl.scratch_bytes ? (Fr*)ctx->ntt_scratch.p : nullptr;

    // the tables, in the plan's order.  The 30-bit kernel's: until one of its full tables comes back empty -- the transform
    // then runs on the 8 x 32 kernel, which still lacks the full inter-pass tables only it looks up.
    NttValues val(log_n, coset_shift);
    if (coset_shift && pl.status == NTT_PLAN_OK)
        if (int rc = evict_coset_tables(ctx, ntt_coset_group(inverse != 0, log_n, val.shift_hex), (size_t)N * sizeof(Fr))) return rc;
    std::vector<Table> got(pl.tables.size());
    bool f30 = pl.f30_eligible, more30 = true;
    for (size_t i = 0; i < pl.tables.size(); ++i) {
        const NttTableReq& r = pl.tables[i];
        if (r.form == NTT_F30 ? !more30 : (r.unless30 && f30)) continue;
        if (int rc = get_table(ctx, r, val, got.data(), &got[i])) return rc;
        if (r.form == NTT_F30 && r.kind == NTT_FULL && !got[i].d) f30 = more30 = false;
    }
    const NttForm form = f30 ? NTT_F30 : NTT_F32;

    for (size_t g0 = 0; g0 < count; g0 += pl.group) {
        const size_t cnt = std::min(pl.group, count - g0);
        prof_begin(ctx);
        for (uint32_t p = 0; p < pl.P; ++p) {
            const NttPassPlan& ps = pl.pass[p];
            NttPassArgs a = ps.a;   // every scalar
            if (ps.short_in) a.n_valid = n_valid;
            for (size_t i = 0; i < pl.tables.size(); ++i)
                if (pl.tables[i].pass == p && pl.tables[i].form == form) wire_table(a, pl.tables[i], got[i]);
            for (size_t v = 0; v < cnt; ++v) {
                Fr* scr = scratch ? scratch + v * N : nullptr;
                a.in[v] = (p == 0) ? (short_in ? short_in[g0 + v] : d_data[g0 + v]) : scr;
                a.out[v] = a.last ? d_data[g0 + v] : scr;
            }
            const unsigned blocks = (unsigned)(a.blocks_per_vec * cnt);
            {
                static const char* names[4] = {"ntt_pass1", "ntt_pass2", "ntt_pass3", "ntt_pass4"};
                StageTimer st(ctx, names[p]);
                if (f30) launch_ntt_pass30(a, blocks, ps.threads, ps.lds[form], ctx->stream);
                else launch_ntt_pass(a, blocks, ps.threads, ps.lds[form], ctx->stream);
            }
            HIPCHK(hipGetLastError());
        }
        if (pl.P && (sync || (ctx->profiling && !ctx->prof_light))) HIPCHK(hipStreamSynchronize(ctx->stream));
        prof_collect(ctx);
    }
    return TYPLONK_OK;
}

}  // namespace tyh

// (entry points: C linkage comes from their declarations in include/typlonk.h)

int typlonk_ntt_fr_devptr(typlonk_ctx* ctx, void* d_data, uint32_t log_n, int inverse, const uint64_t* coset_shift) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    return ntt_run(ctx, (Fr*)d_data, log_n, inverse, coset_shift, /*sync=*/false);
}

int typlonk_ntt_fr_batch_devptr(typlonk_ctx* ctx, void* const* d_data, size_t count, uint32_t log_n, int inverse,
                                const uint64_t* coset_shift) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    if (!d_data && count) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    if (log_n > 32) return fail(ctx, TYPLONK_ERR_DOMAIN, "log_n > 32 (Fr two-adicity)");
    // the vectors are transformed in place and concurrently: two of them must not be the same (or overlapping) storage
    const uint64_t bytes = sizeof(Fr) << log_n;
    for (size_t i = 0; i < count; ++i) {
        if (!d_data[i]) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null data");
        for (size_t j = 0; j < i; ++j) {
            const uintptr_t a = (uintptr_t)d_data[i], b = (uintptr_t)d_data[j];
            if (a < b + bytes && b < a + bytes) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "batched transforms overlap");
        }
    }
    HIPCHK(hipSetDevice(ctx->device));
    return ntt_run_batch(ctx, reinterpret_cast<Fr* const*>(d_data), count, log_n, inverse, coset_shift, /*sync=*/false);
}

int typlonk_ntt_fr_dev(typlonk_ctx* ctx, typlonk_buf* buf, size_t offset, uint32_t log_n, int inverse,
                       const uint64_t* coset_shift) {
    if (!ctx || !buf) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    if (log_n > 32) return fail(ctx, TYPLONK_ERR_DOMAIN, "log_n > 32 (Fr two-adicity)");
    const uint64_t N = 1ull << log_n;
    if (offset > buf->n || N > buf->n - offset) return fail(ctx, TYPLONK_ERR_RANGE, "range outside buffer");
    HIPCHK(hipSetDevice(ctx->device));
    return ntt_run(ctx, buf->d + offset, log_n, inverse, coset_shift, /*sync=*/false);
}

int typlonk_ntt_fr(typlonk_ctx* ctx, uint64_t* data, uint32_t log_n, int inverse, const uint64_t* coset_shift) {
    if (!ctx || !data) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    if (log_n > 32) return fail(ctx, TYPLONK_ERR_DOMAIN, "log_n > 32 (Fr two-adicity)");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t bytes = ((size_t)1 << log_n) * sizeof(Fr);
    int rc = ensure(ctx, ctx->ntt_io, bytes);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(ctx->ntt_io.p, data, bytes, hipMemcpyHostToDevice, ctx->stream));
    rc = ntt_run(ctx, (Fr*)ctx->ntt_io.p, log_n, inverse, coset_shift);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(data, ctx->ntt_io.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return TYPLONK_OK;
}

