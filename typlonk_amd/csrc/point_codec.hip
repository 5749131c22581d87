// Wire format (include/typlonk.h): compressed G1 points decoded / encoded on the device, one thread per point, and the
// byte forms of compact proofs, verifying keys and SRS points built on them.  The per-point logic is point_codec.hpp, shared
// with the host path (ctx = NULL).
#include "host.hpp"
#include "msm_common.hpp"
#include "point_codec.hpp"
#include "host_checks.hpp"

using namespace ty;
using namespace tyh;

namespace ty {

__device__ __forceinline__ void pc_load_raw(const uint8_t* in, uint64_t i, uint32_t (&raw)[12]) {
    const uint4* q = reinterpret_cast<const uint4*>(in + i * 48);   // 48 i bytes from a 256-byte aligned base
    const uint4 a = q[0], b = q[1], c = q[2];
    const uint32_t w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
    for (int k = 0; k < 12; ++k) raw[k] = w[k];
}

struct DecodeArgs {
    const uint8_t* in;    // n * 48 bytes
    uint64_t n;
    uint32_t check_subgroup;
    uint32_t* pts;        // SRS records (PT_WORDS per point, internal form), or NULL
    uint32_t* xy;         // C-ABI points (24 words per point), or NULL
    uint8_t* inf;         // with xy
    uint8_t* status;      // n classes, or NULL
    unsigned long long* first_bad;   // (index << 8 | class) of the lowest rejected point, or NULL
};

__global__ __launch_bounds__(64) void g1_decode_kernel(DecodeArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    uint32_t raw[12];
    pc_load_raw(a.in, i, raw);
    uint32_t st;
    if (a.pts) {
        G1Affine p;
        st = g1_decode(raw, a.check_subgroup != 0, p);
        uint32_t* dst = a.pts + i * PT_WORDS;
        st_fq(dst, p.x);
        st_fq(dst + 12, p.y);
    } else {
        uint32_t xy[24];
        uint8_t inf;
        st = g1_decode_ark(raw, a.check_subgroup != 0, xy, inf);
        uint4* dst = reinterpret_cast<uint4*>(a.xy + i * 24);
#pragma unroll
        for (int k = 0; k < 6; ++k) dst[k] = make_uint4(xy[4 * k], xy[4 * k + 1], xy[4 * k + 2], xy[4 * k + 3]);
        a.inf[i] = inf;
    }
    if (a.status) a.status[i] = (uint8_t)st;
    if (st && a.first_bad) atomicMin(a.first_bad, (unsigned long long)((i << 8) | st));
}

// canonicalisation out of the Montgomery form, a compare of y against (p - 1) / 2 and a byte swap per point
__global__ __launch_bounds__(64) void g1_encode_kernel(const uint32_t* pts, uint64_t n, uint8_t* out) {
    const uint64_t i = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const G1Affine p = ld_affine(pts, i);
    uint32_t raw[12];
    g1_encode(p, raw);
    uint4* dst = reinterpret_cast<uint4*>(out + i * 48);
#pragma unroll
    for (int k = 0; k < 3; ++k) dst[k] = make_uint4(raw[4 * k], raw[4 * k + 1], raw[4 * k + 2], raw[4 * k + 3]);
}

}  // namespace ty

namespace {

namespace P = typlonk::pairing;

const char* class_name(uint32_t cls) {
    switch (cls) {
        case TYPLONK_POINT_ENCODING: return "bad encoding (flags)";
        case TYPLONK_POINT_X_RANGE: return "x >= p";
        case TYPLONK_POINT_NOT_ON_CURVE: return "not on the curve";
        case TYPLONK_POINT_NOT_IN_SUBGROUP: return "not in the subgroup of order r";
        case TYPLONK_SCALAR_RANGE: return "scalar >= r";
    }
    return "unknown";
}

// ---- host path of the point codec ----
void host_decode(const uint8_t* in, size_t count, bool check_subgroup, uint64_t* xy, uint8_t* inf, uint8_t* status) {
    for (size_t i = 0; i < count; ++i) {
        uint32_t raw[12], w[24];
        memcpy(raw, in + 48 * i, 48);
        uint8_t f;
        const uint32_t st = g1_decode_ark(raw, check_subgroup, w, f);
        memcpy(xy + 12 * i, w, 96);
        inf[i] = f;
        if (status) status[i] = (uint8_t)st;
    }
}
// C-ABI point -> 48 bytes; false: a coordinate is not a canonical residue
bool host_encode(const uint64_t* xy, uint8_t inf, uint8_t* out) {
    G1Affine a = G1Affine::inf();
    if (!inf) {
        if (!fq_canonical(xy) || !fq_canonical(xy + 6)) return false;
        uint32_t w[12];
        memcpy(w, xy, 48);
        a.x = fq30_from_ark(w);
        memcpy(w, xy + 6, 48);
        a.y = fq30_from_ark(w);
        // (0, 0) is the internal identity and not a curve point: it has no encoding of its own
        if (a.is_inf()) return false;
    }
    uint32_t raw[12];
    g1_encode(a, raw);
    memcpy(out, raw, 48);
    return true;
}

// ---- Fr ----
bool fr_encode(const uint64_t l[4], uint8_t out[32]) {
    if (!fr_canonical(l)) return false;
    Fr m;
    memcpy(m.v, l, 32);
    const Fr c = fe_from_mont(m);
    memcpy(out, c.v, 32);
    return true;
}
bool fr_decode(const uint8_t in[32], uint64_t l[4]) {
    uint64_t c[4];
    memcpy(c, in, 32);
    if (!fr_canonical(c)) {
        memset(l, 0, 32);
        return false;
    }
    Fr x;
    memcpy(x.v, c, 32);
    const Fr m = fe_to_mont(x);
    memcpy(l, m.v, 32);
    return true;
}

// ---- Fq / Fq2 on the host (arkworks residues): square roots for the G2 point of a key ----
using HQ = h64::Fq;
HQ hq_pow(const HQ& a, const uint64_t (&e)[6]) {
    HQ acc{};
    bool started = false;
    for (int w = 5; w >= 0; --w)
        for (int b = 63; b >= 0; --b) {
            if (started) acc = h64::sqr(acc);
            if ((e[w] >> b) & 1ull) {
                acc = started ? h64::mul(acc, a) : a;
                started = true;
            }
        }
    return acc;
}
// a square root of a, if a is a square
bool hq_sqrt(const HQ& a, HQ* out) {
    static const uint64_t E[6] = {0xee7fbfffffffeaabull, 0x07aaffffac54ffffull, 0xd9cc34a83dac3d89ull,
                                  0xd91dd2e13ce144afull, 0x92c6e9ed90d2eb35ull, 0x0680447a8e5ff9a6ull};   // (p + 1) / 4
    const HQ r = hq_pow(a, E);
    *out = r;
    return h64::eq(h64::sqr(r), a);
}
HQ hq_of(const P::Fq& a) { return P::q64(a); }
// canonical integer of a residue > (p - 1) / 2
bool hq_is_high(const HQ& a) {
    static const uint64_t HALF[6] = {0xdcff7fffffffd555ull, 0x0f55ffff58a9ffffull, 0xb39869507b587b12ull,
                                     0xb23ba5c279c2895full, 0x258dd3db21a5d66bull, 0x0d0088f51cbff34dull};   // (p - 1) / 2
    const P::Fq c = fe_from_mont(P::q32(a));
    uint64_t l[6];
    memcpy(l, c.v, 48);
    for (int i = 5; i >= 0; --i)
        if (l[i] != HALF[i]) return l[i] > HALF[i];
    return false;
}
bool hq_is_zero(const HQ& a) { return h64::is_zero(a); }
// square root in Fq2 = Fq[u] / (u^2 + 1) by the norm: for a = a0 + a1 u, with s^2 = a0^2 + a1^2 and t = (a0 +- s) / 2 a square,
// x0 = sqrt(t), x1 = a1 / (2 x0).  The candidate is squared and compared, so a wrong branch cannot pass.
bool f2_sqrt(const P::Fq2& a, P::Fq2* out) {
    const HQ a0 = hq_of(a.a), a1 = hq_of(a.b);
    const HQ zero{};
    HQ x0 = zero, x1 = zero;
    if (hq_is_zero(a1)) {
        if (!hq_sqrt(a0, &x0)) {   // a0 is not a square: -a0 is (p = 3 mod 4), and (x u)^2 = -x^2
            x0 = zero;
            if (!hq_sqrt(h64::sub(zero, a0), &x1)) return false;
        }
    } else {
        HQ s;
        if (!hq_sqrt(h64::add(h64::sqr(a0), h64::sqr(a1)), &s)) return false;
        const HQ half = h64::inv(hq_of(P::fq_from_u64(2)));
        HQ t = h64::mul(h64::add(a0, s), half);
        if (!hq_sqrt(t, &x0)) {
            t = h64::mul(h64::sub(a0, s), half);
            if (!hq_sqrt(t, &x0)) return false;
        }
        if (hq_is_zero(x0)) return false;
        x1 = h64::mul(a1, h64::inv(h64::dbl(x0)));
    }
    const P::Fq2 r{P::q32(x0), P::q32(x1)};
    if (!(P::f2_mul(r, r) == a)) return false;
    *out = r;
    return true;
}
bool g2_y_is_high(const P::Fq2& y) { return y.b.is_zero() ? hq_is_high(hq_of(y.a)) : hq_is_high(hq_of(y.b)); }
// 48 big-endian bytes (flags already cleared) -> residue; false: >= p
bool fq_from_be(const uint8_t* in, uint8_t top_mask, P::Fq* out) {
    uint64_t l[6];
    for (int i = 0; i < 6; ++i) {
        uint64_t v = 0;
        for (int b = 0; b < 8; ++b) {
            uint8_t byte = in[8 * (5 - i) + b];
            if (i == 5 && b == 0) byte &= top_mask;
            v = (v << 8) | byte;
        }
        l[i] = v;
    }
    if (!fq_canonical(l)) return false;
    P::Fq c;
    memcpy(c.v, l, 48);
    *out = fe_to_mont(c);
    return true;
}
void fq_to_be(const P::Fq& a, uint8_t* out) {
    const P::Fq c = fe_from_mont(a);
    uint64_t l[6];
    memcpy(l, c.v, 48);
    for (int i = 0; i < 6; ++i)
        for (int b = 0; b < 8; ++b) out[8 * (5 - i) + b] = (uint8_t)(l[i] >> (8 * (7 - b)));
}
void g2_encode(const P::G2Affine& q, uint8_t out[96]) {
    fq_to_be(q.x.b, out);
    fq_to_be(q.x.a, out + 48);
    out[0] |= 0x80u | (g2_y_is_high(q.y) ? 0x20u : 0u);
}
uint32_t g2_decode(const uint8_t in[96], bool check_subgroup, uint64_t g2s_xy[24]) {
    memset(g2s_xy, 0, 24 * 8);
    const uint8_t flags = in[0] >> 5;
    if (!(flags & 4u)) return TYPLONK_POINT_ENCODING;
    if (flags & 2u) return TYPLONK_POINT_ENCODING;   // a key's [s]G2 is finite (and infinity with other bits is malformed anyway)
    P::G2Affine q;
    if (!fq_from_be(in, 0x1fu, &q.x.b) || !fq_from_be(in + 48, 0xffu, &q.x.a)) return TYPLONK_POINT_X_RANGE;
    const P::Fq four = P::fq_from_u64(4);
    const P::Fq2 rhs = P::f2_add(P::f2_mul(P::f2_mul(q.x, q.x), q.x), P::Fq2{four, four});
    if (!f2_sqrt(rhs, &q.y)) return TYPLONK_POINT_NOT_ON_CURVE;
    if (g2_y_is_high(q.y) != ((flags & 1u) != 0)) q.y = P::f2_neg(q.y);
    q.infinity = false;
    if (check_subgroup) {
        static const uint32_t R_WORDS[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u,
                                            0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
        if (!P::g2_mul_words(q, R_WORDS).infinity) return TYPLONK_POINT_NOT_IN_SUBGROUP;
    }
    memcpy(g2s_xy, q.x.a.v, 48);
    memcpy(g2s_xy + 6, q.x.b.v, 48);
    memcpy(g2s_xy + 12, q.y.a.v, 48);
    memcpy(g2s_xy + 18, q.y.b.v, 48);
    return 0;
}

// count points through one launch into C-ABI form (d_in may alias nothing)
int device_decode(typlonk_ctx* ctx, const uint8_t* in, size_t count, bool check_subgroup, uint64_t* xy, uint8_t* inf,
                  uint8_t* status) {
    HIPCHK(hipSetDevice(ctx->device));
    DevGuard guard;
    uint8_t* d_in = nullptr;
    uint32_t* d_xy = nullptr;
    uint8_t* d_flags = nullptr;   // inf then status
    HIPCHK(hipMalloc((void**)&d_in, count * 48));
    guard.add(d_in);
    HIPCHK(hipMalloc((void**)&d_xy, count * 96));
    guard.add(d_xy);
    HIPCHK(hipMalloc((void**)&d_flags, 2 * count));
    guard.add(d_flags);
    HIPCHK(hipMemcpyAsync(d_in, in, count * 48, hipMemcpyHostToDevice, ctx->stream));
    DecodeArgs a{};
    a.in = d_in;
    a.n = count;
    a.check_subgroup = check_subgroup ? 1u : 0u;
    a.xy = d_xy;
    a.inf = d_flags;
    a.status = d_flags + count;
    hipLaunchKernelGGL(g1_decode_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, ctx->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(xy, d_xy, count * 96, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(inf, d_flags, count, hipMemcpyDeviceToHost, ctx->stream));
    if (status) HIPCHK(hipMemcpyAsync(status, d_flags + count, count, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return TYPLONK_OK;
}

int decode_points(typlonk_ctx* ctx, const uint8_t* in, size_t count, uint32_t flags, uint64_t* xy, uint8_t* inf, uint8_t* status) {
    const bool check = !(flags & TYPLONK_DECODE_SKIP_SUBGROUP);
    if (!count) return TYPLONK_OK;
    if (!ctx) {
        host_decode(in, count, check, xy, inf, status);
        return TYPLONK_OK;
    }
    return device_decode(ctx, in, count, check, xy, inf, status);
}

// the nine points of a compact proof in wire order
struct PointRef {
    uint64_t* xy;
    uint8_t* inf;
};
void proof_points(typlonk_proof_compact& p, PointRef (&out)[9]) {
    for (int i = 0; i < 3; ++i) out[i] = {p.commit_xy[i], &p.commit_inf[i]};
    out[3] = {p.z_xy, &p.z_inf};
    for (int i = 0; i < 3; ++i) out[4 + i] = {p.t_xy[i], &p.t_inf[i]};
    for (int i = 0; i < 2; ++i) out[7 + i] = {p.w_xy[i], &p.w_inf[i]};
}
constexpr int PROOF_POINTS = 9, PROOF_SCALARS = 7;
static_assert(PROOF_POINTS * 48 + PROOF_SCALARS * 32 == TYPLONK_PROOF_COMPACT_BYTES, "proof layout");
static_assert(4 + 3 * 32 + 9 * 48 + 96 == TYPLONK_VK_WIRE_BYTES, "key layout");

}  // namespace

int typlonk_g1_compress(const uint64_t* xy, const uint8_t* inf, size_t count, uint8_t* out) {
    if (!count) return TYPLONK_OK;
    if (!xy || !out) return TYPLONK_ERR_INVALID_ARG;
    std::vector<uint8_t> buf(count * 48);   // staged: a refused call leaves `out` as it was
    for (size_t i = 0; i < count; ++i)
        if (!host_encode(xy + 12 * i, inf ? inf[i] : 0, &buf[48 * i])) return TYPLONK_ERR_INVALID_ARG;
    memcpy(out, buf.data(), buf.size());
    return TYPLONK_OK;
}

int typlonk_g1_decompress(typlonk_ctx* ctx, const uint8_t* bytes, size_t count, uint32_t flags, uint64_t* xy, uint8_t* inf,
                          uint8_t* status) {
    if (!count) return TYPLONK_OK;
    if (!bytes || !xy || !inf) return ctx ? fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument") : TYPLONK_ERR_INVALID_ARG;
    return decode_points(ctx, bytes, count, flags, xy, inf, status);
}

int typlonk_srs_load_compressed(typlonk_ctx* ctx, const uint8_t* bytes, size_t len, uint32_t flags, uint32_t* srs_id,
                                size_t* first_bad) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    if (!srs_id || (!bytes && len)) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    if (len % 48) return fail(ctx, TYPLONK_ERR_LENGTH, "a compressed SRS is a multiple of 48 bytes");
    const size_t n = len / 48;
    HIPCHK(hipSetDevice(ctx->device));
    SrsEntry e;
    e.len = n;
    DevGuard guard;
    HIPCHK(hipMalloc((void**)&e.d_points, std::max<size_t>(n, 1) * PT_WORDS * 4));
    guard.add(e.d_points);
    if (n) {
        DevGuard tmp;   // freed on every path out of this block
        uint8_t* d_in = nullptr;
        unsigned long long* d_bad = nullptr;
        HIPCHK(hipMalloc((void**)&d_in, len));
        tmp.add(d_in);
        HIPCHK(hipMalloc((void**)&d_bad, 8));
        tmp.add(d_bad);
        HIPCHK(hipMemcpyAsync(d_in, bytes, len, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemsetAsync(d_bad, 0xff, 8, ctx->stream));
        DecodeArgs a{};
        a.in = d_in;
        a.n = n;
        a.check_subgroup = (flags & TYPLONK_DECODE_SKIP_SUBGROUP) ? 0u : 1u;
        a.pts = e.d_points;
        a.first_bad = d_bad;
        hipLaunchKernelGGL(g1_decode_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, a);
        HIPCHK(hipGetLastError());
        unsigned long long bad = 0;
        HIPCHK(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (bad != ~0ull) {
            if (first_bad) *first_bad = (size_t)(bad >> 8);
            return fail(ctx, TYPLONK_ERR_INVALID_ARG,
                        "compressed SRS point " + std::to_string(bad >> 8) + " rejected: " + class_name((uint32_t)(bad & 0xff)));
        }
    }
    guard.dismiss();
    const uint32_t id = ctx->next_srs++;
    ctx->srs[id] = e;
    *srs_id = id;
    return TYPLONK_OK;
}

int typlonk_srs_download_compressed(typlonk_ctx* ctx, uint32_t srs_id, size_t offset, size_t count, uint8_t* out) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    if (!out && count) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    auto it = ctx->srs.find(srs_id);
    if (it == ctx->srs.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown srs id");
    if (offset > it->second.len || count > it->second.len - offset) return fail(ctx, TYPLONK_ERR_RANGE, "range outside SRS");
    if (!count) return TYPLONK_OK;
    HIPCHK(hipSetDevice(ctx->device));
    DevGuard guard;
    uint8_t* d_out = nullptr;
    HIPCHK(hipMalloc((void**)&d_out, count * 48));
    guard.add(d_out);
    hipLaunchKernelGGL(g1_encode_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, ctx->stream,
                       (const uint32_t*)(it->second.d_points + offset * PT_WORDS), (uint64_t)count, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_out, count * 48, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return TYPLONK_OK;
}

int typlonk_proof_compact_to_bytes(const typlonk_proof_compact* proof, uint8_t out[TYPLONK_PROOF_COMPACT_BYTES]) {
    if (!proof || !out) return TYPLONK_ERR_INVALID_ARG;
    typlonk_proof_compact p = *proof;
    PointRef pts[9];
    proof_points(p, pts);
    uint8_t buf[TYPLONK_PROOF_COMPACT_BYTES];
    for (int i = 0; i < PROOF_POINTS; ++i) {
        if (!g1_on_curve(pts[i].xy, *pts[i].inf) || !host_encode(pts[i].xy, *pts[i].inf, buf + 48 * i)) return TYPLONK_ERR_INVALID_ARG;
    }
    for (int i = 0; i < PROOF_SCALARS; ++i)
        if (!fr_encode(p.evals[i], buf + 48 * PROOF_POINTS + 32 * i)) return TYPLONK_ERR_INVALID_ARG;
    memcpy(out, buf, sizeof(buf));
    return TYPLONK_OK;
}

int typlonk_vk_to_bytes(const typlonk_vk* vk, uint8_t out[TYPLONK_VK_WIRE_BYTES]) {
    if (!vk || !out) return TYPLONK_ERR_INVALID_ARG;
    if (vk->log_n < 1 || vk->log_n > TYPLONK_MAX_PROVER_LOG_N) return TYPLONK_ERR_DOMAIN;
    uint8_t buf[TYPLONK_VK_WIRE_BYTES];
    for (int i = 0; i < 4; ++i) buf[i] = (uint8_t)(vk->log_n >> (8 * i));
    uint8_t* p = buf + 4;
    for (int i = 0; i < 3; ++i, p += 32)
        if (!fr_encode(vk->cosets[i], p)) return TYPLONK_ERR_INVALID_ARG;
    for (int i = 0; i < 9; ++i, p += 48) {
        const uint64_t* xy = i < 8 ? vk->commit_xy[i] : vk->srs0_xy;
        const uint8_t inf = i < 8 ? vk->commit_inf[i] : vk->srs0_inf;
        if (!g1_on_curve(xy, inf) || !host_encode(xy, inf, p)) return TYPLONK_ERR_INVALID_ARG;
    }
    P::G2Affine q;
    if (!g2_from_limbs(vk->g2s_xy, &q)) return TYPLONK_ERR_INVALID_ARG;
    g2_encode(q, p);
    memcpy(out, buf, sizeof(buf));
    return TYPLONK_OK;
}

int typlonk_vk_from_bytes(const uint8_t bytes[TYPLONK_VK_WIRE_BYTES], uint32_t flags, typlonk_vk* vk, uint32_t* status) {
    if (!bytes || !vk) return TYPLONK_ERR_INVALID_ARG;
    if (status) *status = 0;
    typlonk_vk out;
    memset(&out, 0, sizeof(out));
    out.log_n = (uint32_t)bytes[0] | ((uint32_t)bytes[1] << 8) | ((uint32_t)bytes[2] << 16) | ((uint32_t)bytes[3] << 24);
    if (out.log_n < 1 || out.log_n > TYPLONK_MAX_PROVER_LOG_N) return TYPLONK_ERR_DOMAIN;
    const uint8_t* p = bytes + 4;
    uint32_t st = 0;
    for (int i = 0; i < 3; ++i, p += 32)
        if (!fr_decode(p, out.cosets[i]) && !st) st = TYPLONK_DECODE_STATUS(TYPLONK_SCALAR_RANGE, i);
    uint64_t xy[9 * 12];
    uint8_t inf[9], cls[9];
    host_decode(p, 9, !(flags & TYPLONK_DECODE_SKIP_SUBGROUP), xy, inf, cls);
    for (int i = 0; i < 9; ++i)
        if (cls[i] && !st) st = TYPLONK_DECODE_STATUS(cls[i], 3 + i);
    memcpy(out.commit_xy, xy, 8 * 96);
    memcpy(out.commit_inf, inf, 8);
    memcpy(out.srs0_xy, xy + 8 * 12, 96);
    out.srs0_inf = inf[8];
    p += 9 * 48;
    if (!st) {   // (the G2 subgroup check is the slow part of a key: not spent on a key that is already refused)
        const uint32_t c2 = g2_decode(p, !(flags & TYPLONK_DECODE_SKIP_SUBGROUP), out.g2s_xy);
        if (c2) st = TYPLONK_DECODE_STATUS(c2, 12);
    }
    if (st) {
        if (status) *status = st;
        return TYPLONK_ERR_INVALID_ARG;
    }
    *vk = out;
    return TYPLONK_OK;
}

int typlonk_proof_compact_from_bytes(typlonk_ctx* ctx, const uint8_t* bytes, size_t count, uint32_t flags,
                                     typlonk_proof_compact* proofs, uint32_t* status) {
    if (!count) return TYPLONK_OK;
    if (!bytes || !proofs || !status) return ctx ? fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument") : TYPLONK_ERR_INVALID_ARG;
    // the 9 * count points, gathered for one launch
    std::vector<uint8_t> in(count * PROOF_POINTS * 48), inf(count * PROOF_POINTS), cls(count * PROOF_POINTS);
    std::vector<uint64_t> xy(count * PROOF_POINTS * 12);
    for (size_t k = 0; k < count; ++k) memcpy(&in[k * PROOF_POINTS * 48], bytes + k * TYPLONK_PROOF_COMPACT_BYTES, PROOF_POINTS * 48);
    const int rc = decode_points(ctx, in.data(), count * PROOF_POINTS, flags, xy.data(), inf.data(), cls.data());
    if (rc) return rc;
    for (size_t k = 0; k < count; ++k) {
        typlonk_proof_compact p;
        memset(&p, 0, sizeof(p));
        PointRef pts[9];
        proof_points(p, pts);
        uint32_t st = 0;
        for (int i = 0; i < PROOF_POINTS; ++i) {
            const size_t j = k * PROOF_POINTS + i;
            memcpy(pts[i].xy, &xy[12 * j], 96);
            *pts[i].inf = inf[j];
            if (cls[j] && !st) st = TYPLONK_DECODE_STATUS(cls[j], i);
        }
        const uint8_t* s = bytes + k * TYPLONK_PROOF_COMPACT_BYTES + PROOF_POINTS * 48;
        for (int i = 0; i < PROOF_SCALARS; ++i)
            if (!fr_decode(s + 32 * i, p.evals[i]) && !st) st = TYPLONK_DECODE_STATUS(TYPLONK_SCALAR_RANGE, PROOF_POINTS + i);
        if (st) {   // all identities / zeros
            for (int i = 0; i < PROOF_POINTS; ++i) {
                uint8_t f;
                write_affine_out(G1Affine::inf(), pts[i].xy, &f);
                *pts[i].inf = f;
            }
            memset(p.evals, 0, sizeof(p.evals));
        }
        proofs[k] = p;
        status[k] = st;
    }
    return TYPLONK_OK;
}

int typlonk_verify_compact_bytes(typlonk_ctx* ctx, const typlonk_vk* vk, const uint8_t* bytes, size_t count,
                                 const uint64_t* const* pi, const size_t* pi_len, uint32_t flags, uint8_t* ok) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    if (count == 0) return TYPLONK_OK;
    if (!vk || !bytes || !ok) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    memset(ok, 0, count);
    // the key and the public-input arguments, as the verifier judges them: whichever proofs decode
    P::G2Affine g2s;
    int rc = verify_compact_check_args(ctx, vk, count, pi, pi_len, &g2s);
    if (rc) return rc;
    std::vector<typlonk_proof_compact> all(count);
    std::vector<uint32_t> st(count);
    rc = typlonk_proof_compact_from_bytes(ctx, bytes, count, flags, all.data(), st.data());
    if (rc) return rc;
    // the decodable proofs, with their public inputs, go to the one verifier; the others never reach it
    std::vector<typlonk_proof_compact> good;
    std::vector<const uint64_t*> gpi;
    std::vector<size_t> glen, index;
    for (size_t k = 0; k < count; ++k) {
        if (st[k]) continue;
        const size_t len = pi_len ? pi_len[k] : 0;
        good.push_back(all[k]);
        gpi.push_back(len ? pi[k] : nullptr);
        glen.push_back(len);
        index.push_back(k);
    }
    if (good.empty()) return TYPLONK_OK;
    std::vector<uint8_t> gok(good.size(), 0);
    rc = typlonk_verify_compact(ctx, vk, good.data(), good.size(), gpi.data(), glen.data(), gok.data());
    if (rc) return rc;
    for (size_t j = 0; j < good.size(); ++j) ok[index[j]] = gok[j];
    return TYPLONK_OK;
}
