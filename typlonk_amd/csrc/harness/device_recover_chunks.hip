// Test-only device harness over the kernels of typlonk_recover_chunks (tests/test_gpu_recover_chunks_kernels.py).
//
// recover_chunks.hip is compiled here as a unit, exactly as the library compiles it (same flags, no extra defines), and each
// entry point runs one of its launchers alone on caller-made inputs: the vanishing products with a NAMED number of slices --
// through the library a shape only ever reaches the plan's own -- and the inversion behind them, the scatter, the scale, and
// the finish.  Every device buffer is allocated at exactly the size a launcher may touch between two guard bands, and nothing is
// launched on a shape a kernel could leave its buffers with: the checks run on the host before the first HIP call.
// Not linked into libtyplonk_hip.so.  It lives beside the unit it wraps, as device_verify_chunks.hip does.
#include "../recover_chunks.hip"

#include <vector>

using namespace ty;

namespace {

constexpr size_t GUARD_BYTES = 4096;
constexpr int GUARD_FILL = 0xA5;   // every allocation starts out as this byte, body and bands

struct Buf {
    char* base = nullptr;
    size_t bytes = 0;
    void* p() const { return base + GUARD_BYTES; }
    Fr* fr() const { return static_cast<Fr*>(p()); }
    // a band, n bytes copied from src (or left as the fill), a band
    hipError_t make(const void* src, size_t n) {
        bytes = n;
        hipError_t e = hipMalloc((void**)&base, n + 2 * GUARD_BYTES);
        if (e == hipSuccess) e = hipMemset(base, GUARD_FILL, n + 2 * GUARD_BYTES);
        if (e == hipSuccess && src && n) e = hipMemcpy(p(), src, n, hipMemcpyHostToDevice);
        return e;
    }
    // the body to the host (dst may be NULL), and whether both bands are still the fill
    bool fetch(void* dst, hipError_t& e) const {
        std::vector<unsigned char> band(2 * GUARD_BYTES);
        if (e == hipSuccess && dst && bytes) e = hipMemcpy(dst, p(), bytes, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(band.data(), base, GUARD_BYTES, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(band.data() + GUARD_BYTES, base + GUARD_BYTES + bytes, GUARD_BYTES, hipMemcpyDeviceToHost);
        bool ok = e == hipSuccess;
        for (size_t i = 0; ok && i < 2 * GUARD_BYTES; ++i) ok = band[i] == GUARD_FILL;
        return ok;
    }
    ~Buf() {
        if (base) (void)hipFree(base);
    }
};

Fr fr_of(const uint32_t* w) {
    Fr f;
    for (int i = 0; i < 8; ++i) f.v[i] = w[i];
    return f;
}

hipError_t finish_launches() {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return e;
}

}  // namespace

// Fr values are 8 words each, Montgomery.  pw: the r = 2^log_r values a_k; missing_idx: `missing` < r indices below r; gl: g^l.
// slices = 0: the plan's own.  Out: z = Zd (r) then Zc (r); zc_inv: r, the inversion run over a copy of Zc; *slices_used,
// *tile = what the plan made of the request.  *guard = 1: every band is still the fill.  Returns the HIP error code,
// hipErrorInvalidValue -- before anything touches the device -- for a shape outside the launchers' contract.
extern "C" int drc_vanish(const uint32_t* pw, uint32_t log_r, const uint32_t* missing_idx, uint64_t missing, const uint32_t* gl, uint32_t slices,
                          uint32_t* z, uint32_t* zc_inv, uint32_t* slices_used, uint32_t* tile, uint32_t* guard) {
    if (!pw || !missing_idx || !gl || !z || !zc_inv || !slices_used || !tile || !guard) return (int)hipErrorInvalidValue;
    if (log_r < 1 || log_r > 12 || slices > 4096) return (int)hipErrorInvalidValue;
    const uint64_t r = 1ull << log_r;
    if (missing >= r) return (int)hipErrorInvalidValue;   // (a call names at least one coset)
    for (uint64_t j = 0; j < missing; ++j)
        if (missing_idx[j] >= r) return (int)hipErrorInvalidValue;
    const RecoverChunksPlan q = recover_chunks_plan(log_r, 0, 1, r - missing, 1, true, false, slices);
    if (q.missing != missing || (uint64_t)q.slices * q.per_slice < missing || (uint64_t)q.tiles * q.tile < q.per_slice) return (int)hipErrorInvalidValue;
    Buf d_pw, d_idx, d_partial, d_z, d_inv;
    hipError_t err = d_pw.make(pw, r * sizeof(Fr));
    if (err == hipSuccess) err = d_idx.make(missing_idx, (missing ? missing : 1) * 4);
    if (err == hipSuccess) err = d_partial.make(nullptr, (size_t)q.slices * 2 * r * sizeof(Fr));
    if (err == hipSuccess) err = d_z.make(nullptr, 2 * r * sizeof(Fr));
    if (err == hipSuccess) err = d_inv.make(nullptr, r * sizeof(Fr));
    if (err != hipSuccess) return (int)err;
    launch_recover_vanish(d_pw.fr(), static_cast<const uint32_t*>(d_idx.p()), fr_of(gl), q, d_partial.fr(), d_z.fr(), 0);
    err = hipMemcpyAsync(d_inv.p(), d_z.fr() + r, r * sizeof(Fr), hipMemcpyDeviceToDevice, 0);
    if (err != hipSuccess) return (int)err;
    launch_recover_invert(d_inv.fr(), r, 0);
    err = finish_launches();
    if (err != hipSuccess) return (int)err;
    bool ok = d_z.fetch(z, err);
    ok = d_inv.fetch(zc_inv, err) && ok;
    ok = d_partial.fetch(nullptr, err) && ok;
    ok = d_pw.fetch(nullptr, err) && ok;
    *slices_used = q.slices;
    *tile = q.tile;
    *guard = ok ? 1u : 0u;
    return (int)err;
}

// cells: count * K * l elements; pos: r entries, each below K or RECOVER_NO_CELL; zd: r.  Out: v, count * n elements.
extern "C" int drc_scatter(const uint32_t* cells, const uint32_t* pos, const uint32_t* zd, uint64_t K, uint32_t log_n, uint32_t log_l, uint64_t count,
                           uint32_t* v, uint32_t* guard) {
    if (!cells || !pos || !zd || !v || !guard) return (int)hipErrorInvalidValue;
    if (log_n < 1 || log_n > 16 || log_l >= log_n || count < 1 || count > 8) return (int)hipErrorInvalidValue;
    const uint64_t n = 1ull << log_n, l = 1ull << log_l, r = n >> log_l;
    if (K < 1 || K > r) return (int)hipErrorInvalidValue;
    for (uint64_t k = 0; k < r; ++k)
        if (pos[k] != RECOVER_NO_CELL && pos[k] >= K) return (int)hipErrorInvalidValue;
    const RecoverChunksPlan pl = recover_chunks_plan(log_n, log_l, 1, K, count, true, false);
    if (pl.log_tk + pl.log_tt > 8 || pl.log_tk > log_n - log_l || pl.log_tt > log_l || (pl.scatter_tiles << (pl.log_tk + pl.log_tt)) != n)
        return (int)hipErrorInvalidValue;
    Buf d_cells, d_pos, d_zd, d_v;
    hipError_t err = d_cells.make(cells, count * K * l * sizeof(Fr));
    if (err == hipSuccess) err = d_pos.make(pos, r * 4);
    if (err == hipSuccess) err = d_zd.make(zd, r * sizeof(Fr));
    if (err == hipSuccess) err = d_v.make(nullptr, count * n * sizeof(Fr));
    if (err != hipSuccess) return (int)err;
    launch_recover_scatter(d_cells.fr(), static_cast<const uint32_t*>(d_pos.p()), d_zd.fr(), K, log_n, log_l, count, pl, d_v.fr(), 0);
    err = finish_launches();
    if (err != hipSuccess) return (int)err;
    bool ok = d_v.fetch(v, err);
    ok = d_cells.fetch(nullptr, err) && ok;
    *guard = ok ? 1u : 0u;
    return (int)err;
}

// v: total elements, scaled in place by zc_inv[i & (r - 1)]; r = 2^log_r, total a multiple of r
extern "C" int drc_scale(uint32_t* v, const uint32_t* zc_inv, uint32_t log_r, uint64_t total, uint32_t* guard) {
    if (!v || !zc_inv || !guard || log_r > 16 || total < 1 || total > (1u << 20) || total % (1ull << log_r)) return (int)hipErrorInvalidValue;
    const uint64_t r = 1ull << log_r;
    Buf d_v, d_z;
    hipError_t err = d_v.make(v, total * sizeof(Fr));
    if (err == hipSuccess) err = d_z.make(zc_inv, r * sizeof(Fr));
    if (err != hipSuccess) return (int)err;
    launch_recover_scale(d_v.fr(), d_z.fr(), r, total, 0);
    err = finish_launches();
    if (err != hipSuccess) return (int)err;
    bool ok = d_v.fetch(v, err);
    ok = d_z.fetch(nullptr, err) && ok;
    *guard = ok ? 1u : 0u;
    return (int)err;
}

// v: count vectors of n = 2^log_n elements, l = 2^log_l, K cells, bound m; fixed: count bytes.  Out: verdict, 2 * count 64-bit
// words (first_excess, then the status); out: count * m elements; dst: count * (m + 2) elements, polynomial p's destination being
// [p (m + 2) + 1, + m) of one buffer that starts out as the fill -- the elements between them must come back as the fill.
extern "C" int drc_finish(const uint32_t* v, uint32_t log_n, uint32_t log_l, uint64_t K, uint64_t m, uint64_t count, const uint8_t* fixed,
                          uint64_t* verdict, uint32_t* out, uint32_t* dst, uint32_t* blocks, uint32_t* guard) {
    if (!v || !fixed || !verdict || !out || !dst || !blocks || !guard) return (int)hipErrorInvalidValue;
    if (log_n < 1 || log_n > 20 || log_l >= log_n || count < 1 || count > 8) return (int)hipErrorInvalidValue;
    const uint64_t n = 1ull << log_n, l = 1ull << log_l, r = n >> log_l;
    if (K < 1 || K > r || m < 1 || m > K * l) return (int)hipErrorInvalidValue;
    const RecoverChunksPlan pl = recover_chunks_plan(log_n, log_l, m, K, count, true, false);
    if (m + pl.excess_len > n || (uint64_t)pl.excess_blocks * pl.excess_span < pl.excess_len || (uint64_t)pl.excess_iters * 256 < pl.excess_span)
        return (int)hipErrorInvalidValue;
    Buf d_v, d_fixed, d_mins, d_res, d_out, d_dst, d_ptr;
    hipError_t err = d_v.make(v, count * n * sizeof(Fr));
    if (err == hipSuccess) err = d_fixed.make(fixed, count);
    if (err == hipSuccess) err = d_mins.make(nullptr, count * pl.excess_blocks * 8);
    if (err == hipSuccess) err = d_res.make(nullptr, 2 * count * 8);
    if (err == hipSuccess) err = d_out.make(nullptr, count * m * sizeof(Fr));
    if (err == hipSuccess) err = d_dst.make(nullptr, count * (m + 2) * sizeof(Fr));
    std::vector<Fr*> ptr(count);
    for (uint64_t p = 0; p < count; ++p) ptr[p] = d_dst.fr() + p * (m + 2) + 1;
    if (err == hipSuccess) err = d_ptr.make(ptr.data(), count * sizeof(Fr*));
    if (err != hipSuccess) return (int)err;
    launch_recover_finish(d_v.fr(), n, m, count, pl, static_cast<const uint8_t*>(d_fixed.p()), static_cast<Fr* const*>(d_ptr.p()), d_out.fr(),
                          static_cast<unsigned long long*>(d_mins.p()), static_cast<unsigned long long*>(d_res.p()), 0);
    err = finish_launches();
    if (err != hipSuccess) return (int)err;
    bool ok = d_res.fetch(verdict, err);
    ok = d_out.fetch(out, err) && ok;
    ok = d_dst.fetch(dst, err) && ok;
    ok = d_mins.fetch(nullptr, err) && ok;
    ok = d_v.fetch(nullptr, err) && ok;
    *blocks = pl.excess_blocks;
    *guard = ok ? 1u : 0u;
    return (int)err;
}
