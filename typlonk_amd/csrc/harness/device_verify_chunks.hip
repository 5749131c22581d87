// Test-only device harness over the kernels of typlonk_verify_chunks (tests/test_gpu_verify_chunks_kernels.py).
//
// verify_chunks.hip is compiled here as a unit, exactly as the library compiles it (same flags, no extra defines).  dvc_fold sorts
// the cells by commitment as the library's host code does, runs the per-call coset constants, the weights kernel and then the
// fold and its sum for one range [lo, hi) with the strip size the caller names -- through the
// library a shape only ever reaches the plan's own -- and hands back everything the kernels wrote; dvc_membership runs the
// membership flags over records in the SRS's internal form (PT_WORDS words a record).  Every output buffer is allocated at exactly
// the size a launcher may write, followed by a guard band.  Nothing is launched on a shape a kernel could leave its buffers with:
// the checks run on the host before the first HIP call.
// Not linked into libtyplonk_hip.so.  It lives beside the unit it wraps, as device_chunks.hip does.
#include "../verify_chunks.hip"

#include <vector>

using namespace ty;

namespace {

constexpr size_t GUARD_BYTES = 4096;
constexpr int GUARD_FILL = 0xA5;   // every allocation starts out as this byte, body and band

struct Buf {
    void* p = nullptr;
    size_t bytes = 0;
    Fr* fr() const { return static_cast<Fr*>(p); }
    // n bytes copied from src (or left as the fill), then the band
    hipError_t make(const void* src, size_t n) {
        bytes = n;
        hipError_t e = hipMalloc(&p, n + GUARD_BYTES);
        if (e == hipSuccess) e = hipMemset(p, GUARD_FILL, n + GUARD_BYTES);
        if (e == hipSuccess && src && n) e = hipMemcpy(p, src, n, hipMemcpyHostToDevice);
        return e;
    }
    // the body to the host (dst may be NULL), and whether the band is still the fill
    bool fetch(void* dst, hipError_t& e) const {
        std::vector<unsigned char> band(GUARD_BYTES);
        if (e == hipSuccess && dst) e = hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(band.data(), static_cast<char*>(p) + bytes, GUARD_BYTES, hipMemcpyDeviceToHost);
        bool ok = e == hipSuccess;
        for (size_t i = 0; ok && i < GUARD_BYTES; ++i) ok = band[i] == GUARD_FILL;
        return ok;
    }
    ~Buf() {
        if (p) (void)hipFree(p);
    }
};

Fr fr_of(const uint32_t* w) {
    Fr f;
    for (int i = 0; i < 8; ++i) f.v[i] = w[i];
    return f;
}

}  // namespace

// Fr values are 8 words each, Montgomery.  pw: N; cell_commit, cell_coset, live: N; evals: N * l; consts: root_r, w_inv, l_inv
// (3 x 8 words); tw: max(l / 2, 1).  Out: s_pi, s_all: N + M; scale, twist: N; coef: l; *blocks = the partial vectors the fold
// wrote.  strip = 0: the plan's own.  *guard = 1: every band is still the fill.  Returns the HIP error code,
// hipErrorInvalidValue -- before anything touches the device -- for a shape outside the launchers' contract.
extern "C" int dvc_fold(const uint32_t* pw, const uint32_t* cell_commit, const uint32_t* cell_coset, const uint8_t* live,
                        const uint32_t* evals, uint64_t N, uint64_t M, uint64_t lo, uint64_t hi, uint32_t log_l, const uint32_t* consts,
                        const uint32_t* tw, uint64_t strip, uint32_t* s_pi, uint32_t* s_all, uint32_t* scale, uint32_t* twist,
                        uint32_t* coef, uint64_t* blocks, uint32_t* guard) {
    if (!pw || !cell_commit || !cell_coset || !live || !evals || !consts || !tw || !s_pi || !s_all || !scale || !twist || !coef ||
        !blocks || !guard)
        return (int)hipErrorInvalidValue;
    if (log_l > VERIFY_CHUNKS_MAX_LOG_L || N == 0 || M == 0 || N > (1u << 20) || M > (1u << 16) || lo >= hi || hi > N ||
        strip > (1u << 20))
        return (int)hipErrorInvalidValue;
    const uint64_t l = 1ull << log_l;
    if (N * l > (1u << 22)) return (int)hipErrorInvalidValue;
    for (uint64_t i = 0; i < N; ++i)
        if (cell_commit[i] >= M) return (int)hipErrorInvalidValue;
    const VerifyChunksPlan pl = verify_chunks_plan(hi - lo, log_l, strip);
    if (pl.lds_bytes > (48u << 10) || pl.blocks > (1u << 20)) return (int)hipErrorInvalidValue;
    // the cells by commitment, ascending within one (verify_chunks_host.hip's counting sort)
    std::vector<uint32_t> first(M + 1, 0), order(N);
    for (uint64_t i = 0; i < N; ++i) ++first[cell_commit[i] + 1];
    for (uint64_t c = 0; c < M; ++c) first[c + 1] += first[c];
    {
        std::vector<uint32_t> next(first.begin(), first.end() - 1);
        for (uint64_t i = 0; i < N; ++i) order[next[cell_commit[i]]++] = (uint32_t)i;
    }
    Buf d_pw, d_order, d_first, d_coset_a, d_coset, d_live, d_evals, d_tw, d_pi, d_all, d_scale, d_twist, d_partial, d_coef;
    hipError_t err = d_pw.make(pw, N * sizeof(Fr));
    if (err == hipSuccess) err = d_order.make(order.data(), N * 4);
    if (err == hipSuccess) err = d_first.make(first.data(), (M + 1) * 4);
    if (err == hipSuccess) err = d_coset_a.make(nullptr, N * sizeof(Fr));
    if (err == hipSuccess) err = d_coset.make(cell_coset, N * 4);
    if (err == hipSuccess) err = d_live.make(live, N);
    if (err == hipSuccess) err = d_evals.make(evals, N * l * sizeof(Fr));
    if (err == hipSuccess) err = d_tw.make(tw, pl.tw * sizeof(Fr));
    if (err == hipSuccess) err = d_pi.make(nullptr, (N + M) * sizeof(Fr));
    if (err == hipSuccess) err = d_all.make(nullptr, (N + M) * sizeof(Fr));
    if (err == hipSuccess) err = d_scale.make(nullptr, N * sizeof(Fr));
    if (err == hipSuccess) err = d_twist.make(nullptr, N * sizeof(Fr));
    if (err == hipSuccess) err = d_partial.make(nullptr, pl.blocks * l * sizeof(Fr));
    if (err == hipSuccess) err = d_coef.make(nullptr, l * sizeof(Fr));
    if (err != hipSuccess) return (int)err;
    launch_chunks_cosets(static_cast<const uint32_t*>(d_coset.p), N, fr_of(consts), fr_of(consts + 8), d_coset_a.fr(), d_twist.fr(), 0);
    launch_chunks_weights(d_pw.fr(), d_coset_a.fr(), static_cast<const uint32_t*>(d_order.p), static_cast<const uint32_t*>(d_first.p),
                          static_cast<const uint8_t*>(d_live.p), N, M, lo, hi, fr_of(consts + 16), d_pi.fr(), d_all.fr(), d_scale.fr(), 0);
    launch_chunks_fold(d_evals.fr(), d_scale.fr(), d_twist.fr(), d_tw.fr(), lo, hi - lo, log_l, pl, d_partial.fr(), 0);
    launch_chunks_fold_sum(d_partial.fr(), pl.blocks, (uint32_t)l, d_coef.fr(), 0);
    err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err != hipSuccess) return (int)err;
    bool ok = d_pi.fetch(s_pi, err);
    ok = d_all.fetch(s_all, err) && ok;
    ok = d_scale.fetch(scale, err) && ok;
    ok = d_twist.fetch(twist, err) && ok;
    ok = d_coef.fetch(coef, err) && ok;
    ok = d_partial.fetch(nullptr, err) && ok;
    ok = d_coset_a.fetch(nullptr, err) && ok;
    *blocks = pl.blocks;
    *guard = ok ? 1u : 0u;
    return (int)err;
}

// pts: n records of PT_WORDS words in the internal form; flags: n bytes; clear != 0: pts comes back with the failing records
// replaced by the identity (else untouched).  *guard as above.
extern "C" int dvc_membership(uint32_t* pts, uint64_t n, uint32_t clear, uint8_t* flags, uint32_t* guard) {
    if (!pts || !flags || !guard || n == 0 || n > (1u << 16)) return (int)hipErrorInvalidValue;
    Buf d_pts, d_flags;
    hipError_t err = d_pts.make(pts, n * PT_WORDS * 4);
    if (err == hipSuccess) err = d_flags.make(nullptr, n);
    if (err != hipSuccess) return (int)err;
    launch_chunks_membership(static_cast<uint32_t*>(d_pts.p), n, static_cast<uint8_t*>(d_flags.p), clear != 0, 0);
    err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err != hipSuccess) return (int)err;
    bool ok = d_pts.fetch(pts, err);
    ok = d_flags.fetch(flags, err) && ok;
    *guard = ok ? 1u : 0u;
    return (int)err;
}
