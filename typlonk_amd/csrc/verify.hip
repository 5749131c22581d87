// libtyplonk_hip.so -- the verifiers: typlonk_circuit_commitments, typlonk_verify; and of the compact shape (include/typlonk.h)
//   typlonk_circuit_vk, typlonk_verify_compact, typlonk_compact_challenges (the transcript in compact_transcript.hpp)
//   plonk::proof::verify (plonk/src/proof.rs:195-281, 441-503) for a batch of proofs of one circuit.
//
// Per proof on the host (microseconds): the transcript's challenges (csrc/transcript.hpp), zeta, r(zeta) = 0, the 13 points
// on the curve, PI(zeta) of a short column and the linearisation scalars of the mirror's verify (host/typlonk_host.hpp).
// On the device: sigma_1 / sigma_2 at every zeta in one typlonk_poly_eval_dev over the circuit's cached coefficients,
// PI(zeta) of a long column (inverse NTT + evaluation), and the two MSMs of the fold.  The six KZG checks of every proof,
//   e(W_j, [s]G2 - z_j G2) = e(C_j - y_j G, G2)   <=>   e(W_j, [s]G2) = e(C_j - y_j G + z_j W_j, G2),
// have a fixed G2 side once rewritten, so the 6K checks weighted with rho_j = rho^(6k + j + 1) become ONE product
//   e(sum rho_j W_j, [s]G2) * e(-sum rho_j (C_j + z_j W_j) + (sum rho_j y_j) G, G2) = 1
// with the linearisation commitment C_5 expanded into its 11 bases (the 8 fixed ones shared by the batch).  A failed fold
// is bisected with the same weights down to the bad proofs.
#include "host.hpp"
#include "transcript.hpp"
#include "compact_transcript.hpp"
#include "../host/pairing_host.hpp"

#include <chrono>

using namespace ty;
using namespace tyh;

namespace {

namespace P = typlonk::pairing;

// public-input columns up to this length are interpolated at zeta on the host (barycentric), longer ones on the device
constexpr size_t PI_HOST_MAX = 2048;

Fr fr_load(const uint64_t l[4]) {
    Fr r;
    memcpy(r.v, l, 32);
    return r;
}
void fr_store(const Fr& a, uint64_t l[4]) { memcpy(l, a.v, 32); }
inline Fr add(const Fr& a, const Fr& b) { return fe_add(a, b); }
inline Fr sub(const Fr& a, const Fr& b) { return fe_sub(a, b); }
inline Fr mul(const Fr& a, const Fr& b) { return fe_mul(a, b); }
inline Fr neg(const Fr& a) { return fe_neg(a); }

bool fr_canonical(const uint64_t* l) {
    static const uint64_t R[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
    for (int i = 3; i >= 0; --i)
        if (l[i] != R[i]) return l[i] < R[i];
    return false;
}
bool fq_canonical(const uint64_t* l) {
    for (int i = 5; i >= 0; --i)
        if (l[i] != h64::P[i]) return l[i] < h64::P[i];
    return false;
}
// y^2 = x^3 + 4 with canonical coordinates (the identity is on the curve)
bool g1_on_curve(const uint64_t xy[12], uint8_t inf) {
    if (inf) return true;
    if (!fq_canonical(xy) || !fq_canonical(xy + 6)) return false;
    h64::Fq x, y;
    memcpy(x.v, xy, 48);
    memcpy(y.v, xy + 6, 48);
    const P::Fq four32 = P::fq_from_u64(4);
    h64::Fq four;
    memcpy(four.v, four32.v, 48);
    return h64::eq(h64::mul(y, y), h64::add(h64::mul(h64::mul(x, x), x), four));
}

// arkworks' Montgomery limbs of the fixed G1 generator (kzg/src/lib.rs:77; tests/test_oracle.py pins them)
const uint64_t G1_GEN[12] = {0x5cb38790fd530c16ull, 0x7817fc679976fff5ull, 0x154f95c7143ba1c1ull, 0xf0ae6acdf3d0e747ull,
                             0xedce6ecc21dbf440ull, 0x120177419e0bfb75ull, 0xbaac93d50ce72271ull, 0x8c22631a7918fd8eull,
                             0xdd595f13570725ceull, 0x51ac582950405194ull, 0x0e1c8c3fad0059c0ull, 0x0bbc3efc5008a26aull};

}  // namespace

namespace tyh {
int circuit_commitments(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const CircuitEntry::Commitments** out) {
    auto ci = ctx->circuits.find(circuit_id);
    if (ci == ctx->circuits.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown circuit id");
    auto si = ctx->srs.find(srs_id);
    if (si == ctx->srs.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown srs id");
    // (a shard on a context WITH a communicator never comes here: typlonk_circuit_commitments / typlonk_circuit_vk /
    // typlonk_prove_compact fold circuit_statement_partial instead.  typlonk_verify and the batched provers stay on one GPU:
    // sharding is for the latency of one large proof; many small ones belong on one GPU per proof)
    if (si->second.total_len)
        return fail(ctx, TYPLONK_ERR_INVALID_ARG,
                    "this call needs a whole SRS, not a shard (a shard's circuit commitments are a collective: they need a "
                    "communicator on the context, typlonk_comm_init; verification and batched proving run on one GPU)");
    CircuitEntry& ce = ci->second;
    const uint64_t n = 1ull << ce.log_n;
    if (si->second.len < n) return fail(ctx, TYPLONK_ERR_LENGTH, "SRS shorter than the circuit's n");
    auto hit = ce.commitments.find(srs_id);
    if (hit == ce.commitments.end()) {
        CircuitEntry::Commitments c;
        const void* ptrs[8];
        size_t ms[8];
        for (int k = 0; k < 8; ++k) {
            ptrs[k] = ce.coef + (uint64_t)k * n;
            ms[k] = n;
        }
        ProfilingOff prof_off(ctx);
        const int rc = msm_batch(ctx, srs_id, ptrs, ms, 8, &c.xy[0][0], c.inf);
        if (rc) return rc;
        hit = ce.commitments.emplace(srs_id, c).first;
    }
    *out = &hit->second;
    return TYPLONK_OK;
}

// A rank's share of the statement on an SRS SHARD: records 0..7 = its partial sums of the eight circuit commitments (the
// MSMs sum only the shard's index range; run once per (circuit, SRS) on this rank, then cached -- what is cached is the
// PARTIAL sum, the fold is the caller's), record 8 = SRS point 0 on the rank whose range starts at index 0 and the identity
// elsewhere.  The fold of the nine records over the ranks is the whole-SRS statement.  No collective here: every failure is
// local and the caller carries it into its fold.
int circuit_statement_partial(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, uint64_t xy[9][12], uint8_t inf[9]) {
    auto ci = ctx->circuits.find(circuit_id);
    if (ci == ctx->circuits.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown circuit id");
    auto si = ctx->srs.find(srs_id);
    if (si == ctx->srs.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown srs id");
    CircuitEntry& ce = ci->second;
    const uint64_t n = 1ull << ce.log_n;
    if (si->second.total() < n) return fail(ctx, TYPLONK_ERR_LENGTH, "SRS shorter than the circuit's n");
    auto hit = ce.commitments.find(srs_id);
    if (hit == ce.commitments.end()) {
        CircuitEntry::Commitments c;
        const void* ptrs[8];
        size_t ms[8];
        for (int k = 0; k < 8; ++k) {
            ptrs[k] = ce.coef + (uint64_t)k * n;
            ms[k] = n;
        }
        ProfilingOff prof_off(ctx);
        const int rc = msm_batch(ctx, srs_id, ptrs, ms, 8, &c.xy[0][0], c.inf);
        if (rc) return rc;
        hit = ce.commitments.emplace(srs_id, c).first;
    }
    memcpy(xy, hit->second.xy, 8 * 96);
    memcpy(inf, hit->second.inf, 8);
    if (si->second.shard_first == 0 && si->second.len > 0) return typlonk_srs_download(ctx, srs_id, 0, 1, xy[8], &inf[8]);
    memset(xy[8], 0, 96);
    inf[8] = 1;
    return TYPLONK_OK;
}
}  // namespace tyh

namespace {

// PI(zeta) = interpolate(pi).evaluate(zeta) for a column of len <= n values (zero beyond), on the host:
//   L_i(zeta) = (zeta^n - 1) / n * w^i / (zeta - w^i), one batched inversion; zeta inside the domain picks the value.
Fr pi_barycentric(const uint64_t* pi, size_t len, const Fr& zeta, const Fr& zn, uint32_t log_n) {
    const Fr w = fr_domain_root(log_n);
    if (zn == Fr::one()) {
        Fr wi = Fr::one();
        for (size_t i = 0; i < len; ++i, wi = mul(wi, w))
            if (wi == zeta) return fr_load(pi + 4 * i);
        return Fr::zero();
    }
    std::vector<Fr> d(len), pre(len + 1);
    std::vector<Fr> wpow(len);
    Fr wi = Fr::one();
    pre[0] = Fr::one();
    for (size_t i = 0; i < len; ++i, wi = mul(wi, w)) {
        wpow[i] = wi;
        d[i] = sub(zeta, wi);
        pre[i + 1] = mul(pre[i], d[i]);
    }
    Fr inv = fe_inv(pre[len]);
    Fr acc = Fr::zero();
    for (size_t i = len; i-- > 0;) {
        const Fr di_inv = mul(inv, pre[i]);
        inv = mul(inv, d[i]);
        acc = add(acc, mul(mul(fr_load(pi + 4 * i), wpow[i]), di_inv));
    }
    return mul(acc, mul(sub(zn, Fr::one()), fr_inv_pow2(log_n)));
}

struct ProofState {
    bool live = false;
    Fr beta, gamma, alpha, zeta, zn, pi_eval;
    Fr sig[2];
    Fr v;   // the compact shape's fifth challenge
};

// PI(zeta) of every live proof: short columns on the host, long ones on the device (inverse NTT + evaluation at the proof's
// zeta).  *any_long (may be NULL) = some column took the device path.
int pi_at_zeta(typlonk_ctx* ctx, std::vector<ProofState>& st, const uint64_t* const* pi, const size_t* pi_len, uint32_t log_n,
               bool* any_long) {
    const uint64_t n = 1ull << log_n;
    int rc = TYPLONK_OK;
    Fr* d_pi = nullptr;
    if (any_long) *any_long = false;
    for (size_t k = 0; k < st.size() && !rc; ++k) {
        ProofState& ps = st[k];
        ps.pi_eval = Fr::zero();
        const size_t len = pi_len ? pi_len[k] : 0;
        if (!ps.live || !len) continue;
        if (len <= PI_HOST_MAX) {
            ps.pi_eval = pi_barycentric(pi[k], len, ps.zeta, ps.zn, log_n);
            continue;
        }
        if (any_long) *any_long = true;
        if (!d_pi) {
            hipError_t he = hipMalloc((void**)&d_pi, n * sizeof(Fr));
            if (he != hipSuccess) {
                d_pi = nullptr;
                rc = fail(ctx, he == hipErrorOutOfMemory ? TYPLONK_ERR_OOM : TYPLONK_ERR_HIP, hipGetErrorString(he));
                break;
            }
        }
        hipError_t he = hipMemcpyAsync(d_pi, pi[k], len * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream);
        if (he == hipSuccess && len < n) he = hipMemsetAsync(d_pi + len, 0, (n - len) * sizeof(Fr), ctx->stream);
        if (he != hipSuccess) {
            rc = fail(ctx, TYPLONK_ERR_HIP, hipGetErrorString(he));
            break;
        }
        rc = ntt_run(ctx, d_pi, log_n, 1, nullptr, /*sync=*/false);
        uint64_t z[4], y[4];
        fr_store(ps.zeta, z);
        const Fr* pp = d_pi;
        if (!rc) rc = poly_eval_run(ctx, &pp, 1, n, z, 1, y);
        if (!rc) ps.pi_eval = fr_load(y);
    }
    if (d_pi) (void)hipFree(d_pi);
    return rc;
}

// [s]G2 from its 24 limbs: canonical coordinates on the twist
bool g2s_load(const uint64_t g2s_xy[24], P::G2Affine* g2s) {
    for (int i = 0; i < 24; i += 6)
        if (!fq_canonical(g2s_xy + i)) return false;
    memcpy(g2s->x.a.v, g2s_xy, 48);
    memcpy(g2s->x.b.v, g2s_xy + 6, 48);
    memcpy(g2s->y.a.v, g2s_xy + 12, 48);
    memcpy(g2s->y.b.v, g2s_xy + 18, 48);
    g2s->infinity = false;
    return P::g2_is_on_curve(*g2s);
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The fold and its bisection, shared by typlonk_verify and typlonk_verify_compact.  A proof shape supplies the scalars of one
// folded check over the live proofs of [lo, hi): s1 over the first m1 bases of the temporary point set (the opening
// witnesses, paired with [s]G2) and s2 over all m2 of them (paired with G2).
struct FoldBisect {
    typlonk_ctx* ctx = nullptr;
    uint32_t bases_id = 0;
    size_t m1 = 0, m2 = 0;
    std::vector<uint8_t> live;   // per proof: passed the host checks
    P::G2Affine g2s;
    double t_msm = 0, t_pair = 0;
    int folds = 0;
    virtual ~FoldBisect() = default;
    virtual void scalars(size_t lo, size_t hi, std::vector<uint64_t>& s1, std::vector<uint64_t>& s2) const = 0;

    // one folded check over the live proofs in [lo, hi): *pass = the pairing product is one
    int fold(size_t lo, size_t hi, bool* pass) {
        std::vector<uint64_t> s1(m1 * 4, 0), s2(m2 * 4, 0);
        scalars(lo, hi, s1, s2);
        auto t0 = std::chrono::steady_clock::now();
        uint64_t xy[2][12];
        uint8_t inf[2];
        int rc = typlonk_msm_g1(ctx, bases_id, s1.data(), m1, xy[0], &inf[0]);
        if (!rc) rc = typlonk_msm_g1(ctx, bases_id, s2.data(), m2, xy[1], &inf[1]);
        t_msm += ms_since(t0);
        if (rc) return rc;
        t0 = std::chrono::steady_clock::now();
        P::G1Aff ps[2];
        for (int i = 0; i < 2; ++i) {
            memcpy(ps[i].x.v, xy[i], 48);
            memcpy(ps[i].y.v, xy[i] + 6, 48);
            ps[i].infinity = inf[i] != 0;
        }
        const P::G2Affine qs[2] = {g2s, P::g2_generator()};
        *pass = P::pairing_product_is_one(ps, qs, 2);
        t_pair += ms_since(t0);
        ++folds;
        return TYPLONK_OK;
    }
    // verdicts of the live proofs in [lo, hi): accept all when their fold holds, else split
    int decide(size_t lo, size_t hi, uint8_t* ok) {
        size_t n_live = 0;
        for (size_t k = lo; k < hi; ++k) n_live += live[k];
        if (!n_live) return TYPLONK_OK;
        bool pass = false;
        int rc = fold(lo, hi, &pass);
        if (rc) return rc;
        if (pass) {
            for (size_t k = lo; k < hi; ++k) ok[k] = live[k] ? 1 : 0;
            return TYPLONK_OK;
        }
        if (n_live == 1) return TYPLONK_OK;   // ok stays 0
        // split the LIVE proofs of the range in half
        size_t seen = 0, mid = lo;
        for (; mid < hi; ++mid) {
            if (live[mid] && seen == n_live / 2) break;
            seen += live[mid];
        }
        rc = decide(lo, mid, ok);
        if (!rc) rc = decide(mid, hi, ok);
        return rc;
    }
    // the temporary point set the MSMs run over (the caller frees it with typlonk_srs_free)
    int load_bases(const std::vector<uint64_t>& xy, const std::vector<uint8_t>& inf) {
        return typlonk_srs_load(ctx, xy.data(), inf.data(), inf.size(), &bases_id);
    }
    void report(double t_host, const double* t_eval) {
        prof_begin(ctx);
        ctx->prof_result.clear();
        ctx->prof_result.push_back({"verify_host", (float)t_host});
        if (t_eval) ctx->prof_result.push_back({"verify_eval", (float)*t_eval});
        ctx->prof_result.push_back({"verify_msm", (float)t_msm});
        ctx->prof_result.push_back({"verify_pairing", (float)t_pair});
        ctx->prof_result.push_back({"verify_folds", (float)folds});
    }
};

// the reference shape: six checks per proof
struct Verifier : FoldBisect {
    // temporary point set: W_{k,j} (6K), then a, b, c, Z, t0..t2 of every proof (7K), the 8 fixed
    size_t K = 0;
    const typlonk_proof* proofs = nullptr;
    std::vector<ProofState>* st = nullptr;
    std::vector<Fr> rho_pow;  // rho^(e + 1), e < 6K
    const CircuitEntry::Commitments* cc = nullptr;
    Fr omega, cosets[3];
    uint64_t n = 0;
    uint32_t flags = 0;

    void scalars(size_t lo, size_t hi, std::vector<uint64_t>& s1, std::vector<uint64_t>& s2) const override {
        Fr fixed[8], gsum = Fr::zero();
        for (Fr& f : fixed) f = Fr::zero();
        for (size_t k = lo; k < hi; ++k) {
            const ProofState& ps = (*st)[k];
            if (!ps.live) continue;
            const typlonk_proof& pr = proofs[k];
            const typlonk_proof_tail& t = pr.tail;
            Fr rho[6], ev[6];
            for (int j = 0; j < 6; ++j) {
                rho[j] = rho_pow[6 * k + j];
                ev[j] = fr_load(t.evals[j]);
                fr_store(rho[j], &s1[4 * (6 * k + j)]);
                const Fr z = j == 4 ? mul(ps.zeta, omega) : ps.zeta;
                fr_store(neg(mul(rho[j], z)), &s2[4 * (6 * k + j)]);   // z_j W_j
                gsum = add(gsum, mul(rho[j], ev[j]));                  // y_j G
            }
            // the linearisation commitment (plonk/src/proof.rs:441-503, as the mirror's verify builds it)
            const Fr a = ev[0], b = ev[1], c = ev[2], zw = ev[4];
            const Fr alpha = ps.alpha, beta = ps.beta, gamma = ps.gamma, zeta = ps.zeta;
            Fr l2 = Fr::one();
            const Fr adv[3] = {a, b, c};
            for (int i = 0; i < 3; ++i) l2 = mul(l2, add(add(adv[i], mul(mul(beta, cosets[i]), zeta)), gamma));
            const Fr vanish = sub(ps.zn, Fr::one());
            Fr l0 = Fr::one();
            if (zeta != Fr::one()) l0 = mul(vanish, fe_inv(mul(fr_from_u64(n), sub(zeta, Fr::one()))));
            Fr l3 = Fr::one();
            for (int i = 0; i < 2; ++i) l3 = mul(l3, add(add(adv[i], mul(beta, ps.sig[i])), gamma));
            const Fr alpha2 = mul(alpha, alpha);
            const Fr constant = add(add(mul(alpha, mul(mul(l3, add(c, gamma)), zw)), mul(l0, alpha2)),
                                    (flags & TYPLONK_VERIFY_PI_AS_PROVER) ? neg(ps.pi_eval) : ps.pi_eval);
            const Fr r5 = rho[5];
            // variable bases: a, b, c, Z, t0, t1, t2 (coefficients of -sum rho_j C_j)
            const Fr zs[7] = {neg(rho[0]), neg(rho[1]), neg(rho[2]),
                              neg(add(add(rho[3], rho[4]), mul(r5, add(mul(l2, alpha), mul(l0, alpha2))))),
                              mul(r5, vanish), mul(r5, mul(vanish, ps.zn)), mul(r5, mul(vanish, mul(ps.zn, ps.zn)))};
            for (int i = 0; i < 7; ++i) fr_store(zs[i], &s2[4 * (6 * K + 7 * k + i)]);
            // fixed bases: q_l q_r q_o q_m q_c, sigma_3, SRS point 0
            const Fr fx[7] = {neg(mul(r5, a)), neg(mul(r5, b)), mul(r5, c), neg(mul(r5, mul(a, b))), neg(r5),
                              mul(r5, mul(mul(mul(l3, alpha), beta), zw)), mul(r5, constant)};
            for (int i = 0; i < 7; ++i) fixed[i] = add(fixed[i], fx[i]);
        }
        fixed[7] = gsum;
        for (int i = 0; i < 8; ++i) fr_store(fixed[i], &s2[4 * (13 * K + i)]);
    }
};

void put_u64(std::vector<uint8_t>& b, uint64_t v) {
    for (int i = 0; i < 8; ++i) b.push_back((uint8_t)(v >> (8 * i)));
}
void put_limbs(std::vector<uint8_t>& b, const uint64_t* l, int count) {
    for (int i = 0; i < count; ++i) put_u64(b, l[i]);
}
void put_point(std::vector<uint8_t>& b, const uint64_t xy[12], uint8_t inf) {
    put_limbs(b, xy, 12);
    b.push_back(inf);
}

}  // namespace

int typlonk_circuit_commitments(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, uint64_t xy[8][12], uint8_t inf[8]) {
    if (!ctx || !xy || !inf) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    if (comm_folds(ctx, srs_id)) {
        // a collective: ALWAYS one fold of 8 records, the rank's partial sums -- or flagged ones when anything failed here
        uint64_t rec_xy[9][12];
        uint8_t rec_inf[9];
        int rc = TYPLONK_OK;
        const hipError_t he = hipSetDevice(ctx->device);
        if (he != hipSuccess) rc = fail(ctx, TYPLONK_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(he));
        if (!rc) rc = circuit_statement_partial(ctx, srs_id, circuit_id, rec_xy, rec_inf);
        rc = comm_fold(ctx, &rec_xy[0][0], rec_inf, 8, rc);
        if (rc) return rc;
        memcpy(xy, rec_xy, 8 * 96);
        memcpy(inf, rec_inf, 8);
        return TYPLONK_OK;
    }
    HIPCHK(hipSetDevice(ctx->device));
    const CircuitEntry::Commitments* c = nullptr;
    const int rc = circuit_commitments(ctx, srs_id, circuit_id, &c);
    if (rc) return rc;
    memcpy(xy, c->xy, sizeof(c->xy));
    memcpy(inf, c->inf, sizeof(c->inf));
    return TYPLONK_OK;
}

int typlonk_verify(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const uint64_t g2s_xy[24],
                   const uint64_t cosets[3][4], const typlonk_proof* proofs, size_t count,
                   const uint64_t* const* pi, const size_t* pi_len, uint32_t flags, uint8_t* ok) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    if (count == 0) return TYPLONK_OK;
    if (!g2s_xy || !cosets || !proofs || !ok) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    if (flags & ~TYPLONK_VERIFY_PI_AS_PROVER) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown flag");
    HIPCHK(hipSetDevice(ctx->device));
    const auto t_start = std::chrono::steady_clock::now();
    memset(ok, 0, count);
    auto ci = ctx->circuits.find(circuit_id);
    if (ci == ctx->circuits.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown circuit id");
    const uint32_t log_n = ci->second.log_n;
    const uint64_t n = 1ull << log_n;
    for (size_t k = 0; k < count; ++k) {
        const size_t len = pi_len ? pi_len[k] : 0;
        if (len > n) return fail(ctx, TYPLONK_ERR_LENGTH, "public-input column longer than n");
        if (len && (!pi || !pi[k])) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null public-input column");
    }
    P::G2Affine g2s;
    if (!g2s_load(g2s_xy, &g2s)) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "g2s is not a point of the twist in canonical coordinates");
    ProfilingOff prof_off(ctx);
    const bool profiling = prof_off.saved;
    const CircuitEntry::Commitments* cc = nullptr;
    int rc = circuit_commitments(ctx, srs_id, circuit_id, &cc);
    if (rc) return rc;
    const CircuitEntry& ce = ci->second;
    uint64_t srs0_xy[12];
    uint8_t srs0_inf = 0;
    rc = typlonk_srs_download(ctx, srs_id, 0, 1, srs0_xy, &srs0_inf);
    if (rc) return rc;

    // ---- per-proof host checks ----
    std::vector<ProofState> st(count);
    for (size_t k = 0; k < count; ++k) {
        const typlonk_proof& pr = proofs[k];
        ProofState& ps = st[k];
        bool good = true;
        for (int i = 0; i < 3; ++i) good = good && g1_on_curve(pr.commit_xy[i], pr.commit_inf[i]) && g1_on_curve(pr.tail.t_xy[i], pr.tail.t_inf[i]);
        good = good && g1_on_curve(pr.z_xy, pr.z_inf);
        for (int i = 0; i < 6; ++i) good = good && g1_on_curve(pr.tail.w_xy[i], pr.tail.w_inf[i]) && fr_canonical(pr.tail.evals[i]);
        good = good && fr_canonical(pr.zeta);
        if (!good) continue;
        ChallengeGenerator g;   // verify_challenges, proof.rs:236-246
        for (int i = 0; i < 3; ++i) g.digest(pr.commit_xy[i], pr.commit_inf[i]);
        uint64_t ch[8];
        g.generate(2, ch);
        ps.beta = fr_load(ch);
        ps.gamma = fr_load(ch + 4);
        g.digest(pr.z_xy, pr.z_inf);
        g.generate(2, ch);
        ps.alpha = fr_load(ch);
        ps.zeta = fr_load(ch + 4);
        if (ps.zeta != fr_load(pr.zeta)) continue;                    // :212-214
        if (!fr_load(pr.tail.evals[5]).is_zero()) continue;          // :234-235
        uint32_t e[2] = {(uint32_t)n, (uint32_t)(n >> 32)};
        ps.zn = fe_pow(ps.zeta, e, 2);
        ps.live = true;
    }
    // PI(zeta): short columns on the host, long ones on the device (inverse NTT + evaluation at the proof's zeta)
    const double t_host_a = ms_since(t_start);
    auto t0 = std::chrono::steady_clock::now();
    rc = pi_at_zeta(ctx, st, pi, pi_len, log_n, nullptr);
    if (rc) return rc;
    // sigma_1(zeta_k), sigma_2(zeta_k) of every live proof: one evaluation over the cached coefficients
    {
        std::vector<size_t> idx;
        std::vector<uint64_t> pts;
        for (size_t k = 0; k < count; ++k)
            if (st[k].live) {
                idx.push_back(k);
                uint64_t z[4];
                fr_store(st[k].zeta, z);
                pts.insert(pts.end(), z, z + 4);
            }
        if (!idx.empty()) {
            const Fr* polys[2] = {ce.coef + 5 * n, ce.coef + 6 * n};
            std::vector<uint64_t> out(2 * idx.size() * 4);
            rc = poly_eval_run(ctx, polys, 2, n, pts.data(), idx.size(), out.data());
            if (rc) return rc;
            for (size_t i = 0; i < idx.size(); ++i)
                for (int p = 0; p < 2; ++p) st[idx[i]].sig[p] = fr_load(&out[4 * (p * idx.size() + i)]);
        }
    }
    const double t_eval = ms_since(t0);
    t0 = std::chrono::steady_clock::now();

    // ---- rho: Blake2b-512 of the batch ----
    std::vector<uint8_t> bytes;
    bytes.reserve(1024 + count * (13 * 97 + 8 * 32));
    put_u64(bytes, n);
    put_u64(bytes, flags);
    put_limbs(bytes, g2s_xy, 24);
    put_point(bytes, srs0_xy, srs0_inf);
    for (int i = 0; i < 8; ++i) put_point(bytes, cc->xy[i], cc->inf[i]);
    for (size_t k = 0; k < count; ++k) {
        const typlonk_proof& pr = proofs[k];
        for (int i = 0; i < 3; ++i) put_point(bytes, pr.commit_xy[i], pr.commit_inf[i]);
        put_point(bytes, pr.z_xy, pr.z_inf);
        for (int i = 0; i < 3; ++i) put_point(bytes, pr.tail.t_xy[i], pr.tail.t_inf[i]);
        for (int i = 0; i < 6; ++i) put_point(bytes, pr.tail.w_xy[i], pr.tail.w_inf[i]);
        put_limbs(bytes, &pr.tail.evals[0][0], 24);
        put_limbs(bytes, pr.zeta, 4);
        uint64_t pv[4];
        fr_store(st[k].pi_eval, pv);   // zero for a proof the host checks rejected
        put_limbs(bytes, pv, 4);
    }
    uint8_t h[64];
    blake2b_512(bytes.data(), bytes.size(), h);
    const Fr rho = fr_from_digest(h);

    Verifier v;
    v.ctx = ctx;
    v.m1 = 6 * count;
    v.m2 = 13 * count + 8;
    for (size_t k = 0; k < count; ++k) v.live.push_back(st[k].live ? 1 : 0);
    v.K = count;
    v.proofs = proofs;
    v.st = &st;
    v.cc = cc;
    v.n = n;
    v.flags = flags;
    v.g2s = g2s;
    v.omega = fr_domain_root(log_n);
    for (int i = 0; i < 3; ++i) v.cosets[i] = fr_load(cosets[i]);
    v.rho_pow.resize(6 * count);
    Fr r = rho;
    for (size_t e = 0; e < 6 * count; ++e, r = mul(r, rho)) v.rho_pow[e] = r;
    // the bases of the fold: proofs the host checks rejected contribute identities
    const size_t nb = 13 * count + 8;
    std::vector<uint64_t> bxy(nb * 12, 0);
    std::vector<uint8_t> binf(nb, 1);
    auto set = [&](size_t i, const uint64_t* xy, uint8_t inf) {
        memcpy(&bxy[12 * i], xy, 96);
        binf[i] = inf;
    };
    for (size_t k = 0; k < count; ++k) {
        if (!st[k].live) continue;
        const typlonk_proof& pr = proofs[k];
        for (int j = 0; j < 6; ++j) set(6 * k + j, pr.tail.w_xy[j], pr.tail.w_inf[j]);
        const size_t b = 6 * count + 7 * k;
        for (int i = 0; i < 3; ++i) set(b + i, pr.commit_xy[i], pr.commit_inf[i]);
        set(b + 3, pr.z_xy, pr.z_inf);
        for (int i = 0; i < 3; ++i) set(b + 4 + i, pr.tail.t_xy[i], pr.tail.t_inf[i]);
    }
    for (int i = 0; i < 5; ++i) set(13 * count + i, cc->xy[i], cc->inf[i]);
    set(13 * count + 5, cc->xy[7], cc->inf[7]);   // sigma_3
    set(13 * count + 6, srs0_xy, srs0_inf);
    set(13 * count + 7, G1_GEN, 0);
    for (size_t i = 0; i < nb; ++i)   // identities in the C-ABI form (0, 1)
        if (binf[i]) {
            memset(&bxy[12 * i], 0, 96);
        }
    const double t_host_b = ms_since(t0);
    rc = v.load_bases(bxy, binf);
    if (rc) return rc;
    rc = v.decide(0, count, ok);
    (void)typlonk_srs_free(ctx, v.bases_id);
    if (rc) {
        memset(ok, 0, count);
        return rc;
    }
    if (profiling) v.report(t_host_a + t_host_b, &t_eval);
    return TYPLONK_OK;
}

// ================================================================================================
// The compact shape (include/typlonk.h, typlonk_prove_compact): two KZG checks per proof against a verifying key.

namespace tyh {
int circuit_vk_fill(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const uint64_t cosets[3][4], typlonk_vk* vk) {
    const CircuitEntry::Commitments* cc = nullptr;
    int rc = circuit_commitments(ctx, srs_id, circuit_id, &cc);
    if (rc) return rc;
    memset(vk, 0, sizeof(*vk));
    vk->log_n = ctx->circuits.at(circuit_id).log_n;
    memcpy(vk->cosets, cosets, sizeof(vk->cosets));
    memcpy(vk->commit_xy, cc->xy, sizeof(vk->commit_xy));
    memcpy(vk->commit_inf, cc->inf, sizeof(vk->commit_inf));
    return typlonk_srs_download(ctx, srs_id, 0, 1, vk->srs0_xy, &vk->srs0_inf);
}
}  // namespace tyh

namespace {

// temporary point set: W_z, W_zw of every proof (2K), then a, b, c, Z, t0..t2 of every proof (7K), then the shared
// q_l q_r q_o q_m q_c sigma_1 sigma_2 sigma_3, P0, G (10)
struct CompactVerifier : FoldBisect {
    size_t K = 0;
    const typlonk_proof_compact* proofs = nullptr;
    const std::vector<ProofState>* st = nullptr;
    std::vector<Fr> rho_pow;  // rho^(e + 1), e < 2K
    Fr omega, cosets[3];
    uint64_t n = 0;

    void scalars(size_t lo, size_t hi, std::vector<uint64_t>& s1, std::vector<uint64_t>& s2) const override {
        Fr fixed[10];
        for (Fr& f : fixed) f = Fr::zero();
        for (size_t k = lo; k < hi; ++k) {
            const ProofState& ps = (*st)[k];
            if (!ps.live) continue;
            const typlonk_proof_compact& pr = proofs[k];
            Fr ev[7];
            for (int i = 0; i < 7; ++i) ev[i] = fr_load(pr.evals[i]);
            const Fr a = ev[0], b = ev[1], c = ev[2], z = ev[3], zw = ev[4], s1e = ev[5], s2e = ev[6];
            const Fr r0 = rho_pow[2 * k], r1 = rho_pow[2 * k + 1];
            const Fr alpha = ps.alpha, beta = ps.beta, gamma = ps.gamma, zeta = ps.zeta;
            Fr vp[7];
            vp[0] = Fr::one();
            for (int i = 1; i < 7; ++i) vp[i] = mul(vp[i - 1], ps.v);
            // witnesses: rho_j on the left, -rho_j z_j on the right
            fr_store(r0, &s1[4 * (2 * k)]);
            fr_store(r1, &s1[4 * (2 * k + 1)]);
            fr_store(neg(mul(r0, zeta)), &s2[4 * (2 * k)]);
            fr_store(neg(mul(r1, mul(zeta, omega))), &s2[4 * (2 * k + 1)]);
            // y_F (r(zeta) = 0 contributes nothing) and Z(zeta w), on G
            const Fr yf = add(add(add(a, mul(vp[1], b)), add(mul(vp[2], c), mul(vp[3], z))), add(mul(vp[5], s1e), mul(vp[6], s2e)));
            fixed[9] = add(fixed[9], add(mul(r0, yf), mul(r1, zw)));
            // [r] expanded as typlonk_verify does with TYPLONK_VERIFY_PI_AS_PROVER, weighted with rho_0 v^4
            Fr l2 = Fr::one();
            for (int i = 0; i < 3; ++i) l2 = mul(l2, add(add(ev[i], mul(mul(beta, cosets[i]), zeta)), gamma));
            const Fr vanish = sub(ps.zn, Fr::one());
            Fr l0 = Fr::one();
            if (zeta != Fr::one()) l0 = mul(vanish, fe_inv(mul(fr_from_u64(n), sub(zeta, Fr::one()))));
            const Fr l3 = mul(add(add(a, mul(beta, s1e)), gamma), add(add(b, mul(beta, s2e)), gamma));
            const Fr alpha2 = mul(alpha, alpha);
            const Fr constant = sub(add(mul(alpha, mul(mul(l3, add(c, gamma)), zw)), mul(l0, alpha2)), ps.pi_eval);
            const Fr r4 = mul(r0, vp[4]);
            // per-proof bases a, b, c, Z, t0, t1, t2: coefficients of -(rho_0 F_C + rho_1 [Z])
            const Fr zs[7] = {neg(r0), neg(mul(r0, vp[1])), neg(mul(r0, vp[2])),
                              neg(add(add(mul(r0, vp[3]), r1), mul(r4, add(mul(l2, alpha), mul(l0, alpha2))))),
                              mul(r4, vanish), mul(r4, mul(vanish, ps.zn)), mul(r4, mul(vanish, mul(ps.zn, ps.zn)))};
            for (int i = 0; i < 7; ++i) fr_store(zs[i], &s2[4 * (2 * K + 7 * k + i)]);
            const Fr fx[9] = {neg(mul(r4, a)), neg(mul(r4, b)), mul(r4, c), neg(mul(r4, mul(a, b))), neg(r4),
                              neg(mul(r0, vp[5])), neg(mul(r0, vp[6])), mul(r4, mul(mul(mul(l3, alpha), beta), zw)),
                              mul(r4, constant)};
            for (int i = 0; i < 9; ++i) fixed[i] = add(fixed[i], fx[i]);
        }
        for (int i = 0; i < 10; ++i) fr_store(fixed[i], &s2[4 * (9 * K + i)]);
    }
};

bool vk_points_valid(const typlonk_vk& vk) {
    for (int i = 0; i < 8; ++i)
        if (!g1_on_curve(vk.commit_xy[i], vk.commit_inf[i])) return false;
    return g1_on_curve(vk.srs0_xy, vk.srs0_inf);
}

}  // namespace

namespace tyh {
int verify_compact_check_args(typlonk_ctx* ctx, const typlonk_vk* vk, size_t count, const uint64_t* const* pi, const size_t* pi_len) {
    const uint32_t log_n = vk->log_n;
    if (log_n < 1 || log_n > TYPLONK_MAX_PROVER_LOG_N) return fail(ctx, TYPLONK_ERR_DOMAIN, "vk log_n outside 1..24");
    const uint64_t n = 1ull << log_n;
    for (size_t k = 0; k < count; ++k) {
        const size_t len = pi_len ? pi_len[k] : 0;
        if (len > n) return fail(ctx, TYPLONK_ERR_LENGTH, "public-input column longer than n");
        if (len && (!pi || !pi[k])) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null public-input column");
    }
    P::G2Affine g2s;
    if (!g2s_load(vk->g2s_xy, &g2s)) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "vk g2s is not a point of the twist in canonical coordinates");
    if (!vk_points_valid(*vk)) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "a vk point is not on the curve");
    for (int i = 0; i < 3; ++i)
        if (!fr_canonical(vk->cosets[i])) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "vk coset is not a canonical residue");
    return TYPLONK_OK;
}
}  // namespace tyh

int typlonk_circuit_vk(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const uint64_t cosets[3][4],
                       const uint64_t g2s_xy[24], typlonk_vk* vk) {
    if (!ctx || !cosets || !g2s_xy || !vk) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    if (comm_folds(ctx, srs_id)) {
        // a collective: ALWAYS one fold of 9 records (the eight partial sums and the P0 record), flagged when anything failed here
        uint64_t rec_xy[9][12];
        uint8_t rec_inf[9];
        int rc = TYPLONK_OK;
        const hipError_t he = hipSetDevice(ctx->device);
        if (he != hipSuccess) rc = fail(ctx, TYPLONK_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(he));
        P::G2Affine g2s;
        if (!rc && !g2s_load(g2s_xy, &g2s)) rc = fail(ctx, TYPLONK_ERR_INVALID_ARG, "g2s is not a point of the twist in canonical coordinates");
        if (!rc) rc = circuit_statement_partial(ctx, srs_id, circuit_id, rec_xy, rec_inf);
        rc = comm_fold(ctx, &rec_xy[0][0], rec_inf, 9, rc);
        if (rc) return rc;
        typlonk_vk out;
        memset(&out, 0, sizeof(out));
        out.log_n = ctx->circuits.at(circuit_id).log_n;
        memcpy(out.cosets, cosets, sizeof(out.cosets));
        memcpy(out.commit_xy, rec_xy, sizeof(out.commit_xy));
        memcpy(out.commit_inf, rec_inf, sizeof(out.commit_inf));
        memcpy(out.srs0_xy, rec_xy[8], sizeof(out.srs0_xy));
        out.srs0_inf = rec_inf[8];
        memcpy(out.g2s_xy, g2s_xy, sizeof(out.g2s_xy));
        *vk = out;
        return TYPLONK_OK;
    }
    HIPCHK(hipSetDevice(ctx->device));
    P::G2Affine g2s;
    if (!g2s_load(g2s_xy, &g2s)) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "g2s is not a point of the twist in canonical coordinates");
    typlonk_vk out;
    const int rc = circuit_vk_fill(ctx, srs_id, circuit_id, cosets, &out);
    if (rc) return rc;
    memcpy(out.g2s_xy, g2s_xy, sizeof(out.g2s_xy));
    *vk = out;
    return TYPLONK_OK;
}

int typlonk_compact_challenges(const typlonk_vk* vk, const typlonk_proof_compact* proof, const uint64_t* pi, size_t pi_len,
                               uint64_t out[5][4]) {
    if (!vk || !proof || !out || (pi_len && !pi)) return TYPLONK_ERR_INVALID_ARG;
    if (vk->log_n > 32) return TYPLONK_ERR_DOMAIN;
    if (pi_len > (1ull << vk->log_n)) return TYPLONK_ERR_LENGTH;
    uint8_t d0[64];
    compact_statement_digest(*vk, pi, pi_len, d0);
    Fr ch[5];
    compact_challenges(d0, *proof, ch);
    for (int i = 0; i < 5; ++i) fr_store(ch[i], out[i]);
    return TYPLONK_OK;
}

int typlonk_verify_compact(typlonk_ctx* ctx, const typlonk_vk* vk, const typlonk_proof_compact* proofs, size_t count,
                           const uint64_t* const* pi, const size_t* pi_len, uint8_t* ok) {
    if (!ctx) return TYPLONK_ERR_INVALID_ARG;
    if (count == 0) return TYPLONK_OK;
    if (!vk || !proofs || !ok) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    HIPCHK(hipSetDevice(ctx->device));
    const auto t_start = std::chrono::steady_clock::now();
    memset(ok, 0, count);
    const int args_rc = verify_compact_check_args(ctx, vk, count, pi, pi_len);
    if (args_rc) return args_rc;
    const uint32_t log_n = vk->log_n;
    const uint64_t n = 1ull << log_n;
    P::G2Affine g2s;
    (void)g2s_load(vk->g2s_xy, &g2s);   // (judged by verify_compact_check_args)
    ProfilingOff prof_off(ctx);
    const bool profiling = prof_off.saved;

    // ---- per-proof host checks: points, scalars, the transcript, zeta^n != 1 ----
    std::vector<ProofState> st(count);
    uint8_t d0_no_pi[64];   // the statement without public values, shared by every proof that has none
    compact_statement_digest(*vk, nullptr, 0, d0_no_pi);
    for (size_t k = 0; k < count; ++k) {
        const typlonk_proof_compact& pr = proofs[k];
        ProofState& ps = st[k];
        bool good = g1_on_curve(pr.z_xy, pr.z_inf);
        for (int i = 0; i < 3; ++i) good = good && g1_on_curve(pr.commit_xy[i], pr.commit_inf[i]) && g1_on_curve(pr.t_xy[i], pr.t_inf[i]);
        for (int i = 0; i < 2; ++i) good = good && g1_on_curve(pr.w_xy[i], pr.w_inf[i]);
        for (int i = 0; i < 7; ++i) good = good && fr_canonical(pr.evals[i]);
        if (!good) continue;
        const size_t len = pi_len ? pi_len[k] : 0;
        uint8_t d0[64];
        if (len) compact_statement_digest(*vk, pi[k], len, d0);
        else memcpy(d0, d0_no_pi, 64);
        Fr ch[5];
        compact_challenges(d0, pr, ch);
        ps.beta = ch[0];
        ps.gamma = ch[1];
        ps.alpha = ch[2];
        ps.zeta = ch[3];
        ps.v = ch[4];
        uint32_t e[2] = {(uint32_t)n, (uint32_t)(n >> 32)};
        ps.zn = fe_pow(ps.zeta, e, 2);
        if (ps.zn == Fr::one()) continue;   // zeta in the domain: Z_H(zeta) = 0 and the quotient is unconstrained
        ps.sig[0] = fr_load(pr.evals[5]);
        ps.sig[1] = fr_load(pr.evals[6]);
        ps.live = true;
    }
    const double t_host_a = ms_since(t_start);
    auto t0 = std::chrono::steady_clock::now();
    bool any_long = false;
    int rc = pi_at_zeta(ctx, st, pi, pi_len, log_n, &any_long);
    if (rc) return rc;
    const double t_eval = ms_since(t0);
    t0 = std::chrono::steady_clock::now();

    // ---- rho: H("typlonk/compact/fold/v1" || vk_bytes || [s]G2 || every proof's points and evaluations || every PI(zeta)) ----
    static const char tag[] = "typlonk/compact/fold/v1";
    std::vector<uint8_t> bytes(tag, tag + sizeof(tag) - 1);
    bytes.reserve(1024 + count * (9 * 96 + 8 * 32));
    compact_vk_bytes(*vk, bytes);
    for (int i = 0; i < 24; ++i) compact_put_u64(bytes, vk->g2s_xy[i]);
    for (size_t k = 0; k < count; ++k) {
        const typlonk_proof_compact& pr = proofs[k];
        for (int i = 0; i < 3; ++i) compact_put_point(bytes, pr.commit_xy[i], pr.commit_inf[i]);
        compact_put_point(bytes, pr.z_xy, pr.z_inf);
        for (int i = 0; i < 3; ++i) compact_put_point(bytes, pr.t_xy[i], pr.t_inf[i]);
        for (int i = 0; i < 2; ++i) compact_put_point(bytes, pr.w_xy[i], pr.w_inf[i]);
        for (int i = 0; i < 7; ++i) compact_put_fr(bytes, pr.evals[i]);
    }
    for (size_t k = 0; k < count; ++k) {
        uint64_t pv[4];
        fr_store(st[k].pi_eval, pv);   // zero for a proof the host checks rejected
        compact_put_fr(bytes, pv);
    }
    uint8_t h[64];
    blake2b_512(bytes.data(), bytes.size(), h);
    const Fr rho = fr_from_digest(h);

    CompactVerifier v;
    v.ctx = ctx;
    v.m1 = 2 * count;
    v.m2 = 9 * count + 10;
    for (size_t k = 0; k < count; ++k) v.live.push_back(st[k].live ? 1 : 0);
    v.g2s = g2s;
    v.K = count;
    v.proofs = proofs;
    v.st = &st;
    v.n = n;
    v.omega = fr_domain_root(log_n);
    for (int i = 0; i < 3; ++i) v.cosets[i] = fr_load(vk->cosets[i]);
    v.rho_pow.resize(2 * count);
    Fr r = rho;
    for (size_t e = 0; e < 2 * count; ++e, r = mul(r, rho)) v.rho_pow[e] = r;
    // the bases of the fold: proofs the host checks rejected contribute identities
    const size_t nb = v.m2;
    std::vector<uint64_t> bxy(nb * 12, 0);
    std::vector<uint8_t> binf(nb, 1);
    auto set = [&](size_t i, const uint64_t* xy, uint8_t inf) {
        memcpy(&bxy[12 * i], xy, 96);
        binf[i] = inf;
    };
    for (size_t k = 0; k < count; ++k) {
        if (!st[k].live) continue;
        const typlonk_proof_compact& pr = proofs[k];
        for (int j = 0; j < 2; ++j) set(2 * k + j, pr.w_xy[j], pr.w_inf[j]);
        const size_t b = 2 * count + 7 * k;
        for (int i = 0; i < 3; ++i) set(b + i, pr.commit_xy[i], pr.commit_inf[i]);
        set(b + 3, pr.z_xy, pr.z_inf);
        for (int i = 0; i < 3; ++i) set(b + 4 + i, pr.t_xy[i], pr.t_inf[i]);
    }
    for (int i = 0; i < 8; ++i) set(9 * count + i, vk->commit_xy[i], vk->commit_inf[i]);
    set(9 * count + 8, vk->srs0_xy, vk->srs0_inf);
    set(9 * count + 9, G1_GEN, 0);
    for (size_t i = 0; i < nb; ++i)   // identities in the C-ABI form (0, 1)
        if (binf[i]) memset(&bxy[12 * i], 0, 96);
    const double t_host_b = ms_since(t0);
    rc = v.load_bases(bxy, binf);
    if (rc) return rc;
    rc = v.decide(0, count, ok);
    (void)typlonk_srs_free(ctx, v.bases_id);
    if (rc) {
        memset(ok, 0, count);
        return rc;
    }
    if (profiling) v.report(t_host_a + t_host_b, any_long ? &t_eval : nullptr);
    return TYPLONK_OK;
}
