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
//
// Both proof shapes share every step but their admission rules, their bytes under rho and their weights: which points and
// scalars are admitted (host_checks.hpp), the scalars of the linearisation commitment (lin_commit.hpp), the walk over a
// proof's fields (ProofView) and everything from rho to the verdicts (FoldBisect).
#include "host.hpp"
#include "host_checks.hpp"
#include "lin_commit.hpp"
#include "transcript.hpp"
#include "compact_transcript.hpp"

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

// arkworks' Montgomery limbs of the fixed G1 generator (kzg/src/lib.rs:77; tests/test_oracle.py pins them)
const uint64_t G1_GEN[12] = {0x5cb38790fd530c16ull, 0x7817fc679976fff5ull, 0x154f95c7143ba1c1ull, 0xf0ae6acdf3d0e747ull,
                             0xedce6ecc21dbf440ull, 0x120177419e0bfb75ull, 0xbaac93d50ce72271ull, 0x8c22631a7918fd8eull,
                             0xdd595f13570725ceull, 0x51ac582950405194ull, 0x0e1c8c3fad0059c0ull, 0x0bbc3efc5008a26aull};

// The eight circuit commitments over the points this SRS entry holds: found in the circuit's cache, or else one batch of
// eight MSMs (no stage events of their own) that is stored there.  On a shard the MSMs sum only the shard's index range: what
// is cached is the rank's PARTIAL sum, the fold is the caller's.
int cached_commitments(typlonk_ctx* ctx, uint32_t srs_id, CircuitEntry& ce, const CircuitEntry::Commitments** out) {
    auto hit = ce.commitments.find(srs_id);
    if (hit == ce.commitments.end()) {
        const uint64_t n = 1ull << ce.log_n;
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
    return cached_commitments(ctx, srs_id, ce, out);
}

// A rank's share of the statement on an SRS SHARD: records 0..7 = its partial sums of the eight circuit commitments
// (cached_commitments), record 8 = SRS point 0 on the rank whose range starts at index 0 and the identity elsewhere.  The fold
// of the nine records over the ranks is the whole-SRS statement.  No collective here: every failure is local and the caller
// carries it into its fold.
int circuit_statement_partial(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, uint64_t xy[9][12], uint8_t inf[9]) {
    auto ci = ctx->circuits.find(circuit_id);
    if (ci == ctx->circuits.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown circuit id");
    auto si = ctx->srs.find(srs_id);
    if (si == ctx->srs.end()) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "unknown srs id");
    CircuitEntry& ce = ci->second;
    const uint64_t n = 1ull << ce.log_n;
    if (si->second.total() < n) return fail(ctx, TYPLONK_ERR_LENGTH, "SRS shorter than the circuit's n");
    const CircuitEntry::Commitments* c = nullptr;
    const int rc = cached_commitments(ctx, srs_id, ce, &c);
    if (rc) return rc;
    memcpy(xy, c->xy, 8 * 96);
    memcpy(inf, c->inf, 8);
    if (si->second.shard_first == 0 && si->second.len > 0) return typlonk_srs_download(ctx, srs_id, 0, 1, xy[8], &inf[8]);
    memset(xy[8], 0, 96);
    inf[8] = 1;
    return TYPLONK_OK;
}

void vk_assemble(uint32_t log_n, const uint64_t cosets[3][4], const uint64_t (*rec_xy)[12], const uint8_t* rec_inf, typlonk_vk* vk) {
    memset(vk, 0, sizeof(*vk));
    vk->log_n = log_n;
    memcpy(vk->cosets, cosets, sizeof(vk->cosets));
    memcpy(vk->commit_xy, rec_xy, sizeof(vk->commit_xy));
    memcpy(vk->commit_inf, rec_inf, sizeof(vk->commit_inf));
    memcpy(vk->srs0_xy, rec_xy[8], sizeof(vk->srs0_xy));
    vk->srs0_inf = rec_inf[8];
}

int circuit_vk_fill(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const uint64_t cosets[3][4], typlonk_vk* vk) {
    const CircuitEntry::Commitments* cc = nullptr;
    int rc = circuit_commitments(ctx, srs_id, circuit_id, &cc);
    if (rc) return rc;
    uint64_t rec_xy[9][12];
    uint8_t rec_inf[9];
    memcpy(rec_xy, cc->xy, sizeof(cc->xy));
    memcpy(rec_inf, cc->inf, sizeof(cc->inf));
    rc = typlonk_srs_download(ctx, srs_id, 0, 1, rec_xy[8], &rec_inf[8]);
    if (rc) return rc;
    vk_assemble(ctx->circuits.at(circuit_id).log_n, cosets, rec_xy, rec_inf, vk);
    return TYPLONK_OK;
}
}  // namespace tyh

namespace {

const char* const G2S_REFUSED = "g2s is not a point of the twist in canonical coordinates";

// The collective form of typlonk_circuit_commitments / typlonk_circuit_vk on an SRS shard: the rank's local work, then ALWAYS
// one fold of `records` records -- 8: the partial sums of the commitments, 9: with the P0 record -- flagged ones when anything
// failed here.  g2s_xy (may be NULL) is judged before the local work.
int statement_fold(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const uint64_t* g2s_xy, size_t records,
                   uint64_t rec_xy[9][12], uint8_t rec_inf[9]) {
    int rc = TYPLONK_OK;
    const hipError_t he = hipSetDevice(ctx->device);
    if (he != hipSuccess) rc = fail(ctx, TYPLONK_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(he));
    P::G2Affine g2s;
    if (!rc && g2s_xy && !g2_from_limbs(g2s_xy, &g2s)) rc = fail(ctx, TYPLONK_ERR_INVALID_ARG, G2S_REFUSED);
    if (!rc) rc = circuit_statement_partial(ctx, srs_id, circuit_id, rec_xy, rec_inf);
    return comm_fold(ctx, &rec_xy[0][0], rec_inf, records, rc);
}

// the public-input columns of a batch: none longer than n, none missing
int pi_args_check(typlonk_ctx* ctx, uint64_t n, size_t count, const uint64_t* const* pi, const size_t* pi_len) {
    for (size_t k = 0; k < count; ++k) {
        const size_t len = pi_len ? pi_len[k] : 0;
        if (len > n) return fail(ctx, TYPLONK_ERR_LENGTH, "public-input column longer than n");
        if (len && (!pi || !pi[k])) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null public-input column");
    }
    return TYPLONK_OK;
}

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

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

struct G1Ref {
    const uint64_t* xy;
    uint8_t inf;
};

// A proof of either shape as the verifier walks it, by reference into the caller's proof: the seven commitments, the shape's
// opening witnesses and evaluations, and the further scalars it hashes into rho (the reference shape's zeta).
struct ProofView {
    G1Ref commit[7];            // [a] [b] [c] [Z] [t_lo] [t_mid] [t_hi]
    G1Ref w[6];
    const uint64_t* evals[7];
    const uint64_t* extra[1];
    int n_w = 0, n_evals = 0, n_extra = 0;

    // every field in the order both shapes hash it for rho; the writers are the shape's
    template <class Point, class Scalar>
    void walk(Point point, Scalar scalar) const {
        for (const G1Ref& p : commit) point(p);
        for (int i = 0; i < n_w; ++i) point(w[i]);
        for (int i = 0; i < n_evals; ++i) scalar(evals[i]);
        for (int i = 0; i < n_extra; ++i) scalar(extra[i]);
    }
    // every point on the curve, every scalar a canonical residue
    bool admissible() const {
        bool good = true;
        walk([&](const G1Ref& p) { good = good && g1_on_curve(p.xy, p.inf); }, [&](const uint64_t* l) { good = good && fr_canonical(l); });
        return good;
    }
};
template <class Proof, class Tail>
void view_commitments(const Proof& pr, const Tail& t, ProofView* v) {
    for (int i = 0; i < 3; ++i) v->commit[i] = {pr.commit_xy[i], pr.commit_inf[i]};
    v->commit[3] = {pr.z_xy, pr.z_inf};
    for (int i = 0; i < 3; ++i) v->commit[4 + i] = {t.t_xy[i], t.t_inf[i]};
    for (int i = 0; i < v->n_w; ++i) v->w[i] = {t.w_xy[i], t.w_inf[i]};
    for (int i = 0; i < v->n_evals; ++i) v->evals[i] = t.evals[i];
}
ProofView view_of(const typlonk_proof& pr) {
    ProofView v;
    v.n_w = v.n_evals = 6;
    v.n_extra = 1;
    v.extra[0] = pr.zeta;
    view_commitments(pr, pr.tail, &v);
    return v;
}
ProofView view_of(const typlonk_proof_compact& pr) {
    ProofView v;
    v.n_w = 2;
    v.n_evals = 7;
    view_commitments(pr, pr, &v);
    return v;
}

// The fold and its bisection, shared by typlonk_verify and typlonk_verify_compact.  The temporary point set of a batch of K
// proofs with n_w opening witnesses each: the witnesses of every proof (n_w K, paired with [s]G2), then a, b, c, Z, t0..t2 of
// every proof (7K), then the shape's shared bases; all of them are paired with G2.  A proof shape supplies the scalars of one
// folded check over the live proofs of [lo, hi): s1 over the witnesses, s2 over the whole set.
struct FoldBisect {
    typlonk_ctx* ctx = nullptr;
    uint32_t bases_id = 0;
    size_t K = 0, n_w = 0, m2 = 0;
    std::vector<ProofView> views;
    std::vector<ProofState> st;   // live: passed the host checks
    std::vector<Fr> rho_pow;      // rho^(e + 1), e < n_w K
    Fr omega, cosets[3];
    uint64_t n = 0;
    P::G2Affine g2s;
    double t_msm = 0, t_pair = 0;
    int folds = 0;

    template <class Proof>
    FoldBisect(typlonk_ctx* c, const Proof* proofs, size_t count, uint32_t log_n, const uint64_t k[3][4], const P::G2Affine& q)
        : ctx(c), K(count), views(count), st(count), omega(fr_domain_root(log_n)), n(1ull << log_n), g2s(q) {
        for (size_t i = 0; i < count; ++i) views[i] = view_of(proofs[i]);
        n_w = (size_t)views[0].n_w;
        for (int i = 0; i < 3; ++i) cosets[i] = fr_load(k[i]);
    }
    virtual ~FoldBisect() = default;
    virtual void scalars(size_t lo, size_t hi, std::vector<uint64_t>& s1, std::vector<uint64_t>& s2) const = 0;

    Fr zeta_pow_n(const Fr& zeta) const {
        const uint32_t e[2] = {(uint32_t)n, (uint32_t)(n >> 32)};
        return fe_pow(zeta, e, 2);
    }
    // out = -weight * (the coefficients of proof k's linearisation commitment, lin_commit.hpp): its share of -sum rho_j C_j
    void lin_terms(size_t k, const Fr& a, const Fr& b, const Fr& c, const Fr& zw, const Fr& pi_signed, const Fr& weight,
                   Fr (&out)[LIN_BASES]) const {
        const ProofState& ps = st[k];
        const LinCommitIn in{a, b, c, zw, {ps.sig[0], ps.sig[1]}, ps.alpha, ps.beta, ps.gamma, ps.zeta, ps.zn, n,
                             {cosets[0], cosets[1], cosets[2]}, pi_signed};
        lin_commit_scalars(in, out);
        const Fr wn = neg(weight);
        for (Fr& f : out) f = mul(wn, f);
    }

    // one folded check over the live proofs in [lo, hi): *pass = the pairing product is one
    int fold(size_t lo, size_t hi, bool* pass) {
        const size_t m1 = n_w * K;
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
        for (size_t k = lo; k < hi; ++k) n_live += st[k].live;
        if (!n_live) return TYPLONK_OK;
        bool pass = false;
        int rc = fold(lo, hi, &pass);
        if (rc) return rc;
        if (pass) {
            for (size_t k = lo; k < hi; ++k) ok[k] = st[k].live ? 1 : 0;
            return TYPLONK_OK;
        }
        if (n_live == 1) return TYPLONK_OK;   // ok stays 0
        // split the LIVE proofs of the range in half
        size_t seen = 0, mid = lo;
        for (; mid < hi; ++mid) {
            if (st[mid].live && seen == n_live / 2) break;
            seen += st[mid].live;
        }
        rc = decide(lo, mid, ok);
        if (!rc) rc = decide(mid, hi, ok);
        return rc;
    }
    // What follows the shape's rho: its powers, the temporary point set (a proof the host checks rejected contributes
    // identities; `shared`: the shape's bases after the proofs'), the verdicts, and with `profiling` the stages -- t_host:
    // the host time before t0, t_eval (may be NULL): the device evaluations.
    int finish(const Fr& rho, const G1Ref* shared, size_t n_shared, uint8_t* ok, bool profiling, double t_host,
               std::chrono::steady_clock::time_point t0, const double* t_eval) {
        rho_pow.resize(n_w * K);
        Fr r = rho;
        for (Fr& p : rho_pow) {
            p = r;
            r = mul(r, rho);
        }
        m2 = (n_w + 7) * K + n_shared;
        std::vector<uint64_t> bxy(m2 * 12, 0);   // identities in the C-ABI form (0, 1)
        std::vector<uint8_t> binf(m2, 1);
        auto set = [&](size_t i, const G1Ref& p) {
            if (!p.inf) memcpy(&bxy[12 * i], p.xy, 96);
            binf[i] = p.inf;
        };
        for (size_t k = 0; k < K; ++k) {
            if (!st[k].live) continue;
            for (size_t j = 0; j < n_w; ++j) set(n_w * k + j, views[k].w[j]);
            for (size_t i = 0; i < 7; ++i) set(n_w * K + 7 * k + i, views[k].commit[i]);
        }
        for (size_t i = 0; i < n_shared; ++i) set((n_w + 7) * K + i, shared[i]);
        t_host += ms_since(t0);
        int rc = typlonk_srs_load(ctx, bxy.data(), binf.data(), m2, &bases_id);
        if (rc) return rc;
        rc = decide(0, K, ok);
        (void)typlonk_srs_free(ctx, bases_id);
        if (rc) {
            memset(ok, 0, K);
            return rc;
        }
        if (!profiling) return TYPLONK_OK;
        prof_begin(ctx);
        ctx->prof_result.clear();
        ctx->prof_result.push_back({"verify_host", (float)t_host});
        if (t_eval) ctx->prof_result.push_back({"verify_eval", (float)*t_eval});
        ctx->prof_result.push_back({"verify_msm", (float)t_msm});
        ctx->prof_result.push_back({"verify_pairing", (float)t_pair});
        ctx->prof_result.push_back({"verify_folds", (float)folds});
        return TYPLONK_OK;
    }
};

// the reference shape: six checks per proof, weighted with rho^(6k + j + 1); [r] is the sixth's commitment.  Shared bases:
// q_l q_r q_o q_m q_c, sigma_3, P0, G (8)
struct Verifier : FoldBisect {
    using FoldBisect::FoldBisect;
    uint32_t flags = 0;

    void scalars(size_t lo, size_t hi, std::vector<uint64_t>& s1, std::vector<uint64_t>& s2) const override {
        Fr fixed[8];
        for (Fr& f : fixed) f = Fr::zero();
        for (size_t k = lo; k < hi; ++k) {
            const ProofState& ps = st[k];
            if (!ps.live) continue;
            Fr rho[6], ev[6];
            for (int j = 0; j < 6; ++j) {
                rho[j] = rho_pow[6 * k + j];
                ev[j] = fr_load(views[k].evals[j]);
                fr_store(rho[j], &s1[4 * (6 * k + j)]);
                const Fr z = j == 4 ? mul(ps.zeta, omega) : ps.zeta;
                fr_store(neg(mul(rho[j], z)), &s2[4 * (6 * k + j)]);   // z_j W_j
                fixed[7] = add(fixed[7], mul(rho[j], ev[j]));          // y_j G
            }
            Fr lin[LIN_BASES];
            lin_terms(k, ev[0], ev[1], ev[2], ev[4], (flags & TYPLONK_VERIFY_PI_AS_PROVER) ? neg(ps.pi_eval) : ps.pi_eval, rho[5], lin);
            // a, b, c, Z, t0, t1, t2 (coefficients of -sum rho_j C_j)
            const Fr zs[7] = {neg(rho[0]), neg(rho[1]), neg(rho[2]), add(neg(add(rho[3], rho[4])), lin[LIN_Z]),
                              lin[LIN_T_LO], lin[LIN_T_MID], lin[LIN_T_HI]};
            for (int i = 0; i < 7; ++i) fr_store(zs[i], &s2[4 * (6 * K + 7 * k + i)]);
            for (int i = 0; i < 7; ++i) fixed[i] = add(fixed[i], lin[i]);   // LIN_QL .. LIN_QC, LIN_SIGMA3, LIN_P0
        }
        for (int i = 0; i < 8; ++i) fr_store(fixed[i], &s2[4 * (13 * K + i)]);
    }
};
static_assert(LIN_QL == 0 && LIN_QC == 4 && LIN_SIGMA3 == 5 && LIN_P0 == 6, "the shared bases follow lin_commit.hpp's order");

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
        uint64_t rec_xy[9][12];
        uint8_t rec_inf[9];
        const int rc = statement_fold(ctx, srs_id, circuit_id, nullptr, 8, rec_xy, rec_inf);
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
    const int pi_rc = pi_args_check(ctx, n, count, pi, pi_len);
    if (pi_rc) return pi_rc;
    P::G2Affine g2s;
    if (!g2_from_limbs(g2s_xy, &g2s)) return fail(ctx, TYPLONK_ERR_INVALID_ARG, G2S_REFUSED);
    ProfilingOff prof_off(ctx);
    const CircuitEntry::Commitments* cc = nullptr;
    int rc = circuit_commitments(ctx, srs_id, circuit_id, &cc);
    if (rc) return rc;
    const CircuitEntry& ce = ci->second;
    uint64_t srs0_xy[12];
    uint8_t srs0_inf = 0;
    rc = typlonk_srs_download(ctx, srs_id, 0, 1, srs0_xy, &srs0_inf);
    if (rc) return rc;

    // ---- per-proof host checks ----
    Verifier v(ctx, proofs, count, log_n, cosets, g2s);
    v.flags = flags;
    for (size_t k = 0; k < count; ++k) {
        const typlonk_proof& pr = proofs[k];
        ProofState& ps = v.st[k];
        if (!v.views[k].admissible()) continue;
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
        ps.zn = v.zeta_pow_n(ps.zeta);
        ps.live = true;
    }
    // PI(zeta): short columns on the host, long ones on the device (inverse NTT + evaluation at the proof's zeta)
    const double t_host = ms_since(t_start);
    auto t0 = std::chrono::steady_clock::now();
    rc = pi_at_zeta(ctx, v.st, pi, pi_len, log_n, nullptr);
    if (rc) return rc;
    // sigma_1(zeta_k), sigma_2(zeta_k) of every live proof: one evaluation over the cached coefficients
    {
        std::vector<size_t> idx;
        std::vector<uint64_t> pts;
        for (size_t k = 0; k < count; ++k)
            if (v.st[k].live) {
                idx.push_back(k);
                uint64_t z[4];
                fr_store(v.st[k].zeta, z);
                pts.insert(pts.end(), z, z + 4);
            }
        if (!idx.empty()) {
            const Fr* polys[2] = {ce.coef + 5 * n, ce.coef + 6 * n};
            std::vector<uint64_t> out(2 * idx.size() * 4);
            rc = poly_eval_run(ctx, polys, 2, n, pts.data(), idx.size(), out.data());
            if (rc) return rc;
            for (size_t i = 0; i < idx.size(); ++i)
                for (int p = 0; p < 2; ++p) v.st[idx[i]].sig[p] = fr_load(&out[4 * (p * idx.size() + i)]);
        }
    }
    const double t_eval = ms_since(t0);
    t0 = std::chrono::steady_clock::now();

    // ---- rho: Blake2b-512 of the batch (raw limbs and a flag byte per point; each proof's zeta and PI(zeta) follow it) ----
    std::vector<uint8_t> bytes;
    bytes.reserve(1024 + count * (13 * 97 + 8 * 32));
    put_u64(bytes, n);
    put_u64(bytes, flags);
    put_limbs(bytes, g2s_xy, 24);
    put_point(bytes, srs0_xy, srs0_inf);
    for (int i = 0; i < 8; ++i) put_point(bytes, cc->xy[i], cc->inf[i]);
    for (size_t k = 0; k < count; ++k) {
        v.views[k].walk([&](const G1Ref& p) { put_point(bytes, p.xy, p.inf); }, [&](const uint64_t* l) { put_limbs(bytes, l, 4); });
        uint64_t pv[4];
        fr_store(v.st[k].pi_eval, pv);   // zero for a proof the host checks rejected
        put_limbs(bytes, pv, 4);
    }
    uint8_t h[64];
    blake2b_512(bytes.data(), bytes.size(), h);

    G1Ref shared[8];
    for (int i = 0; i < 5; ++i) shared[i] = {cc->xy[i], cc->inf[i]};
    shared[5] = {cc->xy[7], cc->inf[7]};   // sigma_3
    shared[6] = {srs0_xy, srs0_inf};
    shared[7] = {G1_GEN, 0};
    return v.finish(fr_from_digest(h), shared, 8, ok, prof_off.saved, t_host, t0, &t_eval);
}

// ================================================================================================
// The compact shape (include/typlonk.h, typlonk_prove_compact): two KZG checks per proof against a verifying key.

namespace {

// two checks per proof, weighted with rho^(2k + 1) (F at zeta: a, b, c, Z, [r], sigma_1, sigma_2 by powers of v, so [r]
// weighs rho_0 v^4) and rho^(2k + 2) (Z at zeta w).  Shared bases: q_l q_r q_o q_m q_c sigma_1 sigma_2 sigma_3, P0, G (10)
struct CompactVerifier : FoldBisect {
    using FoldBisect::FoldBisect;

    void scalars(size_t lo, size_t hi, std::vector<uint64_t>& s1, std::vector<uint64_t>& s2) const override {
        Fr fixed[10];
        for (Fr& f : fixed) f = Fr::zero();
        for (size_t k = lo; k < hi; ++k) {
            const ProofState& ps = st[k];
            if (!ps.live) continue;
            Fr ev[7];
            for (int i = 0; i < 7; ++i) ev[i] = fr_load(views[k].evals[i]);
            const Fr a = ev[0], b = ev[1], c = ev[2], z = ev[3], zw = ev[4], s1e = ev[5], s2e = ev[6];
            const Fr r0 = rho_pow[2 * k], r1 = rho_pow[2 * k + 1];
            Fr vp[7];
            vp[0] = Fr::one();
            for (int i = 1; i < 7; ++i) vp[i] = mul(vp[i - 1], ps.v);
            // witnesses: rho_j on the left, -rho_j z_j on the right
            fr_store(r0, &s1[4 * (2 * k)]);
            fr_store(r1, &s1[4 * (2 * k + 1)]);
            fr_store(neg(mul(r0, ps.zeta)), &s2[4 * (2 * k)]);
            fr_store(neg(mul(r1, mul(ps.zeta, omega))), &s2[4 * (2 * k + 1)]);
            // y_F (r(zeta) = 0 contributes nothing) and Z(zeta w), on G
            const Fr yf = add(add(add(a, mul(vp[1], b)), add(mul(vp[2], c), mul(vp[3], z))), add(mul(vp[5], s1e), mul(vp[6], s2e)));
            fixed[9] = add(fixed[9], add(mul(r0, yf), mul(r1, zw)));
            Fr lin[LIN_BASES];
            lin_terms(k, a, b, c, zw, neg(ps.pi_eval), mul(r0, vp[4]), lin);   // (the compact prover subtracts PI(zeta))
            // per-proof bases a, b, c, Z, t0, t1, t2: coefficients of -(rho_0 F_C + rho_1 [Z])
            const Fr zs[7] = {neg(r0), neg(mul(r0, vp[1])), neg(mul(r0, vp[2])), add(neg(add(mul(r0, vp[3]), r1)), lin[LIN_Z]),
                              lin[LIN_T_LO], lin[LIN_T_MID], lin[LIN_T_HI]};
            for (int i = 0; i < 7; ++i) fr_store(zs[i], &s2[4 * (2 * K + 7 * k + i)]);
            const Fr fx[9] = {lin[LIN_QL], lin[LIN_QR], lin[LIN_QO], lin[LIN_QM], lin[LIN_QC],
                              neg(mul(r0, vp[5])), neg(mul(r0, vp[6])), lin[LIN_SIGMA3], lin[LIN_P0]};
            for (int i = 0; i < 9; ++i) fixed[i] = add(fixed[i], fx[i]);
        }
        for (int i = 0; i < 10; ++i) fr_store(fixed[i], &s2[4 * (9 * K + i)]);
    }
};

}  // namespace

namespace tyh {
int verify_compact_check_args(typlonk_ctx* ctx, const typlonk_vk* vk, size_t count, const uint64_t* const* pi, const size_t* pi_len,
                              P::G2Affine* g2s) {
    const uint32_t log_n = vk->log_n;
    if (log_n < 1 || log_n > TYPLONK_MAX_PROVER_LOG_N) return fail(ctx, TYPLONK_ERR_DOMAIN, "vk log_n outside 1..24");
    const uint64_t n = 1ull << log_n;
    const int pi_rc = pi_args_check(ctx, n, count, pi, pi_len);
    if (pi_rc) return pi_rc;
    if (!g2_from_limbs(vk->g2s_xy, g2s)) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "vk g2s is not a point of the twist in canonical coordinates");
    bool on_curve = g1_on_curve(vk->srs0_xy, vk->srs0_inf);
    for (int i = 0; i < 8; ++i) on_curve = on_curve && g1_on_curve(vk->commit_xy[i], vk->commit_inf[i]);
    if (!on_curve) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "a vk point is not on the curve");
    for (int i = 0; i < 3; ++i)
        if (!fr_canonical(vk->cosets[i])) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "vk coset is not a canonical residue");
    return TYPLONK_OK;
}
}  // namespace tyh

int typlonk_circuit_vk(typlonk_ctx* ctx, uint32_t srs_id, uint32_t circuit_id, const uint64_t cosets[3][4],
                       const uint64_t g2s_xy[24], typlonk_vk* vk) {
    if (!ctx || !cosets || !g2s_xy || !vk) return fail(ctx, TYPLONK_ERR_INVALID_ARG, "null argument");
    typlonk_vk out;
    if (comm_folds(ctx, srs_id)) {
        uint64_t rec_xy[9][12];
        uint8_t rec_inf[9];
        const int rc = statement_fold(ctx, srs_id, circuit_id, g2s_xy, 9, rec_xy, rec_inf);
        if (rc) return rc;
        vk_assemble(ctx->circuits.at(circuit_id).log_n, cosets, rec_xy, rec_inf, &out);
    } else {
        HIPCHK(hipSetDevice(ctx->device));
        P::G2Affine g2s;
        if (!g2_from_limbs(g2s_xy, &g2s)) return fail(ctx, TYPLONK_ERR_INVALID_ARG, G2S_REFUSED);
        const int rc = circuit_vk_fill(ctx, srs_id, circuit_id, cosets, &out);
        if (rc) return rc;
    }
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
    P::G2Affine g2s;
    const int args_rc = verify_compact_check_args(ctx, vk, count, pi, pi_len, &g2s);
    if (args_rc) return args_rc;
    const uint32_t log_n = vk->log_n;
    ProfilingOff prof_off(ctx);

    // ---- per-proof host checks: points, scalars, the transcript, zeta^n != 1 ----
    CompactVerifier v(ctx, proofs, count, log_n, vk->cosets, g2s);
    uint8_t d0_no_pi[64];   // the statement without public values, shared by every proof that has none
    compact_statement_digest(*vk, nullptr, 0, d0_no_pi);
    for (size_t k = 0; k < count; ++k) {
        const typlonk_proof_compact& pr = proofs[k];
        ProofState& ps = v.st[k];
        if (!v.views[k].admissible()) continue;
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
        ps.zn = v.zeta_pow_n(ps.zeta);
        if (ps.zn == Fr::one()) continue;   // zeta in the domain: Z_H(zeta) = 0 and the quotient is unconstrained
        ps.sig[0] = fr_load(pr.evals[5]);
        ps.sig[1] = fr_load(pr.evals[6]);
        ps.live = true;
    }
    const double t_host = ms_since(t_start);
    auto t0 = std::chrono::steady_clock::now();
    bool any_long = false;
    const int rc = pi_at_zeta(ctx, v.st, pi, pi_len, log_n, &any_long);
    if (rc) return rc;
    const double t_eval = ms_since(t0);
    t0 = std::chrono::steady_clock::now();

    // ---- rho: H("typlonk/compact/fold/v1" || vk_bytes || [s]G2 || every proof's points and evaluations || every PI(zeta)) ----
    static const char tag[] = "typlonk/compact/fold/v1";
    std::vector<uint8_t> bytes(tag, tag + sizeof(tag) - 1);
    bytes.reserve(1024 + count * (9 * 96 + 8 * 32));
    compact_vk_bytes(*vk, bytes);
    for (int i = 0; i < 24; ++i) compact_put_u64(bytes, vk->g2s_xy[i]);
    for (size_t k = 0; k < count; ++k)
        v.views[k].walk([&](const G1Ref& p) { compact_put_point(bytes, p.xy, p.inf); }, [&](const uint64_t* l) { compact_put_fr(bytes, l); });
    for (size_t k = 0; k < count; ++k) {
        uint64_t pv[4];
        fr_store(v.st[k].pi_eval, pv);   // zero for a proof the host checks rejected
        compact_put_fr(bytes, pv);
    }
    uint8_t h[64];
    blake2b_512(bytes.data(), bytes.size(), h);

    G1Ref shared[10];
    for (int i = 0; i < 8; ++i) shared[i] = {vk->commit_xy[i], vk->commit_inf[i]};
    shared[8] = {vk->srs0_xy, vk->srs0_inf};
    shared[9] = {G1_GEN, 0};
    return v.finish(fr_from_digest(h), shared, 10, ok, prof_off.saved, t_host, t0, any_long ? &t_eval : nullptr);
}
