// C++ host-side mirror of the reference's interface for the MSM + NTT path, written above the C ABI
// (include/typlonk.h).  The reference is Rust; this image has no Rust toolchain, so the host side is
// C++ with the reference's names, argument meaning and error behaviour (panics -> exceptions):
//
//   kzg::Srs                    /root/reference/kzg/src/srs.rs:8-51      (from_secret, g1_ref)
//   kzg::KzgScheme              /root/reference/kzg/src/lib.rs:15-86     (commit, open, identity)
//   kzg::KzgCommitment/Opening  /root/reference/kzg/src/lib.rs:16-31, 110-158
//   poly::DensePolynomial       ark-poly 0.3.0 as used by the reference  (from_coefficients_vec trims
//                               trailing zeros; degree(); evaluate = Horner; division by X - z)
//   poly::Radix2EvaluationDomain / Evaluations::interpolate / evaluate_over_domain
//                               call sites /root/reference/plonk/src/proof.rs:50,106,115 ;
//                               plonk/src/builder.rs:70,85 ; plonk/src/utils.rs:150-159 (l0_poly)
//   kzg::KzgScheme::verify      /root/reference/kzg/src/lib.rs:66-81 (host pairing, pairing_host.hpp); Srs::g2 srs.rs:26-34
//   plonk::CompiledCircuit      /root/reference/plonk/src/lib.rs:19-35 (srs, domain, gate_constrains, copy_constrains)
//   plonk::CompiledCircuit::verify
//                               /root/reference/plonk/src/proof.rs:195-281, 441-503 (verify, verify_challenges,
//                               verify_openings, linearisation_commitment), plonk/src/utils.rs:96-109
//   plonk::CompiledCircuit::prove / plonk::Proof
//                               /root/reference/plonk/src/proof.rs:26-57, 65-95, 96-194 -> typlonk_prove
//
// Every group / transform operation goes to the GPU through the C ABI; the O(n) glue the reference
// does on the CPU (Horner, synthetic division) is done on the CPU here too, with the library's own
// Fr arithmetic (csrc/ff.hpp).  Nothing here touches the oracle.
#pragma once
#include <array>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/typlonk.h"
#include "../csrc/ff.hpp"
#include "pairing_host.hpp"

namespace typlonk {

inline void check(int rc, typlonk_ctx* ctx = nullptr) {
    if (rc < 0)
        throw std::runtime_error(std::string(typlonk_strerror(rc)) + (ctx ? std::string(": ") + typlonk_last_error(ctx) : ""));
}

// ---- Fr ------------------------------------------------------------------------------------------
// Same bytes as ark_bls12_381::Fr: 4 x u64 little-endian Montgomery limbs.
struct Fr {
    ty::Fr v;
    Fr() : v(ty::Fr::zero()) {}
    explicit Fr(const ty::Fr& x) : v(x) {}
    Fr(int64_t x) {  // Fr::from(i32/i64): negative values wrap to r - |x|
        ty::Fr c = ty::Fr::zero();
        const uint64_t a = x < 0 ? (uint64_t)(-x) : (uint64_t)x;
        c.v[0] = (uint32_t)a;
        c.v[1] = (uint32_t)(a >> 32);
        v = ty::fe_to_mont(c);
        if (x < 0) v = ty::fe_neg(v);
    }
    static Fr zero() { return Fr(); }
    static Fr one() { return Fr(ty::Fr::one()); }
    bool is_zero() const { return v.is_zero(); }
    Fr operator+(const Fr& o) const { return Fr(ty::fe_add(v, o.v)); }
    Fr operator-(const Fr& o) const { return Fr(ty::fe_sub(v, o.v)); }
    Fr operator*(const Fr& o) const { return Fr(ty::fe_mul(v, o.v)); }
    Fr operator-() const { return Fr(ty::fe_neg(v)); }
    Fr& operator+=(const Fr& o) { return *this = *this + o; }
    Fr& operator-=(const Fr& o) { return *this = *this - o; }
    Fr& operator*=(const Fr& o) { return *this = *this * o; }
    bool operator==(const Fr& o) const { return v == o.v; }
    bool operator!=(const Fr& o) const { return !(v == o.v); }
    Fr inverse() const { return Fr(ty::fe_inv(v)); }
    Fr pow(uint64_t e) const {
        uint32_t w[2] = {(uint32_t)e, (uint32_t)(e >> 32)};
        return Fr(ty::fe_pow(v, w, 2));
    }
    const uint64_t* limbs() const { return reinterpret_cast<const uint64_t*>(v.v); }
    uint64_t* limbs() { return reinterpret_cast<uint64_t*>(v.v); }
};
static_assert(sizeof(Fr) == 32, "Fr must be 4 x u64");

// ---- context (one per process / GPU) --------------------------------------------------------------
class Context {
   public:
    explicit Context(int device = 0) { check(typlonk_init(&ctx_, device)); }
    ~Context() { typlonk_destroy(ctx_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    typlonk_ctx* raw() const { return ctx_; }
    // ---- multi-GPU: one process per GPU, the library's own exchange (include/typlonk.h, typlonk_comm_*) ----
    // rank 0 creates the rendezvous id and hands its bytes to the other ranks by whatever channel the host program has
    static std::array<uint8_t, TYPLONK_COMM_ID_BYTES> comm_unique_id() {
        std::array<uint8_t, TYPLONK_COMM_ID_BYTES> id{};
        check(typlonk_comm_unique_id(id.data()));
        return id;
    }
    // collective: returns once all `world` ranks have called it
    void comm_init(const std::array<uint8_t, TYPLONK_COMM_ID_BYTES>& id, int rank, int world) const {
        check(typlonk_comm_init(ctx_, id.data(), rank, world), ctx_);
    }
    void comm_destroy() const { check(typlonk_comm_destroy(ctx_), ctx_); }

   private:
    typlonk_ctx* ctx_ = nullptr;
};

namespace poly {

// ark-poly 0.3.0 DensePolynomial<Fr>
struct DensePolynomial {
    std::vector<Fr> coeffs;

    static DensePolynomial from_coefficients_vec(std::vector<Fr> c) {
        while (!c.empty() && c.back().is_zero()) c.pop_back();  // ark-poly trims trailing zeros
        DensePolynomial p;
        p.coeffs = std::move(c);
        return p;
    }
    static DensePolynomial from_coefficients_slice(const std::vector<Fr>& c) { return from_coefficients_vec(c); }
    bool is_zero() const { return coeffs.empty(); }
    size_t degree() const { return coeffs.empty() ? 0 : coeffs.size() - 1; }
    Fr evaluate(const Fr& x) const {  // Horner
        Fr acc;
        for (size_t i = coeffs.size(); i-- > 0;) acc = acc * x + coeffs[i];
        return acc;
    }
    // (self - self(z)) / (X - z): the division `&polynomial / &root` of kzg/src/lib.rs:58-61.
    // Returns the quotient; *y receives self(z).
    DensePolynomial divide_by_linear(const Fr& z, Fr* y) const {
        std::vector<Fr> q(coeffs.size() > 0 ? coeffs.size() - 1 : 0);
        Fr carry;
        for (size_t i = coeffs.size(); i-- > 1;) {
            carry = carry * z + coeffs[i];
            q[i - 1] = carry;
        }
        if (!coeffs.empty()) carry = carry * z + coeffs[0];
        if (y) *y = carry;
        return from_coefficients_vec(std::move(q));
    }
    DensePolynomial operator*(const Fr& k) const {
        std::vector<Fr> c(coeffs);
        for (auto& x : c) x *= k;
        return from_coefficients_vec(std::move(c));
    }
};

// Fr::get_root_of_unity(2^log_size): TWO_ADIC_ROOT_OF_UNITY = 7^((r-1)/2^32), squared (32 - log_size) times
inline Fr two_adic_root(uint32_t log_size) {
    if (log_size > 32) check(TYPLONK_ERR_DOMAIN);
    ty::Fr c;
    const uint32_t root[8] = {0x439f0d2bu, 0x3829971fu, 0x8c2280b9u, 0xb6368350u, 0x22c813b4u, 0xd09b6819u, 0xdfe81f20u, 0x16a2a19eu};
    for (int i = 0; i < 8; ++i) c.v[i] = root[i];
    Fr w(ty::fe_to_mont(c));
    for (uint32_t i = log_size; i < 32; ++i) w = w * w;
    return w;
}

// ark-poly 0.3.0 Radix2EvaluationDomain<Fr> (what GeneralEvaluationDomain::new returns for BLS12-381 Fr)
class Radix2EvaluationDomain {
   public:
    // GeneralEvaluationDomain::new(num_coeffs): size = next power of two; None (here: exception, the
    // reference unwrap()s, plonk/src/builder.rs:70) beyond the two-adicity 2^32.
    Radix2EvaluationDomain(const Context& ctx, uint64_t num_coeffs) : ctx_(&ctx) {
        log_size_ = 0;
        while ((1ull << log_size_) < num_coeffs) {
            if (++log_size_ > 32) check(TYPLONK_ERR_DOMAIN);
        }
        size_ = 1ull << log_size_;
        const Fr w = two_adic_root(log_size_);
        group_gen = w;
        group_gen_inv = w.inverse();
        size_inv = Fr((int64_t)size_).inverse();
    }
    uint64_t size() const { return size_; }
    uint32_t log_size_of_group() const { return log_size_; }
    Fr element(uint64_t i) const { return group_gen.pow(i); }
    Fr evaluate_vanishing_polynomial(const Fr& tau) const { return tau.pow(size_) - Fr::one(); }

    // natural order in / out; input shorter than size() is zero-padded (ark-poly fft semantics)
    std::vector<Fr> fft(const std::vector<Fr>& coeffs) const { return transform(coeffs, 0, nullptr); }
    std::vector<Fr> ifft(const std::vector<Fr>& evals) const { return transform(evals, 1, nullptr); }
    std::vector<Fr> coset_fft(const std::vector<Fr>& coeffs, const Fr& g) const { return transform(coeffs, 0, &g); }
    std::vector<Fr> coset_ifft(const std::vector<Fr>& evals, const Fr& g) const { return transform(evals, 1, &g); }

    Fr group_gen, group_gen_inv, size_inv;

   private:
    std::vector<Fr> transform(const std::vector<Fr>& in, int inverse, const Fr* coset) const {
        if (in.size() > size_) throw std::runtime_error("more coefficients than the domain size");
        std::vector<Fr> v(in);
        v.resize(size_);
        check(typlonk_ntt_fr(ctx_->raw(), v[0].limbs(), log_size_, inverse, coset ? coset->limbs() : nullptr), ctx_->raw());
        return v;
    }
    const Context* ctx_;
    uint64_t size_;
    uint32_t log_size_;
};

// Evaluations::from_vec_and_domain(v, D).interpolate()  /  DensePolynomial::evaluate_over_domain(D)
inline DensePolynomial interpolate(const std::vector<Fr>& evals, const Radix2EvaluationDomain& d) {
    return DensePolynomial::from_coefficients_vec(d.ifft(evals));
}
inline std::vector<Fr> evaluate_over_domain(const DensePolynomial& p, const Radix2EvaluationDomain& d) {
    return d.fft(p.coeffs);
}
// A GROUP of interpolations -- the reference maps `interpolate` over the three wire columns (plonk/src/proof.rs:50), the five
// selector columns (plonk/src/builder.rs:84-88), the three sigma columns (proof.rs:334-338): one upload, ONE
// typlonk_ntt_fr_batch_devptr (every pass one launch for all columns), one download; ark-poly's trim per column.
inline std::vector<DensePolynomial> interpolate_batch(const Context& ctx, const std::vector<std::vector<Fr>>& columns,
                                                      const Radix2EvaluationDomain& d) {
    const size_t count = columns.size(), n = d.size();
    std::vector<DensePolynomial> out;
    if (!count) return out;
    typlonk_ctx* c = ctx.raw();
    typlonk_buf* buf = nullptr;
    check(typlonk_buf_alloc(c, n * count, &buf), c);
    struct Free {
        typlonk_ctx* c;
        typlonk_buf* b;
        ~Free() { typlonk_buf_free(c, b); }
    } guard{c, buf};
    std::vector<void*> ptrs(count);
    for (size_t v = 0; v < count; ++v) {
        if (columns[v].size() != n) throw std::runtime_error("every column must hold n evaluations");
        check(typlonk_buf_upload(c, buf, v * n, columns[v][0].limbs(), n), c);
        ptrs[v] = (char*)typlonk_buf_devptr(buf) + 32 * n * v;
    }
    check(typlonk_ntt_fr_batch_devptr(c, ptrs.data(), count, d.log_size_of_group(), 1, nullptr), c);
    for (size_t v = 0; v < count; ++v) {
        std::vector<Fr> co(n);
        check(typlonk_buf_download(c, buf, v * n, co[0].limbs(), n), c);
        out.push_back(DensePolynomial::from_coefficients_vec(std::move(co)));
    }
    return out;
}

}  // namespace poly

namespace kzg {

using Poly = poly::DensePolynomial;

// ark_bls12_381::G1Affine at the C ABI: x || y Montgomery limbs + infinity flag
struct G1Point {
    uint64_t xy[12];
    bool infinity;
    bool operator==(const G1Point& o) const {
        if (infinity || o.infinity) return infinity == o.infinity;
        return std::memcmp(xy, o.xy, sizeof(xy)) == 0;
    }
    bool operator!=(const G1Point& o) const { return !(*this == o); }
};

// kzg/src/srs.rs: g1 = [G, sG, s^2 G, ...] of length gates + 3, resident on the device
class Srs {
   public:
    static Srs from_secret(const Context& ctx, const Fr& s, size_t gates) {
        Srs r(ctx);
        r.len_ = gates + 3;
        typlonk::check(typlonk_srs_generate(ctx.raw(), s.limbs(), 0, r.len_, &r.id_), ctx.raw());
        // srs.rs:26-34: g2 = generator, g2s = [s] generator (host-side: the verifier's two G2 elements)
        r.g2_ = pairing::g2_generator();
        r.g2s_ = pairing::g2_mul(r.g2_, s.v);
        r.has_g2_ = true;
        return r;
    }
    // Multi-GPU: this rank's slice [first, first + count) of the same SRS (typlonk_srs_set_shard).  On a context with a
    // communicator (Context::comm_init) plonk::CompiledCircuit's constructor, verifying_key() and prove_compact() are then
    // COLLECTIVES every rank must call in the same order; each returns what one GPU holding the whole SRS returns.
    static Srs from_secret_shard(const Context& ctx, const Fr& s, size_t gates, size_t first, size_t count) {
        Srs r(ctx);
        r.len_ = gates + 3;
        r.local_len_ = count;
        r.sharded_ = true;
        typlonk::check(typlonk_srs_generate(ctx.raw(), s.limbs(), first, count, &r.id_), ctx.raw());
        typlonk::check(typlonk_srs_set_shard(ctx.raw(), r.id_, first, r.len_), ctx.raw());
        r.g2_ = pairing::g2_generator();
        r.g2s_ = pairing::g2_mul(r.g2_, s.v);
        r.has_g2_ = true;
        return r;
    }
    bool sharded() const { return sharded_; }
    // an SRS loaded from points brings its G2 pair along (needed by KzgScheme::verify only)
    void set_g2(const pairing::G2Affine& g2, const pairing::G2Affine& g2s) {
        g2_ = g2;
        g2s_ = g2s;
        has_g2_ = true;
    }
    const pairing::G2Affine& g2() const {
        if (!has_g2_) throw std::runtime_error("this SRS has no G2 elements");
        return g2_;
    }
    const pairing::G2Affine& g2s() const {
        if (!has_g2_) throw std::runtime_error("this SRS has no G2 elements");
        return g2s_;
    }
    static Srs from_points(const Context& ctx, const std::vector<G1Point>& pts) {
        Srs r(ctx);
        r.len_ = pts.size();
        std::vector<uint64_t> xy(pts.size() * 12);
        std::vector<uint8_t> inf(pts.size());
        for (size_t i = 0; i < pts.size(); ++i) {
            std::memcpy(&xy[i * 12], pts[i].xy, 96);
            inf[i] = pts[i].infinity;
        }
        typlonk::check(typlonk_srs_load(ctx.raw(), xy.data(), inf.data(), pts.size(), &r.id_), ctx.raw());
        return r;
    }
    Srs(Srs&& o) noexcept
        : ctx_(o.ctx_), id_(o.id_), len_(o.len_), local_len_(o.local_len_), sharded_(o.sharded_), g2_(o.g2_), g2s_(o.g2s_),
          has_g2_(o.has_g2_) {
        o.id_ = 0;
    }
    Srs(const Srs&) = delete;
    ~Srs() {
        if (id_) typlonk_srs_free(ctx_->raw(), id_);
    }
    size_t len() const { return len_; }   // of the whole SRS, also on a shard
    // optional, once per SRS: fixed-base tables in HBM (window chosen by the library from the length when 0); every later
    // commitment over this SRS is faster, results are unchanged -- nothing in the reference corresponds to it
    void precompute(uint32_t window_bits = 0) const { typlonk::check(typlonk_srs_precompute(ctx_->raw(), id_, window_bits), ctx_->raw()); }
    // typlonk_srs_check against this SRS's own g2s: is g1[i] = [s^i] G for the s of g2s()?  seed: 32 bytes that whoever
    // produced the points cannot have known (typlonk.h).  An invalid SRS is the report's verdict, not an exception; nothing
    // in the reference corresponds to it (Srs::from_secret trusts itself).  (The name hides the status check typlonk::check
    // inside this class, which is why the calls here are qualified.)
    typlonk_srs_report check(const uint8_t seed[32]) const {
        uint64_t limbs[24];
        g2s_limbs(limbs);
        typlonk_srs_report rep;
        typlonk::check(typlonk_srs_check(ctx_->raw(), id_, limbs, seed, &rep), ctx_->raw());
        return rep;
    }
    // typlonk_srs_contribute: a new SRS [t^i] g1[i] with its own g2s = [t] g2s() (and the same g2): an SRS for s t
    Srs contribute(const Fr& t) const {
        uint64_t in[24], out[24];
        g2s_limbs(in);
        Srs r(*ctx_);
        r.len_ = len_;
        typlonk::check(typlonk_srs_contribute(ctx_->raw(), id_, t.limbs(), in, &r.id_, out), ctx_->raw());
        pairing::G2Affine q;
        std::memcpy(q.x.a.v, out, 48);
        std::memcpy(q.x.b.v, out + 6, 48);
        std::memcpy(q.y.a.v, out + 12, 48);
        std::memcpy(q.y.b.v, out + 18, 48);
        q.infinity = false;
        r.set_g2(g2_, q);
        return r;
    }
    // typlonk_srs_g1_ntt: the Lagrange form [L_i(s)] G, i < 2^log_n, of this (monomial) SRS as an SRS of its own, with the same
    // G2 elements, and the way back: the 2^log_n monomial points of a Lagrange SRS.  check() tests the monomial form only.
    // KzgScheme::commit_evaluations commits over the Lagrange form; the provers keep taking the monomial one.
    Srs lagrange(uint32_t log_n) const { return g1_ntt(log_n, TYPLONK_SRS_TO_LAGRANGE); }
    Srs from_lagrange(uint32_t log_n) const { return g1_ntt(log_n, TYPLONK_SRS_FROM_LAGRANGE); }
    // typlonk_srs_open_all_table: the table KzgScheme::open_all needs for the domain of 2^log_n points over this (monomial) SRS:
    // 2^(log_n + 1) records held like an SRS (len() reports them, the destructor frees them) that are no SRS to commit over.
    // Nothing in the reference corresponds to it (it opens point by point).
    Srs open_all_table(uint32_t log_n) const {
        Srs r(*ctx_);
        typlonk::check(typlonk_srs_open_all_table(ctx_->raw(), id_, log_n, &r.id_), ctx_->raw());
        r.len_ = (size_t)2 << log_n;
        if (has_g2_) r.set_g2(g2_, g2s_);
        return r;
    }
    // typlonk_srs_open_chunks_table: the table KzgScheme::open_chunks needs for the domain of 2^log_n points cut into cosets of 2^log_l
    // points -- held as open_all_table's, which it is, word for word, at log_l = 0.  chunk_log_l() reports the log_l of a table.
    Srs open_chunks_table(uint32_t log_n, uint32_t log_l) const {
        Srs r(*ctx_);
        typlonk::check(typlonk_srs_open_chunks_table(ctx_->raw(), id_, log_n, log_l, &r.id_), ctx_->raw());
        r.len_ = (size_t)2 << log_n;
        r.chunk_log_l_ = log_l;
        if (has_g2_) r.set_g2(g2_, g2s_);
        return r;
    }
    uint32_t chunk_log_l() const { return chunk_log_l_; }
    std::vector<G1Point> g1_ref() const {  // downloads the points (the reference returns &Vec<G1Point>); a shard: its slice
        const size_t cnt = sharded_ ? local_len_ : len_;
        std::vector<uint64_t> xy(cnt * 12);
        std::vector<uint8_t> inf(cnt);
        typlonk::check(typlonk_srs_download(ctx_->raw(), id_, 0, cnt, xy.data(), inf.data()), ctx_->raw());
        std::vector<G1Point> out(cnt);
        for (size_t i = 0; i < cnt; ++i) {
            std::memcpy(out[i].xy, &xy[i * 12], 96);
            out[i].infinity = inf[i] != 0;
        }
        return out;
    }
    G1Point g1_generator() const {  // g1_ref()[0] without the other len - 1 points
        G1Point g;
        uint8_t inf = 0;
        typlonk::check(typlonk_srs_download(ctx_->raw(), id_, 0, 1, g.xy, &inf), ctx_->raw());
        g.infinity = inf != 0;
        return g;
    }
    uint32_t id() const { return id_; }
    const Context& ctx() const { return *ctx_; }

   private:
    explicit Srs(const Context& c) : ctx_(&c) {}
    Srs g1_ntt(uint32_t log_n, uint32_t direction) const {
        Srs r(*ctx_);
        typlonk::check(typlonk_srs_g1_ntt(ctx_->raw(), id_, log_n, direction, &r.id_), ctx_->raw());
        r.len_ = (size_t)1 << log_n;
        if (has_g2_) r.set_g2(g2_, g2s_);
        return r;
    }
    void g2s_limbs(uint64_t out[24]) const {   // x.c0 x.c1 y.c0 y.c1 (throws without G2 elements)
        const pairing::G2Affine& q = g2s();
        std::memcpy(out, q.x.a.v, 48);
        std::memcpy(out + 6, q.x.b.v, 48);
        std::memcpy(out + 12, q.y.a.v, 48);
        std::memcpy(out + 18, q.y.b.v, 48);
    }
    const Context* ctx_;
    uint32_t id_ = 0;
    size_t len_ = 0, local_len_ = 0;
    bool sharded_ = false;
    uint32_t chunk_log_l_ = 0;
    pairing::G2Affine g2_{}, g2s_{};
    bool has_g2_ = false;
};

struct KzgCommitment {
    G1Point p;
    const G1Point& inner() const { return p; }
    bool operator==(const KzgCommitment& o) const { return p == o.p; }
};
struct KzgOpening {
    G1Point p;
    Fr y;
    Fr eval() const { return y; }
};

// one multi-proof: the opening of a polynomial at the l points w^(k + r t), t < l, of coset k, with its l evaluations in that order
struct KzgChunkOpening {
    G1Point p;
    std::vector<Fr> ys;
};

// one cell of KzgScheme::verify_chunks: a multi-proof, the commitment it is claimed against (an index into the call's
// commitments) and its coset
struct KzgCell {
    uint32_t commitment, coset;
    KzgChunkOpening opening;
};
struct KzgCellVerdicts {
    std::vector<uint8_t> status;    // TYPLONK_CELL_* per cell
    typlonk_chunks_report report;
    bool all_ok() const { return report.count[TYPLONK_CELL_OK] == status.size(); }
};

// what KzgScheme::recover_chunks returns: per polynomial the recovered coefficients (m of them; all zero when its status is not
// TYPLONK_RECOVER_OK), the status, and for an inconsistent one the lowest excess coefficient
struct KzgRecovered {
    std::vector<std::vector<Fr>> coeffs;
    std::vector<uint8_t> status;          // TYPLONK_RECOVER_* per polynomial
    std::vector<uint64_t> first_excess;   // UINT64_MAX unless TYPLONK_RECOVER_INCONSISTENT
    typlonk_recover_report report;
    bool all_ok() const { return report.count[TYPLONK_RECOVER_OK] == status.size(); }
    Poly poly(size_t p) const { return Poly::from_coefficients_vec(coeffs[p]); }
};

class KzgScheme {
   public:
    explicit KzgScheme(const Srs& srs) : srs_(srs) {}
    KzgCommitment commit(const Poly& polynomial) const { return KzgCommitment{evaluate_in_s(polynomial)}; }
    // kzg/src/lib.rs:55-64
    KzgOpening open(const Poly& polynomial, const Fr& z) const {
        if (polynomial.coeffs.empty()) throw std::runtime_error("at least 1");  // `.expect("at least 1")`
        Fr y;
        const Poly q = polynomial.divide_by_linear(z, &y);
        return KzgOpening{evaluate_in_s(q), y};
    }
    // open(polynomial, w^k) for every k < n in one call (typlonk_open_all_host), n = table.len() / 2 the domain of `table`
    // (Srs::open_all_table of this scheme's SRS) and w its generator: result[k] is what open() gives at Radix2EvaluationDomain
    // (n).element(k).  1 <= coefficients <= n.
    std::vector<KzgOpening> open_all(const Srs& table, const Poly& polynomial) const {
        if (polynomial.coeffs.empty()) throw std::runtime_error("at least 1");
        const size_t n = table.len() / 2;
        std::vector<uint64_t> xy(n * 12);
        std::vector<uint8_t> inf(n);
        std::vector<Fr> ys(n);
        check(typlonk_open_all_host(srs_.ctx().raw(), table.id(), polynomial.coeffs[0].limbs(), polynomial.coeffs.size(), xy.data(),
                                    inf.data(), ys[0].limbs()),
              srs_.ctx().raw());
        std::vector<KzgOpening> out(n);
        for (size_t k = 0; k < n; ++k) {
            std::memcpy(out[k].p.xy, &xy[k * 12], 96);
            out[k].p.infinity = inf[k] != 0;
            out[k].y = ys[k];
        }
        return out;
    }
    // typlonk_open_chunks_host: for each polynomial (all of one length, 1 <= coefficients <= n) its r = n / l multi-proofs over
    // `table` (Srs::open_chunks_table or open_all_table of this scheme's SRS), l = 2^table.chunk_log_l(): result[p][k] opens
    // polynomial p on coset k, the roots of X^l - w^(k l).  A verifier needs [s^l]G2, which an Srs does not hold.
    std::vector<std::vector<KzgChunkOpening>> open_chunks(const Srs& table, const std::vector<Poly>& polynomials) const {
        if (polynomials.empty() || polynomials[0].coeffs.empty()) throw std::runtime_error("at least 1");
        const size_t n = table.len() / 2, l = (size_t)1 << table.chunk_log_l(), r = n / l, count = polynomials.size();
        const size_t m = polynomials[0].coeffs.size();
        std::vector<const uint64_t*> co(count);
        for (size_t p = 0; p < count; ++p) {
            if (polynomials[p].coeffs.size() != m) throw std::runtime_error("open_chunks: the polynomials of one call have one length");
            co[p] = polynomials[p].coeffs[0].limbs();
        }
        std::vector<uint64_t> xy(count * r * 12);
        std::vector<uint8_t> inf(count * r);
        std::vector<Fr> ys(count * n);
        check(typlonk_open_chunks_host(srs_.ctx().raw(), table.id(), co.data(), m, count, xy.data(), inf.data(), ys[0].limbs()),
              srs_.ctx().raw());
        std::vector<std::vector<KzgChunkOpening>> out(count, std::vector<KzgChunkOpening>(r));
        for (size_t p = 0; p < count; ++p)
            for (size_t k = 0; k < r; ++k) {
                KzgChunkOpening& o = out[p][k];
                std::memcpy(o.p.xy, &xy[(p * r + k) * 12], 96);
                o.p.infinity = inf[p * r + k] != 0;
                o.ys.assign(ys.begin() + (p * n + k * l), ys.begin() + (p * n + (k + 1) * l));
            }
        return out;
    }
    // typlonk_verify_chunks: the cells (multi-proofs of open_chunks, in any order, from any number of polynomials) against
    // `commitments`, over the domain of 2^log_n points cut into cosets of 2^log_l.  g2sl = [s^l]G2 for the s of this scheme's
    // SRS, which an Srs does not hold; seed: 32 bytes that whoever made the cells cannot have known (typlonk.h).  A bad cell
    // is its status, not an exception.
    KzgCellVerdicts verify_chunks(uint32_t log_n, uint32_t log_l, const pairing::G2Affine& g2sl, const uint8_t seed[32],
                                  const std::vector<KzgCommitment>& commitments, const std::vector<KzgCell>& cells) const {
        const size_t N = cells.size(), M = commitments.size(), l = (size_t)1 << log_l;
        uint64_t g2[24];
        std::memcpy(g2, g2sl.x.a.v, 48);
        std::memcpy(g2 + 6, g2sl.x.b.v, 48);
        std::memcpy(g2 + 12, g2sl.y.a.v, 48);
        std::memcpy(g2 + 18, g2sl.y.b.v, 48);
        std::vector<uint64_t> cxy(M * 12 + 1), pxy(N * 12 + 1), ev(N * l * 4 + 1);   // (+ 1: data() is never null)
        std::vector<uint8_t> cinf(M + 1), pinf(N + 1);
        std::vector<uint32_t> cc(N + 1), ck(N + 1);
        for (size_t c = 0; c < M; ++c) {
            std::memcpy(&cxy[c * 12], commitments[c].p.xy, 96);
            cinf[c] = commitments[c].p.infinity;
        }
        for (size_t i = 0; i < N; ++i) {
            if (cells[i].opening.ys.size() != l) throw std::runtime_error("verify_chunks: a cell holds 2^log_l evaluations");
            std::memcpy(&pxy[i * 12], cells[i].opening.p.xy, 96);
            pinf[i] = cells[i].opening.p.infinity;
            cc[i] = cells[i].commitment;
            ck[i] = cells[i].coset;
            std::memcpy(&ev[i * l * 4], cells[i].opening.ys[0].limbs(), l * 32);
        }
        KzgCellVerdicts out;
        out.status.assign(N + 1, 0);
        check(typlonk_verify_chunks(srs_.ctx().raw(), srs_.id(), log_n, log_l, g2, seed, cxy.data(), cinf.data(), M, cc.data(), ck.data(),
                                    ev.data(), pxy.data(), pinf.data(), N, out.status.data(), &out.report),
              srs_.ctx().raw());
        out.status.resize(N);
        return out;
    }
    // typlonk_recover_chunks: the polynomials of degree < m whose cells on the K distinct cosets `cosets` (any order, the same for
    // every polynomial) are cells[p][i], the l = 2^log_l evaluations on coset cosets[i] in open_chunks' order.  It uses this
    // scheme's context and no SRS.  A polynomial whose cells no polynomial of degree < m takes, or that holds a value that is no
    // canonical residue, is its status, not an exception.
    KzgRecovered recover_chunks(uint32_t log_n, uint32_t log_l, size_t m, const std::vector<uint32_t>& cosets,
                                const std::vector<std::vector<std::vector<Fr>>>& cells) const {
        const size_t count = cells.size(), K = cosets.size(), l = log_l < 32 ? (size_t)1 << log_l : 0;
        std::vector<uint64_t> ev(count * K * l * 4 + 1), co(count * m * 4 + 1);   // (+ 1: data() is never null)
        for (size_t p = 0; p < count; ++p) {
            if (cells[p].size() != K) throw std::runtime_error("recover_chunks: one cell per named coset");
            for (size_t i = 0; i < K; ++i) {
                if (cells[p][i].size() != l) throw std::runtime_error("recover_chunks: a cell holds 2^log_l evaluations");
                if (l) std::memcpy(&ev[(p * K + i) * l * 4], cells[p][i][0].limbs(), l * 32);
            }
        }
        std::vector<uint32_t> ck(cosets);
        ck.push_back(0);
        KzgRecovered out;
        out.status.assign(count + 1, 0);
        out.first_excess.assign(count + 1, 0);
        check(typlonk_recover_chunks(srs_.ctx().raw(), log_n, log_l, m, ck.data(), K, ev.data(), count, nullptr, nullptr, co.data(), nullptr,
                                     out.status.data(), out.first_excess.data(), &out.report),
              srs_.ctx().raw());
        out.status.resize(count);
        out.first_excess.resize(count);
        out.coeffs.assign(count, std::vector<Fr>(m));
        for (size_t p = 0; p < count; ++p) std::memcpy(out.coeffs[p][0].limbs(), &co[p * m * 4], m * 32);
        return out;
    }
    KzgCommitment identity() const { return commit(Poly::from_coefficients_vec({Fr(1)})); }
    // over a LAGRANGE Srs (Srs::lagrange): the commitment to the polynomial whose evaluations over the domain of srs.len()
    // points these are -- commit(interpolate(evals)) over the monomial Srs -- as one MSM, with no transform
    KzgCommitment commit_evaluations(const std::vector<Fr>& evals) const {
        if (evals.size() > srs_.len()) throw std::runtime_error("more evaluations than Lagrange points");
        return KzgCommitment{msm(evals)};
    }
    // kzg/src/lib.rs:66-81: pairing(W, [s]G2 - z G2) == pairing(C - y G1, G2), as e(W, A) * e(-(C - y G1), G2) == 1
    bool verify(const KzgCommitment& commitment, const KzgOpening& opening, const Fr& z) const;
    const Srs& srs() const { return srs_; }

   private:
    // kzg/src/lib.rs:41-54: assert!(srs.len() > degree) then sum coeff_i * srs_i -> the MSM
    G1Point evaluate_in_s(const Poly& polynomial) const {
        if (!(srs_.len() > polynomial.degree())) throw std::runtime_error("assertion failed: srs.len() > polynomial.degree()");
        return msm(polynomial.coeffs);
    }
    G1Point msm(const std::vector<Fr>& scalars) const {   // sum scalars_i * srs_i
        G1Point out;
        uint8_t inf = 0;
        const uint64_t* sc = scalars.empty() ? nullptr : scalars[0].limbs();
        check(typlonk_msm_g1(srs_.ctx().raw(), srs_.id(), sc, scalars.size(), out.xy, &inf), srs_.ctx().raw());
        out.infinity = inf != 0;
        return out;
    }
    const Srs& srs_;
};

// group helpers used by the tests (KzgCommitment: Add / Mul<Fr>, kzg/src/lib.rs:110-158)
inline G1Point g1_add(const G1Point& a, const G1Point& b) {
    uint64_t xy[24];
    uint8_t inf[2] = {(uint8_t)a.infinity, (uint8_t)b.infinity};
    std::memcpy(xy, a.xy, 96);
    std::memcpy(xy + 12, b.xy, 96);
    G1Point out;
    uint8_t oi = 0;
    check(typlonk_g1_sum_host(xy, inf, 2, out.xy, &oi));
    out.infinity = oi != 0;
    return out;
}
inline G1Point g1_mul(const Context& ctx, const G1Point& p, const Fr& k) {
    Srs one = Srs::from_points(ctx, {p});
    return KzgScheme(one).commit(Poly::from_coefficients_vec({k})).p;
}
inline G1Point g1_neg(const Context& ctx, const G1Point& p) { return g1_mul(ctx, p, -Fr::one()); }
// sum_i k_i P_i: one small MSM over an SRS made of the points (the verifier's linear combinations of commitments)
inline G1Point g1_lincomb(const Context& ctx, const std::vector<G1Point>& pts, const std::vector<Fr>& ks) {
    Srs bases = Srs::from_points(ctx, pts);
    std::vector<Fr> c = ks;
    G1Point out;
    uint8_t inf = 0;
    check(typlonk_msm_g1(ctx.raw(), bases.id(), c[0].limbs(), c.size(), out.xy, &inf), ctx.raw());
    out.infinity = inf != 0;
    return out;
}
inline pairing::G1Aff to_pairing(const G1Point& p, bool negate = false) {
    pairing::G1Aff a;
    std::memcpy(a.x.v, p.xy, 48);
    std::memcpy(a.y.v, p.xy + 6, 48);
    if (negate) a.y = ty::fe_neg(a.y);
    a.infinity = p.infinity;
    return a;
}
// C - y * G on the host (g1_host64.hpp), G = the FIXED generator G1Point::prime_subgroup_generator() the reference's
// verifier uses (kzg/src/lib.rs:76) -- not srs[0], which an Srs::from_points caller is free to choose --, with no device
// round trip: a verifier that checks six openings does twelve double-and-add ladders on the host instead of six SRS
// uploads + MSMs.
inline G1Point g1_sub_y_times_generator(const G1Point& c, const Fr& y) {
    namespace H = ty::h64;
    // arkworks' Montgomery limbs of the generator (the constants pinned in tests/test_oracle.py)
    static const uint64_t GEN[12] = {0x5cb38790fd530c16ull, 0x7817fc679976fff5ull, 0x154f95c7143ba1c1ull, 0xf0ae6acdf3d0e747ull,
                                     0xedce6ecc21dbf440ull, 0x120177419e0bfb75ull, 0xbaac93d50ce72271ull, 0x8c22631a7918fd8eull,
                                     0xdd595f13570725ceull, 0x51ac582950405194ull, 0x0e1c8c3fad0059c0ull, 0x0bbc3efc5008a26aull};
    static const uint64_t ONE[6] = {0x760900000002fffdull, 0xebf4000bc40c0002ull, 0x5f48985753c758baull,
                                    0x77ce585370525745ull, 0x5c071a97a256ec6dull, 0x15f65ec3fa80e493ull};   // R mod p
    auto lift = [&](const uint64_t* xy) {
        H::Xyzz r;
        std::memcpy(r.x.v, xy, 48);
        std::memcpy(r.y.v, xy + 6, 48);
        std::memcpy(r.zz.v, ONE, 48);
        std::memcpy(r.zzz.v, ONE, 48);
        return r;
    };
    const ty::Fr k = ty::fe_from_mont(ty::fe_neg(y.v));   // canonical -y
    const H::Xyzz g = lift(GEN);
    H::Xyzz acc = H::inf();
    for (int w = 7; w >= 0; --w)
        for (int b = 31; b >= 0; --b) {
            acc = H::xyzz_dbl(acc);
            if ((k.v[w] >> b) & 1u) acc = H::xyzz_add(acc, g);
        }
    if (!c.infinity) acc = H::xyzz_add(acc, lift(c.xy));
    G1Point out;
    out.infinity = !H::xyzz_to_affine(acc, out.xy);
    if (out.infinity) {
        std::memset(out.xy, 0, 48);
        std::memcpy(out.xy + 6, ONE, 48);   // GroupAffine::zero() = (0, 1, infinity)
    }
    return out;
}
inline bool KzgScheme::verify(const KzgCommitment& commitment, const KzgOpening& opening, const Fr& z) const {
    const pairing::G2Affine a = pairing::g2_add(srs_.g2s(), pairing::g2_neg(pairing::g2_mul(srs_.g2(), z.v)));
    const G1Point b = g1_sub_y_times_generator(commitment.p, opening.y);  // C - y G1
    const pairing::G1Aff ps[2] = {to_pairing(opening.p), to_pairing(b, /*negate=*/true)};
    const pairing::G2Affine qs[2] = {a, srs_.g2()};
    return pairing::pairing_product_is_one(ps, qs, 2);
}

}  // namespace kzg

namespace plonk {

// plonk::proof::Proof (/root/reference/plonk/src/proof.rs:65-95)
struct PermutationProof {
    kzg::KzgCommitment commitment;
    kzg::KzgOpening z, zw;
};
struct Proof {
    kzg::KzgCommitment a_commit, b_commit, c_commit;
    kzg::KzgOpening a, b, c;          // openings at evaluation_point
    PermutationProof permutation;     // [Z], Z at zeta, Z at zeta * w
    Fr evaluation_point;              // zeta
    kzg::KzgCommitment t[3];          // quotient slices
    kzg::KzgOpening r;                // linearisation polynomial at zeta: r.eval() == 0 for a valid proof
    Fr beta, gamma, alpha;            // the challenges used (the reference's verifier recomputes them, :236-246)
    std::vector<Fr> public_inputs;    // padded column (filled by plonk::Circuit::prove; the verifier reads it, :205-210)
};

// The prover-relevant part of plonk::CompiledCircuit (/root/reference/plonk/src/lib.rs:19-35): the SRS, the domain,
// the five selector polynomials (gate_constrains, builder.rs:76-90) and the sigma columns with their cosets
// (copy_constrains, permutation/src/lib.rs:141-154).  The tables come from the front end
// (CircuitDescription::build; circuit_host.hpp) as EVALUATIONS over the domain, exactly as builder.rs:85 interpolates
// them; they are interpolated on the device once and cached for every later proof (typlonk_circuit_load).
// a copy constraint: two flat cells col * n + row that must carry one value (PermutationBuilder::add_constrain)
struct CellPair {
    uint32_t a, b;
};
static_assert(sizeof(CellPair) == 8, "a pair list is the C ABI's array of 2 * count cells");

// Permutation { perm } (permutation/src/lib.rs:95-98) as PermutationBuilder::build would make it from the pairs, but canonical:
// every class of cells ascending, its highest cell back to its lowest (typlonk_permutation_from_pairs; on the device)
struct CellPermutation {
    std::vector<uint32_t> perm;   // 3n successors
    uint64_t classes = 0;         // classes among the 3n cells, singletons included
    static CellPermutation from_pairs(const Context& ctx, uint32_t log_n, const std::vector<CellPair>& pairs) {
        CellPermutation out;
        if (log_n >= 1 && log_n <= TYPLONK_MAX_PROVER_LOG_N) out.perm.resize((size_t)3 << log_n);
        check(typlonk_permutation_from_pairs(ctx.raw(), pairs.empty() ? nullptr : &pairs[0].a, pairs.size(), log_n,
                                             out.perm.empty() ? nullptr : out.perm.data(), &out.classes), ctx.raw());
        return out;
    }
};

class CompiledCircuit {
   public:
    CompiledCircuit(const kzg::Srs& srs, uint32_t log_n, const std::vector<Fr> (&selector_evals)[5],
                    const std::vector<Fr> (&sigma_evals)[3], const Fr (&cosets)[3])
        : srs_(srs), log_n_(log_n), n_((size_t)1 << log_n) {
        for (int i = 0; i < 3; ++i) cosets_[i] = cosets[i];
        typlonk_ctx* c = srs.ctx().raw();
        typlonk_buf* polys[8];
        for (int k = 0; k < 8; ++k) {
            const std::vector<Fr>& ev = k < 5 ? selector_evals[k] : sigma_evals[k - 5];
            if (ev.size() != n_) throw std::runtime_error("circuit table must hold n evaluations");
            polys[k] = upload(ev);
        }
        {   // interpolate(), builder.rs:84-88 and proof.rs:334-338: the eight columns as ONE batched inverse transform
            void* ptrs[8];
            for (int k = 0; k < 8; ++k) ptrs[k] = typlonk_buf_devptr(polys[k]);
            const int rc = typlonk_ntt_fr_batch_devptr(c, ptrs, 8, log_n, 1, nullptr);
            if (rc < 0) {
                for (typlonk_buf* b : polys) typlonk_buf_free(c, b);
                check(rc, c);
            }
        }
        // the commitments of the fixed polynomials: [q_l] .. [q_c] (builder.rs:86) and [sigma_0..2], which the
        // reference's verifier recomputes with three MSMs on EVERY verify() (permutation/src/lib.rs:178-194 via
        // proof.rs:459) -- here once per circuit, one batch of eight MSMs straight from the interpolated buffers
        {
            const void* ptrs[8];
            size_t lens[8];
            uint64_t xy[8][12];
            uint8_t inf[8];
            for (int k = 0; k < 8; ++k) {
                ptrs[k] = typlonk_buf_devptr(polys[k]);
                lens[k] = n_;
            }
            // (an SRS shard: the ranks' partial sums folded by the library, a collective -- the same points on every rank)
            const int rc = srs.sharded() ? typlonk_msm_g1_sharded_batch_devptr(c, srs.id(), ptrs, lens, 8, &xy[0][0], inf)
                                         : typlonk_msm_g1_batch_devptr(c, srs.id(), ptrs, lens, 8, &xy[0][0], inf);
            if (rc < 0) {
                for (typlonk_buf* b : polys) typlonk_buf_free(c, b);
                check(rc, c);
            }
            for (int k = 0; k < 8; ++k) {
                kzg::G1Point g;
                std::memcpy(g.xy, xy[k], 96);
                g.infinity = inf[k] != 0;
                (k < 5 ? fixed_commitments[k] : sigma_commitments[k - 5]) = kzg::KzgCommitment{g};
            }
        }
        for (int i = 0; i < 3; ++i) {  // the verifier evaluates the sigma polynomials at zeta (sigma_evals)
            std::vector<Fr> co(n_);
            const int rc = typlonk_buf_download(c, polys[5 + i], 0, co[0].limbs(), n_);
            if (rc < 0) {
                for (typlonk_buf* b : polys) typlonk_buf_free(c, b);
                check(rc, c);
            }
            sigma_polys_[i] = poly::DensePolynomial::from_coefficients_vec(std::move(co));
        }
        const typlonk_buf* sel[5] = {polys[0], polys[1], polys[2], polys[3], polys[4]};
        const typlonk_buf* sig[3] = {polys[5], polys[6], polys[7]};
        const int rc = typlonk_circuit_load(c, sel, sig, log_n, &circuit_);
        for (typlonk_buf* b : polys) typlonk_buf_free(c, b);
        check(rc, c);
    }
    // The same from what a front end holds before Permutation::compile (permutation/src/lib.rs:101-128): the selector
    // evaluations and the permutation itself, `perm` = 3n successors over the flat cells col * n + row (empty: no copy
    // constraints).  typlonk_circuit_compile_host makes the sigma columns, interpolates all eight on the device and keeps
    // the permutation with the circuit (check_witness never has to recover it); a perm that is no permutation of the cells
    // throws with the number of defects and the lowest defective cell.  The eight commitments come from the library's cache
    // (typlonk_circuit_commitments: on an SRS shard a collective, like the other constructor's MSMs).  Nothing of
    // Permutation::compile runs on the host here; the first verify() of this mirror pays for it once (ensure_sigma_polys).
    CompiledCircuit(const kzg::Srs& srs, uint32_t log_n, const std::vector<Fr> (&selector_evals)[5],
                    const std::vector<uint32_t>& perm, const Fr (&cosets)[3])
        : srs_(srs), log_n_(log_n), n_((size_t)1 << log_n) {
        for (int i = 0; i < 3; ++i) cosets_[i] = cosets[i];
        typlonk_ctx* c = srs.ctx().raw();
        const uint64_t* sel[5];
        for (int k = 0; k < 5; ++k) {
            if (selector_evals[k].size() != n_) throw std::runtime_error("circuit table must hold n evaluations");
            sel[k] = selector_evals[k][0].limbs();
        }
        if (!perm.empty() && perm.size() != 3 * n_) throw std::runtime_error("perm must hold 3n successors");
        uint64_t ks[3][4];
        for (int i = 0; i < 3; ++i) std::memcpy(ks[i], cosets_[i].limbs(), 32);
        check(typlonk_circuit_compile_host(c, sel, n_, perm.empty() ? nullptr : perm.data(), ks, log_n, &circuit_, nullptr), c);
        fetch_commitments();
    }
    // The same from what a front end holds before PermutationBuilder::build (permutation/src/lib.rs:48-93): the copy
    // constraints themselves, pairs of flat cells that must carry one value.  typlonk_circuit_compile_pairs_host makes the
    // canonical permutation of their classes on the device (every class ascending; CellPermutation::from_pairs returns the
    // same map) and compiles from it; a pair outside the table throws with the lowest bad pair named.  classes() is the
    // number of classes among the 3n cells.
    CompiledCircuit(const kzg::Srs& srs, uint32_t log_n, const std::vector<Fr> (&selector_evals)[5],
                    const std::vector<CellPair>& pairs, const Fr (&cosets)[3])
        : srs_(srs), log_n_(log_n), n_((size_t)1 << log_n) {
        for (int i = 0; i < 3; ++i) cosets_[i] = cosets[i];
        typlonk_ctx* c = srs.ctx().raw();
        const uint64_t* sel[5];
        for (int k = 0; k < 5; ++k) {
            if (selector_evals[k].size() != n_) throw std::runtime_error("circuit table must hold n evaluations");
            sel[k] = selector_evals[k][0].limbs();
        }
        uint64_t ks[3][4];
        for (int i = 0; i < 3; ++i) std::memcpy(ks[i], cosets_[i].limbs(), 32);
        check(typlonk_circuit_compile_pairs_host(c, sel, n_, pairs.empty() ? nullptr : &pairs[0].a, pairs.size(), ks, log_n, &circuit_,
                                                 &classes_), c);
        fetch_commitments();
    }
    CompiledCircuit(const CompiledCircuit&) = delete;
    ~CompiledCircuit() {
        if (circuit_) typlonk_circuit_free(srs_.ctx().raw(), circuit_);
    }
    size_t rows() const { return n_; }
    uint64_t classes() const { return classes_; }   // of the constructor from pairs (0 for the others)
    kzg::KzgCommitment fixed_commitments[5];  // [q_l], [q_r], [q_o], [q_m], [q_c]  (GateConstrains::fixed_commitments)
    kzg::KzgCommitment sigma_commitments[3];  // what CompiledPermutation::sigma_commitments returns

    // CompiledCircuit::prove (proof.rs:26-57) from the point where the witness columns exist: `advice` = the three
    // columns padded to n rows with their blinding rows (:43-49), `public_inputs` = the padded public-input column or
    // empty for the all-zero one (:52-53).  A witness that does not satisfy the circuit throws (the reference panics).
    Proof prove(const std::vector<Fr> (&advice)[3], const std::vector<Fr>& public_inputs = {}) const {
        typlonk_ctx* c = srs_.ctx().raw();
        typlonk_proof raw;
        // the columns go over as they are, in host memory (typlonk_prove_host: each is uploaded right before its
        // interpolation and commitment are queued, beside the previous column's kernels) -- as the Rust layer's Backend::prove
        for (int i = 0; i < 3; ++i)
            if (advice[i].size() != n_) throw std::runtime_error("witness column must hold n values");
        if (!public_inputs.empty() && public_inputs.size() != n_) throw std::runtime_error("public-input column must hold n values");
        uint64_t ks[3][4];
        for (int i = 0; i < 3; ++i) std::memcpy(ks[i], cosets_[i].limbs(), 32);
        const uint64_t* wc[3] = {advice[0][0].limbs(), advice[1][0].limbs(), advice[2][0].limbs()};
        check(typlonk_prove_host(c, srs_.id(), circuit_, wc, public_inputs.empty() ? nullptr : public_inputs[0].limbs(), ks, &raw), c);
        return from_raw(raw);
    }

    // prove() for many witnesses in one call (typlonk_prove_batch_host, batched across proofs in waves): advice[k] and
    // public_inputs[k] (empty = the all-zero column; the vector itself may be empty) as for prove().  proofs[k] equals
    // prove(advice[k], public_inputs[k]); status[k] is TYPLONK_OK or TYPLONK_ERR_UNSATISFIED (a witness that does not
    // satisfy the circuit: its proof is filled all the same and will not verify) -- no throw for those.
    std::vector<Proof> prove_batch(const std::vector<std::array<std::vector<Fr>, 3>>& advice,
                                   const std::vector<std::vector<Fr>>& public_inputs, std::vector<int>* status) const {
        typlonk_ctx* c = srs_.ctx().raw();
        const size_t count = advice.size();
        if (!public_inputs.empty() && public_inputs.size() != count) throw std::runtime_error("one public-input column per witness");
        std::vector<const uint64_t*> wc(3 * count), pc(count, nullptr);
        for (size_t k = 0; k < count; ++k) {
            for (int i = 0; i < 3; ++i) {
                if (advice[k][i].size() != n_) throw std::runtime_error("witness column must hold n values");
                wc[3 * k + i] = advice[k][i][0].limbs();
            }
            if (!public_inputs.empty() && !public_inputs[k].empty()) {
                if (public_inputs[k].size() != n_) throw std::runtime_error("public-input column must hold n values");
                pc[k] = public_inputs[k][0].limbs();
            }
        }
        uint64_t ks[3][4];
        for (int i = 0; i < 3; ++i) std::memcpy(ks[i], cosets_[i].limbs(), 32);
        std::vector<typlonk_proof> raw(count);
        std::vector<int> st(count, TYPLONK_OK);
        check(typlonk_prove_batch_host(c, srs_.id(), circuit_, wc.data(), pc.data(), count, ks, raw.data(), st.data()), c);
        std::vector<Proof> out;
        out.reserve(count);
        for (const typlonk_proof& r : raw) out.push_back(from_raw(r));
        if (status) *status = st;
        return out;
    }

    // typlonk_proof (the C ABI's form) -> Proof
    static Proof from_raw(const typlonk_proof& raw) {
        Proof p;
        auto pt = [](const uint64_t xy[12], uint8_t inf) {
            kzg::G1Point g;
            std::memcpy(g.xy, xy, 96);
            g.infinity = inf != 0;
            return g;
        };
        auto fr = [](const uint64_t l[4]) {
            Fr f;
            std::memcpy(f.v.v, l, 32);
            return f;
        };
        p.a_commit = {pt(raw.commit_xy[0], raw.commit_inf[0])};
        p.b_commit = {pt(raw.commit_xy[1], raw.commit_inf[1])};
        p.c_commit = {pt(raw.commit_xy[2], raw.commit_inf[2])};
        const typlonk_proof_tail& t = raw.tail;
        p.a = {pt(t.w_xy[0], t.w_inf[0]), fr(t.evals[0])};
        p.b = {pt(t.w_xy[1], t.w_inf[1]), fr(t.evals[1])};
        p.c = {pt(t.w_xy[2], t.w_inf[2]), fr(t.evals[2])};
        p.permutation.commitment = {pt(raw.z_xy, raw.z_inf)};
        p.permutation.z = {pt(t.w_xy[3], t.w_inf[3]), fr(t.evals[3])};
        p.permutation.zw = {pt(t.w_xy[4], t.w_inf[4]), fr(t.evals[4])};
        p.evaluation_point = fr(raw.zeta);
        for (int i = 0; i < 3; ++i) p.t[i] = {pt(t.t_xy[i], t.t_inf[i])};
        p.r = {pt(t.w_xy[5], t.w_inf[5]), fr(t.evals[5])};
        p.beta = fr(raw.beta);
        p.gamma = fr(raw.gamma);
        p.alpha = fr(raw.alpha);
        return p;
    }

    // plonk::proof::verify (proof.rs:195-235): recompute the challenges from the commitments (verify_challenges,
    // :236-246), check the five openings (verify_openings, :247-272), rebuild the linearisation commitment (:441-503)
    // and check its opening, which must evaluate to zero.  `public_inputs` as for prove().
    //
    // Public inputs: the reference's prover ADDS PI(zeta) to r (proof.rs:401-402) and its verifier adds public_eval to the
    // constant it SUBTRACTS (:497-502), so with PI(zeta) != 0 the reference rejects its own honest proofs (its tests only
    // use vec![0]).  The default follows the reference; PublicInputSign::AsProver is the consistent verifier.
    enum class PublicInputSign { AsReference, AsProver };
    bool verify(const Proof& proof, const std::vector<Fr>& public_inputs = {},
                PublicInputSign pi_sign = PublicInputSign::AsReference) const {
        const Context& ctx = srs_.ctx();
        const kzg::KzgScheme scheme(srs_);
        // verify_challenges
        uint64_t xy[4][12];
        uint8_t inf[4];
        const kzg::G1Point* cm[4] = {&proof.a_commit.p, &proof.b_commit.p, &proof.c_commit.p, &proof.permutation.commitment.p};
        for (int i = 0; i < 4; ++i) {
            std::memcpy(xy[i], cm[i]->xy, 96);
            inf[i] = cm[i]->infinity;
        }
        uint64_t ch[8];
        Fr beta, gamma, alpha, point;
        check(typlonk_transcript_challenges(&xy[0][0], inf, 3, 2, ch));
        std::memcpy(beta.v.v, ch, 32);
        std::memcpy(gamma.v.v, ch + 4, 32);
        check(typlonk_transcript_challenges(&xy[0][0], inf, 4, 2, ch));
        std::memcpy(alpha.v.v, ch, 32);
        std::memcpy(point.v.v, ch + 4, 32);
        if (proof.evaluation_point != point) return false;  // :212-214
        const poly::Radix2EvaluationDomain domain(ctx, n_);
        Fr public_eval = Fr::zero();
        if (!public_inputs.empty()) public_eval = poly::interpolate(public_inputs, domain).evaluate(point);
        // verify_openings
        const Fr w = domain.element(1);
        if (!scheme.verify(proof.a_commit, proof.a, point) || !scheme.verify(proof.b_commit, proof.b, point) ||
            !scheme.verify(proof.c_commit, proof.c, point))
            return false;
        if (!scheme.verify(proof.permutation.commitment, proof.permutation.z, point) ||
            !scheme.verify(proof.permutation.commitment, proof.permutation.zw, point * w))
            return false;
        // linearisation_commitment
        const Fr a = proof.a.eval(), b = proof.b.eval(), c = proof.c.eval();
        const Fr zw_eval = proof.permutation.zw.eval();
        const Fr advice[3] = {a, b, c};
        Fr sigma_evals[3];
        ensure_sigma_polys();
        for (int i = 0; i < 3; ++i) sigma_evals[i] = sigma_polys_[i].evaluate(point);  // permutation/src/lib.rs:165-176
        Fr l2 = Fr::one();
        for (int i = 0; i < 3; ++i) l2 *= advice[i] + beta * cosets_[i] * point + gamma;
        const Fr zn = point.pow(n_);
        const Fr vanish = zn - Fr::one();
        Fr l0 = Fr::one();  // L0(zeta) = (zeta^n - 1) / (n (zeta - 1)); 1 at zeta = 1  (utils.rs:150-159)
        if (point != Fr::one()) l0 = vanish * (Fr((int64_t)n_) * (point - Fr::one())).inverse();
        Fr l3 = Fr::one();
        for (int i = 0; i < 2; ++i) l3 *= advice[i] + beta * sigma_evals[i] + gamma;
        const Fr constant = alpha * (l3 * (c + gamma) * zw_eval) + l0 * alpha * alpha +
                            (pi_sign == PublicInputSign::AsReference ? public_eval : -public_eval);
        const std::vector<kzg::G1Point> bases = {fixed_commitments[0].p, fixed_commitments[1].p, fixed_commitments[2].p,
                                                 fixed_commitments[3].p, fixed_commitments[4].p, proof.permutation.commitment.p,
                                                 sigma_commitments[2].p, srs_.g1_generator(), proof.t[0].p, proof.t[1].p, proof.t[2].p};
        const std::vector<Fr> ks = {a, b, -c, a * b, Fr::one(), l2 * alpha + l0 * alpha * alpha,
                                    -(l3 * alpha * beta * zw_eval), -constant, -vanish, -(vanish * zn), -(vanish * zn * zn)};
        const kzg::KzgCommitment r{kzg::g1_lincomb(ctx, bases, ks)};
        return scheme.verify(r, proof.r, point) && proof.r.eval().is_zero();
    }

    // The same decision for a batch through the C ABI (typlonk_verify): sigma and long public-input columns evaluated on the
    // device, the six KZG checks of every proof folded into one pairing product, bisected when it fails.  result[k] is
    // verify(proofs[k], public_inputs[k], pi_sign) -- the G2 generator is the fixed one (an Srs whose g2 was replaced with
    // set_g2 is not supported).  public_inputs: empty, or one column per proof (each empty = all zero, at most n values).
    std::vector<bool> verify_batch(const std::vector<Proof>& proofs, const std::vector<std::vector<Fr>>& public_inputs = {},
                                   PublicInputSign pi_sign = PublicInputSign::AsReference) const {
        typlonk_ctx* c = srs_.ctx().raw();
        if (!public_inputs.empty() && public_inputs.size() != proofs.size())
            throw std::runtime_error("one public-input column per proof");
        std::vector<typlonk_proof> raw(proofs.size());
        auto pt = [](const kzg::G1Point& g, uint64_t xy[12], uint8_t* inf) {
            std::memcpy(xy, g.xy, 96);
            *inf = g.infinity ? 1 : 0;
        };
        for (size_t k = 0; k < proofs.size(); ++k) {
            const Proof& p = proofs[k];
            typlonk_proof& r = raw[k];
            std::memset(&r, 0, sizeof(r));
            pt(p.a_commit.p, r.commit_xy[0], &r.commit_inf[0]);
            pt(p.b_commit.p, r.commit_xy[1], &r.commit_inf[1]);
            pt(p.c_commit.p, r.commit_xy[2], &r.commit_inf[2]);
            pt(p.permutation.commitment.p, r.z_xy, &r.z_inf);
            for (int i = 0; i < 3; ++i) pt(p.t[i].p, r.tail.t_xy[i], &r.tail.t_inf[i]);
            const kzg::KzgOpening* op[6] = {&p.a, &p.b, &p.c, &p.permutation.z, &p.permutation.zw, &p.r};
            for (int i = 0; i < 6; ++i) {
                pt(op[i]->p, r.tail.w_xy[i], &r.tail.w_inf[i]);
                std::memcpy(r.tail.evals[i], op[i]->y.limbs(), 32);
            }
            std::memcpy(r.zeta, p.evaluation_point.limbs(), 32);
        }
        uint64_t g2s[24];
        g2s_limbs(g2s);
        uint64_t ks[3][4];
        for (int i = 0; i < 3; ++i) std::memcpy(ks[i], cosets_[i].limbs(), 32);
        std::vector<const uint64_t*> pis(proofs.size(), nullptr);
        std::vector<size_t> lens(proofs.size(), 0);
        for (size_t k = 0; k < public_inputs.size(); ++k)
            if (!public_inputs[k].empty()) {
                pis[k] = public_inputs[k][0].limbs();
                lens[k] = public_inputs[k].size();
            }
        std::vector<uint8_t> ok(proofs.size() + 1, 0);
        check(typlonk_verify(c, srs_.id(), circuit_, g2s, ks, raw.data(), raw.size(), pis.data(), lens.data(),
                             pi_sign == PublicInputSign::AsProver ? TYPLONK_VERIFY_PI_AS_PROVER : 0u, ok.data()),
              c);
        return std::vector<bool>(ok.begin(), ok.begin() + proofs.size());
    }

    // ---- the compact proof shape (include/typlonk.h): batched openings, a transcript that binds the statement ----
    // The verifying key: all typlonk_verify_compact needs instead of this object (log n, the cosets, the eight commitments,
    // SRS point 0 and the SRS's [s]G2).  On a sharded SRS: a collective (one fold of 9 records), the whole-SRS key on every rank.
    typlonk_vk verifying_key() const {
        typlonk_ctx* c = srs_.ctx().raw();
        uint64_t g2s[24], ks[3][4];
        g2s_limbs(g2s);
        for (int i = 0; i < 3; ++i) std::memcpy(ks[i], cosets_[i].limbs(), 32);
        typlonk_vk vk;
        check(typlonk_circuit_vk(c, srs_.id(), circuit_, ks, g2s, &vk), c);
        return vk;
    }
    // A compact proof (typlonk_prove_compact_host): `advice` as for prove(); `public_inputs` = the statement's public values
    // themselves (at most n, not padded: their number is part of the statement).  A witness that does not satisfy the circuit
    // throws, as prove() does.  On a sharded SRS (kzg::Srs::from_secret_shard, Context::comm_init) the call is a collective:
    // four folds of 12, 1, 3 and 2 records inside the library, the same proof on every rank as from one GPU with the whole SRS;
    // a rank whose call fails throws its own error, its peers TYPLONK_ERR_COMM naming it.
    typlonk_proof_compact prove_compact(const std::vector<Fr> (&advice)[3], const std::vector<Fr>& public_inputs = {}) const {
        typlonk_ctx* c = srs_.ctx().raw();
        for (int i = 0; i < 3; ++i)
            if (advice[i].size() != n_) throw std::runtime_error("witness column must hold n values");
        uint64_t ks[3][4];
        for (int i = 0; i < 3; ++i) std::memcpy(ks[i], cosets_[i].limbs(), 32);
        const uint64_t* wc[3] = {advice[0][0].limbs(), advice[1][0].limbs(), advice[2][0].limbs()};
        typlonk_proof_compact out;
        check(typlonk_prove_compact_host(c, srs_.id(), circuit_, wc, n_, public_inputs.empty() ? nullptr : public_inputs[0].limbs(),
                                         public_inputs.size(), ks, &out),
              c);
        return out;
    }
    // prove_compact() for many witnesses in one call (typlonk_prove_batch_compact_host, batched across proofs in waves):
    // advice[k] as for prove_batch(), public_inputs[k] = proof k's public values (the vector or an entry may be empty).
    // proofs[k] equals prove_compact(advice[k], public_inputs[k]); status[k] is TYPLONK_OK or TYPLONK_ERR_UNSATISFIED (its
    // proof is filled all the same and will not verify) -- no throw for those.
    std::vector<typlonk_proof_compact> prove_batch_compact(const std::vector<std::array<std::vector<Fr>, 3>>& advice,
                                                           const std::vector<std::vector<Fr>>& public_inputs,
                                                           std::vector<int>* status) const {
        typlonk_ctx* c = srs_.ctx().raw();
        const size_t count = advice.size();
        if (!public_inputs.empty() && public_inputs.size() != count) throw std::runtime_error("one public-input list per witness");
        std::vector<const uint64_t*> wc(3 * count), pc(count, nullptr);
        std::vector<size_t> lens(count, 0);
        for (size_t k = 0; k < count; ++k) {
            for (int i = 0; i < 3; ++i) {
                if (advice[k][i].size() != n_) throw std::runtime_error("witness column must hold n values");
                wc[3 * k + i] = advice[k][i][0].limbs();
            }
            if (!public_inputs.empty() && !public_inputs[k].empty()) {
                pc[k] = public_inputs[k][0].limbs();
                lens[k] = public_inputs[k].size();
            }
        }
        uint64_t ks[3][4];
        for (int i = 0; i < 3; ++i) std::memcpy(ks[i], cosets_[i].limbs(), 32);
        std::vector<typlonk_proof_compact> out(count);
        std::vector<int> st(count, TYPLONK_OK);
        check(typlonk_prove_batch_compact_host(c, srs_.id(), circuit_, wc.data(), n_, pc.data(), lens.data(), count, ks, out.data(),
                                               st.data()),
              c);
        if (status) *status = st;
        return out;
    }
    // Which gate rows and which copy constraints does a witness fail (typlonk_witness_check_host)?  Exact, no SRS work, a
    // fraction of a proof's cost: what to call before prove() on a witness of unknown quality -- the reference only panics in
    // vanishes() (proof.rs:504-507).  gate_rows / copy_cells hold the lowest failing rows and cells (x, perm[x]; flat cells
    // col * n + row), at most `cap` each; the counts are totals.  Throws for a malformed circuit (sigma is no permutation).
    struct WitnessReport {
        uint64_t gate_failures = 0, copy_failures = 0;
        std::vector<uint32_t> gate_rows;
        std::vector<std::array<uint32_t, 2>> copy_cells;
        bool satisfied() const { return gate_failures == 0 && copy_failures == 0; }
    };
    WitnessReport check_witness(const std::vector<Fr> (&advice)[3], const std::vector<Fr>& public_inputs = {}, uint32_t cap = 16) const {
        typlonk_ctx* c = srs_.ctx().raw();
        for (int i = 0; i < 3; ++i)
            if (advice[i].size() != n_) throw std::runtime_error("witness column must hold n values");
        uint64_t ks[3][4];
        for (int i = 0; i < 3; ++i) std::memcpy(ks[i], cosets_[i].limbs(), 32);
        const uint64_t* wc[3] = {advice[0][0].limbs(), advice[1][0].limbs(), advice[2][0].limbs()};
        const uint64_t* pc[1] = {public_inputs.empty() ? nullptr : public_inputs[0].limbs()};
        const size_t lens[1] = {public_inputs.size()};
        typlonk_witness_report rep{};
        std::vector<uint32_t> gate(cap), copy(2 * (size_t)cap);
        check(typlonk_witness_check_host(c, circuit_, wc, n_, pc, lens, 1, ks, cap, &rep, gate.data(), copy.data()), c);
        WitnessReport out;
        out.gate_failures = rep.gate_failures;
        out.copy_failures = rep.copy_failures;
        out.gate_rows.assign(gate.begin(), gate.begin() + rep.gate_listed);
        for (uint32_t k = 0; k < rep.copy_listed; ++k) out.copy_cells.push_back({copy[2 * k], copy[2 * k + 1]});
        return out;
    }
    // The three wire columns of a witness from the circuit's inputs, computed on the device (typlonk_witness_solve; the
    // reference's C::run filling the advice columns, builder.rs:381-396): `cells` are the flat indices (col * n + row) of the
    // assigned cells -- the inputs and, if wanted, the three blinding rows -- and `values` their values; every other free class
    // reads 0 and every driven row's c cell is computed.  The columns come back to the host here, for check_witness / prove();
    // a caller that keeps them on the device calls the C ABI directly.  Throws for a cell in a driven class, two cells of one
    // class, or a circuit whose rows depend on each other in a cycle.
    void solve_witness(const std::vector<uint32_t>& cells, const std::vector<Fr>& values, std::vector<Fr> (&advice)[3],
                       const std::vector<Fr>& public_inputs = {}) const {
        typlonk_ctx* c = srs_.ctx().raw();
        if (cells.size() != values.size()) throw std::runtime_error("one value per assigned cell");
        uint64_t ks[3][4];
        for (int i = 0; i < 3; ++i) std::memcpy(ks[i], cosets_[i].limbs(), 32);
        typlonk_buf* out[3] = {nullptr, nullptr, nullptr};
        typlonk_buf* pib = nullptr;
        auto release = [&] {
            for (typlonk_buf* b : out)
                if (b) typlonk_buf_free(c, b);
            if (pib) typlonk_buf_free(c, pib);
        };
        int rc = 0;
        for (int i = 0; i < 3 && rc >= 0; ++i) rc = typlonk_buf_alloc(c, n_, &out[i]);
        if (rc >= 0 && !public_inputs.empty()) {
            rc = typlonk_buf_alloc(c, public_inputs.size(), &pib);
            if (rc >= 0) rc = typlonk_buf_upload(c, pib, 0, public_inputs[0].limbs(), public_inputs.size());
        }
        const typlonk_buf* pis[1] = {pib};
        const size_t lens[1] = {public_inputs.size()};
        if (rc >= 0)
            rc = typlonk_witness_solve(c, circuit_, ks, cells.empty() ? nullptr : cells.data(), cells.size(),
                                       values.empty() ? nullptr : values[0].limbs(), pis, lens, 1, out);
        for (int i = 0; i < 3 && rc >= 0; ++i) {
            advice[i].assign(n_, Fr());
            rc = typlonk_buf_download(c, out[i], 0, advice[i][0].limbs(), n_);
        }
        release();
        check(rc, c);
    }
    // The advice solve_witness computes itself (typlonk_circuit_set_hints): each hint fills the free class of cell `dst` with
    // 1 / x (TYPLONK_HINT_INV0; 0 for x = 0) or with bits [shift, shift + width) of x (TYPLONK_HINT_BITS), x being the value the
    // solve writes to cell `src`.  Replaces the circuit's whole set; an empty vector removes it.  Throws for a refused set (a hint
    // into a driven class, two into one class, a dependency cycle ...), which leaves the installed one in force.  Cells of a
    // hinted class are no longer accepted by solve_witness.
    void set_hints(const std::vector<typlonk_hint>& hints) const {
        typlonk_ctx* c = srs_.ctx().raw();
        uint64_t ks[3][4];
        for (int i = 0; i < 3; ++i) std::memcpy(ks[i], cosets_[i].limbs(), 32);
        check(typlonk_circuit_set_hints(c, circuit_, ks, hints.empty() ? nullptr : hints.data(), hints.size()), c);
    }
    // what a solve of this circuit costs: driven rows, free classes, levels and kernel launches (typlonk_witness_solve_plan)
    typlonk_solve_info solve_info() const {
        typlonk_ctx* c = srs_.ctx().raw();
        uint64_t ks[3][4];
        for (int i = 0; i < 3; ++i) std::memcpy(ks[i], cosets_[i].limbs(), 32);
        typlonk_solve_info info{};
        check(typlonk_witness_solve_plan(c, circuit_, ks, &info), c);
        return info;
    }

   private:
    void g2s_limbs(uint64_t g2s[24]) const {
        const pairing::G2Affine& q = srs_.g2s();
        std::memcpy(g2s, q.x.a.v, 48);
        std::memcpy(g2s + 6, q.x.b.v, 48);
        std::memcpy(g2s + 12, q.y.a.v, 48);
        std::memcpy(g2s + 18, q.y.b.v, 48);
    }
    typlonk_buf* upload(const std::vector<Fr>& v) const {
        typlonk_ctx* c = srs_.ctx().raw();
        typlonk_buf* b = nullptr;
        check(typlonk_buf_alloc(c, v.size(), &b), c);
        const int rc = typlonk_buf_upload(c, b, 0, v[0].limbs(), v.size());
        if (rc < 0) {
            typlonk_buf_free(c, b);
            check(rc, c);
        }
        return b;
    }
    // the eight commitments of a compiled circuit from the library's cache; the sigma polynomials stay to be made
    void fetch_commitments() {
        typlonk_ctx* c = srs_.ctx().raw();
        uint64_t xy[8][12];
        uint8_t inf[8];
        const int rc = typlonk_circuit_commitments(c, srs_.id(), circuit_, xy, inf);
        if (rc < 0) {
            typlonk_circuit_free(c, circuit_);
            circuit_ = 0;
            check(rc, c);
        }
        sigma_lazy_ = true;  // (the sigma polynomials are this mirror's verify()'s alone: ensure_sigma_polys makes them there)
        for (int k = 0; k < 8; ++k) {
            kzg::G1Point g;
            std::memcpy(g.xy, xy[k], 96);
            g.infinity = inf[k] != 0;
            (k < 5 ? fixed_commitments[k] : sigma_commitments[k - 5]) = kzg::KzgCommitment{g};
        }
    }
    // verify() evaluates the sigma polynomials at zeta.  A circuit compiled from a permutation has none on the host until the
    // first verify(): the permutation comes back from the library's cache (typlonk_circuit_permutation, no recovery under the
    // circuit's own cosets), then Permutation::compile on the host (3n products) and one batch of three interpolations.
    void ensure_sigma_polys() const {
        if (!sigma_lazy_) return;
        typlonk_ctx* c = srs_.ctx().raw();
        uint64_t ks[3][4];
        for (int i = 0; i < 3; ++i) std::memcpy(ks[i], cosets_[i].limbs(), 32);
        std::vector<uint32_t> perm(3 * n_);
        uint64_t defects = 0;
        check(typlonk_circuit_permutation(c, circuit_, ks, perm.data(), &defects), c);
        const poly::Radix2EvaluationDomain domain(srs_.ctx(), n_);
        std::vector<Fr> roots(n_);
        Fr x = Fr::one();
        for (size_t j = 0; j < n_; ++j, x = x * domain.group_gen) roots[j] = x;
        std::vector<std::vector<Fr>> sigma(3, std::vector<Fr>(n_));
        for (size_t cell = 0; cell < 3 * n_; ++cell)
            sigma[cell >> log_n_][cell & (n_ - 1)] = cosets_[perm[cell] >> log_n_] * roots[perm[cell] & (n_ - 1)];
        const auto polys = poly::interpolate_batch(srs_.ctx(), sigma, domain);
        for (int i = 0; i < 3; ++i) sigma_polys_[i] = polys[i];
        sigma_lazy_ = false;
    }
    const kzg::Srs& srs_;
    uint32_t log_n_;
    size_t n_;
    Fr cosets_[3];
    uint32_t circuit_ = 0;
    uint64_t classes_ = 0;
    mutable poly::DensePolynomial sigma_polys_[3];
    mutable bool sigma_lazy_ = false;
};

// typlonk_verify_compact: compact proofs against a verifying key, on any context -- it needs no SRS and no loaded circuit.
// public_inputs: empty, or one list of public values per proof (each empty = none).  result[k] = proof k is accepted.
inline std::vector<bool> verify_compact(const Context& ctx, const typlonk_vk& vk, const std::vector<typlonk_proof_compact>& proofs,
                                        const std::vector<std::vector<Fr>>& public_inputs = {}) {
    if (!public_inputs.empty() && public_inputs.size() != proofs.size()) throw std::runtime_error("one public-input list per proof");
    std::vector<const uint64_t*> pis(proofs.size(), nullptr);
    std::vector<size_t> lens(proofs.size(), 0);
    for (size_t k = 0; k < public_inputs.size(); ++k)
        if (!public_inputs[k].empty()) {
            pis[k] = public_inputs[k][0].limbs();
            lens[k] = public_inputs[k].size();
        }
    std::vector<uint8_t> ok(proofs.size() + 1, 0);
    check(typlonk_verify_compact(ctx.raw(), &vk, proofs.data(), proofs.size(), pis.data(), lens.data(), ok.data()), ctx.raw());
    return std::vector<bool>(ok.begin(), ok.begin() + proofs.size());
}

// ---- the wire format (include/typlonk.h): compact proofs and verifying keys as bytes, points compressed ----
// Proof <-> its 656 bytes.  to_bytes throws for a field that is not canonical or a point off the curve.
inline std::vector<uint8_t> proof_to_bytes(const typlonk_proof_compact& proof) {
    std::vector<uint8_t> out(TYPLONK_PROOF_COMPACT_BYTES);
    check(typlonk_proof_compact_to_bytes(&proof, out.data()));
    return out;
}
// `bytes` = count * 656.  Every point is decoded -- on the curve, in the subgroup -- by one kernel launch on `ctx` (nullptr: on the
// host); status[k] != 0 names the class and field of the first bad field of proof k (TYPLONK_DECODE_CLASS / _FIELD), and that
// proof is all identities.  The challenge fields are zero: the verifier recomputes them.
inline std::vector<typlonk_proof_compact> proofs_from_bytes(const Context* ctx, const std::vector<uint8_t>& bytes,
                                                            std::vector<uint32_t>* status, uint32_t flags = 0) {
    if (bytes.size() % TYPLONK_PROOF_COMPACT_BYTES) throw std::runtime_error("proofs are 656 bytes each");
    const size_t count = bytes.size() / TYPLONK_PROOF_COMPACT_BYTES;
    std::vector<typlonk_proof_compact> out(count);
    std::vector<uint32_t> st(count, 0);
    typlonk_ctx* c = ctx ? ctx->raw() : nullptr;
    check(typlonk_proof_compact_from_bytes(c, bytes.data(), count, flags, out.data(), st.data()), c);
    if (status) *status = st;
    return out;
}
inline std::vector<uint8_t> vk_to_bytes(const typlonk_vk& vk) {
    std::vector<uint8_t> out(TYPLONK_VK_WIRE_BYTES);
    check(typlonk_vk_to_bytes(&vk, out.data()));
    return out;
}
// throws for a key that is refused (a bad field, log_n outside 1..24)
inline typlonk_vk vk_from_bytes(const std::vector<uint8_t>& bytes, uint32_t flags = 0) {
    if (bytes.size() != TYPLONK_VK_WIRE_BYTES) throw std::runtime_error("a verifying key is 628 bytes");
    typlonk_vk vk;
    uint32_t st = 0;
    const int rc = typlonk_vk_from_bytes(bytes.data(), flags, &vk, &st);
    if (rc < 0)
        throw std::runtime_error(std::string(typlonk_strerror(rc)) + ": key field " + std::to_string(TYPLONK_DECODE_FIELD(st)) +
                                 ", class " + std::to_string(TYPLONK_DECODE_CLASS(st)));
    return vk;
}
// verify_compact over the wire form: a proof that does not decode is false and never reaches the verifier
inline std::vector<bool> verify_compact_bytes(const Context& ctx, const typlonk_vk& vk, const std::vector<uint8_t>& bytes,
                                              const std::vector<std::vector<Fr>>& public_inputs = {}, uint32_t flags = 0) {
    if (bytes.size() % TYPLONK_PROOF_COMPACT_BYTES) throw std::runtime_error("proofs are 656 bytes each");
    const size_t count = bytes.size() / TYPLONK_PROOF_COMPACT_BYTES;
    if (!public_inputs.empty() && public_inputs.size() != count) throw std::runtime_error("one public-input list per proof");
    std::vector<const uint64_t*> pis(count, nullptr);
    std::vector<size_t> lens(count, 0);
    for (size_t k = 0; k < public_inputs.size(); ++k)
        if (!public_inputs[k].empty()) {
            pis[k] = public_inputs[k][0].limbs();
            lens[k] = public_inputs[k].size();
        }
    std::vector<uint8_t> ok(count + 1, 0);
    check(typlonk_verify_compact_bytes(ctx.raw(), &vk, bytes.data(), count, pis.data(), lens.data(), flags, ok.data()), ctx.raw());
    return std::vector<bool>(ok.begin(), ok.begin() + count);
}

}  // namespace plonk
}  // namespace typlonk
