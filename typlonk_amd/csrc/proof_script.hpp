// The Fiat-Shamir script of each proof shape, host side: which values of a proof are hashed, in which order, and which
// challenges each step fills.  Every prover drives its transcript through one of the two -- typlonk_prove and
// typlonk_prove_batch through RefScript, typlonk_prove_compact (sharded or not) and typlonk_prove_batch_compact through
// CompactScript -- so a change of the order is made here and nowhere else.  The hashes themselves are transcript.hpp (the
// reference's ChallengeGenerator) and compact_transcript.hpp; the verifier restates the compact order as
// compact_challenges.
#pragma once
#include "compact_transcript.hpp"
#include "transcript.hpp"

namespace ty {

struct RefScript {
    using Proof = typlonk_proof;
    ChallengeGenerator g;
    void after_round1(Proof& o) {                      // (beta, gamma) <- H([a], [b], [c])      proof.rs:111
        uint64_t ch[8];
        for (int i = 0; i < 3; ++i) g.digest(o.commit_xy[i], o.commit_inf[i]);
        g.generate(2, ch);
        memcpy(o.beta, ch, 32);
        memcpy(o.gamma, ch + 4, 32);
    }
    void after_round2(Proof& o) {                      // (alpha, zeta) <- H([a], [b], [c], [Z])  proof.rs:133-136
        uint64_t ch[8];
        g.digest(o.z_xy, o.z_inf);
        g.generate(2, ch);
        memcpy(o.alpha, ch, 32);
        memcpy(o.zeta, ch + 4, 32);
    }
};

// d0: the statement's digest (compact_statement_digest); a sharded proof has it only once its first collective has folded
// the key, so the script is constructed there
struct CompactScript {
    using Proof = typlonk_proof_compact;
    CompactTranscript tr;
    explicit CompactScript(const uint8_t d0[64]) : tr(d0) {}
    void after_round1(Proof& o) {                      // [a] [b] [c] -> beta, gamma
        for (int i = 0; i < 3; ++i) tr.point(o.commit_xy[i], o.commit_inf[i]);
        const Fr beta = tr.squeeze('b'), gamma = tr.squeeze('g');
        memcpy(o.beta, beta.v, 32);
        memcpy(o.gamma, gamma.v, 32);
    }
    void after_round2(Proof& o) {                      // [Z] -> alpha (zeta only once the quotient is bound)
        tr.point(o.z_xy, o.z_inf);
        const Fr alpha = tr.squeeze('a');
        memcpy(o.alpha, alpha.v, 32);
    }
    Fr after_quotient(Proof& o) {                      // [t_lo] [t_mid] [t_hi] -> zeta
        for (int i = 0; i < 3; ++i) tr.point(o.t_xy[i], o.t_inf[i]);
        const Fr zeta = tr.squeeze('z');
        memcpy(o.zeta, zeta.v, 32);
        return zeta;
    }
    Fr after_evals(Proof& o) {                         // the seven evaluations -> v
        for (int i = 0; i < 7; ++i) tr.scalar(o.evals[i]);
        const Fr v = tr.squeeze('v');
        memcpy(o.v, v.v, 32);
        return v;
    }
};

}  // namespace ty
