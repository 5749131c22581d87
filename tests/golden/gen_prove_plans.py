"""Generates tests/golden/prove_plans.json: what the provers of commit e6afaa5 -- the last one before csrc/prove_plan.hpp --
asked ensure() for over ONE call -- the largest request per buffer -- with their pinned slots, wave size and region offsets.
The requests are that commit's own formulas restated by hand, in call order and each beside the place it stood; the fixture
keeps the largest of each list.  Nothing here reads prove_plan.hpp.

    python tests/golden/gen_prove_plans.py      # rewrites the fixture deterministically
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
FR = 32                                   # sizeof(Fr): 8 x 32-bit limbs
LOG_NS = [0, 1, 3, 10, 11, 12, 16, 20, 22, 24]
PROOFS = [1, 2, 5, 64, 70]
SESSION, WAVE = 0, 1

# sizeof(PbTables), prove_batch.hip:60-68 with PB_MAX = 64, PB_ITEMS = 8, LIN_TERMS = 10:
#   gp 64 x 5 Fr | quot 64 x (4 Fr + 8 u32) | lin 64 x 11 Fr | item 512 x (3 pointers + u64) | ritem 128 x the same |
#   fold 64 x (11 + 6) Fr | zpow 128 x 32 Fr
PB_TABLES = 64 * 5 * FR + 64 * (4 * FR + 32) + 64 * 11 * FR + 512 * 32 + 128 * 32 + 64 * 17 * FR + 128 * 32 * FR


def n_hi(log_n):
    """entries of domain_twiddles' hi table for the 4n domain (ntt_host.hip:179-190, ntt_plan.hpp ntt_push_pair)"""
    log4 = log_n + 2
    return 1 << (log4 - (log4 + 1) // 2)


def session(log_n, cached):
    """typlonk_prove: rounds 1, 2, 3 of prover.hip; cached = 0: typlonk_quotient_dev without a circuit id, alone"""
    n = 1 << log_n
    nblk = (n + 2047) // 2048
    n4 = 4 * n
    if not cached:
        return {"quot_ext": [14 * n4 * FR],                       # quotient_run, prover.hip:166
                "quot_tab": [n_hi(log_n) * FR]}                   # :204
    opens = max(8 * 2048, 8 * nblk) * FR                          # prover_ops_tmp, :362-365
    return {"prover_mem": [19 * n * FR],                          # prover_round1_impl, :459
            "quot_ext": [5 * n4 * FR] * 4                         # prover_extend: a, b, c, PI, :350
                        + [5 * n4 * FR]                           # prover_extend: Z (round 2)
                        + [5 * n4 * FR],                          # quotient_run with a cached circuit, :166
            "ops_tmp": [(4 * n + nblk + 8) * FR]                  # typlonk_grand_product_dev (round 2), :234
                       + [opens] * 4,                             # round 3: prover_open_round3, prover_fetch, r's opening, the last fetch
            "quot_tab": [n_hi(log_n) * FR],                       # quotient_run, :204
            "batch_tab": []}


def wave(log_n, count):
    """prove_batch_impl, prove_batch.hip:704-718, and wave_quotient, :459"""
    n = 1 << log_n
    nblk = (n + 2047) // 2048
    G = min(count, 64, max(1, (1 << 22) >> log_n))                # :704
    return G, {"prover_mem": [G * 39 * n * FR],                   # :706
               "ops_tmp": [G * 8 * nblk * FR],                    # :707
               "batch_tab": [PB_TABLES],                          # :708
               "quot_tab": [n_hi(log_n) * FR],                    # wave_quotient, :459; the same in every wave of the call
               "quot_ext": []}


def largest(req):
    return {buf: max(asked, default=0) for buf, asked in req.items()}


def main():
    cases = []
    for lg in LOG_NS:
        for proofs in PROOFS:
            cases.append([lg, proofs, SESSION, 1, 1, 16, largest(session(lg, 1))])
            G, req = wave(lg, proofs)
            cases.append([lg, proofs, WAVE, 1, G, G * 16, largest(req)])                 # slots: prove_batch.hip:710-716
        cases.append([lg, 1, SESSION, 0, 1, None, largest(session(lg, 0))])
    out = {
        "about": "What commit e6afaa5 (the parent of prove_plan.hpp) requested, restated by hand from its formulas by "
                 "tests/golden/gen_prove_plans.py (each formula cites its line there); not captured from a run, and nothing in it "
                 "comes from prove_plan.hpp.  case = [log_n, proofs, mode (0 session, 1 wave), cached, G, pinned slots, "
                 "{buffer: the largest ensure() request in bytes, 0: none}].  A session with cached = 0 is typlonk_quotient_dev without "
                 "a circuit id, which touches quot_ext and quot_tab only.",
        # prover_round1_impl's carving loop (prover.hip:468-475) and PB_EV .. PB_STRIDE (prove_batch.hip:35), in units of n
        "regions": {"ev": [0, 3], "co": [3, 3], "pi": [6, 1], "z": [7, 1], "t": [8, 4], "q": [12, 6], "r": [18, 1], "ext": [19, 20]},
        "stride": [19, 39],
        # which q each shape used: prover.hip:658-667 (reference), :773-780 (batched openings), :953-962 (compact) and the
        # same in prove_batch.hip:511, 529, 629-650
        "q": {"wit_a": 0, "wit_b": 1, "wit_c": 2, "wit_z": 3, "wit_zw": 4, "wit_r": 5, "batched_f": 5, "batched_wit": 0,
              "compact_f": 1, "compact_wit": 0},
        # REF_SLOTS, COMPACT_SLOTS (host.hpp:410-411) and the wave's PB_SLOT_F, PB_SLOT_R (prove_batch.hip:33).  The single
        # prover had r(zeta) in slot 0 and F(zeta) in slot 0 (batched openings) or 1 (compact), over values already fetched;
        # it now uses the wave's slots.  f of the reference shape (batched openings) had no slot in a wave: null
        "ref_slots": {"wire": 0, "z": 3, "sig0": 4, "sig1": 5, "pi": 6, "zw": 8, "count": 9, "r": 9, "f": None},
        "compact_slots": {"wire": 0, "z": 3, "sig0": 5, "sig1": 6, "pi": 7, "zw": 4, "count": 8, "r": 9, "f": 8},
        "slots_per_proof": 16,
        "cases": cases,
    }
    with open(os.path.join(HERE, "prove_plans.json"), "w") as f:
        f.write("{\n")
        for k, v in out.items():
            if k != "cases":
                f.write(json.dumps(k) + ": " + json.dumps(v) + ",\n")
        f.write('"cases": [\n' + ",\n".join(json.dumps(c, separators=(",", ":")) for c in cases) + "\n]\n}\n")


if __name__ == "__main__":
    main()
