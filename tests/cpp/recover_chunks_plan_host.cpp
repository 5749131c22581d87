// recover_chunks_refusal and recover_chunks_plan (csrc/recover_chunks_plan.hpp) as the host compiles them, without any HIP header:
// reads cases
//   log_n log_l m K count nulls coset_mode [K cosets] want_coeffs want_evals want_dev [offsets_null, then count x (buffer length offset)] slices
// from stdin or from the file named by the first argument.  nulls: bit 0 a null ctx, 1 evals, 2 status, 3 report.  coset_mode: 0 = the
// cosets 0 .. K - 1 (made here, at most 2^17 of them: a K past that is refused before one is read), 1 = K cosets follow, 2 = a
// null pointer.  A buffer is named by a small number, 0 a null entry of coeffs_dev; the triples are read for count <= 64 only.
// slices = 0: the plan's own.  Prints one line of JSON per case: the verdict's code and text, and for an admitted call the plan and
// "covered": 1 when the slices, walked tile by tile the kernel's way, take every missing factor exactly once and no slice is empty,
// and the scatter's tiles take every (coset, point) exactly once (-1: too large to walk)
// (tests/test_recover_chunks_plan_host.py).
#include <cstdio>
#include <vector>

#include "../../typlonk_amd/csrc/recover_chunks_plan.hpp"

using namespace ty;

namespace {

bool rd(FILE* in, long long* v) { return fscanf(in, "%lld", v) == 1; }

int covered(const RecoverChunksPlan& p, uint32_t log_n, uint32_t log_l) {
    if (p.n > (1ull << 20)) return -1;
    std::vector<unsigned char> seen(p.missing, 0);
    bool ok = p.slices >= 1;
    for (uint32_t s = 0; s < p.slices && ok; ++s) {
        const uint64_t lo = (uint64_t)s * p.per_slice, hi = lo + p.per_slice < p.missing ? lo + p.per_slice : p.missing;
        ok = p.missing == 0 || lo < hi;   // no slice without a factor
        for (uint32_t t = 0; t < p.tiles && ok; ++t)
            for (uint32_t q = 0; q < p.tile && ok; ++q) {
                const uint64_t j = lo + (uint64_t)t * p.tile + q;
                if (j >= hi) continue;
                ok = !seen[j];
                seen[j] = 1;
            }
    }
    for (uint64_t j = 0; j < p.missing && ok; ++j) ok = seen[j] != 0;
    // the scatter: tile b of a polynomial, thread q on its way out
    std::vector<unsigned char> cell(p.n, 0);
    const uint32_t log_r = log_n - log_l;
    ok = ok && p.log_tk <= log_r && p.log_tt <= log_l && p.log_tk + p.log_tt <= 8;
    const uint64_t tiles_t = ok ? 1ull << (log_l - p.log_tt) : 1;
    for (uint64_t b = 0; b < p.scatter_tiles && ok; ++b) {
        const uint64_t k0 = (b / tiles_t) << p.log_tk, t0 = (b % tiles_t) << p.log_tt;
        for (uint32_t q = 0; q < (1u << (p.log_tk + p.log_tt)) && ok; ++q) {
            const uint64_t k = k0 + (q & ((1u << p.log_tk) - 1)), t = t0 + (q >> p.log_tk);
            ok = k < p.r && t < p.l && !cell[k + (t << log_r)];
            if (ok) cell[k + (t << log_r)] = 1;
        }
    }
    for (uint64_t i = 0; i < p.n && ok; ++i) ok = cell[i] != 0;
    return ok ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    FILE* in = argc > 1 ? fopen(argv[1], "r") : stdin;
    if (!in) return 2;
    for (;;) {
        long long v[7];
        for (int i = 0; i < 7; ++i)
            if (!rd(in, &v[i])) return i == 0 ? 0 : 2;   // a case cut short is an error
        RecoverChunksArgs a;
        a.log_n = (uint32_t)v[0];
        a.log_l = (uint32_t)v[1];
        a.m = (uint64_t)v[2];
        a.K = (uint64_t)v[3];
        a.count = (uint64_t)v[4];
        const long long nulls = v[5], mode = v[6];
        a.ctx = !(nulls & 1);
        a.evals = !(nulls & 2);
        a.status = !(nulls & 4);
        a.report = !(nulls & 8);
        std::vector<uint32_t> cosets;
        if (mode == 0) {
            const uint64_t k = a.K < (1ull << 17) ? a.K : (1ull << 17);
            for (uint64_t i = 0; i < k; ++i) cosets.push_back((uint32_t)i);
        } else if (mode == 1) {
            if (a.K > (1ull << 17)) return 2;
            for (uint64_t i = 0; i < a.K; ++i) {
                long long c;
                if (!rd(in, &c)) return 2;
                cosets.push_back((uint32_t)c);
            }
        }
        if (cosets.empty()) cosets.push_back(0);   // (a pointer that is not null, to no entry that is read)
        a.cosets = mode == 2 ? nullptr : cosets.data();
        long long w[3];
        for (int i = 0; i < 3; ++i)
            if (!rd(in, &w[i])) return 2;
        a.want_coeffs = w[0] != 0;
        a.want_evals = w[1] != 0;
        a.want_dev = w[2] != 0;
        std::vector<const void*> ids;
        std::vector<uint64_t> lens, offs;
        static const char names[64] = {};
        bool offsets_null = true;
        if (a.want_dev) {
            long long on;
            if (!rd(in, &on) || a.count > 64) return 2;
            offsets_null = on != 0;
            for (uint64_t p = 0; p < a.count; ++p) {
                long long t[3];
                for (int i = 0; i < 3; ++i)
                    if (!rd(in, &t[i])) return 2;
                if (t[0] < 0 || t[0] >= 64) return 2;
                ids.push_back(t[0] ? &names[t[0]] : nullptr);
                lens.push_back((uint64_t)t[1]);
                offs.push_back((uint64_t)t[2]);
            }
            if (ids.empty()) {   // count = 0: the arrays are there, with no entry
                ids.push_back(nullptr);
                lens.push_back(0);
                offs.push_back(0);
            }
        }
        a.buf_id = a.want_dev ? ids.data() : nullptr;
        a.buf_len = a.want_dev ? lens.data() : nullptr;
        a.offsets = a.want_dev && !offsets_null ? offs.data() : nullptr;
        long long slices;
        if (!rd(in, &slices)) return 2;
        const RecoverVerdict verdict = recover_chunks_refusal(a);
        printf("{\"code\":%d,\"text\":\"%s\",\"tile\":%u", verdict.code, verdict.text, RECOVER_TILE);
        if (verdict.code == RECOVER_ADMITTED) {
            const RecoverChunksPlan p = recover_chunks_plan(a.log_n, a.log_l, a.m, a.K, a.count, a.want_coeffs, a.want_evals, (uint32_t)slices);
            printf(",\"n\":%llu,\"l\":%llu,\"r\":%llu,\"known\":%llu,\"missing\":%llu,\"vanish_xblocks\":%u,\"slices\":%u,\"per_slice\":%llu,\"tiles\":%u,"
                   "\"log_tk\":%u,\"log_tt\":%u,\"scatter_tiles\":%llu,\"excess_len\":%llu,\"excess_blocks\":%u,\"excess_span\":%llu,\"excess_iters\":%u,"
                   "\"bytes_consts\":%llu,\"bytes_partial\":%llu,\"bytes_index\":%llu,\"bytes_cells\":%llu,\"bytes_work\":%llu,\"bytes_out\":%llu,"
                   "\"bytes_evals\":%llu,\"bytes_verdict\":%llu,\"bytes_total\":%llu,\"covered\":%d",
                   (unsigned long long)p.n, (unsigned long long)p.l, (unsigned long long)p.r, (unsigned long long)p.known, (unsigned long long)p.missing,
                   p.vanish_xblocks, p.slices, (unsigned long long)p.per_slice, p.tiles, p.log_tk, p.log_tt, (unsigned long long)p.scatter_tiles,
                   (unsigned long long)p.excess_len, p.excess_blocks, (unsigned long long)p.excess_span, p.excess_iters,
                   (unsigned long long)p.bytes_consts, (unsigned long long)p.bytes_partial, (unsigned long long)p.bytes_index,
                   (unsigned long long)p.bytes_cells, (unsigned long long)p.bytes_work, (unsigned long long)p.bytes_out,
                   (unsigned long long)p.bytes_evals, (unsigned long long)p.bytes_verdict, (unsigned long long)p.bytes_total,
                   covered(p, a.log_n, a.log_l));
        }
        printf("}\n");
    }
}
