// Host-callable launchers of the HIP kernels; each is defined in the .hip unit that holds the kernel,
// so the units compile independently (and in parallel).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ff.hpp"
#include "msm_plan.hpp"
#include "ntt_args.hpp"

namespace ty {

// Resident SRS points are 96 B of payload (x || y packed) on a 128-B stride: every gather of the
// accumulate kernel then touches exactly one 128-B line instead of 1.75 on average (PMC FETCH_SIZE
// of msm_accum_kernel: 3.9 GB -> see profiles/).
constexpr int PT_WORDS = 32;
constexpr int MSM_HEAVY_GRID = 1024;   // workgroups of msm_heavy_kernel (two wavefronts each; grid-strided over the tasks)

// arguments of the quotient pointwise kernel (quotient.hip): every array holds 4n coset evaluations
struct QuotientArgs {
    const Fr* wires[3];
    const Fr* z;
    const Fr* sel[5];  // q_l q_r q_o q_m q_c
    const Fr* sigma[3];
    const Fr* pi;
    const Fr* l0;
    const Fr* w_lo;    // powers of w_{4n}: lo[e & mask] * hi[e >> w_h]
    const Fr* bx_hi;   // beta * g * w_hi[j]  (launch_fr_scale per call: beta is per proof)
    Fr* out;
    uint64_t n4;
    uint32_t w_h;
    uint32_t k0_is_one;  // cosets[0] = 1 (plonk/src/lib.rs: the first wire's coset is H itself): no multiplication
    Fr alpha, alpha2, beta, gamma;
    Fr k[3];
    Fr zh_inv[4];      // 1 / (g^n * i^k - 1), k = index mod 4
};
void launch_fr_fill(Fr* out, uint64_t n, const Fr& value, hipStream_t s);
void launch_fr_scale(const Fr* in, uint64_t n, const Fr& factor, Fr* out, hipStream_t s);
void launch_quotient_pointwise(const QuotientArgs& a, hipStream_t s);

// grand product (plonk_ops.hip)
struct GrandProductArgs {
    const Fr* wires[3];   // witness column evaluations over the domain (n each)
    const Fr* sigma[3];   // sigma evaluations (n each)
    const Fr* w_lo;       // powers of w_n (two-level table)
    const Fr* w_hi;
    Fr* num;
    Fr* den;
    uint64_t n;
    uint32_t w_h;
    Fr beta, gamma;
    Fr kbeta[3];          // k_i * beta
};
void launch_gp_terms(const GrandProductArgs& a, hipStream_t s);
void launch_product_scan(const Fr* in, uint64_t n, int reverse, Fr* block_scratch, Fr* out, hipStream_t s);
void launch_fr_inv(const Fr* in, Fr* out, hipStream_t s);   // out[0] = in[0]^-1 on the device (one wavefront)
void launch_gp_finish(const Fr* nprefix, const Fr* dsuffix, const Fr* inv_total /* device */, uint64_t n, Fr* z, hipStream_t s);

// open(): y = p(z) and q = (p - y)/(X - z) in one suffix scan; q may be null; blocks: max(2048, ceil(m/2048)) + 1 Fr
// (the carries of more than 2048 workgroups are scanned in rounds of 2048 by the single-workgroup top stage)
void launch_open(const Fr* c, uint64_t m, const Fr& z, Fr* q, Fr* blocks, Fr* y, hipStream_t s);
struct LincombArgs {
    const Fr* poly[12];
    Fr scalar[12];
    Fr constant;
    Fr* out;
    uint64_t n;
    uint32_t terms;
};
void launch_lincomb(const LincombArgs& a, hipStream_t s);
// count <= 8 openings (quotients[k] != null: y and (p - y)/(X - z)) or evaluations (null) of polynomials of m
// coefficients, each at z0 (zsel[k] = 0) or z1 (1), in three launches; blocks: 8 * ceil(m/2048) Fr; ys[k]: device scalar
void launch_open_multi(const Fr* const* polys, Fr* const* quotients, Fr* const* ys, const uint8_t* zsel, uint32_t count,
                       uint64_t m, const Fr& z0, const Fr& z1, Fr* blocks, hipStream_t s);

// can this device run the 4096-element tiles (144 KiB of dynamic LDS)?  false: the opt-in was refused -> 1024-element tiles
bool ntt_big_tiles_available();
void launch_ntt_pass(const NttPassArgs& a, unsigned blocks, unsigned threads, size_t lds_bytes, hipStream_t s);
// the same pass on 9 x 30-bit limbs: every table in `a` is a full table in the 2^270 domain, 36 B of LDS per element
void launch_ntt_pass30(const NttPassArgs& a, unsigned blocks, unsigned threads, size_t lds_bytes, hipStream_t s);
void launch_ntt_full_table(const Fr* lo, const Fr* hi, uint32_t h, uint64_t S, uint64_t n, Fr* out, hipStream_t s);

void launch_convert_points(uint32_t* pts, const uint8_t* inf, uint64_t n, hipStream_t s);
void launch_msm_digits(const Fr* scalars, uint64_t m, uint32_t c, uint32_t W, uint32_t top_v, uint32_t* keys,
                       uint32_t* counts, hipStream_t s);
void launch_scan(const uint32_t* counts, uint64_t n, uint32_t* block_sums, uint32_t* offsets, uint32_t* cursor,
                 hipStream_t s);
// device pointers of one segmented sort (host.hpp, SortBufs): blk_hist, blk_base: nseg * nblk (+ 1) words; blk_cnt: the same
// (the staged level-1 scatter's per-workgroup count rows); seg_start: 2 * nseg words; hist514: MSM_SCHED_WORDS words
struct MsmSortPtrs {
    uint32_t *blk_hist, *blk_base, *scan_scratch, *blk_cnt, *seg_start, *entries, *counts, *offsets, *sorted, *hist514, *heavy, *tasks,
        *order;
};
// the whole segmented bucket sort of one chunk, bucket schedule (order[]) included, in the shape the plan gave it
// (msm_plan.hpp: sh.prio set = the sort runs beside an accumulation); staged_mode: 0 = the direct level-1 scatter everywhere
void launch_msm_segsort(const Fr* scalars, uint64_t m, const MsmShape& sh, const MsmSortPtrs& p, uint32_t cap, int staged_mode,
                        hipStream_t s);
// zbuf: srs_tables_scratch_bytes(len, T) bytes of scratch (one denominator per table entry)
size_t srs_tables_scratch_bytes(uint64_t len, uint32_t T);
void launch_srs_tables(uint32_t* pts, uint32_t* zbuf, uint64_t len, uint32_t c, uint32_t T, hipStream_t s);
void launch_bucket_order(const uint32_t* counts, const uint32_t* offsets, uint32_t n, uint32_t cap, uint32_t* hist514,
                         uint32_t* order, uint32_t* heavy, uint32_t* tasks, hipStream_t s);
void launch_msm_heavy(const uint32_t* points, const uint32_t* sorted, const uint32_t* hist516, uint32_t* heavy,
                      const uint32_t* tasks, uint32_t* partial, uint32_t* buckets, hipStream_t s);
void launch_msm_scatter(const uint32_t* keys, uint64_t m, uint64_t total, uint32_t* cursor, uint32_t* sorted,
                        hipStream_t s);
// lanes = 1, 2, 4, 8, 16: lanes per bucket (msm_accum_kernel / msm_accum_ml_kernel<L>); the first `split` buckets of the
// schedule (the larger ones) get `lanes`, the others lanes / 2 (split >= nbuckets: all get `lanes`)
void launch_msm_accum(const uint32_t* points, const uint32_t* offsets, const uint32_t* sorted, const uint32_t* order,
                      uint32_t nbuckets, uint32_t cap, bool init, uint32_t lanes, uint32_t split, uint32_t* buckets,
                      hipStream_t s);

// Row/column bucket reduction (msm_reduce.hip; RcShape and the bit planes it returns: msm_plan.hpp)
void launch_msm_rc_reduce(const uint32_t* buckets, const RcShape& sh, uint32_t* pb, uint32_t* pa, uint32_t* sums,
                          uint32_t* bitsum, uint32_t* out, hipStream_t s);
// launch_msm_rc_reduce with the form of its bit planes named (cl, ch >= 6): rows = one addition per wavefront (fq30_rows.hpp;
// what launch_msm_rc_reduce runs wherever the shape allows it), else one thread per point (msm_rc2_planes_kernel)
void launch_msm_rc_reduce_form(const uint32_t* buckets, const RcShape& sh, uint32_t* pb, uint32_t* pa, uint32_t* sums,
                               uint32_t* bitsum, uint32_t* out, bool rows, hipStream_t s);
// the same bit planes in two launches (msm_reduce.hip); needs msm_rc2_ok(sh); prow, pcol: nsets << (c1 - 6) points each
void launch_msm_rc2_reduce(const uint32_t* buckets, const RcShape& sh, uint32_t* prow, uint32_t* pcol, uint32_t* out,
                           hipStream_t s);
void launch_msm_rc_combine(const uint32_t* planes, const RcShape& sh, uint32_t* set_sums, hipStream_t s);
// comb: the fixed-base table of G (srs_comb_bytes() bytes, filled once by launch_srs_comb)
// divsteps inversion against the Fermat ladder on threads * per_thread residues; out: {mismatches, max rounds, calls}
void launch_fq_inv_selftest(uint64_t seed, uint32_t threads, uint32_t per_thread, uint32_t* out, hipStream_t st);
size_t srs_comb_bytes();
void launch_srs_comb(uint32_t* comb, hipStream_t st);
void launch_srs_generate(const Fr& s, uint64_t start, uint64_t n, const uint32_t* comb, uint32_t* pts, hipStream_t st);
// typlonk_srs_check / typlonk_srs_contribute (kernels: srs_gen.hip; host: srs_check.hip)
// out: three 64-bit words -- {all ones, 0, 0} going in; {min (index << 8 | class) of the failing points, their number,
// 1 when record 0 is not the fixed generator} coming out
void launch_srs_membership(const uint32_t* pts, uint64_t n, unsigned long long* out, hipStream_t st);
// pw[i] = rho^i, pw_shift[i] = rho^(i - 1) with pw_shift[0] = 0; n elements each
void launch_fr_powers(const Fr& rho, uint64_t n, Fr* pw, Fr* pw_shift, hipStream_t st);
// dst[i] = [t^i] src[i], canonical affine records; src and dst must not overlap
void launch_srs_contribute(const Fr& t, uint64_t n, const uint32_t* src, uint32_t* dst, hipStream_t st);
// typlonk_srs_g1_ntt and the FK20 openings (kernels: g1_fft.hip; host: srs_check.hip, open_chunks.hip)
// Stage 1 <= stage <= l of `blocks` transforms of 2^l >= 2 points in one launch, l <= 25, root = the generator of the domain of
// size 2^stage (forward) or its inverse: block b is src[b * src_stride, + 2^l), read by stage 1 bit-reversed, and
// dst[b * dst_stride, + 2^l), worked on in place by the later stages.  Strides in records, >= 2^l; src and dst must not overlap.
void launch_srs_g1_ntt_batch_stage(const Fr& root, uint32_t l, uint32_t stage, uint64_t blocks, const uint32_t* src, uint64_t src_stride,
                                   uint32_t* dst, uint64_t dst_stride, hipStream_t st);
// the same stage of one transform, blocks = 1, src and dst its first records: the faster kernel there (g1_fft.hip)
void launch_srs_g1_ntt_stage(const Fr& root, uint32_t log_n, uint32_t stage, const uint32_t* src, uint32_t* dst, hipStream_t st);
// pts[i] <- [k] pts[i], canonical affine records, in place
void launch_srs_g1_scale(const Fr& k, uint64_t n, uint32_t* pts, hipStream_t st);
// dst[o] = sum_{j < l} [k[(p l + j) period + i]] tab[j period + i], p = o / period, i = o % period, o < outputs: k CANONICAL words
// (not Montgomery residues) on the device, canonical affine records.  l and g powers of two, g <= min(l, 64) the slices an
// output's terms are cut into (open_chunks_plan.hpp); every g gives the same words.  outputs a multiple of period >= 1.
void launch_g1_pointwise_msm(const Fr* k, const uint32_t* tab, uint32_t* dst, uint64_t outputs, uint64_t period, uint32_t l, uint32_t g,
                             hipStream_t st);
// dst[j 2r + i] = src[(r - 2 - i) l + j] for i + 1 < r, the identity for r - 1 <= i < 2r; j < l.  r >= 2; reads src[0, r l - l)
void launch_open_chunks_gather(const uint32_t* src, uint32_t* dst, uint64_t r, uint64_t l, hipStream_t st);
// c[(p l + j) 2r + i] = k * (f_((r-1) l + j), 0 x r, f_(j), f_(l + j), ..., f_((r-2) l + j))[i] for the m <= r l coefficients of
// f[p] (zero above), p < count; f: `count` device pointers, on the device
void launch_open_chunks_coeffs(const Fr* const* f, uint64_t m, uint64_t r, uint64_t l, uint64_t count, const Fr& k, Fr* c, hipStream_t st);
// e[p n + i] = f[p][i] for i < m, zero for m <= i < n
void launch_open_chunks_pad(const Fr* const* f, uint64_t m, uint64_t n, uint64_t count, Fr* e, hipStream_t st);
// out[p r l + k l + t] = ev[p r l + k + r t]; ev and out must not overlap
void launch_open_chunks_evals(const Fr* ev, uint64_t r, uint64_t l, uint64_t count, Fr* out, hipStream_t st);
// typlonk_verify_chunks (kernels: verify_chunks.hip; host: verify_chunks_host.hip; the fold's shape: verify_chunks_plan.hpp)
// flags[i] = the reject class of record i (PC_OK, PC_NOT_ON_CURVE, PC_NOT_IN_SUBGROUP); clear: a failing record becomes the identity
void launch_chunks_membership(uint32_t* pts, uint64_t n, uint8_t* flags, bool clear, hipStream_t st);
// once per call: coset_a[i] = root_r^(cell_coset[i]) and twist[i] = w_inv^(cell_coset[i]), i < N
void launch_chunks_cosets(const uint32_t* cell_coset, uint64_t N, const Fr& root_r, const Fr& w_inv, Fr* coset_a, Fr* twist, hipStream_t st);
// The weights of the fold over the cells i of [lo, hi) with live[i] != 0 ("in"), pw[i] = rho^i: s_pi[i] = pw[i],
// s_all[i] = pw[i] coset_a[i], scale[i] = pw[i] l_inv for a cell that is in and zero for any other; s_pi[N + c] = 0 and
// s_all[N + c] = the sum of pw[i] over the cells in among order[first[c] .. first[c + 1]), c < M -- the cells of commitment c,
// ascending: `order` is a permutation of [0, N) sorted by commitment, first[0] = 0, first[M] = N.  s_pi, s_all: N + M
// elements; scale: N.
void launch_chunks_weights(const Fr* pw, const Fr* coset_a, const uint32_t* order, const uint32_t* first, const uint8_t* live, uint64_t N,
                           uint64_t M, uint64_t lo, uint64_t hi, const Fr& l_inv, Fr* s_pi, Fr* s_all, Fr* scale, hipStream_t st);
// partial[b l + j] = sum over the cells i of workgroup b's strip of twist[i]^j sum_t scale[i] evals[i l + t] mu^(-j t), j < l =
// 2^log_l, over the `cells` >= 1 cells from lo on; tw[j] = mu^(-j), j < max(l / 2, 1), mu the generator of the size-l domain;
// pl = verify_chunks_plan(cells, log_l[, strip]); partial: pl.blocks * l elements
struct VerifyChunksPlan;
void launch_chunks_fold(const Fr* evals, const Fr* scale, const Fr* twist, const Fr* tw, uint64_t lo, uint64_t cells, uint32_t log_l,
                        const VerifyChunksPlan& pl, Fr* partial, hipStream_t st);
// out[j] = sum_{b < blocks} partial[b l + j] in that order, j < l
void launch_chunks_fold_sum(const Fr* partial, uint64_t blocks, uint32_t l, Fr* out, hipStream_t st);
// typlonk_recover_chunks (kernels: recover_chunks.hip; host: recover_chunks_host.hip; every shape: recover_chunks_plan.hpp)
struct RecoverChunksPlan;
// z[k] = prod_j (pw[k] - pw[missing_idx[j]]) and z[r + k] = prod_j (gl pw[k] - pw[missing_idx[j]]), k < r, j < pl.missing, cut
// into pl.slices partial products (partial: pl.slices * 2r elements) that are multiplied in slice order; pw: r elements
void launch_recover_vanish(const Fr* pw, const uint32_t* missing_idx, const Fr& gl, const RecoverChunksPlan& pl, Fr* partial, Fr* z, hipStream_t st);
// z[i] <- 1 / z[i], i < cnt
void launch_recover_invert(Fr* z, uint64_t cnt, hipStream_t st);
// v[p n + k + r t] = cells[(p K + pos[k]) l + t] zd[k], or zero where pos[k] = RECOVER_NO_CELL; k < r, t < l, p < count
void launch_recover_scatter(const Fr* cells, const uint32_t* pos, const Fr* zd, uint64_t K, uint32_t log_n, uint32_t log_l, uint64_t count,
                            const RecoverChunksPlan& pl, Fr* v, hipStream_t st);
// v[i] *= zc_inv[i & (r - 1)], i < total
void launch_recover_scale(Fr* v, const Fr* zc_inv, uint64_t r, uint64_t total, hipStream_t st);
// Per polynomial p < count of v (n apart): first = the lowest j of [m, m + pl.excess_len) with v[p n + j] != 0.  status = fixed[p]
// when that is not zero, else TYPLONK_RECOVER_INCONSISTENT when there is such a j, else TYPLONK_RECOVER_OK.  verdict[p] = first for an
// inconsistent polynomial and all ones otherwise, verdict[count + p] = status; dst[p][0, m) (dst or dst[p] NULL: none) and
// out[p m, + m) (out NULL: none) = v[p n, + m) for an OK polynomial, zeros for any other.  mins: count * pl.excess_blocks words.
void launch_recover_finish(const Fr* v, uint64_t n, uint64_t m, uint64_t count, const RecoverChunksPlan& pl, const uint8_t* fixed,
                           Fr* const* dst, Fr* out, unsigned long long* mins, unsigned long long* verdict, hipStream_t st);

}  // namespace ty
