// The launch shape of typlonk_open_chunks_*'s pointwise pass (g1_pointwise_msm_kernel, g1_fft.hip), decided on the host before
// anything is queued, in the manner of msm_plan / ntt_plan / solve_plan: a pure function of (count, r, l) with no HIP include, so
// that a host program can walk it over a grid (tests/cpp/open_chunks_plan_host.cpp).
//
// The pass computes count * 2r outputs, each the sum of l scalar multiples.  One thread takes one (output, slice): the l terms of
// an output are cut into g slices of l / g, g a power of two, never above l nor above 64 (the slices of an output lie in one
// wavefront).  A thread's chain is 255 steps of one doubling and l / g mixed additions, OPEN_CHUNKS_DBL + OPEN_CHUNKS_MADD * l / g
// multiplication times a step (g1.hpp).  g = 1 shares the doublings among all l terms and is the least work; but count * 2r / 64
// wavefronts may be far fewer than the device holds, and then the chain is the call's whole latency.  The device runs 2048 of
// these wavefronts at once (256 CUs x 4 SIMDs x the 2 waves that 213 VGPRs allow), yet the second wave of a SIMD adds little:
// measured, two waves on a SIMD finish 1.12 times what one does (profiles/r31_open_chunks.txt: 2^15 outputs of 64 terms take
// 80.2 ms at g = 2, one wave a SIMD, and 71.5 ms at g = 4, two).  So with q = the wavefronts per SIMD, rounded up, the time of
// a launch goes as
//     (DBL + MADD * l / g) * (q == 1 ? 1.12 : q)
// and g is the power of two that makes it least, the smaller one on a tie.  The first rule -- the smallest g that reaches 2048
// wavefronts -- chose g = 16 for 2^13 outputs of 16 terms, 8.3 ms, where g = 8 takes 6.9 ms; this one agrees with the fastest g of
// all four shapes that were swept (the same file).
#pragma once
#include <cstdint>

namespace ty {

constexpr uint64_t OPEN_CHUNKS_SIMDS = 1024;          // 256 CUs x 4
constexpr uint32_t OPEN_CHUNKS_MAX_SLICES = 64;
constexpr uint64_t OPEN_CHUNKS_DBL = 8, OPEN_CHUNKS_MADD = 10;   // multiplication times of g1_dbl and g1_madd
constexpr uint64_t OPEN_CHUNKS_ONE_WAVE_PCT = 112;    // a SIMD with one wave takes 1.12 x as long per wave as one with two or more

struct OpenChunksPlan {
    uint32_t g;          // slices per output: a power of two, <= min(l, 64)
    uint32_t per;        // terms per slice, l / g
    uint64_t outputs;    // count * 2r
    uint64_t threads;    // outputs * g; thread t: slice t % g of output t / g
    uint64_t blocks;     // of 64 threads
};

// the model's time of the launch with g slices, in arbitrary units
inline uint64_t open_chunks_cost(uint64_t outputs, uint64_t l, uint64_t g) {
    const uint64_t waves = (outputs * g + 63) / 64, q = (waves + OPEN_CHUNKS_SIMDS - 1) / OPEN_CHUNKS_SIMDS;
    return (OPEN_CHUNKS_DBL + OPEN_CHUNKS_MADD * (l / g)) * (q == 1 ? OPEN_CHUNKS_ONE_WAVE_PCT : 100 * q);
}

// count >= 1 polynomials, r >= 2 cosets of l = 2^log_l points; count * 2r <= 2^25
inline OpenChunksPlan open_chunks_plan(uint64_t count, uint64_t r, uint64_t l) {
    OpenChunksPlan p;
    p.outputs = count * 2 * r;
    uint64_t best = 1;
    for (uint64_t g = 2; g <= l && g <= OPEN_CHUNKS_MAX_SLICES; g *= 2)
        if (open_chunks_cost(p.outputs, l, g) < open_chunks_cost(p.outputs, l, best)) best = g;
    p.g = (uint32_t)best;
    p.per = (uint32_t)(l / best);
    p.threads = p.outputs * best;
    p.blocks = (p.threads + 63) / 64;
    return p;
}

}  // namespace ty
