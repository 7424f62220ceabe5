// excise_core.h — the index maps of the excision kernel (excise_kernels.hip), host/device portable like fft_core.h: tests/cpu emulates
// the workgroup's lanes phase by phase with g++ to validate them without a GPU.
//
// A block runs forward on the plan PL of B and inverse on RevPlan<PL>, the plan with PL's radices reversed and the same lanes.  The
// forward's last pass leaves lane b (butterfly b = tid + it T) with bins b + r NB(last), r < R(last); RevPlan's pass 0 takes elements
// b + r NB'(0) with NB'(0) = B / R'(0) = B / R(last) = NB(last): the same registers, so the gain multiply happens in them and the spectrum
// never goes through LDS or memory.  RevPlan's last pass leaves lane b with samples b + q NB'(last), q < R'(last): NB'(last) R'(last) = B,
// so q and q + R'(last) / 2 are samples i and i + H of one lane — the overlap-add of a block's second half with the next block's first
// half is lane-local too.
#pragma once
#include "fft_plans.h"

namespace gm {

template <class PL> struct RevPlan;
template <int N, int T, int A, int B> struct RevPlan<Plan<N, T, A, B>> { using type = Plan<N, T, B, A>; };
template <int N, int T, int A, int B, int C> struct RevPlan<Plan<N, T, A, B, C>> { using type = Plan<N, T, C, B, A>; };

template <class PL> struct ExciseMap {
    using RP = typename RevPlan<PL>::type;
    static constexpr int N = PL::N, H = N / 2, T = PL::T;
    static constexpr int NBL = PL::NB(PL::NP - 1);          // bin of forward output (b, r): b + r NBL
    static constexpr int RNBL = RP::NB(RP::NP - 1);         // sample of inverse output (b, q): b + q RNBL
    static constexpr int RRL = RP::RL, HQ = RRL / 2;        // outputs q < HQ: the first half; q + HQ is sample i + H
    static constexpr int LDS_ELEMS = PL::LDS_ELEMS > RP::LDS_ELEMS ? PL::LDS_ELEMS : RP::LDS_ELEMS;
    static_assert(RP::T == T && RP::R0 == PL::RL && RP::IT0 == PL::ITL && RP::NB(0) == NBL, "the forward's last-pass registers are the inverse's pass-0 inputs");
    static_assert(RRL % 2 == 0 && HQ * RNBL == H, "outputs q and q + RL/2 of a lane are samples i and i + H");
};

// ---- the per-block adaptive rule (gnss_mi355x.h, "Block-adapt mode"), one lane's share of it --------------------------------------
// The words of p = re*re + im*im are non-negative floats, which order as their bit patterns.  med_b is the element of rank
// (B - 1) div 2 with its low 16 bits cleared: the largest word v with 16 zero low bits and count(p < v) <= rank.  Bit 31 can never be
// set (every word is below it), so the search runs over bits 30 .. 16: 15 rounds.  In a round every lane counts its own words below
// the candidate (ex_sel_below); the workgroup adds the counts (integers, any order) and every lane takes the same step (ex_sel_step).
constexpr int EX_SEL_TOP_BIT = 30, EX_SEL_LOW_BIT = 16, EX_SEL_ROUNDS = EX_SEL_TOP_BIT - EX_SEL_LOW_BIT + 1;

GM_HD float ex_power(cf v) { return v.x * v.x + v.y * v.y; }                      // each product and the sum rounded on its own
GM_HD uint32_t ex_word(float p) { uint32_t w; __builtin_memcpy(&w, &p, 4); return w; }
GM_HD float ex_float(uint32_t w) { float p; __builtin_memcpy(&p, &w, 4); return p; }
GM_HD uint32_t ex_sel_cand(uint32_t med, int bit) { return med | (1u << bit); }
GM_HD bool ex_sel_below(uint32_t word, uint32_t cand) { return word < cand; }
GM_HD uint32_t ex_sel_step(uint32_t med, uint32_t cand, uint32_t total_below, uint32_t rank) { return total_below <= rank ? cand : med; }
GM_HD bool ex_flag(float p, float factor, float med) { return p > factor * med; }  // one f32 product, strictly greater

// The flags of a block as a bit image, bit k & 31 of word k >> 5 (B / 32 words).  A bin is zeroed where any flag lies within `guard`
// (0 .. 16) bins of it, circularly: the 2 guard + 1 bits around bit k, taken from the three words around k's own.
GM_HD bool ex_zeroed(const uint32_t* bits, int k, int guard, int B) {
    const int nw = B >> 5, w = k >> 5;
    const uint32_t w0 = bits[(w + nw - 1) & (nw - 1)], w1 = bits[w], w2 = bits[(w + 1) & (nw - 1)];
    const int first = 32 + (k & 31) - guard;                                       // 16 .. 63: the window's first bit of the 96
    const uint64_t lo = (uint64_t(w1) << 32) | w0;
    const uint64_t win = (lo >> first) | (uint64_t(w2) << (64 - first));
    return (win & ((1ull << (2 * guard + 1)) - 1)) != 0;
}

}  // namespace gm
