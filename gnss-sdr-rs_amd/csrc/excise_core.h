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

}  // namespace gm
