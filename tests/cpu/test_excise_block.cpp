// CPU run of the block-adapt rule's portable parts (gnss-sdr-rs_amd/csrc/excise_core.h: ex_sel_*, ex_flag, ex_zeroed) the way
// ex_block_decide of csrc/excise_kernels.hip uses them: the T "lanes" of a workgroup own bins b + r NBL; a round's counts are added
// over the lanes (a phase boundary stands for the barrier), every lane takes the same step; the flags go into a bit image, and every
// lane widens its own bins from three words of it.  Against a sort and a naive circular window, on: random words, all zeros (med = 0,
// nothing flagged), all equal, ties straddling the rank, denormals, one infinity, an impulse at either end (the circular guard), for
// B = 256, 1024 and 4096 and guard 0, 2 and 16.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "excise_core.h"

using namespace gm;

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// the selection as the workgroup runs it -> the median word
template <class PL> static uint32_t select_lanes(const std::vector<float>& p) {
    constexpr int B = PL::N, T = PL::T, NBL = PL::NB(PL::NP - 1), RL = PL::RL, ITL = PL::ITL;
    const uint32_t rank = uint32_t(B - 1) / 2;
    std::vector<uint32_t> med(T, 0);                                       // every lane keeps its own copy, as on the device
    for (int bit = EX_SEL_TOP_BIT; bit >= EX_SEL_LOW_BIT; --bit) {
        uint32_t total = 0;
        for (int tid = 0; tid < T; ++tid) {
            const uint32_t cand = ex_sel_cand(med[tid], bit);
            for (int it = 0; it < ITL; ++it)
                for (int r = 0; r < RL; ++r)
                    if (tid + it * T < NBL && ex_sel_below(ex_word(p[(tid + it * T) + r * NBL]), cand)) ++total;
        }
        for (int tid = 0; tid < T; ++tid) med[tid] = ex_sel_step(med[tid], ex_sel_cand(med[tid], bit), total, rank);
    }
    for (int tid = 1; tid < T; ++tid) EXPECT(med[tid] == med[0], "lanes disagree");
    return med[0];
}

template <class PL> static void one_case(const char* name, const std::vector<float>& p, float factor, int want_flags = -1) {
    constexpr int B = PL::N, T = PL::T, NBL = PL::NB(PL::NP - 1), RL = PL::RL, ITL = PL::ITL;
    // every bin is owned by exactly one (lane, it, r)
    std::vector<int> owner(B, 0);
    for (int tid = 0; tid < T; ++tid)
        for (int it = 0; it < ITL; ++it)
            for (int r = 0; r < RL; ++r)
                if (tid + it * T < NBL) ++owner[(tid + it * T) + r * NBL];
    for (int k = 0; k < B; ++k) EXPECT(owner[k] == 1, "%s B=%d: bin %d owned %d times", name, B, k, owner[k]);
    const uint32_t med = select_lanes<PL>(p);
    std::vector<uint32_t> sorted(B);
    for (int k = 0; k < B; ++k) sorted[k] = ex_word(p[k]);
    std::sort(sorted.begin(), sorted.end());
    const uint32_t want = sorted[(B - 1) / 2] & 0xFFFF0000u;
    EXPECT(med == want, "%s B=%d: median word %08x, sort says %08x", name, B, med, want);
    EXPECT((med & 0xFFFFu) == 0, "%s: low bits", name);
    // flags -> bit image -> widened mask, against the naive window
    std::vector<uint32_t> bits(B / 32, 0);
    std::vector<char> flag(B, 0);
    int n_flag = 0;
    for (int k = 0; k < B; ++k)
        if (ex_flag(p[k], factor, ex_float(med))) { flag[k] = 1; ++n_flag; bits[k >> 5] |= 1u << (k & 31); }
    if (want_flags >= 0) EXPECT(n_flag == want_flags, "%s B=%d: %d flags, expected %d", name, B, n_flag, want_flags);
    for (int guard : {0, 1, 2, 15, 16})
        for (int k = 0; k < B; ++k) {
            bool z = false;
            for (int d = -guard; d <= guard; ++d) z = z || flag[(k + d + B) & (B - 1)];
            EXPECT(ex_zeroed(bits.data(), k, guard, B) == z, "%s B=%d guard %d bin %d", name, B, guard, k);
        }
    std::printf("%-22s B=%5d median word %08x (%g), %d flags at factor %g\n", name, B, med, double(ex_float(med)), n_flag, double(factor));
}

template <class PL> static void all_cases() {
    constexpr int B = PL::N;
    unsigned s = 12345u + B;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
    std::vector<float> p(B);
    // exponentially distributed words (noise of one block) with a few strong bins
    for (auto& v : p) v = -std::log((float(rnd() % 1000000) + 0.5f) / 1e6f) * float(B);
    p[3] *= 500.0f; p[B - 1] *= 900.0f; p[B / 2] *= 700.0f;
    one_case<PL>("random", p, 16.0f);
    one_case<PL>("random, factor 6", p, 6.0f);
    // random words of every exponent
    for (auto& v : p) v = ex_float((rnd() << 8 ^ rnd()) & 0x7F7FFFFFu);
    one_case<PL>("random words", p, 16.0f);
    std::fill(p.begin(), p.end(), 0.0f);
    one_case<PL>("all zeros", p, 16.0f, 0);
    std::fill(p.begin(), p.end(), 3.25f);
    one_case<PL>("all equal", p, 16.0f, 0);
    // ties straddling the rank: the value at the rank repeats on both sides of it
    for (int k = 0; k < B; ++k) p[(k * 7) % B] = k < B / 4 ? 1.0f : (k < 3 * B / 4 ? 2.0f : 100.0f);
    one_case<PL>("ties at the rank", p, 16.0f, B / 4);
    for (int k = 0; k < B; ++k) p[k] = k < (B - 1) / 2 ? 1.0f : (k == (B - 1) / 2 ? 1.5f : 1.5000001f);
    one_case<PL>("rank on a step", p, 16.0f, 0);
    // denormals: the truncated median is 0 or a denormal with 16 low zero bits; everything above 0 * factor is flagged when it is 0
    for (int k = 0; k < B; ++k) p[k] = ex_float(uint32_t(1 + (k * 37) % 60000));
    one_case<PL>("denormals below 2^16", p, 16.0f, B);
    for (int k = 0; k < B; ++k) p[k] = ex_float(uint32_t(0x10000 + (k * 37) % 0x700000));
    one_case<PL>("denormals", p, 16.0f);
    // one infinity
    for (auto& v : p) v = 1.0f + float(rnd() % 1000) / 1000.0f;
    p[B / 3] = std::numeric_limits<float>::infinity();
    one_case<PL>("one infinity", p, 16.0f, 1);
    one_case<PL>("infinite factor", p, std::numeric_limits<float>::infinity(), 0);
    // the circular guard: an impulse in bin 0 and one in bin B - 1
    for (auto& v : p) v = 1.0f;
    p[0] = 1000.0f;
    one_case<PL>("impulse in bin 0", p, 16.0f, 1);
    p[0] = 1.0f; p[B - 1] = 1000.0f;
    one_case<PL>("impulse in bin B - 1", p, 16.0f, 1);
    p[31] = p[32] = 17.0f;                                                 // either side of a word boundary of the bit image
    one_case<PL>("word boundary", p, 16.0f, 3);
}

int main() {
    static_assert(EX_SEL_ROUNDS == 15, "15 rounds");
    all_cases<Plan256>();
    all_cases<Plan512>();
    all_cases<Plan1024>();
    all_cases<Plan2048>();
    all_cases<Plan4096>();
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
