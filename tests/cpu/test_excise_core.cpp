// CPU emulation of the excision kernel's block loop (gnss-sdr-rs_amd/csrc/excise_kernels.hip) from the portable headers it is built
// on (csrc/fft_core.h, csrc/excise_core.h): the T "threads" of a workgroup are run phase by phase, a phase boundary standing for a
// workgroup barrier.  For every block length: three blocks of a random stream through forward transform -> gain multiply on the
// forward's last-pass registers -> inverse transform on the plan with the radices reversed -> lane-local overlap-add, against a
// float64 O(B^2) evaluation of the definition (gnss_mi355x.h).  What this validates without a GPU: that the forward's last-pass
// registers ARE the reversed plan's pass-0 inputs, that outputs q and q + RL/2 of a lane are samples i and i + H, and the bound
// |y - y_ref| <= 1e-5 max|x| the GPU test asks of the device.
#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

#include "excise_core.h"

using namespace gm;
typedef std::complex<double> cd;

template <class PL, bool INV, int S> struct Middle {
    static void run(std::vector<cf>& lds, const std::vector<cf>& tw) {
        if constexpr (S <= PL::NP - 2) {
            constexpr int IT = PL::IT(S), R = PL::R[S];
            std::vector<cf> regs(size_t(PL::T) * IT * R);
            for (int tid = 0; tid < PL::T; ++tid)
                Fft<PL, INV>::template mid_stage1<S>(*reinterpret_cast<cf(*)[IT][R]>(&regs[size_t(tid) * IT * R]), lds.data(), tw.data(), tid);
            for (int tid = 0; tid < PL::T; ++tid)
                Fft<PL, INV>::template mid_stage2<S>(*reinterpret_cast<cf(*)[IT][R]>(&regs[size_t(tid) * IT * R]), lds.data(), tid);
            Middle<PL, INV, S + 1>::run(lds, tw);
        }
    }
};

static void dft(const std::vector<cd>& x, std::vector<cd>& X, bool inv) {
    const int N = int(x.size());
    std::vector<cd> w(N);
    for (int i = 0; i < N; ++i) w[i] = std::polar(1.0, (inv ? 2.0 : -2.0) * M_PI * i / N);
    for (int k = 0; k < N; ++k) {
        cd acc = 0;
        size_t idx = 0;
        for (int n = 0; n < N; ++n) { acc += x[n] * w[idx]; idx += k; if (idx >= size_t(N)) idx -= N; }
        X[k] = acc;
    }
}

template <class PL> static double run_block_loop(const char* name) {
    using MAP = ExciseMap<PL>;
    using RP = typename MAP::RP;
    constexpr int B = MAP::N, H = MAP::H, T = MAP::T, NB0 = PL::NB(0), NBL = MAP::NBL, RNBL = MAP::RNBL, RRL = MAP::RRL, HQ = MAP::HQ;
    constexpr int NBLOCKS = 3;
    std::vector<cf> x((NBLOCKS + 1) * H), lds(MAP::LDS_ELEMS), twf(PL::TW_TOTAL + 1), twi(RP::TW_TOTAL + 1), y((NBLOCKS - 1) * H, cf_make(1e30f, 1e30f));
    std::vector<float> wa(B), ws(B), g(B);
    fill_twiddles<PL>(twf.data(), false, [](double a) { return std::cos(a); }, [](double a) { return std::sin(a); });
    fill_twiddles<RP>(twi.data(), true, [](double a) { return std::cos(a); }, [](double a) { return std::sin(a); });
    unsigned s = 999u + B;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return float(int(s >> 8) % 2001 - 1000) / 100.f; };
    float xmax = 0.f;
    for (auto& v : x) { v = cf_make(rnd(), rnd()); xmax = std::fmax(xmax, std::hypot(v.x, v.y)); }
    for (int i = 0; i < B; ++i) {
        const double sn = std::sin(M_PI * double(i) / double(B));
        wa[i] = float(sn); ws[i] = float(sn / double(B));
        g[i] = (i % 7 == 3) ? 0.0f : (i % 5 == 1 ? 0.25f + 0.5f * float(i) / float(B) : 1.0f);
    }
    std::vector<cf> prev(size_t(T) * RP::ITL * HQ);
    for (int j = 0; j < NBLOCKS; ++j) {
        // forward on PL: pass 0 (windowed loads), barrier, scatter, middle passes, last pass into registers X
        std::vector<cf> X(size_t(T) * PL::ITL * PL::RL), u(size_t(T) * RP::ITL * RRL);
        {
            std::vector<cf> regs(size_t(T) * PL::IT0 * PL::R0);
            for (int tid = 0; tid < T; ++tid)
                Fft<PL, false>::pass0_stage1(*reinterpret_cast<cf(*)[PL::IT0][PL::R0]>(&regs[size_t(tid) * PL::IT0 * PL::R0]), [&](int it, int r) {
                    const int i = (tid + it * T) + r * NB0;
                    const cf v = x[j * H + i];
                    return cf_make(wa[i] * v.x, wa[i] * v.y); }, tid);
            for (int tid = 0; tid < T; ++tid)
                Fft<PL, false>::pass0_stage2(*reinterpret_cast<cf(*)[PL::IT0][PL::R0]>(&regs[size_t(tid) * PL::IT0 * PL::R0]), lds.data(), tid);
        }
        Middle<PL, false, 1>::run(lds, twf);
        for (int tid = 0; tid < T; ++tid) {
            cf v[PL::ITL][PL::RL];
            auto& Xt = *reinterpret_cast<cf(*)[PL::ITL][PL::RL]>(&X[size_t(tid) * PL::ITL * PL::RL]);
            Fft<PL, false>::last_stage1(v, lds.data(), twf.data(), tid);
            Fft<PL, false>::last_stage2(v, [&](int it, int q, cf val) { Xt[it][q] = val; }, tid);
        }
        // inverse on RP: pass 0 takes the SAME registers, times the gain of bin (tid + it T) + r NBL
        {
            std::vector<cf> regs(size_t(T) * RP::IT0 * RP::R0);
            for (int tid = 0; tid < T; ++tid) {
                auto& Xt = *reinterpret_cast<cf(*)[PL::ITL][PL::RL]>(&X[size_t(tid) * PL::ITL * PL::RL]);
                Fft<RP, true>::pass0_stage1(*reinterpret_cast<cf(*)[RP::IT0][RP::R0]>(&regs[size_t(tid) * RP::IT0 * RP::R0]), [&](int it, int r) {
                    const float gk = g[(tid + it * T) + r * NBL];
                    return cf_make(gk * Xt[it][r].x, gk * Xt[it][r].y); }, tid);
            }
            for (int tid = 0; tid < T; ++tid)
                Fft<RP, true>::pass0_stage2(*reinterpret_cast<cf(*)[RP::IT0][RP::R0]>(&regs[size_t(tid) * RP::IT0 * RP::R0]), lds.data(), tid);
        }
        Middle<RP, true, 1>::run(lds, twi);
        for (int tid = 0; tid < T; ++tid) {
            cf v[RP::ITL][RRL];
            auto& ut = *reinterpret_cast<cf(*)[RP::ITL][RRL]>(&u[size_t(tid) * RP::ITL * RRL]);
            auto& pt = *reinterpret_cast<cf(*)[RP::ITL][HQ]>(&prev[size_t(tid) * RP::ITL * HQ]);
            Fft<RP, true>::last_stage1(v, lds.data(), twi.data(), tid);
            Fft<RP, true>::last_stage2(v, [&](int it, int q, cf val) { ut[it][q] = val; }, tid);
            for (int it = 0; it < RP::ITL; ++it) {
                const int b = tid + it * T;
                if (b >= RNBL) continue;
                for (int q = 0; q < HQ; ++q) {
                    const int i = b + q * RNBL;
                    if (i >= H) { std::printf("%s: sample index %d outside the first half\n", name, i); return 1.0; }
                    if (j > 0) {
                        cf& dst = y[(j - 1) * H + i];
                        if (dst.x != 1e30f) { std::printf("%s: output %d written twice\n", name, i); return 1.0; }
                        dst = cf_make(pt[it][q].x + ws[i] * ut[it][q].x, pt[it][q].y + ws[i] * ut[it][q].y);
                    }
                    pt[it][q] = cf_make(ws[i + H] * ut[it][q + HQ].x, ws[i + H] * ut[it][q + HQ].y);
                }
            }
        }
    }
    // the definition in float64 (the f32 window words and gains as given)
    std::vector<std::vector<cd>> ub(NBLOCKS, std::vector<cd>(B));
    for (int j = 0; j < NBLOCKS; ++j) {
        std::vector<cd> in(B), sp(B);
        for (int i = 0; i < B; ++i) in[i] = double(wa[i]) * cd(x[j * H + i].x, x[j * H + i].y);
        dft(in, sp, false);
        for (int k = 0; k < B; ++k) sp[k] *= double(g[k]);
        dft(sp, ub[j], true);
    }
    double worst = 0;
    for (int sgm = 0; sgm < NBLOCKS - 1; ++sgm)
        for (int i = 0; i < H; ++i) {
            const cd want = double(ws[i + H]) * ub[sgm][i + H] + double(ws[i]) * ub[sgm + 1][i];
            const cf got = y[sgm * H + i];
            if (got.x == 1e30f) { std::printf("%s: output %d never written\n", name, sgm * H + i); return 1.0; }
            worst = std::fmax(worst, std::abs(want - cd(got.x, got.y)) / (1e-5 * double(xmax)));
        }
    std::printf("%-10s B=%5d T=%4d reversed [", name, B, T);
    for (int p = 0; p < RP::NP; ++p) std::printf("%s%d", p ? "," : "", RP::R[p]);
    std::printf("] largest |y - y_ref| / (1e-5 max|x|) = %.4f\n", worst);
    return worst;
}

int main() {
    double worst = 0;
    worst = std::fmax(worst, run_block_loop<Plan256>("Plan256"));
    worst = std::fmax(worst, run_block_loop<Plan512>("Plan512"));
    worst = std::fmax(worst, run_block_loop<Plan1024>("Plan1024"));
    worst = std::fmax(worst, run_block_loop<Plan2048>("Plan2048"));
    worst = std::fmax(worst, run_block_loop<Plan4096>("Plan4096"));
    std::printf("worst %.4f\n", worst);
    return worst <= 1.0 ? 0 : 1;
}
