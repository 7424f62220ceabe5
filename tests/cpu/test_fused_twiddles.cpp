// CPU check of the constant twiddles folded into the butterflies (gnss-sdr-rs_amd/csrc/fft_core.h: ct::rotation, Rot, DftS, BflyTw).
// For both directions and every twiddle row the hybrid plans use — (R, M, K) = (25, 125, 0..4) and (16, 64, 0..3) — 2000 random
// butterflies go through BflyTw's stage 1 + stage 2 and through the plain Bfly + ConstTw path; each is compared with a float64 DFT
// of the float64-twiddled inputs.  The error of an output is taken relative to the RMS magnitude of its butterfly's true outputs
// (an output that happens to be near zero says nothing about a relative error of its own).
//   every output finite; fused maximum <= 1.5 x the plain maximum on the same inputs
// (the fused form has no more roundings per output than the plain one, but its constants are ratios of rounded scales: up to
// 1.5 ulp of constant error against 0.5).
// The same check for the second layer of pass 0's radix 20 = 4 x 5 (Good-Thomas, no twiddles): Bfly<20>::stage2 with DftS<5> at unit
// scales against the plain Dft<5>.
// Last line: relative L2 error of the whole inverse transform of the product's CorrPlan8000 under the product's trait
// (acq_corr_plans.h, through fft_plans.h); tests/test_fused_twiddles.py builds the program a second time with -DGM_NO_FUSED_TW, which
// turns the form off everywhere, and compares the two figures.
#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

#include "fft_core.h"
#include "fft_plans.h"

using namespace gm;

static unsigned g_seed = 20240611u;
static float rnd() {
    g_seed = g_seed * 1664525u + 1013904223u;
    return float(int(g_seed >> 8) % 20001 - 10000) / 1000.f;
}

static int g_fail = 0;
static double g_worst_ratio = 0;

template <int R, int M, int K, bool INV> static void row() {
    constexpr int NBF = 2000;
    std::complex<double> w[R], wr[R * R];
    for (int r = 0; r < R; ++r) w[r] = std::polar(1.0, (INV ? 2.0 : -2.0) * M_PI * double((long(K) * r) % M) / M);
    for (int i = 0; i < R * R; ++i) wr[i] = std::polar(1.0, (INV ? 2.0 : -2.0) * M_PI * double(i % R) / R);
    double max_f = 0, max_p = 0;
    bool finite = true;
    for (int n = 0; n < NBF; ++n) {
        cf x[R], vf[R], vp[R], yf[R], yp[R];
        for (int r = 0; r < R; ++r) x[r] = cf_make(rnd(), rnd());
        BflyTw<R, INV, K, M>::stage1([&](int r) { return x[r]; }, vf);
        BflyTw<R, INV, K, M>::stage2(vf, [&](int k, cf val) { yf[k] = val; });
        Bfly<R, INV>::stage1([&](int r) { return ConstTw<INV, K, M, R>::mul(x[r], r); }, vp);
        Bfly<R, INV>::stage2(vp, [&](int k, cf val) { yp[k] = val; });
        std::complex<double> ref[R];
        double pw = 0;
        for (int k = 0; k < R; ++k) {
            std::complex<double> acc = 0;
            for (int r = 0; r < R; ++r) acc += std::complex<double>(x[r].x, x[r].y) * w[r] * wr[(k * r) % R];
            ref[k] = acc;
            pw += std::norm(acc);
        }
        const double rms = std::sqrt(pw / R);
        for (int k = 0; k < R; ++k) {
            finite = finite && std::isfinite(yf[k].x) && std::isfinite(yf[k].y) && std::isfinite(yp[k].x) && std::isfinite(yp[k].y);
            max_f = std::fmax(max_f, std::abs(ref[k] - std::complex<double>(yf[k].x, yf[k].y)) / rms);
            max_p = std::fmax(max_p, std::abs(ref[k] - std::complex<double>(yp[k].x, yp[k].y)) / rms);
        }
    }
    const double ratio = max_f / max_p;
    const bool ok = finite && max_f <= 1.5 * max_p && max_p < 1e-5;
    g_worst_ratio = std::fmax(g_worst_ratio, ratio);
    if (!ok) ++g_fail;
    std::printf("row R=%2d M=%3d K=%d %s  fused_max=%.3e plain_max=%.3e ratio=%.3f %s\n", R, M, K, INV ? "inv" : "fwd", max_f, max_p, ratio,
                ok ? "ok" : (finite ? "FAIL" : "FAIL (not finite)"));
}

template <bool INV> static void row20() {
    constexpr int R = 20, NBF = 2000;
    std::complex<double> wr[R];
    for (int i = 0; i < R; ++i) wr[i] = std::polar(1.0, (INV ? 2.0 : -2.0) * M_PI * double(i) / R);
    double max_f = 0, max_p = 0;
    bool finite = true;
    for (int n = 0; n < NBF; ++n) {
        cf x[R], v[R], yf[R], yp[R];
        for (int r = 0; r < R; ++r) x[r] = cf_make(rnd(), rnd());
        Bfly<R, INV>::stage1([&](int r) { return x[r]; }, v);
        Bfly<R, INV>::template stage2<DftS<5, INV, UnitScales>>(v, [&](int k, cf val) { yf[k] = val; });
        Bfly<R, INV>::stage2(v, [&](int k, cf val) { yp[k] = val; });
        std::complex<double> ref[R];
        double pw = 0;
        for (int k = 0; k < R; ++k) {
            std::complex<double> acc = 0;
            for (int r = 0; r < R; ++r) acc += std::complex<double>(x[r].x, x[r].y) * wr[(k * r) % R];
            ref[k] = acc;
            pw += std::norm(acc);
        }
        const double rms = std::sqrt(pw / R);
        for (int k = 0; k < R; ++k) {
            finite = finite && std::isfinite(yf[k].x) && std::isfinite(yf[k].y);
            max_f = std::fmax(max_f, std::abs(ref[k] - std::complex<double>(yf[k].x, yf[k].y)) / rms);
            max_p = std::fmax(max_p, std::abs(ref[k] - std::complex<double>(yp[k].x, yp[k].y)) / rms);
        }
    }
    const double ratio = max_f / max_p;
    const bool ok = finite && max_f <= 1.5 * max_p && max_p < 1e-5;
    g_worst_ratio = std::fmax(g_worst_ratio, ratio);
    if (!ok) ++g_fail;
    std::printf("row20 R=20 (4 x 5, unit scales) %s  fused_max=%.3e plain_max=%.3e ratio=%.3f %s\n", INV ? "inv" : "fwd", max_f, max_p, ratio, ok ? "ok" : "FAIL");
}

template <bool INV> static void rows() {
    row<25, 125, 0, INV>(); row<25, 125, 1, INV>(); row<25, 125, 2, INV>(); row<25, 125, 3, INV>(); row<25, 125, 4, INV>();
    row<16, 64, 0, INV>(); row<16, 64, 1, INV>(); row<16, 64, 2, INV>(); row<16, 64, 3, INV>();
}

// the whole transform, lane by lane and barrier phase by barrier phase (as tests/cpu/test_fft_core.cpp runs it)
template <class HP, bool INV> static double run_hybrid() {
    constexpr int N = HP::N, T = HP::T;
    std::vector<cf> x(N), xs(N), y(N, cf_make(1e30f, 1e30f)), lds(HP::LDS_ELEMS);
    unsigned s = 777u + N;
    for (int i = 0; i < N; ++i) {
        s = s * 1664525u + 1013904223u; float a = float(int(s >> 8) % 2001 - 1000) / 100.f;
        s = s * 1664525u + 1013904223u; float b = float(int(s >> 8) % 2001 - 1000) / 100.f;
        x[i] = cf_make(a, b);
        xs[HP::in_slot(i)] = x[i];
    }
    using F = Fft<HP, INV>;
    std::vector<cf> r0(size_t(T) * HP::R0), r1(size_t(T) * HP::R[1]);
    for (int tid = 0; tid < T; ++tid)
        F::pass0_stage1(*reinterpret_cast<cf(*)[1][HP::R0]>(&r0[size_t(tid) * HP::R0]), [&](int, int r) { return xs[tid + r * HP::NB(0)]; }, tid);
    for (int tid = 0; tid < T; ++tid) F::pass0_stage2(*reinterpret_cast<cf(*)[1][HP::R0]>(&r0[size_t(tid) * HP::R0]), lds.data(), tid);
    for (int tid = 0; tid < T; ++tid) F::template mid_stage1<1>(*reinterpret_cast<cf(*)[1][HP::R[1]]>(&r1[size_t(tid) * HP::R[1]]), lds.data(), nullptr, tid);
    for (int tid = 0; tid < T; ++tid) F::template mid_stage2<1>(*reinterpret_cast<cf(*)[1][HP::R[1]]>(&r1[size_t(tid) * HP::R[1]]), lds.data(), tid);
    for (int tid = 0; tid < T; ++tid) {
        cf v[1][HP::RL];
        F::last_stage1(v, lds.data(), nullptr, tid);
        F::last_stage2(v, [&](int, int q, cf val) { y[HP::out_index(tid, q)] = val; }, tid);
    }
    std::vector<std::complex<double>> w(N);
    for (int i = 0; i < N; ++i) w[i] = std::polar(1.0, (INV ? 2.0 : -2.0) * M_PI * i / N);
    double num = 0, den = 0;
    for (int k = 0; k < N; ++k) {
        std::complex<double> acc = 0;
        size_t idx = 0;
        for (int n = 0; n < N; ++n) { acc += std::complex<double>(x[n].x, x[n].y) * w[idx]; idx += k; if (idx >= size_t(N)) idx -= N; }
        num += std::norm(acc - std::complex<double>(y[k].x, y[k].y)); den += std::norm(acc);
    }
    return std::sqrt(num / den);
}

int main() {
    rows<true>();
    rows<false>();
    row20<true>();
    row20<false>();
    std::printf("rows: %d failed, worst fused/plain ratio %.3f (bound 1.5)\n", g_fail, g_worst_ratio);
    using HP = CorrPlan8000;
    std::printf("fused=%d\n", int(fuse_tw_v<HP>));
    std::printf("Hybrid8000 fwd rel_l2_err=%.4e\n", run_hybrid<HP, false>());
    std::printf("Hybrid8000 inv rel_l2_err=%.4e\n", run_hybrid<HP, true>());
    return g_fail ? 1 : 0;
}
