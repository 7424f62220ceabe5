// trk_persist_plan.h — the launch layout of the persistent tracking kernel, decided once per handle by one pure function.
// Host-only arithmetic (no HIP header): gm_trk_create asks the device three numbers (TrkPersistDevice), reads the diagnostic
// overrides (TrkPersistKnobs) and keeps the TrkPersistPlan; a launch copies it.  tests/cpu/test_trk_persist_plan.cpp runs it under g++.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/gnss_mi355x.h"

#if defined(__HIPCC__)
#define GM_PLAN_HD __host__ __device__ __forceinline__
#else
#define GM_PLAN_HD inline
#endif

namespace gm {

struct TrkDevCfg {
    float fs;
    int n_channels, n_arms;
    float el_space, vel_space;
    int code_index_mode, boc11;
    int code_len;             // chips per period
    float code_len_f;
    int gps_ca;               // 1: built-in C/A table rows (row = prn or prn-1 by mode)
    int n_codes;
    float lock_threshold; uint32_t max_lost_epochs;
    float pll_tau1, pll_tau2, dll_tau1, dll_tau2, pll_dt, dll_dt;
    float nominal_code_rate;
    // per-launch constants of the scalar epilogue, computed once on the host with IEEE f32 / f64 division
    // (fill_trk_derived): quotients of configuration constants and correctly rounded reciprocals for the
    // constant-divisor divisions
    float inv_fs, inv_len, inv_2pi;
    float pll_dt_tau1, pll_tau2_tau1, dll_dt_tau1, dll_tau2_tau1;   // dt/tau1, tau2/tau1 (LoopFilter::update :68-70)
    int div_fs_ok;            // fs significand not all ones: div_const(x, fs) is the correctly rounded quotient
    int strict_libm;          // gm_trk_cfg.strict_libm: carrier cos / sin by gm_libm.h's sincosf_glibc
    int strict_sum_order;     // gm_trk_cfg.strict_sum_order: the six / ten sums added sample by sample (trk_serial_sum_kernel)
};
inline void fill_trk_derived(TrkDevCfg& d) {
    d.inv_fs = 1.0f / d.fs; d.inv_len = 1.0f / d.code_len_f; d.inv_2pi = 1.0f / (2.0f * 3.14159265358979323846f);
    d.pll_dt_tau1 = d.pll_dt / d.pll_tau1; d.pll_tau2_tau1 = d.pll_tau2 / d.pll_tau1;
    d.dll_dt_tau1 = d.dll_dt / d.dll_tau1; d.dll_tau2_tau1 = d.dll_tau2 / d.dll_tau1;
    uint32_t bits; __builtin_memcpy(&bits, &d.fs, 4);
    d.div_fs_ok = ((bits & 0x7fffffu) != 0x7fffffu && d.fs > 1.0f && d.fs < 1.0e12f) ? 1 : 0;
}

// Persistent tracking geometry: workgroups of TRK_PERSIST_THREADS lanes, TRK_PERSIST_WG_PER_CU of them per CU.
// Two independent workgroups per CU let one channel's serial exchange + loop-filter epilogue (one wave) overlap
// the other's correlation phase.
#ifndef GM_TRK_THREADS          // (A/B switch of the workgroup shape: 256 x 4 per CU and 1024 x 1 were measured in round 6, DESIGN_HISTORY R6.10)
#define GM_TRK_THREADS 512
#define GM_TRK_WG_PER_CU 2
#endif
constexpr int TRK_PERSIST_THREADS = GM_TRK_THREADS;
constexpr int TRK_PERSIST_WG_PER_CU = GM_TRK_WG_PER_CU;

inline int trk_persistent_slots(int n_channels) { return (n_channels + 7) / 8 * 8; }   // the unpacked grid is slots * G workgroups

// persistent kernel's dynamic LDS.  Plain: [code_len + 3 floats of the padded chip row].  BOC: [2 code_len + 6 half chips, whole
// float4s][the padded chip row] — the table the fast path reads sits FIRST, at a compile-time LDS address, so that its look-ups are
// `v_lshlrev` + `ds_read offset:constant` (a run-time base costs a half-rate v_lshl_add with a scalar source per look-up)
GM_PLAN_HD int boc_plain_offset(int code_len) { return (2 * code_len + 6 + 3) & ~3; }

// samples of one nominal code period: generate_ca_code_samples(..).len() = round(fs / (code_rate / len)) at the nominal rate
inline float trk_nominal_period(const TrkDevCfg& c) { return roundf(c.fs / (c.nominal_code_rate / c.code_len_f)); }

// What the device said (trk_persist_probe, trk_kernels.hip).  per_cu_*: resident workgroups per CU of the plain (or strict) and of
// the FAIR3 instantiation this configuration's key names, each already capped at TRK_PERSIST_WG_PER_CU; where the key has no
// FAIR3 instantiation per_cu_fair repeats per_cu_plain.
struct TrkPersistDevice { int cus; int per_cu_plain; int per_cu_fair; };

// The diagnostic overrides (GM_DIAGNOSTICS=1 only), read once at gm_trk_create; the values here are the defaults.
struct TrkPersistKnobs {
    int g = 0;            // GM_TRK_G: workgroups per channel, unpacked (kept only if the grid stays resident)
    int packed = 1;       // GM_TRK_PACKED: 0 forbids the packed layout
    int packed_g = 0;     // GM_TRK_PACKED_G: fewer workgroups per channel in the packed layout
    int stagger_k = 0;    // GM_TRK_STAGGER_K: 10 ns ticks per row of samples and stagger class
    int fair = 2;         // GM_TRK_FAIR: TrkPersistArgs::fair_mode, 0 turns the priority toggle off
};

// Everything of a persistent launch that does not change between the launches of a handle.
struct TrkPersistPlan {
    int key;                  // (arms == 5 ? 4 : 0) | (code index FIXED ? 2 : 0) | (BOC(1,1) ? 1 : 0)
    int strict, fair3;        // with key: the instantiation (trk_persistent_instance)
    int G;                    // workgroups per channel
    int GS;                   // granules per arm in the exchange block: 16 for G <= 16 (a DPP row per arm), else G
    int packed;               // 0: channel slots x G (a channel's workgroups on one XCD); else the packed layout's workgroups per XCD
    int grid;                 // workgroups of the launch
    uint32_t per;             // samples per workgroup slice (multiple of 64)
    int fair_mode;            // the GM_TRK_FAIR knob
    int fair_share;           // CUs per XCD when the epochs are throughput-shaped (>= 8 samples per lane), else 0
    uint32_t stagger;         // 10 ns ticks a channel of stagger class 1 waits before its first epoch (0: none)
    uint32_t stagger_tab[2];  // the classes, 2 bits per channel of an XCD: [0] XCDs holding ceil(C / 8) channels, [1] the others
    size_t lds_bytes;         // dynamic LDS: the chip row as floats with one guard entry in front and two behind (+ the BOC half-chip table), whole 16 B
    size_t xchg_bytes;        // the exchange block: 2 * C * GS * (2 * arms) granules of partials + C * G of XCC_IDs, 8 bytes each
};

inline size_t trk_persist_lds_bytes(const TrkDevCfg& cfg) {
    size_t floats = size_t(cfg.code_len) + 3;                                    // the padded chip row
    if (cfg.boc11) floats += size_t(boc_plain_offset(cfg.code_len));             // + the half-chip table of the BOC fast path in front of it
    return (floats * sizeof(float) + 15) & ~size_t(15);
}

// the compile-time arms / code-index mode / BOC of the sample code
inline int trk_persist_key(const TrkDevCfg& cfg) {
    return (cfg.n_arms == 5 ? 4 : 0) | (cfg.code_index_mode == GM_CODE_INDEX_FIXED ? 2 : 0) | (cfg.boc11 ? 1 : 0);
}
// can a launch of this configuration take the FAIR3 instantiation (three arms with the co-tenant priority toggle)?
inline bool trk_persist_may_fair3(const TrkDevCfg& cfg, const TrkPersistKnobs& k) { return cfg.n_arms == 3 && !cfg.strict_libm && k.fair != 0; }

inline TrkPersistPlan trk_persist_plan(const TrkDevCfg& cfg, bool share_device, const TrkPersistDevice& dev, const TrkPersistKnobs& knobs) {
    TrkPersistPlan p{};
    const int C = cfg.n_channels, nv = 2 * cfg.n_arms;
    const int cus = dev.cus > 0 ? dev.cus : 1;
    const float nn = trk_nominal_period(cfg);
    p.key = trk_persist_key(cfg);
    p.strict = cfg.strict_libm ? 1 : 0;
    // All C * G workgroups must be resident at once (the exchange between a channel's workgroups spins): where the launch may
    // take either of two instantiations, G is sized for the one that fits fewer per CU.
    const bool may_fair3 = trk_persist_may_fair3(cfg, knobs);
    const int per_cu = may_fair3 && dev.per_cu_fair < dev.per_cu_plain ? dev.per_cu_fair : dev.per_cu_plain;
    const size_t slots = size_t(trk_persistent_slots(C));
    // share_device: a quarter of the places (gm_trk_cfg: the other stages' kernels run beside a tracking launch)
    const size_t places = (size_t(cus) * per_cu) / (share_device ? 4 : 1);
    int g = 1;
    bool packed = false;
    {   // the most workgroups per channel the chip holds at once (any count, not only powers of two: 36 channels take 12 each,
        // 480 of the 512 places, where 8 left a third of the chip idle and two-workgroup CUs beside one-workgroup CUs);
        // 17..31 fall back to 16, the width of the DPP totals path
        const size_t fit = places / slots;
        g = int(fit < 1 ? 1 : fit > 32 ? 32 : fit);
        while (g > 1 && g * nv > 256) --g;
        if (g > 16 && g < 32) g = 16;
    }
    {   // Packed layout: a channel count that does not fill the eight XCDs evenly (36 -> 5, 5, 5, 5, 4, 4, 4, 4 slots of 12
        // workgroups: 432 of 512 places, and the launch lasts as long as the 5-channel XCDs) is dealt as ONE run of C * G
        // workgroups, 14 each at 36 channels (504 places); a channel at the edge of an XCD's piece exchanges through the fabric.
        // Only where correlation fills the epoch (>= 8 samples per lane): a latency-chain launch wants its channels on one XCD.
        int gp = int(places / size_t(C) < 16 ? places / size_t(C) : 16);
        while (gp > 1 && gp * nv > 256) --gp;
        if (knobs.packed_g >= 1 && knobs.packed_g < gp) gp = knobs.packed_g;
        const bool shaped = nn > 0 && gp >= 1 && nn / float(gp) / float(TRK_PERSIST_THREADS) >= 8.0f;
        if ((C % 8) != 0 && gp > g && shaped && knobs.packed != 0) { g = gp; packed = true; }
    }
    // GM_TRK_G: must keep the grid resident (its own check, on all the places: share_device does not narrow it)
    if (knobs.g >= 1 && knobs.g <= 32 && size_t(knobs.g) * slots <= size_t(cus) * per_cu && knobs.g * nv <= 256) { g = knobs.g; packed = false; }
    p.G = g;
    p.GS = g <= 16 ? 16 : g;
    p.packed = packed ? (C * g + 7) / 8 : 0;
    p.grid = packed ? 8 * p.packed : int(slots) * g;     // channel slots: n_channels rounded up to the eight XCDs (empty workgroups leave at once)
    {   // slice length from the nominal code period (+1 % margin; +0.2 % where an epoch is many samples per lane: there the margin is
        // rows of work on every workgroup but the last, which takes whatever a longer period adds anyway), whole wavefronts
        const float margin = (nn > 0 && nn / float(g) / float(TRK_PERSIST_THREADS) >= 8.0f) ? 1.002f : 1.01f;
        const uint64_t n_nom = nn > 0 ? uint64_t(nn * margin) + 64 : 64;
        p.per = uint32_t(((n_nom + g - 1) / g + 63) / 64 * 64);
    }
    const uint32_t rows = p.per / uint32_t(TRK_PERSIST_THREADS);                 // samples per lane and epoch
    const int cus_xcd = cus >= 8 ? cus / 8 : 32;
    p.fair_mode = knobs.fair;
    p.fair_share = (rows >= 8 && p.fair_mode != 0) ? cus_xcd : 0;
    p.fair3 = (!p.strict && cfg.n_arms == 3 && p.fair_share) ? 1 : 0;
    // Stagger (see the kernel): only when an epoch is many samples per lane, i.e. when correlation, not the serial chain, fills it.
    // The dispatcher deals an XCD's workgroups round-robin over its CUs (measured: tools/trk_placement.py), so ordinals o and
    // o + CUs-per-XCD share a CU; channel `l` of an XCD owns ordinals [l G, (l + 1) G).  Channels that share a CU get different
    // classes (0, 1, 2: a greedy colouring — the conflict graph of five channels of twelve workgroups on 32 CUs is a 5-cycle,
    // so two classes do not do), class k starts k thirds of an epoch late.
    // (measured, round 6: the stagger alone buys NOTHING — 21.2 us per code period at BASELINE configs[4] with and without, plus
    // its own delay — because the co-tenants are not symmetric: see `fair_share`.  Off unless asked for; kept for experiments.)
    p.stagger = rows >= 8 && g >= 2 && !packed ? rows * uint32_t(knobs.stagger_k < 0 ? 0 : knobs.stagger_k) : 0u;
    if (p.stagger) {
        const int most = (C + 7) / 8;
        for (int v = 0; v < 2; ++v) {
            const int count = most - v;
            if (count < 1 || count > 8) continue;
            int cls[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int l = 0; l < count; ++l) {           // greedy: the smallest class no earlier co-tenant has
                bool used[4] = {false, false, false, false};
                for (int m = 0; m < l; ++m) {
                    bool share = false;                  // some ordinal of l and some ordinal of m differ by a multiple of `cus_xcd`
                    for (int o = l * g; o < (l + 1) * g && !share; ++o)
                        for (int q = m * g; q < (m + 1) * g; ++q)
                            if ((o - q) % cus_xcd == 0) { share = true; break; }
                    if (share) used[cls[m]] = true;
                }
                cls[l] = !used[0] ? 0 : !used[1] ? 1 : !used[2] ? 2 : 3;
                p.stagger_tab[v] |= uint32_t(cls[l]) << (2 * l);
            }
        }
    }
    p.lds_bytes = trk_persist_lds_bytes(cfg);
    p.xchg_bytes = (size_t(2) * C * p.GS * nv + size_t(C) * g) * sizeof(unsigned long long);
    return p;
}

// GM_TRK_STAMP_WG=-2 has every workgroup b write stamps[b], [512 + b] and [1024 + b]: do the `cap_words` armed by
// gm_trk_debug_stamps hold that?  (Every other stamp_block writes inside the [epochs][48] words the caller sized.)
inline bool stamps_fit(const TrkPersistPlan& p, int stamp_block, size_t cap_words) {
    return stamp_block != -2 || cap_words >= size_t(1024) + size_t(p.grid);
}

}  // namespace gm
