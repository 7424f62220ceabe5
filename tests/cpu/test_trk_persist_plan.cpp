// The persistent tracking kernel's launch layout (csrc/trk_persist_plan.h) on the host: anchor configurations, the invariants of
// the fit / packed / slice rules over a sweep, the residency rule where two instantiations are possible, and stamps_fit.
// Exits non-zero on any failure.
#include <stdio.h>

#include <initializer_list>

#include "trk_persist_plan.h"

using namespace gm;

static int g_fail = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            ++g_fail;                                      \
            if (g_fail <= 40) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                  \
    } while (0)

static TrkDevCfg config(int channels, int arms, float fs, int code_len) {
    TrkDevCfg c{};
    c.fs = fs; c.n_channels = channels; c.n_arms = arms;
    c.code_index_mode = GM_CODE_INDEX_FAITHFUL; c.boc11 = 0;
    c.code_len = code_len; c.code_len_f = float(code_len);
    c.nominal_code_rate = 1.023e6f;
    return c;
}

struct Anchor { int channels, arms; float fs; int code_len, share, G, packed, grid; unsigned per; int fair_share, fair3; };
// cus = 256, two workgroups per CU for either instantiation, default knobs, 1.023 Mcps
static const Anchor anchors[] = {
    {32, 3, 25e6f, 1023, 0, 16, 0, 512, 1600, 0, 0},
    {32, 3, 4.092e6f, 1023, 0, 16, 0, 512, 320, 0, 0},
    {36, 5, 25e6f, 1023, 0, 12, 0, 480, 2112, 0, 0},
    {36, 5, 25e6f, 4092, 0, 14, 1, 504, 7168, 32, 0},
    {36, 3, 25e6f, 4092, 0, 14, 1, 504, 7168, 32, 1},
    {32, 3, 100e6f, 1023, 0, 16, 0, 512, 6272, 32, 1},
    {32, 5, 100e6f, 1023, 0, 16, 0, 512, 6272, 32, 0},
    {8, 3, 4.092e6f, 1023, 0, 32, 0, 256, 192, 0, 0},
    {8, 5, 100e6f, 1023, 0, 16, 0, 128, 6272, 32, 0},
    {64, 5, 25e6f, 1023, 0, 8, 0, 512, 3200, 0, 0},
    {36, 5, 25e6f, 4092, 1, 3, 0, 120, 33472, 32, 0},
};

static void test_anchors() {
    const TrkPersistDevice dev{256, 2, 2};
    const TrkPersistKnobs knobs;
    for (const Anchor& a : anchors) {
        const TrkDevCfg c = config(a.channels, a.arms, a.fs, a.code_len);
        const TrkPersistPlan p = trk_persist_plan(c, a.share != 0, dev, knobs);
        printf("anchor C=%d arms=%d fs=%g len=%d share=%d -> G=%d packed=%d grid=%d per=%u fair_share=%d fair3=%d key=%d lds=%zu xchg=%zu\n",
               a.channels, a.arms, double(a.fs), a.code_len, a.share, p.G, p.packed, p.grid, p.per, p.fair_share, p.fair3, p.key, p.lds_bytes, p.xchg_bytes);
        CHECK(p.G == a.G && (p.packed != 0) == (a.packed != 0) && p.grid == a.grid && p.per == a.per && p.fair_share == a.fair_share && p.fair3 == a.fair3,
              "C=%d arms=%d fs=%g len=%d share=%d", a.channels, a.arms, double(a.fs), a.code_len, a.share);
        CHECK(p.key == (a.arms == 5 ? 4 : 0) && p.strict == 0 && p.stagger == 0 && p.fair_mode == 2, "instantiation of C=%d arms=%d", a.channels, a.arms);
        CHECK(p.lds_bytes == ((size_t(a.code_len) + 3) * 4 + 15) / 16 * 16, "lds of len=%d", a.code_len);
    }
}

static void test_invariants() {
    const float rates[] = {2.046e6f, 4.092e6f, 25e6f, 100e6f};
    const int cu_counts[] = {64, 256};
    long points = 0;
    for (int idx = 1; idx <= 132; ++idx) {
        const int C = idx <= 129 ? idx : 256 << (idx - 130);      // 1..129, 256, 512, 1024
        for (int arms = 3; arms <= 5; arms += 2)
            for (float fs : rates)
                for (int share = 0; share <= 1; ++share)
                    for (int cus : cu_counts)
                        for (int per_cu = 1; per_cu <= 2; ++per_cu) {
                            const TrkDevCfg c = config(C, arms, fs, 1023);
                            const TrkPersistPlan p = trk_persist_plan(c, share != 0, TrkPersistDevice{cus, per_cu, per_cu}, TrkPersistKnobs());
                            const int nv = 2 * arms, G = p.G;
                            ++points;
#define AT "C=%d arms=%d fs=%g share=%d cus=%d per_cu=%d: G=%d packed=%d grid=%d per=%u", C, arms, double(fs), share, cus, per_cu, G, p.packed, p.grid, p.per
                            CHECK(G >= 1 && G * nv <= 256, AT);
                            CHECK(!(G >= 17 && G <= 31), AT);
                            CHECK(p.per % 64 == 0 && double(p.per) * G >= double(trk_nominal_period(c)), AT);
                            CHECK(!p.packed || (C % 8 != 0 && G <= 16), AT);
                            CHECK(p.GS == (G <= 16 ? 16 : G), AT);
                            CHECK(p.packed == (p.packed ? (C * G + 7) / 8 : 0), AT);
                            CHECK(p.grid == (p.packed ? 8 * ((C * G + 7) / 8) : (C + 7) / 8 * 8 * G), AT);
                            CHECK(p.xchg_bytes == (size_t(2) * C * p.GS * nv + size_t(C) * G) * 8, AT);
                            CHECK(G == 1 || p.grid <= cus * per_cu / (share ? 4 : 1), AT);      // resident together, or nothing to wait for
#undef AT
                        }
    }
    printf("invariants: %ld points\n", points);
}

// where a launch may take FAIR3, G comes from the smaller residency of the two instantiations; elsewhere from the plain one's
static void test_residency_rule() {
    const TrkPersistDevice one_fair{256, 2, 1}, one{256, 1, 1}, two{256, 2, 2};
    const TrkPersistKnobs knobs;
    auto same = [](const TrkPersistPlan& a, const TrkPersistPlan& b) { return a.G == b.G && a.packed == b.packed && a.grid == b.grid && a.per == b.per && a.xchg_bytes == b.xchg_bytes; };
    for (int C : {8, 32, 36}) {
        for (float fs : {4.092e6f, 100e6f}) {
            TrkDevCfg c3 = config(C, 3, fs, 1023), c5 = config(C, 5, fs, 1023), cs = c3;
            cs.strict_libm = 1;
            CHECK(same(trk_persist_plan(c3, false, one_fair, knobs), trk_persist_plan(c3, false, one, knobs)), "three arms plan for 1 per CU, C=%d fs=%g", C, double(fs));
            CHECK(same(trk_persist_plan(c5, false, one_fair, knobs), trk_persist_plan(c5, false, two, knobs)), "five arms plan for 2 per CU, C=%d fs=%g", C, double(fs));
            CHECK(same(trk_persist_plan(cs, false, one_fair, knobs), trk_persist_plan(cs, false, two, knobs)), "strict_libm plans for 2 per CU, C=%d fs=%g", C, double(fs));
            CHECK(trk_persist_plan(cs, false, one_fair, knobs).strict == 1 && trk_persist_plan(cs, false, one_fair, knobs).fair3 == 0, "strict never FAIR3");
            TrkPersistKnobs off; off.fair = 0;      // the knob that rules FAIR3 out: the plain figure again
            CHECK(same(trk_persist_plan(c3, false, one_fair, off), trk_persist_plan(c3, false, two, off)) && trk_persist_plan(c3, false, one_fair, off).fair3 == 0,
                  "GM_TRK_FAIR=0 plans for 2 per CU, C=%d fs=%g", C, double(fs));
        }
    }
    const TrkPersistPlan p = trk_persist_plan(config(32, 3, 100e6f, 1023), false, one_fair, knobs);
    CHECK(p.G == 8 && p.grid == 256 && p.fair3 == 1, "32 x 3 arms at 100 Msps on one FAIR3 workgroup per CU: G=%d grid=%d fair3=%d", p.G, p.grid, p.fair3);
}

static void test_knobs() {
    const TrkPersistDevice dev{256, 2, 2};
    const TrkDevCfg c = config(36, 5, 25e6f, 4092);
    TrkPersistKnobs k;
    k.packed = 0;
    TrkPersistPlan p = trk_persist_plan(c, false, dev, k);
    CHECK(p.G == 12 && p.packed == 0 && p.grid == 480, "GM_TRK_PACKED=0: G=%d packed=%d grid=%d", p.G, p.packed, p.grid);
    k = TrkPersistKnobs(); k.packed_g = 13;
    p = trk_persist_plan(c, false, dev, k);
    CHECK(p.G == 13 && p.packed == (36 * 13 + 7) / 8 && p.grid == 472, "GM_TRK_PACKED_G=13: G=%d packed=%d grid=%d", p.G, p.packed, p.grid);
    k = TrkPersistKnobs(); k.g = 4;
    p = trk_persist_plan(c, true, dev, k);      // the override's own check is on all the places, share_device or not
    CHECK(p.G == 4 && p.packed == 0 && p.grid == 160, "GM_TRK_G=4: G=%d packed=%d grid=%d", p.G, p.packed, p.grid);
    k.g = 13;                                   // 13 * 40 slots > 512 places: ignored
    p = trk_persist_plan(c, false, dev, k);
    CHECK(p.G == 14 && p.packed != 0, "GM_TRK_G=13 does not fit: G=%d packed=%d", p.G, p.packed);
    k = TrkPersistKnobs(); k.stagger_k = 3;
    p = trk_persist_plan(config(36, 5, 25e6f, 1023), false, dev, k);      // 12 each, unpacked, 4 rows per lane: no stagger
    CHECK(p.stagger == 0 && p.stagger_tab[0] == 0, "stagger under 8 rows per lane: %u", p.stagger);
    k.packed = 0;
    p = trk_persist_plan(c, false, dev, k);     // 12 each, unpacked: 100264 / 12 -> 8384 samples, 16 rows per lane
    CHECK(p.per == 8384 && p.stagger == 16u * 3u, "stagger: per=%u stagger=%u", p.per, p.stagger);
    // channel l of an XCD sits on CUs (12 l .. 12 l + 11) mod 32: {0..11}, {12..23}, {24..31, 0..3}, {4..15}, {16..27}; the pairs that
    // share a CU are 0-2, 0-3, 1-3, 1-4, 2-4 (a 5-cycle), so the greedy classes are 0, 0, 1, 1, 2 — and 0, 0, 1, 1 on an XCD of four
    CHECK(p.stagger_tab[0] == (1u << 4 | 1u << 6 | 2u << 8) && p.stagger_tab[1] == (1u << 4 | 1u << 6),
          "stagger classes: %#x %#x", p.stagger_tab[0], p.stagger_tab[1]);
}

static void test_stamps_fit() {
    const TrkPersistPlan p = trk_persist_plan(config(36, 5, 25e6f, 4092), false, TrkPersistDevice{256, 2, 2}, TrkPersistKnobs());
    CHECK(p.grid == 504, "grid=%d", p.grid);
    CHECK(!stamps_fit(p, -2, 0) && !stamps_fit(p, -2, 48) && !stamps_fit(p, -2, 1024 + 503) && stamps_fit(p, -2, 1024 + 504) && stamps_fit(p, -2, 4096), "every-workgroup stamps");
    for (int b : {-3, -1, 0, 1, 503, 504})
        CHECK(stamps_fit(p, b, 0) && stamps_fit(p, b, 48) && stamps_fit(p, b, 4096), "stamp_block=%d", b);
}

int main() {
    test_anchors();
    test_invariants();
    test_residency_rule();
    test_knobs();
    test_stamps_fit();
    printf("trk_persist_plan: %d failed\n", g_fail);
    return g_fail ? 1 : 0;
}
