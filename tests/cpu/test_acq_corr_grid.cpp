// Stage C's grid geometry (csrc/acq_corr_grid.h) on the host: the launcher's plan against the mirrors of the device decodes.
//
//   test_acq_corr_grid [--wrong=each_floor | --wrong=swap_hk] [--census] [--shapes]
//
// The sweep.  n_workers 1..70 x n_bins 1..512 (H = 1: n_bins = D; H = 3: n_bins = 3 D, the scratch sized for P x D), n_int in
// {1, 2, 3, 5, 15, 16, 17}, WG_PER_CU in {1, 2}, split_planes as gm_acq_create sizes it for every P from n_workers to 70.  For every
// combination: every (worker, bin, integration) visited exactly once by the blocks 0 .. grid - 1; n_int = the part count wherever an
// item is cut; every ticket below GM_CORR_SPLIT_MAX_ITEMS; plane index + n_int <= split_planes; `share` of the plan = the slots the
// decode fills.  Composite walk with cb 0 and 4: every item exactly once in 8 * slots blocks.  Long slabs: they tile the item list,
// slab * M <= 65535, no empty slab.
//
// How the in-LDS sweep is made affordable (3.3e8 items per pass over the domain).  A block's item is corr_decode_item(xcd, slot) of
// the slot corr_decode_slot(wslot) names, two functions as the device text is two statements.  (1) the UNCUT walk of every (n_workers,
// n_bins, map_mode) the sweep meets is checked once: slots 0 .. share - 1 of the eight XCDs cover the item list exactly once and slot
// `share` is empty.  (2) every plan: wslots below split_from decode to themselves with one part; the wslots from split_from to the end
// of the grid hand every slot in [split_from, share) its parts 0 .. k - 1 exactly once, k = n_int.  (1) and (2) together are the claim,
// because the item of a slot is the same call in both.  (3) and directly, without that argument: n_bins <= 40 walks the whole grid
// of every plan block by block with a count per (worker, bin, integration).
//
// --wrong swaps in a wrong decode, to show that the checks fail: each_floor rounds the leftover share of map 2 down instead of up;
// swap_hk exchanges h / split_k with h % split_k.  --census prints the classes reached over the sweep, one `class ...` line each;
// --shapes reads shapes from stdin and prints the class and the plan of each (formats at read_shapes).
// Exits non-zero on any failure.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "acq_corr_grid.h"

using namespace gm;

static int g_fail = 0;
static std::mutex g_mu;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            std::lock_guard<std::mutex> lk(g_mu);          \
            ++g_fail;                                      \
            if (g_fail <= 40) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                  \
    } while (0)

// ---- the decodes under test: the header's mirrors, or a wrong one
static int g_wrong = 0;      // 1 each_floor, 2 swap_hk
static CorrSlot decode_slot(int wslot, int split_from, int split_k) {
    if (g_wrong == 2 && wslot >= split_from) {
        const int h = wslot - split_from;
        return CorrSlot{split_from + h % split_k, h / split_k, split_k};
    }
    return corr_decode_slot(wslot, split_from, split_k);
}
static CorrItem decode_item(int xcd, int slot, int n_workers, int n_bins, int map_mode) {
    if (g_wrong == 1 && map_mode == 2) {
        const int q = n_bins >> 3, whole = q * n_workers;
        if (slot >= whole) {
            const int left = (n_bins - 8 * q) * n_workers, each = left >> 3;
            const int j = slot - whole, item = xcd * each + j;
            if (j >= each || item >= left) return CorrItem{false, -1, -1};
            return CorrItem{true, item % n_workers, 8 * q + item / n_workers};
        }
    }
    return corr_decode_item(xcd, slot, n_workers, n_bins, map_mode);
}

// ---- classes
static const char* cut_name(int c) { return c == CORR_CUT_ALL ? "all" : c == CORR_CUT_TAIL ? "tail" : "none"; }
static const char* why_name(int w) {
    switch (w) {
        case CORR_WHY_CUT: return "cut";
        case CORR_WHY_M1: return "m1";
        case CORR_WHY_STRICT: return "strict";
        case CORR_WHY_OFF: return "off";
        case CORR_WHY_SHARE: return "share";
        case CORR_WHY_MAX_K: return "max_k";
        case CORR_WHY_SCRATCH: return "scratch";
        case CORR_WHY_ONE_WG_ROUNDS: return "one_wg_rounds";
        case CORR_WHY_CLAMPED: return "clamped";
    }
    return "?";
}
static std::string lds_class(int wg, const CorrGridPlan& p) {
    char b[160];
    const int map = p.map_mode >= 16 ? 16 : p.map_mode;      // the tiled walk is one class whatever cb and rows_max
    snprintf(b, sizeof b, "lds wg=%d map=%d cut=%s why=%s rounds=%s", wg, map, cut_name(p.cut), why_name(p.why), p.share <= p.slots ? "one" : "several");
    return b;
}
static std::string comp_class(const CompGridPlan& p) {
    char b[96];
    snprintf(b, sizeof b, "comp cb=%d rounds=%s", p.cb, p.slots <= 32 ? "one" : "several");
    return b;
}
static std::string long_class(uint32_t items, uint32_t slab) {
    const uint32_t n = long_slab_count(items, slab);
    return std::string("long slabs=") + (n <= 1 ? "one" : (items % slab ? "several_ragged" : "several"));
}

static CorrGridIn lds_in(int n_workers, int n_bins, int n_int, int wg, size_t P, size_t D, bool strict) {
    CorrGridIn in;
    in.n_workers = n_workers; in.n_bins = n_bins; in.n_int = n_int; in.wg_per_cu = wg;
    in.can_split = n_int >= 2;                                  // gm_acq_create: scratch and tickets for M >= 2
    in.split_planes = in.can_split ? int(corr_split_planes(P, D, size_t(n_int))) : 0;
    in.strict_sum = strict;
    return in;
}

// ---- (1) the uncut walk of one (n_workers, n_bins, map_mode): every item exactly once in slots 0 .. share - 1, nothing at `share`
static void check_uncut(int nw, int nb, int map_mode, int share, std::vector<uint8_t>& seen) {
    const int items = nw * nb;
    seen.assign(size_t(items), 0);
    long visits = 0;
    bool last_used = false;
    for (int xcd = 0; xcd < 8; ++xcd)
        for (int slot = 0; slot < share; ++slot) {
            const CorrItem it = decode_item(xcd, slot, nw, nb, map_mode);
            if (!it.active) continue;
            if (it.w < 0 || it.w >= nw || it.d < 0 || it.d >= nb) { CHECK(false, "nw=%d nb=%d map=%d xcd=%d slot=%d -> w=%d d=%d", nw, nb, map_mode, xcd, slot, it.w, it.d); return; }
            ++seen[size_t(it.d) * nw + it.w];
            ++visits;
            if (slot == share - 1) last_used = true;
        }
    bool once = visits == items;
    for (int i = 0; i < items && once; ++i) once = seen[size_t(i)] == 1;
    CHECK(once, "uncut walk nw=%d nb=%d map=%d share=%d: %ld visits of %d items, not one each", nw, nb, map_mode, share, visits, items);
    for (int xcd = 0; xcd < 8; ++xcd)
        CHECK(!decode_item(xcd, share, nw, nb, map_mode).active, "nw=%d nb=%d map=%d: slot share=%d of XCD %d is not empty", nw, nb, map_mode, share, xcd);
    if (map_mode < 16) CHECK(last_used, "nw=%d nb=%d map=%d: no XCD uses slot share - 1 = %d (plan and decode disagree on the share)", nw, nb, map_mode, share - 1);
}

// ---- (2) the slot decode of one plan, and the ticket / plane ranges
static void check_slots(const CorrGridIn& in, const CorrGridPlan& p, std::vector<uint32_t>& parts_seen) {
    const int wslots = p.grid / 8;
#define AT "nw=%d nb=%d M=%d wg=%d planes=%d: map=%d share=%d from=%d k=%d items=%d grid=%d", in.n_workers, in.n_bins, in.n_int, in.wg_per_cu, \
           in.split_planes, p.map_mode, p.share, p.split_from, p.split_k, p.split_items, p.grid
    CHECK(p.grid % 8 == 0 && p.grid == 8 * (p.split_from + p.split_items * p.split_k) && p.split_from + p.split_items == p.share, AT);
    CHECK((p.cut == CORR_CUT_NONE) == (p.split_k == 1) && (p.cut == CORR_CUT_NONE) == (p.split_items == 0) && (p.why == CORR_WHY_CUT) == (p.cut != CORR_CUT_NONE), AT);
    CHECK(p.cut != CORR_CUT_ALL || (p.split_from == 0 && p.share <= p.slots), AT);
    CHECK(p.cut != CORR_CUT_TAIL || (p.split_from > 0 && p.share > p.slots && in.wg_per_cu != 1), AT);
    if (p.cut != CORR_CUT_NONE) {
        CHECK(p.split_k == in.n_int, AT);                                                  // a part is one integration
        CHECK(in.n_int % p.split_k == 0 && in.can_split && !in.strict_sum && in.n_int <= GM_CORR_SPLIT_MAX_K, AT);
        // the largest ticket and the end of the last item's planes, over the XCDs and the cut slots
        const size_t t_max = corr_ticket_index(7, p.share - 1, p.split_from, p.split_items);
        CHECK(t_max < size_t(GM_CORR_SPLIT_MAX_ITEMS), AT);
        CHECK(corr_plane0_index(7, p.share - 1, p.split_from, p.split_items, in.n_int) + size_t(in.n_int) <= size_t(in.split_planes), AT);
        CHECK(corr_ticket_index(0, p.split_from, p.split_from, p.split_items) == 0, AT);
    }
    for (int w = 0; w < p.split_from && w < wslots; ++w) {
        const CorrSlot s = decode_slot(w, p.split_from, p.split_k);
        if (s.slot != w || s.part != 0 || s.parts != 1) { CHECK(false, AT); break; }
    }
    parts_seen.assign(size_t(p.split_items), 0u);
    bool ok = true;
    for (int w = p.split_from; w < wslots && ok; ++w) {
        const CorrSlot s = decode_slot(w, p.split_from, p.split_k);
        ok = s.slot >= p.split_from && s.slot < p.share && s.parts == p.split_k && s.part >= 0 && s.part < s.parts &&
             !(parts_seen[size_t(s.slot - p.split_from)] >> s.part & 1u);
        if (ok) parts_seen[size_t(s.slot - p.split_from)] |= 1u << s.part;
    }
    for (int i = 0; i < p.split_items && ok; ++i) ok = parts_seen[size_t(i)] == (p.split_k >= 32 ? ~0u : (1u << p.split_k) - 1u);
    CHECK(ok, AT);
#undef AT
}

// ---- (3) the whole grid of one plan, block by block, a count per (worker, bin, integration)
static void check_grid(const CorrGridIn& in, const CorrGridPlan& p, std::vector<uint8_t>& cnt) {
    const int nw = in.n_workers, nb = in.n_bins, M = in.n_int;
    cnt.assign(size_t(nw) * nb * M, 0);
    bool ok = true;
    for (int b = 0; b < p.grid && ok; ++b) {
        const int xcd = b & 7, wslot = b >> 3;
        const CorrSlot s = decode_slot(wslot, p.split_from, p.split_k);
        const CorrItem it = decode_item(xcd, s.slot, nw, nb, p.map_mode);
        if (!it.active) continue;
        ok = it.w >= 0 && it.w < nw && it.d >= 0 && it.d < nb && (s.parts == 1 || (s.parts == M && s.part >= 0 && s.part < M));
        if (!ok) break;
        uint8_t* c = &cnt[(size_t(it.d) * nw + it.w) * M];
        if (s.parts == 1) for (int m = 0; m < M; ++m) ++c[m];      // an uncut workgroup runs the m loop itself
        else ++c[s.part];                                          // a part is integration `part`
        if (s.parts > 1) {
            ok = corr_ticket_index(xcd, s.slot, p.split_from, p.split_items) < size_t(GM_CORR_SPLIT_MAX_ITEMS) &&
                 corr_plane0_index(xcd, s.slot, p.split_from, p.split_items, M) + size_t(M) <= size_t(in.split_planes);
        }
    }
    for (size_t i = 0; i < cnt.size() && ok; ++i) ok = cnt[i] == 1;
    CHECK(ok, "whole grid nw=%d nb=%d M=%d wg=%d planes=%d: map=%d share=%d from=%d k=%d items=%d grid=%d", nw, nb, M, in.wg_per_cu, in.split_planes,
          p.map_mode, p.share, p.split_from, p.split_k, p.split_items, p.grid);
}

static const int kInts[] = {1, 2, 3, 5, 15, 16, 17};
constexpr int P_MAX = 70, BINS_MAX = 512, DIRECT_BINS = 40;

struct Tally { std::set<std::string> classes; long plans = 0, uncut = 0, direct = 0, clamp_items = 0, clamp_planes = 0; };

static void sweep_lds(int nw, Tally& t) {
    std::vector<uint8_t> seen, cnt;
    std::vector<uint32_t> parts_seen;
    for (int nb = 1; nb <= BINS_MAX; ++nb) {
        int uncut_done[3] = {0, 0, 0};                           // map modes whose uncut walk this (nw, nb) has been through
        for (int H = 1; H <= 3; H += 2) {
            if (nb % H) continue;
            const int D = nb / H;
            for (int wg = 1; wg <= 2; ++wg)
                for (int M : kInts) {
                    int last_planes = -1;
                    for (int P = nw; P <= P_MAX; ++P) {
                        const CorrGridIn in = lds_in(nw, nb, M, wg, size_t(P), size_t(D), false);
                        if (in.split_planes == last_planes) continue;      // the plan sees P through split_planes only
                        last_planes = in.split_planes;
                        const CorrGridPlan p = corr_grid_plan(in);
                        ++t.plans;
                        t.classes.insert(lds_class(wg, p));
                        CHECK(p.map_mode >= 0 && p.map_mode <= 2, "nw=%d nb=%d: map %d without an override", nw, nb, p.map_mode);
                        if (p.map_mode < 0 || p.map_mode > 2) continue;
                        if (!uncut_done[p.map_mode]) { check_uncut(nw, nb, p.map_mode, p.share, seen); uncut_done[p.map_mode] = 1; ++t.uncut; }
                        check_slots(in, p, parts_seen);
                        if (nb <= DIRECT_BINS) { check_grid(in, p, cnt); ++t.direct; }
                        // would the two clamps on split_items have bitten?  (the census of DESIGN.md §4.2: never, while n_int is the handle's M)
                        if (p.cut != CORR_CUT_NONE) {
                            const int want = p.cut == CORR_CUT_ALL ? p.share : std::min(p.share, (p.slots + p.split_k - 1) / p.split_k);
                            if (want > GM_CORR_SPLIT_MAX_ITEMS / 8) ++t.clamp_items;
                            else if (want * M > in.split_planes / 8) ++t.clamp_planes;
                        }
                    }
                    // strict_sum_order: never cut, whatever else holds
                    const CorrGridIn si = lds_in(nw, nb, M, wg, size_t(nw), size_t(D), true);
                    const CorrGridPlan sp = corr_grid_plan(si);
                    CHECK(sp.cut == CORR_CUT_NONE && sp.grid == 8 * sp.share && sp.why == (M < 2 ? CORR_WHY_M1 : CORR_WHY_STRICT), "strict nw=%d nb=%d M=%d", nw, nb, M);
                    t.classes.insert(lds_class(wg, sp));
                }
        }
    }
}

// composite walk: every item exactly once in 8 * slots blocks, cb 0 and 4 (and the default of the worker count)
static void sweep_comp(int nw, Tally& t) {
    std::vector<uint8_t> seen;
    for (int nb = 1; nb <= BINS_MAX; ++nb)
        for (int cb_env : {-1, 0, 4}) {
            const CompGridPlan p = comp_grid_plan(nw, nb, cb_env);
            if (cb_env < 0) { t.classes.insert(comp_class(p)); CHECK(p.cb == (nw > 4 ? 4 : 0), "default cb nw=%d: %d", nw, p.cb); continue; }
            const int items = nw * nb;
            seen.assign(size_t(items), 0);
            long visits = 0;
            bool ok = true;
            for (int b = 0; b < 8 * p.slots && ok; ++b) {
                const CorrItem it = comp_decode_item(b & 7, b >> 3, nw, nb, p.cb, p.rows_max);
                if (!it.active) continue;
                ok = it.w >= 0 && it.w < nw && it.d >= 0 && it.d < nb;
                if (ok) { ++seen[size_t(it.d) * nw + it.w]; ++visits; }
            }
            ok = ok && visits == items;
            for (int i = 0; i < items && ok; ++i) ok = seen[size_t(i)] == 1;
            CHECK(ok, "composite walk nw=%d nb=%d cb=%d rows_max=%d slots=%d: %ld visits of %d items", nw, nb, p.cb, p.rows_max, p.slots, visits, items);
            for (int xcd = 0; xcd < 8; ++xcd)
                CHECK(!comp_decode_item(xcd, p.slots, nw, nb, p.cb, p.rows_max).active, "composite nw=%d nb=%d cb=%d: slot %d of XCD %d is not empty", nw, nb, p.cb, p.slots, xcd);
        }
}

// the diagnostic tiled walk of the in-LDS kernels (map_mode >= 16): the same walk, cut or not
static void sweep_tiled(int nw, Tally& t) {
    std::vector<uint8_t> seen, cnt;
    std::vector<uint32_t> parts_seen;
    for (int nb = 1; nb <= 64; ++nb)
        for (int wg = 1; wg <= 2; ++wg)
            for (int M : {1, 2, 3}) {
                CorrGridIn in = lds_in(nw, nb, M, wg, size_t(nw), size_t(nb), false);
                in.cb_env = 4;
                const CorrGridPlan p = corr_grid_plan(in);
                if (p.map_mode < 16) continue;                     // more than 15 rows: the plain maps
                CHECK((p.map_mode >> 4) == 4, "tiled nw=%d nb=%d: map %d", nw, nb, p.map_mode);
                check_uncut(nw, nb, p.map_mode, p.share, seen);
                check_slots(in, p, parts_seen);
                check_grid(in, p, cnt);
                (void)t;
            }
}

static void sweep_long(Tally& t) {
    const size_t Ls[] = {1024, 6144, 63488, 262144, 524288};
    for (size_t L : Ls)
        for (int M : kInts)
            for (size_t P = 1; P <= size_t(P_MAX); ++P)
                for (size_t D = 1; D <= size_t(BINS_MAX); D += (D < 48 ? 1 : 29)) {
                    const size_t slab = long_slab_items(P, D, size_t(M), L);
                    CHECK(slab >= 1 && slab <= P * D && slab * M <= 65535 && (slab * M * L * 8 <= (size_t(128) << 20) || slab == 1), "long P=%zu D=%zu M=%d L=%zu: slab %zu", P, D, M, L, slab);
                    for (size_t nw : {size_t(1), P}) {
                        const uint32_t items = uint32_t(nw * D), n = long_slab_count(items, uint32_t(slab));
                        uint32_t next = 0;
                        bool ok = n >= 1;
                        for (uint32_t k = 0; k < n && ok; ++k) {
                            const LongSlab s = long_slab_at(items, uint32_t(slab), k);
                            ok = s.item0 == next && s.n >= 1 && s.n <= slab && size_t(s.n) * M <= 65535;
                            next = s.item0 + s.n;
                        }
                        CHECK(ok && next == items, "long slabs P=%zu D=%zu M=%d L=%zu nw=%zu: %u slabs of %zu end at %u of %u", P, D, M, L, nw, n, slab, next, items);
                        t.classes.insert(long_class(items, uint32_t(slab)));
                    }
                }
}

// the anchors: shapes whose plan is written down (the launcher's comments)
static void test_anchors() {
    struct A { int P, D, M, wg, map, share, from, k, items, grid, cut, why; };
    const A as[] = {
        {32, 41, 10, 2, 2, 164, 157, 10, 7, 1816, CORR_CUT_TAIL, CORR_WHY_CUT},       // configs[1]: 1312 items on 512 slots
        {8, 32, 2, 2, 1, 32, 0, 2, 32, 512, CORR_CUT_ALL, CORR_WHY_CUT},              // the lag sweep's cut group
        {8, 32, 2, 1, 1, 32, 0, 2, 32, 512, CORR_CUT_ALL, CORR_WHY_CUT},
        {64, 64, 1, 2, 1, 512, 512, 1, 0, 4096, CORR_CUT_NONE, CORR_WHY_M1},          // the lag sweep's full grid
        {1, 41, 10, 1, 1, 6, 0, 10, 6, 480, CORR_CUT_ALL, CORR_WHY_CUT},              // a one-PRN AcquisitionWorker handle
        {32, 41, 2, 1, 2, 164, 164, 1, 0, 1312, CORR_CUT_NONE, CORR_WHY_ONE_WG_ROUNDS},
    };
    for (const A& a : as) {
        const CorrGridPlan p = corr_grid_plan(lds_in(a.P, a.D, a.M, a.wg, size_t(a.P), size_t(a.D), false));
        printf("anchor P=%d D=%d M=%d wg=%d -> map=%d share=%d from=%d k=%d items=%d grid=%d %s\n", a.P, a.D, a.M, a.wg, p.map_mode, p.share,
               p.split_from, p.split_k, p.split_items, p.grid, lds_class(a.wg, p).c_str());
        CHECK(p.map_mode == a.map && p.share == a.share && p.split_from == a.from && p.split_k == a.k && p.split_items == a.items && p.grid == a.grid &&
              p.cut == a.cut && p.why == a.why, "anchor P=%d D=%d M=%d wg=%d", a.P, a.D, a.M, a.wg);
    }
    CHECK(corr_split_planes(1, 41, 10) == 8 * 74 && corr_split_planes(32, 41, 10) == 2560 && corr_split_planes(1, 1, 2) == 8 * 66, "scratch sizing");
    const CompGridPlan c = comp_grid_plan(36, 41, -1);
    CHECK(c.cb == 4 && c.rows_max == 7 && c.slots == 9 * 7 * 4, "composite 36 x 41: cb=%d rows_max=%d slots=%d", c.cb, c.rows_max, c.slots);
    CHECK(long_slab_items(64, 64, 1, 6144) == 2730 && long_slab_items(2, 2, 17, 262144) == 3 && long_slab_items(70, 512, 17, 1024) == 963, "long slabs");
    // the diagnostic overrides, as values
    CorrGridIn in = lds_in(8, 32, 2, 2, 8, 32, false);
    in.split_env = 0;
    CHECK(corr_grid_plan(in).cut == CORR_CUT_NONE && corr_grid_plan(in).why == CORR_WHY_OFF, "GM_CORR_SPLIT=0");
    in.split_env = 1;
    CHECK(corr_grid_plan(in).cut == CORR_CUT_NONE && corr_grid_plan(in).why == CORR_WHY_OFF, "GM_CORR_SPLIT=1");
    in.split_env = -1; in.map_forced = 0;
    CHECK(corr_grid_plan(in).map_mode == 0, "GM_CORR_MAP=0");
    in.map_forced = -1; in.items_env = 5;
    CHECK(corr_grid_plan(in).split_items == 5 && corr_grid_plan(in).split_from == 27 && corr_grid_plan(in).grid == 8 * 37, "GM_CORR_SPLIT_ITEMS=5");
    in.items_env = -1; in.stamps = true;
    CHECK(corr_grid_plan(in).cut == CORR_CUT_NONE, "stamps armed");
}

// --shapes: one shape per line of stdin ->  "shape <the line> -> <class> | <numbers>"
//   lds <P> <D> <M> <n_workers> <H> <wg_per_cu> <strict> <cb_env>   | map_mode share slots split_from split_k split_items grid cut why split_planes
//   comp <n_workers> <n_bins> <cb_env>                              | cb rows_max slots
//   long <P> <D> <M> <L> <n_workers> <H>                            | long_slab long_slabs
static int read_shapes() {
    char line[256];
    int bad = 0;
    while (fgets(line, sizeof line, stdin)) {
        line[strcspn(line, "\r\n")] = 0;
        int a[8];
        long long L;
        if (sscanf(line, "lds %d %d %d %d %d %d %d %d", &a[0], &a[1], &a[2], &a[3], &a[4], &a[5], &a[6], &a[7]) == 8) {
            CorrGridIn in = lds_in(a[3], a[1] * a[4], a[2], a[5], size_t(a[0]), size_t(a[1]), a[6] != 0);
            in.cb_env = a[7];
            const CorrGridPlan p = corr_grid_plan(in);
            printf("shape %s -> %s | %d %d %d %d %d %d %d %d %d %d\n", line, lds_class(a[5], p).c_str(), p.map_mode, p.share, p.slots, p.split_from, p.split_k,
                   p.split_items, p.grid, p.cut, p.why, in.split_planes);
        } else if (sscanf(line, "comp %d %d %d", &a[0], &a[1], &a[2]) == 3) {
            const CompGridPlan p = comp_grid_plan(a[0], a[1], a[2]);
            printf("shape %s -> %s | %d %d %d\n", line, comp_class(p).c_str(), p.cb, p.rows_max, p.slots);
        } else if (sscanf(line, "long %d %d %d %lld %d %d", &a[0], &a[1], &a[2], &L, &a[3], &a[4]) == 6) {
            const uint32_t slab = uint32_t(long_slab_items(size_t(a[0]), size_t(a[1]), size_t(a[2]), size_t(L))), items = uint32_t(a[3]) * uint32_t(a[1] * a[4]);
            printf("shape %s -> %s | %u %u\n", line, long_class(items, slab).c_str(), slab, long_slab_count(items, slab));
        } else if (line[0]) {
            printf("bad shape line: %s\n", line);
            ++bad;
        }
    }
    return bad;
}

int main(int argc, char** argv) {
    bool census = false, shapes = false;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--wrong=each_floor")) g_wrong = 1;
        else if (!strcmp(argv[i], "--wrong=swap_hk")) g_wrong = 2;
        else if (!strcmp(argv[i], "--census")) census = true;
        else if (!strcmp(argv[i], "--shapes")) shapes = true;
        else { printf("unknown argument %s\n", argv[i]); return 2; }
    }
    if (shapes) return read_shapes() ? 2 : 0;
    test_anchors();
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : nt > 8 ? 8 : nt;
    std::vector<Tally> tallies(nt);
    std::vector<std::thread> pool;
    for (unsigned k = 0; k < nt; ++k)
        pool.emplace_back([k, nt, &tallies] {
            for (int nw = P_MAX - int(k); nw >= 1; nw -= int(nt)) { sweep_lds(nw, tallies[k]); sweep_comp(nw, tallies[k]); sweep_tiled(nw, tallies[k]); }
        });
    for (std::thread& th : pool) th.join();
    Tally all;
    for (const Tally& t : tallies) {
        all.classes.insert(t.classes.begin(), t.classes.end());
        all.plans += t.plans; all.uncut += t.uncut; all.direct += t.direct; all.clamp_items += t.clamp_items; all.clamp_planes += t.clamp_planes;
    }
    sweep_long(all);
    printf("sweep: %ld plans, %ld uncut walks, %ld whole grids block by block\n", all.plans, all.uncut, all.direct);
    printf("clamps on split_items that would have bitten: MAX_ITEMS %ld, split_planes %ld\n", all.clamp_items, all.clamp_planes);
    (void)census;      // (the census is always printed; the switch is accepted for scripts that name it)
        for (const std::string& c : all.classes) printf("class %s\n", c.c_str());
    printf("acq_corr_grid: %d failed\n", g_fail);
    return g_fail ? 1 : 0;
}
