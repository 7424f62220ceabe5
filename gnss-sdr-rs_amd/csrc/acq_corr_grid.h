// acq_corr_grid.h — how stage C's workgroups are dealt onto (worker, Doppler bin, integration) items, decided by pure functions.
// Host-only arithmetic (no HIP header): Launch<PL>::corr (acq_kernels.hip), CompLaunch::corr (acq_composite.hip) and gm_acq_create
// (gm_api.hip) call the plan functions; the kernels decode the plan on the device, and the host mirrors of those decodes below
// restate the device text line for line.  tests/cpu/test_acq_corr_grid.cpp runs both under g++ and holds them to each other:
// every (worker, bin, integration) exactly once, every ticket and scratch index in range.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/gnss_mi355x.h"

namespace gm {

// tail split of the correlation grid: per XCD about one resident round of slots (64) worth of parts, one part per
// integration (up to GM_CORR_SPLIT_MAX_K integrations; longer dwells are not cut); the scratch holds GM_CORR_SPLIT_MAX_SLABS
// power planes — one per part — and there is one ticket per cut item
constexpr int GM_CORR_SPLIT_MAX_K = 16;
constexpr int GM_CORR_SPLIT_MAX_SLABS = 8 * 320;
constexpr int GM_CORR_SPLIT_MAX_ITEMS = 8 * 80;

// ------------------------------------------------------------------------------------ in-LDS stage C: the plan
// What Launch<PL>::corr knows when it decides.  The four diagnostic overrides (GM_DIAGNOSTICS=1 only) arrive as values: corr()
// reads the environment, this header does not.
struct CorrGridIn {
    int n_workers = 0, n_bins = 0, n_int = 0;
    int wg_per_cu = 2;        // CorrPlanOf<PL>::type::WG_PER_CU
    bool can_split = false;   // the plan has a split slab AND the handle has the scratch and the tickets (gm_acq_create: M >= 2)
    int split_planes = 0;     // power planes the scratch holds (corr_split_planes)
    bool strict_sum = false;  // gm_acq_cfg.strict_sum_order
    bool stamps = false;      // gm_acq_debug_stamps armed (diagnostic build)
    int map_forced = -1;      // GM_CORR_MAP
    int cb_env = -1;          // GM_CORR_CB
    int split_env = -1;       // GM_CORR_SPLIT
    int items_env = -1;       // GM_CORR_SPLIT_ITEMS
};

// which items of the grid are cut into one part per integration (gm_acq_corr_grid_info.cut) ...
enum CorrCut { CORR_CUT_NONE = GM_CORR_CUT_NONE, CORR_CUT_ALL = GM_CORR_CUT_ALL, CORR_CUT_TAIL = GM_CORR_CUT_TAIL };
// ... and, for CORR_CUT_NONE, the first rule that said so (gm_acq_corr_grid_info.why; 0 when the grid is cut)
enum CorrWhy {
    CORR_WHY_CUT = GM_CORR_WHY_CUT,                  // (it is cut)
    CORR_WHY_M1 = GM_CORR_WHY_M1,                    // n_int < 2: nothing to cut into
    CORR_WHY_STRICT = GM_CORR_WHY_STRICT,            // strict_sum_order keeps the sequential accumulation
    CORR_WHY_OFF = GM_CORR_WHY_OFF,                  // no slab / scratch / tickets, stamps armed, GM_CORR_SPLIT = 0 or 1
    CORR_WHY_SHARE = GM_CORR_WHY_SHARE,              // one round, but more items per XCD than tickets
    CORR_WHY_MAX_K = GM_CORR_WHY_MAX_K,              // n_int > GM_CORR_SPLIT_MAX_K
    CORR_WHY_SCRATCH = GM_CORR_WHY_SCRATCH,          // every item would be cut and the scratch does not hold share * n_int planes per XCD
    CORR_WHY_ONE_WG_ROUNDS = GM_CORR_WHY_ONE_WG_ROUNDS,   // one workgroup per CU on a grid of several rounds
    CORR_WHY_CLAMPED = GM_CORR_WHY_CLAMPED,          // split_items clamped to zero
};

struct CorrGridPlan {
    int map_mode;             // 0 equal shares, 1 whole bins per XCD, 2 whole bins + evenly split leftovers, >= 16: (cb << 4) | rows_max, the tiled walk
    int share;                // slots per XCD before the cut (the tiled walk's empty ones included)
    int slots;                // resident workgroups per XCD: 32 * wg_per_cu
    int split_from, split_k, split_items;
    int grid;                 // workgroups of the launch: 8 * (split_from + split_items * split_k)
    int cut, why;             // CorrCut, CorrWhy
};

inline CorrGridPlan corr_grid_plan(const CorrGridIn& in) {
    CorrGridPlan p{};
    const int n_workers = in.n_workers, n_bins = in.n_bins, n_int = in.n_int;
    // Tile map: whole Doppler bins per XCD (best L2 locality) unless that costs an XCD an extra round of
    // workgroups (2 x 32 resident per XCD) compared with equal shares of the item list.  Measured on configs[1]
    // geometry: P = 12: 125 -> 88 us, P = 24: 195 -> 165 us with equal shares; P = 32: whole bins 3 % faster.
    const int per_xcd_bins = ((n_bins + 7) / 8) * n_workers, per_xcd_even = (n_bins * n_workers + 7) / 8;
    const int slots = 32 * in.wg_per_cu;
    const int q = n_bins / 8, left = (n_bins - 8 * q) * n_workers;
    const int per_xcd_mixed = q * n_workers + (left + 7) / 8;
    int map_mode = ((per_xcd_bins + slots - 1) / slots > (per_xcd_even + slots - 1) / slots) ? 0 : 1;
    if (map_mode == 1 && per_xcd_mixed < per_xcd_bins) map_mode = 2;   // same locality, balanced leftovers
    if (in.map_forced >= 0) map_mode = in.map_forced;
    // GM_CORR_CB = cb (diagnostic): tiled walk of the equal shares
    const int cb = in.cb_env >= 0 ? in.cb_env : 0;
    int share = map_mode == 0 ? per_xcd_even : (map_mode == 1 ? per_xcd_bins : per_xcd_mixed);
    if (cb > 0) {
        const int rows_max = (per_xcd_even + n_workers - 2) / n_workers + 1;
        if (rows_max <= 15 && cb <= 1000) {
            map_mode = (cb << 4) | rows_max;
            share = ((n_workers + cb - 1) / cb) * rows_max * cb;       // slots per XCD, the ragged ends' empty ones included
        }
    }
    // Grid tail.  When the queue of an XCD runs dry its resident workgroups finish one by one, and the launch ends a
    // whole workgroup duration (M transforms, ~45 us alone on a CU) after the last one started: about half a duration
    // of idle slots.  The LAST items of every XCD are therefore cut into n_int parts of one integration each, enough of
    // them that every resident slot ends on a short workgroup (items * n_int ~ slots).  Measured at configs[1]:
    // 0.229 -> 0.206 ms per launch; the part count and the item count barely matter between (2, 4) and (10, 8).
    // GM_CORR_SPLIT = 0 / 1 (no cut) and GM_CORR_SPLIT_ITEMS override for diagnostics.
    int split_from = share, split_k = 1, split_items = 0;
    int cut = CORR_CUT_NONE, why = CORR_WHY_OFF;
    if (n_int < 2) why = CORR_WHY_M1;
    else if (in.strict_sum) why = CORR_WHY_STRICT;   // (strict_sum_order also keeps the reference's sequential accumulation over the integrations: no split)
    else if (!in.can_split || in.split_env == 0 || in.stamps) why = CORR_WHY_OFF;
    else if (!(share > slots || share <= GM_CORR_SPLIT_MAX_ITEMS / 8)) why = CORR_WHY_SHARE;
    if (in.can_split && in.split_env != 0 && !in.stamps && !in.strict_sum && (share > slots || share <= GM_CORR_SPLIT_MAX_ITEMS / 8)) {
        // share <= slots: the whole grid is resident at once and (for few workers, e.g. the reference's single-PRN
        // search) leaves most of the chip idle: then EVERY item is cut, which multiplies the parallelism by k
        const bool all = share <= slots;
        // one integration per part (see the kernel): k = n_int, when the scratch holds the planes
        if (n_int >= 2 && n_int <= GM_CORR_SPLIT_MAX_K && (!all || share * n_int <= in.split_planes / 8)) split_k = n_int;
        if (n_int >= 2 && split_k == 1) why = n_int > GM_CORR_SPLIT_MAX_K ? CORR_WHY_MAX_K : CORR_WHY_SCRATCH;
        // one workgroup per CU (N = 16368 ...): the cut tail does not pay on a grid of several rounds (same box, back to back:
        // 0.440 against 0.432 ms per 32-PRN launch with and without; comparisons ACROSS boxes are worthless for a
        // 2 % question — the chips differ by more); it stays for grids that fit the chip at once, where it multiplies the parallelism
        if (in.wg_per_cu == 1 && !all && in.split_env < 0) {
            if (split_k > 1) why = CORR_WHY_ONE_WG_ROUNDS;
            split_k = 1;
        }
        if (in.split_env == 1) {
            if (split_k > 1) why = CORR_WHY_OFF;
            split_k = 1;
        }
        if (split_k > 1) {
            split_items = in.items_env > 0 ? in.items_env : (all ? share : (slots + split_k - 1) / split_k);
            if (split_items > share) split_items = share;
            if (split_items > GM_CORR_SPLIT_MAX_ITEMS / 8) split_items = GM_CORR_SPLIT_MAX_ITEMS / 8;
            if (split_items * n_int > in.split_planes / 8) split_items = in.split_planes / 8 / n_int;   // one plane per integration; the scratch holds split_planes of them
            if (split_items <= 0) { split_items = 0; split_k = 1; why = CORR_WHY_CLAMPED; }
            split_from = share - split_items;
            if (split_k > 1) { cut = split_from == 0 ? CORR_CUT_ALL : CORR_CUT_TAIL; why = CORR_WHY_CUT; }
        }
    }
    p.map_mode = map_mode; p.share = share; p.slots = slots;
    p.split_from = split_from; p.split_k = split_k; p.split_items = split_items;
    p.grid = 8 * (split_from + split_items * split_k);
    p.cut = cut; p.why = why;
    return p;
}

// gm_acq_create: planes the tail split can ever use for a handle of P codes, D bins and M integrations: every item cut (small grids:
// P*D items x M planes), or per XCD one resident round of parts (64 slots; an item's M planes each) — never more than
// GM_CORR_SPLIT_MAX_SLABS (a one-PRN AcquisitionWorker handle at N = 16368 takes 290 planes = 19 MB instead of 2560 = 251 MB)
inline size_t corr_split_planes(size_t P, size_t D, size_t M) {
    size_t planes = size_t(8) * ((P * D + 7) / 8) * M;      // (the launcher deals items to the XCDs in equal shares of ceil(P*D / 8))
    const size_t tail = size_t(8) * (64 + M);
    if (planes < tail) planes = tail;
    if (planes > size_t(GM_CORR_SPLIT_MAX_SLABS)) planes = size_t(GM_CORR_SPLIT_MAX_SLABS);
    return planes;
}

// ------------------------------------------------------------------------------------ in-LDS stage C: the decode, mirrored
// Mirrors acq_corr_kernel (acq_kernels.hip) and acq_corr_ws31_kernel (acq_corr_ws31.h), which hold the same text:
//   "const int xcd = blockIdx.x & 7, wslot = blockIdx.x >> 3;" down to the end of the "if (map_mode == 0) ... else ..." chain.
struct CorrSlot { int slot, part, parts; };
// the lines "int slot = wslot, part = 0, parts = 1; if (wslot >= split_from) { ... }"
inline CorrSlot corr_decode_slot(int wslot, int split_from, int split_k) {
    CorrSlot s{wslot, 0, 1};
    if (wslot >= split_from) {
        const int h = wslot - split_from;
        s.slot = split_from + h / split_k;
        s.part = h % split_k;
        s.parts = split_k;
    }
    return s;
}
struct CorrItem { bool active; int w, d; };      // active false: the workgroup returns; w: index into worker_list
// the chain "if (map_mode == 0) {...} else if (map_mode >= 16) {...} else if (map_mode == 1) {...} else {...}"
inline CorrItem corr_decode_item(int xcd, int slot, int n_workers, int n_bins, int map_mode) {
    const CorrItem none{false, -1, -1};
    if (map_mode == 0) {          // equal contiguous share of the bin-major item list per XCD
        const int items = n_bins * n_workers, share = (items + 7) >> 3;
        const int item = xcd * share + slot;
        if (slot >= share || item >= items) return none;
        const int d = item / n_workers;
        return CorrItem{true, item - d * n_workers, d};
    } else if (map_mode >= 16) {  // equal shares as in mode 0, walked in blocks of cb workers x the share's strip of bins
        const int cb = map_mode >> 4, rows_max = map_mode & 15;
        const int items = n_bins * n_workers, share = (items + 7) >> 3;
        const int it_lo = xcd * share, it_hi = it_lo + share < items ? it_lo + share : items;
        const int d_lo = it_lo / n_workers, per_blk = rows_max * cb;
        const int blk = slot / per_blk, rem = slot - blk * per_blk, dr = rem / cb, w = blk * cb + (rem - dr * cb);
        const int item = (d_lo + dr) * n_workers + w;
        if (w >= n_workers || item < it_lo || item >= it_hi) return none;
        return CorrItem{true, w, d_lo + dr};
    } else if (map_mode == 1) {   // whole bins per XCD (bin d on XCD d % 8)
        const int d = xcd + 8 * (slot / n_workers);
        if (d >= n_bins) return none;
        return CorrItem{true, slot % n_workers, d};
    } else {                      // whole bins for the first 8*floor(D/8) bins, the leftover bins' workers split evenly
        const int q = n_bins >> 3, whole = q * n_workers;
        if (slot < whole) return CorrItem{true, slot % n_workers, xcd + 8 * (slot / n_workers)};
        const int left = (n_bins - 8 * q) * n_workers, each = (left + 7) >> 3;
        const int j = slot - whole, item = xcd * each + j;
        if (j >= each || item >= left) return none;
        return CorrItem{true, item % n_workers, 8 * q + item / n_workers};
    }
}
// where a part of a cut item meets the others: the ticket "split_counter + size_t(xcd) * split_items + (slot - split_from)" and the
// first of the item's n_int planes "item_plane0 = (size_t(xcd) * split_items + (slot - split_from)) * size_t(n_int)"
inline size_t corr_ticket_index(int xcd, int slot, int split_from, int split_items) { return size_t(xcd) * split_items + (slot - split_from); }
inline size_t corr_plane0_index(int xcd, int slot, int split_from, int split_items, int n_int) {
    return corr_ticket_index(xcd, slot, split_from, split_items) * size_t(n_int);
}

// ------------------------------------------------------------------------------------ composite stage C
struct CompGridPlan { int cb, rows_max, slots; };      // slots per XCD: the launch is 8 * slots workgroups
// cb_env: GM_COMP_CB (diagnostic: workers per block, 0: plain order), -1: unset
inline CompGridPlan comp_grid_plan(int n_workers, int n_bins, int cb_env) {
    const int items = n_workers * n_bins, share = (items + 7) / 8;
    // measured at 36 codes x 41 bins x N = 2 x 16000: plain order 0.351 ms, blocks of 4 / 8 / 12 workers 0.313 / 0.314 / 0.314,
    // blocks of 2 or 6 no gain (6 x ~5 bins is exactly the resident set: every workgroup of a round then starts a new table)
    const int cb = cb_env >= 0 ? cb_env : (n_workers > 4 ? 4 : 0);
    // bins a strip can touch: a share of `share` items starting anywhere in a row
    const int rows_max = (share + n_workers - 2) / n_workers + 1;
    const int slots = cb > 0 ? ((n_workers + cb - 1) / cb) * rows_max * cb : share;
    return CompGridPlan{cb, rows_max, slots};
}
// Mirrors comp_corr_kernel (acq_composite.hip) and comp_corr_ws_body (acq_comp_ws.h), which hold the same walk:
//   "const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;" down to "const int d = item / n_workers, p = ...".
inline CorrItem comp_decode_item(int xcd, int slot, int n_workers, int n_bins, int cb, int rows_max) {
    const CorrItem none{false, -1, -1};
    const int items = n_bins * n_workers, share = (items + 7) >> 3;
    const int it_lo = xcd * share, it_hi = it_lo + share < items ? it_lo + share : items;
    int item;
    if (cb <= 0) {
        item = it_lo + slot;
        if (slot >= share || item >= it_hi) return none;
    } else {
        const int d_lo = it_lo / n_workers, per_blk = rows_max * cb;
        const int blk = slot / per_blk, rem = slot - blk * per_blk, dr = rem / cb, w = blk * cb + (rem - dr * cb);
        item = (d_lo + dr) * n_workers + w;
        if (w >= n_workers || item < it_lo || item >= it_hi) return none;
    }
    const int d = item / n_workers;
    return CorrItem{true, item - d * n_workers, d};
}

// ------------------------------------------------------------------------------------ long path
// gm_acq_create: (worker, bin) items per slab of the inverse's intermediate: at most 128 MiB (inside the 256 MiB Infinity Cache beside
// the spectra it reads), at least one item, and a grid of at most 65535 rows of C1
inline size_t long_slab_items(size_t P, size_t D, size_t M, size_t L) {
    size_t slab = (size_t(128) << 20) / (M * L * 8);
    if (slab < 1) slab = 1;
    if (slab > P * D) slab = P * D;
    if (slab * M > 65535) slab = 65535 / M;
    return slab;
}
// Mirrors launch_long_corr (acq_long.hip): "for (uint32_t item0 = 0; item0 < items; item0 += a.slab_items) { const uint32_t n = ... }"
struct LongSlab { uint32_t item0, n; };
inline uint32_t long_slab_count(uint32_t items, uint32_t slab_items) { return slab_items ? (items + slab_items - 1) / slab_items : 0; }
inline LongSlab long_slab_at(uint32_t items, uint32_t slab_items, uint32_t k) {
    const uint32_t item0 = k * slab_items;
    return LongSlab{item0, items - item0 < slab_items ? items - item0 : slab_items};
}

}  // namespace gm
