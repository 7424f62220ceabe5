// gm_api.hip — the extern "C" boundary (include/gnss_mi355x.h) over the HIP kernels.
// Host-side scalar pieces of the reference API (code table, Doppler table construction, manager,
// loop-filter constants) are restated here in C++; everything that touches sample data runs on the GPU.
// There is no CPU fallback for the compute entries: without a device they return GM_ERR_NO_DEVICE.
#include <dlfcn.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <complex>
#include <condition_variable>
#include <mutex>
#include <string>
#include <vector>

#include "gm_internal.h"

using gm::cf;

// The diagnostic gate (gm_internal.h).  The process environment is walked ONCE, and only for the literal GM_DIAGNOSTICS=1;
// the GM_* overrides are looked up (in the same block) only when it is there.
extern char** environ;
namespace gm {
static const char* env_lookup(const char* name) {
    const size_t n = strlen(name);
    for (char** e = environ; e && *e; ++e)
        if (!strncmp(*e, name, n) && (*e)[n] == '=') return *e + n + 1;
    return nullptr;
}
int diag_int(const char* name, int dflt) {
    static const bool on = [] { const char* v = env_lookup("GM_DIAGNOSTICS"); return v && !strcmp(v, "1"); }();
    if (!on) return dflt;
    const char* v = env_lookup(name);
    return (v && *v) ? atoi(v) : dflt;
}
}  // namespace gm

namespace {

thread_local std::string g_last_error;
int g_device = -1;

int set_err(int code, const char* what) {
    g_last_error = what ? what : "";
    return code;
}
int hip_fail(hipError_t e, const char* where) {
    char buf[256];
    snprintf(buf, sizeof(buf), "%s: %s", where, hipGetErrorString(e));
    g_last_error = buf;
    return GM_ERR_HIP;
}
#define HIPC(expr)                                         \
    do {                                                   \
        hipError_t _e = (expr);                            \
        if (_e != hipSuccess) return hip_fail(_e, #expr);  \
    } while (0)

int ensure_device(int dev) {
    if (dev < 0) return set_err(GM_ERR_NO_DEVICE, "gm_init() has not selected a HIP device");
    HIPC(hipSetDevice(dev));
    return GM_OK;
}

#define PI_F 3.14159265358979323846f
const float CA_RATE = 1.023e6f, CA_LEN = 1023.0f;

// ---- C/A code: IS-GPS-200 G1/G2 generator == GPS_CA_CODE_32_PRN (gps_ca_constants.rs)
const uint16_t kG2Delay[32] = {5,   6,   7,   8,   17,  18,  139, 140, 141, 251, 252, 254, 255, 256, 257, 258,
                               469, 470, 471, 472, 473, 474, 509, 512, 513, 514, 515, 516, 859, 860, 861, 862};
struct CaTable {
    int8_t rows[32][1023];
    CaTable() {
        uint8_t g1[1023], g2[1023];
        uint16_t r1 = 0x3ff, r2 = 0x3ff;   // bit k-1 = stage k
        for (int i = 0; i < 1023; ++i) {
            g1[i] = (r1 >> 9) & 1;
            g2[i] = (r2 >> 9) & 1;
            const uint16_t f1 = ((r1 >> 2) ^ (r1 >> 9)) & 1;                                     // 3,10
            const uint16_t f2 = ((r2 >> 1) ^ (r2 >> 2) ^ (r2 >> 5) ^ (r2 >> 7) ^ (r2 >> 8) ^ (r2 >> 9)) & 1;  // 2,3,6,8,9,10
            r1 = uint16_t(((r1 << 1) | f1) & 0x3ff);
            r2 = uint16_t(((r2 << 1) | f2) & 0x3ff);
        }
        for (int p = 0; p < 32; ++p)
            for (int i = 0; i < 1023; ++i)
                rows[p][i] = (g1[i] ^ g2[(i + 1023 - kG2Delay[p]) % 1023]) ? 1 : -1;
    }
};
const CaTable& ca_table() {
    static const CaTable t;
    return t;
}

// ---- BeiDou B1I ranging codes (BASELINE configs[3]'s third constellation; the reference has no BeiDou code: SURVEY §8c5).
// BDS-SIS-ICD-B1I: a Gold code of two 11-stage LFSRs, G1(x) = 1 + x + x^7 + x^8 + x^9 + x^10 + x^11 and
// G2(x) = 1 + x + x^2 + x^3 + x^4 + x^5 + x^8 + x^9 + x^11, both started from 01010101010, truncated by one chip to 2046;
// satellite i takes G1's output XOR the modulo-2 sum of two G2 stages (phase assignment table below, PRN 1..37).
const uint8_t kB1iPhase[37][2] = {{1, 3}, {1, 4}, {1, 5}, {1, 6}, {1, 8}, {1, 9}, {1, 10}, {1, 11}, {2, 7}, {3, 4}, {3, 5}, {3, 6},
                                  {3, 8}, {3, 9}, {3, 10}, {3, 11}, {4, 5}, {4, 6}, {4, 8}, {4, 9}, {4, 10}, {4, 11}, {5, 6}, {5, 8},
                                  {5, 9}, {5, 10}, {5, 11}, {6, 8}, {6, 9}, {6, 10}, {6, 11}, {8, 9}, {8, 10}, {8, 11}, {9, 10},
                                  {9, 11}, {10, 11}};
int b1i_code(uint32_t prn, int8_t* out, uint32_t n_chips) {   // n_chips <= 2047 (2046 = the ICD's truncated code)
    if (prn < 1 || prn > 37 || n_chips > 2047) return GM_ERR_OUT_OF_RANGE;
    uint8_t g1[11], g2[11];                      // stage k at index k-1
    for (int k = 0; k < 11; ++k) g1[k] = g2[k] = uint8_t(k & 1);   // 0 1 0 1 0 1 0 1 0 1 0
    const int a = kB1iPhase[prn - 1][0] - 1, b = kB1iPhase[prn - 1][1] - 1;
    for (uint32_t i = 0; i < n_chips; ++i) {
        const uint8_t chip = g1[10] ^ g2[a] ^ g2[b];
        out[i] = chip ? -1 : 1;                  // logic 0 -> +1, logic 1 -> -1
        const uint8_t f1 = g1[0] ^ g1[6] ^ g1[7] ^ g1[8] ^ g1[9] ^ g1[10];
        const uint8_t f2 = g2[0] ^ g2[1] ^ g2[2] ^ g2[3] ^ g2[4] ^ g2[7] ^ g2[8] ^ g2[10];
        for (int k = 10; k > 0; --k) { g1[k] = g1[k - 1]; g2[k] = g2[k - 1]; }
        g1[0] = f1; g2[0] = f2;
    }
    return GM_OK;
}

size_t num_samples_per_code(float code_rate, float fs, float len) {   // ca_code.rs:13-16
    const float v = roundf(fs / (code_rate / len));
    return v > 0.0f ? size_t(v) : 0;
}

// resample a +-1 chip sequence: idx = floor((i as f32 * code_rate) / fs)  (ca_code.rs:17-22)
int resample_code(const int8_t* chips, size_t code_len, bool wrap, float code_rate, float fs, size_t n, int8_t* out) {
    for (size_t i = 0; i < n; ++i) {
        const float f = floorf((float(i) * code_rate) / fs);
        size_t ind = f > 0.0f ? size_t(f) : 0;
        if (ind >= code_len) {
            if (!wrap) return GM_ERR_OUT_OF_RANGE;   // ca_code[ind] panics in the reference
            ind %= code_len;
        }
        out[i] = chips[ind];
    }
    return GM_OK;
}

void loop_filter_new(float bw, float zeta, float gain, float* tau1, float* tau2) {   // do_tracking.rs:59-65
    const float w = bw * 8.0f * zeta / (4.0f * (zeta * zeta) + 1.0f);
    *tau1 = gain / (w * w);
    *tau2 = (2.0f * zeta) / w;
}

// HIP-event timing of the acquisition kernels on the handle's stream: a pool of event triples, one per
// gm_acq_search_dev call since timing was (re-)enabled, averaged by gm_acq_timing_summary.
struct Timing {
    static constexpr int CAP = 512;
    std::vector<hipEvent_t> ev;   // CAP * 4 events, created on first enable
    bool on = false;
    int stride = 1;               // record every stride-th search (an event record costs ~2 us of stream time)
    int calls = 0;                // searches since enable
    bool this_call = false;       // the search in flight is a recorded one (its decision event follows)
    int count = 0;                // calls recorded since enable (only the last CAP are kept)
    bool decide_valid = false;
};

}  // namespace

// device mirror of MulticastRingBuffer (functions further down)
struct gm_ring {
    int device = -1;
    cf* d_buf = nullptr;
    size_t size = 0, mask = 0;
    // single writer / many readers like the reference ring: the writer publishes `head` (release) after its
    // synchronous H2D copy, readers load it (acquire) before launching kernels on the mirror
    std::atomic<uint64_t> head{0};
    // `notifier` + `condvar` of the reference ring (multicast_ring_buffer.rs:42-43,95-98): gm_ring_wait_head sleeps here
    std::mutex notifier;
    std::condition_variable condvar;
    // asynchronous writer (gm_ring_write_samples_async): pinned staging slots, a copy stream, and `head` published once the copy
    // has landed.  Published by PULL: every chunk leaves an entry {event, head after it} in `pending`; whoever looks at the head
    // (gm_ring_get_head / _wait_head / the stage entries that snapshot the ring) first retires the entries whose events have
    // completed (ring_refresh_head).  Round 4 published from a hipLaunchHostFunc callback on the copy stream: the runtime's
    // callback thread wakes up milliseconds late now and then, and the stream — hence the next block's copy and front-end kernel
    // — waits behind the callback (7-9 ms stalls every five or six blocks of the receiver loop, tools/trk_async_probe.py).
    static constexpr int SLOTS = 4;
    static constexpr size_t SLOT_SAMPLES_MAX = size_t(1) << 19;      // 32 ms at 16.4 Msps: one copy + one front-end launch per block of that size (the
                                                                     // front-end kernel's fixed ~45 us weigh 15 % on a 2^18 block, 8 % on this one)
    size_t slot_samples = 0;                                        // min(ring size, SLOT_SAMPLES_MAX), set at create
    cf* staging[SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t slot_done[SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    bool slot_used[SLOTS] = {false, false, false, false};
    hipStream_t copy_stream = nullptr;
    // gm_frontend_write_ring: the front-end kernels run on a stream of their own behind the copies (event per slot), so the copy
    // of block k + 1 travels while the kernel of block k runs
    hipStream_t fe_stream = nullptr;
    hipEvent_t h2d_done[SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    hipStream_t last_enq_stream = nullptr;       // the stream ev_enq was last recorded on (see ring_end_block)
    uint64_t write_pos = 0;       // writer-private: samples enqueued so far (>= head)
    uint64_t slot_seq = 0;
    struct Pending { int slot; uint64_t new_head; };
    std::mutex pend_mu;
    std::vector<Pending> pending;           // FIFO, at most SLOTS entries (a slot is re-used only after its entry has been retired)
    // what the writer has ENQUEUED on copy_stream so far, and an event recorded there behind it: a consumer that must not wait on
    // the host (gm_trk_update_all_async) orders its own stream behind `ev_enq` on the DEVICE and may then use `enqueued` as its head
    // — the device-side counterpart of the Condvar wait of do_tracking::run (do_tracking.rs:392-406).  enq_mu: writer and
    // consumer may be different host threads; the pair (enqueued, ev_enq) is read and written under it.
    std::mutex enq_mu;
    hipEvent_t ev_enq = nullptr;
    uint64_t enqueued = 0;
    bool ev_enq_armed = false;
};

// Wait for an event the way a latency path wants it: poll (hipEventQuery) for up to ~2 ms before handing over to the runtime's blocking
// wait.  hipEventSynchronize's wake-up through the interrupt path costs milliseconds on this platform when the event is already (or
// almost) complete — measured 7-9 ms per wait in the receiver loop, against the ~0.3 ms the awaited front-end block takes
// (tools/trk_async_probe.py) — and the device idles meanwhile, because the host is what feeds it.
static hipError_t wait_event_polling(hipEvent_t ev) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipEventQuery(ev);
        if (q != hipErrorNotReady) return q;
        (void)hipGetLastError();
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) return hipEventSynchronize(ev);
    }
}

// head := max(head, new_head), never backwards: readers and the writer may retire chunks concurrently (head by pull), and a
// plain store after a stale load would let the older of two retirements land last.  compare-exchange max loop, then the wake-up.
static void ring_publish(gm_ring* r, uint64_t new_head) {
    uint64_t cur = r->head.load(std::memory_order_relaxed);
    bool moved = false;
    while (int64_t(new_head - cur) > 0) {
        if (r->head.compare_exchange_weak(cur, new_head, std::memory_order_release, std::memory_order_relaxed)) { moved = true; break; }
    }
    if (!moved) return;
    std::lock_guard<std::mutex> g(r->notifier);     // "Wake up Tracking after writing new samples" (:94-98)
    r->condvar.notify_all();
}
// retire the chunks whose copies (and front-end kernels) have run: head := the newest completed one.  Any host thread; the
// ring's device must be current.  `all`: the copy stream has just been synchronised — everything is complete.
static void ring_refresh_head(gm_ring* r, bool all = false) {
    if (!r->copy_stream) return;
    uint64_t newest = 0;
    bool any = false;
    {
        std::lock_guard<std::mutex> g(r->pend_mu);
        size_t done = 0;
        while (done < r->pending.size()) {
            if (!all) {
                const hipError_t q = hipEventQuery(r->slot_done[r->pending[done].slot]);
                if (q != hipSuccess) { (void)hipGetLastError(); break; }
            }
            newest = r->pending[done].new_head; any = true; ++done;
        }
        if (done) r->pending.erase(r->pending.begin(), r->pending.begin() + done);
    }
    if (any) ring_publish(r, newest);               // monotonic by construction (two readers retiring at once: ADVICE round 5)
}
static int ring_async_init(gm_ring* r) {
    if (r->copy_stream) return GM_OK;
    {   // The writer's copies at the device's LOWEST stream priority, the front-end kernels (gm_frontend_write_ring) at the HIGHEST: HIP deals
        // streams of one priority to that priority's hardware queues in creation order, and the normal-priority ones are where every other
        // stream of the process lives (a first torch.cuda.Stream() creates 32 of them).  With both at the default priority the receiver
        // chain ran at 218 x real time in a clean process and at 117 x behind four torch streams; low / high: 218 / 216 / 212 x with 0 / 4 / 16
        // of them (tools/rx_order_probe.py, DESIGN_HISTORY R6.12).  GM_RING_COPY_PRIORITY / GM_RING_FE_PRIORITY: diagnostic overrides.
        int least = 0, greatest = 0;
        HIPC(hipDeviceGetStreamPriorityRange(&least, &greatest));
        const int pr = gm::diag_int("GM_RING_COPY_PRIORITY", 99);
        HIPC(hipStreamCreateWithPriority(&r->copy_stream, hipStreamNonBlocking, pr == 99 ? least : pr));
    }
    for (int i = 0; i < gm_ring::SLOTS; ++i) {
        HIPC(hipHostMalloc(reinterpret_cast<void**>(&r->staging[i]), r->slot_samples * 8, hipHostMallocDefault));
        HIPC(hipEventCreateWithFlags(&r->slot_done[i], hipEventDisableTiming));
    }
    r->write_pos = r->head.load(std::memory_order_relaxed);
    return GM_OK;
}
// The stream the ring writers' kernels run on, and the events that order it behind the copies (see struct gm_ring).  At the device's
// HIGHEST priority: see ring_async_init.
static int ring_fe_init(gm_ring* r) {
    if (r->fe_stream) return GM_OK;
    if (gm::diag_int("GM_RING_FE_STREAM", 1) == 0) r->fe_stream = r->copy_stream;      // diagnostic: kernels on the copy stream (round 4's form)
    else {
        int least = 0, greatest = 0;
        HIPC(hipDeviceGetStreamPriorityRange(&least, &greatest));
        const int pr = gm::diag_int("GM_RING_FE_PRIORITY", 99);
        HIPC(hipStreamCreateWithPriority(&r->fe_stream, hipStreamNonBlocking, pr == 99 ? greatest : pr));
    }
    for (int i = 0; i < gm_ring::SLOTS; ++i) HIPC(hipEventCreateWithFlags(&r->h2d_done[i], hipEventDisableTiming));
    return GM_OK;
}
// The next staging slot, about to be re-used: its previous chunk must have run — and is retired first (its entry names the slot's event)
static int ring_begin_block(gm_ring* r, int* slot) {
    *slot = int(r->slot_seq++ % gm_ring::SLOTS);
    if (!r->slot_used[*slot]) return GM_OK;
    HIPC(wait_event_polling(r->slot_done[*slot]));
    ring_refresh_head(r);
    return GM_OK;
}
// The work of one chunk (staging slot `slot`, `cnt` samples at write_pos) has been enqueued on `st` (copy_stream or fe_stream): its event,
// the writer's position, and the entry that publishes the head once the event has completed
static int ring_end_block(gm_ring* r, int slot, hipStream_t st, uint64_t cnt) {
    HIPC(hipEventRecord(r->slot_done[slot], st));
    r->slot_used[slot] = true;
    r->write_pos += cnt;
    {
        std::lock_guard<std::mutex> g(r->pend_mu);
        r->pending.push_back(gm_ring::Pending{slot, r->write_pos});
    }
    {   // the enqueued head and its event (see struct gm_ring): "everything enqueued so far" — when the writer changes streams
        // (plain copies and front-end blocks on one ring), the new stream first waits for what the event covered before
        std::lock_guard<std::mutex> g(r->enq_mu);
        if (!r->ev_enq) HIPC(hipEventCreateWithFlags(&r->ev_enq, hipEventDisableTiming));
        if (r->ev_enq_armed && r->last_enq_stream != st) HIPC(hipStreamWaitEvent(st, r->ev_enq, 0));
        r->last_enq_stream = st;
        HIPC(hipEventRecord(r->ev_enq, st));
        r->enqueued = r->write_pos;
        r->ev_enq_armed = true;
    }
    return GM_OK;
}
// The block loop of every writer that runs kernels behind the copy: `n` samples of `bps` bytes each, at most `block` a step.  A step
// stages its bytes in the next pinned slot, copies them on copy_stream into the caller's landing zone raw[slot] (raw_bytes each,
// allocated on first use), and makes fe_stream wait for that copy; `stage(d_raw, chunk, &cnt)` then enqueues the block's kernels on
// fe_stream, the last of them writing `cnt` samples into the ring at write_pos.
template <class Stage>
static int ring_write_blocks(gm_ring* r, const void* samples, size_t n, size_t bps, size_t block, void** raw, size_t raw_bytes, Stage&& stage) {
    const uint8_t* src = static_cast<const uint8_t*>(samples);
    while (n) {
        const size_t chunk = n < block ? n : block;
        int slot = 0;
        if (int rc = ring_begin_block(r, &slot)) return rc;
        if (!raw[slot]) HIPC(hipMalloc(&raw[slot], raw_bytes));
        memcpy(r->staging[slot], src, chunk * bps);
        // (the kernel reading the pinned staging slot itself instead of a device copy of it — no copy, no event — was measured:
        //  30 x real time against 52: the front-end's loads then wait on host memory)
        HIPC(hipMemcpyAsync(raw[slot], r->staging[slot], chunk * bps, hipMemcpyHostToDevice, r->copy_stream));
        HIPC(hipEventRecord(r->h2d_done[slot], r->copy_stream));
        HIPC(hipStreamWaitEvent(r->fe_stream, r->h2d_done[slot], 0));
        uint64_t cnt = 0;
        if (int rc = stage(raw[slot], chunk, &cnt)) return rc;
        if (int rc = ring_end_block(r, slot, r->fe_stream, cnt)) return rc;
        src += chunk * bps; n -= chunk;
    }
    return GM_OK;
}

// ====================================================================== per-call device blocks: what the known-cell entries share
// gm_acq_refine_doppler, gm_acq_local_search, gm_acq_array_prompts, gm_acq_cancel, gm_trk_bank and gm_trk_array_prompts each run a small
// kernel at cells the caller names and return host results synchronously.  Each keeps ONE grow-only device block on its handle and
// carves it per call.  Here: the block, the carve, and the two pieces of host arithmetic more than one of them uses.  What needs a
// handle's fields sits in front of the entries that use it ("known cells on gm_acq", "known records on gm_trk").
// An entry supplies its rules, its carve, its launch and its result loop.
static size_t round256(size_t b) { return (b + 255) & ~size_t(255); }
struct CallBlock {
    void* d = nullptr;
    size_t bytes = 0;
    // room for `total` bytes: the new block before the old one goes, so a failure leaves the handle as it was
    int reserve(hipStream_t stream, size_t total, const char* nomem_text) {
        if (total <= bytes) return GM_OK;
        void* blk = nullptr;
        if (hipMalloc(&blk, total) != hipSuccess) {
            (void)hipGetLastError();
            return set_err(GM_ERR_NOMEM, nomem_text);
        }
        if (d)                                 // (nothing can be in flight on a block that does not exist yet)
            if (hipError_t e = hipStreamSynchronize(stream); e != hipSuccess) { hipFree(blk); return hip_fail(e, "hipStreamSynchronize"); }
        hipFree(d);
        d = blk; bytes = total;
        return GM_OK;
    }
    void release() { hipFree(d); d = nullptr; bytes = 0; }
};
// the parts of a block in the order they are taken, each 256-byte aligned; `end` is the block's size so far
struct Carve {
    size_t end = 0;
    size_t take(size_t b) { const size_t at = end; end += round256(b); return at; }
};
static size_t fmt_bytes(int fmt) { return fmt == GM_FMT_C32 ? 8 : (fmt == GM_FMT_I8_IQ ? 2 : 1); }     // per sample, of the three formats
// the vertex of the parabola through (-1, y0), (0, y1), (1, y2), in grid steps, f64; 0 where y1 is no strict maximum; clamped to half a step
static double parabola_offset(double y0, double y1, double y2) {
    const double den = y0 - 2.0 * y1 + y2;
    const double x = den < 0.0 ? 0.5 * (y0 - y2) / den : 0.0;
    return x > 0.5 ? 0.5 : (x < -0.5 ? -0.5 : x);
}

// ====================================================================== acquisition handle
struct gm_acq {
    int device = -1;
    gm_acq_cfg cfg{};
    const gm::PlanOps* plan = nullptr;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    uint32_t N = 0, D = 0, M = 0, P = 0;
    uint32_t K = 1;                        // gm_acq_cfg.coherent_periods (0 -> 1): a dwell is K * M periods, M groups of K folded coherently
    cf* d_rho = nullptr;                   // [D][K] the fold's phasor words (gm_acq_coherent_phasors)
    gm::StageFLaunch coh_fwd = nullptr;    // K >= 2: stage F of this handle's form (acq_stage_f_variants.h)
    // gm_acq_set_edge_search (K >= 2): H hypotheses about where the groups start, each with the secondary row's signs in the fold
    // (EdgeLoad, acq_stage_f_variants.h).  Stage F writes the spectra [H * D][M][.], stage C runs with H * D bins into `d_full`, the
    // reduction picks a hypothesis per (worker, bin) cell into the ordinary metrics block and `d_choice`.  All buffers are the edge
    // search's own: the handle's are untouched, so switching it off (H = 0) is the handle as it was.
    struct Edge {
        uint32_t H = 0;                    // 0: off
        std::vector<uint32_t> offsets;     // [H] ascending period offsets
        uint32_t o_max = 0, neg = 0;       // offsets[H - 1]; bit k set: secondary[k] = -1
        uint32_t* d_offsets = nullptr;
        cf* d_spectra = nullptr;           // [H * D][M][L or N]
        cf* d_tmp = nullptr;               // composite sizes whose forward step 2 runs per dwell: the sub-transforms [H * D * M][N]
        uint32_t* d_full = nullptr;        // [3][P][H][D] metric words of every hypothesis (gm_acq_edge_metrics)
        uint32_t* d_choice = nullptr;      // [P][D] the hypothesis each cell of the last search chose (gm_acq_edge_choice)
        float* d_long_part = nullptr;      // any-length sizes: [3][P * H * D][Q] partials
        float* d_planes = nullptr;         // strict_sum_order on composite / any-length sizes: [P * H * D][N] power planes
        gm::StageFLaunch fwd = nullptr;    // stage F of this handle's form
    } edge;
    // gm_acq_set_code_drift: per-bin true code periods T_d; period p of the dwell starts at floor(p T_d + 0.5) in bin d and stage F
    // reads it from there (DriftLoad, acq_stage_f_variants.h) into the spectrum buffer the handle (or its edge search) has anyway.
    // Re-planned whenever the edge search changes (R = K M + the last offset).
    struct Drift {
        bool on = false;
        std::vector<double> T;             // [D]
        uint32_t R = 0;                    // periods of the dwell
        std::vector<uint64_t> starts;      // [D][R]
        uint64_t dwell = 0;                // max_d starts[d][R - 1] + N samples
        uint64_t* d_starts = nullptr;      // [D][R]
        cf* d_rho = nullptr;               // [max(H, 1)][D][M][K] phasor words continued to the real starts (no secondary signs)
        gm::StageFLaunch fwd = nullptr;    // stage F of this handle's form
    } drift;
    float code_rate = CA_RATE;
    std::vector<float> table_freq;
    std::vector<uint8_t> prn_ids, dev_prn_ids;
    cf* d_tw_mix = nullptr;       // forward base twiddles of stage F's own plan (PlanOps::fill_tw_mix)
    cf *d_tables = nullptr, *d_tw_fwd = nullptr, *d_tw_inv = nullptr, *d_code_fft = nullptr, *d_spectra = nullptr;
    cf* d_code_fft_paired = nullptr;   // Q == 1: the code spectra in the layout acq_corr_kernel reads (PairLayout)
    uint16_t* d_order = nullptr;       // Q == 1, permuted storage orders: element index stored at each position (PlanOps::fill_order)
    float* d_table_freq = nullptr;
    int8_t* d_code_samples = nullptr;
    void* d_samples = nullptr;
    size_t samples_cap = 0;
    uint32_t* d_metrics = nullptr;         // [3][P][D] words
    uint32_t* d_worker_list = nullptr;
    std::vector<uint32_t> worker_list;
    uint64_t mask = ~0ull;
    uint32_t n_workers = 0;
    gm_acq_result* d_results = nullptr;
    uint8_t *d_found = nullptr, *d_prn_ids = nullptr;
    uint32_t results_cap = 0;
    const void* last_metrics = nullptr;
    Timing tm;
    // composite transform size N = Q * plan->n (acq_composite.hip); Q == 1: the fused single-LDS-buffer kernels
    float* d_split_scratch = nullptr;      // partial power planes of the correlation grid's tail split
    int split_planes = 0;                  // ... how many of them the scratch holds (sized from the handle's geometry at create)
    uint32_t* d_split_counter = nullptr;   // arrival tickets, one per split item, zero between launches
    gm_acq_corr_grid_info last_grid{};     // the grid of the last stage-C launch, written by the launcher (gm_acq_debug_corr_grid)
    uint32_t Q = 1, Nb = 0;
    const gm::CompOps* comp = nullptr;     // Q > 1: the (Q, base plan) kernels
    cf* d_comp_tmp = nullptr;              // [max(D*M, P)][Q][Nb]: forward sub-transforms before the Q-point DFTs
    cf* d_comp_twn = nullptr;              // [Q][Nb] inverse twiddles W_N^{-n1 k2}, paired positions
    float* d_planes = nullptr;             // composite sizes with strict_sum_order: the accumulated power planes [P * D][N] (launch_plane_strict_sum)
    cf* d_code_comb = nullptr;             // Q > 1: [P][Q][Q][Nb] conj(code) x W_Q^{-n1 k1} x W_N^{-n1 k2}, what comp corr multiplies the spectra by
    // any-length sizes (gm_acq_cfg.any_length, acq_long.hip): transform length L = Q * Nb (L = N native, L >= 2N padded); Q may be 1
    const gm::LongOps* lng = nullptr;
    uint32_t L = 0, long_lim = 0, long_slab = 0;   // L; the signal's extension (N native, 2N padded); (worker, bin) items per slab
    float long_scale = 1.0f;               // (N / L)^2
    cf* d_long_code = nullptr;             // [P][L] natural code spectra (native: d_code_fft itself)
    cf* d_long_z = nullptr;                // [long_slab][M][L] the inverse's intermediate
    float* d_long_part = nullptr;          // [3][P * D][Q] partial {max, argmax, sum}
    // gm_acq_decide_dev on the metrics of the last search, on a handle of an in-LDS size: the decision is NOT launched but kept here
    // and rides along with the next search's stage F (PlanOps::mix_fft: trailing workgroups) — anything else that consumes or
    // invalidates it (fetch, synchronize, another decide, a stream change, timing) launches decide_kernel first (acq_flush_decision)
    // gm_acq_prepare_dev: stage F of the NEXT dwell on a stream of the handle's own into a second spectrum buffer.  d_spectra is
    // the buffer the next in-stream stage F writes / the last stage C read; d_spectra_alt the other one, whose last reader is an
    // EARLIER stage C than the most recent one.  ev_s: recorded on the handle's stream just in front of every stage C launch — a
    // preparation that waits for it starts together with the most recent stage C (every earlier one has ended by then) and, at the
    // lowest priority, gets the CUs that stage C no longer needs
    // A preparation is named by a TOKEN (a generation number, never 0), not by the address of the samples it was made from: a
    // ring-backed receiver reuses addresses by construction, and a search that matched on the pointer would silently take the OLD
    // samples' spectra.  Only gm_acq_search_prepared_dev(token) consumes it.
    struct Ahead {
        cf* d_spectra_alt = nullptr;
        hipStream_t side = nullptr;
        hipEvent_t ev_s = nullptr, ev_f = nullptr, ev_in = nullptr;   // ev_in: the caller's `ready_stream` at the time of the call
        bool valid = false;                 // d_spectra_alt holds (or will hold: ev_f) the spectra of the preparation `token`
        uint64_t token = 0, next_token = 1;
        const void* samples = nullptr;      // composite sizes only (nothing is prepared: the search runs from these at search_prepared)
        int fmt = 0;
        bool comp_wait = false;             // composite sizes: ev_in was recorded on the caller's ready_stream, the search waits for it
    } ahead;
    bool defer_decisions = false;   // gm_acq_set_deferred_decision
    bool dec_deferred = false;
    gm::DecideArgs dec_args{};
    bool comp_post_folded = false;         // ... and, for base plans with an order table, the signal's forward step 2 (CompOps::fold_post): d_spectra = the sub-transforms
    // fine Doppler (gm_acq_finer_doppler): host copy of the chip rows, lazily built device state
    std::vector<int8_t> chips;             // [P][code_len]
    uint32_t code_len = 1023;
    const void* last_samples = nullptr;    // device snapshot of the last search
    int last_fmt = GM_FMT_C32;
    struct Fine {
        const gm::PlanOps *p1 = nullptr, *p2 = nullptr;
        uint32_t size_use = 0, sats_cap = 0;
        int8_t* d_chips = nullptr;
        cf *d_tw1 = nullptr, *d_tw2 = nullptr, *d_B = nullptr;
        float *d_mean = nullptr, *d_rowmax = nullptr, *d_peak_pow = nullptr;
        uint32_t *d_rowarg = nullptr, *d_sat_worker = nullptr, *d_sat_cp = nullptr, *d_peak_idx = nullptr;
    } fine;
    // the known-cell entries' device blocks, one each: gm_acq_refine_doppler (the satellite list, the prompts, the period times, the
    // per-satellite centre and step, the spectra and the peaks), gm_acq_local_search, gm_acq_array_prompts (the candidates and z) and
    // gm_acq_cancel (candidate constants, the segment tables o and b, the amplitudes)
    CallBlock refine, local, array, cancel;
    int8_t* d_cancel_chips = nullptr;      // gm_acq_cancel: a device copy of the raw chip rows [P][code_len], uploaded at the first call
};

// the fused single-LDS-buffer kernels (acq_kernels.hip): neither a composite nor an any-length size
static bool acq_fused(const gm_acq* a) { return a->Q == 1 && !a->lng; }

// stage F of one of the three variant families (Load: gm::CohLoad, gm::EdgeLoad, gm::DriftLoad) for this handle's form; null: no such plan
template <class Load> static gm::StageFLaunch acq_find_stage_f(const gm_acq* a) {
    return a->lng ? gm::find_stage_f<Load>(gm::STAGE_F_LONG, a->lng->nb)
                  : (a->Q == 1 ? gm::find_stage_f<Load>(gm::STAGE_F_MIX, a->plan->n) : gm::find_stage_f<Load>(gm::STAGE_F_COMP, a->comp->nb));
}
// code periods one dwell holds: K * M, plus the last offset while the edge search is on
static size_t acq_dwell_periods(const gm_acq* a) { return size_t(a->K) * a->M + (a->edge.H ? a->edge.o_max : 0u); }
static void acq_edge_free(gm_acq::Edge& e) {
    hipFree(e.d_offsets); hipFree(e.d_spectra); hipFree(e.d_tmp); hipFree(e.d_full); hipFree(e.d_choice); hipFree(e.d_long_part);
    hipFree(e.d_planes);
    e = gm_acq::Edge{};
}
static void acq_drift_free(gm_acq::Drift& d) {
    hipFree(d.d_starts); hipFree(d.d_rho);
    d = gm_acq::Drift{};
}
// samples one dwell holds (gm_acq_dwell_samples): the periods back to back, or up to the end of the last compensated period
static size_t acq_dwell_samples(const gm_acq* a) { return a->drift.on ? size_t(a->drift.dwell) : acq_dwell_periods(a) * a->N; }

static int acq_set_mask(gm_acq* a, uint64_t mask) {
    std::vector<uint32_t> wl;
    for (uint32_t i = 0; i < a->P; ++i)
        if (i >= 64 || ((mask >> i) & 1ull)) wl.push_back(i);
    a->mask = mask;
    if (wl != a->worker_list || a->n_workers != wl.size()) {
        a->worker_list = wl;
        a->n_workers = uint32_t(wl.size());
        if (!wl.empty())
            HIPC(hipMemcpyAsync(a->d_worker_list, a->worker_list.data(), wl.size() * sizeof(uint32_t),
                                hipMemcpyHostToDevice, a->stream));
        HIPC(hipStreamSynchronize(a->stream));
    }
    return GM_OK;
}

// decide_kernel stages a code's 3 * n_bins words in dynamic LDS (launch_decide: 12 bytes per bin of the 64 KB one workgroup may ask for):
// every entry that reaches it with a caller's n_bins refuses more on the host instead of handing the runtime a launch it rejects
static_assert(size_t(GM_ACQ_DECIDE_MAX_BINS) * 12 <= 65536 && size_t(GM_ACQ_DECIDE_MAX_BINS + 1) * 12 > 65536, "the limit the header states");
static const char* const DECIDE_BINS_MSG = "n_bins above GM_ACQ_DECIDE_MAX_BINS = 5461 (the decision stages 12 bytes per bin in 64 KB of LDS)";

static int acq_flush_decision(gm_acq* a) {
    if (a->dec_deferred) {
        a->dec_deferred = false;
        gm::launch_decide(a->stream, a->dec_args);
        HIPC(hipGetLastError());
    }
    return GM_OK;
}

static int acq_reserve_results(gm_acq* a, uint32_t n) {
    if (n <= a->results_cap) return GM_OK;
    if (int rc = acq_flush_decision(a)) return rc;
    // results + found flags live in ONE host-pinned, device-visible block: decide_kernel writes its P x 41 bytes straight into
    // host memory and gm_acq_fetch_results is a stream synchronisation and a memcpy — the two device-to-host copies it used to
    // issue cost the host-buffer entry (gm_acq_search) ~25 us per dwell
    // (the new blocks are allocated BEFORE the old ones go: a failed allocation leaves the handle as it was)
    void* blk = nullptr;
    uint8_t* ids = nullptr;
    HIPC(hipHostMalloc(&blk, (sizeof(gm_acq_result) + 1) * size_t(n), hipHostMallocDefault));
    if (hipError_t e = hipMalloc(&ids, n); e != hipSuccess) { hipHostFree(blk); return hip_fail(e, "hipMalloc(prn ids)"); }
    if (a->d_results) {
        if (hipError_t e = hipStreamSynchronize(a->stream); e != hipSuccess) { hipHostFree(blk); hipFree(ids); return hip_fail(e, "hipStreamSynchronize"); }
        hipHostFree(a->d_results);
        hipFree(a->d_prn_ids);
    }
    a->dev_prn_ids.clear();
    a->d_results = static_cast<gm_acq_result*>(blk);
    a->d_found = reinterpret_cast<uint8_t*>(a->d_results + n);
    a->d_prn_ids = ids;
    a->results_cap = n;
    return GM_OK;
}

// ---------------------------------------------------------------- known cells on gm_acq: what gm_acq_refine_doppler, gm_acq_local_search,
// gm_acq_array_prompts and gm_acq_cancel share beyond CallBlock and Carve
namespace {
struct RefinePlan { uint32_t J = 0, G = 0, Z = 0; double half_span = 0.0, step = 0.0; };
// the fine-Doppler grid of a cell list: host copies the result loops read, and where the kernels find them
struct CellGrid { std::vector<double> t, fc, step; const double *d_t = nullptr, *d_fc = nullptr, *d_step = nullptr; };
}
// these samples, or the snapshot of the last search
static int acq_call_input(const gm_acq* a, const void* d_samples, int fmt, const void** in, int* in_fmt) {
    if (d_samples) {
        if (fmt < GM_FMT_C32 || fmt > GM_FMT_I8_REAL) return set_err(GM_ERR_INVALID_ARG, "bad sample format");
    } else if (!a->last_samples) return set_err(GM_ERR_INVALID_ARG, "no search has run on this handle yet");
    *in = d_samples ? d_samples : a->last_samples;
    *in_fmt = d_samples ? fmt : a->last_fmt;
    return GM_OK;
}
// the rules of a known cell (gm_acq_cand), shared by gm_acq_local_search and gm_acq_array_prompts
static int acq_cand_rules(const gm_acq* a, const gm_acq_cand& c) {
    if (c.worker >= a->P) return set_err(GM_ERR_INVALID_ARG, "candidate.worker outside the handle's workers");
    if (c.doppler_bin < 0 || uint32_t(c.doppler_bin) >= a->D) return set_err(GM_ERR_INVALID_ARG, "candidate.doppler_bin outside the handle's bins");
    if (c.code_phase_samples >= a->N) return set_err(GM_ERR_INVALID_ARG, "candidate.code_phase_samples >= fft_size");
    if (c.offset_periods > (a->edge.H ? a->edge.o_max : 0u))
        return set_err(GM_ERR_INVALID_ARG, "candidate.offset_periods above the edge search's last offset (0 without an edge search)");
    return GM_OK;
}
static gm::RefineSat acq_cand_cell(const gm_acq_cand& c) {
    return gm::RefineSat{c.worker, c.code_phase_samples, uint32_t(c.doppler_bin), c.offset_periods};
}
// the period times of every group of every cell (f64, relative to the group's first period: whole samples over fs; the code-drift
// starts while they are on) and the cells' centre frequencies, beside the caller's g.step; all three uploaded to d_t, d_fc, d_step
static int acq_cell_grid(const gm_acq* a, const std::vector<gm::RefineSat>& cells, uint32_t J, uint32_t G, char* d_t, char* d_fc, char* d_step,
                         CellGrid& g) {
    const uint32_t S = uint32_t(cells.size()), R_u = J * G, N = a->N;
    const double fs = double(a->cfg.fs);
    g.t.resize(size_t(S) * R_u); g.fc.resize(S);
    for (uint32_t i = 0; i < S; ++i) {
        const uint32_t d = cells[i].bin, o = cells[i].offset;
        g.fc[i] = double(a->table_freq[d]);
        for (uint32_t gi = 0; gi < G; ++gi)
            for (uint32_t k = 0; k < J; ++k) {
                const uint32_t q0 = o + gi * J, q = q0 + k;
                const uint64_t s0 = a->drift.on ? a->drift.starts[size_t(d) * a->drift.R + q0] : uint64_t(q0) * N;
                const uint64_t s1 = a->drift.on ? a->drift.starts[size_t(d) * a->drift.R + q] : uint64_t(q) * N;
                g.t[size_t(i) * R_u + gi * J + k] = double(s1 - s0) / fs;
            }
    }
    HIPC(hipMemcpyAsync(d_t, g.t.data(), g.t.size() * 8, hipMemcpyHostToDevice, a->stream));
    HIPC(hipMemcpyAsync(d_fc, g.fc.data(), size_t(S) * 8, hipMemcpyHostToDevice, a->stream));
    HIPC(hipMemcpyAsync(d_step, g.step.data(), size_t(S) * 8, hipMemcpyHostToDevice, a->stream));
    g.d_t = reinterpret_cast<const double*>(d_t); g.d_fc = reinterpret_cast<const double*>(d_fc);
    g.d_step = reinterpret_cast<const double*>(d_step);
    return GM_OK;
}
// the fields gm::RefineArgs, gm::LocalArgs and gm::ArrayArgs share ...
template <class Args> static void acq_cell_args(Args& g, const gm_acq* a, const void* in, int in_fmt, uint32_t R_u) {
    g.samples = in; g.fmt = in_fmt;
    g.starts = a->drift.on ? a->drift.d_starts : nullptr; g.R = a->drift.on ? a->drift.R : 0u;
    g.tables = a->d_tables; g.code_samples = a->d_code_samples;
    g.N = a->N; g.R_u = R_u;
}
// ... and those of the two with a fine-Doppler grid
template <class Args> static void acq_grid_args(Args& g, const gm_acq* a, const RefinePlan& p, cf* z, const CellGrid& cg) {
    g.J = p.J; g.G = p.G; g.Z = p.Z;
    g.neg = (a->K >= 2 && a->edge.H) ? a->edge.neg : 0u;
    g.z = z; g.t = cg.d_t; g.fc = cg.d_fc; g.step = cg.d_step;
}

extern "C" {

int gm_abi_version(void) { return GM_ABI_VERSION; }

int gm_device_count(int* count) {
    if (!count) return set_err(GM_ERR_INVALID_ARG, "count is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return hip_fail(e, "hipGetDeviceCount"); }
    *count = n;
    return GM_OK;
}

int gm_init(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return set_err(GM_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n) return set_err(GM_ERR_INVALID_ARG, "device index out of range");
    HIPC(hipSetDevice(device));
    g_device = device;
    return GM_OK;
}

const char* gm_last_error(void) { return g_last_error.c_str(); }

const char* gm_status_string(int s) {
    switch (s) {
        case GM_OK: return "ok";
        case GM_ERR_INVALID_ARG: return "invalid argument";
        case GM_ERR_UNSUPPORTED_N: return "no FFT plan for this fft_size";
        case GM_ERR_NO_DEVICE: return "no HIP device";
        case GM_ERR_HIP: return "HIP runtime error";
        case GM_ERR_OUT_OF_RANGE: return "index out of range";
        case GM_ERR_ALIGNMENT: return "fft_size must be a multiple of 8";
        case GM_ERR_NOMEM: return "out of memory";
        default: return "unknown status";
    }
}

// ---------------------------------------------------------------- code table / Doppler table (host)
int gm_b1i_code(uint32_t prn, int8_t* out_chips, uint32_t n_chips) {
    if (!out_chips) return set_err(GM_ERR_INVALID_ARG, "null out");
    if (int rc = b1i_code(prn, out_chips, n_chips)) return set_err(rc, "B1I PRN 1..37, at most 2047 chips");
    return GM_OK;
}

int gm_ca_code_row(int row, int8_t out[1023]) {
    if (row < 0 || row > 31 || !out) return set_err(GM_ERR_OUT_OF_RANGE, "row must be 0..31");
    memcpy(out, ca_table().rows[row], 1023);
    return GM_OK;
}

int gm_generate_ca_code_samples(uint8_t prn, float code_rate, float fs, int8_t* out, size_t cap, size_t* n_out) {
    if (prn < 1 || prn > 32) return set_err(GM_ERR_OUT_OF_RANGE, "prn must be 1..=32");
    const size_t n = num_samples_per_code(code_rate, fs, CA_LEN);
    if (n_out) *n_out = n;
    std::vector<int8_t> tmp(n);
    const int rc = resample_code(ca_table().rows[prn - 1], 1023, false, code_rate, fs, n, tmp.data());
    if (rc) return set_err(rc, "chip index reached 1023 (the reference panics)");
    if (out) memcpy(out, tmp.data(), n < cap ? n : cap);
    return GM_OK;
}

int gm_doppler_table_new(float f_if, float doppler_hz, float fs, size_t n, float* freq_out, gm_c32* table) {
    if (!table && n) return set_err(GM_ERR_INVALID_ARG, "table_out is null");
    const float carr_freq = f_if + doppler_hz;               // doppler_shift.rs:13
    const float phase_step = 2.0f * PI_F * carr_freq / fs;   // :14
    for (size_t i = 0; i < n; ++i) {
        const float phase = float(i) * phase_step;           // :17
        table[i].re = cosf(phase);                           // :18
        table[i].im = -sinf(phase);
    }
    if (freq_out) *freq_out = carr_freq;                     // :20
    return GM_OK;
}

int gm_apply_doppler_shift(const gm_c32* samples, const gm_c32* table, gm_c32* output, size_t n) {
    if (!samples || !table || !output) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (int rc = ensure_device(g_device)) return rc;
    const size_t n4 = (n / 4) * 4;
    if (!n4) return GM_OK;
    cf *ds = nullptr, *dt = nullptr, *dout = nullptr;
    HIPC(hipMalloc(&ds, n4 * 8)); HIPC(hipMalloc(&dt, n4 * 8)); HIPC(hipMalloc(&dout, n4 * 8));
    HIPC(hipMemcpy(ds, samples, n4 * 8, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(dt, table, n4 * 8, hipMemcpyHostToDevice));
    gm::launch_apply_doppler(nullptr, ds, dt, dout, n);
    HIPC(hipGetLastError());
    HIPC(hipMemcpy(output, dout, n4 * 8, hipMemcpyDeviceToHost));   // tail n%4 untouched, like the reference
    hipFree(ds); hipFree(dt); hipFree(dout);
    return GM_OK;
}

// ---------------------------------------------------------------- FFT<T> / RealFFT<T>
int gm_fft_supported_sizes(uint32_t* sizes, int cap) { return gm::list_plans(sizes, cap); }

// the in-LDS plan of a length, decided on the size_t value: nothing above 16384 has one (int(n) of 2^32 + 256 is 256)
static const gm::PlanOps* plan_for(size_t n) { return n <= 16384 ? gm::find_plan(int(n)) : nullptr; }

// power-of-two lengths above one LDS buffer: L = N1 * N2, both in-LDS power-of-two plans.  The loop takes the SMALLEST N2 in 256, 512, ...
// with N1 = L / N2 >= N2 a plan of at most 16384: N2 = 256 up to 2^22, then 16384 x 512 ... 16384 x 16384 (32768 = 256 x 128: none)
static bool pow2_split(size_t n, const gm::PlanOps** p1, const gm::PlanOps** p2) {
    if (n < 2 || (n & (n - 1)) || n > (size_t(1) << 28)) return false;
    for (size_t n2 = 256; n2 * n2 <= n || n2 <= 16384; n2 *= 2) {
        if (n % n2) continue;
        const size_t n1 = n / n2;
        if (n1 < n2) break;
        const gm::PlanOps *a = plan_for(n1), *b = plan_for(n2);
        if (a && b && a->big_cols && b->big_rows) { *p1 = a; *p2 = b; return true; }
    }
    return false;
}
// the four-step transform of length p1->n * p2->n on `batch` device arrays: columns by p1 (grid p2->n), rows by p2 (grid p1->n)
static int fft_run_four_step(const gm::PlanOps* p1, const gm::PlanOps* p2, int dir, cf* d_data, size_t batch, hipStream_t st) {
    const size_t n = size_t(p1->n) * size_t(p2->n);
    std::vector<cf> t1(size_t(p1->tw_total) + 1), t2(size_t(p2->tw_total) + 1);
    p1->fill_tw(t1.data(), dir != 0);
    p2->fill_tw(t2.data(), dir != 0);
    cf *d_t1 = nullptr, *d_t2 = nullptr, *d_b = nullptr;
    auto done = [&](int code) { hipFree(d_t1); hipFree(d_t2); hipFree(d_b); return code; };
    if (hipMalloc(&d_t1, t1.size() * 8) != hipSuccess || hipMalloc(&d_t2, t2.size() * 8) != hipSuccess || hipMalloc(&d_b, n * 8) != hipSuccess)
        return done(set_err(GM_ERR_NOMEM, "hipMalloc (long FFT)"));
    if (hipMemcpy(d_t1, t1.data(), t1.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_t2, t2.data(), t2.size() * 8, hipMemcpyHostToDevice) != hipSuccess) return done(set_err(GM_ERR_HIP, "hipMemcpy"));
    for (size_t it = 0; it < batch; ++it) {
        cf* x = d_data + it * n;
        p1->big_cols(st, x, d_b, d_t1, uint32_t(p2->n), dir != 0);
        p2->big_rows(st, d_b, x, d_t2, uint32_t(p1->n), dir != 0);
    }
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return done(set_err(GM_ERR_HIP, "long FFT kernels"));
    return done(GM_OK);
}
static int fft_run_big(size_t n, int dir, cf* d_data, size_t batch, hipStream_t st) {
    const gm::PlanOps *p1 = nullptr, *p2 = nullptr;
    if (!pow2_split(n, &p1, &p2)) return set_err(GM_ERR_UNSUPPORTED_N, "no in-LDS FFT plan for this length");
    return fft_run_four_step(p1, p2, dir, d_data, batch, st);
}

static int fft_run(size_t n, int dir, cf* d_data, size_t batch, hipStream_t st) {
    const gm::PlanOps* pl = plan_for(n);
    if (!pl) return fft_run_big(n, dir, d_data, batch, st);
    std::vector<cf> tw(size_t(pl->tw_total) + 1);
    pl->fill_tw(tw.data(), dir != 0);
    cf* d_tw = nullptr;
    HIPC(hipMalloc(&d_tw, tw.size() * sizeof(cf)));
    HIPC(hipMemcpy(d_tw, tw.data(), tw.size() * sizeof(cf), hipMemcpyHostToDevice));
    pl->fft_batch(st, d_data, d_tw, dir != 0, int(batch));
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(st));
    hipFree(d_tw);
    return GM_OK;
}

// Bluestein's transform length for n: the smallest power of two L >= max(256, 2n - 1) that has a transform (32768 = 256 x 128 has no
// two in-LDS factors: 65536 then); 0 where there is none (n above 2^23, decided before 2n is formed)
static size_t bluestein_len(size_t n) {
    if (n > (size_t(1) << 23)) return 0;
    size_t L = 256;
    while (L < 2 * n - 1) L *= 2;
    const gm::PlanOps *p1 = nullptr, *p2 = nullptr;
    while (L <= (size_t(1) << 24) && !plan_for(L) && !pow2_split(L, &p1, &p2)) L *= 2;
    return L <= (size_t(1) << 24) ? L : 0;
}
// a length FFT<T> serves: an in-LDS plan, a four-step pair, or Bluestein on one of the two
static bool fft_len_supported(size_t n) {
    const gm::PlanOps *p1 = nullptr, *p2 = nullptr;
    return plan_for(n) || pow2_split(n, &p1, &p2) || bluestein_len(n);
}

// FFT<T>::new is generic over the length (src/fft.rs:10-19: rustfft plans any N).  Lengths without an in-LDS plan go
// through Bluestein's chirp-z identity on the smallest power-of-two plan L >= 2N - 1:
//   X[k] = c[k] * sum_n (x[n] c[n]) conj(c[k - n]),   c[n] = exp(-j pi n^2 / N)   (phase from n^2 mod 2N: exact in integers)
// i.e. one length-L circular convolution = two forward transforms (the chirp's is cached per N) and one inverse on the
// device; the three O(N) chirp products are host loops (this entry takes and returns host buffers).  L up to 2^24 (N <= 2^23):
// powers of two above one LDS buffer run as a four-step transform (fft_run_big).
static int fft_bluestein(size_t n, int dir, gm_c32* inout, size_t batch) {
    const size_t L = bluestein_len(n);
    if (!L) return set_err(GM_ERR_UNSUPPORTED_N, "length above 2^23: no FFT plan (Bluestein needs a power of two >= 2N - 1, at most 2^24)");
    std::vector<cf> c(n), b(L, gm::cf_make(0.f, 0.f));
    for (size_t i = 0; i < n; ++i) {
        const double a = M_PI * double((uint64_t(i) * i) % (2 * n)) / double(n);
        c[i] = gm::cf_make(float(cos(a)), float(-sin(a)));
    }
    b[0] = gm::cf_make(1.f, 0.f);
    for (size_t i = 1; i < n; ++i) b[i] = b[L - i] = gm::cf_make(c[i].x, -c[i].y);
    cf *d_b = nullptr, *d_a = nullptr, *d_y = nullptr;
    int rc = GM_OK;
    auto done = [&](int code) { hipFree(d_b); hipFree(d_a); hipFree(d_y); return code; };
    if (hipMalloc(&d_b, L * 8) != hipSuccess || hipMalloc(&d_a, L * 8) != hipSuccess || hipMalloc(&d_y, L * 8) != hipSuccess)
        return done(set_err(GM_ERR_HIP, "hipMalloc"));
    if (hipMemcpy(d_b, b.data(), L * 8, hipMemcpyHostToDevice) != hipSuccess) return done(set_err(GM_ERR_HIP, "hipMemcpy"));
    if ((rc = fft_run(L, 0, d_b, 1, nullptr))) return done(rc);
    std::vector<cf> a(L), y(L);
    const float inv_l = 1.0f / float(L);
    for (size_t it = 0; it < batch; ++it) {
        gm_c32* x = inout + it * n;
        for (size_t i = 0; i < L; ++i) a[i] = gm::cf_make(0.f, 0.f);
        for (size_t i = 0; i < n; ++i) {       // inverse transform: conj(FFT(conj(x)))
            const cf xi = gm::cf_make(x[i].re, dir ? -x[i].im : x[i].im);
            a[i] = gm::cf_make(xi.x * c[i].x - xi.y * c[i].y, xi.x * c[i].y + xi.y * c[i].x);
        }
        if (hipMemcpy(d_a, a.data(), L * 8, hipMemcpyHostToDevice) != hipSuccess) return done(set_err(GM_ERR_HIP, "hipMemcpy"));
        if ((rc = fft_run(L, 0, d_a, 1, nullptr))) return done(rc);
        gm::launch_apply_doppler(nullptr, d_a, d_b, d_y, L);                    // elementwise complex product (L % 4 == 0)
        if (hipGetLastError() != hipSuccess) return done(set_err(GM_ERR_HIP, "product kernel"));
        if ((rc = fft_run(L, 1, d_y, 1, nullptr))) return done(rc);
        if (hipMemcpy(y.data(), d_y, L * 8, hipMemcpyDeviceToHost) != hipSuccess) return done(set_err(GM_ERR_HIP, "hipMemcpy"));
        for (size_t k = 0; k < n; ++k) {
            const float yr = y[k].x * inv_l, yi = y[k].y * inv_l;
            const float re = yr * c[k].x - yi * c[k].y, im = yr * c[k].y + yi * c[k].x;
            x[k].re = re; x[k].im = dir ? -im : im;
        }
    }
    return done(GM_OK);
}

int gm_fft_c2c_f32(size_t n, int dir, gm_c32* inout, size_t batch) {
    if (!inout || !n || !batch) return set_err(GM_ERR_INVALID_ARG, "null or empty");
    if (int rc = ensure_device(g_device)) return rc;
    {
        const gm::PlanOps *p1 = nullptr, *p2 = nullptr;
        if (!plan_for(n) && !pow2_split(n, &p1, &p2)) return fft_bluestein(n, dir, inout, batch);
    }
    cf* d = nullptr;
    HIPC(hipMalloc(&d, n * batch * 8));
    HIPC(hipMemcpy(d, inout, n * batch * 8, hipMemcpyHostToDevice));
    const int rc = fft_run(n, dir, d, batch, nullptr);
    if (!rc) HIPC(hipMemcpy(inout, d, n * batch * 8, hipMemcpyDeviceToHost));
    hipFree(d);
    return rc;
}

int gm_fft_power_spectrum_f32(size_t n, gm_c32* inout, float* power) {
    if (!inout || !power || !n) return set_err(GM_ERR_INVALID_ARG, "null or empty");
    if (int rc = ensure_device(g_device)) return rc;
    const gm::PlanOps *pp1 = nullptr, *pp2 = nullptr;
    if (!plan_for(n) && !pow2_split(n, &pp1, &pp2)) {            // any other length: Bluestein, then |X|^2 on the host
        if (int rc = fft_bluestein(n, 0, inout, 1)) return rc;
        for (size_t i = 0; i < n; ++i) power[i] = inout[i].re * inout[i].re + inout[i].im * inout[i].im;   // norm_sqr (fft.rs:28)
        return GM_OK;
    }
    cf* d = nullptr; float* dp = nullptr;
    HIPC(hipMalloc(&d, n * 8)); HIPC(hipMalloc(&dp, n * 4));
    HIPC(hipMemcpy(d, inout, n * 8, hipMemcpyHostToDevice));
    int rc = fft_run(n, 0, d, 1, nullptr);
    if (!rc) {
        gm::launch_power(nullptr, d, dp, n);
        HIPC(hipGetLastError());
        HIPC(hipMemcpy(inout, d, n * 8, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(power, dp, n * 4, hipMemcpyDeviceToHost));
    }
    hipFree(d); hipFree(dp);
    return rc;
}

int gm_rfft_f32(size_t n, const float* in, gm_c32* out) {
    if (!in || !out || !n) return set_err(GM_ERR_INVALID_ARG, "null or empty");
    if (!fft_len_supported(n)) return set_err(GM_ERR_UNSUPPORTED_N, "no FFT plan for this length");   // before n words are read
    std::vector<gm_c32> buf(n);
    for (size_t i = 0; i < n; ++i) { buf[i].re = in[i]; buf[i].im = 0.0f; }
    const int rc = gm_fft_c2c_f32(n, 0, buf.data(), 1);
    if (!rc) memcpy(out, buf.data(), (n / 2 + 1) * sizeof(gm_c32));
    return rc;
}

// Diagnostic: the four-step transform of a NAMED factor pair (the public entries reach only the pairs pow2_split chooses)
int gm_debug_fft_four_step(uint32_t n1, uint32_t n2, int dir, gm_c32* inout, size_t batch) {
    if (!inout || !batch) return set_err(GM_ERR_INVALID_ARG, "null or empty");
    const gm::PlanOps *p1 = plan_for(n1), *p2 = plan_for(n2);
    if (!p1 || !p2 || !p1->big_cols || !p2->big_rows)
        return set_err(GM_ERR_UNSUPPORTED_N, "both factors must be power-of-two in-LDS plans");
    if (batch > (size_t(1) << 31) / (size_t(n1) * n2)) return set_err(GM_ERR_OUT_OF_RANGE, "more than 2^31 points in one call");
    if (int rc = ensure_device(g_device)) return rc;
    const size_t bytes = size_t(n1) * n2 * batch * 8;                    // n1 * n2 <= 2^28
    cf* d = nullptr;
    HIPC(hipMalloc(&d, bytes));
    int rc = hipMemcpy(d, inout, bytes, hipMemcpyHostToDevice) == hipSuccess ? GM_OK : set_err(GM_ERR_HIP, "hipMemcpy");
    if (!rc) rc = fft_run_four_step(p1, p2, dir, d, batch, nullptr);
    if (!rc && hipMemcpy(inout, d, bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = set_err(GM_ERR_HIP, "hipMemcpy");
    hipFree(d);
    return rc;
}

// ---------------------------------------------------------------- acquisition
int gm_acq_destroy(gm_acq* a) {
    if (!a) return GM_OK;
    if (a->device >= 0) hipSetDevice(a->device);
    acq_edge_free(a->edge);
    acq_drift_free(a->drift);
    hipFree(a->d_planes);
    if (a->d_long_code != a->d_code_fft) hipFree(a->d_long_code);
    hipFree(a->d_long_z); hipFree(a->d_long_part);
    hipFree(a->d_comp_tmp); hipFree(a->d_comp_twn); hipFree(a->d_code_comb); hipFree(a->d_split_scratch); hipFree(a->d_split_counter);
    hipFree(a->fine.d_chips); hipFree(a->fine.d_tw1); hipFree(a->fine.d_tw2); hipFree(a->fine.d_B); hipFree(a->fine.d_mean);
    hipFree(a->fine.d_rowmax); hipFree(a->fine.d_rowarg); hipFree(a->fine.d_sat_worker); hipFree(a->fine.d_sat_cp);
    hipFree(a->fine.d_peak_pow); hipFree(a->fine.d_peak_idx);
    a->refine.release(); a->local.release(); a->array.release(); a->cancel.release(); hipFree(a->d_cancel_chips);
    if (a->device >= 0) hipSetDevice(a->device);
    hipFree(a->d_tw_mix);
    hipFree(a->d_tables); hipFree(a->d_tw_fwd); hipFree(a->d_tw_inv); hipFree(a->d_code_fft); hipFree(a->d_code_fft_paired); hipFree(a->d_order);
    hipFree(a->d_spectra); hipFree(a->d_rho); hipFree(a->d_table_freq); hipFree(a->d_code_samples); hipFree(a->d_samples);
    hipFree(a->d_metrics); hipFree(a->d_worker_list); if (a->d_results) hipHostFree(a->d_results);
    hipFree(a->d_prn_ids);
    for (auto& e : a->tm.ev) if (e) hipEventDestroy(e);
    if (a->ahead.side) { hipStreamSynchronize(a->ahead.side); hipStreamDestroy(a->ahead.side); }
    if (a->ahead.ev_s) hipEventDestroy(a->ahead.ev_s);
    if (a->ahead.ev_f) hipEventDestroy(a->ahead.ev_f);
    if (a->ahead.ev_in) hipEventDestroy(a->ahead.ev_in);
    hipFree(a->ahead.d_spectra_alt);
    if (a->own_stream && a->stream) hipStreamDestroy(a->stream);
    delete a;
    return GM_OK;
}

// Which path serves an fft_size — the one rule behind gm_acq_plan_info and gm_acq_create.  In-LDS plan, else Q x base composite
// (acq_composite.hip), else with any_length the long path (acq_long.hip): L = N over the largest base that divides N with Q <= 32,
// else the smallest Q x base >= 2N (equal lengths: the larger base).  *pl: the base plan, *comp / *lng: the composite / long kernels.
static int acq_choose(uint32_t n, int32_t any_length, gm_acq_plan* info, const gm::PlanOps** pl, const gm::CompOps** comp,
                      const gm::LongOps** lng) {
    gm_acq_plan o{GM_ACQ_FORM_LDS, n, 1, n};
    const gm::PlanOps* p = nullptr;
    const gm::CompOps* c = nullptr;
    const gm::LongOps* l = nullptr;
    if (!n) return GM_ERR_INVALID_ARG;
    if (n % 8) return GM_ERR_ALIGNMENT;
    if ((p = gm::find_plan(int(n)))) {
    } else if ((c = gm::find_comp(n))) {
        p = gm::find_plan(c->nb);
        o = gm_acq_plan{GM_ACQ_FORM_COMPOSITE, uint32_t(c->nb), uint32_t(c->q), n};
    } else if (any_length && n >= 1024 && n <= 262144) {
        int nl = 0;
        const gm::LongOps* bases = gm::long_bases(&nl);
        for (int i = 0; i < nl && !l; ++i)       // largest base first
            if (n % uint32_t(bases[i].nb) == 0 && n / uint32_t(bases[i].nb) <= 32) {
                l = &bases[i];
                o = gm_acq_plan{GM_ACQ_FORM_LONG, uint32_t(l->nb), n / uint32_t(l->nb), n};
            }
        if (!l) {
            uint64_t best = 0;
            for (int i = 0; i < nl; ++i) {
                const uint64_t nb = uint64_t(bases[i].nb), q = (2 * uint64_t(n) + nb - 1) / nb;
                if (q <= 32 && (!best || q * nb < best)) { best = q * nb; l = &bases[i]; }
            }
            if (l) o = gm_acq_plan{GM_ACQ_FORM_LONG_PADDED, uint32_t(l->nb), uint32_t(best / uint64_t(l->nb)), uint32_t(best)};
        }
        if (l) p = gm::find_plan(l->nb);
    }
    if (!p) return GM_ERR_UNSUPPORTED_N;
    if (info) *info = o;
    if (pl) *pl = p;
    if (comp) *comp = c;
    if (lng) *lng = l;
    return GM_OK;
}

int gm_acq_plan_info(uint32_t fft_size, int32_t any_length, gm_acq_plan* out) {
    const int rc = acq_choose(fft_size, any_length, out, nullptr, nullptr, nullptr);
    if (rc == GM_ERR_ALIGNMENT) return set_err(rc, "fft_size % 8 != 0");
    if (rc == GM_ERR_UNSUPPORTED_N) return set_err(rc, "no acquisition path for this fft_size (gm_acq_cfg.any_length: multiples of 8 in [1024, 262144])");
    if (rc) return set_err(rc, "fft_size is required");
    return GM_OK;
}

int gm_acq_create(const gm_acq_cfg* cfg, gm_acq** out) {
    if (!cfg || !out) return set_err(GM_ERR_INVALID_ARG, "null cfg/out");
    *out = nullptr;
    if (!cfg->fft_size || !cfg->n_integrations || !cfg->n_bins || !cfg->n_prn || !cfg->prn_ids)
        return set_err(GM_ERR_INVALID_ARG, "fft_size, n_integrations, n_bins, n_prn, prn_ids are required");
    if (!cfg->tables && !cfg->doppler_hz) return set_err(GM_ERR_INVALID_ARG, "doppler_hz or tables required");
    if (cfg->tables && !cfg->table_freq) return set_err(GM_ERR_INVALID_ARG, "table_freq required with tables");
    if (cfg->fft_size % 8) return set_err(GM_ERR_ALIGNMENT, "fft_size % 8 != 0");
    if (cfg->coherent_periods > uint32_t(gm::GM_COHERENT_MAX)) return set_err(GM_ERR_INVALID_ARG, "coherent_periods > 32");
    const gm::PlanOps* pl = nullptr;
    const gm::CompOps* comp = nullptr;
    const gm::LongOps* lng = nullptr;
    gm_acq_plan form{};
    if (acq_choose(cfg->fft_size, cfg->any_length, &form, &pl, &comp, &lng) != GM_OK) pl = nullptr;
    uint32_t comp_q = comp ? uint32_t(comp->q) : 1;
    if (pl && !comp && !lng && !cfg->strict_sum_order && !cfg->reference_products && gm::diag_int("GM_COMP_BASE", 0) > 0) {      // diagnostic: a size with a fused plan through the composite path
        const gm::CompOps* c = gm::find_comp(cfg->fft_size);
        if (c && c->nb == gm::diag_int("GM_COMP_BASE", 0)) { comp = c; pl = gm::find_plan(c->nb); comp_q = uint32_t(c->q); }
    }
    if (!pl) return set_err(GM_ERR_UNSUPPORTED_N, cfg->any_length ? "no acquisition path for this fft_size (any_length: multiples of 8 in [1024, 262144])"
                                                                 : "no in-LDS FFT plan for this fft_size, nor Q x {16384, 16368, 16000, 8192, 8184, 8000, 6000, 5000, 4000} with Q in {2,3,4,5,6,8}");
    // (strict_sum_order on a composite size: the kernels also store the power planes and a second kernel sums them in the reference's
    //  order — P * D * N * 4 bytes of planes: 189 MB at the configs[3] Galileo geometry)
    if (cfg->reference_products && (comp_q > 1 || lng))
        return set_err(GM_ERR_INVALID_ARG, "reference_products needs an fft_size with an in-LDS plan (gm_fft_supported_sizes)");
    if (int rc = ensure_device(g_device)) return rc;

    gm_acq* a = new gm_acq();
    a->device = g_device;
    a->cfg = *cfg;
    a->plan = pl;
    a->N = cfg->fft_size; a->D = cfg->n_bins; a->M = cfg->n_integrations; a->P = cfg->n_prn;
    a->K = cfg->coherent_periods > 1 ? cfg->coherent_periods : 1;
    a->Q = lng ? form.q : comp_q; a->Nb = uint32_t(pl->n); a->comp = comp;
    a->lng = lng;
    if (lng) {
        a->L = form.transform_len;
        a->long_lim = form.form == GM_ACQ_FORM_LONG_PADDED ? 2 * cfg->fft_size : cfg->fft_size;
        const double r = double(cfg->fft_size) / double(a->L);
        a->long_scale = float(r * r);
    }
    if (cfg->threshold == 0.0f) a->cfg.threshold = 7.0f;
    a->code_rate = cfg->codes ? (cfg->code_rate > 0 ? cfg->code_rate : CA_RATE) : CA_RATE;
    a->prn_ids.assign(cfg->prn_ids, cfg->prn_ids + a->P);
    const size_t N = a->N, D = a->D, M = a->M, P = a->P, K = a->K;
    int rc = GM_OK;
    auto fail = [&](int code) { gm_acq_destroy(a); return code; };
    if (K > 1 && !(a->coh_fwd = acq_find_stage_f<gm::CohLoad>(a)))
        return fail(set_err(GM_ERR_UNSUPPORTED_N, "no coherent stage F for this handle's base plan"));

    // Doppler tables (do_acquisition.rs:252-262) — host glibc cosf/sinf like the reference
    std::vector<gm_c32> tables(D * N);
    a->table_freq.resize(D);
    if (cfg->tables) {
        memcpy(tables.data(), cfg->tables, D * N * sizeof(gm_c32));
        memcpy(a->table_freq.data(), cfg->table_freq, D * sizeof(float));
    } else {
        for (size_t d = 0; d < D; ++d)
            gm_doppler_table_new(cfg->f_if, cfg->doppler_hz[d], cfg->fs, N, &a->table_freq[d], &tables[d * N]);
    }
    // the coherent fold's phasors: rho[d][k] = exp(-j 2 pi f_d k N / fs), bin d's table phasor continued to sample k N — in f64 with
    // the phase reduced to one cycle before cos / sin, then rounded to f32 (K = 1: the single word (1, 0))
    std::vector<gm_c32> rho(D * K);
    for (size_t d = 0; d < D; ++d)
        for (size_t k = 0; k < K; ++k) {
            const double cyc = double(a->table_freq[d]) * double(k * N) / double(cfg->fs);
            const double ang = 2.0 * 3.14159265358979323846 * (cyc - ::floor(cyc));
            rho[d * K + k] = gm_c32{float(::cos(ang)), float(0.0 - ::sin(ang))};      // (0.0 - : k = 0 is (1, +0))
        }
    // replica samples (AcquisitionWorker::new :132-135)
    std::vector<int8_t> code_samples(P * N);
    a->code_len = cfg->codes ? cfg->code_len : 1023u;
    a->chips.resize(P * size_t(a->code_len));
    for (size_t p = 0; p < P; ++p) {
        if (cfg->codes) {
            if (!cfg->code_len) return fail(set_err(GM_ERR_INVALID_ARG, "code_len required with codes"));
            memcpy(&a->chips[p * a->code_len], cfg->codes + p * cfg->code_len, cfg->code_len);
            rc = resample_code(cfg->codes + p * cfg->code_len, cfg->code_len, true, a->code_rate, cfg->fs, N,
                               &code_samples[p * N]);
        } else {
            const uint8_t prn = a->prn_ids[p];
            if (prn < 1 || prn > 32) return fail(set_err(GM_ERR_OUT_OF_RANGE, "prn must be 1..=32"));
            // rustfft's process() panics unless the replica length equals fft_size (:135-137)
            if (num_samples_per_code(CA_RATE, cfg->fs, CA_LEN) != N)
                return fail(set_err(GM_ERR_INVALID_ARG, "fft_size != round(fs / 1 kHz)"));
            memcpy(&a->chips[p * 1023], ca_table().rows[prn - 1], 1023);
            rc = resample_code(ca_table().rows[prn - 1], 1023, false, CA_RATE, cfg->fs, N, &code_samples[p * N]);
        }
        if (rc) return fail(set_err(rc, "code resampling index out of range"));
    }
    // inverse twiddles: the in-LDS correlation kernel's own plan (CorrPlanOf) for a size that fits one LDS image, the registered plan's
    // (what the composite kernels run on) for Q x base
    const bool twi_corr = acq_fused(a);
    std::vector<cf> twf(size_t(pl->tw_total) + 1), twi(size_t(twi_corr ? pl->tw_total_corr : pl->tw_total) + 1);
    pl->fill_tw(twf.data(), false);
    if (twi_corr) pl->fill_tw_corr(twi.data());
    else pl->fill_tw(twi.data(), true);
    std::vector<cf> twm(size_t(pl->tw_total_mix) + 1);
    pl->fill_tw_mix(twm.data(), false);

#define HIPA(expr)                                                     \
    do {                                                               \
        hipError_t _e = (expr);                                        \
        if (_e != hipSuccess) return fail(hip_fail(_e, #expr));        \
    } while (0)
    HIPA(hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking));
    a->own_stream = true;
    HIPA(hipMalloc(&a->d_tables, D * N * 8));
    HIPA(hipMalloc(&a->d_table_freq, D * 4));
    HIPA(hipMalloc(&a->d_tw_fwd, twf.size() * 8));
    HIPA(hipMalloc(&a->d_tw_inv, twi.size() * 8));
    HIPA(hipMalloc(&a->d_tw_mix, twm.size() * 8));
    HIPA(hipMalloc(&a->d_code_samples, P * N));
    HIPA(hipMalloc(&a->d_code_fft, P * N * 8));
    HIPA(hipMalloc(&a->d_spectra, D * M * (a->lng ? size_t(a->L) : N) * 8));
    a->samples_cap = K * M * N * 8;
    HIPA(hipMalloc(&a->d_samples, a->samples_cap));
    HIPA(hipMalloc(&a->d_metrics, 3 * P * D * 4));
    HIPA(hipMemsetAsync(a->d_metrics, 0, 3 * P * D * 4, a->stream));
    HIPA(hipMalloc(&a->d_worker_list, P * 4));
    HIPA(hipMalloc(&a->d_rho, D * K * 8));
    HIPA(hipMemcpy(a->d_rho, rho.data(), D * K * 8, hipMemcpyHostToDevice));
    if (acq_fused(a) && pl->split_slab && M >= 2) {
        // planes the tail split can ever use for THIS handle (corr_split_planes, acq_corr_grid.h): never more than GM_CORR_SPLIT_MAX_SLABS
        const size_t planes = gm::corr_split_planes(P, D, M);
        a->split_planes = int(planes);
        HIPA(hipMalloc(&a->d_split_scratch, planes * pl->split_slab * sizeof(float)));
        HIPA(hipMalloc(&a->d_split_counter, gm::GM_CORR_SPLIT_MAX_ITEMS * sizeof(uint32_t)));
        HIPA(hipMemsetAsync(a->d_split_counter, 0, gm::GM_CORR_SPLIT_MAX_ITEMS * sizeof(uint32_t), a->stream));
    }
    HIPA(hipMemcpy(a->d_tables, tables.data(), D * N * 8, hipMemcpyHostToDevice));
    HIPA(hipMemcpy(a->d_table_freq, a->table_freq.data(), D * 4, hipMemcpyHostToDevice));
    HIPA(hipMemcpy(a->d_tw_fwd, twf.data(), twf.size() * 8, hipMemcpyHostToDevice));
    HIPA(hipMemcpy(a->d_tw_inv, twi.data(), twi.size() * 8, hipMemcpyHostToDevice));
    HIPA(hipMemcpy(a->d_tw_mix, twm.data(), twm.size() * 8, hipMemcpyHostToDevice));
    HIPA(hipMemcpy(a->d_code_samples, code_samples.data(), P * N, hipMemcpyHostToDevice));
    if ((rc = acq_reserve_results(a, uint32_t(P)))) return fail(rc);
    HIPA(hipMemcpy(a->d_prn_ids, a->prn_ids.data(), P, hipMemcpyHostToDevice));
    a->dev_prn_ids = a->prn_ids;
    // replica spectra: forward FFT of the resampled code (:136-138)
    int (*fill_order)(uint16_t*) = a->lng ? nullptr : (a->Q == 1 ? pl->fill_order : comp->fill_order);
    if (const int n_order = fill_order ? fill_order(nullptr) : 0) {      // this (base) size's correlation plan reads a permuted spectrum
        std::vector<uint16_t> order(static_cast<size_t>(n_order), 0);
        fill_order(order.data());
        HIPA(hipMalloc(&a->d_order, order.size() * sizeof(uint16_t)));
        HIPA(hipMemcpy(a->d_order, order.data(), order.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    }
    if (a->lng) {     // the signal's two forward steps on the chips (zero-padded to L), natural order
        const size_t L = a->L;
        if (L == N) a->d_long_code = a->d_code_fft;
        else HIPA(hipMalloc(&a->d_long_code, P * L * 8));
        a->lng->fwd_sub(a->stream, nullptr, GM_FMT_C32, nullptr, a->d_code_samples, a->d_tw_fwd, a->d_long_code, uint32_t(P), a->Q,
                        uint32_t(N), uint32_t(N), 1);
        gm::launch_long_fwd_post(a->stream, a->d_long_code, uint32_t(P), a->Q, a->Nb);
        // the inverse's intermediate, per slab of (worker, bin) items (long_slab_items, acq_corr_grid.h)
        const size_t slab = gm::long_slab_items(P, D, M, L);
        a->long_slab = uint32_t(slab);
        HIPA(hipMalloc(&a->d_long_z, slab * M * L * 8));
        HIPA(hipMalloc(&a->d_long_part, 3 * P * D * a->Q * 4));
        if (cfg->strict_sum_order) HIPA(hipMalloc(&a->d_planes, P * D * N * sizeof(float)));
        if (L != N) {     // gm_acq_code_fft's length-N spectrum (the API's view): the same chips through the any-length FFT (Bluestein)
            std::vector<gm_c32> cb(P * N);
            for (size_t i = 0; i < P * N; ++i) { cb[i].re = float(code_samples[i]); cb[i].im = 0.0f; }
            HIPA(hipStreamSynchronize(a->stream));
            if ((rc = gm_fft_c2c_f32(N, 0, cb.data(), P))) return fail(rc);
            HIPA(hipMemcpy(a->d_code_fft, cb.data(), P * N * 8, hipMemcpyHostToDevice));
        }
    } else if (a->Q == 1) {
        pl->code_fft(a->stream, a->d_code_samples, a->d_tw_fwd, a->d_code_fft, int(P));
        HIPA(hipMalloc(&a->d_code_fft_paired, P * N * 8));
        pl->pair_codes(a->stream, a->d_code_fft, a->d_code_fft_paired, int(P));
    } else {     // the signal's two forward steps on the chips: natural order (the API's view), then every block paired
        const size_t tmp_items = D * M > P ? D * M : P;
        HIPA(hipMalloc(&a->d_comp_tmp, tmp_items * N * 8));
        if (cfg->strict_sum_order) HIPA(hipMalloc(&a->d_planes, P * D * N * sizeof(float)));
        HIPA(hipMalloc(&a->d_comp_twn, N * 8));
        HIPA(hipMalloc(&a->d_code_fft_paired, P * N * 8));
        std::vector<gm::cf> twn(N);
        comp->fill_twn(twn.data());
        HIPA(hipMemcpy(a->d_comp_twn, twn.data(), N * 8, hipMemcpyHostToDevice));
        comp->fwd_sub(a->stream, nullptr, GM_FMT_C32, nullptr, a->d_code_samples, a->d_tw_mix, a->d_comp_tmp, uint32_t(P), 1, nullptr);
        comp->fwd_post(a->stream, a->d_comp_tmp, a->d_code_fft, uint32_t(P), 0, nullptr);
        comp->relayout(a->stream, a->d_code_fft, a->d_code_fft_paired, int(P * a->Q));
        HIPA(hipMalloc(&a->d_code_comb, P * a->Q * N * 8));      // [code][n1][k1][pos]: the whole code-side factor per sub-transform
        comp->comb(a->stream, a->d_code_fft_paired, a->d_comp_twn, a->d_code_comb, uint32_t(P));
        if (a->d_order) {     // sub-transforms leave in storage order: the signal's forward step 2 goes into the table as well (CompOps::fold_post)
            gm::cf* comb2 = nullptr;
            HIPA(hipMalloc(&comb2, P * a->Q * N * 8));
            comp->fold_post(a->stream, a->d_code_comb, a->d_order, comb2, uint32_t(P));
            HIPA(hipStreamSynchronize(a->stream));
            hipFree(a->d_code_comb);
            a->d_code_comb = comb2;
            a->comp_post_folded = true;
        }
    }
    HIPA(hipGetLastError());
    HIPA(hipStreamSynchronize(a->stream));
    a->worker_list.clear();
    a->n_workers = 0xffffffffu;   // force the first upload
    if ((rc = acq_set_mask(a, ~0ull))) return fail(rc);
#undef HIPA
    *out = a;
    return GM_OK;
}

int gm_acq_set_stream(gm_acq* a, void* s) {
    if (!a) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (a->dec_deferred) { if (int rc = ensure_device(a->device)) return rc; if (int rc = acq_flush_decision(a)) return rc; }
    if (a->own_stream && a->stream) { hipStreamSynchronize(a->stream); hipStreamDestroy(a->stream); }
    a->stream = reinterpret_cast<hipStream_t>(s);
    a->own_stream = false;
    return GM_OK;
}

int gm_acq_set_prn_mask(gm_acq* a, uint64_t mask) {
    if (!a) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (int rc = ensure_device(a->device)) return rc;
    return acq_set_mask(a, mask);
}

// Stage F of a coherent handle (K >= 2), of its edge search and of a handle with code-drift compensation (K = 1 included), on stream
// `st` into `spectra` (acq_stage_f_variants.h): the family's kernel of the handle's form — with the drift compensation every period
// from its own start, with the edge search H hypotheses, [H * D][M][.] — and then the post pass of the form in chunks of at most 65535
// items (grid rows).  clear_tickets: the tail split's tickets for the in-LDS form to clear on its way, or null.
static void acq_stage_f_variant(const gm_acq* a, hipStream_t st, const void* d_samples, int fmt, cf* spectra, uint32_t* clear_tickets) {
    const gm_acq::Edge& eg = a->edge;
    const gm_acq::Drift& dr = a->drift;
    const bool edge = eg.H > 0;
    gm::StageFArgs c{};
    c.samples = d_samples; c.fmt = fmt; c.K = a->K; c.rho = a->d_rho; c.H = 1;
    if (dr.on) { c.starts = dr.d_starts; c.R = dr.R; c.rho = dr.d_rho; }
    if (edge) { c.offsets = eg.d_offsets; c.H = eg.H; c.neg = eg.neg; }
    c.tables = a->d_tables; c.n_bins = a->D; c.n_int = a->M; c.Q = a->Q; c.N = a->N; c.lim = a->long_lim;
    c.order = a->lng ? nullptr : a->d_order;
    c.clear_tickets = clear_tickets;
    const gm::StageFLaunch fwd = dr.on ? dr.fwd : (edge ? eg.fwd : a->coh_fwd);
    const uint32_t items = c.H * a->D * a->M;
    if (a->lng) {
        c.tw_fwd = a->d_tw_fwd; c.out = spectra;
        fwd(st, c);
        for (uint32_t i0 = 0; i0 < items; i0 += 65535u)
            gm::launch_long_fwd_post(st, spectra + size_t(i0) * a->L, items - i0 < 65535u ? items - i0 : 65535u, a->Q, a->Nb);
    } else if (a->Q == 1) {
        c.tw_fwd = a->d_tw_mix; c.out = spectra;
        fwd(st, c);
    } else {
        // the sub-transforms ARE what the correlation kernel reads (comp_post_folded), else forward step 2 follows
        cf* const tmp = edge ? eg.d_tmp : a->d_comp_tmp;
        c.tw_fwd = a->d_tw_mix; c.out = a->comp_post_folded ? spectra : tmp;
        fwd(st, c);
        if (!a->comp_post_folded)
            for (uint32_t i0 = 0; i0 < items; i0 += 65535u)
                a->comp->fwd_post(st, tmp + size_t(i0) * a->N, spectra + size_t(i0) * a->N, items - i0 < 65535u ? items - i0 : 65535u, 1, a->d_order);
    }
}

// stage F (unless `prepared`: then the spectra wait in the second buffer) + stage C of one dwell on the handle's stream
static int acq_search_common(gm_acq* a, const void* d_samples, int fmt, void* d_metrics, bool prepared) {
    uint32_t* const met_out = d_metrics ? static_cast<uint32_t*>(d_metrics) : a->d_metrics;
    // edge search: stage C sees H * D bins and writes the block of every hypothesis; the reduction at the end fills met_out
    const gm_acq::Edge& eg = a->edge;
    const bool edge = eg.H > 0;
    const uint32_t Dv = edge ? eg.H * a->D : a->D;
    uint32_t* met = edge ? eg.d_full : met_out;
    float* const planes = edge ? eg.d_planes : a->d_planes;
    const size_t PD = size_t(a->P) * Dv;
    const bool t = a->tm.on && (a->tm.calls++ % a->tm.stride == 0);
    a->tm.this_call = t;
    // a timed dwell measures its own kernels only: a decision still pending from the dwell before runs now, in front of the first
    // event, not as trailing workgroups of the timed stage F
    if (t) { if (int rc = acq_flush_decision(a)) return rc; }
    hipEvent_t* ev = t ? &a->tm.ev[size_t(a->tm.count % Timing::CAP) * 4] : nullptr;
    if (t) HIPC(hipEventRecord(ev[0], a->stream));
    gm_acq::Ahead& ah = a->ahead;
    bool tickets_cleared = a->d_split_counter != nullptr;
    if (prepared) {
        // the spectra were prepared (gm_acq_prepare_dev): take that buffer once its stage F is through; the tail split's tickets,
        // which the in-stream stage F clears on its way, are left to corr() (a memset, if it cuts the tail)
        if (int rc = acq_flush_decision(a)) return rc;
        ah.valid = false;
        std::swap(a->d_spectra, ah.d_spectra_alt);
        HIPC(hipStreamWaitEvent(a->stream, ah.ev_f, 0));
        tickets_cleared = false;
    } else if (a->drift.on || edge || a->K > 1) {
        // (with the drift compensation or the edge search on, never prepared: gm_acq_prepare_dev runs nothing ahead then; none of
        // these handles defers its decision)
        acq_stage_f_variant(a, a->stream, d_samples, fmt, edge ? eg.d_spectra : a->d_spectra, a->d_split_counter);
        a->dec_deferred = false;
    } else if (a->lng) {
        a->lng->fwd_sub(a->stream, d_samples, fmt, a->d_tables, nullptr, a->d_tw_fwd, a->d_spectra, a->D * a->M, a->Q, a->N, a->long_lim, a->M);
        gm::launch_long_fwd_post(a->stream, a->d_spectra, a->D * a->M, a->Q, a->Nb);
    } else if (a->Q == 1) {
        a->plan->mix_fft(a->stream, d_samples, fmt, a->d_tables, a->d_tw_mix, a->d_spectra, int(a->D), int(a->M), a->d_split_counter, a->d_order,
                         a->dec_deferred ? &a->dec_args : nullptr);
        a->dec_deferred = false;
    } else {
        // the sub-transforms ARE what the correlation kernel reads (comp_post_folded), else forward step 2 follows
        cf* sub = a->comp_post_folded ? a->d_spectra : a->d_comp_tmp;
        a->comp->fwd_sub(a->stream, d_samples, fmt, a->d_tables, nullptr, a->d_tw_mix, sub, a->D * a->M, a->M, a->d_order);
        if (!a->comp_post_folded) {
            a->comp->fwd_post(a->stream, a->d_comp_tmp, a->d_spectra, a->D * a->M, 1, a->d_order);
        }
    }
    if (t) HIPC(hipEventRecord(ev[1], a->stream));
    if (ah.side) HIPC(hipEventRecord(ah.ev_s, a->stream));
    cf* const spectra = edge ? eg.d_spectra : a->d_spectra;
    if (a->lng) {
        if (a->n_workers) {
            const size_t part = size_t(a->P) * Dv * a->Q;
            float* const lp = edge ? eg.d_long_part : a->d_long_part;
            gm::LongCorrArgs la{};
            la.spectra = spectra; la.code_fft = a->d_long_code; la.tw_inv = a->d_tw_inv; la.Z = a->d_long_z;
            la.pmax = lp; la.parg = reinterpret_cast<uint32_t*>(lp + part); la.psum = lp + 2 * part;
            la.mmax = reinterpret_cast<float*>(met); la.margmax = met + PD; la.msum = reinterpret_cast<float*>(met + 2 * PD);
            la.planes = planes; la.worker_list = a->d_worker_list;
            la.n_workers = a->n_workers; la.n_bins = Dv; la.n_int = a->M; la.Q = a->Q; la.Nb = a->Nb; la.N = a->N;
            la.slab_items = a->long_slab; la.scale = a->long_scale;
            gm::launch_long_corr(a->stream, a->lng, la, &a->last_grid);
            if (planes)      // strict_sum_order: the plane sums once more, in is_good_satellite's own order (:229-235)
                gm::launch_plane_strict_sum(a->stream, planes, reinterpret_cast<float*>(met + 2 * PD), a->d_worker_list, int(a->n_workers), int(Dv), uint32_t(a->N));
        }
    } else if (a->Q == 1) {
        a->plan->corr(a->stream, spectra, a->plan->code_paired ? a->d_code_fft_paired : a->d_code_fft, a->d_tw_inv, reinterpret_cast<float*>(met), met + PD,
                      reinterpret_cast<float*>(met + 2 * PD), a->d_worker_list, int(a->n_workers), int(Dv), int(a->M),
                      a->d_split_scratch, a->split_planes, a->d_split_counter, a->cfg.strict_sum_order ? 1 : 0, tickets_cleared ? 1 : 0,
                      a->cfg.reference_products ? 1 : 0, &a->last_grid);
    } else if (a->n_workers) {
        a->comp->corr(a->stream, spectra, a->d_code_comb, a->d_comp_twn, a->d_tw_inv, reinterpret_cast<float*>(met),
                      met + PD, reinterpret_cast<float*>(met + 2 * PD), a->d_worker_list, int(a->n_workers), int(Dv), int(a->M), planes,
                      &a->last_grid);
        if (planes)      // strict_sum_order: the plane sums once more, in is_good_satellite's own order (:229-235)
            gm::launch_plane_strict_sum(a->stream, planes, reinterpret_cast<float*>(met + 2 * PD), a->d_worker_list, int(a->n_workers), int(Dv), uint32_t(a->N));
    }
    if (edge) {       // per (worker, bin) cell the hypothesis with the largest max (lowest h on ties): its words, and h into the choice plane
        gm::launch_edge_reduce(a->stream, eg.d_full, met_out, eg.d_choice, a->d_worker_list, a->n_workers, a->P, eg.H, a->D);
        met = met_out;
    }
    if (t) { HIPC(hipEventRecord(ev[2], a->stream)); a->tm.count++; a->tm.decide_valid = false; }
    HIPC(hipGetLastError());
    a->last_metrics = met;
    a->last_samples = d_samples; a->last_fmt = fmt;
    return GM_OK;
}

int gm_acq_search_dev(gm_acq* a, const void* d_samples, int fmt, void* d_metrics) {
    if (!a || !d_samples) return set_err(GM_ERR_INVALID_ARG, "null handle/samples");
    if (fmt < GM_FMT_C32 || fmt > GM_FMT_I8_REAL) return set_err(GM_ERR_INVALID_ARG, "bad sample format");
    if (int rc = ensure_device(a->device)) return rc;
    // always from the samples as they are NOW: a preparation (gm_acq_prepare_dev) is never matched by address
    return acq_search_common(a, d_samples, fmt, d_metrics, false);
}

int gm_acq_search_prepared_dev(gm_acq* a, uint64_t token, void* d_metrics) {
    if (!a) return set_err(GM_ERR_INVALID_ARG, "null handle");
    gm_acq::Ahead& ah = a->ahead;
    if (!token || !ah.valid || ah.token != token)
        return set_err(GM_ERR_INVALID_ARG, "no such preparation (token stale, consumed, replaced or dropped)");
    if (int rc = ensure_device(a->device)) return rc;
    if (!acq_fused(a) || a->edge.H || a->drift.on) {       // composite and any-length sizes (and an edge search, and a drift handle) prepare nothing: the whole search runs now, from the samples named then,
        ah.valid = false;                   // behind what `ready_stream` held at the time of gm_acq_prepare_dev
        if (ah.comp_wait) { HIPC(hipStreamWaitEvent(a->stream, ah.ev_in, 0)); ah.comp_wait = false; }
        return acq_search_common(a, ah.samples, ah.fmt, d_metrics, false);
    }
    return acq_search_common(a, ah.samples, ah.fmt, d_metrics, true);
}

int gm_acq_drop_prepared(gm_acq* a) {
    if (!a) return set_err(GM_ERR_INVALID_ARG, "null handle");
    a->ahead.valid = false;                 // (a stage F still running on the side stream finishes into the spare buffer: harmless)
    return GM_OK;
}

int gm_acq_prepare_dev(gm_acq* a, const void* d_samples, int fmt, void* ready_stream, uint64_t* token) {
    if (!a || !d_samples || !token) return set_err(GM_ERR_INVALID_ARG, "null handle/samples/token");
    if (fmt < GM_FMT_C32 || fmt > GM_FMT_I8_REAL) return set_err(GM_ERR_INVALID_ARG, "bad sample format");
    *token = 0;
    gm_acq::Ahead& ah = a->ahead;
    if (int rc = ensure_device(a->device)) return rc;
    if (!acq_fused(a) || a->edge.H || a->drift.on) {       // composite and any-length sizes, and every size while the edge search or the drift compensation is on: nothing is prepared, gm_acq_search_prepared_dev does all of it —
        // but the ordering promise is the same: the samples are complete once the work queued on `ready_stream` so far has run, so
        // the event is recorded NOW and the search waits for it on the handle's stream (the token used to be handed
        // out before `ready_stream` was looked at)
        ah.valid = false; ah.comp_wait = false;
        if (ready_stream) {
            if (!ah.ev_in) HIPC(hipEventCreateWithFlags(&ah.ev_in, hipEventDisableTiming));
            HIPC(hipEventRecord(ah.ev_in, reinterpret_cast<hipStream_t>(ready_stream)));
            ah.comp_wait = true;
        }
        ah.valid = true; ah.samples = d_samples; ah.fmt = fmt; ah.token = *token = ah.next_token++;
        return GM_OK;
    }
    if (!ah.side) {
        // all four resources or none: a failure half-way must leave the handle as it was (a later call starts over)
        cf* buf = nullptr; hipStream_t side = nullptr; hipEvent_t e[3] = {nullptr, nullptr, nullptr};
        // lowest priority: its workgroups are wanted where stage C has none left to place (the idle CUs of its last round), not
        // beside stage C's first round on every CU — the dispatcher honours that only in part (N = 16368: 307.3 us per dwell at
        // normal priority, 304.7 at the lowest, before the ticket memset went: DESIGN_HISTORY R4 has the table)
        int least = 0, greatest = 0;
        hipError_t er = hipMalloc(&buf, size_t(a->D) * a->M * a->N * 8);
        if (er == hipSuccess) er = hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (er == hipSuccess) er = hipStreamCreateWithPriority(&side, hipStreamNonBlocking, gm::diag_int("GM_PREPARE_PRIORITY", least));
        for (int i = 0; i < 3 && er == hipSuccess; ++i) er = hipEventCreateWithFlags(&e[i], hipEventDisableTiming);
        if (er == hipSuccess) er = hipEventRecord(e[0], a->stream);      // first time: behind whatever the handle's stream holds so far
        if (er != hipSuccess) {
            for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x);
            if (side) (void)hipStreamDestroy(side);
            if (buf) (void)hipFree(buf);
            return set_err(GM_ERR_HIP, hipGetErrorString(er));
        }
        ah.d_spectra_alt = buf; ah.side = side; ah.ev_s = e[0]; ah.ev_f = e[1]; ah.ev_in = e[2];
    }
    // the buffer to fill was last read by a stage C in front of the most recent one: free at ev_s (an earlier, unclaimed
    // preparation is overwritten in stream order)
    HIPC(hipStreamWaitEvent(ah.side, ah.ev_s, 0));
    if (ready_stream) {                     // ... and the samples are complete once the work queued on `ready_stream` so far has run
        HIPC(hipEventRecord(ah.ev_in, reinterpret_cast<hipStream_t>(ready_stream)));
        HIPC(hipStreamWaitEvent(ah.side, ah.ev_in, 0));
    }
    ah.valid = false;
    if (a->K > 1)
        acq_stage_f_variant(a, ah.side, d_samples, fmt, ah.d_spectra_alt, nullptr);
    else
        a->plan->mix_fft(ah.side, d_samples, fmt, a->d_tables, a->d_tw_mix, ah.d_spectra_alt, int(a->D), int(a->M), nullptr, a->d_order, nullptr);
    HIPC(hipEventRecord(ah.ev_f, ah.side));
    HIPC(hipGetLastError());
    ah.valid = true; ah.samples = d_samples; ah.fmt = fmt; ah.token = *token = ah.next_token++;
    return GM_OK;
}

int gm_acq_decide_dev(gm_acq* a, const void* d_metrics, uint32_t n_prn, const uint8_t* prn_ids, uint64_t local_tail) {
    if (!a || !n_prn) return set_err(GM_ERR_INVALID_ARG, "null handle / n_prn == 0");
    if (a->D > GM_ACQ_DECIDE_MAX_BINS) return set_err(GM_ERR_OUT_OF_RANGE, DECIDE_BINS_MSG);
    if (int rc = ensure_device(a->device)) return rc;
    if (int rc = acq_flush_decision(a)) return rc;
    if (int rc = acq_reserve_results(a, n_prn)) return rc;
    const uint32_t* met = d_metrics ? static_cast<const uint32_t*>(d_metrics) : a->d_metrics;
    const uint8_t* ids = prn_ids ? prn_ids : (n_prn == a->P ? a->prn_ids.data() : nullptr);
    if (!ids) return set_err(GM_ERR_INVALID_ARG, "prn_ids required when n_prn differs from the handle's");
    if (a->dev_prn_ids.size() != n_prn || memcmp(a->dev_prn_ids.data(), ids, n_prn) != 0) {   // upload only on change
        a->dev_prn_ids.assign(ids, ids + n_prn);
        HIPC(hipMemcpyAsync(a->d_prn_ids, a->dev_prn_ids.data(), n_prn, hipMemcpyHostToDevice, a->stream));
        HIPC(hipStreamSynchronize(a->stream));
    }
    const size_t PD = size_t(n_prn) * a->D;
    gm::DecideArgs da;
    da.mmax = reinterpret_cast<const float*>(met);
    da.margmax = met + PD;
    da.msum = reinterpret_cast<const float*>(met + 2 * PD);
    da.table_freq = a->d_table_freq;
    da.prn_ids = a->d_prn_ids;
    da.mask_lo = (d_metrics && n_prn != a->P) ? ~0ull : a->mask;
    da.n_prn = int(n_prn); da.n_bins = int(a->D); da.fft_size = int(a->N);
    da.fs = a->cfg.fs; da.threshold = a->cfg.threshold; da.code_rate = a->code_rate;
    da.best_bin_mode = a->cfg.decision_mode == GM_DECIDE_BEST_BIN ? 1 : 0;
    da.local_tail = local_tail;
    da.results = a->d_results; da.found = a->d_found;
    if (a->defer_decisions && acq_fused(a) && a->K == 1 && !a->drift.on && !(a->tm.on && a->tm.this_call) && met == a->last_metrics && a->D <= 64) {
        a->dec_args = da;          // runs with the next gm_acq_search_dev's stage F, or at the next flush point
        a->dec_deferred = true;
        return GM_OK;
    }
    gm::launch_decide(a->stream, da);
    if (a->tm.on && a->tm.this_call && a->tm.count > 0) {
        a->tm.this_call = false;
        HIPC(hipEventRecord(a->tm.ev[size_t((a->tm.count - 1) % Timing::CAP) * 4 + 3], a->stream));
        a->tm.decide_valid = true;
    }
    HIPC(hipGetLastError());
    return GM_OK;
}

int gm_acq_synchronize(gm_acq* a) {
    if (!a) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (int rc = ensure_device(a->device)) return rc;
    if (int rc = acq_flush_decision(a)) return rc;
    HIPC(hipStreamSynchronize(a->stream));
    return GM_OK;
}

int gm_acq_set_deferred_decision(gm_acq* a, int on) {
    if (!a) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (!on && a->dec_deferred) { if (int rc = ensure_device(a->device)) return rc; if (int rc = acq_flush_decision(a)) return rc; }
    a->defer_decisions = on != 0;
    return GM_OK;
}

int gm_acq_fetch_results(gm_acq* a, uint32_t n_prn, gm_acq_result* results, uint8_t* found) {
    if (!a || !results || !found) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (n_prn > a->results_cap) return set_err(GM_ERR_INVALID_ARG, "n_prn exceeds the last decide call");
    if (int rc = ensure_device(a->device)) return rc;
    if (int rc = acq_flush_decision(a)) return rc;
    HIPC(hipStreamSynchronize(a->stream));          // decide_kernel's stores to the pinned block are visible once its stream has drained
    memcpy(results, a->d_results, sizeof(gm_acq_result) * n_prn);
    memcpy(found, a->d_found, n_prn);
    return GM_OK;
}

int gm_acq_search(gm_acq* a, const void* samples, size_t n_samples, int fmt, uint64_t local_tail, uint64_t prn_mask,
                  gm_acq_result* results, uint8_t* found) {
    if (!a || !samples || !results || !found) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (fmt < GM_FMT_C32 || fmt > GM_FMT_I8_REAL) return set_err(GM_ERR_INVALID_ARG, "bad sample format");
    const size_t need = acq_dwell_samples(a);
    if (n_samples < need)
        return set_err(GM_ERR_OUT_OF_RANGE, a->drift.on ? "samples_chunk shorter than gm_acq_dwell_samples (code drift: up to the end of the last compensated period)"
                                            : a->edge.H ? "samples_chunk shorter than (coherent_periods*num_integrations + the last edge offset)*fft_size"
                                                      : "samples_chunk shorter than coherent_periods*num_integrations*fft_size");
    if (int rc = ensure_device(a->device)) return rc;
    const size_t bps = fmt_bytes(fmt);
    if (int rc = acq_set_mask(a, prn_mask)) return rc;
    HIPC(hipMemcpyAsync(a->d_samples, samples, need * bps, hipMemcpyHostToDevice, a->stream));   // (a pinned staging block of the handle's own: measured, no gain)
    if (int rc = gm_acq_search_dev(a, a->d_samples, fmt, nullptr)) return rc;
    if (int rc = gm_acq_decide_dev(a, nullptr, a->P, nullptr, local_tail)) return rc;
    return gm_acq_fetch_results(a, a->P, results, found);
}

// run()'s snapshot + search (do_acquisition.rs:297-313) against the DEVICE ring: the coherent_periods*n_integrations*fft_size
// samples ending at `head` (local_tail = head - K*M*N) are copied device-to-device (wrap-aware, like
// copy_to_slice :107-129) and searched; no host round trip of the samples.
int gm_acq_search_ring(gm_acq* a, gm_ring* ring, uint64_t prn_mask, gm_acq_result* results, uint8_t* found,
                       uint64_t* local_tail_out) {
    if (!a || !ring || !results || !found) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (a->device != ring->device) return set_err(GM_ERR_INVALID_ARG, "ring lives on another device");
    const size_t need = acq_dwell_samples(a);     // (edge search: K*M + the last offset periods; drift: to the end of the last period)
    if (need > ring->size) return set_err(GM_ERR_OUT_OF_RANGE, "ring smaller than the dwell (coherent_periods*num_integrations*fft_size; gm_acq_dwell_samples)");
    if (int rc = ensure_device(ring->device)) return rc;
    ring_refresh_head(ring);
    const uint64_t head = ring->head.load(std::memory_order_acquire);
    if ((int64_t)(head - need) < 0) return set_err(GM_ERR_OUT_OF_RANGE, "not enough samples yet (head < K*M*N)");   // :299
    if (int rc = ensure_device(a->device)) return rc;
    const uint64_t local_tail = head - need;
    const size_t ps = size_t(local_tail & ring->mask);
    cf* dst = static_cast<cf*>(a->d_samples);
    if (ps + need <= ring->size) {
        HIPC(hipMemcpyAsync(dst, ring->d_buf + ps, need * 8, hipMemcpyDeviceToDevice, a->stream));
    } else {
        const size_t first = ring->size - ps;
        HIPC(hipMemcpyAsync(dst, ring->d_buf + ps, first * 8, hipMemcpyDeviceToDevice, a->stream));
        HIPC(hipMemcpyAsync(dst + first, ring->d_buf, (need - first) * 8, hipMemcpyDeviceToDevice, a->stream));
    }
    if (int rc = acq_set_mask(a, prn_mask)) return rc;
    if (int rc = gm_acq_search_dev(a, a->d_samples, GM_FMT_C32, nullptr)) return rc;
    if (int rc = gm_acq_decide_dev(a, nullptr, a->P, nullptr, local_tail)) return rc;
    if (local_tail_out) *local_tail_out = local_tail;
    return gm_acq_fetch_results(a, a->P, results, found);
}

// Fine Doppler: finer_doppler (acquisition_bk.rs:215-302, legacy) for every found result of the last
// search, on the snapshot that search used (still resident in HBM).  fft_size = 8 * next_pow2((K*M-1)*N) as N1 x N2 (K: coherent_periods).
int gm_acq_finer_doppler(gm_acq* a, const gm_acq_result* results, const uint8_t* found, uint32_t n_prn, float* fine_freq_hz,
                         uint64_t* peak_index, float* peak_mag, uint64_t* fft_size_out) {
    if (!a || !results || !found) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (n_prn > a->P) return set_err(GM_ERR_INVALID_ARG, "n_prn exceeds the handle's workers");
    const uint32_t periods = a->K * a->M;                                // the snapshot: K*M periods
    if (periods < 2) return set_err(GM_ERR_INVALID_ARG, "fine Doppler needs coherent_periods*num_integrations >= 2 ((K*M-1)*N samples after the code phase)");
    if (!a->last_samples) return set_err(GM_ERR_INVALID_ARG, "no search has run on this handle yet");
    if (int rc = ensure_device(a->device)) return rc;
    gm_acq::Fine& f = a->fine;
    if (uint64_t(periods - 1) * a->N > (1ull << 21)) return set_err(GM_ERR_UNSUPPORTED_N, "fine-Doppler FFT longer than 2^24");
    const uint32_t size_use = (periods - 1) * a->N;                      // :240
    if (!f.p1) {
        uint64_t p2 = 1;
        while (p2 < size_use) p2 <<= 1;                                  // next_power_of_two :249
        const uint64_t n = 8 * p2;
        if (n > (1ull << 24)) return set_err(GM_ERR_UNSUPPORTED_N, "fine-Doppler FFT longer than 2^24");
        // N = N1 * N2 with both factors among the power-of-two in-LDS plans, as square as possible
        int lg = 0;
        while ((1ull << lg) < n) ++lg;
        const gm::PlanOps *b1 = nullptr, *b2 = nullptr;
        for (int l2 = lg / 2; l2 >= 8 && !b1; --l2) {
            const gm::PlanOps *q1 = gm::find_plan(1 << (lg - l2)), *q2 = gm::find_plan(1 << l2);
            if (q1 && q2 && q1->fine_cols && q2->fine_rows) { b1 = q1; b2 = q2; }
        }
        if (!b1) return set_err(GM_ERR_UNSUPPORTED_N, "no pair of in-LDS plans factors the fine-Doppler FFT size");
        std::vector<cf> t1(size_t(b1->tw_total) + 1), t2(size_t(b2->tw_total) + 1);
        b1->fill_tw(t1.data(), false);
        b2->fill_tw(t2.data(), false);
        HIPC(hipMalloc(&f.d_tw1, t1.size() * 8));
        HIPC(hipMalloc(&f.d_tw2, t2.size() * 8));
        HIPC(hipMemcpy(f.d_tw1, t1.data(), t1.size() * 8, hipMemcpyHostToDevice));
        HIPC(hipMemcpy(f.d_tw2, t2.data(), t2.size() * 8, hipMemcpyHostToDevice));
        HIPC(hipMalloc(&f.d_chips, a->chips.size()));
        HIPC(hipMemcpy(f.d_chips, a->chips.data(), a->chips.size(), hipMemcpyHostToDevice));
        HIPC(hipMalloc(&f.d_mean, 2 * sizeof(float)));
        f.p1 = b1; f.p2 = b2; f.size_use = size_use;
    }
    const uint32_t N1 = uint32_t(f.p1->n), N2 = uint32_t(f.p2->n);
    if (fft_size_out) *fft_size_out = uint64_t(N1) * N2;
    // edge search: every found worker is refined on the K*M periods its winning hypothesis searched, i.e. from period o* on (whole
    // periods do not move the code phase) — one pass per distinct offset among the found workers; without it one pass at offset 0
    std::vector<uint32_t> off(n_prn, 0u);
    if (a->edge.H)
        if (int rc = gm_acq_result_offsets(a, results, found, n_prn, off.data())) return rc;
    std::vector<uint32_t> passes;
    for (uint32_t p = 0; p < n_prn; ++p)
        if (found[p] && std::find(passes.begin(), passes.end(), off[p]) == passes.end()) passes.push_back(off[p]);
    const size_t bps = fmt_bytes(a->last_fmt);
    // (not compensated: the code is stripped over K*M contiguous periods from period o* on; a drift dwell of periods shorter than
    //  fft_size ends before them — checked for the largest offset before any pass runs, so no output is half filled)
    if (a->drift.on && !passes.empty() &&
        (uint64_t(*std::max_element(passes.begin(), passes.end())) + periods) * a->N > a->drift.dwell)
        return set_err(GM_ERR_OUT_OF_RANGE, "the code-drift dwell is shorter than the contiguous periods the fine Doppler reads (it is not compensated)");
    // a code phase lies inside one period: cp + (K*M-1)*N then stays inside the K*M periods a pass reads (:260 would panic beyond
    // them); checked for every found worker before any pass runs, so no output is half filled
    for (uint32_t p = 0; p < n_prn; ++p)
        if (found[p] && results[p].code_phase_samples >= a->N)
            return set_err(GM_ERR_OUT_OF_RANGE, "result.code_phase_samples is not below fft_size");
    for (const uint32_t o_star : passes) {
    const void* const snap = static_cast<const char*>(a->last_samples) + size_t(o_star) * a->N * bps;
    std::vector<uint32_t> workers, cps, slot(n_prn, 0xFFFFFFFFu);
    for (uint32_t p = 0; p < n_prn; ++p) {
        if (!found[p] || off[p] != o_star) continue;
        slot[p] = uint32_t(workers.size());
        workers.push_back(p);
        cps.push_back(uint32_t(results[p].code_phase_samples));
    }
    const uint32_t S = uint32_t(workers.size());
    if (S > f.sats_cap) {
        hipFree(f.d_B); hipFree(f.d_rowmax); hipFree(f.d_rowarg); hipFree(f.d_sat_worker); hipFree(f.d_sat_cp);
        hipFree(f.d_peak_pow); hipFree(f.d_peak_idx);
        f.d_B = nullptr; f.sats_cap = 0;
        HIPC(hipMalloc(&f.d_B, size_t(S) * N1 * N2 * 8));
        HIPC(hipMalloc(&f.d_rowmax, size_t(S) * N1 * 4));
        HIPC(hipMalloc(&f.d_rowarg, size_t(S) * N1 * 4));
        HIPC(hipMalloc(&f.d_sat_worker, S * 4));
        HIPC(hipMalloc(&f.d_sat_cp, S * 4));
        HIPC(hipMalloc(&f.d_peak_pow, S * 4));
        HIPC(hipMalloc(&f.d_peak_idx, S * 4));
        f.sats_cap = S;
    }
    HIPC(hipMemcpyAsync(f.d_sat_worker, workers.data(), S * 4, hipMemcpyHostToDevice, a->stream));
    HIPC(hipMemcpyAsync(f.d_sat_cp, cps.data(), S * 4, hipMemcpyHostToDevice, a->stream));
    gm::FineArgs fa{};
    fa.samples = snap; fa.fmt = a->last_fmt; fa.mean = f.d_mean;
    fa.chips = f.d_chips; fa.code_len = a->code_len; fa.code_rate = a->code_rate; fa.fs = a->cfg.fs;
    fa.sat_worker = f.d_sat_worker; fa.sat_code_phase = f.d_sat_cp;
    fa.size_use = size_use; fa.N1 = N1; fa.N2 = N2; fa.B = f.d_B; fa.tw1 = f.d_tw1; fa.tw2 = f.d_tw2;
    fa.rowmax = f.d_rowmax; fa.rowarg = f.d_rowarg;
    gm::launch_fine_mean(a->stream, snap, a->last_fmt, periods * a->N, f.d_mean);
    f.p1->fine_cols(a->stream, fa, int(S));
    f.p2->fine_rows(a->stream, fa, int(S));
    gm::launch_fine_final(a->stream, f.d_rowmax, f.d_rowarg, N1 / uint32_t(f.p2->fine_rows_per_wg), int(S), f.d_peak_pow, f.d_peak_idx);
    HIPC(hipGetLastError());
    std::vector<float> pw(S);
    std::vector<uint32_t> pi(S);
    HIPC(hipMemcpyAsync(pw.data(), f.d_peak_pow, S * 4, hipMemcpyDeviceToHost, a->stream));
    HIPC(hipMemcpyAsync(pi.data(), f.d_peak_idx, S * 4, hipMemcpyDeviceToHost, a->stream));
    HIPC(hipStreamSynchronize(a->stream));
    const uint64_t fft_size = uint64_t(N1) * N2;
    const uint64_t one_side = uint64_t(ceilf((float(fft_size) + 1.0f) / 2.0f));       // :250
    for (uint32_t p = 0; p < n_prn; ++p) {
        if (slot[p] == 0xFFFFFFFFu) continue;
        const uint64_t idx = pi[slot[p]];
        if (peak_index) peak_index[p] = idx;
        if (peak_mag) peak_mag[p] = sqrtf(pw[slot[p]]);
        if (fine_freq_hz)   // :251-253; the upper half is where the legacy indexes out of bounds (:285-288): negative frequency
            fine_freq_hz[p] = idx > one_side ? -((float(fft_size - idx) * a->cfg.fs) / float(fft_size))
                                             : (float(idx) * a->cfg.fs) / float(fft_size);
    }
    }     // passes
    return GM_OK;
}

int gm_acq_search_c32(gm_acq* a, const gm_c32* s, size_t n, uint64_t tail, uint64_t mask, gm_acq_result* r, uint8_t* f) {
    return gm_acq_search(a, s, n, GM_FMT_C32, tail, mask, r, f);
}
int gm_acq_search_i8(gm_acq* a, const int8_t* s, size_t n, uint64_t tail, uint64_t mask, gm_acq_result* r, uint8_t* f) {
    return gm_acq_search(a, s, n, GM_FMT_I8_IQ, tail, mask, r, f);
}

int gm_acq_metrics(gm_acq* a, float* mx, uint32_t* am, float* sm) {
    if (!a) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (int rc = ensure_device(a->device)) return rc;
    HIPC(hipStreamSynchronize(a->stream));
    const size_t PD = size_t(a->P) * a->D;
    const uint32_t* met = a->last_metrics ? static_cast<const uint32_t*>(a->last_metrics) : a->d_metrics;
    if (mx) HIPC(hipMemcpy(mx, met, PD * 4, hipMemcpyDeviceToHost));
    if (am) HIPC(hipMemcpy(am, met + PD, PD * 4, hipMemcpyDeviceToHost));
    if (sm) HIPC(hipMemcpy(sm, met + 2 * PD, PD * 4, hipMemcpyDeviceToHost));
    return GM_OK;
}

int gm_acq_code_fft(gm_acq* a, uint32_t worker, gm_c32* out) {
    if (!a || !out || worker >= a->P) return set_err(GM_ERR_INVALID_ARG, "bad worker index");
    if (int rc = ensure_device(a->device)) return rc;
    // natural order at every size (the composite path keeps blocks k1*Nb + k2 in natural order too)
    HIPC(hipMemcpy(out, a->d_code_fft + size_t(worker) * a->N, size_t(a->N) * 8, hipMemcpyDeviceToHost));
    return GM_OK;
}

int gm_acq_tables(gm_acq* a, gm_c32* tables, float* freq) {
    if (!a) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (int rc = ensure_device(a->device)) return rc;
    if (tables) HIPC(hipMemcpy(tables, a->d_tables, size_t(a->D) * a->N * 8, hipMemcpyDeviceToHost));
    if (freq) memcpy(freq, a->table_freq.data(), a->D * sizeof(float));
    return GM_OK;
}

int gm_acq_coherent_phasors(gm_acq* a, gm_c32* out) {
    if (!a || !out) return set_err(GM_ERR_INVALID_ARG, "null handle/out");
    if (int rc = ensure_device(a->device)) return rc;
    HIPC(hipMemcpy(out, a->d_rho, size_t(a->D) * a->K * 8, hipMemcpyDeviceToHost));
    return GM_OK;
}

static int drift_build(const gm_acq* a, uint32_t n_offsets, const uint32_t* offsets, const double* T, gm_acq::Drift& out);

// ---------------------------------------------------------------- edge search (additive entries, ABI 9)
// the argument rules of gm_acq_edge_dwell_periods / gm_acq_set_edge_search; *neg: bit k set where secondary[k] = -1
static int edge_check(uint32_t K, uint32_t n, const uint32_t* offsets, const int8_t* secondary, uint32_t* neg) {
    if (K < 2) return set_err(GM_ERR_INVALID_ARG, "the edge search needs a coherent handle (coherent_periods >= 2)");
    if (K > uint32_t(gm::GM_COHERENT_MAX)) return set_err(GM_ERR_INVALID_ARG, "coherent_periods > 32");
    if (n > 32) return set_err(GM_ERR_INVALID_ARG, "more than 32 edge offsets");
    if (!offsets) return set_err(GM_ERR_INVALID_ARG, "null offsets");
    for (uint32_t h = 0; h < n; ++h) {
        if (offsets[h] > 63) return set_err(GM_ERR_INVALID_ARG, "edge offset above 63 periods");
        if (h && offsets[h] <= offsets[h - 1]) return set_err(GM_ERR_INVALID_ARG, "edge offsets must ascend strictly");
    }
    *neg = 0;
    if (secondary)
        for (uint32_t k = 0; k < K; ++k) {
            if (secondary[k] != 1 && secondary[k] != -1) return set_err(GM_ERR_INVALID_ARG, "secondary row entries must be +1 or -1");
            if (secondary[k] < 0) *neg |= 1u << k;
        }
    return GM_OK;
}

int gm_acq_edge_dwell_periods(uint32_t coherent_periods, uint32_t n_integrations, uint32_t n_offsets, const uint32_t* offsets,
                              const int8_t* secondary, uint64_t* dwell_periods) {
    if (!dwell_periods || !n_integrations) return set_err(GM_ERR_INVALID_ARG, "null dwell_periods / n_integrations == 0");
    const uint32_t K = coherent_periods > 1 ? coherent_periods : 1;
    if (!n_offsets) {                       // the edge search off: the handle's own dwell
        if (K > uint32_t(gm::GM_COHERENT_MAX)) return set_err(GM_ERR_INVALID_ARG, "coherent_periods > 32");
        *dwell_periods = uint64_t(K) * n_integrations;
        return GM_OK;
    }
    uint32_t neg = 0;
    if (int rc = edge_check(K, n_offsets, offsets, secondary, &neg)) return rc;
    *dwell_periods = uint64_t(K) * n_integrations + offsets[n_offsets - 1];
    return GM_OK;
}

int gm_acq_set_edge_search(gm_acq* a, uint32_t n_offsets, const uint32_t* offsets, const int8_t* secondary) {
    if (!a) return set_err(GM_ERR_INVALID_ARG, "null handle");
    uint32_t neg = 0;
    if (n_offsets)
        if (int rc = edge_check(a->K, n_offsets, offsets, secondary, &neg)) return rc;
    if (int rc = ensure_device(a->device)) return rc;
    if (int rc = acq_flush_decision(a)) return rc;
    a->ahead.valid = false;                 // an outstanding preparation is dropped: its token becomes stale
    a->ahead.comp_wait = false;
    HIPC(hipStreamSynchronize(a->stream));
    if (!n_offsets) {
        if (a->drift.on && a->edge.H) {     // the compensation is planned again for the shorter dwell before the edge search goes
            gm_acq::Drift nd;
            if (int rc = drift_build(a, 0, nullptr, a->drift.T.data(), nd)) return rc;
            acq_drift_free(a->drift);
            a->drift = std::move(nd);
        }
        if (a->edge.H) a->last_samples = nullptr;
        acq_edge_free(a->edge);
        return GM_OK;
    }
    gm_acq::Edge e;
    e.H = n_offsets; e.offsets.assign(offsets, offsets + n_offsets); e.o_max = offsets[n_offsets - 1]; e.neg = neg;
    e.fwd = acq_find_stage_f<gm::EdgeLoad>(a);
    if (!e.fwd) return set_err(GM_ERR_UNSUPPORTED_N, "no edge-search stage F for this handle's base plan");
    const size_t H = n_offsets, D = a->D, M = a->M, P = a->P, N = a->N, T = a->lng ? size_t(a->L) : N;
    // everything new is allocated before anything old goes: a failure leaves the handle as it was
    void* smp = nullptr;
    size_t smp_bytes = (size_t(a->K) * M + e.o_max) * N * 8;
    gm_acq::Drift nd;                       // code-drift compensation on: planned again for the new hypotheses
    if (a->drift.on) {
        if (int rc = drift_build(a, n_offsets, offsets, a->drift.T.data(), nd)) return rc;
        // (the larger of the two dwells: the compensation may be switched off later, and the buffer must then hold the plain dwell)
        if (size_t(nd.dwell) * 8 > smp_bytes) smp_bytes = size_t(nd.dwell) * 8;
    }
    bool ok = hipMalloc(&e.d_offsets, H * 4) == hipSuccess && hipMalloc(&e.d_spectra, H * D * M * T * 8) == hipSuccess &&
              hipMalloc(&e.d_full, 3 * P * H * D * 4) == hipSuccess && hipMalloc(&e.d_choice, P * D * 4) == hipSuccess;
    if (ok && a->Q > 1 && !a->lng && !a->comp_post_folded) ok = hipMalloc(&e.d_tmp, H * D * M * N * 8) == hipSuccess;
    if (ok && a->lng) ok = hipMalloc(&e.d_long_part, 3 * P * H * D * a->Q * 4) == hipSuccess;
    if (ok && a->d_planes) ok = hipMalloc(&e.d_planes, P * H * D * N * sizeof(float)) == hipSuccess;
    if (ok && smp_bytes > a->samples_cap) ok = hipMalloc(&smp, smp_bytes) == hipSuccess;
    if (ok) ok = hipMemset(e.d_full, 0, 3 * P * H * D * 4) == hipSuccess && hipMemset(e.d_choice, 0, P * D * 4) == hipSuccess &&
                 hipMemcpy(e.d_offsets, e.offsets.data(), H * 4, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        hipFree(smp);
        acq_edge_free(e);
        acq_drift_free(nd);
        return set_err(GM_ERR_NOMEM, "the edge search's buffers do not fit (gnss_mi355x.h states the formula); the handle is as it was");
    }
    if (smp) { hipFree(a->d_samples); a->d_samples = smp; a->samples_cap = smp_bytes; }
    acq_edge_free(a->edge);
    a->edge = std::move(e);
    if (nd.on) { acq_drift_free(a->drift); a->drift = std::move(nd); }
    a->last_samples = nullptr;              // (gm_acq_finer_doppler: the next search's snapshot)
    return GM_OK;
}

int gm_acq_edge_metrics(gm_acq* a, float* mx, uint32_t* am, float* sm) {
    if (!a) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (!a->edge.H) return set_err(GM_ERR_INVALID_ARG, "the edge search is off (gm_acq_set_edge_search)");
    if (int rc = ensure_device(a->device)) return rc;
    HIPC(hipStreamSynchronize(a->stream));
    const size_t n = size_t(a->P) * a->edge.H * a->D;
    if (mx) HIPC(hipMemcpy(mx, a->edge.d_full, n * 4, hipMemcpyDeviceToHost));
    if (am) HIPC(hipMemcpy(am, a->edge.d_full + n, n * 4, hipMemcpyDeviceToHost));
    if (sm) HIPC(hipMemcpy(sm, a->edge.d_full + 2 * n, n * 4, hipMemcpyDeviceToHost));
    return GM_OK;
}

int gm_acq_edge_choice(gm_acq* a, uint32_t* hypothesis) {
    if (!a || !hypothesis) return set_err(GM_ERR_INVALID_ARG, "null handle/out");
    if (!a->edge.H) return set_err(GM_ERR_INVALID_ARG, "the edge search is off (gm_acq_set_edge_search)");
    if (int rc = ensure_device(a->device)) return rc;
    HIPC(hipStreamSynchronize(a->stream));
    HIPC(hipMemcpy(hypothesis, a->edge.d_choice, size_t(a->P) * a->D * 4, hipMemcpyDeviceToHost));
    return GM_OK;
}

int gm_acq_result_offsets(gm_acq* a, const gm_acq_result* results, const uint8_t* found, uint32_t n_prn, uint32_t* offset_periods) {
    if (!a || !results || !found || !offset_periods) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (!a->edge.H) return set_err(GM_ERR_INVALID_ARG, "the edge search is off (gm_acq_set_edge_search)");
    if (n_prn > a->P) return set_err(GM_ERR_INVALID_ARG, "n_prn exceeds the handle's workers");
    std::vector<uint32_t> choice(size_t(a->P) * a->D);
    if (int rc = gm_acq_edge_choice(a, choice.data())) return rc;
    for (uint32_t p = 0; p < n_prn; ++p) {
        if (!found[p]) continue;
        const int32_t d = results[p].doppler_bin;
        if (d < 0 || uint32_t(d) >= a->D) return set_err(GM_ERR_OUT_OF_RANGE, "result.doppler_bin outside the handle's bins");
        const uint32_t h = choice[size_t(p) * a->D + uint32_t(d)];
        offset_periods[p] = a->edge.offsets[h < a->edge.H ? h : 0];
    }
    return GM_OK;
}

// ---------------------------------------------------------------- code-drift compensation (additive entries, ABI 9)
// the argument rules of gm_acq_code_drift_plan / gm_acq_set_code_drift: every T finite and within 8 samples of fft_size
static int drift_check(uint32_t N, uint32_t n_bins, const double* T) {
    if (!N || N % 8) return set_err(GM_ERR_INVALID_ARG, "fft_size must be a positive multiple of 8");
    if (!n_bins || !T) return set_err(GM_ERR_INVALID_ARG, "null period_samples / n_bins == 0");
    for (uint32_t d = 0; d < n_bins; ++d)
        if (!(::fabs(T[d] - double(N)) <= 8.0)) return set_err(GM_ERR_INVALID_ARG, "period_samples must be within 8 samples of fft_size");   // (NaN fails too)
    return GM_OK;
}
// s[d][p] = floor(p T_d + 0.5), p < R, in f64; -> the dwell: max_d s[d][R - 1] + N
static uint64_t drift_starts(uint32_t N, uint32_t R, uint32_t n_bins, const double* T, uint64_t* starts) {
    uint64_t last = 0;
    for (uint32_t d = 0; d < n_bins; ++d)
        for (uint32_t p = 0; p < R; ++p) {
            const uint64_t s = uint64_t(::floor(double(p) * T[d] + 0.5));
            if (starts) starts[size_t(d) * R + p] = s;
            if (p == R - 1 && s > last) last = s;
        }
    return last + N;
}

int gm_acq_code_drift_plan(uint32_t fft_size, uint32_t n_periods, uint32_t n_bins, const double* period_samples, uint64_t* starts,
                           uint64_t* dwell_samples) {
    if (!dwell_samples || !n_periods) return set_err(GM_ERR_INVALID_ARG, "null dwell_samples / n_periods == 0");
    if (int rc = drift_check(fft_size, n_bins, period_samples)) return rc;
    *dwell_samples = drift_starts(fft_size, n_periods, n_bins, period_samples, starts);
    return GM_OK;
}

// plans the compensation of handle `a` for the periods T under the edge search (n_offsets, offsets) — 0: none — into `out`, device
// memory included; nothing of the handle changes.  GM_ERR_NOMEM leaves `out` empty.
static int drift_build(const gm_acq* a, uint32_t n_offsets, const uint32_t* offsets, const double* T, gm_acq::Drift& out) {
    const size_t D = a->D, M = a->M, K = a->K, H = n_offsets ? n_offsets : 1;
    gm_acq::Drift dr;
    dr.on = true;
    dr.T.assign(T, T + D);
    dr.R = uint32_t(K * M) + (n_offsets ? offsets[n_offsets - 1] : 0u);
    dr.starts.resize(D * dr.R);
    dr.dwell = drift_starts(a->N, dr.R, a->D, dr.T.data(), dr.starts.data());
    dr.fwd = acq_find_stage_f<gm::DriftLoad>(a);
    if (!dr.fwd) return set_err(GM_ERR_UNSUPPORTED_N, "no code-drift stage F for this handle's base plan");
    // the phasor words, as gm_acq_create forms the plain fold's: bin d's table phasor continued over the samples from the group's first
    // period to period k's real start — f64, the phase reduced to one cycle, rounded to f32 (T = fft_size: the plain fold's words)
    std::vector<gm_c32> rho(H * D * M * K);
    for (size_t h = 0; h < H; ++h)
        for (size_t d = 0; d < D; ++d)
            for (size_t m = 0; m < M; ++m) {
                const uint64_t* s = &dr.starts[d * dr.R + (n_offsets ? offsets[h] : 0u) + m * K];
                for (size_t k = 0; k < K; ++k) {
                    const double cyc = double(a->table_freq[d]) * double(s[k] - s[0]) / double(a->cfg.fs);
                    const double ang = 2.0 * 3.14159265358979323846 * (cyc - ::floor(cyc));
                    rho[((h * D + d) * M + m) * K + k] = gm_c32{float(::cos(ang)), float(0.0 - ::sin(ang))};
                }
            }
    const bool ok = hipMalloc(&dr.d_starts, dr.starts.size() * 8) == hipSuccess && hipMalloc(&dr.d_rho, rho.size() * 8) == hipSuccess &&
                    hipMemcpy(dr.d_starts, dr.starts.data(), dr.starts.size() * 8, hipMemcpyHostToDevice) == hipSuccess &&
                    hipMemcpy(dr.d_rho, rho.data(), rho.size() * 8, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        acq_drift_free(dr);
        return set_err(GM_ERR_NOMEM, "the code-drift tables do not fit (gnss_mi355x.h states the formula); the handle is as it was");
    }
    out = std::move(dr);
    return GM_OK;
}

int gm_acq_set_code_drift(gm_acq* a, uint32_t n_bins, const double* period_samples) {
    if (!a) return set_err(GM_ERR_INVALID_ARG, "null handle");
    const bool off = !n_bins || !period_samples;
    if (!off) {
        if (n_bins != a->D) return set_err(GM_ERR_INVALID_ARG, "n_bins differs from the handle's");
        if (int rc = drift_check(a->N, n_bins, period_samples)) return rc;
    }
    if (int rc = ensure_device(a->device)) return rc;
    if (int rc = acq_flush_decision(a)) return rc;
    a->ahead.valid = false;                 // an outstanding preparation is dropped: its token becomes stale
    a->ahead.comp_wait = false;
    HIPC(hipStreamSynchronize(a->stream));
    if (off) {
        if (a->drift.on) a->last_samples = nullptr;
        acq_drift_free(a->drift);
        return GM_OK;
    }
    // everything new is allocated before anything old goes: a failure leaves the handle as it was
    gm_acq::Drift nd;
    if (int rc = drift_build(a, a->edge.H, a->edge.H ? a->edge.offsets.data() : nullptr, period_samples, nd)) return rc;
    void* smp = nullptr;
    // (the buffer never holds less than the dwell without the compensation: switching it off releases tables only)
    const size_t plain_bytes = acq_dwell_periods(a) * a->N * 8;
    const size_t smp_bytes = size_t(nd.dwell) * 8 > plain_bytes ? size_t(nd.dwell) * 8 : plain_bytes;
    if (smp_bytes > a->samples_cap && hipMalloc(&smp, smp_bytes) != hipSuccess) {
        (void)hipGetLastError();
        acq_drift_free(nd);
        return set_err(GM_ERR_NOMEM, "the code-drift dwell's sample buffer does not fit (gnss_mi355x.h states the formula); the handle is as it was");
    }
    if (smp) { hipFree(a->d_samples); a->d_samples = smp; a->samples_cap = smp_bytes; }
    acq_drift_free(a->drift);
    a->drift = std::move(nd);
    a->last_samples = nullptr;              // (gm_acq_finer_doppler: the next search's snapshot)
    return GM_OK;
}

int gm_acq_dwell_samples(gm_acq* a, uint64_t* out) {
    if (!a || !out) return set_err(GM_ERR_INVALID_ARG, "null handle/out");
    *out = acq_dwell_samples(a);
    return GM_OK;
}

int gm_acq_code_drift_starts(gm_acq* a, uint64_t* out) {
    if (!a || !out) return set_err(GM_ERR_INVALID_ARG, "null handle/out");
    if (!a->drift.on) return set_err(GM_ERR_INVALID_ARG, "the code-drift compensation is off (gm_acq_set_code_drift)");
    if (int rc = ensure_device(a->device)) return rc;
    HIPC(hipMemcpy(out, a->drift.d_starts, a->drift.starts.size() * 8, hipMemcpyDeviceToHost));
    return GM_OK;
}

int gm_acq_code_drift_phasors(gm_acq* a, uint32_t h, gm_c32* out) {
    if (!a || !out) return set_err(GM_ERR_INVALID_ARG, "null handle/out");
    if (!a->drift.on) return set_err(GM_ERR_INVALID_ARG, "the code-drift compensation is off (gm_acq_set_code_drift)");
    if (h >= (a->edge.H ? a->edge.H : 1u)) return set_err(GM_ERR_INVALID_ARG, "no such hypothesis");
    if (int rc = ensure_device(a->device)) return rc;
    const size_t n = size_t(a->D) * a->M * a->K;
    HIPC(hipMemcpy(out, a->drift.d_rho + size_t(h) * n, n * 8, hipMemcpyDeviceToHost));
    return GM_OK;
}

// ---------------------------------------------------------------- fine Doppler from per-period prompts (additive entries, ABI 9)
// the argument rules of gm_acq_refine_plan / gm_acq_refine_doppler and what a call uses for `bin` (gnss_mi355x.h states them)
static int refine_rules(uint32_t coherent_periods, uint32_t M, const gm_acq_refine_cfg* cfg, double fs, uint32_t N, uint32_t D,
                        const float* table_freq, uint32_t bin, RefinePlan& o) {
    const gm_acq_refine_cfg c = cfg ? *cfg : gm_acq_refine_cfg{0u, 0u, 0.0f};
    const uint32_t K = coherent_periods > 1 ? coherent_periods : 1;
    if (K > uint32_t(gm::GM_COHERENT_MAX)) return set_err(GM_ERR_INVALID_ARG, "coherent_periods > 32");
    if (!M || !N || !D || !table_freq || !(fs > 0.0)) return set_err(GM_ERR_INVALID_ARG, "n_integrations, fft_size, n_bins, table_freq and fs are required");
    if (bin >= D) return set_err(GM_ERR_INVALID_ARG, "doppler bin outside the handle's bins");
    if (K >= 2) {
        if (c.span_periods && c.span_periods != K) return set_err(GM_ERR_INVALID_ARG, "span_periods must be 0 or coherent_periods on a coherent handle");
        o.J = K; o.G = M;
    } else {
        o.J = c.span_periods ? c.span_periods : M;
        o.G = M / o.J;
    }
    if (o.J < 2) return set_err(GM_ERR_INVALID_ARG, "the fine Doppler needs at least 2 periods per group (one period carries no frequency information)");
    if (o.G < 1) return set_err(GM_ERR_INVALID_ARG, "span_periods exceeds n_integrations");
    o.Z = c.n_freq ? c.n_freq : 257u;
    if (o.Z < 3 || o.Z > 4097 || !(o.Z & 1u)) return set_err(GM_ERR_INVALID_ARG, "n_freq must be odd, 3 .. 4097");
    const double limit = fs / (2.0 * double(N));          // per-period prompts alias beyond it
    double hs = double(c.half_span_hz);
    if (c.half_span_hz == 0.0f) {
        if (D == 1) hs = fs / (2.0 * double(N) * double(K));
        else {
            const double f = double(table_freq[bin]);
            const double lo = bin > 0 ? ::fabs(f - double(table_freq[bin - 1])) : 0.0;
            const double hi = bin + 1 < D ? ::fabs(double(table_freq[bin + 1]) - f) : 0.0;
            hs = 0.5 * (lo > hi ? lo : hi);
        }
        if (hs > limit) hs = limit;
    }
    if (!(hs > 0.0) || !(hs <= limit)) return set_err(GM_ERR_INVALID_ARG, "half_span_hz must lie in (0, fs / (2 fft_size)]");   // (NaN fails too)
    o.half_span = hs;
    o.step = hs / double((o.Z - 1) / 2);
    return GM_OK;
}

int gm_acq_refine_plan(uint32_t coherent_periods, uint32_t n_integrations, const gm_acq_refine_cfg* cfg, float fs, uint32_t fft_size,
                       uint32_t n_bins, const float* table_freq, uint32_t bin, uint32_t* span_periods, uint32_t* n_groups,
                       uint32_t* n_freq, double* half_span_hz, double* step_hz) {
    RefinePlan o;
    if (int rc = refine_rules(coherent_periods, n_integrations, cfg, double(fs), fft_size, n_bins, table_freq, bin, o)) return rc;
    if (span_periods) *span_periods = o.J;
    if (n_groups) *n_groups = o.G;
    if (n_freq) *n_freq = o.Z;
    if (half_span_hz) *half_span_hz = o.half_span;
    if (step_hz) *step_hz = o.step;
    return GM_OK;
}

int gm_acq_refine_doppler(gm_acq* a, const gm_acq_result* results, const uint8_t* found, uint32_t n_prn, const gm_acq_refine_cfg* cfg,
                          gm_acq_refine_out* out, gm_c32* prompts, float* spectrum) {
    if (!a || !results || !found || !out) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (n_prn > a->P) return set_err(GM_ERR_INVALID_ARG, "n_prn exceeds the handle's workers");
    const void* in = nullptr;
    int in_fmt = 0;
    if (int rc = acq_call_input(a, nullptr, 0, &in, &in_fmt)) return rc;          // the snapshot of the last search
    const uint32_t N = a->N, D = a->D;
    const double fs = double(a->cfg.fs);
    // every argument is checked before anything runs or is written
    std::vector<RefinePlan> plans(n_prn);
    std::vector<uint32_t> list;
    RefinePlan common;
    if (int rc = refine_rules(a->cfg.coherent_periods, a->M, cfg, fs, N, D, a->table_freq.data(), 0, common)) return rc;
    for (uint32_t p = 0; p < n_prn; ++p) {
        if (!found[p]) continue;
        const int32_t d = results[p].doppler_bin;
        if (d < 0 || uint32_t(d) >= D) return set_err(GM_ERR_INVALID_ARG, "result.doppler_bin outside the handle's bins");
        if (results[p].code_phase_samples >= N) return set_err(GM_ERR_INVALID_ARG, "result.code_phase_samples >= fft_size");
        if (int rc = refine_rules(a->cfg.coherent_periods, a->M, cfg, fs, N, D, a->table_freq.data(), uint32_t(d), plans[p])) return rc;
        list.push_back(p);
    }
    if (list.empty()) return GM_OK;
    if (int rc = ensure_device(a->device)) return rc;
    if (int rc = acq_flush_decision(a)) return rc;
    const uint32_t S = uint32_t(list.size()), J = common.J, G = common.G, Z = common.Z, R_u = J * G;
    std::vector<uint32_t> off(n_prn, 0u);
    if (a->edge.H)
        if (int rc = gm_acq_result_offsets(a, results, found, n_prn, off.data())) return rc;
    // the block: [sats | z | t | fc | step | spectrum | peak values | peak indices], every part 256-byte aligned
    Carve cv;
    const size_t o_sat = cv.take(size_t(S) * sizeof(gm::RefineSat)), o_z = cv.take(size_t(S) * R_u * 8), o_t = cv.take(size_t(S) * R_u * 8),
                 o_fc = cv.take(size_t(S) * 8), o_step = cv.take(size_t(S) * 8), o_spec = cv.take(size_t(S) * Z * 4),
                 o_pv = cv.take(size_t(S) * 4), o_pi = cv.take(size_t(S) * 4);
    if (int rc = a->refine.reserve(a->stream, cv.end,
                                   "the fine-Doppler block does not fit (gnss_mi355x.h states the formula); the handle is as it was"))
        return rc;
    char* const base = static_cast<char*>(a->refine.d);
    // host side of the block's inputs: the satellite list, and the grid of its cells
    std::vector<gm::RefineSat> sats(S);
    CellGrid cg;
    cg.step.resize(S);
    for (uint32_t i = 0; i < S; ++i) {
        const uint32_t p = list[i];
        sats[i] = gm::RefineSat{p, uint32_t(results[p].code_phase_samples), uint32_t(results[p].doppler_bin), off[p]};
        cg.step[i] = plans[p].step;
    }
    HIPC(hipMemcpyAsync(base + o_sat, sats.data(), size_t(S) * sizeof(gm::RefineSat), hipMemcpyHostToDevice, a->stream));
    if (int rc = acq_cell_grid(a, sats, J, G, base + o_t, base + o_fc, base + o_step, cg)) return rc;
    gm::RefineArgs ra{};
    acq_cell_args(ra, a, in, in_fmt, R_u);
    acq_grid_args(ra, a, common, reinterpret_cast<cf*>(base + o_z), cg);
    ra.sats = reinterpret_cast<const gm::RefineSat*>(base + o_sat); ra.n_sats = S;
    ra.spectrum = reinterpret_cast<float*>(base + o_spec);
    ra.peak_val = reinterpret_cast<float*>(base + o_pv); ra.peak_idx = reinterpret_cast<uint32_t*>(base + o_pi);
    gm::launch_refine(a->stream, ra);
    HIPC(hipGetLastError());
    std::vector<float> spec(size_t(S) * Z);
    std::vector<uint32_t> pi(S);
    std::vector<gm_c32> zh(prompts ? size_t(S) * R_u : 0);
    HIPC(hipMemcpyAsync(spec.data(), base + o_spec, spec.size() * 4, hipMemcpyDeviceToHost, a->stream));
    HIPC(hipMemcpyAsync(pi.data(), base + o_pi, size_t(S) * 4, hipMemcpyDeviceToHost, a->stream));
    if (prompts) HIPC(hipMemcpyAsync(zh.data(), base + o_z, zh.size() * 8, hipMemcpyDeviceToHost, a->stream));
    HIPC(hipStreamSynchronize(a->stream));
    for (uint32_t i = 0; i < S; ++i) {
        const uint32_t p = list[i];
        const float* sp = &spec[size_t(i) * Z];
        const uint32_t pk = pi[i] < Z ? pi[i] : (Z - 1) / 2;      // (no comparable value at all, e.g. samples that are not numbers: the centre)
        gm_acq_refine_out& r = out[p];
        r.at_edge = (pk == 0 || pk == Z - 1) ? 1u : 0u;
        double delta = (double(pk) - double((Z - 1) / 2)) * cg.step[i];
        if (!r.at_edge) delta += parabola_offset(sp[pk - 1], sp[pk], sp[pk + 1]) * cg.step[i];     // through the peak and its neighbours
        r.carrier_hz = cg.fc[i] + delta;
        r.delta_hz = float(delta); r.step_hz = float(cg.step[i]); r.half_span_hz = float(plans[p].half_span);
        r.peak_power = sp[pk]; r.center_power = sp[(Z - 1) / 2];
        r.peak_index = pk;
        r.doppler_bin = sats[i].bin; r.offset_periods = sats[i].offset; r.span_periods = J; r.n_groups = G; r.n_freq = Z;
        if (prompts) memcpy(prompts + size_t(p) * R_u, &zh[size_t(i) * R_u], size_t(R_u) * 8);
        if (spectrum) memcpy(spectrum + size_t(p) * Z, sp, size_t(Z) * 4);
    }
    return GM_OK;
}

// ---------------------------------------------------------------- lag window x fine Doppler at known cells (additive entries, ABI 9)
static int local_rules(uint32_t coherent_periods, uint32_t M, const gm_acq_local_cfg* cfg, double fs, uint32_t N, uint32_t D,
                       const float* table_freq, uint32_t bin, RefinePlan& o, uint32_t& L) {
    const gm_acq_local_cfg c = cfg ? *cfg : gm_acq_local_cfg{0u, 0u, 0u, 0.0f};
    const gm_acq_refine_cfg rc{c.span_periods, c.n_freq, c.half_span_hz};
    if (int rv = refine_rules(coherent_periods, M, &rc, fs, N, D, table_freq, bin, o)) return rv;
    if (c.lag_half_window > 64u) return set_err(GM_ERR_INVALID_ARG, "lag_half_window > 64");
    if (2u * c.lag_half_window + 1u > N) return set_err(GM_ERR_INVALID_ARG, "the lag window (2 lag_half_window + 1) exceeds fft_size");
    L = c.lag_half_window;
    return GM_OK;
}

int gm_acq_local_plan(uint32_t coherent_periods, uint32_t n_integrations, const gm_acq_local_cfg* cfg, float fs, uint32_t fft_size,
                      uint32_t n_bins, const float* table_freq, uint32_t bin, uint32_t* n_lags, uint32_t* span_periods,
                      uint32_t* n_groups, uint32_t* n_freq, double* half_span_hz, double* step_hz) {
    RefinePlan o;
    uint32_t L = 0;
    if (int rc = local_rules(coherent_periods, n_integrations, cfg, double(fs), fft_size, n_bins, table_freq, bin, o, L)) return rc;
    if (n_lags) *n_lags = 2 * L + 1;
    if (span_periods) *span_periods = o.J;
    if (n_groups) *n_groups = o.G;
    if (n_freq) *n_freq = o.Z;
    if (half_span_hz) *half_span_hz = o.half_span;
    if (step_hz) *step_hz = o.step;
    return GM_OK;
}

int gm_acq_local_search(gm_acq* a, const void* d_samples, int fmt, const gm_acq_cand* cands, uint32_t n_cands,
                        const gm_acq_local_cfg* cfg, gm_acq_local_out* out, gm_c32* prompts, float* surface) {
    if (!a || !cands || !out) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    const void* in = nullptr;
    int in_fmt = 0;
    if (int rc = acq_call_input(a, d_samples, fmt, &in, &in_fmt)) return rc;
    const uint32_t N = a->N, D = a->D;
    const double fs = double(a->cfg.fs);
    // every argument is checked before anything runs or is written
    RefinePlan common;
    uint32_t L = 0;
    if (int rc = local_rules(a->cfg.coherent_periods, a->M, cfg, fs, N, D, a->table_freq.data(), 0, common, L)) return rc;
    std::vector<RefinePlan> plans(n_cands);
    for (uint32_t c = 0; c < n_cands; ++c) {
        if (int rc = acq_cand_rules(a, cands[c])) return rc;
        const int32_t d = cands[c].doppler_bin;
        uint32_t l = 0;
        if (int rc = local_rules(a->cfg.coherent_periods, a->M, cfg, fs, N, D, a->table_freq.data(), uint32_t(d), plans[c], l)) return rc;
    }
    if (!n_cands) return GM_OK;
    if (int rc = ensure_device(a->device)) return rc;
    if (int rc = acq_flush_decision(a)) return rc;
    const uint32_t S = n_cands, W = 2 * L + 1, J = common.J, G = common.G, Z = common.Z, R_u = J * G;
    const size_t rows = size_t(S) * W;
    // the block: [cands | z | t | fc | step | surface | row maxima | row indices | row sums | picks], every part 256-byte aligned
    Carve cv;
    const size_t o_cand = cv.take(size_t(S) * sizeof(gm::RefineSat)), o_z = cv.take(rows * R_u * 8), o_t = cv.take(size_t(S) * R_u * 8),
                 o_fc = cv.take(size_t(S) * 8), o_step = cv.take(size_t(S) * 8), o_surf = cv.take(rows * Z * 4), o_rv = cv.take(rows * 4),
                 o_ri = cv.take(rows * 4), o_rs = cv.take(rows * 8), o_pk = cv.take(size_t(S) * sizeof(gm::LocalPick));
    if (int rc = a->local.reserve(a->stream, cv.end,
                                  "the local-search block does not fit (gnss_mi355x.h states the formula); the handle is as it was"))
        return rc;
    char* const base = static_cast<char*>(a->local.d);
    // host side of the block's inputs: the candidates, and the grid of their cells
    std::vector<gm::RefineSat> cs(S);
    CellGrid cg;
    cg.step.resize(S);
    for (uint32_t c = 0; c < S; ++c) {
        cs[c] = acq_cand_cell(cands[c]);
        cg.step[c] = plans[c].step;
    }
    HIPC(hipMemcpyAsync(base + o_cand, cs.data(), size_t(S) * sizeof(gm::RefineSat), hipMemcpyHostToDevice, a->stream));
    if (int rc = acq_cell_grid(a, cs, J, G, base + o_t, base + o_fc, base + o_step, cg)) return rc;
    gm::LocalArgs la{};
    acq_cell_args(la, a, in, in_fmt, R_u);
    acq_grid_args(la, a, common, reinterpret_cast<cf*>(base + o_z), cg);
    la.cands = reinterpret_cast<const gm::RefineSat*>(base + o_cand); la.n_cands = S;
    la.L = L;
    la.guard = uint32_t(::ceil(fs / double(a->code_rate))) + 1u;
    la.surface = reinterpret_cast<float*>(base + o_surf);
    la.row_val = reinterpret_cast<float*>(base + o_rv); la.row_idx = reinterpret_cast<uint32_t*>(base + o_ri);
    la.row_sum = reinterpret_cast<double*>(base + o_rs); la.picks = reinterpret_cast<gm::LocalPick*>(base + o_pk);
    gm::launch_local(a->stream, la);
    HIPC(hipGetLastError());
    std::vector<gm::LocalPick> pk(S);
    HIPC(hipMemcpyAsync(pk.data(), base + o_pk, size_t(S) * sizeof(gm::LocalPick), hipMemcpyDeviceToHost, a->stream));
    // the caller's arrays have the block's layout: filled directly, after every check and launch has passed
    if (prompts) HIPC(hipMemcpyAsync(prompts, base + o_z, rows * R_u * 8, hipMemcpyDeviceToHost, a->stream));
    if (surface) HIPC(hipMemcpyAsync(surface, base + o_surf, rows * Z * 4, hipMemcpyDeviceToHost, a->stream));
    HIPC(hipStreamSynchronize(a->stream));
    for (uint32_t c = 0; c < S; ++c) {
        const gm::LocalPick& p = pk[c];
        const uint32_t d = cs[c].bin, o = cs[c].offset, ls = p.l < W ? p.l : L, js = p.j < Z ? p.j : (Z - 1) / 2;
        gm_acq_local_out& r = out[c];
        r.freq_at_edge = (js == 0 || js == Z - 1) ? 1u : 0u;
        double delta = (double(js) - double((Z - 1) / 2)) * cg.step[c];
        if (!r.freq_at_edge) delta += parabola_offset(p.s_jm, p.s0, p.s_jp) * cg.step[c];         // along j
        r.carrier_hz = cg.fc[c] + delta;
        r.delta_hz = float(delta); r.step_hz = float(cg.step[c]); r.half_span_hz = float(plans[c].half_span);
        r.peak_power = p.s0;
        r.floor_power = p.n_floor ? float(p.floor_sum / (double(p.n_floor) * double(Z))) : 0.0f;
        r.n_floor = p.n_floor;
        r.peak_lag_index = ls; r.peak_freq_index = js;
        const uint32_t lam = (cs[c].code_phase + N - L + ls) % N;          // lambda_{l*}: cp < N, L < N
        r.code_phase_samples = lam;
        r.lag_at_edge = (ls == 0 || ls == W - 1) ? 1u : 0u;
        r.code_phase_fine = double(lam);
        if (!r.lag_at_edge) {
            // the vertex of a symmetric triangle through the three amplitudes
            const double am = ::sqrt(double(p.s_lm)), a0 = ::sqrt(double(p.s0)), ap = ::sqrt(double(p.s_lp));
            const double den = 2.0 * (a0 - (am < ap ? am : ap));
            double frac = den > 0.0 ? (ap - am) / den : 0.0;
            frac = frac > 0.5 ? 0.5 : (frac < -0.5 ? -0.5 : frac);
            const double lambda = double(lam) + frac;
            double fine = lambda;
            if (a->drift.on) {
                // the starts' roundings, and the samples in front of the lag, which belong to the previous (shorter or longer) period
                const double T = a->drift.T[d];
                double e = 0.0;
                for (uint32_t i = 0; i < R_u; ++i) e += double(a->drift.starts[size_t(d) * a->drift.R + o + i]) - double(o + i) * T;
                fine = lambda + e / double(R_u) - (lambda / double(N)) * (double(N) - T);
            }
            fine = ::fmod(fine, double(N));
            if (fine < 0.0) fine += double(N);
            if (fine >= double(N)) fine -= double(N);
            r.code_phase_fine = fine;
        }
        r.doppler_bin = d; r.offset_periods = o; r.span_periods = J; r.n_groups = G; r.n_freq = Z; r.n_lags = W;
    }
    return GM_OK;
}

// ---------------------------------------------------------------- beam rows from the array's own correlations (additive entries, ABI 9)
// the argument rules of gm_acq_array_plan / gm_acq_array_prompts (gnss_mi355x.h states them)
static int array_rules(uint32_t coherent_periods, uint32_t M, uint32_t A, uint32_t L, uint32_t& R_u, uint32_t& words) {
    const uint32_t K = coherent_periods > 1 ? coherent_periods : 1;
    if (K > uint32_t(gm::GM_COHERENT_MAX)) return set_err(GM_ERR_INVALID_ARG, "coherent_periods > 32");
    if (!M) return set_err(GM_ERR_INVALID_ARG, "n_integrations is required");
    if (A < 2 || A > uint32_t(gm::NL_A_MAX)) return set_err(GM_ERR_INVALID_ARG, "n_antennas must be 2 .. 8");
    if (L < 1 || L > uint32_t(gm::ST_L_MAX)) return set_err(GM_ERR_INVALID_ARG, "taps must be 1 .. 8");
    if (A * L > uint32_t(gm::ST_M_MAX)) return set_err(GM_ERR_INVALID_ARG, "n_antennas * taps must not exceed 32");
    const uint64_t r = uint64_t(K) * M, wds = r * A * L;
    if (wds > 0xFFFFFFFFull) return set_err(GM_ERR_INVALID_ARG, "periods * taps * n_antennas does not fit 32 bits");
    R_u = uint32_t(r); words = uint32_t(wds);
    return GM_OK;
}

int gm_acq_array_plan(uint32_t coherent_periods, uint32_t n_integrations, uint32_t n_antennas, uint32_t taps, uint32_t* periods,
                      uint32_t* words_per_cand) {
    uint32_t R_u = 0, words = 0;
    if (int rc = array_rules(coherent_periods, n_integrations, n_antennas, taps, R_u, words)) return rc;
    if (periods) *periods = R_u;
    if (words_per_cand) *words_per_cand = words;
    return GM_OK;
}

int gm_acq_array_prompts(gm_acq* a, const void* d_samples, int fmt, uint32_t n_antennas, uint32_t taps, const gm_acq_cand* cands,
                         uint32_t n_cands, gm_c32* z) {
    if (!a || !d_samples || !cands || !z) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (fmt != GM_FMT_C32 && fmt != GM_FMT_I8_IQ) return set_err(GM_ERR_INVALID_ARG, "the array stream is GM_FMT_C32 or GM_FMT_I8_IQ");
    // every argument is checked before anything runs or is written
    uint32_t R_u = 0, words = 0;
    if (int rc = array_rules(a->K, a->M, n_antennas, taps, R_u, words)) return rc;
    if (n_cands > 1024u) return set_err(GM_ERR_INVALID_ARG, "n_cands > 1024");
    for (uint32_t c = 0; c < n_cands; ++c)
        if (int rc = acq_cand_rules(a, cands[c])) return rc;
    if (!n_cands) return GM_OK;
    if (int rc = ensure_device(a->device)) return rc;
    if (int rc = acq_flush_decision(a)) return rc;
    // the block: [cands | z], each part 256-byte aligned
    const size_t z_bytes = size_t(n_cands) * words * 8;
    Carve cv;
    const size_t o_cand = cv.take(size_t(n_cands) * sizeof(gm::RefineSat)), o_z = cv.take(z_bytes);
    if (int rc = a->array.reserve(a->stream, cv.end,
                                  "the array-prompts block does not fit (gnss_mi355x.h states the formula); the handle is as it was"))
        return rc;
    char* const base = static_cast<char*>(a->array.d);
    std::vector<gm::RefineSat> cs(n_cands);
    for (uint32_t c = 0; c < n_cands; ++c) cs[c] = acq_cand_cell(cands[c]);
    HIPC(hipMemcpyAsync(base + o_cand, cs.data(), size_t(n_cands) * sizeof(gm::RefineSat), hipMemcpyHostToDevice, a->stream));
    gm::ArrayArgs aa{};
    acq_cell_args(aa, a, d_samples, fmt, R_u);
    aa.cands = reinterpret_cast<const gm::RefineSat*>(base + o_cand); aa.n_cands = n_cands;
    aa.A = n_antennas; aa.L = taps;
    aa.z = reinterpret_cast<cf*>(base + o_z);
    gm::launch_array(a->stream, aa);
    HIPC(hipGetLastError());
    // the caller's array has the block's layout: filled directly, after every check and the launch have passed
    HIPC(hipMemcpyAsync(z, base + o_z, z_bytes, hipMemcpyDeviceToHost, a->stream));
    HIPC(hipStreamSynchronize(a->stream));
    return GM_OK;
}

// gm_array_row_solve: gnss_mi355x.h states the nine steps; all f64, host only
namespace {
struct zc { double re, im; };
// cyclic Hermitian Jacobi on Q [m][m] (both triangles kept), V the accumulated rotations: Q <- J^H Q J, V <- V J, until the
// off-diagonal energy is below 1e-30 of the whole (or 64 sweeps)
void hermitian_jacobi(uint32_t m, std::vector<zc>& Q, std::vector<zc>& V) {
    for (uint32_t i = 0; i < m * m; ++i) V[i] = zc{0.0, 0.0};
    for (uint32_t i = 0; i < m; ++i) V[i * m + i].re = 1.0;
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0.0, all = 0.0;
        for (uint32_t p = 0; p < m; ++p)
            for (uint32_t q = 0; q < m; ++q) {
                const double e = Q[p * m + q].re * Q[p * m + q].re + Q[p * m + q].im * Q[p * m + q].im;
                all += e;
                if (p != q) off += e;
            }
        if (!(off > 1e-30 * all)) break;
        for (uint32_t p = 0; p + 1 < m; ++p)
            for (uint32_t q = p + 1; q < m; ++q) {
                const zc b = Q[p * m + q];
                const double g = ::hypot(b.re, b.im);
                if (g == 0.0) continue;
                const double app = Q[p * m + p].re, aqq = Q[q * m + q].re;
                // b = g e^{j phi}: the 2 x 2 block [[app, b], [conj b, aqq]] is diagonalised by J = [[c, s e^{j phi}], [-s e^{-j phi}, c]]
                const double tau = (aqq - app) / (2.0 * g);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (::fabs(tau) + ::sqrt(1.0 + tau * tau));
                const double c = 1.0 / ::sqrt(1.0 + t * t), s = t * c;
                const zc e{b.re / g, b.im / g};                           // e^{j phi}
                const zc se{s * e.re, s * e.im};                          // s e^{j phi}
                // columns: X[:, p] <- c X[:, p] - conj(se) X[:, q];  X[:, q] <- se X[:, p] + c X[:, q]   (X = Q, then V)
                auto cols = [&](std::vector<zc>& X) {
                    for (uint32_t k = 0; k < m; ++k) {
                        const zc xp = X[k * m + p], xq = X[k * m + q];
                        X[k * m + p] = zc{c * xp.re - (se.re * xq.re + se.im * xq.im), c * xp.im - (se.re * xq.im - se.im * xq.re)};
                        X[k * m + q] = zc{se.re * xp.re - se.im * xp.im + c * xq.re, se.re * xp.im + se.im * xp.re + c * xq.im};
                    }
                };
                cols(Q);
                // rows (J^H from the left): X[p, :] <- c X[p, :] - se X[q, :];  X[q, :] <- conj(se) X[p, :] + c X[q, :]
                for (uint32_t k = 0; k < m; ++k) {
                    const zc xp = Q[p * m + k], xq = Q[q * m + k];
                    Q[p * m + k] = zc{c * xp.re - (se.re * xq.re - se.im * xq.im), c * xp.im - (se.re * xq.im + se.im * xq.re)};
                    Q[q * m + k] = zc{se.re * xp.re + se.im * xp.im + c * xq.re, se.re * xp.im - se.im * xp.re + c * xq.im};
                }
                Q[p * m + q] = zc{0.0, 0.0}; Q[q * m + p] = zc{0.0, 0.0};
                Q[p * m + p].im = 0.0; Q[q * m + q].im = 0.0;
                cols(V);
            }
    }
}
}  // namespace

int gm_array_row_solve(uint32_t m, uint32_t n, const gm_c32* z, const gm_c32* R, size_t n_blocks, float loading, gm_c32* row,
                       gm_array_row_info* info) {
    if (!z || !row || !info) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (m < 2 || m > uint32_t(gm::ST_M_MAX)) return set_err(GM_ERR_INVALID_ARG, "m must be 2 .. 32");
    if (!n) return set_err(GM_ERR_INVALID_ARG, "n = 0: no prompt vector");
    if (R && !n_blocks) return set_err(GM_ERR_INVALID_ARG, "R without blocks");
    double load = 1e-4;
    if (loading != 0.0f) {
        if (!(loading >= 1e-6f && loading <= 1.0f)) return set_err(GM_ERR_INVALID_ARG, "loading must be 0 or lie in [1e-6, 1]");   // (NaN fails too)
        load = double(loading);
    }
    const size_t mm = size_t(m) * m;
    for (size_t i = 0; i < size_t(n) * m; ++i)
        if (!std::isfinite(z[i].re) || !std::isfinite(z[i].im)) return set_err(GM_ERR_INVALID_ARG, "a prompt word is not finite");
    // 1. Rs, from the upper triangles
    std::vector<zc> Rs(mm, zc{0.0, 0.0});
    if (R) {
        for (size_t b = 0; b < n_blocks; ++b)
            for (uint32_t p = 0; p < m; ++p)
                for (uint32_t q = p; q < m; ++q) {
                    const gm_c32 v = R[b * mm + size_t(p) * m + q];
                    if (!std::isfinite(v.re) || !std::isfinite(v.im)) return set_err(GM_ERR_INVALID_ARG, "a word of R is not finite");
                    Rs[p * m + q].re += double(v.re);
                    if (p != q) Rs[p * m + q].im += double(v.im);
                }
    } else {
        for (uint32_t p = 0; p < m; ++p) Rs[p * m + p].re = 1.0;
    }
    // 2. the loading
    double tr = 0.0;
    for (uint32_t p = 0; p < m; ++p) tr += Rs[p * m + p].re;
    if (!(tr > 0.0) || !std::isfinite(tr)) return set_err(GM_ERR_INVALID_ARG, "the trace of R is not positive and finite");
    const double dl = load * (tr / double(m));
    // 3. Cholesky, Rl = C C^H, left-looking, columns ascending; Rl[i][j] for i >= j is conj(Rs[j][i])
    std::vector<zc> Cf(mm, zc{0.0, 0.0});
    for (uint32_t j = 0; j < m; ++j) {
        double pj = Rs[j * m + j].re + dl;
        for (uint32_t k = 0; k < j; ++k) pj -= Cf[j * m + k].re * Cf[j * m + k].re + Cf[j * m + k].im * Cf[j * m + k].im;
        if (!(pj > 0.0) || !std::isfinite(pj)) return set_err(GM_ERR_INVALID_ARG, "a Cholesky pivot is not positive and finite");
        const double d = ::sqrt(pj);
        Cf[j * m + j] = zc{d, 0.0};
        for (uint32_t i = j + 1; i < m; ++i) {
            double xr = Rs[j * m + i].re, xi = -Rs[j * m + i].im;
            for (uint32_t k = 0; k < j; ++k) {                            // - C[i][k] conj(C[j][k])
                const zc ci = Cf[i * m + k], cj = Cf[j * m + k];
                xr -= ci.re * cj.re + ci.im * cj.im;
                xi -= ci.im * cj.re - ci.re * cj.im;
            }
            Cf[i * m + j] = zc{xr / d, xi / d};
        }
    }
    // 4. zt_i = C^-1 z_i (forward substitution), Q = sum_i zt_i zt_i^H
    std::vector<zc> Q(mm, zc{0.0, 0.0}), V(mm), zt(m);
    for (uint32_t i = 0; i < n; ++i) {
        for (uint32_t p = 0; p < m; ++p) {
            double xr = double(z[size_t(i) * m + p].re), xi = double(z[size_t(i) * m + p].im);
            for (uint32_t k = 0; k < p; ++k) {
                const zc c = Cf[p * m + k];
                xr -= c.re * zt[k].re - c.im * zt[k].im;
                xi -= c.re * zt[k].im + c.im * zt[k].re;
            }
            zt[p] = zc{xr / Cf[p * m + p].re, xi / Cf[p * m + p].re};
        }
        for (uint32_t p = 0; p < m; ++p)
            for (uint32_t q = 0; q < m; ++q) {                            // zt[p] conj(zt[q])
                Q[p * m + q].re += zt[p].re * zt[q].re + zt[p].im * zt[q].im;
                Q[p * m + q].im += zt[p].im * zt[q].re - zt[p].re * zt[q].im;
            }
    }
    // 5. the two largest eigenvalues and the first eigenvector
    hermitian_jacobi(m, Q, V);
    uint32_t i1 = 0;
    for (uint32_t p = 1; p < m; ++p)
        if (Q[p * m + p].re > Q[i1 * m + i1].re) i1 = p;
    const double lambda1 = Q[i1 * m + i1].re;
    double lambda2 = -1.0;
    for (uint32_t p = 0; p < m; ++p)
        if (p != i1 && Q[p * m + p].re > lambda2) lambda2 = Q[p * m + p].re;
    if (lambda2 < 0.0) lambda2 = 0.0;
    if (!(lambda1 > 0.0) || !std::isfinite(lambda1)) return set_err(GM_ERR_INVALID_ARG, "lambda1 is not greater than 0");
    // 6. s = C v
    std::vector<zc> s(m);
    for (uint32_t p = 0; p < m; ++p) {
        double xr = 0.0, xi = 0.0;
        for (uint32_t k = 0; k <= p; ++k) {
            const zc c = Cf[p * m + k], v = V[k * m + i1];
            xr += c.re * v.re - c.im * v.im;
            xi += c.re * v.im + c.im * v.re;
        }
        s[p] = zc{xr, xi};
    }
    // 7. the word of largest modulus real and positive;  8. s^H s = m;  9. one rounding to f32
    uint32_t ref = 0;
    double best = -1.0, e = 0.0;
    for (uint32_t p = 0; p < m; ++p) {
        const double a2 = s[p].re * s[p].re + s[p].im * s[p].im;
        e += a2;
        if (a2 > best) { best = a2; ref = p; }
    }
    if (!(best > 0.0) || !std::isfinite(e)) return set_err(GM_ERR_INVALID_ARG, "the row came out zero or not finite");
    const double g = ::sqrt(best), scale = ::sqrt(double(m) / e);
    const zc rot{s[ref].re / g, -s[ref].im / g};                          // conj of the word's phase
    for (uint32_t p = 0; p < m; ++p) {
        row[p].re = float((s[p].re * rot.re - s[p].im * rot.im) * scale);
        row[p].im = float((s[p].re * rot.im + s[p].im * rot.re) * scale);
    }
    row[ref].im = 0.0f;
    info->lambda1 = lambda1; info->lambda2 = lambda2; info->ref_index = ref; info->reserved = 0;
    return GM_OK;
}

// ---------------------------------------------------------------- subtracting found satellites from a dwell (additive entries, ABI 9)
// the segments of one candidate on a dwell of D samples (gnss_mi355x.h states the rule; tests/acq_cancel_model.py restates it): host f64
struct CancelPlan {
    double T = 0.0;                         // the period in use (period_samples, or fft_size where that is 0)
    int64_t q0 = 0;
    std::vector<double> o;                  // [Q + 1]
    std::vector<uint64_t> b;                // [Q + 1], b[0] = 0, b[Q] = D
    uint32_t Q = 0;
};
constexpr uint64_t CANCEL_MAX_DWELL = 1ull << 40;      // (a dwell is K * M + o_max periods of at most 2^18 samples)
static int cancel_rules(uint64_t D, uint32_t N, double cp, double period, CancelPlan& p) {
    if (N < 16) return set_err(GM_ERR_INVALID_ARG, "fft_size below 16");
    if (!D || D > CANCEL_MAX_DWELL) return set_err(GM_ERR_INVALID_ARG, "dwell_samples is 0 or above 2^40");
    if (double(D) / (double(N) - 8.0) > double(1u << 24)) return set_err(GM_ERR_INVALID_ARG, "dwell_samples holds more than 2^24 code periods");
    if (!(cp >= 0.0 && cp < double(N))) return set_err(GM_ERR_INVALID_ARG, "code_phase outside [0, fft_size)");
    if (period != 0.0 && !(::fabs(period - double(N)) <= 8.0))
        return set_err(GM_ERR_INVALID_ARG, "period_samples not within 8 of fft_size (0: fft_size)");
    const double T = period != 0.0 ? period : double(N);
    p.T = T;
    p.q0 = -int64_t(::ceil(cp / T));
    p.o.clear(); p.b.clear();
    for (uint64_t k = 0;; ++k) {
        const double o = cp + double(p.q0 + int64_t(k)) * T;
        p.o.push_back(o);
        if (o >= double(D)) { p.b.push_back(D); break; }
        const double c = ::ceil(o);
        p.b.push_back(c <= 0.0 ? 0ull : uint64_t(c));          // (o < D: ceil(o) <= D)
    }
    p.Q = uint32_t(p.o.size() - 1);
    return GM_OK;
}

int gm_acq_cancel_plan(uint64_t dwell_samples, uint32_t fft_size, double code_phase, double period_samples, uint32_t* n_segments,
                       uint64_t* bounds, uint32_t bounds_cap) {
    CancelPlan p;
    if (int rc = cancel_rules(dwell_samples, fft_size, code_phase, period_samples, p)) return rc;
    if (bounds && bounds_cap < p.Q + 1) return set_err(GM_ERR_INVALID_ARG, "bounds_cap below n_segments + 1");
    if (n_segments) *n_segments = p.Q;
    if (bounds) memcpy(bounds, p.b.data(), size_t(p.Q + 1) * sizeof(uint64_t));
    return GM_OK;
}

int gm_acq_cancel(gm_acq* a, const void* d_samples, int fmt, const gm_acq_cancel_cand* cands, uint32_t n_cands, void* d_out,
                  gm_acq_cancel_out* out, gm_c32* amps, uint32_t amps_stride) {
    if (!a || (!cands && n_cands) || !d_out) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (n_cands > 64) return set_err(GM_ERR_INVALID_ARG, "more than 64 candidates");
    const void* in = nullptr;
    int in_fmt = 0;
    if (int rc = acq_call_input(a, d_samples, fmt, &in, &in_fmt)) return rc;
    const uint32_t N = a->N;
    const uint64_t D = acq_dwell_samples(a);
    const double fs = double(a->cfg.fs);
    // every argument is checked before anything runs or is written
    {   // the output may be the c32 input itself (in place); any other overlap of the two ranges is refused
        const uintptr_t i0 = reinterpret_cast<uintptr_t>(in), i1 = i0 + D * fmt_bytes(in_fmt);
        const uintptr_t o0 = reinterpret_cast<uintptr_t>(d_out), o1 = o0 + D * 8u;
        if (!(o0 == i0 && in_fmt == GM_FMT_C32) && o0 < i1 && i0 < o1)
            return set_err(GM_ERR_INVALID_ARG, "d_out overlaps the input (only d_out == the c32 input itself is allowed)");
        if (o0 & 7u) return set_err(GM_ERR_INVALID_ARG, "d_out is not aligned to a c32 sample");
    }
    std::vector<CancelPlan> plans(n_cands);
    uint32_t q_max = 0;
    for (uint32_t c = 0; c < n_cands; ++c) {
        const gm_acq_cancel_cand& cd = cands[c];
        if (cd.worker >= a->P) return set_err(GM_ERR_INVALID_ARG, "candidate.worker outside the handle's workers");
        if (cd.reserved) return set_err(GM_ERR_INVALID_ARG, "candidate.reserved must be 0");
        if (!(::fabs(cd.carrier_hz) < fs)) return set_err(GM_ERR_INVALID_ARG, "candidate.carrier_hz is not a number or |carrier_hz| >= fs");
        if (int rc = cancel_rules(D, N, cd.code_phase, cd.period_samples, plans[c])) return rc;
        q_max = plans[c].Q > q_max ? plans[c].Q : q_max;
    }
    if (amps && amps_stride < q_max) return set_err(GM_ERR_INVALID_ARG, "amps_stride below the largest n_segments");
    if (int rc = ensure_device(a->device)) return rc;
    if (int rc = acq_flush_decision(a)) return rc;
    if (!a->d_cancel_chips) {
        int8_t* chips = nullptr;
        if (hipMalloc(&chips, a->chips.size()) != hipSuccess) {
            (void)hipGetLastError();
            return set_err(GM_ERR_NOMEM, "the chip rows of gm_acq_cancel do not fit; the handle is as it was");
        }
        if (hipError_t e = hipMemcpy(chips, a->chips.data(), a->chips.size(), hipMemcpyHostToDevice); e != hipSuccess) {
            hipFree(chips);
            return hip_fail(e, "hipMemcpy");
        }
        a->d_cancel_chips = chips;
    }
    // the block: [candidate constants | o | b | amplitudes], every part 256-byte aligned; the tables are [n_cands][stride]
    const uint32_t S = n_cands, stride = q_max + 1;
    const size_t cells = size_t(S) * stride;
    Carve cv;
    const size_t o_cand = cv.take(size_t(S) * sizeof(gm::CancelCand)), o_o = cv.take(cells * 8), o_b = cv.take(cells * 8), o_a = cv.take(cells * 8);
    if (int rc = a->cancel.reserve(a->stream, cv.end + 256,          // (the block ends 256 bytes behind the amplitudes)
                                   "the cancellation block does not fit (gnss_mi355x.h states the formula); the handle is as it was"))
        return rc;
    char* const base = static_cast<char*>(a->cancel.d);
    std::vector<gm::CancelCand> cs(S);
    std::vector<double> o(cells, 0.0);
    std::vector<uint64_t> b(cells, D);
    for (uint32_t c = 0; c < S; ++c) {
        const CancelPlan& p = plans[c];
        cs[c] = gm::CancelCand{double(a->code_len) / p.T, cands[c].carrier_hz / fs, cands[c].code_phase, 1.0 / p.T,
                               cands[c].worker, a->code_len, p.Q, int32_t(p.q0)};
        std::copy(p.o.begin(), p.o.end(), o.begin() + size_t(c) * stride);
        std::copy(p.b.begin(), p.b.end(), b.begin() + size_t(c) * stride);
    }
    if (S) {
        HIPC(hipMemcpyAsync(base + o_cand, cs.data(), size_t(S) * sizeof(gm::CancelCand), hipMemcpyHostToDevice, a->stream));
        HIPC(hipMemcpyAsync(base + o_o, o.data(), cells * 8, hipMemcpyHostToDevice, a->stream));
        HIPC(hipMemcpyAsync(base + o_b, b.data(), cells * 8, hipMemcpyHostToDevice, a->stream));
    }
    gm::CancelArgs ca{};
    ca.samples = in; ca.fmt = in_fmt; ca.D = D;
    ca.cands = reinterpret_cast<const gm::CancelCand*>(base + o_cand); ca.n_cands = S; ca.q_max = q_max; ca.stride = stride;
    ca.o = reinterpret_cast<const double*>(base + o_o); ca.b = reinterpret_cast<const uint64_t*>(base + o_b);
    ca.chips = a->d_cancel_chips;
    ca.amps = reinterpret_cast<cf*>(base + o_a); ca.out = static_cast<cf*>(d_out);
    gm::launch_cancel(a->stream, ca);
    HIPC(hipGetLastError());
    std::vector<cf> am(cells);
    if (S) HIPC(hipMemcpyAsync(am.data(), base + o_a, cells * 8, hipMemcpyDeviceToHost, a->stream));
    HIPC(hipStreamSynchronize(a->stream));  // (the host vectors above live until here)
    for (uint32_t c = 0; c < S; ++c) {
        const CancelPlan& p = plans[c];
        const cf* row = &am[size_t(c) * stride];
        if (amps) memcpy(amps + size_t(c) * amps_stride, row, size_t(p.Q) * sizeof(cf));
        if (!out) continue;
        double energy = 0.0;
        for (uint32_t k = 0; k < p.Q; ++k)
            energy += double(p.b[k + 1] - p.b[k]) * (double(row[k].x) * double(row[k].x) + double(row[k].y) * double(row[k].y));
        gm_acq_cancel_out& r = out[c];
        r.removed_energy = energy;
        r.amp_rms = float(::sqrt(energy / double(D)));
        r.n_segments = p.Q;
        r.first_samples = uint32_t(p.b[1] - p.b[0]);
        r.last_samples = uint32_t(p.b[p.Q] - p.b[p.Q - 1]);
        r.worker = cands[c].worker;
        r.reserved = 0;
    }
    return GM_OK;
}

int gm_acq_enable_timing(gm_acq* a, int on) {
    if (!a) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (int rc = ensure_device(a->device)) return rc;
    if (on && a->tm.ev.empty()) {
        a->tm.ev.assign(size_t(Timing::CAP) * 4, nullptr);
        for (auto& e : a->tm.ev) HIPC(hipEventCreate(&e));
    }
    a->tm.on = on != 0;
    a->tm.stride = on > 1 ? on : 1;      // on = k > 1: every k-th search is timed
    a->tm.calls = 0;
    a->tm.this_call = false;
    a->tm.count = 0;
    a->tm.decide_valid = false;
    return GM_OK;
}

int gm_acq_last_timing(gm_acq* a, float* ms_mix, float* ms_corr, float* ms_decide) {
    if (!a || !a->tm.on || a->tm.count == 0) return set_err(GM_ERR_INVALID_ARG, "timing not enabled / nothing recorded");
    if (int rc = ensure_device(a->device)) return rc;
    HIPC(hipStreamSynchronize(a->stream));
    hipEvent_t* ev = &a->tm.ev[size_t((a->tm.count - 1) % Timing::CAP) * 4];
    float t = 0;
    if (ms_mix) { HIPC(hipEventElapsedTime(&t, ev[0], ev[1])); *ms_mix = t; }
    if (ms_corr) { HIPC(hipEventElapsedTime(&t, ev[1], ev[2])); *ms_corr = t; }
    if (ms_decide) {
        *ms_decide = 0;
        if (a->tm.decide_valid) { HIPC(hipEventElapsedTime(&t, ev[2], ev[3])); *ms_decide = t; }
    }
    return GM_OK;
}

int gm_acq_timing_summary(gm_acq* a, uint32_t* launches, float* avg_ms_mix, float* avg_ms_corr) {
    if (!a || !a->tm.on) return set_err(GM_ERR_INVALID_ARG, "timing not enabled");
    if (int rc = ensure_device(a->device)) return rc;
    HIPC(hipStreamSynchronize(a->stream));
    const int n = a->tm.count < Timing::CAP ? a->tm.count : Timing::CAP;
    double sm = 0, sc = 0;
    for (int i = 0; i < n; ++i) {
        hipEvent_t* ev = &a->tm.ev[size_t(i) * 4];
        float t = 0;
        HIPC(hipEventElapsedTime(&t, ev[0], ev[1])); sm += t;
        HIPC(hipEventElapsedTime(&t, ev[1], ev[2])); sc += t;
    }
    if (launches) *launches = uint32_t(n);
    if (avg_ms_mix) *avg_ms_mix = n ? float(sm / n) : 0.f;
    if (avg_ms_corr) *avg_ms_corr = n ? float(sc / n) : 0.f;
    return GM_OK;
}

// Host replay of the decision (same arithmetic as decide_kernel) for callers that hold the metrics on the
// host, e.g. after a gloo/MPI all-gather.  No device needed.
int gm_acq_decide_host(const float* mmax, const uint32_t* margmax, const float* msum, const float* table_freq,
                       uint32_t n_prn, uint32_t n_bins, const uint8_t* prn_ids, uint32_t fft_size, float fs,
                       float code_rate, float threshold, uint64_t local_tail, gm_acq_result* results, uint8_t* found) {
    if (!mmax || !margmax || !msum || !table_freq || !prn_ids || !results || !found || fft_size < 2)
        return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (threshold == 0.0f) threshold = 7.0f;
    if (!(code_rate > 0.0f)) code_rate = CA_RATE;
    const float nm1 = float(fft_size - 1);
    for (uint32_t p = 0; p < n_prn; ++p) {
        gm_acq_result r;
        memset(&r, 0, sizeof(r));
        r.prn = prn_ids[p]; r.doppler_bin = -1;
        found[p] = 0;
        float gmax = 0.0f, bfreq = 0.0f, bsum = 0.0f;
        uint32_t bphase = 0;
        int bbin = -1;
        for (uint32_t d = 0; d < n_bins; ++d) {
            const size_t o = size_t(p) * n_bins + d;
            if (mmax[o] > gmax) { gmax = mmax[o]; bfreq = table_freq[d]; bphase = margmax[o]; bsum = msum[o]; bbin = int(d); }
            const float avg = (bsum - gmax) / nm1;
            if (gmax / avg > threshold) {
                r.code_phase_samples = bphase;
                r.code_phase_chips = float(bphase) * code_rate / fs;
                r.carrier_freq = bfreq; r.fs = fs; r.mag_relative = gmax;
                r.sample_global_index = local_tail + bphase; r.doppler_bin = bbin;
                found[p] = 1;
                break;
            }
        }
        results[p] = r;
    }
    return GM_OK;
}

// Diagnostic (not in the reference): arm (out == NULL) / read back phase stamps of workgroup 0 of acq_corr_kernel:
// out = [n_integrations][8 waves][8 phases] shader-clock values of the last search.
int gm_acq_debug_stamps(gm_acq* a, long long* out) {
    if (!a) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (!gm::corr_stamps_built())
        return set_err(GM_ERR_UNSUPPORTED, "the stamped correlation kernels are in a diagnostic build only (GM_EXTRA_FLAGS=-DGM_DIAG_STAMPS, tools/README.md)");
    if (int rc = ensure_device(a->device)) return rc;
    static long long* d_st = nullptr;
    const size_t bytes = size_t(a->M) * 64 * sizeof(long long);
    if (!out) {
        if (d_st) { gm::set_corr_stamps(nullptr); hipFree(d_st); d_st = nullptr; }
        HIPC(hipMalloc(&d_st, bytes));
        HIPC(hipMemset(d_st, 0, bytes));
        HIPC(hipStreamSynchronize(nullptr));
        gm::set_corr_stamps(d_st);
        return GM_OK;
    }
    if (!d_st) return set_err(GM_ERR_INVALID_ARG, "stamps not armed");
    HIPC(hipStreamSynchronize(a->stream));
    HIPC(hipMemcpy(out, d_st, bytes, hipMemcpyDeviceToHost));
    gm::set_corr_stamps(nullptr);
    hipFree(d_st); d_st = nullptr;
    return GM_OK;
}

// Diagnostic (not in the reference): the grid of the handle's last stage-C launch as its launcher decided it (Launch<PL>::corr,
// CompLaunch::corr, launch_long_corr write gm_acq::last_grid); nothing is computed here, and no device is needed.
int gm_acq_debug_corr_grid(gm_acq* a, gm_acq_corr_grid_info* out) {
    if (!a || !out) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    *out = a->last_grid;
    return GM_OK;
}

int gm_acq_manager_mode_for(size_t n) { return n == 0 ? 0 : (n <= 4 ? 1 : 2); }   // update_mode :50-56

int gm_acq_manager_pacing_and_list(int mode, uint32_t active, uint64_t* interval_ms, uint32_t* mask) {
    if (!interval_ms || !mask) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    uint64_t interval; uint32_t size;                         // get_pacing_and_list :58-73
    switch (mode) {
        case 0: interval = 500; size = 32; break;
        case 1: interval = 1000; size = 8; break;
        case 2: interval = 2000; size = 5; break;
        default: return set_err(GM_ERR_INVALID_ARG, "mode must be 0..2");
    }
    uint32_t m = 0, taken = 0;
    for (uint32_t prn = 1; prn <= 32 && taken < size; ++prn)
        if (!((active >> (prn - 1)) & 1u)) { m |= 1u << (prn - 1); ++taken; }
    *interval_ms = interval; *mask = m;
    return GM_OK;
}

}  // extern "C"

// ====================================================================== ring mirror (struct gm_ring is defined above)

extern "C" {

int gm_ring_create(size_t buf_size, gm_ring** out) {
    if (!out) return set_err(GM_ERR_INVALID_ARG, "null out");
    *out = nullptr;
    if (!buf_size || (buf_size & (buf_size - 1))) return set_err(GM_ERR_INVALID_ARG, "Buffer size must be a power of two");
    if (int rc = ensure_device(g_device)) return rc;
    gm_ring* r = new gm_ring();
    r->device = g_device; r->size = buf_size; r->mask = buf_size - 1;
    r->slot_samples = buf_size < gm_ring::SLOT_SAMPLES_MAX ? buf_size : gm_ring::SLOT_SAMPLES_MAX;
    hipError_t e = hipMalloc(&r->d_buf, buf_size * 8);
    if (e == hipSuccess) e = hipMemset(r->d_buf, 0, buf_size * 8);
    // hipMemset of device memory returns before the fill has run and is ordered on the NULL stream only; the ring's writers work on
    // NON-BLOCKING streams, which that stream does not order: without this wait the fill can land on top of the first blocks written
    // (seen in round 6 as a tracking run that differed from its twin by a few zeroed samples, only in a long-lived process)
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) { hipFree(r->d_buf); delete r; return hip_fail(e, "hipMalloc(ring)"); }
    *out = r;
    return GM_OK;
}

int gm_ring_destroy(gm_ring* r) {
    if (!r) return GM_OK;
    hipSetDevice(r->device);
    if (r->copy_stream) { hipStreamSynchronize(r->copy_stream); hipStreamDestroy(r->copy_stream); }
    if (r->fe_stream && r->fe_stream != r->copy_stream) { hipStreamSynchronize(r->fe_stream); hipStreamDestroy(r->fe_stream); }
    for (hipEvent_t e : r->h2d_done) if (e) hipEventDestroy(e);
    if (r->ev_enq) hipEventDestroy(r->ev_enq);
    for (int i = 0; i < gm_ring::SLOTS; ++i) {
        if (r->staging[i]) hipHostFree(r->staging[i]);
        if (r->slot_done[i]) hipEventDestroy(r->slot_done[i]);
    }
    hipFree(r->d_buf);
    delete r;
    return GM_OK;
}

// write_samples without blocking the producer on the H2D copy: the samples are staged in pinned host
// memory, copied on the ring's own stream, and `head` advances (and the Condvar fires) only once they are in HBM, so a
// reader that sees the new head may launch kernels on the mirror without any stream dependency.  Single writer, like
// the reference ring; do not mix with gm_ring_write_samples without a gm_ring_flush in between.
int gm_ring_write_samples_async(gm_ring* r, const gm_c32* s, size_t n) {
    if (!r || (!s && n)) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (n > r->size) return set_err(GM_ERR_OUT_OF_RANGE, "write larger than the ring");
    if (int rc = ensure_device(r->device)) return rc;
    if (int rc = ring_async_init(r)) return rc;
    const cf* src = reinterpret_cast<const cf*>(s);
    while (n) {
        const size_t chunk = n < r->slot_samples ? n : r->slot_samples;
        int slot = 0;
        if (int rc = ring_begin_block(r, &slot)) return rc;
        memcpy(r->staging[slot], src, chunk * 8);
        const size_t start = size_t(r->write_pos & r->mask);
        const size_t first = start + chunk <= r->size ? chunk : r->size - start;
        HIPC(hipMemcpyAsync(r->d_buf + start, r->staging[slot], first * 8, hipMemcpyHostToDevice, r->copy_stream));
        if (first < chunk)
            HIPC(hipMemcpyAsync(r->d_buf, r->staging[slot] + first, (chunk - first) * 8, hipMemcpyHostToDevice, r->copy_stream));
        if (int rc = ring_end_block(r, slot, r->copy_stream, chunk)) return rc;
        src += chunk; n -= chunk;
    }
    return GM_OK;
}

int gm_ring_flush(gm_ring* r) {
    if (!r) return set_err(GM_ERR_INVALID_ARG, "null ring");
    if (!r->copy_stream) return GM_OK;
    if (int rc = ensure_device(r->device)) return rc;
    HIPC(hipStreamSynchronize(r->copy_stream));
    if (r->fe_stream) HIPC(hipStreamSynchronize(r->fe_stream));
    ring_refresh_head(r, true);
    return GM_OK;
}

// The Condvar wait of do_tracking::run (do_tracking.rs:392-406): sleep until head has reached `required_idx`
// (wrapping signed comparison like :393) or timeout_ms has passed.  *reached = 1 / 0.
int gm_ring_wait_head(gm_ring* r, uint64_t required_idx, uint32_t timeout_ms, int* reached) {
    if (!r) return set_err(GM_ERR_INVALID_ARG, "null ring");
    auto ok = [&] { return int64_t(r->head.load(std::memory_order_acquire) - required_idx) >= 0; };
    if (r->copy_stream) { if (int rc = ensure_device(r->device)) return rc; }
    // the asynchronous writer's chunks are retired by whoever looks (ring_refresh_head): look, then sleep on the Condvar in short
    // slices (a synchronous writer, or another reader's refresh, notifies it) until the head is there or the time is up
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(timeout_ms);
    bool got = false;
    for (;;) {
        ring_refresh_head(r);
        if ((got = ok())) break;
        const auto now = std::chrono::steady_clock::now();
        if (now >= deadline) break;
        std::unique_lock<std::mutex> g(r->notifier);
        auto slice = std::chrono::microseconds(100);
        if (deadline - now < slice) slice = std::chrono::duration_cast<std::chrono::microseconds>(deadline - now);
        if ((got = r->condvar.wait_for(g, slice, ok))) break;
    }
    if (reached) *reached = got ? 1 : 0;
    return GM_OK;
}

int gm_ring_write_samples(gm_ring* r, const gm_c32* s, size_t n) {
    if (!r || (!s && n)) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (n > r->size) return set_err(GM_ERR_OUT_OF_RANGE, "write larger than the ring");
    if (int rc = ensure_device(r->device)) return rc;
    if (r->copy_stream) {       // chunks of the asynchronous writer still in flight: land and retire them first, so that `head` is the
        HIPC(hipStreamSynchronize(r->copy_stream));      // writer's position (a synchronous write placed at a stale head would overwrite them)
        if (r->fe_stream) HIPC(hipStreamSynchronize(r->fe_stream));
        ring_refresh_head(r, true);
    }
    const uint64_t cur = r->head.load(std::memory_order_relaxed);
    const size_t start = size_t(cur & r->mask);
    if (start + n <= r->size) {
        HIPC(hipMemcpy(r->d_buf + start, s, n * 8, hipMemcpyHostToDevice));
    } else {
        const size_t first = r->size - start;
        HIPC(hipMemcpy(r->d_buf + start, s, first * 8, hipMemcpyHostToDevice));
        HIPC(hipMemcpy(r->d_buf, s + first, (n - first) * 8, hipMemcpyHostToDevice));
    }
    r->write_pos = cur + n;
    ring_publish(r, cur + n);
    return GM_OK;
}

int gm_ring_get_head(gm_ring* r, uint64_t* head) {
    if (!r || !head) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (r->copy_stream) { if (int rc = ensure_device(r->device)) return rc; ring_refresh_head(r); }
    *head = r->head.load(std::memory_order_acquire);
    return GM_OK;
}

int gm_ring_get_enqueued_head(gm_ring* r, uint64_t* head) {
    if (!r || !head) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    uint64_t h = r->head.load(std::memory_order_acquire);
    {
        std::lock_guard<std::mutex> g(r->enq_mu);
        if (r->ev_enq_armed && int64_t(r->enqueued - h) > 0) h = r->enqueued;
    }
    *head = h;
    return GM_OK;
}

int gm_ring_copy_to_slice(gm_ring* r, uint64_t start, gm_c32* dest, size_t n) {
    if (!r || (!dest && n)) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (n > r->size) return set_err(GM_ERR_OUT_OF_RANGE, "slice larger than the ring");
    if (int rc = ensure_device(r->device)) return rc;
    const size_t ps = size_t(start & r->mask);
    if (ps + n <= r->size) {
        HIPC(hipMemcpy(dest, r->d_buf + ps, n * 8, hipMemcpyDeviceToHost));
    } else {
        const size_t first = r->size - ps;
        HIPC(hipMemcpy(dest, r->d_buf + ps, first * 8, hipMemcpyDeviceToHost));
        HIPC(hipMemcpy(dest + first, r->d_buf, (n - first) * 8, hipMemcpyDeviceToHost));
    }
    return GM_OK;
}

}  // extern "C"

// ====================================================================== plane ring: P rings on one time axis, written from device memory
// gnss_mi355x.h states the contract.  One writer; the head counts what has been ENQUEUED.  `mu` guards the head and the events: the
// writer and the readers (tracking handles, gm_plane_ring_copy_to_slice) may be different host threads.
struct gm_plane_ring {
    int device = -1;
    cf* d_buf = nullptr;                  // [P][size]
    uint32_t P = 0;
    uint64_t size = 0, mask = 0;
    hipStream_t own_stream = nullptr;     // non-blocking: the writer's stream when the caller names none, and gm_plane_ring_copy_to_slice's
    std::mutex mu;
    uint64_t enqueued = 0;                // samples per plane whose writes have been enqueued
    hipEvent_t ev_write = nullptr;        // recorded behind every write
    bool write_armed = false;
    hipStream_t last_stream = nullptr;    // the stream ev_write was last recorded on
    // one event per reader stream, recorded behind every tracking launch on the ring; the next write waits for the armed ones
    struct Reader { hipStream_t st; hipEvent_t ev; bool armed; };
    std::vector<Reader> readers;
};
static constexpr uint32_t PLANE_RING_MAX_PLANES = 64;
static constexpr uint64_t PLANE_RING_MAX_BYTES = 1ull << 34;
static constexpr size_t PLANE_RING_MAX_READERS = 64;

static int plane_ring_rules(uint32_t n_planes, uint64_t plane_size, uint64_t* bytes) {
    if (n_planes < 1 || n_planes > PLANE_RING_MAX_PLANES) return set_err(GM_ERR_OUT_OF_RANGE, "n_planes must be in 1 .. 64");
    if (!plane_size || (plane_size & (plane_size - 1))) return set_err(GM_ERR_OUT_OF_RANGE, "plane_size must be a power of two");
    if (plane_size > PLANE_RING_MAX_BYTES / 8 / n_planes) return set_err(GM_ERR_OUT_OF_RANGE, "n_planes * plane_size * 8 must be at most 2^34 bytes");
    if (bytes) *bytes = uint64_t(n_planes) * plane_size * 8;
    return GM_OK;
}
// `st` is about to write the ring: behind the last write where that went to another stream, and behind every reader still armed
static int plane_ring_before_write(gm_plane_ring* r, hipStream_t st) {
    if (r->write_armed && r->last_stream != st) HIPC(hipStreamWaitEvent(st, r->ev_write, 0));
    for (auto& rd : r->readers)
        if (rd.armed) { HIPC(hipStreamWaitEvent(st, rd.ev, 0)); rd.armed = false; }      // (later writes are ordered behind this one)
    return GM_OK;
}
static int plane_ring_after_write(gm_plane_ring* r, hipStream_t st, uint64_t n) {
    HIPC(hipEventRecord(r->ev_write, st));
    r->last_stream = st; r->write_armed = true;
    r->enqueued += n;
    return GM_OK;
}
// a reader on `st`: behind everything the writer has enqueued; *head = the enqueued head it may then use.  Call with r->mu held.
static int plane_ring_begin_read(gm_plane_ring* r, hipStream_t st, uint64_t* head) {
    if (r->write_armed) HIPC(hipStreamWaitEvent(st, r->ev_write, 0));
    *head = r->enqueued;
    return GM_OK;
}
// the reader's launches are on `st`: its event, which the next write waits for.  Call with r->mu held.
static int plane_ring_end_read(gm_plane_ring* r, hipStream_t st) {
    gm_plane_ring::Reader* slot = nullptr;
    for (auto& rd : r->readers)
        if (rd.st == st) { slot = &rd; break; }
    if (!slot && r->readers.size() >= PLANE_RING_MAX_READERS) {      // more reader streams than places: take one whose launches have run
        for (auto& rd : r->readers)
            if (!rd.armed) { slot = &rd; break; }
        if (!slot) { slot = &r->readers[0]; HIPC(hipEventSynchronize(slot->ev)); }
        slot->st = st;
    }
    if (!slot) {
        hipEvent_t ev = nullptr;
        HIPC(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        r->readers.push_back(gm_plane_ring::Reader{st, ev, false});
        slot = &r->readers.back();
    }
    HIPC(hipEventRecord(slot->ev, st));
    slot->armed = true;
    return GM_OK;
}
static int plane_ring_write_rules(const gm_plane_ring* r, const void* src, size_t in_stride, size_t n) {
    if (!r || !src) return set_err(GM_ERR_INVALID_ARG, "null plane ring or planes");
    if (n > r->size) return set_err(GM_ERR_OUT_OF_RANGE, "write larger than a plane");
    if (in_stride < n) return set_err(GM_ERR_OUT_OF_RANGE, "in_stride below n");
    return GM_OK;
}

extern "C" {

int gm_plane_ring_plan(uint32_t n_planes, uint64_t plane_size, uint64_t* bytes) { return plane_ring_rules(n_planes, plane_size, bytes); }

int gm_plane_ring_create(uint32_t n_planes, uint64_t plane_size, gm_plane_ring** out) {
    if (!out) return set_err(GM_ERR_INVALID_ARG, "null out");
    *out = nullptr;
    uint64_t bytes = 0;
    if (int rc = plane_ring_rules(n_planes, plane_size, &bytes)) return rc;
    if (int rc = ensure_device(g_device)) return rc;
    gm_plane_ring* r = new gm_plane_ring();
    r->device = g_device; r->P = n_planes; r->size = plane_size; r->mask = plane_size - 1;
    hipError_t e = hipMalloc(&r->d_buf, bytes);
    if (e == hipSuccess) e = hipMemset(r->d_buf, 0, bytes);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);      // the fill has run before a non-blocking stream can write (gm_ring_create)
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&r->own_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&r->ev_write, hipEventDisableTiming);
    if (e != hipSuccess) { gm_plane_ring_destroy(r); return hip_fail(e, "gm_plane_ring_create"); }
    *out = r;
    return GM_OK;
}

int gm_plane_ring_destroy(gm_plane_ring* r) {
    if (!r) return GM_OK;
    hipSetDevice(r->device);
    if (r->write_armed) hipEventSynchronize(r->ev_write);
    for (auto& rd : r->readers) { if (rd.armed) hipEventSynchronize(rd.ev); hipEventDestroy(rd.ev); }
    if (r->own_stream) { hipStreamSynchronize(r->own_stream); hipStreamDestroy(r->own_stream); }
    if (r->ev_write) hipEventDestroy(r->ev_write);
    hipFree(r->d_buf);
    delete r;
    return GM_OK;
}

int gm_plane_ring_info(gm_plane_ring* r, uint32_t* n_planes, uint64_t* plane_size, uint64_t* bytes, void** d_base) {
    if (!r) return set_err(GM_ERR_INVALID_ARG, "null plane ring");
    if (n_planes) *n_planes = r->P;
    if (plane_size) *plane_size = r->size;
    if (bytes) *bytes = uint64_t(r->P) * r->size * 8;
    if (d_base) *d_base = r->d_buf;
    return GM_OK;
}

int gm_plane_ring_write_dev(gm_plane_ring* r, const void* d_planes, size_t in_stride, size_t n, void* stream) {
    if (int rc = plane_ring_write_rules(r, d_planes, in_stride, n)) return rc;
    if (!n) return GM_OK;
    {   // the source range [d_planes, d_planes + (P - 1) * in_stride + n) may not touch the ring
        const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_planes), r0 = reinterpret_cast<uintptr_t>(r->d_buf);
        const unsigned __int128 s_len = ((unsigned __int128)(r->P - 1) * in_stride + n) * 8, r_len = (unsigned __int128)r->P * r->size * 8;
        if ((unsigned __int128)s0 < (unsigned __int128)r0 + r_len && (unsigned __int128)r0 < (unsigned __int128)s0 + s_len)
            return set_err(GM_ERR_OUT_OF_RANGE, "the source planes overlap the ring");
    }
    if (int rc = ensure_device(r->device)) return rc;
    hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : r->own_stream;
    std::lock_guard<std::mutex> g(r->mu);
    if (int rc = plane_ring_before_write(r, st)) return rc;
    gm::PlaneRingWriteArgs a;
    a.src = static_cast<const cf*>(d_planes); a.ring = r->d_buf;
    a.in_stride = in_stride; a.plane_size = r->size; a.start = r->enqueued & r->mask; a.n = n; a.n_planes = r->P;
    a.wide = (reinterpret_cast<uintptr_t>(d_planes) % 16 == 0 && in_stride % 2 == 0 && n % 2 == 0 && a.start % 2 == 0 && r->size % 2 == 0) ? 1 : 0;
    gm::launch_plane_ring_write(st, a);
    HIPC(hipGetLastError());
    return plane_ring_after_write(r, st, n);
}

int gm_plane_ring_write(gm_plane_ring* r, const gm_c32* planes, size_t in_stride, size_t n) {
    if (int rc = plane_ring_write_rules(r, planes, in_stride, n)) return rc;
    if (!n) return GM_OK;
    if (int rc = ensure_device(r->device)) return rc;
    std::lock_guard<std::mutex> g(r->mu);
    hipStream_t st = r->own_stream;
    if (int rc = plane_ring_before_write(r, st)) return rc;
    const uint64_t start = r->enqueued & r->mask, first = start + n <= r->size ? n : r->size - start;
    for (uint32_t p = 0; p < r->P; ++p) {
        const gm_c32* s = planes + size_t(p) * in_stride;
        cf* d = r->d_buf + uint64_t(p) * r->size;
        HIPC(hipMemcpyAsync(d + start, s, first * 8, hipMemcpyHostToDevice, st));
        if (first < n) HIPC(hipMemcpyAsync(d, s + first, (n - first) * 8, hipMemcpyHostToDevice, st));
    }
    if (int rc = plane_ring_after_write(r, st, n)) return rc;
    HIPC(hipStreamSynchronize(st));
    return GM_OK;
}

int gm_plane_ring_get_head(gm_plane_ring* r, uint64_t* head) {
    if (!r || !head) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    std::lock_guard<std::mutex> g(r->mu);
    *head = r->enqueued;
    return GM_OK;
}

int gm_plane_ring_copy_to_slice(gm_plane_ring* r, uint32_t plane, uint64_t start, gm_c32* dest, size_t n) {
    if (!r || (!dest && n)) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (plane >= r->P) return set_err(GM_ERR_OUT_OF_RANGE, "plane at or above n_planes");
    if (n > r->size) return set_err(GM_ERR_OUT_OF_RANGE, "slice larger than a plane");
    if (int rc = ensure_device(r->device)) return rc;
    if (!n) return GM_OK;
    hipStream_t st = r->own_stream;
    {
        std::lock_guard<std::mutex> g(r->mu);
        uint64_t head = 0;
        if (int rc = plane_ring_begin_read(r, st, &head)) return rc;
    }
    const cf* d = r->d_buf + uint64_t(plane) * r->size;
    const uint64_t ps = start & r->mask, first = ps + n <= r->size ? n : r->size - ps;
    HIPC(hipMemcpyAsync(dest, d + ps, first * 8, hipMemcpyDeviceToHost, st));
    if (first < n) HIPC(hipMemcpyAsync(dest + first, d, (n - first) * 8, hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));      // the copy has run before the call returns: no write can be waiting for it
    return GM_OK;
}

int gm_plane_ring_synchronize(gm_plane_ring* r) {
    if (!r) return set_err(GM_ERR_INVALID_ARG, "null plane ring");
    if (int rc = ensure_device(r->device)) return rc;
    std::lock_guard<std::mutex> g(r->mu);
    if (r->write_armed) HIPC(hipEventSynchronize(r->ev_write));
    for (auto& rd : r->readers)
        if (rd.armed) { HIPC(hipEventSynchronize(rd.ev)); rd.armed = false; }
    return GM_OK;
}

}  // extern "C"

// ====================================================================== tracking handle
struct gm_trk {
    int device = -1;
    gm_trk_cfg cfg{};
    gm::TrkDevCfg dc{};
    hipStream_t stream = nullptr;
    bool own_stream = false;
    uint32_t C = 0;
    int slices = 1;
    std::vector<int8_t> h_codes;
    int8_t* d_codes = nullptr;
    gm_trk_state* d_states = nullptr;
    float* d_partials = nullptr;
    uint8_t* d_ready = nullptr;
    cf* d_scratch = nullptr; size_t scratch_cap = 0;
    float* d_terms = nullptr; size_t terms_cap = 0;   // strict_sum_order: [C][2 * arms][terms_cap] per-sample products of one epoch
    // results of a call of e passes, n = e * C entries: ONE device block laid out for that n as [outs n | processed n | lost n |
    // lost_prn n] (trk_reserve_epochs), so that outs + processed + lost leave in ONE device-to-host copy; d_outs .. d_lostprn point into it
    uint8_t* d_res = nullptr; size_t res_cap = 0, res_n = 0;
    gm_trk_out* d_outs = nullptr; uint8_t *d_proc = nullptr, *d_lost = nullptr, *d_lostprn = nullptr;
    uint8_t* h_res = nullptr; size_t h_cap = 0;    // pinned landing area of gm_trk_update_all: [outs | processed | lost] of the call's passes
    uint32_t epochs_cap = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timing = false; uint32_t timed_launches = 0;
    // persistent multi-epoch kernel: its launch layout (decided once, at create), granule exchange buffer, launch counter
    gm::TrkPersistPlan plan{};
    unsigned long long* d_xchg = nullptr;
    int* d_error = nullptr;             // host-pinned, device-visible: written by the kernel only when an exchange times out
    int* d_error_dev = nullptr;         // its device-memory twin, read by every later launch (trk_persistent_kernel)
    uint32_t launch_seq = 0;
    long long* d_stamps = nullptr; uint32_t stamps_cap = 0;   // diagnostic phase stamps (gm_trk_debug_stamps)
    // gm_trk_update_all_async: results of call k land in pinned slot k % TICKETS ([outs | processed | lost] of that call's epochs),
    // `done` recorded behind the copies; gm_trk_collect hands them over and frees the slot
    static constexpr int TICKETS = 8;
    struct Ticket { uint8_t* h = nullptr; hipEvent_t done = nullptr; bool in_flight = false; uint32_t epochs = 0; uint64_t id = 0; } tk[TICKETS];
    uint8_t* tk_block = nullptr;          // ONE pinned allocation cut into the TICKETS slots (a pinned allocation costs ~1 ms: not per slot, not in a receiver's loop)
    size_t tk_cap = 0;                    // bytes per slot
    uint64_t next_ticket = 1;
    // the known-record entries' device blocks: gm_trk_bank's [records | taps | offsets | out | done | partials] (trk_bank_run) and
    // gm_trk_array_prompts' [records | z | done | partials]
    CallBlock bank, array;
    // gm_trk_array_prompts_dev shares `array` with the synchronous entry: the stream the last array call of either kind went to (a call
    // on another stream waits for it on the host first, stage_join's rule), and the pinned copies of the records that calls still in
    // flight read: ONE pinned allocation cut into ARRAY_SLOTS equal slots of the largest call's records (1024), taken in turn; a slot
    // is taken again once the event behind its copy has passed
    hipStream_t array_last = nullptr;
    static constexpr int ARRAY_SLOTS = 16;
    uint8_t* array_recs = nullptr;        // [ARRAY_SLOTS][GM_TRK_ARRAY_MAX_STATES] TrkBankRec, built at the first device call
    hipEvent_t array_ev[ARRAY_SLOTS] = {};
    uint32_t array_next = 0;
    // gm_trk_update_planes: the plane of every channel (gm_trk_set_channel_planes).  h_planes is what the rules are checked against;
    // d_planes is what the kernel reads, installed on the handle's stream from the pinned planes_stage (planes_ev: that copy has run).
    // Both are made at the first entry that needs them; no other entry reads them.
    std::vector<uint32_t> h_planes;
    uint32_t* d_planes = nullptr;
    uint32_t* planes_stage = nullptr;
    hipEvent_t planes_ev = nullptr;
};

static int trk_check_error(gm_trk* t);
static int trk_reserve_tickets(gm_trk* t, size_t bytes);
// strict_sum_order: room for `samples` per-sample products per sum and channel
static int trk_reserve_terms(gm_trk* t, size_t samples) {
    samples = (samples + 3) & ~size_t(3);       // rows of the streams stay 16-byte aligned
    if (!t->dc.strict_sum_order || samples <= t->terms_cap) return GM_OK;
    HIPC(hipStreamSynchronize(t->stream));
    hipFree(t->d_terms); t->d_terms = nullptr; t->terms_cap = 0;
    HIPC(hipMalloc(&t->d_terms, size_t(t->C) * 2 * size_t(t->dc.n_arms) * samples * sizeof(float)));
    t->terms_cap = samples;
    return GM_OK;
}
static int trk_reserve_epochs(gm_trk* t, uint32_t e) {
    const size_t n = size_t(e) * t->C, bytes = (n * (sizeof(gm_trk_out) + 3) + 3) & ~size_t(3);
    if (bytes > t->res_cap) {
        HIPC(hipStreamSynchronize(t->stream));      // nothing in flight still writes the block about to be replaced
        hipFree(t->d_res); t->d_res = nullptr; t->res_cap = 0; t->res_n = 0;
        HIPC(hipMalloc(&t->d_res, bytes));
        t->res_cap = bytes;
    }
    if (n * (sizeof(gm_trk_out) + 2) > t->h_cap) {
        HIPC(hipStreamSynchronize(t->stream));
        if (t->h_res) { hipHostFree(t->h_res); t->h_res = nullptr; t->h_cap = 0; }
        HIPC(hipHostMalloc(reinterpret_cast<void**>(&t->h_res), n * (sizeof(gm_trk_out) + 2), hipHostMallocDefault));
        t->h_cap = n * (sizeof(gm_trk_out) + 2);
    }
    if (n != t->res_n) {
        // a new layout: with three arms the persistent kernel writes the six live sums only, ive..qvl must read 0 — and bytes that were
        // flags under the previous layout may now lie inside `outs`.  Ordered on the handle's stream (a non-blocking stream does not
        // synchronise with the NULL stream a plain hipMemset runs on).  A loop that keeps its pass count pays this once.
        HIPC(hipMemsetAsync(t->d_res, 0, bytes, t->stream));
        t->res_n = n;
    }
    t->d_outs = reinterpret_cast<gm_trk_out*>(t->d_res);
    t->d_proc = t->d_res + n * sizeof(gm_trk_out);
    t->d_lost = t->d_proc + n;
    t->d_lostprn = t->d_lost + n;
    if (e > t->epochs_cap) t->epochs_cap = e;
    return GM_OK;
}

extern "C" {

int gm_loop_filter_new(float bw, float zeta, float gain, float* tau1, float* tau2) {
    if (!tau1 || !tau2) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    loop_filter_new(bw, zeta, gain, tau1, tau2);
    return GM_OK;
}
float gm_loop_filter_update(float tau1, float tau2, float d_err, float err, float dt) {   // :68-70
    return d_err * (dt / tau1) + (d_err - err) * (tau2 / tau1);
}

int gm_trk_destroy(gm_trk* t) {
    if (!t) return GM_OK;
    if (t->device >= 0) hipSetDevice(t->device);
    hipFree(t->d_codes); hipFree(t->d_states); hipFree(t->d_partials); hipFree(t->d_ready); hipFree(t->d_scratch); hipFree(t->d_terms);
    if (t->array_last) hipStreamSynchronize(t->array_last);
    for (auto& e : t->array_ev) if (e) hipEventDestroy(e);
    if (t->array_recs) hipHostFree(t->array_recs);
    if (t->planes_ev) { hipEventSynchronize(t->planes_ev); hipEventDestroy(t->planes_ev); }
    if (t->planes_stage) hipHostFree(t->planes_stage);
    hipFree(t->d_planes);
    hipFree(t->d_res); t->bank.release(); t->array.release();
    if (t->h_res) hipHostFree(t->h_res);
    for (auto& k : t->tk) if (k.done) hipEventDestroy(k.done);
    if (t->tk_block) hipHostFree(t->tk_block);
    hipFree(t->d_xchg); if (t->d_error) hipHostFree(t->d_error); hipFree(t->d_error_dev); hipFree(t->d_stamps);
    if (t->ev0) hipEventDestroy(t->ev0);
    if (t->ev1) hipEventDestroy(t->ev1);
    if (t->own_stream && t->stream) hipStreamDestroy(t->stream);
    delete t;
    return GM_OK;
}

int gm_trk_create(const gm_trk_cfg* cfg, gm_trk** out) {
    if (!cfg || !out) return set_err(GM_ERR_INVALID_ARG, "null cfg/out");
    *out = nullptr;
    if (!(cfg->fs > 0) || !cfg->n_channels) return set_err(GM_ERR_INVALID_ARG, "fs and n_channels are required");
    const uint32_t arms = cfg->n_arms ? cfg->n_arms : 3;
    if (arms != 3 && arms != 5) return set_err(GM_ERR_INVALID_ARG, "n_arms must be 3 or 5");
    if (cfg->codes && (!cfg->n_codes || !cfg->code_len)) return set_err(GM_ERR_INVALID_ARG, "n_codes/code_len required");
    if (cfg->codes && cfg->code_len > (1u << 24)) return set_err(GM_ERR_OUT_OF_RANGE, "code_len beyond 2^24 chips (chip phases are f32)");
    {   // the kernels replace `% code_len` by one conditional subtraction: arm spacings must stay below a code period
        const float len = cfg->codes ? float(cfg->code_len) : 1023.0f;
        if (cfg->early_late_space >= len || cfg->very_early_late_space >= len || cfg->early_late_space < 0 ||
            cfg->very_early_late_space < 0)
            return set_err(GM_ERR_INVALID_ARG, "arm spacing must be in [0, code_len)");
    }
    if (int rc = ensure_device(g_device)) return rc;
    gm_trk* t = new gm_trk();
    t->device = g_device; t->cfg = *cfg; t->C = cfg->n_channels;
    gm::TrkDevCfg& d = t->dc;
    d.fs = cfg->fs; d.n_channels = int(cfg->n_channels); d.n_arms = int(arms);
    d.el_space = cfg->early_late_space > 0 ? cfg->early_late_space : 0.5f;
    d.vel_space = cfg->very_early_late_space > 0 ? cfg->very_early_late_space : 1.0f;
    d.code_index_mode = cfg->code_index_mode; d.boc11 = cfg->boc11;
    d.strict_libm = cfg->strict_libm ? 1 : 0;
    d.strict_sum_order = cfg->strict_sum_order ? 1 : 0;
    d.gps_ca = cfg->codes ? 0 : 1;
    d.code_len = cfg->codes ? int(cfg->code_len) : 1023;
    d.code_len_f = float(d.code_len);
    d.n_codes = cfg->codes ? int(cfg->n_codes) : 32;
    d.lock_threshold = cfg->lock_threshold > 0 ? cfg->lock_threshold : 15.0f;
    d.max_lost_epochs = cfg->max_lost_epochs ? cfg->max_lost_epochs : 20u;
    loop_filter_new(cfg->pll_bw > 0 ? cfg->pll_bw : 25.0f, cfg->pll_zeta > 0 ? cfg->pll_zeta : 0.7f,
                    cfg->pll_gain > 0 ? cfg->pll_gain : 0.25f, &d.pll_tau1, &d.pll_tau2);
    loop_filter_new(cfg->dll_bw > 0 ? cfg->dll_bw : 2.0f, cfg->dll_zeta > 0 ? cfg->dll_zeta : 0.7f,
                    cfg->dll_gain > 0 ? cfg->dll_gain : 1.0f, &d.dll_tau1, &d.dll_tau2);
    d.pll_dt = cfg->pll_dt > 0 ? cfg->pll_dt : 0.001f;
    d.dll_dt = cfg->dll_dt > 0 ? cfg->dll_dt : 0.001f;
    d.nominal_code_rate = cfg->nominal_code_rate > 0 ? cfg->nominal_code_rate : CA_RATE;
    gm::fill_trk_derived(d);
    // The persistent kernel's launch layout (trk_persist_plan.h) from what the device says about the instantiation(s) this
    // configuration can launch and the diagnostic overrides, which are read here and nowhere else.
    gm::TrkPersistKnobs knobs;
    knobs.g = gm::diag_int("GM_TRK_G", knobs.g); knobs.packed = gm::diag_int("GM_TRK_PACKED", knobs.packed);
    knobs.packed_g = gm::diag_int("GM_TRK_PACKED_G", knobs.packed_g); knobs.stagger_k = gm::diag_int("GM_TRK_STAGGER_K", knobs.stagger_k);
    knobs.fair = gm::diag_int("GM_TRK_FAIR", knobs.fair);
    {   // the kernel keeps the channel's chip row in LDS as floats (three tables of it for BOC): a code that cannot fit is
        // refused here, from the kernel's own static size and the device's limit, not found out by a launch that fails
        gm::TrkPersistProbe probe;
        const hipError_t e = gm::trk_persist_probe(d, knobs, t->device, &probe);
        if (e != hipSuccess) { gm_trk_destroy(t); return hip_fail(e, "trk_persist_probe"); }
        const size_t need = probe.static_lds + gm::trk_persist_lds_bytes(d), limit = probe.lds_limit;
        if (need > limit) {
            gm_trk_destroy(t);
            char msg[192];
            snprintf(msg, sizeof(msg), "code_len %d needs %zu bytes of LDS per workgroup (chip tables + the kernel's own), the device allows %zu bytes",
                     d.code_len, need, limit);
            return set_err(GM_ERR_OUT_OF_RANGE, msg);
        }
        t->plan = gm::trk_persist_plan(d, cfg->share_device != 0, probe.dev, knobs);
        if (gm::diag_int("GM_TRK_PLAN_PRINT", 0) != 0) {      // diagnostic: what the device said and what was decided (tools/trk_persist_plan_ab.py)
            const gm::TrkPersistPlan& p = t->plan;
            fprintf(stderr, "gm_trk plan: key %d strict %d fair3 %d | cus %d per_cu_plain %d per_cu_fair %d static_lds %zu | G %d packed %d grid %d per %u "
                    "fair_share %d lds %zu xchg %zu\n", p.key, p.strict, p.fair3, probe.dev.cus, probe.dev.per_cu_plain, probe.dev.per_cu_fair,
                    probe.static_lds, p.G, p.packed, p.grid, p.per, p.fair_share, p.lds_bytes, p.xchg_bytes);
        }
    }
    if (cfg->codes) t->h_codes.assign(cfg->codes, cfg->codes + size_t(cfg->n_codes) * cfg->code_len);
    else t->h_codes.assign(&ca_table().rows[0][0], &ca_table().rows[0][0] + 32 * 1023);

    // slices per channel: fill the chip (>= ~1000 workgroups) without going under 256 samples each
    const size_t n_nom = num_samples_per_code(d.nominal_code_rate, d.fs, d.code_len_f);
    size_t target = (1024 + t->C - 1) / t->C;
    if (target < 1) target = 1;
    size_t per = ((n_nom + target - 1) / target + 255) / 256 * 256;
    if (per < 256) per = 256;
    size_t s = (n_nom + per - 1) / per;
    t->slices = int(s < 1 ? 1 : (s > 256 ? 256 : s));

    auto fail = [&](int code) { gm_trk_destroy(t); return code; };
#define HIPT(expr)                                                     \
    do {                                                               \
        hipError_t _e = (expr);                                        \
        if (_e != hipSuccess) return fail(hip_fail(_e, #expr));        \
    } while (0)
    {   // the tracking loop is the receiver's latency path (one short launch per block of samples): its own stream is the device's
        // most urgent one, so a launch is not queued behind a front-end block or an acquisition dwell in flight on another stream
        // (measured: 0.45 ms of waiting per call behind the front-end kernel of the same block, tools/trk_call_time.py)
        int least = 0, greatest = 0;
        HIPT(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIPT(hipStreamCreateWithPriority(&t->stream, hipStreamNonBlocking, greatest));
    }
    t->own_stream = true;
    HIPT(hipMalloc(&t->d_codes, t->h_codes.size()));
    HIPT(hipMemcpy(t->d_codes, t->h_codes.data(), t->h_codes.size(), hipMemcpyHostToDevice));
    HIPT(hipMalloc(&t->d_states, sizeof(gm_trk_state) * t->C));
    std::vector<gm_trk_state> init(t->C);
    for (auto& st : init) {   // TrackingChannel::new :118-146
        memset(&st, 0, sizeof(st));
        st.num_samples_per_code = n_nom;
        st.code_rate = d.nominal_code_rate;
    }
    HIPT(hipMemcpy(t->d_states, init.data(), sizeof(gm_trk_state) * t->C, hipMemcpyHostToDevice));
    HIPT(hipMalloc(&t->d_partials, sizeof(float) * t->C * size_t(t->slices) * 10));
    HIPT(hipMalloc(&t->d_ready, t->C));
    HIPT(hipMemsetAsync(t->d_ready, 0, t->C, t->stream));      // (the handle's stream is non-blocking: a NULL-stream memset would not be ordered with it)
    HIPT(hipEventCreate(&t->ev0));
    HIPT(hipEventCreate(&t->ev1));
    {   // the exchange block of the persistent kernel's workgroups, and its time-out flag
        HIPT(hipMalloc(&t->d_xchg, t->plan.xchg_bytes));
        HIPT(hipMemsetAsync(t->d_xchg, 0, t->plan.xchg_bytes, t->stream));
        HIPT(hipHostMalloc(reinterpret_cast<void**>(&t->d_error), sizeof(int), hipHostMallocDefault));   // read on the host after a stream sync: no copy
        *t->d_error = 0;
        HIPT(hipMalloc(&t->d_error_dev, sizeof(int)));
        HIPT(hipMemsetAsync(t->d_error_dev, 0, sizeof(int), t->stream));
    }
    if (int rc = trk_reserve_epochs(t, 1)) return fail(rc);
    if (int rc = trk_reserve_tickets(t, size_t(128) * t->C * (sizeof(gm_trk_out) + 2))) return fail(rc);     // gm_trk_update_all_async's result slots
    HIPT(hipStreamSynchronize(t->stream));      // the clears above have landed before any caller-supplied stream (gm_trk_set_stream) can run a kernel
#undef HIPT
    *out = t;
    return GM_OK;
}

int gm_trk_set_stream(gm_trk* t, void* s) {
    if (!t) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (t->own_stream && t->stream) { hipStreamSynchronize(t->stream); hipStreamDestroy(t->stream); }
    t->stream = reinterpret_cast<hipStream_t>(s);
    t->own_stream = false;
    return GM_OK;
}

int gm_trk_get_state(gm_trk* t, uint32_t ch, gm_trk_state* out) {
    if (!t || !out || ch >= t->C) return set_err(GM_ERR_INVALID_ARG, "bad channel");
    if (int rc = ensure_device(t->device)) return rc;
    HIPC(hipStreamSynchronize(t->stream));
    HIPC(hipMemcpy(out, t->d_states + ch, sizeof(*out), hipMemcpyDeviceToHost));
    return GM_OK;
}

int gm_trk_set_state(gm_trk* t, uint32_t ch, const gm_trk_state* in) {
    if (!t || !in || ch >= t->C) return set_err(GM_ERR_INVALID_ARG, "bad channel");
    if (int rc = ensure_device(t->device)) return rc;
    HIPC(hipStreamSynchronize(t->stream));
    HIPC(hipMemcpy(t->d_states + ch, in, sizeof(*in), hipMemcpyHostToDevice));
    return GM_OK;
}

int gm_trk_get_states(gm_trk* t, gm_trk_state* out) {
    if (!t || !out) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (int rc = ensure_device(t->device)) return rc;
    HIPC(hipStreamSynchronize(t->stream));
    HIPC(hipMemcpy(out, t->d_states, size_t(t->C) * sizeof(*out), hipMemcpyDeviceToHost));
    return GM_OK;
}

int gm_trk_set_states(gm_trk* t, const gm_trk_state* in, const uint8_t* which) {
    if (!t || !in) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (int rc = ensure_device(t->device)) return rc;
    HIPC(hipStreamSynchronize(t->stream));
    if (!which) {
        HIPC(hipMemcpy(t->d_states, in, size_t(t->C) * sizeof(*in), hipMemcpyHostToDevice));
        return GM_OK;
    }
    for (uint32_t c = 0; c < t->C; ) {          // runs of flagged channels, one copy each
        if (!which[c]) { ++c; continue; }
        uint32_t e = c;
        while (e < t->C && which[e]) ++e;
        HIPC(hipMemcpy(t->d_states + c, in + c, size_t(e - c) * sizeof(*in), hipMemcpyHostToDevice));
        c = e;
    }
    return GM_OK;
}

int gm_trk_start(gm_trk* t, uint32_t ch, const gm_acq_result* r) {   // :148-154
    if (!t || !r || ch >= t->C) return set_err(GM_ERR_INVALID_ARG, "bad channel");
    gm_trk_state s;
    if (int rc = gm_trk_get_state(t, ch, &s)) return rc;
    s.prn = r->prn;
    s.carrier_freq = r->carrier_freq;
    s.code_phase = r->code_phase_chips;
    s.next_sample_index = r->sample_global_index;
    s.active = 1;
    // FIXED: sample_global_index already points at the code start, so the replica starts at chip 0 (the reference
    // passes the acquisition delay in chips AND the aligned sample index)
    if (t->cfg.code_index_mode == GM_CODE_INDEX_FIXED) s.code_phase = 0.0f;
    if (t->cfg.code_index_mode == GM_CODE_INDEX_FIXED && s.code_rate == 0.0f)
        s.code_rate = t->dc.nominal_code_rate;   // FIXED: undo reset()'s code_rate = 0 (reference bug)
    return gm_trk_set_state(t, ch, &s);
}

int gm_trk_reset(gm_trk* t, uint32_t ch) {   // :311-327
    if (!t || ch >= t->C) return set_err(GM_ERR_INVALID_ARG, "bad channel");
    gm_trk_state s;
    if (int rc = gm_trk_get_state(t, ch, &s)) return rc;
    const uint64_t n = s.num_samples_per_code;
    memset(&s, 0, sizeof(s));
    s.num_samples_per_code = n;   // reset() leaves num_samples_per_code untouched
    return gm_trk_set_state(t, ch, &s);
}

int gm_trk_get_ca_chip(gm_trk* t, uint32_t ch, float phase, float* chip) {   // :274-277
    if (!t || !chip || ch >= t->C) return set_err(GM_ERR_INVALID_ARG, "bad channel");
    gm_trk_state s;
    if (int rc = gm_trk_get_state(t, ch, &s)) return rc;
    const int len = t->dc.code_len;
    int row, idx;
    const float f = floorf(phase);
    if (t->dc.code_index_mode == GM_CODE_INDEX_FAITHFUL) {
        row = t->dc.gps_ca ? int(s.prn) : int(s.prn) - 1;
        if (!(f > 0.0f)) idx = 0;
        else if (f >= 18446744073709551616.0f) idx = int(18446744073709551615ull % (unsigned long long)len);
        else idx = int((unsigned long long)f % (unsigned long long)len);
    } else {
        row = int(s.prn) - 1;
        long li = long(f) % len;
        idx = int(li < 0 ? li + len : li);
    }
    if (row < 0 || row >= t->dc.n_codes) return set_err(GM_ERR_OUT_OF_RANGE, "code table row out of bounds (the reference panics)");
    *chip = float(t->h_codes[size_t(row) * len + idx]);
    return GM_OK;
}

static int trk_unit(gm_trk* t, uint32_t ch, const gm_c32* samples, size_t n, int mode, gm_trk_out* out, uint8_t* lost,
                    uint8_t* lost_prn) {
    if (!t || !samples || !out || ch >= t->C) return set_err(GM_ERR_INVALID_ARG, "bad argument");
    if (int rc = ensure_device(t->device)) return rc;
    gm_trk_state s;
    if (int rc = gm_trk_get_state(t, ch, &s)) return rc;
    if (n < s.num_samples_per_code || s.num_samples_per_code == 0)
        return set_err(GM_ERR_OUT_OF_RANGE, "fewer samples than num_samples_per_code (the reference panics)");
    const int row = t->dc.gps_ca ? (t->dc.code_index_mode == GM_CODE_INDEX_FAITHFUL ? int(s.prn) : int(s.prn) - 1)
                                 : int(s.prn) - 1;
    if (row < 0 || row >= t->dc.n_codes) return set_err(GM_ERR_OUT_OF_RANGE, "code table row out of bounds (the reference panics)");
    const size_t need = s.num_samples_per_code;
    if (need > t->scratch_cap) {
        hipFree(t->d_scratch); t->d_scratch = nullptr; t->scratch_cap = 0;
        HIPC(hipMalloc(&t->d_scratch, need * 8 * 2));
        t->scratch_cap = need * 2;
    }
    if (int rc = trk_reserve_terms(t, need)) return rc;
    if (int rc = trk_reserve_epochs(t, 1)) return rc;          // the result block laid out for one pass
    HIPC(hipMemcpyAsync(t->d_scratch, samples, need * 8, hipMemcpyHostToDevice, t->stream));
    // the unit entries run regardless of ChannelState (the reference's early_late_correlation/do_work do not test it)
    const uint8_t was_active = s.active;
    if (!was_active) { s.active = 1; HIPC(hipMemcpyAsync(t->d_states + ch, &s, sizeof(s), hipMemcpyHostToDevice, t->stream)); HIPC(hipStreamSynchronize(t->stream)); }
    gm::TrkSrc src;
    src.base = t->d_scratch; src.mask = ~0ull; src.head = 0; src.linear = 1; src.only_channel = int(ch);
    gm::launch_trk_epoch(t->stream, t->dc, t->d_codes, t->d_states, src, t->slices, t->d_partials, t->d_ready, mode,
                         t->d_outs, t->d_proc, t->d_lost, t->d_lostprn, t->d_terms, t->terms_cap, t->d_error);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(t->stream));
    HIPC(hipMemcpy(out, t->d_outs + ch, sizeof(*out), hipMemcpyDeviceToHost));
    uint8_t l = 0, lp = 0;
    HIPC(hipMemcpy(&l, t->d_lost + ch, 1, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(&lp, t->d_lostprn + ch, 1, hipMemcpyDeviceToHost));
    if (lost) *lost = l;
    if (lost_prn) *lost_prn = lp;
    if (!was_active && !l) {   // restore the caller's ChannelState
        gm_trk_state s2;
        HIPC(hipMemcpy(&s2, t->d_states + ch, sizeof(s2), hipMemcpyDeviceToHost));
        s2.active = 0;
        HIPC(hipMemcpy(t->d_states + ch, &s2, sizeof(s2), hipMemcpyHostToDevice));
    }
    return GM_OK;
}

int gm_trk_correlate(gm_trk* t, uint32_t ch, const gm_c32* samples, size_t n, gm_trk_out* out) {
    return trk_unit(t, ch, samples, n, gm::TRK_MODE_CORRELATE, out, nullptr, nullptr);
}
int gm_trk_do_work(gm_trk* t, uint32_t ch, const gm_c32* samples, size_t n, gm_trk_out* out, uint8_t* lost, uint8_t* lost_prn) {
    return trk_unit(t, ch, samples, n, gm::TRK_MODE_DO_WORK, out, lost, lost_prn);
}

}  // extern "C"

// ---- gm_trk_bank: taps x carrier offsets at caller-supplied records (gnss_mi355x.h states the definition and the limits) -------------
// ---- known records on gm_trk: what gm_trk_bank and gm_trk_array_prompts share beyond CallBlock and Carve ---------------------------------
// the rules both plans begin with
static int trk_call_rules(const void* cfg, const char* null_cfg_text, float fs, bool custom_codes, uint32_t n_codes, uint32_t code_len) {
    if (!cfg) return set_err(GM_ERR_INVALID_ARG, null_cfg_text);
    if (!(fs > 0) || !std::isfinite(fs)) return set_err(GM_ERR_INVALID_ARG, "fs is required");
    if (custom_codes && (!n_codes || !code_len)) return set_err(GM_ERR_INVALID_ARG, "n_codes/code_len required");
    return GM_OK;
}
static int trk_call_states_rule(const gm_trk* t, const gm_trk_state* states, uint32_t n_states) {
    if (!states && n_states != t->C) return set_err(GM_ERR_INVALID_ARG, "states NULL: n_states must be n_channels");
    return GM_OK;
}
// n = round(fs / (code_rate / code_len)) as the tracker forms it (trk_kernels.hip samples_per_code); false: a record with this n is skipped
static bool trk_bank_samples_per_code(float fs, float code_rate, float lenf, uint32_t& n) {
    const float v = roundf(fs / (code_rate / lenf));
    n = 0;
    if (!(v > 0.0f) || !(v < 2147483648.0f)) return false;
    n = uint32_t(v);
    return true;
}
static int trk_bank_row(const gm_trk* t, const gm_trk_state& s) {      // trk_kernels.hip code_row
    return t->dc.gps_ca ? (t->dc.code_index_mode == GM_CODE_INDEX_FAITHFUL ? int(s.prn) : int(s.prn) - 1) : int(s.prn) - 1;
}
// the records of a call, from `states` or the handle's own channels as they stand: n, and run = active with a code row and a sample
// count; the caller's window gate may clear run
static int trk_call_records(gm_trk* t, const gm_trk_state* states, uint32_t n_states, std::vector<gm::TrkBankRec>& recs) {
    recs.assign(n_states, gm::TrkBankRec{});
    if (states) {
        for (uint32_t r = 0; r < n_states; ++r) recs[r].st = states[r];
    } else {
        std::vector<gm_trk_state> own(t->C);
        if (int rc = gm_trk_get_states(t, own.data())) return rc;
        for (uint32_t r = 0; r < n_states; ++r) recs[r].st = own[r];
    }
    for (auto& r : recs) {
        const int row = trk_bank_row(t, r.st);
        r.run = (r.st.active && row >= 0 && row < t->dc.n_codes && trk_bank_samples_per_code(t->dc.fs, r.st.code_rate, t->dc.code_len_f, r.n)) ? 1 : 0;
    }
    return GM_OK;
}
// slices of `slice` samples and the first partial of every record (none, and n = 0, for a record that does not run)
static int trk_call_slices(std::vector<gm::TrkBankRec>& recs, uint32_t slice, uint64_t& total, uint32_t& max_slices) {
    total = 0; max_slices = 0;
    for (auto& r : recs) {
        if (!r.run) r.n = 0;
        r.slices = r.run ? (r.n + slice - 1) / slice : 0;
        if (total + r.slices > 0xffffffffull) return set_err(GM_ERR_NOMEM, "the call's partial sums exceed 2^32 slices");
        r.poff = uint32_t(total);
        total += r.slices;
        if (r.slices > max_slices) max_slices = r.slices;
    }
    return GM_OK;
}
// the results land in host blocks of the call's own and reach the caller's only once everything has succeeded
static int trk_call_finish(gm_trk* t, const uint8_t* d_words, size_t n_words, const uint8_t* d_done, uint32_t R, gm_c32* out, uint8_t* done) {
    std::vector<gm_c32> h_out(n_words);
    std::vector<uint8_t> h_done(R);
    HIPC(hipMemcpyAsync(h_out.data(), d_words, n_words * 8, hipMemcpyDeviceToHost, t->stream));
    HIPC(hipMemcpyAsync(h_done.data(), d_done, R, hipMemcpyDeviceToHost, t->stream));
    HIPC(hipStreamSynchronize(t->stream));
    memcpy(out, h_out.data(), n_words * 8);
    if (done) memcpy(done, h_done.data(), R);
    return GM_OK;
}

// gm_trk_bank_plan's argument rules, shared by the device entries; F: the effective number of offsets
static int trk_bank_rules(float fs, bool custom_codes, uint32_t n_codes, uint32_t code_len, const gm_trk_bank_cfg* cfg, uint32_t n_states,
                          uint32_t& F) {
    if (int rc = trk_call_rules(cfg, "null bank cfg", fs, custom_codes, n_codes, code_len)) return rc;
    // the chip row shares the workgroup's 64 KB of LDS with the slice's samples and sign words (44 KB, trk_bank.hip)
    if (custom_codes && code_len > 16384) return set_err(GM_ERR_OUT_OF_RANGE, "the bank serves codes of at most 16384 chips");
    if (!cfg->taps_chips) return set_err(GM_ERR_INVALID_ARG, "null taps_chips");
    if (cfg->n_offsets && !cfg->offsets_hz) return set_err(GM_ERR_INVALID_ARG, "null offsets_hz with n_offsets > 0");
    F = cfg->n_offsets ? cfg->n_offsets : 1;
    if (cfg->n_taps < 1 || cfg->n_taps > uint32_t(gm::GM_TRK_BANK_MAX_TAPS)) return set_err(GM_ERR_OUT_OF_RANGE, "n_taps must be in 1 .. 64");
    if (F > uint32_t(gm::GM_TRK_BANK_MAX_OFFSETS)) return set_err(GM_ERR_OUT_OF_RANGE, "n_offsets must be at most 8");
    if (F * cfg->n_taps > uint32_t(gm::GM_TRK_BANK_MAX_WORDS)) return set_err(GM_ERR_OUT_OF_RANGE, "n_offsets * n_taps must be at most 256");
    if (n_states < 1 || n_states > uint32_t(gm::GM_TRK_BANK_MAX_STATES)) return set_err(GM_ERR_OUT_OF_RANGE, "n_states must be in 1 .. 1024");
    const float half_len = 0.5f * float(custom_codes ? code_len : 1023u);
    for (uint32_t k = 0; k < cfg->n_taps; ++k) {
        const float tau = cfg->taps_chips[k];
        if (!std::isfinite(tau)) return set_err(GM_ERR_INVALID_ARG, "a tap is not finite");
        if (fabsf(tau) > 64.0f || !(fabsf(tau) < half_len)) return set_err(GM_ERR_OUT_OF_RANGE, "|tap| must be at most 64 chips and below code_len / 2");
    }
    for (uint32_t k = 0; k < cfg->n_offsets; ++k) {
        const float df = cfg->offsets_hz[k];
        if (!std::isfinite(df)) return set_err(GM_ERR_INVALID_ARG, "a carrier offset is not finite");
        if (fabsf(df) > 0.5f * fs) return set_err(GM_ERR_OUT_OF_RANGE, "|offset| must be at most fs / 2");
    }
    return GM_OK;
}
// the launch and the copies of both forms: recs carry st, n and run; slices and partial offsets are filled in here
static int trk_bank_run(gm_trk* t, std::vector<gm::TrkBankRec>& recs, const gm_trk_bank_cfg* cfg, uint32_t F, const cf* base, uint64_t mask,
                        int linear, gm_c32* out, uint8_t* done) {
    const uint32_t R = uint32_t(recs.size()), T = cfg->n_taps;
    uint64_t total = 0;
    uint32_t max_slices = 0;
    if (int rc = trk_call_slices(recs, gm::GM_TRK_BANK_SLICE, total, max_slices)) return rc;
    std::vector<float> offs(F, 0.0f);
    for (uint32_t k = 0; k < cfg->n_offsets; ++k) offs[k] = cfg->offsets_hz[k];
    const size_t words = size_t(F) * T;
    Carve cv;
    const size_t o_recs = cv.take(R * sizeof(gm::TrkBankRec)), o_taps = cv.take(T * 4), o_offs = cv.take(F * 4), o_out = cv.take(R * words * 8),
                 o_done = cv.take(R), o_part = cv.take(size_t(total) * words * 8);
    if (int rc = t->bank.reserve(t->stream, cv.end, "gm_trk_bank: device block")) return rc;
    uint8_t* d = static_cast<uint8_t*>(t->bank.d);
    HIPC(hipMemcpyAsync(d + o_recs, recs.data(), R * sizeof(gm::TrkBankRec), hipMemcpyHostToDevice, t->stream));
    HIPC(hipMemcpyAsync(d + o_taps, cfg->taps_chips, T * 4, hipMemcpyHostToDevice, t->stream));
    HIPC(hipMemcpyAsync(d + o_offs, offs.data(), F * 4, hipMemcpyHostToDevice, t->stream));
    gm::TrkBankArgs a;
    a.recs = reinterpret_cast<const gm::TrkBankRec*>(d + o_recs);
    a.taps = reinterpret_cast<const float*>(d + o_taps); a.offs = reinterpret_cast<const float*>(d + o_offs);
    a.T = int(T); a.F = int(F);
    a.base = base; a.mask = mask; a.linear = linear;
    a.partials = reinterpret_cast<float*>(d + o_part);
    gm::launch_trk_bank(t->stream, t->dc, t->d_codes, a, int(R), max_slices, reinterpret_cast<gm_c32*>(d + o_out), d + o_done);
    HIPC(hipGetLastError());
    return trk_call_finish(t, d + o_out, size_t(R) * words, d + o_done, R, out, done);
}

// ---- gm_trk_array_prompts: per-antenna, per-tap prompts of an array stream at caller-supplied records (gnss_mi355x.h states the
// definition and the limits) -- gm_trk_array_plan's argument rules, shared by the device entry
static int trk_array_rules(float fs, bool custom_codes, uint32_t n_codes, uint32_t code_len, const gm_trk_array_cfg* cfg, uint32_t n_states) {
    if (int rc = trk_call_rules(cfg, "null array cfg", fs, custom_codes, n_codes, code_len)) return rc;
    for (uint32_t v : cfg->reserved)
        if (v) return set_err(GM_ERR_INVALID_ARG, "gm_trk_array_cfg.reserved must be 0");
    if (!std::isfinite(cfg->tap_chips)) return set_err(GM_ERR_INVALID_ARG, "tap_chips is not finite");
    // the chip row shares the workgroup's 64 KB of LDS with the slice's ref image (33 KB, trk_array.hip)
    if (custom_codes && code_len > 16384) return set_err(GM_ERR_OUT_OF_RANGE, "the array prompts serve codes of at most 16384 chips");
    if (cfg->n_antennas < uint32_t(gm::GM_TRK_ARRAY_MIN_ANTENNAS) || cfg->n_antennas > uint32_t(gm::GM_TRK_ARRAY_MAX_ANTENNAS))
        return set_err(GM_ERR_OUT_OF_RANGE, "n_antennas must be in 2 .. 8");
    if (cfg->taps < 1 || cfg->taps > uint32_t(gm::GM_TRK_ARRAY_MAX_TAPS)) return set_err(GM_ERR_OUT_OF_RANGE, "taps must be in 1 .. 8");
    if (cfg->n_antennas * cfg->taps > uint32_t(gm::GM_TRK_ARRAY_MAX_WORDS)) return set_err(GM_ERR_OUT_OF_RANGE, "n_antennas * taps must be at most 32");
    if (n_states < 1 || n_states > uint32_t(gm::GM_TRK_ARRAY_MAX_STATES)) return set_err(GM_ERR_OUT_OF_RANGE, "n_states must be in 1 .. 1024");
    const float half_len = 0.5f * float(custom_codes ? code_len : 1023u);
    if (fabsf(cfg->tap_chips) > 64.0f || !(fabsf(cfg->tap_chips) < half_len))
        return set_err(GM_ERR_OUT_OF_RANGE, "|tap_chips| must be at most 64 chips and below code_len / 2");
    return GM_OK;
}

// what the synchronous and the device entry share behind their own pointer checks: the handle's rules and the index rule
static int trk_array_call_rules(const gm_trk* t, uint64_t first_index, uint64_t n_time, const gm_trk_array_cfg* cfg, uint32_t n_states) {
    if (int rc = trk_array_rules(t->dc.fs, !t->dc.gps_ca, uint32_t(t->dc.n_codes), uint32_t(t->dc.code_len), cfg, n_states)) return rc;
    constexpr uint64_t INDEX_MAX = 1ull << 62;
    if (first_index >= INDEX_MAX || n_time >= INDEX_MAX || first_index + n_time >= INDEX_MAX)
        return set_err(GM_ERR_OUT_OF_RANGE, "first_index + n_time must be below 2^62");
    return GM_OK;
}
// before array work on `st`: the last array call of the handle, where it went to another stream, has run (stage_join's rule)
static int trk_array_join(gm_trk* t, hipStream_t st) {
    if (t->array_last && t->array_last != st) HIPC(hipStreamSynchronize(t->array_last));
    return GM_OK;
}
// which records run, their slices, and the block [records | z | done | partials] with room for them; the caller has joined `st`
struct TrkArrayCall { size_t o_recs = 0, o_z = 0, o_done = 0, o_part = 0; uint32_t max_slices = 0; };
static int trk_array_carve(gm_trk* t, hipStream_t st, std::vector<gm::TrkBankRec>& recs, uint64_t first_index, uint64_t n_time,
                           const gm_trk_array_cfg* cfg, TrkArrayCall& c) {
    const uint32_t R = uint32_t(recs.size()), M = cfg->n_antennas * cfg->taps;
    // the kernel reads the time samples [max(0, s - (L-1)), s + n) of a record that runs, and nothing else
    const uint64_t H = cfg->taps - 1;
    for (auto& r : recs) {
        const uint64_t start = r.st.next_sample_index;
        if (r.run && (start > H ? start - H : 0) < first_index) r.run = 0;                          // the halo is in front of the buffer
        if (r.run && !(start - first_index <= n_time && uint64_t(r.n) <= n_time - (start - first_index))) r.run = 0;   // s + n > first_index + n_time
    }
    uint64_t total = 0;
    if (int rc = trk_call_slices(recs, gm::GM_TRK_ARRAY_SLICE, total, c.max_slices)) return rc;    // (at most 1024 x 2^19 slices: never refused)
    Carve cv;
    c.o_recs = cv.take(R * sizeof(gm::TrkBankRec)); c.o_z = cv.take(size_t(R) * M * 8); c.o_done = cv.take(R);
    c.o_part = cv.take(size_t(total) * M * 8);
    return t->array.reserve(st, cv.end, "gm_trk_array_prompts: device block");
}
static void trk_array_launch(gm_trk* t, hipStream_t st, const void* d_samples, int fmt, uint64_t first_index, const gm_trk_array_cfg* cfg,
                             const TrkArrayCall& c, uint32_t R, gm_c32* d_z, uint8_t* d_done) {
    uint8_t* d = static_cast<uint8_t*>(t->array.d);
    gm::TrkArrayArgs a;
    a.recs = reinterpret_cast<const gm::TrkBankRec*>(d + c.o_recs);
    a.samples = d_samples; a.first_index = first_index;
    a.fmt = fmt; a.A = int(cfg->n_antennas); a.L = int(cfg->taps); a.tau = cfg->tap_chips;
    a.partials = reinterpret_cast<cf*>(d + c.o_part);
    gm::launch_trk_array(st, t->dc, t->d_codes, a, int(R), c.max_slices, d_z, d_done);
}

extern "C" {

int gm_trk_bank_plan(const gm_trk_cfg* trk, const gm_trk_bank_cfg* cfg, uint32_t n_states, gm_trk_bank_plan_out* out) {
    if (!trk) return set_err(GM_ERR_INVALID_ARG, "null tracking cfg");
    uint32_t F = 0;
    if (int rc = trk_bank_rules(trk->fs, trk->codes != nullptr, trk->n_codes, trk->code_len, cfg, n_states, F)) return rc;
    if (!out) return GM_OK;
    memset(out, 0, sizeof(*out));
    out->n_taps = cfg->n_taps; out->n_offsets = F;
    out->out_words = uint64_t(n_states) * F * cfg->n_taps;
    uint32_t n = 0;
    const bool ok = trk_bank_samples_per_code(trk->fs, trk->nominal_code_rate > 0 ? trk->nominal_code_rate : CA_RATE,
                                              trk->codes ? float(trk->code_len) : 1023.0f, n);
    out->samples = n;
    out->slices = ok ? (n + gm::GM_TRK_BANK_SLICE - 1) / gm::GM_TRK_BANK_SLICE : 0;
    out->tap_groups = (cfg->n_taps + 15) / 16;
    return GM_OK;
}

int gm_trk_bank(gm_trk* t, gm_ring* ring, const gm_trk_state* states, uint32_t n_states, const gm_trk_bank_cfg* cfg, gm_c32* out,
                uint8_t* done) {
    if (!t || !ring || !out) return set_err(GM_ERR_INVALID_ARG, "null handle, ring or out");
    if (t->device != ring->device) return set_err(GM_ERR_INVALID_ARG, "ring lives on another device");
    if (int rc = trk_call_states_rule(t, states, n_states)) return rc;
    uint32_t F = 0;
    if (int rc = trk_bank_rules(t->dc.fs, !t->dc.gps_ca, uint32_t(t->dc.n_codes), uint32_t(t->dc.code_len), cfg, n_states, F)) return rc;
    if (int rc = ensure_device(t->device)) return rc;
    std::vector<gm::TrkBankRec> recs;
    if (int rc = trk_call_records(t, states, n_states, recs)) return rc;
    ring_refresh_head(ring);
    const uint64_t head = ring->head.load(std::memory_order_acquire);      // the PUBLISHED head, as gm_trk_update_all reads it
    for (auto& r : recs) {
        const uint64_t start = r.st.next_sample_index;
        if (r.run && int64_t(head - (start + r.n)) < 0) r.run = 0;            // the tracker's gate (:170-172)
        if (r.run && head - start > uint64_t(ring->size)) r.run = 0;          // the epoch's first sample is no longer in the ring
    }
    return trk_bank_run(t, recs, cfg, F, ring->d_buf, ring->mask, 0, out, done);
}

int gm_trk_bank_samples(gm_trk* t, const gm_trk_state* state, const gm_c32* samples, size_t n, const gm_trk_bank_cfg* cfg, gm_c32* out) {
    if (!t || !state || !samples || !out) return set_err(GM_ERR_INVALID_ARG, "null handle, state, samples or out");
    uint32_t F = 0;
    if (int rc = trk_bank_rules(t->dc.fs, !t->dc.gps_ca, uint32_t(t->dc.n_codes), uint32_t(t->dc.code_len), cfg, 1, F)) return rc;
    if (n != state->num_samples_per_code || n == 0 || n >= (size_t(1) << 31))
        return set_err(GM_ERR_OUT_OF_RANGE, "n must equal num_samples_per_code (1 .. 2^31 - 1)");
    const int row = trk_bank_row(t, *state);
    if (row < 0 || row >= t->dc.n_codes) return set_err(GM_ERR_OUT_OF_RANGE, "code table row out of bounds");
    if (int rc = ensure_device(t->device)) return rc;
    if (n > t->scratch_cap) {
        HIPC(hipStreamSynchronize(t->stream));
        hipFree(t->d_scratch); t->d_scratch = nullptr; t->scratch_cap = 0;
        HIPC(hipMalloc(&t->d_scratch, n * 8 * 2));
        t->scratch_cap = n * 2;
    }
    HIPC(hipMemcpyAsync(t->d_scratch, samples, n * 8, hipMemcpyHostToDevice, t->stream));
    std::vector<gm::TrkBankRec> recs(1);
    recs[0].st = *state; recs[0].n = uint32_t(n); recs[0].run = 1; recs[0].slices = 0; recs[0].poff = 0;
    return trk_bank_run(t, recs, cfg, F, t->d_scratch, ~0ull, 1, out, nullptr);
}

int gm_trk_array_plan(const gm_trk_cfg* trk, const gm_trk_array_cfg* cfg, uint32_t n_states, gm_trk_array_plan_out* out) {
    if (!trk) return set_err(GM_ERR_INVALID_ARG, "null tracking cfg");
    if (int rc = trk_array_rules(trk->fs, trk->codes != nullptr, trk->n_codes, trk->code_len, cfg, n_states)) return rc;
    if (!out) return GM_OK;
    memset(out, 0, sizeof(*out));
    out->words_per_record = cfg->taps * cfg->n_antennas;
    out->out_words = uint64_t(n_states) * out->words_per_record;
    uint32_t n = 0;
    const bool ok = trk_bank_samples_per_code(trk->fs, trk->nominal_code_rate > 0 ? trk->nominal_code_rate : CA_RATE,
                                              trk->codes ? float(trk->code_len) : 1023.0f, n);
    out->samples = n;
    out->slices = ok ? (n + gm::GM_TRK_ARRAY_SLICE - 1) / gm::GM_TRK_ARRAY_SLICE : 0;
    return GM_OK;
}

int gm_trk_array_prompts(gm_trk* t, const void* d_samples, int fmt, uint64_t first_index, uint64_t n_time, const gm_trk_state* states,
                         uint32_t n_states, const gm_trk_array_cfg* cfg, gm_c32* z, uint8_t* done) {
    if (!t || !d_samples || !z) return set_err(GM_ERR_INVALID_ARG, "null handle, samples or z");
    if (fmt != GM_FMT_C32 && fmt != GM_FMT_I8_IQ) return set_err(GM_ERR_INVALID_ARG, "fmt must be GM_FMT_C32 or GM_FMT_I8_IQ");
    if (int rc = trk_call_states_rule(t, states, n_states)) return rc;
    if (int rc = trk_array_call_rules(t, first_index, n_time, cfg, n_states)) return rc;
    if (int rc = ensure_device(t->device)) return rc;
    if (int rc = trk_array_join(t, t->stream)) return rc;
    const uint32_t R = n_states, M = cfg->n_antennas * cfg->taps;
    std::vector<gm::TrkBankRec> recs;
    if (int rc = trk_call_records(t, states, n_states, recs)) return rc;
    TrkArrayCall c;
    if (int rc = trk_array_carve(t, t->stream, recs, first_index, n_time, cfg, c)) return rc;
    uint8_t* d = static_cast<uint8_t*>(t->array.d);
    HIPC(hipMemcpyAsync(d + c.o_recs, recs.data(), R * sizeof(gm::TrkBankRec), hipMemcpyHostToDevice, t->stream));
    trk_array_launch(t, t->stream, d_samples, fmt, first_index, cfg, c, R, reinterpret_cast<gm_c32*>(d + c.o_z), d + c.o_done);
    HIPC(hipGetLastError());
    t->array_last = t->stream;
    return trk_call_finish(t, d + c.o_z, size_t(R) * M, d + c.o_done, R, z, done);
}

// The persistent kernel's workgroups wait for one another, so its whole grid must be resident at once: ONE persistent
// launch per device at a time.  Launches of different handles (different streams) are chained through an event per device:
// each waits, on the GPU, for the previous persistent launch of that device and records the event behind itself — no host
// blocking, and two tracking managers can no longer strand half of each other's grids until the 0.2 s time-out.
namespace {
struct PersistChain { std::mutex mu; hipEvent_t ev = nullptr; bool armed = false; };
PersistChain g_persist_chain[16];
}

// `epochs` passes of process_channels on the handle's stream; the data gate of every pass (:170-172) uses `head`
static int trk_launch_all(gm_trk* t, gm_ring* ring, uint32_t epochs, uint64_t head) {
    if (int rc = trk_reserve_epochs(t, epochs)) return rc;
    if (t->dc.strict_sum_order) {
        // the reference's sequential sums: three launches per pass (products, one serial wave per channel, scalar epilogue)
        // instead of the persistent kernel; the data gate of every pass reads the head as of this call, like the persistent form
        const float nn = gm::trk_nominal_period(t->dc);
        if (int rc = trk_reserve_terms(t, (nn > 0 ? size_t(nn * 1.01f) : 0) + 64)) return rc;
        // the strict launches (256 threads, 40-48 KB of LDS each) must not take CU slots away from another handle's persistent
        // grid on this device either: same chain — wait for the previous launch of the device, record behind the last one
        PersistChain& schain = g_persist_chain[t->device & 15];
        std::lock_guard<std::mutex> schain_lock(schain.mu);
        if (!schain.ev) HIPC(hipEventCreateWithFlags(&schain.ev, hipEventDisableTiming));
        if (schain.armed) HIPC(hipStreamWaitEvent(t->stream, schain.ev, 0));
        if (t->timing) HIPC(hipEventRecord(t->ev0, t->stream));
        gm::TrkSrc src;
        src.base = ring->d_buf; src.mask = ring->mask; src.head = head; src.linear = 0; src.only_channel = -1;
        for (uint32_t e = 0; e < epochs; ++e) {
            const size_t o = size_t(e) * t->C;
            gm::launch_trk_epoch(t->stream, t->dc, t->d_codes, t->d_states, src, t->slices, t->d_partials, t->d_ready, gm::TRK_MODE_DO_WORK,
                                 t->d_outs + o, t->d_proc + o, t->d_lost + o, t->d_lostprn + o, t->d_terms, t->terms_cap, t->d_error);
        }
        if (t->timing) { HIPC(hipEventRecord(t->ev1, t->stream)); t->timed_launches = epochs; }
        HIPC(hipEventRecord(schain.ev, t->stream));
        schain.armed = true;
        HIPC(hipGetLastError());
        return GM_OK;
    }
    PersistChain& chain = g_persist_chain[t->device & 15];
    std::lock_guard<std::mutex> chain_lock(chain.mu);
    if (!chain.ev) HIPC(hipEventCreateWithFlags(&chain.ev, hipEventDisableTiming));
    if (chain.armed) HIPC(hipStreamWaitEvent(t->stream, chain.ev, 0));
    if (t->timing) HIPC(hipEventRecord(t->ev0, t->stream));
    // one persistent launch per <= 4095 epochs (the epoch index lives in the low 12 bits of the granule tag)
    for (uint32_t e0 = 0; e0 < epochs; e0 += 4095) {
        const uint32_t ne = epochs - e0 < 4095 ? epochs - e0 : 4095;
        const size_t o = size_t(e0) * t->C;
        t->launch_seq = (t->launch_seq + 1) & 0xfffffu;
        if (t->launch_seq == 0) t->launch_seq = 1;
        gm::TrkPersistCall c;
        c.codes = t->d_codes; c.states = t->d_states; c.ring = ring->d_buf; c.mask = ring->mask; c.head = head;
        c.epochs = int(ne); c.tag_base = t->launch_seq << 12; c.xchg = t->d_xchg;
        c.outs = t->d_outs + o; c.processed = t->d_proc + o; c.lost = t->d_lost + o; c.lost_prn = t->d_lostprn + o;
        c.error = t->d_error; c.error_dev = t->d_error_dev;
        c.stamps = (t->d_stamps && e0 == 0 && ne <= t->stamps_cap) ? t->d_stamps : nullptr; c.stamps_words = size_t(t->stamps_cap) * 48;
        gm::launch_trk_persistent(t->stream, t->dc, t->plan, c);
    }
    if (t->timing) { HIPC(hipEventRecord(t->ev1, t->stream)); t->timed_launches = epochs; }
    HIPC(hipEventRecord(chain.ev, t->stream));
    chain.armed = true;
    HIPC(hipGetLastError());
    return GM_OK;
}

int gm_trk_update_all_dev(gm_trk* t, gm_ring* ring, uint32_t epochs) {
    if (!t || !ring || !epochs) return set_err(GM_ERR_INVALID_ARG, "bad argument");
    if (t->device != ring->device) return set_err(GM_ERR_INVALID_ARG, "ring lives on another device");
    if (int rc = ensure_device(t->device)) return rc;
    ring_refresh_head(ring);
    return trk_launch_all(t, ring, epochs, ring->head.load(std::memory_order_acquire));      // the PUBLISHED head: the samples are in HBM
}

// the pinned result slots of gm_trk_update_all_async: one block, at least `bytes` per slot (grown only while no ticket is in flight)
static int trk_reserve_tickets(gm_trk* t, size_t bytes) {
    if (bytes <= t->tk_cap) return GM_OK;
    for (const auto& k : t->tk)
        if (k.in_flight) return set_err(GM_ERR_OUT_OF_RANGE, "a larger max_epochs than the result slots hold: collect the tickets in flight first");
    if (t->tk_block) { hipHostFree(t->tk_block); t->tk_block = nullptr; t->tk_cap = 0; }
    const size_t per = round256(bytes);
    HIPC(hipHostMalloc(reinterpret_cast<void**>(&t->tk_block), per * gm_trk::TICKETS, hipHostMallocDefault));
    t->tk_cap = per;
    for (int i = 0; i < gm_trk::TICKETS; ++i) {
        t->tk[i].h = t->tk_block + size_t(i) * per;
        if (!t->tk[i].done) HIPC(hipEventCreateWithFlags(&t->tk[i].done, hipEventDisableTiming));
    }
    return GM_OK;
}

static uint32_t trk_epochs_done(const uint8_t* proc, uint32_t max_epochs, uint32_t C) {
    uint32_t done = 0;
    for (uint32_t e = 0; e < max_epochs; ++e) {
        bool any = false;
        for (uint32_t c = 0; c < C; ++c) any |= proc[size_t(e) * C + c] != 0;
        if (any) done = e + 1;
    }
    return done;
}

// The same passes without a host wait: ordered on the DEVICE behind whatever the ring's writer has enqueued so far
// — an event on the ring's copy stream, the counterpart of the Condvar wait at do_tracking.rs:392-406 — with the data gate on that
// enqueued head; results into a pinned slot, handed over by gm_trk_collect.
int gm_trk_update_all_async(gm_trk* t, gm_ring* ring, uint32_t max_epochs, uint64_t* ticket) {
    if (!t || !ring || !max_epochs || !ticket) return set_err(GM_ERR_INVALID_ARG, "bad argument");
    if (t->device != ring->device) return set_err(GM_ERR_INVALID_ARG, "ring lives on another device");
    *ticket = 0;
    gm_trk::Ticket& k = t->tk[t->next_ticket % gm_trk::TICKETS];
    if (k.in_flight) return set_err(GM_ERR_OUT_OF_RANGE, "all result slots are in flight: gm_trk_collect the oldest ticket first");
    if (int rc = ensure_device(t->device)) return rc;
    // slot: [outs n | processed n | lost n | pad to 8 | states C] — the states as they stand behind THIS call's passes
    const size_t n = size_t(max_epochs) * t->C, bytes = n * (sizeof(gm_trk_out) + 2);
    const size_t st_off = (bytes + 7) & ~size_t(7), st_bytes = size_t(t->C) * sizeof(gm_trk_state);
    if (int rc = trk_reserve_tickets(t, st_off + st_bytes)) return rc;
    static const int trace_slow = gm::diag_int("GM_TRK_TRACE_SLOW", 0);      // diagnostic: which runtime call of this entry takes milliseconds
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return (long)std::chrono::duration_cast<std::chrono::microseconds>(b - a).count(); };
    const auto t0 = now();
    ring_refresh_head(ring);
    const auto t1 = now();
    uint64_t head = ring->head.load(std::memory_order_acquire);
    {
        std::lock_guard<std::mutex> g(ring->enq_mu);
        if (ring->ev_enq_armed) {
            HIPC(hipStreamWaitEvent(t->stream, ring->ev_enq, 0));
            if (int64_t(ring->enqueued - head) > 0) head = ring->enqueued;
        }
    }
    const auto t2 = now();
    if (int rc = trk_launch_all(t, ring, max_epochs, head)) return rc;
    const auto t3 = now();
    gm::launch_trk_results_to_host(t->stream, t->d_res, k.h, bytes, t->d_states, k.h + st_off, st_bytes);   // -> the pinned slot (trk_kernels.hip)
    const auto t4 = now();
    HIPC(hipEventRecord(k.done, t->stream));
    const auto t5 = now();
    if (trace_slow && us(t0, t5) > 1000)
        fprintf(stderr, "gm_trk_update_all_async slow: refresh %ld us, wait-event %ld, launch %ld, copy %ld, record %ld\n", us(t0, t1), us(t1, t2), us(t2, t3), us(t3, t4), us(t4, t5));
    k.in_flight = true; k.epochs = max_epochs; k.id = *ticket = t->next_ticket++;
    return GM_OK;
}

int gm_trk_collect(gm_trk* t, uint64_t ticket, int wait, gm_trk_out* outs, uint8_t* processed, uint8_t* lost, gm_trk_state* states,
                   uint32_t* epochs_done, int* ready) {
    if (!t || !ticket || !ready) return set_err(GM_ERR_INVALID_ARG, "bad argument");
    gm_trk::Ticket& k = t->tk[ticket % gm_trk::TICKETS];
    if (!k.in_flight || k.id != ticket) return set_err(GM_ERR_INVALID_ARG, "no such ticket (collected already, or never issued)");
    if (int rc = ensure_device(t->device)) return rc;
    *ready = 0;
    // contract (include/gnss_mi355x.h): a collect that returns an ERROR has consumed the ticket — the slot is released on hard HIP
    // errors too, or it would be lost for good and every TICKETS-th asynchronous call refused from then on
    if (wait) {
        const hipError_t w = wait_event_polling(k.done);
        if (w != hipSuccess) { k.in_flight = false; return hip_fail(w, "wait(ticket)"); }
    } else {
        const hipError_t q = hipEventQuery(k.done);
        if (q == hipErrorNotReady) { (void)hipGetLastError(); return GM_OK; }
        if (q != hipSuccess) { k.in_flight = false; return hip_fail(q, "hipEventQuery(ticket)"); }
    }
    k.in_flight = false;
    if (int rc = trk_check_error(t)) return rc;
    const size_t n = size_t(k.epochs) * t->C;
    if (outs) memcpy(outs, k.h, n * sizeof(gm_trk_out));
    if (processed) memcpy(processed, k.h + n * sizeof(gm_trk_out), n);
    if (lost) memcpy(lost, k.h + n * sizeof(gm_trk_out) + n, n);
    if (states) memcpy(states, k.h + ((n * (sizeof(gm_trk_out) + 2) + 7) & ~size_t(7)), size_t(t->C) * sizeof(gm_trk_state));
    if (epochs_done) *epochs_done = trk_epochs_done(k.h + n * sizeof(gm_trk_out), k.epochs, t->C);
    *ready = 1;
    return GM_OK;
}

int gm_trk_update_all(gm_trk* t, gm_ring* ring, uint32_t max_epochs, gm_trk_out* outs, uint8_t* processed, uint8_t* lost,
                      uint32_t* epochs_done) {
    if (int rc = gm_trk_update_all_dev(t, ring, max_epochs)) return rc;
    // the three result arrays land in one pinned area behind the launch, on its stream: one synchronisation per call
    // (three blocking hipMemcpy calls from pageable memory cost more than the 16 epochs of a 16 ms block)
    const size_t n = size_t(max_epochs) * t->C;
    uint8_t* h_outs = t->h_res;
    uint8_t* h_proc = h_outs + n * sizeof(gm_trk_out);
    uint8_t* h_lost = h_proc + n;
    if (outs) HIPC(hipMemcpyAsync(h_outs, t->d_res, n * (sizeof(gm_trk_out) + 2), hipMemcpyDeviceToHost, t->stream));      // [outs | processed | lost]: one copy
    else HIPC(hipMemcpyAsync(h_proc, t->d_proc, 2 * n, hipMemcpyDeviceToHost, t->stream));
    HIPC(hipStreamSynchronize(t->stream));
    if (int rc = trk_check_error(t)) return rc;
    const uint8_t* proc = h_proc;
    if (outs) memcpy(outs, h_outs, n * sizeof(gm_trk_out));
    if (processed) memcpy(processed, h_proc, n);
    if (lost) memcpy(lost, h_lost, n);
    if (epochs_done) *epochs_done = trk_epochs_done(proc, max_epochs, t->C);
    return GM_OK;
}

// ---- tracking on planes: channel c on plane planes[c] of a gm_plane_ring (gnss_mi355x.h states the contract) -------------------------
// gm_trk_planes_plan's argument rules, shared by the device entries; planes NULL: every channel on plane 0
static int trk_planes_rules(float fs, uint32_t n_channels, bool custom_codes, uint32_t n_codes, uint32_t code_len, bool strict_sum_order,
                            uint32_t n_planes, const uint32_t* planes, uint32_t max_epochs) {
    if (!(fs > 0) || !std::isfinite(fs) || !n_channels) return set_err(GM_ERR_INVALID_ARG, "fs and n_channels are required");
    if (custom_codes && (!n_codes || !code_len)) return set_err(GM_ERR_INVALID_ARG, "n_codes/code_len required");
    if (strict_sum_order)
        return set_err(GM_ERR_INVALID_ARG, "tracking on planes: the sequential-sum path (strict_sum_order) is not built on planes; the switch is not ignored");
    if (!max_epochs) return set_err(GM_ERR_INVALID_ARG, "max_epochs must be at least 1");
    if (max_epochs > 4095) return set_err(GM_ERR_OUT_OF_RANGE, "max_epochs must be at most 4095");
    if (n_planes < 1 || n_planes > PLANE_RING_MAX_PLANES) return set_err(GM_ERR_OUT_OF_RANGE, "n_planes must be in 1 .. 64");
    // the chip row sits in the workgroup's LDS as int8, beside the kernel's own few hundred bytes
    if (custom_codes && code_len > 16384) return set_err(GM_ERR_OUT_OF_RANGE, "tracking on planes serves codes of at most 16384 chips");
    for (uint32_t c = 0; planes && c < n_channels; ++c)
        if (planes[c] >= n_planes) {
            char msg[128];
            snprintf(msg, sizeof(msg), "channel %u is mapped to plane %u, the ring has %u planes", c, planes[c], n_planes);
            return set_err(GM_ERR_OUT_OF_RANGE, msg);
        }
    return GM_OK;
}
// the map's device and staging blocks, made at the first entry that needs them (a new handle's map: every channel on plane 0)
static int trk_planes_ensure(gm_trk* t) {
    if (t->d_planes) return GM_OK;
    uint32_t* d = nullptr;
    HIPC(hipMalloc(&d, size_t(t->C) * 4));
    hipError_t e = hipMemsetAsync(d, 0, size_t(t->C) * 4, t->stream);
    if (e == hipSuccess && !t->planes_stage) e = hipHostMalloc(reinterpret_cast<void**>(&t->planes_stage), size_t(t->C) * 4, hipHostMallocDefault);
    if (e == hipSuccess && !t->planes_ev) e = hipEventCreateWithFlags(&t->planes_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(t->planes_ev, t->stream);
    if (e != hipSuccess) { hipStreamSynchronize(t->stream); hipFree(d); return hip_fail(e, "gm_trk: the plane map's blocks"); }
    t->d_planes = d;
    t->h_planes.assign(t->C, 0u);
    return GM_OK;
}
// every refusal of the device entries, before anything runs
static int trk_planes_call_rules(gm_trk* t, gm_plane_ring* pr, uint32_t max_epochs) {
    if (!t || !pr) return set_err(GM_ERR_INVALID_ARG, "null handle or plane ring");
    if (t->device != pr->device) return set_err(GM_ERR_INVALID_ARG, "plane ring lives on another device");
    return trk_planes_rules(t->dc.fs, t->C, !t->dc.gps_ca, uint32_t(t->dc.n_codes), uint32_t(t->dc.code_len), t->dc.strict_sum_order != 0, pr->P,
                            t->h_planes.empty() ? nullptr : t->h_planes.data(), max_epochs);
}
// `epochs` passes on the handle's stream, behind the ring's enqueued writes and the device's previous tracking launch
static int trk_launch_planes(gm_trk* t, gm_plane_ring* pr, uint32_t epochs) {
    if (int rc = ensure_device(t->device)) return rc;
    if (int rc = trk_planes_ensure(t)) return rc;
    if (int rc = trk_reserve_epochs(t, epochs)) return rc;
    std::lock_guard<std::mutex> ring_lock(pr->mu);
    uint64_t head = 0;
    if (int rc = plane_ring_begin_read(pr, t->stream, &head)) return rc;
    // a workgroup of this kernel holding a CU slot while another handle's persistent grid starts is the stall the chain prevents:
    // same chain as the strict path of trk_launch_all — wait for the device's previous tracking launch, record behind this one
    PersistChain& chain = g_persist_chain[t->device & 15];
    std::lock_guard<std::mutex> chain_lock(chain.mu);
    if (!chain.ev) HIPC(hipEventCreateWithFlags(&chain.ev, hipEventDisableTiming));
    if (chain.armed) HIPC(hipStreamWaitEvent(t->stream, chain.ev, 0));
    if (t->timing) HIPC(hipEventRecord(t->ev0, t->stream));
    gm::TrkPlanesArgs a;
    a.cfg = t->dc; a.codes = t->d_codes; a.states = t->d_states; a.map = t->d_planes;
    a.ring = pr->d_buf; a.plane_size = pr->size; a.mask = pr->mask; a.head = head; a.n_planes = pr->P; a.epochs = int(epochs);
    a.outs = t->d_outs; a.processed = t->d_proc; a.lost = t->d_lost; a.lost_prn = t->d_lostprn;
    gm::launch_trk_planes(t->stream, a);
    if (t->timing) { HIPC(hipEventRecord(t->ev1, t->stream)); t->timed_launches = epochs; }
    HIPC(hipEventRecord(chain.ev, t->stream));
    chain.armed = true;
    HIPC(hipGetLastError());
    return plane_ring_end_read(pr, t->stream);
}

int gm_trk_planes_plan(const gm_trk_cfg* trk, uint32_t n_planes, const uint32_t* planes, uint32_t max_epochs, gm_trk_planes_plan_out* out) {
    if (!trk) return set_err(GM_ERR_INVALID_ARG, "null tracking cfg");
    if (int rc = trk_planes_rules(trk->fs, trk->n_channels, trk->codes != nullptr, trk->n_codes, trk->code_len, trk->strict_sum_order != 0,
                                  n_planes, planes, max_epochs))
        return rc;
    if (!out) return GM_OK;
    memset(out, 0, sizeof(*out));
    out->workgroups = trk->n_channels; out->threads = 256;
    out->chip_row_bytes = trk->codes ? trk->code_len : 1023u;
    uint64_t used = 0;
    for (uint32_t c = 0; c < trk->n_channels; ++c) used |= 1ull << (planes ? planes[c] : 0u);
    out->planes_used = uint32_t(__builtin_popcountll(used));
    uint32_t n = 0;
    const bool ok = trk_bank_samples_per_code(trk->fs, trk->nominal_code_rate > 0 ? trk->nominal_code_rate : CA_RATE,
                                              trk->codes ? float(trk->code_len) : 1023.0f, n);
    out->samples = n;
    out->samples_per_lane = ok ? (n + 255u) / 256u : 0;
    out->result_bytes = (uint64_t(max_epochs) * trk->n_channels * (sizeof(gm_trk_out) + 3) + 3) & ~uint64_t(3);
    return GM_OK;
}

int gm_trk_set_channel_planes(gm_trk* t, const uint32_t* planes) {
    if (!t) return set_err(GM_ERR_INVALID_ARG, "null handle");
    for (uint32_t c = 0; planes && c < t->C; ++c)
        if (planes[c] >= PLANE_RING_MAX_PLANES) return set_err(GM_ERR_OUT_OF_RANGE, "a plane index above 63: no plane ring has such a plane");
    if (int rc = ensure_device(t->device)) return rc;
    if (int rc = trk_planes_ensure(t)) return rc;
    HIPC(hipEventSynchronize(t->planes_ev));                 // the previous install has read the staging words
    for (uint32_t c = 0; c < t->C; ++c) t->planes_stage[c] = planes ? planes[c] : 0u;
    HIPC(hipMemcpyAsync(t->d_planes, t->planes_stage, size_t(t->C) * 4, hipMemcpyHostToDevice, t->stream));      // stream-ordered: behind the launches enqueued so far
    HIPC(hipEventRecord(t->planes_ev, t->stream));
    t->h_planes.assign(t->planes_stage, t->planes_stage + t->C);
    return GM_OK;
}

int gm_trk_get_channel_planes(gm_trk* t, uint32_t* planes) {
    if (!t || !planes) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    for (uint32_t c = 0; c < t->C; ++c) planes[c] = t->h_planes.empty() ? 0u : t->h_planes[c];
    return GM_OK;
}

int gm_trk_update_planes_dev(gm_trk* t, gm_plane_ring* pr, uint32_t epochs) {
    if (int rc = trk_planes_call_rules(t, pr, epochs)) return rc;
    return trk_launch_planes(t, pr, epochs);
}

int gm_trk_update_planes(gm_trk* t, gm_plane_ring* pr, uint32_t max_epochs, gm_trk_out* outs, uint8_t* processed, uint8_t* lost,
                         uint32_t* epochs_done) {
    if (int rc = trk_planes_call_rules(t, pr, max_epochs)) return rc;
    if (int rc = trk_launch_planes(t, pr, max_epochs)) return rc;
    // gm_trk_update_all's hand-over: [outs | processed | lost] into the pinned area in one copy behind the launch, one synchronisation
    const size_t n = size_t(max_epochs) * t->C;
    uint8_t* h_outs = t->h_res;
    uint8_t* h_proc = h_outs + n * sizeof(gm_trk_out);
    uint8_t* h_lost = h_proc + n;
    if (outs) HIPC(hipMemcpyAsync(h_outs, t->d_res, n * (sizeof(gm_trk_out) + 2), hipMemcpyDeviceToHost, t->stream));
    else HIPC(hipMemcpyAsync(h_proc, t->d_proc, 2 * n, hipMemcpyDeviceToHost, t->stream));
    HIPC(hipStreamSynchronize(t->stream));
    if (outs) memcpy(outs, h_outs, n * sizeof(gm_trk_out));
    if (processed) memcpy(processed, h_proc, n);
    if (lost) memcpy(lost, h_lost, n);
    if (epochs_done) *epochs_done = trk_epochs_done(h_proc, max_epochs, t->C);
    return GM_OK;
}

static int trk_check_error(gm_trk* t) {
    const int err = *static_cast<volatile int*>(t->d_error);      // the stream has been synchronised by the caller
    if (err) {
        *t->d_error = 0;
        (void)hipMemsetAsync(t->d_error_dev, 0, sizeof(int), t->stream);
        (void)hipStreamSynchronize(t->stream);
        if (err == 2) return set_err(GM_ERR_OUT_OF_RANGE, "tracking (strict_sum_order): a code period longer than the product streams were sized for (nominal + 1 %)");
        return set_err(GM_ERR_HIP, "tracking: inter-workgroup exchange timed out (workgroups of a channel not co-resident?)");
    }
    return GM_OK;
}

int gm_trk_synchronize(gm_trk* t) {
    if (!t) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (int rc = ensure_device(t->device)) return rc;
    HIPC(hipStreamSynchronize(t->stream));
    return trk_check_error(t);
}

// Diagnostic: s_memtime stamps of workgroup 0 at 8 phase boundaries of each epoch of the next launches
// (epochs <= cap).  out = [cap][8] after gm_trk_synchronize.  Not part of the reference API.
int gm_trk_debug_stamps(gm_trk* t, uint32_t cap, long long* out) {
    if (!t) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (int rc = ensure_device(t->device)) return rc;
    if (!out) {   // arm
        hipFree(t->d_stamps); t->d_stamps = nullptr; t->stamps_cap = 0;
        if (cap) { HIPC(hipMalloc(&t->d_stamps, size_t(cap) * 48 * sizeof(long long))); HIPC(hipMemset(t->d_stamps, 0, size_t(cap) * 384)); HIPC(hipStreamSynchronize(nullptr)); t->stamps_cap = cap; }
        return GM_OK;
    }
    if (!t->d_stamps || cap > t->stamps_cap) return set_err(GM_ERR_INVALID_ARG, "stamps not armed");
    HIPC(hipStreamSynchronize(t->stream));
    HIPC(hipMemcpy(out, t->d_stamps, size_t(cap) * 384, hipMemcpyDeviceToHost));
    return GM_OK;
}

int gm_trk_enable_timing(gm_trk* t, int on) {
    if (!t) return set_err(GM_ERR_INVALID_ARG, "null handle");
    t->timing = on != 0;
    return GM_OK;
}

int gm_trk_last_timing(gm_trk* t, float* ms_total, uint32_t* launches) {
    if (!t || !t->timing) return set_err(GM_ERR_INVALID_ARG, "timing not enabled");
    if (int rc = ensure_device(t->device)) return rc;
    HIPC(hipStreamSynchronize(t->stream));
    float ms = 0;
    HIPC(hipEventElapsedTime(&ms, t->ev0, t->ev1));
    if (ms_total) *ms_total = ms;
    if (launches) *launches = t->timed_launches;
    return GM_OK;
}

// Diagnostic: the tracking loop's scalar device math on caller-supplied arguments (trk_debug_math_kernel; ops in gnss_mi355x.h).
// Host buffers, synchronous: H2D, one kernel on the NULL stream, D2H.  Not part of the reference API.
int gm_debug_math(int op, const float* x, size_t n, float p0, float p1, float p2, uint32_t* out0, uint32_t* out1) {
    if (!x || !out0 || !out1) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (op < 0 || op > 10) return set_err(GM_ERR_OUT_OF_RANGE, "op must be 0..10");
    if (n > (size_t(1) << 24)) return set_err(GM_ERR_OUT_OF_RANGE, "n must be at most 2^24");
    (void)p2;                                              // reserved: no op reads a third parameter
    const bool two = op == 7 || op == 8;                   // p0 = fs, p1 = len
    const bool one = op == 4 || op == 5 || op == 9 || op == 10 || two;
    if (one && !(p0 > 0.0f && p0 < 3.0e38f)) return set_err(GM_ERR_OUT_OF_RANGE, "p0 (divisor / fs / len) must be positive and finite");
    if (two && !(p1 > 0.0f && p1 < 3.0e38f)) return set_err(GM_ERR_OUT_OF_RANGE, "p1 (len) must be positive and finite");
    if (op == 10 && !(p0 >= 1.0f && p0 <= 16777216.0f && p0 == float(int(p0)))) return set_err(GM_ERR_OUT_OF_RANGE, "len must be an integer in 1..2^24");
    if (int rc = ensure_device(g_device)) return rc;
    if (!n) return GM_OK;
    const float inv = op == 7 ? 1.0f / p1 : (one ? 1.0f / p0 : 0.0f);      // RN(1 / divisor), as fill_trk_derived forms it
    float* dx = nullptr;
    uint32_t* dout = nullptr;
    HIPC(hipMalloc(&dx, n * 4));
    hipError_t e = hipMalloc(&dout, n * 8);
    if (e == hipSuccess) e = hipMemcpy(dx, x, n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        gm::launch_trk_debug_math(nullptr, op, dx, uint32_t(n), p0, p1, inv, dout, dout + n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out0, dout, n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out1, dout + n, n * 4, hipMemcpyDeviceToHost);
    hipFree(dx); hipFree(dout);
    if (e != hipSuccess) return hip_fail(e, "gm_debug_math");
    return GM_OK;
}

}  // extern "C"

// ====================================================================== digital front-end
struct gm_frontend {
    int device = -1;
    float f_if = 0, fs_in = 0, fs_out = 0, phase_step = 0, alpha = 0.001f, con = 0;
    std::vector<float> lut;                 // [2][2048]
    float* d_lut = nullptr;
    gm::FeState* d_state = nullptr;
    hipStream_t stream = nullptr;
    void* d_io = nullptr;                   // scratch for the host-buffer entry
    size_t io_cap = 0;
    void* d_raw[gm_ring::SLOTS] = {nullptr, nullptr, nullptr, nullptr};   // raw-format landing zones of the ring writer
    gm::FrontendArgs::Stream* d_batch = nullptr;   // stream descriptors of gm_frontend_process_dev_batch
    uint32_t batch_cap = 0;
    // tabulated NCO phase orbit (fe_kernels.hip, fast form): built on first use
    bool tab_tried = false, on_orbit = true;       // on_orbit: the device phase_accumulator is entry `pos` of the orbit from 0
    std::vector<float> tab;                        // |phase| / 2048 before step k, k < mu + lambda'
    float* d_tab = nullptr;
    uint32_t tab_mu = 0, tab_lambda = 0;           // lambda' = the period repeated until >= FE_FAST_SEG
    uint32_t pos = 0;                              // table index of the next sample
    float* d_spec = nullptr;                       // [FE_SPEC_K][32] + 1 floats: the speculative form's run records (fe_kernels.hip)
    uint32_t forms[3] = {0, 0, 0};                 // launches on behalf of this handle: sequential, table, speculative (gm_frontend_debug_forms)
};
static constexpr int FE_SPEC_K = gm::FE_SPEC_K_MAX;
static constexpr size_t FE_SPEC_MIN = size_t(gm::FE_FAST_SEG) * 48;     // blocks shorter than 48 pipeline segments stay on one workgroup

// r -> fract(fl(r + s)): the fast form of `(phase + step) % 2048` in revolutions (fe_kernels.hip nco_segment_fast)
static inline float fe_orbit_step(float r, float s) { const float t = r + s; return t - floorf(t); }

// The orbit of the NCO phase from 0: transient mu and period lambda by Brent's algorithm, then the table.  Only for the
// settings the sequential kernel's fast form covers (|step| < 2048, not denormal-small); false otherwise or when the
// orbit is longer than 2^24 + 2^16 steps (never seen: periods are <= 2^23).
static bool frontend_build_table(gm_frontend* f) {
    if (f->tab_tried) return !f->tab.empty();
    f->tab_tried = true;
    const float step = f->phase_step;
    if (!(fabsf(step) < 2048.0f) || !(step == 0.0f || fabsf(step) > 1.0e-20f)) return false;
    const float s = fabsf(step) * (1.0f / 2048.0f);
    const uint64_t cap = (1ull << 24) + (1ull << 16);
    uint64_t power = 1, lam = 1;
    float tort = 0.0f, hare = fe_orbit_step(0.0f, s);
    while (tort != hare) {
        if (power == lam) { tort = hare; power *= 2; lam = 0; }
        hare = fe_orbit_step(hare, s);
        if (++lam > cap) return false;
    }
    uint64_t mu = 0;
    tort = hare = 0.0f;
    for (uint64_t i = 0; i < lam; ++i) hare = fe_orbit_step(hare, s);
    while (tort != hare) { tort = fe_orbit_step(tort, s); hare = fe_orbit_step(hare, s); if (++mu > cap) return false; }
    const uint64_t reps = (uint64_t(gm::FE_FAST_SEG) + lam - 1) / lam;
    const uint64_t lam2 = lam * reps;
    if (mu + lam2 > cap) return false;
    f->tab.resize(size_t(mu + lam2));
    float r = 0.0f;
    for (size_t k = 0; k < f->tab.size(); ++k) { f->tab[k] = r; r = fe_orbit_step(r, s); }
    if (hipMalloc(&f->d_tab, f->tab.size() * sizeof(float)) != hipSuccess ||
        hipMemcpy(f->d_tab, f->tab.data(), f->tab.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(f->d_tab); f->d_tab = nullptr; f->tab.clear();
        return false;
    }
    f->tab_mu = uint32_t(mu); f->tab_lambda = uint32_t(lam2);
    return true;
}
static inline uint32_t frontend_fold(const gm_frontend* f, uint64_t p) {
    const uint64_t len = uint64_t(f->tab_mu) + f->tab_lambda;
    return uint32_t(p < len ? p : f->tab_mu + (p - f->tab_mu) % f->tab_lambda);
}

static gm::FrontendArgs::Stream frontend_stream(gm_frontend* f, const void* d_in, void* d_out, uint64_t out_start,
                                                 uint64_t out_mask, size_t n) {
    gm::FrontendArgs::Stream s{};
    s.in = d_in; s.out = d_out; s.out_start = out_start; s.out_mask = out_mask; s.n_samples = n; s.state = f->d_state;
    s.phase_step = f->phase_step;
    s.fast_fmod = fabsf(f->phase_step) < 2048.0f ? 1 : 0;     // false for NaN too
    s.ph_table = nullptr;
    if (f->on_orbit && frontend_build_table(f)) {             // fast form: phases looked up, position tracked on the host
        const size_t n8 = n & ~size_t(7);
        s.ph_table = f->d_tab;
        s.tab_len = f->tab_mu + f->tab_lambda; s.tab_lambda = f->tab_lambda;
        s.tab_pos = f->pos;
        s.tab_pos_end = frontend_fold(f, uint64_t(f->pos) + n8);
        s.tab_scale = f->phase_step < 0.0f ? -2048.0f : 2048.0f;
        f->pos = s.tab_pos_end;
    }
    return s;
}

static int frontend_launch(gm_frontend* f, hipStream_t st, const void* d_in, int fmt, void* d_out, uint64_t out_start,
                           uint64_t out_mask, size_t n) {
    gm::FrontendArgs a{};
    a.streams = nullptr;
    a.one = frontend_stream(f, d_in, d_out, out_start, out_mask, n);
    a.lut = f->d_lut; a.alpha = f->alpha; a.con = f->con;
    // the speculative form: a long block whose output does not alias its input (the runs' warm-ups re-read earlier samples)
    const int spec = gm::diag_int("GM_FE_SPEC", 1);
    if (a.one.ph_table && spec != 0 && n >= FE_SPEC_MIN && d_in != d_out) {
        if (!f->d_spec) {
            HIPC(hipMalloc(&f->d_spec, (size_t(FE_SPEC_K) * 32 + 1) * sizeof(float)));
            HIPC(hipMemsetAsync(f->d_spec, 0, (size_t(FE_SPEC_K) * 32 + 1) * sizeof(float), st));
        }
        {
            const int k = gm::diag_int("GM_FE_SPEC_K", 32);      // 32 runs: 126 -> 113 us per 2^19-sample block against 16 (48, 64: 107 us, more runs to repair; DESIGN_HISTORY R6.5)
            a.spec_k = k < 2 ? 2 : (k > FE_SPEC_K ? FE_SPEC_K : k);
            a.spec_warm = gm::diag_int("GM_FE_SPEC_WARM", 0);
        }
        a.spec_buf = f->d_spec; a.spec_poison = spec == 2 ? 1 : 0;
        a.spec_repairs = reinterpret_cast<unsigned int*>(f->d_spec + size_t(FE_SPEC_K) * 32);
        gm::launch_frontend_spec(st, a, fmt);
        ++f->forms[2];
    } else if (a.one.ph_table) { gm::launch_frontend_fast(st, a, 1, fmt); ++f->forms[1]; }
    else { gm::launch_frontend(st, a, 1, fmt); ++f->forms[0]; }
    HIPC(hipGetLastError());
    return GM_OK;
}

extern "C" {

int gm_frontend_create(float f_if, float fs_in, float fs_out, gm_frontend** out) {   // DigitalFrontend::new frontend.rs:19-30
    if (!out) return set_err(GM_ERR_INVALID_ARG, "null out");
    *out = nullptr;
    if (int rc = ensure_device(g_device)) return rc;
    gm_frontend* f = new gm_frontend;
    f->device = g_device; f->f_if = f_if; f->fs_in = fs_in; f->fs_out = fs_out;
    f->lut.resize(2 * 2048);
    for (int i = 0; i < 2048; ++i) {                          // NcoLut::new nco_lut.rs:28-32
        const float angle = ((2.0f * PI_F) * float(i)) / 2048.0f;
        f->lut[i] = cosf(angle);
        f->lut[2048 + i] = -sinf(angle);
    }
    f->phase_step = (f_if / fs_in) * 2048.0f;                 // :34
    f->alpha = 0.001f;                                        // DcRemoverSimd::new(0.001), frontend.rs:21
    f->con = 1.0f - f->alpha;                                 // dc_remove.rs:12
    hipError_t e = hipMalloc(&f->d_lut, 2 * 2048 * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(f->d_lut, f->lut.data(), 2 * 2048 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&f->d_state, sizeof(gm::FeState));
    if (e == hipSuccess) e = hipMemset(f->d_state, 0, sizeof(gm::FeState));
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);    // the fill has run before a kernel on a non-blocking stream can touch the state (see gm_ring_create)
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { gm_frontend_destroy(f); return hip_fail(e, "gm_frontend_create"); }
    *out = f;
    return GM_OK;
}

int gm_frontend_destroy(gm_frontend* f) {
    if (!f) return GM_OK;
    hipSetDevice(f->device);
    if (f->stream) { hipStreamSynchronize(f->stream); hipStreamDestroy(f->stream); }
    hipFree(f->d_lut); hipFree(f->d_state); hipFree(f->d_io); hipFree(f->d_batch); hipFree(f->d_tab); hipFree(f->d_spec);
    for (void* p : f->d_raw) hipFree(p);
    delete f;
    return GM_OK;
}

int gm_frontend_debug_repairs(gm_frontend* f, uint32_t* runs) {
    if (!f || !runs) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    *runs = 0;
    if (!f->d_spec) return GM_OK;
    if (int rc = ensure_device(f->device)) return rc;
    HIPC(hipDeviceSynchronize());
    HIPC(hipMemcpy(runs, f->d_spec + size_t(FE_SPEC_K) * 32, sizeof(uint32_t), hipMemcpyDeviceToHost));
    return GM_OK;
}

int gm_frontend_debug_forms(gm_frontend* f, uint32_t counts[3]) {
    if (!f || !counts) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    memcpy(counts, f->forms, sizeof(f->forms));
    return GM_OK;
}

int gm_frontend_lut(gm_frontend* f, float* lut_re, float* lut_im, float* phase_step) {
    if (!f) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (lut_re) memcpy(lut_re, f->lut.data(), 2048 * sizeof(float));
    if (lut_im) memcpy(lut_im, f->lut.data() + 2048, 2048 * sizeof(float));
    if (phase_step) *phase_step = f->phase_step;
    return GM_OK;
}

int gm_frontend_get_state(gm_frontend* f, float* phase_accumulator, float bias_re[8], float bias_im[8]) {
    if (!f) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (int rc = ensure_device(f->device)) return rc;
    gm::FeState s;
    HIPC(hipStreamSynchronize(f->stream));
    HIPC(hipMemcpy(&s, f->d_state, sizeof(s), hipMemcpyDeviceToHost));
    if (phase_accumulator) *phase_accumulator = s.phase_accumulator;
    if (bias_re) memcpy(bias_re, s.bias_re, sizeof(s.bias_re));
    if (bias_im) memcpy(bias_im, s.bias_im, sizeof(s.bias_im));
    return GM_OK;
}

int gm_frontend_set_state(gm_frontend* f, float phase_accumulator, const float bias_re[8], const float bias_im[8]) {
    if (!f || !bias_re || !bias_im) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (int rc = ensure_device(f->device)) return rc;
    gm::FeState s;
    s.phase_accumulator = phase_accumulator;
    memcpy(s.bias_re, bias_re, sizeof(s.bias_re));
    memcpy(s.bias_im, bias_im, sizeof(s.bias_im));
    HIPC(hipStreamSynchronize(f->stream));
    HIPC(hipMemcpy(f->d_state, &s, sizeof(s), hipMemcpyHostToDevice));
    // where on the tabulated orbit is this phase?  (0 = its start; any other value is looked up; a phase that is not on
    // the orbit from 0 sends this front-end down the sequential kernel from here on)
    f->on_orbit = false;
    if (phase_accumulator == 0.0f && !std::signbit(phase_accumulator)) { f->on_orbit = true; f->pos = 0; }
    else if (frontend_build_table(f)) {
        const bool neg = f->phase_step < 0.0f;
        const bool sign_ok = neg ? !(phase_accumulator > 0.0f) : !(phase_accumulator < 0.0f);
        if (sign_ok && fabsf(phase_accumulator) < 2048.0f) {
            const float r = fabsf(phase_accumulator) * (1.0f / 2048.0f);
            for (size_t k = 0; k < f->tab.size(); ++k)
                if (f->tab[k] == r && (r != 0.0f || std::signbit(phase_accumulator) == neg || k == 0)) { f->on_orbit = true; f->pos = uint32_t(k); break; }
        }
    }
    return GM_OK;
}

// DigitalFrontend::process_block (frontend.rs:33-62) on a host buffer, in place: H2D, kernel, D2H.
int gm_frontend_process_block(gm_frontend* f, float* raw_floats, size_t n_floats) {
    if (!f || (!raw_floats && n_floats)) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (int rc = ensure_device(f->device)) return rc;
    const size_t n = n_floats / 2;                // whole samples; an odd trailing float is never inside a 16-float chunk
    if (!n) return GM_OK;
    if (f->io_cap < n) {
        hipFree(f->d_io); f->d_io = nullptr; f->io_cap = 0;
        HIPC(hipMalloc(&f->d_io, n * 8));
        f->io_cap = n;
    }
    HIPC(hipMemcpyAsync(f->d_io, raw_floats, n * 8, hipMemcpyHostToDevice, f->stream));
    if (int rc = frontend_launch(f, f->stream, f->d_io, GM_FMT_C32, f->d_io, 0, ~0ull, n)) return rc;
    HIPC(hipMemcpyAsync(raw_floats, f->d_io, n * 8, hipMemcpyDeviceToHost, f->stream));
    HIPC(hipStreamSynchronize(f->stream));
    return GM_OK;
}

// Device-resident form: d_in (c32 or int8 IQ) -> d_out (c32), asynchronous on `stream` (NULL: the handle's own).
int gm_frontend_process_dev(gm_frontend* f, const void* d_in, int fmt, void* d_out, size_t n_samples, void* stream) {
    if (!f || !d_in || !d_out) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (fmt != GM_FMT_C32 && fmt != GM_FMT_I8_IQ) return set_err(GM_ERR_INVALID_ARG, "front-end input is c32 or int8 IQ");
    if (int rc = ensure_device(f->device)) return rc;
    return frontend_launch(f, stream ? static_cast<hipStream_t>(stream) : f->stream, d_in, fmt, d_out, 0, ~0ull, n_samples);
}

// Many independent streams (antennas, bands) in ONE launch: one workgroup per stream, each with its own front-end state
// and NCO step.  Descriptors travel in a small device array owned by fes[0]; asynchronous on `stream` (NULL: fes[0]'s).
int gm_frontend_process_dev_batch(gm_frontend* const* fes, uint32_t n_streams, const void* const* d_in, int fmt,
                                  void* const* d_out, size_t n_samples, void* stream) {
    if (!fes || !d_in || !d_out || !n_streams) return set_err(GM_ERR_INVALID_ARG, "null pointer / no streams");
    if (fmt != GM_FMT_C32 && fmt != GM_FMT_I8_IQ) return set_err(GM_ERR_INVALID_ARG, "front-end input is c32 or int8 IQ");
    gm_frontend* f0 = fes[0];
    if (!f0) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (int rc = ensure_device(f0->device)) return rc;
    std::vector<gm::FrontendArgs::Stream> h(n_streams);
    for (uint32_t i = 0; i < n_streams; ++i) {
        if (!fes[i] || !d_in[i] || !d_out[i] || fes[i]->device != f0->device) return set_err(GM_ERR_INVALID_ARG, "bad stream entry");
        for (uint32_t j = 0; j < i; ++j)
            if (fes[j] == fes[i]) return set_err(GM_ERR_INVALID_ARG, "a front-end may appear once per batch (its state is sequential)");
        h[i] = frontend_stream(fes[i], d_in[i], d_out[i], 0, ~0ull, n_samples);
    }
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : f0->stream;
    if (f0->batch_cap < n_streams) {
        HIPC(hipStreamSynchronize(st));
        hipFree(f0->d_batch); f0->d_batch = nullptr; f0->batch_cap = 0;
        HIPC(hipMalloc(&f0->d_batch, n_streams * sizeof(gm::FrontendArgs::Stream)));
        f0->batch_cap = n_streams;
    }
    HIPC(hipMemcpyAsync(f0->d_batch, h.data(), n_streams * sizeof(gm::FrontendArgs::Stream), hipMemcpyHostToDevice, st));
    HIPC(hipStreamSynchronize(st));     // the descriptors were read from pageable host memory
    gm::FrontendArgs a{};
    a.streams = f0->d_batch; a.lut = f0->d_lut; a.alpha = f0->alpha; a.con = f0->con;
    bool all_fast = true;
    for (uint32_t i = 0; i < n_streams; ++i) all_fast = all_fast && h[i].ph_table != nullptr;
    if (all_fast) gm::launch_frontend_fast(st, a, int(n_streams), fmt);
    else gm::launch_frontend(st, a, int(n_streams), fmt);
    for (uint32_t i = 0; i < n_streams; ++i) ++fes[i]->forms[all_fast ? 1 : 0];      // the launched form, once for every member
    HIPC(hipGetLastError());
    return GM_OK;
}

int gm_frontend_synchronize(gm_frontend* f) {
    if (!f) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (int rc = ensure_device(f->device)) return rc;
    HIPC(hipStreamSynchronize(f->stream));
    return GM_OK;
}

// rf_thread's block step (rf_thread.rs:43-48): process_block + shared_ring_buffer.write_samples, fused and
// non-blocking: raw samples (c32, or int8 IQ = 2 B/sample over PCIe) are staged in the ring's pinned slots, copied on
// the ring's stream, processed there straight into the ring mirror, and `head` is published when they have landed.
int gm_frontend_write_ring(gm_frontend* f, gm_ring* r, const void* samples, size_t n_samples, int fmt) {
    if (!f || !r || (!samples && n_samples)) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (fmt != GM_FMT_C32 && fmt != GM_FMT_I8_IQ) return set_err(GM_ERR_INVALID_ARG, "front-end input is c32 or int8 IQ");
    if (f->device != r->device) return set_err(GM_ERR_INVALID_ARG, "front-end and ring live on different devices");
    if (n_samples > r->size) return set_err(GM_ERR_OUT_OF_RANGE, "write larger than the ring");
    if (int rc = ensure_device(r->device)) return rc;
    if (int rc = ring_async_init(r)) return rc;
    if (int rc = ring_fe_init(r)) return rc;
    return ring_write_blocks(r, samples, n_samples, fmt == GM_FMT_C32 ? 8 : 2, r->slot_samples, f->d_raw, gm_ring::SLOT_SAMPLES_MAX * 8,
                             [&](const void* d_raw, size_t chunk, uint64_t* cnt) {
                                 *cnt = chunk;
                                 return frontend_launch(f, r->fe_stream, d_raw, fmt, r->d_buf, r->write_pos, r->mask, chunk);
                             });
}

}  // extern "C"

// ====================================================================== streaming stages: what gm_resampler, gm_excisor and gm_ddc share
// A stage turns a stream of inputs into a stream of outputs call by call, whatever the cuts: a history of the last inputs travels between
// calls in two device buffers used alternately, and the counters say where in the stream the next call starts.  Each handle inherits
// this state and adds its plan, its tables, `*_count` (outputs of the next n inputs) and `*_launch` (that kernel's argument block).
// The antenna-array stages (gm_nuller, gm_stap, gm_beamformer) inherit it through ArrayStage, further down: blocks of B time samples of
// A elements each, per block a matrix R and weights w that a call can hand back.  ArrayStage owns what the three share (the count, the
// format verdict, the block / loading / steering-row rules, the capture, the two process bodies, the common argument fields), and
// each handle adds its plan, its `*_launch` and whatever only it keeps.
namespace {
constexpr uint64_t RS_INDEX_MAX = 1ull << 62;
// every gm_*_plan entry: a stream of inputs_so_far, then n_in more, ends at or below 2^62
int stage_check_span(uint64_t inputs_so_far, uint64_t n_in) {
    if (inputs_so_far > RS_INDEX_MAX || n_in > RS_INDEX_MAX || inputs_so_far + n_in > RS_INDEX_MAX)
        return set_err(GM_ERR_INVALID_ARG, "inputs_so_far + n_in above 2^62");
    return GM_OK;
}

struct StreamStage {
    int device = -1;
    void* d_hist[2] = {nullptr, nullptr};   // the last blanked inputs (hist_bytes each): d_hist[cur] is read by the next call, the other written
    size_t hist_bytes = 0;
    int cur = 0;
    unsigned long long* d_blanked = nullptr;
    hipStream_t stream = nullptr, last_stream = nullptr;    // the handle's own, and the one the last call ran on
    uint64_t base = 0;                      // absolute index of the first input since create / reset
    uint64_t inputs = 0, outputs = 0;       // since create / reset
    void* d_in = nullptr; size_t in_cap = 0;    // bytes; staging of the host-buffer entry
    cf* d_out = nullptr; size_t out_cap = 0;    // samples
};

// the end of a handle's create (behind its own fills): zeroed history and counter, then the stream
hipError_t stage_create(StreamStage* s, size_t hist_bytes) {
    s->hist_bytes = hist_bytes;
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
        e = hipMalloc(&s->d_hist[i], hist_bytes);
        if (e == hipSuccess) e = hipMemset(s->d_hist[i], 0, hist_bytes);
    }
    if (e == hipSuccess) e = hipMalloc(&s->d_blanked, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(s->d_blanked, 0, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);    // the fills have run before a kernel on a non-blocking stream can touch the state (see gm_ring_create)
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    return e;
}
// the start of a handle's destroy: the streams drained, the shared buffers freed
void stage_destroy(StreamStage* s) {
    hipSetDevice(s->device);
    if (s->last_stream && s->last_stream != s->stream) hipStreamSynchronize(s->last_stream);
    if (s->stream) { hipStreamSynchronize(s->stream); hipStreamDestroy(s->stream); }
    hipFree(s->d_hist[0]); hipFree(s->d_hist[1]); hipFree(s->d_blanked); hipFree(s->d_in); hipFree(s->d_out);
}
// before work on `st` that reads what the last call wrote (the history; the excisor's gains): that call has run
int stage_join(StreamStage* s, hipStream_t st) {
    if (s->last_stream && s->last_stream != st) HIPC(hipStreamSynchronize(s->last_stream));
    return GM_OK;
}
int stage_sync(StreamStage* s) {
    HIPC(hipStreamSynchronize(s->stream));
    return stage_join(s, s->stream);
}
int stage_synchronize(StreamStage* s) {
    if (!s) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (int rc = ensure_device(s->device)) return rc;
    return stage_sync(s);
}
int stage_stats(StreamStage* s, uint64_t* inputs, uint64_t* outputs, uint64_t* blanked) {
    if (int rc = stage_synchronize(s)) return rc;
    if (blanked) {
        unsigned long long b = 0;
        HIPC(hipMemcpy(&b, s->d_blanked, sizeof(b), hipMemcpyDeviceToHost));
        *blanked = b;
    }
    if (inputs) *inputs = s->inputs;
    if (outputs) *outputs = s->outputs;
    return GM_OK;
}
// `also()` enqueues on the handle's stream whatever else the handle zeroes
template <class Also>
int stage_reset(StreamStage* s, uint64_t input_index, Also&& also) {
    if (!s) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (input_index > RS_INDEX_MAX) return set_err(GM_ERR_INVALID_ARG, "input_index above 2^62");
    if (int rc = ensure_device(s->device)) return rc;
    if (int rc = stage_sync(s)) return rc;
    HIPC(hipMemsetAsync(s->d_hist[0], 0, s->hist_bytes, s->stream));
    HIPC(hipMemsetAsync(s->d_hist[1], 0, s->hist_bytes, s->stream));
    HIPC(hipMemsetAsync(s->d_blanked, 0, sizeof(unsigned long long), s->stream));
    HIPC(also());
    HIPC(hipStreamSynchronize(s->stream));
    s->cur = 0; s->base = input_index; s->inputs = 0; s->outputs = 0;
    return GM_OK;
}
// a launch has gone out on `st`: the history buffers change roles, the counters advance
int stage_launched(StreamStage* s, hipStream_t st, uint64_t n_in, uint64_t n_out) {
    HIPC(hipGetLastError());
    s->cur ^= 1; s->inputs += n_in; s->outputs += n_out; s->last_stream = st;
    return GM_OK;
}

// The checks the process entries share: nothing is touched when one fails.  `fmt_err`: the caller's verdict on its format argument, null
// where it is fine (or there is none); `plan_entry`: the entry that gives the output count; *cnt: that count.
template <class H>
int stage_check_call(const H* h, uint64_t (*count)(const H*, uint64_t), const char* fmt_err, const void* in, size_t n_in, const void* out,
                     size_t out_cap, const char* plan_entry, uint64_t* cnt) {
    if (!h) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (fmt_err) return set_err(GM_ERR_INVALID_ARG, fmt_err);
    if (!in && n_in) return set_err(GM_ERR_INVALID_ARG, "null input");
    if (uint64_t(n_in) > (1ull << 31) || h->base + h->inputs + n_in > RS_INDEX_MAX)
        return set_err(GM_ERR_INVALID_ARG, "at most 2^31 samples a call, 2^62 a stream");
    *cnt = count(h, n_in);
    if (*cnt > out_cap)
        return set_err(GM_ERR_OUT_OF_RANGE, (std::string("out_cap below the call's output count (") + plan_entry + " gives it)").c_str());
    if (*cnt && !out) return set_err(GM_ERR_INVALID_ARG, "null output");
    return GM_OK;
}
// the device entries' own refusal: the `cnt` outputs may not lie over the inputs
int stage_check_overlap(const void* d_in, size_t in_bytes, const void* d_out, uint64_t cnt) {
    const uintptr_t i0 = reinterpret_cast<uintptr_t>(d_in), i1 = i0 + in_bytes;
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(d_out), o1 = o0 + cnt * 8;
    if (cnt && in_bytes && i0 < o1 && o0 < i1) return set_err(GM_ERR_INVALID_ARG, "d_out overlaps d_in");
    return GM_OK;
}
// The host-buffer entries behind their checks: grow the staging, H2D, `launch(stream, d_in, d_out)`, D2H, wait.  A stage with several
// output planes (the channelizer) stages them as [planes][per_plane] and delivers plane i at out + i * out_pitch.
template <class Launch>
int stage_process(StreamStage* s, const void* in, size_t in_bytes, gm_c32* out, uint64_t per_plane, size_t* n_out, Launch&& launch,
                  uint64_t planes = 1, size_t out_pitch = 0) {
    if (n_out) *n_out = size_t(per_plane);
    if (!in_bytes) return GM_OK;
    const uint64_t cnt = per_plane * planes;
    if (int rc = ensure_device(s->device)) return rc;
    if (s->in_cap < in_bytes || s->out_cap < cnt) HIPC(hipStreamSynchronize(s->stream));
    if (s->in_cap < in_bytes) {
        hipFree(s->d_in); s->d_in = nullptr; s->in_cap = 0;
        HIPC(hipMalloc(&s->d_in, in_bytes));
        s->in_cap = in_bytes;
    }
    if (s->out_cap < cnt) {
        hipFree(s->d_out); s->d_out = nullptr; s->out_cap = 0;
        HIPC(hipMalloc(reinterpret_cast<void**>(&s->d_out), size_t(cnt) * sizeof(cf)));
        s->out_cap = size_t(cnt);
    }
    if (int rc = stage_join(s, s->stream)) return rc;
    HIPC(hipMemcpyAsync(s->d_in, in, in_bytes, hipMemcpyHostToDevice, s->stream));
    if (int rc = launch(s->stream, s->d_in, s->d_out)) return rc;
    if (cnt && planes == 1) HIPC(hipMemcpyAsync(out, s->d_out, size_t(cnt) * sizeof(cf), hipMemcpyDeviceToHost, s->stream));
    for (uint64_t i = 0; cnt && planes > 1 && i < planes; ++i)
        HIPC(hipMemcpyAsync(out + i * out_pitch, s->d_out + i * per_plane, size_t(per_plane) * sizeof(cf), hipMemcpyDeviceToHost, s->stream));
    HIPC(hipStreamSynchronize(s->stream));
    return GM_OK;
}
}  // namespace

// ====================================================================== rate conversion and pulse blanking (gm_resampler)
// gnss_mi355x.h states the definition; tests/resample_model.py restates it in float64.
namespace {
struct ResamplerPlan {
    uint32_t up = 1, down = 1, T = 0, PHI = 0;
    double cutoff = 0.9, beta = 8.0;
    float thr = 0.0f;
};

int resampler_rules(const gm_resampler_cfg* c, ResamplerPlan& p) {
    if (!c) return set_err(GM_ERR_INVALID_ARG, "null cfg");
    if (c->reserved) return set_err(GM_ERR_INVALID_ARG, "gm_resampler_cfg.reserved must be 0");
    if (c->up < 1 || c->down < 1 || c->up > (1u << 24) || c->down > (1u << 24)) return set_err(GM_ERR_INVALID_ARG, "up and down: 1 .. 2^24");
    uint32_t a = c->up, b = c->down;
    while (b) { const uint32_t t = a % b; a = b; b = t; }
    p.up = c->up / a; p.down = c->down / a;
    if (uint64_t(p.up) > 16ull * p.down || uint64_t(p.down) > 16ull * p.up) return set_err(GM_ERR_INVALID_ARG, "up / down outside [1/16, 16]");
    if (c->taps) {
        if (c->taps % 8 || c->taps < 8 || c->taps > 256) return set_err(GM_ERR_INVALID_ARG, "taps: a multiple of 8 in 8 .. 256");
        p.T = c->taps;
    } else {
        const uint32_t ceil_ratio = p.down > p.up ? (p.down + p.up - 1) / p.up : 1;
        p.T = std::min<uint32_t>(256, 32 * ceil_ratio);
    }
    if (c->n_phases) {
        if (c->n_phases < 16 || c->n_phases > 1024 || (c->n_phases & (c->n_phases - 1))) return set_err(GM_ERR_INVALID_ARG, "n_phases: a power of two in 16 .. 1024");
        p.PHI = c->n_phases;
    } else p.PHI = 256;
    if (!(c->cutoff >= 0.0f && c->cutoff <= 1.0f)) return set_err(GM_ERR_INVALID_ARG, "cutoff: (0, 1], 0 for the default");
    if (!(c->kaiser_beta >= 0.0f && c->kaiser_beta <= 20.0f)) return set_err(GM_ERR_INVALID_ARG, "kaiser_beta: [0, 20]");
    if (!(c->blank_threshold >= 0.0f)) return set_err(GM_ERR_INVALID_ARG, "blank_threshold: >= 0");
    p.cutoff = c->cutoff == 0.0f ? 0.9 : double(c->cutoff);
    p.beta = c->kaiser_beta == 0.0f ? 8.0 : double(c->kaiser_beta);
    p.thr = c->blank_threshold;
    return GM_OK;
}

// total_out(A) = max(0, ceil((A - T/2) * up / down)), with B = A - T/2 = b * down + B': b * up + ceil(B' * up / down); B' * up < 2^48
uint64_t resampler_total_out(const ResamplerPlan& p, uint64_t A) {
    const uint64_t half = p.T / 2;
    if (A <= half) return 0;
    const uint64_t B = A - half, b = B / p.down, Br = B % p.down;
    return b * p.up + (Br * p.up + p.down - 1) / p.down;
}

double bessel_i0(double x) {                      // sum_k ((x/2)^k / k!)^2: every term positive, x <= 20
    const double h = 0.5 * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; ++k) {
        term *= (h / k) * (h / k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

void resampler_design(const ResamplerPlan& p, float* table) {
    const double PI = 3.14159265358979323846;
    const double rho = p.up < p.down ? double(p.up) / double(p.down) : 1.0, fc = p.cutoff * rho;
    const double inv_i0 = 1.0 / bessel_i0(p.beta), halfT = 0.5 * double(p.T);
    std::vector<double> row(p.T);
    for (uint32_t phi = 0; phi <= p.PHI; ++phi) {
        double sum = 0.0;
        for (uint32_t j = 0; j < p.T; ++j) {
            const double t = double(j) - (halfT - 1.0) - double(phi) / double(p.PHI);
            double h = 0.0;
            if (fabs(t) <= halfT) {
                const double u = t / halfT, w = 1.0 - u * u, x = fc * t;
                const double sinc = x == 0.0 ? 1.0 : sin(PI * x) / (PI * x);
                h = fc * sinc * bessel_i0(p.beta * sqrt(w > 0.0 ? w : 0.0)) * inv_i0;
            }
            row[j] = h;
            sum += h;
        }
        for (uint32_t j = 0; j < p.T; ++j) table[size_t(phi) * p.T + j] = float(row[j] / sum);
    }
}
}  // namespace

struct gm_resampler : StreamStage {         // history: the last T blanked inputs (cf)
    ResamplerPlan plan;
    std::vector<float> table;               // [PHI + 1][T]
    float* d_table = nullptr;
    cf* d_scratch = nullptr;                // gm_frontend_write_ring_resampled: the front-end's linear output (SLOT_SAMPLES_MAX samples)
};

// one call's kernels on `st`, outputs to out[(out_start + k) & out_mask]; the caller has checked every argument; n_in > 0
static int resampler_launch(gm_resampler* r, hipStream_t st, const void* d_in, int fmt, uint64_t n_in, cf* out, uint64_t out_start,
                            uint64_t out_mask, uint64_t n_out) {
    const ResamplerPlan& p = r->plan;
    const uint64_t A = r->base + r->inputs, m0 = resampler_total_out(p, A);
    gm::ResampleArgs a{};
    a.in = d_in; a.n_in = n_in;
    a.hist_in = static_cast<const cf*>(r->d_hist[r->cur]); a.hist_out = static_cast<cf*>(r->d_hist[r->cur ^ 1]);
    a.table = r->d_table; a.T = p.T; a.PHI = p.PHI; a.up = p.up; a.down = p.down;
    a.a0 = m0 / p.up; a.mr0 = m0 % p.up; a.in_index = A;
    a.n_out = n_out; a.tile_out = gm::resample_tile_out(p.T, p.up, p.down);
    a.out = out; a.out_start = out_start; a.out_mask = out_mask;
    a.thr2 = p.thr * p.thr; a.blank = p.thr > 0.0f ? 1 : 0;
    a.blanked = r->d_blanked;
    gm::launch_resample(st, a, fmt);
    return stage_launched(r, st, n_in, n_out);
}
static uint64_t resampler_count(const gm_resampler* r, uint64_t n_in) {
    const uint64_t A = r->base + r->inputs;
    return resampler_total_out(r->plan, A + n_in) - resampler_total_out(r->plan, A);
}
static const char* resampler_fmt_err(int fmt) {
    return fmt != GM_FMT_C32 && fmt != GM_FMT_I8_IQ ? "resampler input is c32 or int8 IQ" : nullptr;
}

extern "C" {

int gm_resampler_plan(const gm_resampler_cfg* cfg, uint64_t inputs_so_far, uint64_t n_in, uint32_t* up_reduced, uint32_t* down_reduced,
                      uint32_t* taps, uint32_t* n_phases, uint64_t* n_out) {
    ResamplerPlan p;
    if (int rc = resampler_rules(cfg, p)) return rc;
    if (int rc = stage_check_span(inputs_so_far, n_in)) return rc;
    if (up_reduced) *up_reduced = p.up;
    if (down_reduced) *down_reduced = p.down;
    if (taps) *taps = p.T;
    if (n_phases) *n_phases = p.PHI;
    if (n_out) *n_out = resampler_total_out(p, inputs_so_far + n_in) - resampler_total_out(p, inputs_so_far);
    return GM_OK;
}

int gm_resampler_design(const gm_resampler_cfg* cfg, float* table) {
    ResamplerPlan p;
    if (int rc = resampler_rules(cfg, p)) return rc;
    if (!table) return set_err(GM_ERR_INVALID_ARG, "null table");
    resampler_design(p, table);
    return GM_OK;
}

int gm_resampler_create(const gm_resampler_cfg* cfg, gm_resampler** out) {
    if (!out) return set_err(GM_ERR_INVALID_ARG, "null out");
    *out = nullptr;
    ResamplerPlan p;
    if (int rc = resampler_rules(cfg, p)) return rc;
    if (int rc = ensure_device(g_device)) return rc;
    gm_resampler* r = new gm_resampler;
    r->device = g_device; r->plan = p;
    r->table.resize(size_t(p.PHI + 1) * p.T);
    resampler_design(p, r->table.data());
    hipError_t e = hipMalloc(&r->d_table, r->table.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(r->d_table, r->table.data(), r->table.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = stage_create(r, size_t(p.T) * sizeof(cf));
    if (e != hipSuccess) { gm_resampler_destroy(r); return hip_fail(e, "gm_resampler_create"); }
    *out = r;
    return GM_OK;
}

int gm_resampler_destroy(gm_resampler* r) {
    if (!r) return GM_OK;
    stage_destroy(r);
    hipFree(r->d_table); hipFree(r->d_scratch);
    delete r;
    return GM_OK;
}

int gm_resampler_reset(gm_resampler* r, uint64_t input_index) {
    return stage_reset(r, input_index, [] { return hipSuccess; });
}

int gm_resampler_taps(gm_resampler* r, float* table) {
    if (!r || !table) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    memcpy(table, r->table.data(), r->table.size() * sizeof(float));
    return GM_OK;
}

int gm_resampler_stats(gm_resampler* r, uint64_t* inputs, uint64_t* outputs, uint64_t* blanked) {
    return stage_stats(r, inputs, outputs, blanked);
}

int gm_resampler_process_dev(gm_resampler* r, const void* d_in, int fmt, size_t n_in, void* d_out, size_t out_cap, size_t* n_out,
                             void* stream) {
    uint64_t cnt = 0;
    if (int rc = stage_check_call(r, resampler_count, resampler_fmt_err(fmt), d_in, n_in, d_out, out_cap, "gm_resampler_plan", &cnt)) return rc;
    if (int rc = stage_check_overlap(d_in, n_in * (fmt == GM_FMT_C32 ? 8 : 2), d_out, cnt)) return rc;
    if (n_out) *n_out = size_t(cnt);
    if (!n_in) return GM_OK;
    if (int rc = ensure_device(r->device)) return rc;
    return resampler_launch(r, stream ? static_cast<hipStream_t>(stream) : r->stream, d_in, fmt, n_in, static_cast<cf*>(d_out), 0, ~0ull, cnt);
}

int gm_resampler_process(gm_resampler* r, const void* in, int fmt, size_t n_in, gm_c32* out, size_t out_cap, size_t* n_out) {
    uint64_t cnt = 0;
    if (int rc = stage_check_call(r, resampler_count, resampler_fmt_err(fmt), in, n_in, out, out_cap, "gm_resampler_plan", &cnt)) return rc;
    return stage_process(r, in, n_in * (fmt == GM_FMT_C32 ? 8 : 2), out, cnt, n_out, [&](hipStream_t st, const void* d_in, cf* d_out) {
        return resampler_launch(r, st, d_in, fmt, n_in, d_out, 0, ~0ull, cnt);
    });
}

int gm_resampler_synchronize(gm_resampler* r) { return stage_synchronize(r); }

}  // extern "C"

// ====================================================================== narrowband interference excision (gm_excisor)
// gnss_mi355x.h states the definition; tests/excise_model.py restates it in float64.
namespace {
struct ExcisorPlan {
    uint32_t B = 1024, guard = 0;
    float factor = 4.0f, thr = 0.0f;
};

int excisor_rules(const gm_excisor_cfg* c, ExcisorPlan& p) {
    if (!c) return set_err(GM_ERR_INVALID_ARG, "null cfg");
    for (int i = 0; i < 4; ++i)
        if (c->reserved[i]) return set_err(GM_ERR_INVALID_ARG, "gm_excisor_cfg.reserved must be 0");
    if (c->block) {
        if (c->block != 256 && c->block != 512 && c->block != 1024 && c->block != 2048 && c->block != 4096)
            return set_err(GM_ERR_INVALID_ARG, "block: 256, 512, 1024, 2048 or 4096");
        p.B = c->block;
    } else p.B = 1024;
    if (c->guard_bins > 16) return set_err(GM_ERR_INVALID_ARG, "guard_bins: 0 .. 16");
    if (!(c->threshold_factor == 0.0f || c->threshold_factor > 1.0f)) return set_err(GM_ERR_INVALID_ARG, "threshold_factor: > 1, 0 for the default");
    if (!(c->blank_threshold >= 0.0f)) return set_err(GM_ERR_INVALID_ARG, "blank_threshold: >= 0");
    p.guard = c->guard_bins;
    p.factor = c->threshold_factor == 0.0f ? 4.0f : c->threshold_factor;
    p.thr = c->blank_threshold;
    return GM_OK;
}

// total_out(A) = H * max(0, A div H - 1)
uint64_t excisor_total_out(const ExcisorPlan& p, uint64_t A) {
    const uint64_t H = p.B / 2, q = A / H;
    return q > 1 ? (q - 1) * H : 0;
}

// gm_excisor_block_cfg's argument rules and defaults
constexpr size_t EX_BSTAT_BYTES = size_t(gm::EX_BSTAT_SLOTS) * gm::EX_BSTAT_STRIDE * sizeof(unsigned long long);

int excisor_block_rules(const gm_excisor_block_cfg* c, float& factor, uint32_t& guard) {
    if (!c) return set_err(GM_ERR_INVALID_ARG, "null cfg");
    for (int i = 0; i < 6; ++i)
        if (c->reserved[i]) return set_err(GM_ERR_INVALID_ARG, "gm_excisor_block_cfg.reserved must be 0");
    if (c->guard_bins > 16) return set_err(GM_ERR_INVALID_ARG, "guard_bins: 0 .. 16");
    if (!(c->threshold_factor == 0.0f || c->threshold_factor > 1.0f)) return set_err(GM_ERR_INVALID_ARG, "threshold_factor: > 1, 0 for the default");
    factor = c->threshold_factor == 0.0f ? 16.0f : c->threshold_factor;
    guard = c->guard_bins;
    return GM_OK;
}

void excisor_windows(uint32_t B, float* wa, float* ws) {
    const double PI = 3.14159265358979323846;
    for (uint32_t i = 0; i < B; ++i) {
        const double s = sin(PI * double(i) / double(B));
        if (wa) wa[i] = float(s);
        if (ws) ws[i] = float(s / double(B));
    }
}
}  // namespace

struct gm_excisor : StreamStage {           // history: the last 3H blanked inputs (cf)
    ExcisorPlan plan;
    std::vector<float> wa, ws;              // [B] each
    float *d_wa = nullptr, *d_ws = nullptr, *d_gains = nullptr;
    float* h_gains = nullptr;               // pinned staging of gm_excisor_set_gains
    hipEvent_t gains_ev = nullptr; bool gains_pending = false;
    cf *d_tw_fwd = nullptr, *d_tw_inv = nullptr;
    bool block_adapt = false; float block_factor = 16.0f; uint32_t block_guard = 0;   // block-adapt mode: host state, handed to every launch
    unsigned long long* d_bstat = nullptr;  // [EX_BSTAT_SLOTS] rows of {blocks, blocks flagged, bins flagged, bins zeroed}: the counters are the rows' sums
    float* cap_p = nullptr; unsigned char* cap_m = nullptr; uint64_t cap_blocks = 0;  // the armed capture (the caller's device buffers)
    float *d_partial = nullptr, *d_P = nullptr;   // the periodogram's partial sums [EX_CHUNKS_MAX][B] and its words [B]
    uint32_t* d_stat = nullptr;             // {median word, flagged, zeroed} of the last adapt
    cf *d_scratch = nullptr, *d_mid = nullptr;  // gm_frontend_write_ring_conditioned: the front-end's linear output, and the excisor's in front of a resampler
};

static uint64_t excisor_count(const gm_excisor* x, uint64_t n_in) {
    const uint64_t A = x->base + x->inputs;
    return excisor_total_out(x->plan, A + n_in) - excisor_total_out(x->plan, A);
}
// one call's kernels on `st`, outputs to out[(out_start + k) & out_mask]; the caller has checked every argument; n_in > 0
static int excisor_launch(gm_excisor* x, hipStream_t st, const void* d_in, int fmt, uint64_t n_in, cf* out, uint64_t out_start,
                          uint64_t out_mask, uint64_t n_out, bool capture = false) {
    const ExcisorPlan& p = x->plan;
    const uint64_t H = p.B / 2, A = x->base + x->inputs, s0 = excisor_total_out(p, A) / H;
    if (x->gains_pending && st != x->stream) HIPC(hipStreamWaitEvent(st, x->gains_ev, 0));     // gains set on the handle's stream
    gm::ExciseArgs a{};
    a.in = d_in; a.n_in = n_in;
    a.hist_in = static_cast<const cf*>(x->d_hist[x->cur]); a.hist_out = static_cast<cf*>(x->d_hist[x->cur ^ 1]);
    a.wa = x->d_wa; a.ws = x->d_ws; a.gains = x->d_gains; a.tw_fwd = x->d_tw_fwd; a.tw_inv = x->d_tw_inv;
    a.B = p.B;
    a.rel0 = int64_t(s0 * H) - int64_t(H) - int64_t(A);
    a.n_seg = uint32_t(n_out / H); a.G = gm::excise_tile_segments(a.n_seg);
    a.out = out; a.out_start = out_start; a.out_mask = out_mask;
    a.thr2 = p.thr * p.thr; a.blank = p.thr > 0.0f ? 1 : 0;
    a.blanked = x->d_blanked;
    a.block_adapt = x->block_adapt ? 1 : 0; a.bfactor = x->block_factor; a.bguard = x->block_guard; a.bstat = x->d_bstat;
    if (capture && x->block_adapt) { a.cap_p = x->cap_p; a.cap_m = x->cap_m; }     // (the caller has checked cap_blocks)
    gm::launch_excise(st, a, fmt);
    return stage_launched(x, st, n_in, n_out);
}
static const char* excisor_fmt_err(int fmt) {
    return fmt != GM_FMT_C32 && fmt != GM_FMT_I8_IQ ? "excisor input is c32 or int8 IQ" : nullptr;
}

extern "C" {

int gm_excisor_plan(const gm_excisor_cfg* cfg, uint64_t inputs_so_far, uint64_t n_in, uint32_t* block, uint32_t* guard_bins,
                    float* threshold_factor, uint64_t* n_out) {
    ExcisorPlan p;
    if (int rc = excisor_rules(cfg, p)) return rc;
    if (int rc = stage_check_span(inputs_so_far, n_in)) return rc;
    if (block) *block = p.B;
    if (guard_bins) *guard_bins = p.guard;
    if (threshold_factor) *threshold_factor = p.factor;
    if (n_out) *n_out = excisor_total_out(p, inputs_so_far + n_in) - excisor_total_out(p, inputs_so_far);
    return GM_OK;
}

int gm_excisor_windows(const gm_excisor_cfg* cfg, float* analysis, float* synthesis) {
    ExcisorPlan p;
    if (int rc = excisor_rules(cfg, p)) return rc;
    if (!analysis && !synthesis) return set_err(GM_ERR_INVALID_ARG, "null windows");
    excisor_windows(p.B, analysis, synthesis);
    return GM_OK;
}

int gm_excisor_create(const gm_excisor_cfg* cfg, gm_excisor** out) {
    if (!out) return set_err(GM_ERR_INVALID_ARG, "null out");
    *out = nullptr;
    ExcisorPlan p;
    if (int rc = excisor_rules(cfg, p)) return rc;
    if (int rc = ensure_device(g_device)) return rc;
    gm_excisor* x = new gm_excisor;
    x->device = g_device; x->plan = p;
    const size_t B = p.B, wbytes = B * sizeof(float), hist_bytes = 3 * (B / 2) * sizeof(cf);
    x->wa.resize(B); x->ws.resize(B);
    excisor_windows(p.B, x->wa.data(), x->ws.data());
    std::vector<cf> twf(gm::EX_TW_MAX), twi(gm::EX_TW_MAX);
    int n_fwd = 0, n_inv = 0;
    gm::excise_twiddles(p.B, twf.data(), twi.data(), &n_fwd, &n_inv);
    const std::vector<float> ones(B, 1.0f);
    hipError_t e = hipMalloc(&x->d_wa, wbytes);
    if (e == hipSuccess) e = hipMalloc(&x->d_ws, wbytes);
    if (e == hipSuccess) e = hipMalloc(&x->d_gains, wbytes);
    if (e == hipSuccess) e = hipMalloc(&x->d_P, wbytes);
    if (e == hipSuccess) e = hipMalloc(&x->d_partial, size_t(gm::EX_CHUNKS_MAX) * wbytes);
    if (e == hipSuccess) e = hipMalloc(&x->d_stat, 4 * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&x->d_tw_fwd, gm::EX_TW_MAX * sizeof(cf));
    if (e == hipSuccess) e = hipMalloc(&x->d_tw_inv, gm::EX_TW_MAX * sizeof(cf));
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&x->h_gains), wbytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMemcpy(x->d_wa, x->wa.data(), wbytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(x->d_ws, x->ws.data(), wbytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(x->d_gains, ones.data(), wbytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(x->d_tw_fwd, twf.data(), gm::EX_TW_MAX * sizeof(cf), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(x->d_tw_inv, twi.data(), gm::EX_TW_MAX * sizeof(cf), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(x->d_P, 0, wbytes);
    if (e == hipSuccess) e = hipMemset(x->d_stat, 0, 4 * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&x->d_bstat, EX_BSTAT_BYTES);
    if (e == hipSuccess) e = hipMemset(x->d_bstat, 0, EX_BSTAT_BYTES);
    if (e == hipSuccess) e = stage_create(x, hist_bytes);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&x->gains_ev, hipEventDisableTiming);
    if (e != hipSuccess) { gm_excisor_destroy(x); return hip_fail(e, "gm_excisor_create"); }
    *out = x;
    return GM_OK;
}

int gm_excisor_destroy(gm_excisor* x) {
    if (!x) return GM_OK;
    stage_destroy(x);
    if (x->gains_ev) hipEventDestroy(x->gains_ev);
    hipFree(x->d_wa); hipFree(x->d_ws); hipFree(x->d_gains); hipFree(x->d_P); hipFree(x->d_partial); hipFree(x->d_stat);
    hipFree(x->d_tw_fwd); hipFree(x->d_tw_inv); hipFree(x->d_bstat); hipFree(x->d_scratch); hipFree(x->d_mid);
    if (x->h_gains) hipHostFree(x->h_gains);
    delete x;
    return GM_OK;
}

int gm_excisor_reset(gm_excisor* x, uint64_t input_index) {
    return stage_reset(x, input_index, [&] { return hipMemsetAsync(x->d_bstat, 0, EX_BSTAT_BYTES, x->stream); });
}

int gm_excisor_set_gains(gm_excisor* x, const float* gains) {
    if (!x || !gains) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    const size_t B = x->plan.B;
    for (size_t k = 0; k < B; ++k)
        if (!(gains[k] >= 0.0f && gains[k] <= 1.0f)) return set_err(GM_ERR_INVALID_ARG, "every gain in [0, 1]");
    if (int rc = ensure_device(x->device)) return rc;
    if (x->gains_pending) HIPC(hipEventSynchronize(x->gains_ev));     // the staging words of the last call have left
    if (int rc = stage_join(x, x->stream)) return rc;                 // a call in flight elsewhere reads the old gains
    memcpy(x->h_gains, gains, B * sizeof(float));
    HIPC(hipMemcpyAsync(x->d_gains, x->h_gains, B * sizeof(float), hipMemcpyHostToDevice, x->stream));
    HIPC(hipEventRecord(x->gains_ev, x->stream));
    x->gains_pending = true;
    return GM_OK;
}

int gm_excisor_gains(gm_excisor* x, float* gains) {
    if (!x || !gains) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (int rc = ensure_device(x->device)) return rc;
    if (int rc = stage_sync(x)) return rc;
    HIPC(hipMemcpy(gains, x->d_gains, x->plan.B * sizeof(float), hipMemcpyDeviceToHost));
    return GM_OK;
}

int gm_excisor_adapt_dev(gm_excisor* x, const void* d_in, int fmt, size_t n, void* stream) {
    if (!x) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (const char* err = excisor_fmt_err(fmt)) return set_err(GM_ERR_INVALID_ARG, err);
    if (!d_in) return set_err(GM_ERR_INVALID_ARG, "null input");
    const ExcisorPlan& p = x->plan;
    if (n < p.B || uint64_t(n) > (1ull << 31)) return set_err(GM_ERR_INVALID_ARG, "adapt takes block .. 2^31 samples");
    if (int rc = ensure_device(x->device)) return rc;
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : x->stream;
    if (x->gains_pending && st != x->stream) HIPC(hipStreamWaitEvent(st, x->gains_ev, 0));       // the mask is written behind a set_gains
    const uint64_t H = p.B / 2, J = (uint64_t(n) - p.B) / H + 1;
    const uint64_t per = (J + gm::EX_CHUNKS_MAX - 1) / gm::EX_CHUNKS_MAX;
    gm::ExcisePsdArgs pa{};
    pa.in = d_in; pa.wa = x->d_wa; pa.tw_fwd = x->d_tw_fwd; pa.B = p.B;
    pa.J = J; pa.C = uint32_t(per < 4 ? 4 : per); pa.n_chunks = uint32_t((J + pa.C - 1) / pa.C);
    pa.partial = x->d_partial;
    pa.thr2 = p.thr * p.thr; pa.blank = p.thr > 0.0f ? 1 : 0;
    gm::ExciseMaskArgs ma{};
    ma.partial = x->d_partial; ma.n_chunks = pa.n_chunks; ma.B = p.B;
    ma.factor = p.factor; ma.guard = p.guard;
    ma.P = x->d_P; ma.gains = x->d_gains; ma.stat = x->d_stat;
    gm::launch_excise_adapt(st, pa, ma, fmt);
    HIPC(hipGetLastError());
    x->last_stream = st;
    return GM_OK;
}

int gm_excisor_psd(gm_excisor* x, float* P, float* median, uint32_t* n_flagged, uint32_t* n_zeroed) {
    if (!x) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (int rc = ensure_device(x->device)) return rc;
    if (int rc = stage_sync(x)) return rc;
    uint32_t stat[4] = {0, 0, 0, 0};
    HIPC(hipMemcpy(stat, x->d_stat, sizeof(stat), hipMemcpyDeviceToHost));
    if (P) HIPC(hipMemcpy(P, x->d_P, x->plan.B * sizeof(float), hipMemcpyDeviceToHost));
    if (median) memcpy(median, &stat[0], sizeof(float));
    if (n_flagged) *n_flagged = stat[1];
    if (n_zeroed) *n_zeroed = stat[2];
    return GM_OK;
}

int gm_excisor_stats(gm_excisor* x, uint64_t* inputs, uint64_t* outputs, uint64_t* blanked) {
    return stage_stats(x, inputs, outputs, blanked);
}

int gm_excisor_process_dev(gm_excisor* x, const void* d_in, int fmt, size_t n_in, void* d_out, size_t out_cap, size_t* n_out,
                           void* stream) {
    uint64_t cnt = 0;
    if (int rc = stage_check_call(x, excisor_count, excisor_fmt_err(fmt), d_in, n_in, d_out, out_cap, "gm_excisor_plan", &cnt)) return rc;
    if (int rc = stage_check_overlap(d_in, n_in * (fmt == GM_FMT_C32 ? 8 : 2), d_out, cnt)) return rc;
    const bool capture = x->block_adapt && (x->cap_p || x->cap_m) && cnt >= x->plan.B / 2;
    if (capture && x->cap_blocks < cnt / (x->plan.B / 2) + 1)
        return set_err(GM_ERR_OUT_OF_RANGE, "the armed capture holds fewer blocks than the call's segments + 1");
    if (n_out) *n_out = size_t(cnt);
    if (!n_in) return GM_OK;
    if (int rc = ensure_device(x->device)) return rc;
    return excisor_launch(x, stream ? static_cast<hipStream_t>(stream) : x->stream, d_in, fmt, n_in, static_cast<cf*>(d_out), 0, ~0ull, cnt,
                          capture);
}

int gm_excisor_block_plan(const gm_excisor_block_cfg* cfg, float* threshold_factor, uint32_t* guard_bins) {
    float factor = 0.0f;
    uint32_t guard = 0;
    if (int rc = excisor_block_rules(cfg, factor, guard)) return rc;
    if (threshold_factor) *threshold_factor = factor;
    if (guard_bins) *guard_bins = guard;
    return GM_OK;
}

int gm_excisor_set_block_adapt(gm_excisor* x, const gm_excisor_block_cfg* cfg) {
    if (!x) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (!cfg) {                                      // off: the armed capture goes with the mode
        x->block_adapt = false; x->cap_p = nullptr; x->cap_m = nullptr; x->cap_blocks = 0;
        return GM_OK;
    }
    float factor = 0.0f;
    uint32_t guard = 0;
    if (int rc = excisor_block_rules(cfg, factor, guard)) return rc;
    x->block_adapt = true; x->block_factor = factor; x->block_guard = guard;
    return GM_OK;
}

int gm_excisor_block_stats(gm_excisor* x, uint64_t* blocks, uint64_t* blocks_flagged, uint64_t* bins_flagged, uint64_t* bins_zeroed) {
    if (!x) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (int rc = ensure_device(x->device)) return rc;
    if (int rc = stage_sync(x)) return rc;
    unsigned long long rows[gm::EX_BSTAT_SLOTS * gm::EX_BSTAT_STRIDE], c[4] = {0, 0, 0, 0};
    HIPC(hipMemcpy(rows, x->d_bstat, EX_BSTAT_BYTES, hipMemcpyDeviceToHost));
    for (int r = 0; r < gm::EX_BSTAT_SLOTS; ++r)
        for (int k = 0; k < 4; ++k) c[k] += rows[r * gm::EX_BSTAT_STRIDE + k];
    if (blocks) *blocks = c[0];
    if (blocks_flagged) *blocks_flagged = c[1];
    if (bins_flagged) *bins_flagged = c[2];
    if (bins_zeroed) *bins_zeroed = c[3];
    return GM_OK;
}

int gm_excisor_block_capture(gm_excisor* x, float* d_power, uint8_t* d_mask, size_t cap_blocks) {
    if (!x) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (!d_power && !d_mask) {
        x->cap_p = nullptr; x->cap_m = nullptr; x->cap_blocks = 0;
        return GM_OK;
    }
    if (!x->block_adapt) return set_err(GM_ERR_INVALID_ARG, "a capture needs the block-adapt mode on");
    x->cap_p = d_power; x->cap_m = d_mask; x->cap_blocks = cap_blocks;
    return GM_OK;
}

int gm_excisor_process(gm_excisor* x, const void* in, int fmt, size_t n_in, gm_c32* out, size_t out_cap, size_t* n_out) {
    uint64_t cnt = 0;
    if (int rc = stage_check_call(x, excisor_count, excisor_fmt_err(fmt), in, n_in, out, out_cap, "gm_excisor_plan", &cnt)) return rc;
    return stage_process(x, in, n_in * (fmt == GM_FMT_C32 ? 8 : 2), out, cnt, n_out, [&](hipStream_t st, const void* d_in, cf* d_out) {
        return excisor_launch(x, st, d_in, fmt, n_in, d_out, 0, ~0ull, cnt);
    });
}

int gm_excisor_synchronize(gm_excisor* x) { return stage_synchronize(x); }

}  // extern "C"

// ====================================================================== the chain of optional stages behind a ring writer's head stage
// head stage (front-end kernel or down-converter: the caller's part) -> a linear buffer -> (excisor) -> (resampler) -> the ring at
// write_pos; ring indices count the LAST stage's outputs.  Either handle may be null.

// `n` samples leave the head stage in this call: *total of them reach the ring — or a stage's stream would pass 2^62
static int chain_count(const gm_excisor* x, const gm_resampler* rs, uint64_t n, uint64_t* total) {
    if (x) {
        if (x->base + x->inputs + n > RS_INDEX_MAX) return set_err(GM_ERR_INVALID_ARG, "at most 2^62 samples a stream");
        n = excisor_count(x, n);
    }
    if (rs) {
        if (rs->base + rs->inputs + n > RS_INDEX_MAX) return set_err(GM_ERR_INVALID_ARG, "at most 2^62 samples a stream");
        n = resampler_count(rs, n);
    }
    *total = n;
    return GM_OK;
}
// before a call's first block: the excisor's linear output in front of a resampler, and the histories the stages' last calls wrote
static int chain_begin(gm_excisor* x, gm_resampler* rs, hipStream_t st) {
    if (x && rs && !x->d_mid) HIPC(hipMalloc(reinterpret_cast<void**>(&x->d_mid), (gm_ring::SLOT_SAMPLES_MAX + gm::EX_BLOCK_MAX) * sizeof(cf)));   // a block's outputs: up to its inputs + H
    if (x) if (int rc = stage_join(x, st)) return rc;
    if (rs) if (int rc = stage_join(rs, st)) return rc;
    return GM_OK;
}
// One block's launches on fe_stream: the head stage has left `n` samples in `lin`; *cnt of them reach the ring.  A stage with no input
// is not launched (an excisor delivers nothing until it has seen a whole segment), and the head then does not move.  One buffer of each
// kind serves every block: the stream runs block k's kernels before block k + 1's first kernel.
static int chain_launch(gm_excisor* x, gm_resampler* rs, gm_ring* r, const cf* lin, uint64_t n, uint64_t* cnt) {
    if (x && n) {
        const uint64_t n_in = n;
        n = excisor_count(x, n_in);
        if (int rc = excisor_launch(x, r->fe_stream, lin, GM_FMT_C32, n_in, rs ? x->d_mid : r->d_buf, rs ? 0 : r->write_pos, rs ? ~0ull : r->mask, n)) return rc;
        lin = x->d_mid;
    }
    if (rs && n) {
        const uint64_t n_in = n;
        n = resampler_count(rs, n_in);
        if (int rc = resampler_launch(rs, r->fe_stream, lin, GM_FMT_C32, n_in, r->d_buf, r->write_pos, r->mask, n)) return rc;
    }
    *cnt = n;
    return GM_OK;
}

// gm_frontend_write_ring with the chain behind the front-end kernel, whose linear output lands in the scratch buffer of the chain's first stage
static int frontend_write_ring_chain(gm_frontend* f, gm_excisor* x, gm_resampler* rs, gm_ring* r, const void* samples, size_t n_samples, int fmt,
                                     uint64_t* n_out_total, const char* devices_err) {
    if (!f || !r || (!samples && n_samples)) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (fmt != GM_FMT_C32 && fmt != GM_FMT_I8_IQ) return set_err(GM_ERR_INVALID_ARG, "front-end input is c32 or int8 IQ");
    if (f->device != r->device || (x && x->device != r->device) || (rs && rs->device != r->device)) return set_err(GM_ERR_INVALID_ARG, devices_err);
    uint64_t total = 0;
    if (int rc = chain_count(x, rs, n_samples, &total)) return rc;
    if (total > r->size) return set_err(GM_ERR_OUT_OF_RANGE, "write larger than the ring");
    if (n_out_total) *n_out_total = total;
    if (int rc = ensure_device(r->device)) return rc;
    if (int rc = ring_async_init(r)) return rc;
    if (int rc = ring_fe_init(r)) return rc;
    cf*& lin = x ? x->d_scratch : rs->d_scratch;
    if (!lin) HIPC(hipMalloc(reinterpret_cast<void**>(&lin), gm_ring::SLOT_SAMPLES_MAX * sizeof(cf)));
    if (int rc = chain_begin(x, rs, r->fe_stream)) return rc;
    return ring_write_blocks(r, samples, n_samples, fmt == GM_FMT_C32 ? 8 : 2, r->slot_samples, f->d_raw, gm_ring::SLOT_SAMPLES_MAX * 8,
                             [&](const void* d_raw, size_t chunk, uint64_t* cnt) {
                                 if (int rc = frontend_launch(f, r->fe_stream, d_raw, fmt, lin, 0, ~0ull, chunk)) return rc;
                                 return chain_launch(x, rs, r, lin, chunk, cnt);
                             });
}

extern "C" {

int gm_frontend_write_ring_resampled(gm_frontend* f, gm_resampler* rs, gm_ring* r, const void* samples, size_t n_samples, int fmt,
                                     uint64_t* n_out_total) {
    if (!rs) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    return frontend_write_ring_chain(f, nullptr, rs, r, samples, n_samples, fmt, n_out_total, "front-end, resampler and ring live on different devices");
}

int gm_frontend_write_ring_conditioned(gm_frontend* f, gm_excisor* x, gm_resampler* rs, gm_ring* r, const void* samples, size_t n_samples,
                                       int fmt, uint64_t* n_out_total) {
    if (!x) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    return frontend_write_ring_chain(f, x, rs, r, samples, n_samples, fmt, n_out_total,
                                     "front-end, excisor, resampler and ring live on different devices");
}

}  // extern "C"

// ====================================================================== real-IF down-conversion (gm_ddc)
// gnss_mi355x.h states the definition; tests/ddc_model.py restates it.  The filter is the resampler's: its rules, its table, its counts.
namespace {
struct DdcPlan {
    ResamplerPlan rs;
    uint64_t inc = 0;
};

int ddc_rules(const gm_ddc_cfg* c, DdcPlan& p) {
    if (!c) return set_err(GM_ERR_INVALID_ARG, "null cfg");
    if (!std::isfinite(c->mix_cycles_per_sample)) return set_err(GM_ERR_INVALID_ARG, "mix_cycles_per_sample must be finite");
    const gm_resampler_cfg rc{c->up, c->down, c->taps, c->n_phases, c->cutoff, c->kaiser_beta, c->blank_threshold, c->reserved};
    if (int rc2 = resampler_rules(&rc, p.rs)) return rc2;
    const double frac = c->mix_cycles_per_sample - floor(c->mix_cycles_per_sample);      // [0, 1]: 1 only when a tiny negative value rounds up
    p.inc = frac < 1.0 ? uint64_t(floor(ldexp(frac, 64))) : 0;                            // exact: a scaling by 2^64 loses nothing; 2^64 wraps to 0
    return GM_OK;
}

// Whi[h] = exp(-j 2 pi h / 2^12), Wlo[l] = exp(-j 2 pi l / 2^24): the f64 value rounded once (either pointer may be null)
void ddc_phasor_tables(cf* whi, cf* wlo) {
    const double PI = 3.14159265358979323846;
    for (int i = 0; i < gm::DDC_TABLE; ++i) {
        const double ah = 2.0 * PI * double(i) / 4096.0, al = 2.0 * PI * double(i) / 16777216.0;
        if (whi) { whi[i].x = float(cos(ah)); whi[i].y = float(0.0 - sin(ah)); }       // (0.0 - 0.0: no negative zero in word 0)
        if (wlo) { wlo[i].x = float(cos(al)); wlo[i].y = float(0.0 - sin(al)); }
    }
}
}  // namespace

struct gm_ddc : StreamStage {               // history: the last T blanked input bytes (int8)
    DdcPlan plan;
    std::vector<float> table;               // [PHI + 1][T]
    std::vector<cf> whi, wlo;               // [DDC_TABLE] each
    float* d_table = nullptr;
    cf *d_whi = nullptr, *d_wlo = nullptr;
    void* d_raw[gm_ring::SLOTS] = {nullptr, nullptr, nullptr, nullptr};   // gm_ddc_write_ring: the landing zones of the raw bytes
    cf* d_scratch = nullptr;                // gm_ddc_write_ring: the linear output in front of an excisor or a resampler (SLOT_SAMPLES_MAX samples)
};

static uint64_t ddc_count(const gm_ddc* d, uint64_t n_in) {
    const uint64_t A = d->base + d->inputs;
    return resampler_total_out(d->plan.rs, A + n_in) - resampler_total_out(d->plan.rs, A);
}
// one call's kernels on `st`, outputs to out[(out_start + k) & out_mask]; the caller has checked every argument; n_in > 0
static int ddc_launch(gm_ddc* d, hipStream_t st, const void* d_in, uint64_t n_in, cf* out, uint64_t out_start, uint64_t out_mask,
                      uint64_t n_out) {
    const ResamplerPlan& p = d->plan.rs;
    const uint64_t A = d->base + d->inputs, m0 = resampler_total_out(p, A);
    gm::DdcArgs a{};
    a.in = static_cast<const int8_t*>(d_in); a.n_in = n_in;
    a.hist_in = static_cast<const int8_t*>(d->d_hist[d->cur]); a.hist_out = static_cast<int8_t*>(d->d_hist[d->cur ^ 1]);
    a.table = d->d_table; a.whi = d->d_whi; a.wlo = d->d_wlo;
    a.T = p.T; a.PHI = p.PHI; a.up = p.up; a.down = p.down;
    a.a0 = m0 / p.up; a.mr0 = m0 % p.up; a.in_index = A; a.inc = d->plan.inc;
    a.n_out = n_out; a.tile_out = gm::resample_tile_out(p.T, p.up, p.down);
    a.out = out; a.out_start = out_start; a.out_mask = out_mask;
    a.thr2 = p.thr * p.thr; a.blank = p.thr > 0.0f ? 1 : 0;
    a.blanked = d->d_blanked;
    gm::launch_ddc(st, a);
    return stage_launched(d, st, n_in, n_out);
}

extern "C" {

int gm_ddc_plan(const gm_ddc_cfg* cfg, uint64_t inputs_so_far, uint64_t n_in, uint32_t* up_reduced, uint32_t* down_reduced,
                uint32_t* taps, uint32_t* n_phases, uint64_t* phase_inc, uint64_t* n_out) {
    DdcPlan p;
    if (int rc = ddc_rules(cfg, p)) return rc;
    if (int rc = stage_check_span(inputs_so_far, n_in)) return rc;
    if (up_reduced) *up_reduced = p.rs.up;
    if (down_reduced) *down_reduced = p.rs.down;
    if (taps) *taps = p.rs.T;
    if (n_phases) *n_phases = p.rs.PHI;
    if (phase_inc) *phase_inc = p.inc;
    if (n_out) *n_out = resampler_total_out(p.rs, inputs_so_far + n_in) - resampler_total_out(p.rs, inputs_so_far);
    return GM_OK;
}

int gm_ddc_create(const gm_ddc_cfg* cfg, gm_ddc** out) {
    if (!out) return set_err(GM_ERR_INVALID_ARG, "null out");
    *out = nullptr;
    DdcPlan p;
    if (int rc = ddc_rules(cfg, p)) return rc;
    if (int rc = ensure_device(g_device)) return rc;
    gm_ddc* d = new gm_ddc;
    d->device = g_device; d->plan = p;
    d->table.resize(size_t(p.rs.PHI + 1) * p.rs.T);
    resampler_design(p.rs, d->table.data());
    d->whi.resize(gm::DDC_TABLE); d->wlo.resize(gm::DDC_TABLE);
    ddc_phasor_tables(d->whi.data(), d->wlo.data());
    const size_t wbytes = gm::DDC_TABLE * sizeof(cf);
    hipError_t e = hipMalloc(&d->d_table, d->table.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(d->d_table, d->table.data(), d->table.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d->d_whi), wbytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d->d_wlo), wbytes);
    if (e == hipSuccess) e = hipMemcpy(d->d_whi, d->whi.data(), wbytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d->d_wlo, d->wlo.data(), wbytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = stage_create(d, p.rs.T);
    if (e != hipSuccess) { gm_ddc_destroy(d); return hip_fail(e, "gm_ddc_create"); }
    *out = d;
    return GM_OK;
}

int gm_ddc_destroy(gm_ddc* d) {
    if (!d) return GM_OK;
    stage_destroy(d);
    hipFree(d->d_table); hipFree(d->d_whi); hipFree(d->d_wlo); hipFree(d->d_scratch);
    for (void* p : d->d_raw) hipFree(p);
    delete d;
    return GM_OK;
}

int gm_ddc_reset(gm_ddc* d, uint64_t input_index) {
    return stage_reset(d, input_index, [] { return hipSuccess; });
}

int gm_ddc_stats(gm_ddc* d, uint64_t* inputs, uint64_t* outputs, uint64_t* blanked) {
    return stage_stats(d, inputs, outputs, blanked);
}

int gm_ddc_synchronize(gm_ddc* d) { return stage_synchronize(d); }

int gm_ddc_tables(gm_ddc* d, float* table, gm_c32* whi, gm_c32* wlo) {
    if (!d && table) return set_err(GM_ERR_INVALID_ARG, "the filter table needs a handle");
    if (!d) {                 // the phasor tables are the same for every handle: a null handle gives them without a device
        ddc_phasor_tables(reinterpret_cast<cf*>(whi), reinterpret_cast<cf*>(wlo));
        return GM_OK;
    }
    if (table) memcpy(table, d->table.data(), d->table.size() * sizeof(float));
    if (whi) memcpy(whi, d->whi.data(), gm::DDC_TABLE * sizeof(cf));
    if (wlo) memcpy(wlo, d->wlo.data(), gm::DDC_TABLE * sizeof(cf));
    return GM_OK;
}

int gm_ddc_process_dev(gm_ddc* d, const void* d_in, size_t n_in, void* d_out, size_t out_cap, size_t* n_out, void* stream) {
    uint64_t cnt = 0;
    if (int rc = stage_check_call(d, ddc_count, nullptr, d_in, n_in, d_out, out_cap, "gm_ddc_plan", &cnt)) return rc;
    if (int rc = stage_check_overlap(d_in, n_in, d_out, cnt)) return rc;
    if (n_out) *n_out = size_t(cnt);
    if (!n_in) return GM_OK;
    if (int rc = ensure_device(d->device)) return rc;
    return ddc_launch(d, stream ? static_cast<hipStream_t>(stream) : d->stream, d_in, n_in, static_cast<cf*>(d_out), 0, ~0ull, cnt);
}

int gm_ddc_process(gm_ddc* d, const int8_t* in, size_t n_in, gm_c32* out, size_t out_cap, size_t* n_out) {
    uint64_t cnt = 0;
    if (int rc = stage_check_call(d, ddc_count, nullptr, in, n_in, out, out_cap, "gm_ddc_plan", &cnt)) return rc;
    return stage_process(d, in, n_in, out, cnt, n_out, [&](hipStream_t st, const void* d_in, cf* d_out) {
        return ddc_launch(d, st, d_in, n_in, d_out, 0, ~0ull, cnt);
    });
}

// The ring writer with the down-converter as the head stage: raw bytes -> down-converter -> the chain of optional stages (through
// d_scratch) or, with neither, the ring at write_pos
int gm_ddc_write_ring(gm_ddc* d, gm_excisor* x, gm_resampler* rs, gm_ring* r, const int8_t* samples, size_t n_samples,
                      uint64_t* n_out_total) {
    if (!d || !r || (!samples && n_samples)) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (d->device != r->device || (x && x->device != r->device) || (rs && rs->device != r->device))
        return set_err(GM_ERR_INVALID_ARG, "down-converter, excisor, resampler and ring live on different devices");
    if (d->base + d->inputs + n_samples > RS_INDEX_MAX) return set_err(GM_ERR_INVALID_ARG, "at most 2^62 samples a stream");
    uint64_t total = 0;
    if (int rc = chain_count(x, rs, ddc_count(d, n_samples), &total)) return rc;
    if (total > r->size) return set_err(GM_ERR_OUT_OF_RANGE, "write larger than the ring");
    if (n_out_total) *n_out_total = total;
    if (int rc = ensure_device(r->device)) return rc;
    if (int rc = ring_async_init(r)) return rc;
    if (int rc = ring_fe_init(r)) return rc;
    const bool chained = x || rs;
    if (chained && !d->d_scratch) HIPC(hipMalloc(reinterpret_cast<void**>(&d->d_scratch), gm_ring::SLOT_SAMPLES_MAX * sizeof(cf)));
    if (int rc = stage_join(d, r->fe_stream)) return rc;
    if (int rc = chain_begin(x, rs, r->fe_stream)) return rc;
    // a block is at most the ring's staging slot, and, where the down-converter raises the rate, short enough that its outputs fit the
    // linear buffers (a call delivers at most n * up / down + 1)
    const ResamplerPlan& p = d->plan.rs;
    size_t block = r->slot_samples;
    if (p.up > p.down) block = std::min<size_t>(block, size_t((gm_ring::SLOT_SAMPLES_MAX - 1) * uint64_t(p.down) / p.up));
    return ring_write_blocks(r, samples, n_samples, 1, block, d->d_raw, gm_ring::SLOT_SAMPLES_MAX, [&](const void* d_raw, size_t chunk, uint64_t* cnt) {
        *cnt = ddc_count(d, chunk);
        if (!chained) return ddc_launch(d, r->fe_stream, d_raw, chunk, r->d_buf, r->write_pos, r->mask, *cnt);
        if (int rc = ddc_launch(d, r->fe_stream, d_raw, chunk, d->d_scratch, 0, ~0ull, *cnt)) return rc;
        return chain_launch(x, rs, r, d->d_scratch, *cnt, cnt);
    });
}

}  // extern "C"

// ====================================================================== polyphase filter bank (gm_channelizer)
// gnss_mi355x.h states the definition; tests/channelizer_model.py restates it in float64.
namespace {
struct ChannelizerPlan {
    uint32_t M = 0, D = 0, P = 0, L = 0, C = 0;
    uint32_t channels[gm::CH_M_MAX] = {};
    double cutoff = 0.9, beta = 8.0;
    float thr = 0.0f;
};

int channelizer_rules(const gm_channelizer_cfg* c, ChannelizerPlan& p) {
    if (!c) return set_err(GM_ERR_INVALID_ARG, "null cfg");
    if (c->reserved) return set_err(GM_ERR_INVALID_ARG, "gm_channelizer_cfg.reserved must be 0");
    const uint32_t M = c->n_channels;
    if (M != 4 && M != 8 && M != 16 && M != 32 && M != 64) return set_err(GM_ERR_INVALID_ARG, "n_channels: 4, 8, 16, 32 or 64");
    if (c->decim < 1 || c->decim > M) return set_err(GM_ERR_INVALID_ARG, "decim: 1 .. n_channels");
    if (c->taps_per_branch && (c->taps_per_branch < 2 || c->taps_per_branch > 32)) return set_err(GM_ERR_INVALID_ARG, "taps_per_branch: 2 .. 32, 0 for the default");
    if (!std::isfinite(c->cutoff) || !std::isfinite(c->kaiser_beta) || !std::isfinite(c->blank_threshold))
        return set_err(GM_ERR_INVALID_ARG, "cutoff, kaiser_beta and blank_threshold must be finite");
    if (!(c->cutoff >= 0.0f && c->cutoff <= 1.0f)) return set_err(GM_ERR_INVALID_ARG, "cutoff: (0, 1], 0 for the default");
    if (!(c->kaiser_beta >= 0.0f && c->kaiser_beta <= 20.0f)) return set_err(GM_ERR_INVALID_ARG, "kaiser_beta: [0, 20]");
    if (!(c->blank_threshold >= 0.0f)) return set_err(GM_ERR_INVALID_ARG, "blank_threshold: >= 0");
    p.M = M; p.D = c->decim; p.P = c->taps_per_branch ? c->taps_per_branch : 16; p.L = p.M * p.P;
    if (c->n_out_channels == 0) {
        if (c->out_channels) return set_err(GM_ERR_INVALID_ARG, "out_channels without n_out_channels");
        p.C = M;
        for (uint32_t k = 0; k < M; ++k) p.channels[k] = k;
    } else {
        if (c->n_out_channels > M || !c->out_channels) return set_err(GM_ERR_INVALID_ARG, "n_out_channels: at most n_channels, with the list");
        uint64_t seen = 0;
        for (uint32_t i = 0; i < c->n_out_channels; ++i) {
            const uint32_t k = c->out_channels[i];
            if (k >= M) return set_err(GM_ERR_INVALID_ARG, "out_channels: an index outside 0 .. n_channels - 1");
            if (seen >> k & 1) return set_err(GM_ERR_INVALID_ARG, "out_channels: an index listed twice");
            seen |= 1ull << k;
            p.channels[i] = k;
        }
        p.C = c->n_out_channels;
    }
    p.cutoff = c->cutoff == 0.0f ? 0.9 : double(c->cutoff);
    p.beta = c->kaiser_beta == 0.0f ? 8.0 : double(c->kaiser_beta);
    p.thr = c->blank_threshold;
    return GM_OK;
}

// total_out(A) = max(0, ceil((A - L/2) / D))
uint64_t channelizer_total_out(const ChannelizerPlan& p, uint64_t A) {
    const uint64_t half = p.L / 2;
    return A <= half ? 0 : (A - half + p.D - 1) / p.D;
}

void channelizer_design(const ChannelizerPlan& p, float* g) {
    const double PI = 3.14159265358979323846;
    const double fc = p.cutoff / double(p.D), inv_i0 = 1.0 / bessel_i0(p.beta), halfL = 0.5 * double(p.L);
    std::vector<double> h(p.L);
    double sum = 0.0;
    for (uint32_t j = 0; j < p.L; ++j) {
        const double t = double(j) - (halfL - 1.0);
        const double u = t / halfL, w = 1.0 - u * u, x = fc * t;
        const double sinc = x == 0.0 ? 1.0 : sin(PI * x) / (PI * x);
        h[j] = fc * sinc * bessel_i0(p.beta * sqrt(w > 0.0 ? w : 0.0)) * inv_i0;      // |t| <= L/2 for every j
        sum += h[j];
    }
    for (uint32_t j = 0; j < p.L; ++j) g[j] = float(h[j] / sum);
}
}  // namespace

struct gm_channelizer : StreamStage {       // history: the last L blanked inputs (cf)
    ChannelizerPlan plan;
    std::vector<float> taps;                // [L]
    float* d_taps = nullptr;
    cf* d_rot = nullptr;                    // [M] exp(-j 2 pi e / M)
};

// one call's kernels on `st`, plane i to out + i * out_stride; the caller has checked every argument; n_in > 0
static int channelizer_launch(gm_channelizer* c, hipStream_t st, const void* d_in, int fmt, uint64_t n_in, cf* out, uint64_t out_stride,
                              uint64_t n_out) {
    const ChannelizerPlan& p = c->plan;
    const uint64_t A = c->base + c->inputs;
    gm::ChannelizerArgs a{};
    a.in = d_in; a.n_in = n_in;
    a.hist_in = static_cast<const cf*>(c->d_hist[c->cur]); a.hist_out = static_cast<cf*>(c->d_hist[c->cur ^ 1]);
    a.taps = c->d_taps; a.rot = c->d_rot;
    a.M = p.M; a.D = p.D; a.P = p.P; a.L = p.L;
    a.m0 = channelizer_total_out(p, A); a.in_index = A;
    a.n_out = n_out; a.tile_out = gm::channelizer_tile_out(p.L, p.D);
    a.pad_shift = p.D % 64 == 0 ? 6 : 5;
    a.out = out; a.out_stride = out_stride;
    for (int k = 0; k < gm::CH_M_MAX; ++k) a.plane_of[k] = -1;
    for (uint32_t i = 0; i < p.C; ++i) a.plane_of[p.channels[i]] = int8_t(i);
    a.thr2 = p.thr * p.thr; a.blank = p.thr > 0.0f ? 1 : 0;
    a.blanked = c->d_blanked;
    gm::launch_channelizer(st, a, fmt);
    return stage_launched(c, st, n_in, n_out);
}
static uint64_t channelizer_count(const gm_channelizer* c, uint64_t n_in) {
    const uint64_t A = c->base + c->inputs;
    return channelizer_total_out(c->plan, A + n_in) - channelizer_total_out(c->plan, A);
}
static const char* channelizer_fmt_err(int fmt) {
    return fmt != GM_FMT_C32 && fmt != GM_FMT_I8_IQ ? "channelizer input is c32 or int8 IQ (a real stream takes a gm_ddc in front)" : nullptr;
}

extern "C" {

int gm_channelizer_plan(const gm_channelizer_cfg* cfg, uint64_t inputs_so_far, uint64_t n_in, uint32_t* n_out_channels,
                        uint32_t* taps_per_branch, uint32_t* n_taps, uint64_t* n_out) {
    ChannelizerPlan p;
    if (int rc = channelizer_rules(cfg, p)) return rc;
    if (int rc = stage_check_span(inputs_so_far, n_in)) return rc;
    if (n_out_channels) *n_out_channels = p.C;
    if (taps_per_branch) *taps_per_branch = p.P;
    if (n_taps) *n_taps = p.L;
    if (n_out) *n_out = channelizer_total_out(p, inputs_so_far + n_in) - channelizer_total_out(p, inputs_so_far);
    return GM_OK;
}

int gm_channelizer_design(const gm_channelizer_cfg* cfg, float* taps) {
    ChannelizerPlan p;
    if (int rc = channelizer_rules(cfg, p)) return rc;
    if (!taps) return set_err(GM_ERR_INVALID_ARG, "null taps");
    channelizer_design(p, taps);
    return GM_OK;
}

int gm_channelizer_create(const gm_channelizer_cfg* cfg, gm_channelizer** out) {
    if (!out) return set_err(GM_ERR_INVALID_ARG, "null out");
    *out = nullptr;
    ChannelizerPlan p;
    if (int rc = channelizer_rules(cfg, p)) return rc;
    if (int rc = ensure_device(g_device)) return rc;
    gm_channelizer* c = new gm_channelizer;
    c->device = g_device; c->plan = p;
    c->taps.resize(p.L);
    channelizer_design(p, c->taps.data());
    std::vector<cf> rot(p.M);
    for (uint32_t e = 0; e < p.M; ++e) {
        const gm::ct::cs v = gm::ct::cossin2pi(long(e), long(p.M));
        rot[e] = gm::cf_make(float(v.c), float(-v.s));
    }
    hipError_t e = hipMalloc(&c->d_taps, p.L * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(c->d_taps, c->taps.data(), p.L * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&c->d_rot), p.M * sizeof(cf));
    if (e == hipSuccess) e = hipMemcpy(c->d_rot, rot.data(), p.M * sizeof(cf), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = stage_create(c, size_t(p.L) * sizeof(cf));
    if (e != hipSuccess) { gm_channelizer_destroy(c); return hip_fail(e, "gm_channelizer_create"); }
    *out = c;
    return GM_OK;
}

int gm_channelizer_destroy(gm_channelizer* c) {
    if (!c) return GM_OK;
    stage_destroy(c);
    hipFree(c->d_taps); hipFree(c->d_rot);
    delete c;
    return GM_OK;
}

int gm_channelizer_reset(gm_channelizer* c, uint64_t input_index) {
    return stage_reset(c, input_index, [] { return hipSuccess; });
}

int gm_channelizer_taps(gm_channelizer* c, float* taps) {
    if (!c || !taps) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    memcpy(taps, c->taps.data(), c->taps.size() * sizeof(float));
    return GM_OK;
}

int gm_channelizer_stats(gm_channelizer* c, uint64_t* inputs, uint64_t* outputs, uint64_t* blanked) {
    return stage_stats(c, inputs, outputs, blanked);
}

int gm_channelizer_process_dev(gm_channelizer* c, const void* d_in, int fmt, size_t n_in, void* d_out, size_t out_stride, size_t out_cap,
                               size_t* n_out, void* stream) {
    uint64_t cnt = 0;
    if (int rc = stage_check_call(c, channelizer_count, channelizer_fmt_err(fmt), d_in, n_in, d_out, out_cap, "gm_channelizer_plan", &cnt)) return rc;
    if (out_stride < out_cap) return set_err(GM_ERR_OUT_OF_RANGE, "out_stride below out_cap");
    if (cnt)
        if (int rc = stage_check_overlap(d_in, n_in * (fmt == GM_FMT_C32 ? 8 : 2), d_out, uint64_t(c->plan.C) * out_stride)) return rc;
    if (n_out) *n_out = size_t(cnt);
    if (!n_in) return GM_OK;
    if (int rc = ensure_device(c->device)) return rc;
    return channelizer_launch(c, stream ? static_cast<hipStream_t>(stream) : c->stream, d_in, fmt, n_in, static_cast<cf*>(d_out), out_stride, cnt);
}

int gm_channelizer_process(gm_channelizer* c, const void* in, int fmt, size_t n_in, gm_c32* out, size_t out_cap, size_t* n_out) {
    uint64_t cnt = 0;
    if (int rc = stage_check_call(c, channelizer_count, channelizer_fmt_err(fmt), in, n_in, out, out_cap, "gm_channelizer_plan", &cnt)) return rc;
    return stage_process(c, in, n_in * (fmt == GM_FMT_C32 ? 8 : 2), out, cnt, n_out, [&](hipStream_t st, const void* d_in, cf* d_out) {
        return channelizer_launch(c, st, d_in, fmt, n_in, d_out, cnt, cnt);
    }, c->plan.C, out_cap);
}

int gm_channelizer_synchronize(gm_channelizer* c) { return stage_synchronize(c); }

// The GLONASS L1OF ranging code: nine stages, all ones; each clock the output is stage 7, then stage 5 xor stage 9 enters stage 1
int gm_glonass_code(int8_t* out) {
    if (!out) return set_err(GM_ERR_INVALID_ARG, "null out");
    unsigned s[10];
    for (int i = 1; i <= 9; ++i) s[i] = 1;
    for (int n = 0; n < 511; ++n) {
        out[n] = s[7] ? -1 : 1;              // +1 stands for logic 0
        const unsigned in = s[5] ^ s[9];
        for (int i = 9; i > 1; --i) s[i] = s[i - 1];
        s[1] = in;
    }
    return GM_OK;
}

}  // extern "C"

// ====================================================================== antenna-array stages: what gm_nuller, gm_stap and gm_beamformer share
// A stream of time samples of A interleaved elements, cut into blocks of B: total_out(T) = B * (T div B).  Per finished block the kernels
// form a matrix R (r_words) and weights w (w_words: a row per output plane), which a call can hand back: process_dev to the device
// buffers the caller armed with *_capture, process to host arrays through the handle's own d_blk.  A handle derives from ArrayStage, sets
// these numbers in its create (array_shape) and supplies `*_launch(handle, stream, d_in, fmt, n_in, out, out_stride, n_out, cap_R, cap_w)`:
// its kernels' argument block, the shared fields filled by array_fill_args.
namespace {
struct ArrayStage : StreamStage {
    std::string fmt_err, plan_entry;        // the format verdict; the entry that gives the output count
    uint32_t A = 0, B = 0;                  // elements per time sample; time samples per block
    size_t r_words = 0, w_words = 0;        // words of R and of w per block
    uint32_t planes = 1;                    // output planes (the rows of w)
    float loading = 0.0f;
    bool fixed = false;                     // static mode
    cf* cap_R = nullptr; cf* cap_w = nullptr; size_t cap_blocks = 0;     // the caller's capture (device)
    cf* d_blk = nullptr; size_t blk_cap = 0;                             // blocks; the host-buffer entry's own capture: [blk_cap][r_words] then [blk_cap][w_words]
};

void array_shape(ArrayStage* n, const char* name, uint32_t A, uint32_t B, float loading, size_t r_words, size_t w_words, uint32_t planes = 1) {
    n->fmt_err = std::string(name) + " input is interleaved c32 or int8 IQ";
    n->plan_entry = std::string("gm_") + name + "_plan";
    n->A = A; n->B = B; n->loading = loading; n->r_words = r_words; n->w_words = w_words; n->planes = planes;
}
void array_destroy(ArrayStage* n) {
    stage_destroy(n);
    hipFree(n->d_blk);
}

// ---- the argument rules
bool array_finite(const gm_c32* v, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i].re) || !std::isfinite(v[i].im)) return false;
    return true;
}
// the block length (0: 1024) and the diagonal loading (0: 1e-4)
int array_block_rules(uint32_t block, float loading, uint32_t* B, float* resolved) {
    *B = block ? block : 1024;
    if (*B < 256 || *B > 16384 || (*B & (*B - 1))) return set_err(GM_ERR_INVALID_ARG, "block: a power of two in 256 .. 16384, 0 for the default");
    if (!std::isfinite(loading)) return set_err(GM_ERR_INVALID_ARG, "loading must be finite");
    if (loading != 0.0f && !(loading >= 1e-6f && loading <= 1.0f)) return set_err(GM_ERR_INVALID_ARG, "loading: [1e-6, 1], 0 for the default");
    *resolved = loading == 0.0f ? 1e-4f : loading;
    return GM_OK;
}
// one steering row: n finite words, not all zero (`zero_err`: the entry's words for that)
int array_row_rules(const gm_c32* s, uint32_t n, const char* zero_err) {
    if (!array_finite(s, n)) return set_err(GM_ERR_INVALID_ARG, "steering must be finite");
    bool any = false;
    for (uint32_t i = 0; i < n; ++i) any = any || s[i].re != 0.0f || s[i].im != 0.0f;
    if (!any) return set_err(GM_ERR_INVALID_ARG, zero_err);
    return GM_OK;
}
// gm_nuller's and gm_stap's steering vector of n words: e_0 where the cfg has none
int array_steering_rules(const gm_c32* s, uint32_t n, cf* dst, uint32_t dst_words) {
    for (uint32_t i = 0; i < dst_words; ++i) dst[i] = gm::cf_make(i == 0 ? 1.0f : 0.0f, 0.0f);
    if (!s) return GM_OK;
    if (int rc = array_row_rules(s, n, "steering is all zero")) return rc;
    for (uint32_t i = 0; i < n; ++i) dst[i] = gm::cf_make(s[i].re, s[i].im);
    return GM_OK;
}

// ---- the counts
// total_out(T) = B * (T div B)
uint64_t array_total_out(uint32_t B, uint64_t T) { return T / B * B; }
uint64_t array_count(const ArrayStage* n, uint64_t n_in) {
    const uint64_t T = n->base + n->inputs;
    return array_total_out(n->B, T + n_in) - array_total_out(n->B, T);
}
// the gm_*_plan entries behind their rules
int array_plan(uint32_t B, float resolved, uint64_t inputs_so_far, uint64_t n_in, uint32_t* block, float* loading, uint64_t* n_out) {
    if (int rc = stage_check_span(inputs_so_far, n_in)) return rc;
    if (block) *block = B;
    if (loading) *loading = resolved;
    if (n_out) *n_out = array_total_out(B, inputs_so_far + n_in) - array_total_out(B, inputs_so_far);
    return GM_OK;
}
int array_stats(ArrayStage* n, uint64_t* inputs, uint64_t* outputs, uint64_t* blocks, uint64_t* blanked) {
    if (int rc = stage_stats(n, inputs, outputs, blanked)) return rc;
    if (blocks) *blocks = n->outputs / n->B;
    return GM_OK;
}

// ---- a call
// the fields that NullerArgs, StapArgs and BeamArgs have in common
template <class Args>
void array_fill_args(Args& a, const ArrayStage* n, const void* d_in, uint64_t n_in, cf* out, uint64_t n_out, cf* cap_R, cf* cap_w) {
    const uint64_t T = n->base + n->inputs;
    a.in = d_in; a.n_in = n_in;
    a.hist_in = static_cast<const cf*>(n->d_hist[n->cur]); a.hist_out = static_cast<cf*>(n->d_hist[n->cur ^ 1]);
    a.A = n->A; a.B = n->B;
    a.pending = uint32_t(T % n->B); a.pending_out = uint32_t((T + n_in) % n->B);
    a.n_blocks = n_out / n->B;
    a.out = out; a.cap_R = cap_R; a.cap_w = cap_w;
    a.loading = n->loading; a.adaptive = n->fixed ? 0 : 1;
}
int array_check_call(const ArrayStage* n, int fmt, const void* in, size_t n_in, const void* out, size_t out_cap, uint64_t* cnt) {
    if (!n) return set_err(GM_ERR_INVALID_ARG, "null handle");
    const char* fmt_err = fmt != GM_FMT_C32 && fmt != GM_FMT_I8_IQ ? n->fmt_err.c_str() : nullptr;
    return stage_check_call(n, array_count, fmt_err, in, n_in, out, out_cap, n->plan_entry.c_str(), cnt);
}
size_t array_in_bytes(const ArrayStage* n, int fmt, size_t n_in) { return n_in * n->A * (fmt == GM_FMT_C32 ? 8 : 2); }

int array_capture(ArrayStage* n, void* d_R, void* d_w, size_t cap_blocks) {
    if (!n) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if ((d_R == nullptr) != (d_w == nullptr)) return set_err(GM_ERR_INVALID_ARG, "d_R and d_w: both or neither");
    if ((d_R == nullptr) != (cap_blocks == 0)) return set_err(GM_ERR_INVALID_ARG, "cap_blocks: 0 exactly where the pointers are null");
    n->cap_R = static_cast<cf*>(d_R); n->cap_w = static_cast<cf*>(d_w); n->cap_blocks = cap_blocks;
    return GM_OK;
}
// the fixed weights of gm_nuller and gm_stap live in the handle (w[w_words]) and travel in the argument block
template <class H>
int array_set_host_weights(H* n, const gm_c32* w) {
    if (!n) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (!w) { n->fixed = false; return GM_OK; }
    if (!array_finite(w, n->w_words)) return set_err(GM_ERR_INVALID_ARG, "weights must be finite");
    for (size_t i = 0; i < n->w_words; ++i) n->w[i] = gm::cf_make(w[i].re, w[i].im);
    n->fixed = true;
    return GM_OK;
}

// The device entries.  Plane p's outputs start at d_out + p * out_cap: a plane's room is its stride, a count above it is out of range,
// and the planes together, (planes - 1) * out_cap + count words, may not lie over the inputs.
template <class H, class Launch>
int array_process_dev(H* n, Launch launch, const void* d_in, int fmt, size_t n_in, void* d_out, size_t out_cap, size_t* n_out, void* stream) {
    uint64_t cnt = 0;
    if (int rc = array_check_call(n, fmt, d_in, n_in, d_out, out_cap, &cnt)) return rc;
    if (n->cap_w && cnt / n->B > n->cap_blocks) return set_err(GM_ERR_OUT_OF_RANGE, "the capture is smaller than the call's blocks");
    if (cnt)
        if (int rc = stage_check_overlap(d_in, array_in_bytes(n, fmt, n_in), d_out, uint64_t(n->planes - 1) * out_cap + cnt)) return rc;
    if (n_out) *n_out = size_t(cnt);
    if (!n_in) return GM_OK;
    if (int rc = ensure_device(n->device)) return rc;
    return launch(n, stream ? static_cast<hipStream_t>(stream) : n->stream, d_in, fmt, n_in, static_cast<cf*>(d_out), out_cap, cnt, n->cap_R, n->cap_w);
}
// The host-buffer entries: R and w (either may be null) take the words of the call's blocks, `cap_blocks` the room in each.  R is not
// written in static mode.  Plane p is delivered at out + p * out_cap.
template <class H, class Launch>
int array_process(H* n, Launch launch, const void* in, int fmt, size_t n_in, gm_c32* out, size_t out_cap, size_t* n_out, gm_c32* R, gm_c32* w,
                  size_t cap_blocks) {
    uint64_t cnt = 0;
    if (int rc = array_check_call(n, fmt, in, n_in, out, out_cap, &cnt)) return rc;
    const uint64_t blocks = cnt / n->B;
    const bool want = (R || w) && blocks;
    if ((R || w) && blocks > cap_blocks) return set_err(GM_ERR_OUT_OF_RANGE, "cap_blocks below the call's blocks");
    if (want && n->blk_cap < blocks) {
        if (int rc = ensure_device(n->device)) return rc;
        if (int rc = stage_sync(n)) return rc;
        hipFree(n->d_blk); n->d_blk = nullptr; n->blk_cap = 0;
        HIPC(hipMalloc(reinterpret_cast<void**>(&n->d_blk), size_t(blocks) * (n->r_words + n->w_words) * sizeof(cf)));
        n->blk_cap = size_t(blocks);
    }
    cf* d_R = want ? n->d_blk : nullptr;
    cf* d_w = want ? n->d_blk + n->blk_cap * n->r_words : nullptr;
    if (int rc = stage_process(n, in, array_in_bytes(n, fmt, n_in), out, cnt, n_out, [&](hipStream_t st, const void* d_in, cf* d_out) {
            return launch(n, st, d_in, fmt, n_in, d_out, cnt, cnt, d_R, d_w);
        }, n->planes, out_cap)) return rc;
    if (want) {      // stage_process has waited for the kernels
        if (R && !n->fixed) HIPC(hipMemcpy(R, d_R, size_t(blocks) * n->r_words * sizeof(cf), hipMemcpyDeviceToHost));
        if (w) HIPC(hipMemcpy(w, d_w, size_t(blocks) * n->w_words * sizeof(cf), hipMemcpyDeviceToHost));
    }
    return GM_OK;
}
}  // namespace

// ====================================================================== adaptive spatial nulling of an antenna array (gm_nuller)
// gnss_mi355x.h states the definition; tests/nuller_model.py restates it in float64.
namespace {
struct NullerPlan {
    uint32_t A = 0, B = 0;
    float loading = 0.0f;
    cf s[gm::NL_A_MAX] = {};
};

int nuller_rules(const gm_nuller_cfg* c, NullerPlan& p) {
    if (!c) return set_err(GM_ERR_INVALID_ARG, "null cfg");
    if (c->reserved) return set_err(GM_ERR_INVALID_ARG, "gm_nuller_cfg.reserved must be 0");
    if (c->n_antennas < 2 || c->n_antennas > uint32_t(gm::NL_A_MAX)) return set_err(GM_ERR_INVALID_ARG, "n_antennas: 2 .. 8");
    if (int rc = array_block_rules(c->block, c->loading, &p.B, &p.loading)) return rc;
    p.A = c->n_antennas;
    return array_steering_rules(c->steering, p.A, p.s, uint32_t(gm::NL_A_MAX));
}
}  // namespace

struct gm_nuller : ArrayStage {             // history: the converted time samples of the unfinished block (cf [B][A]); R is [A][A], w is [A]
    NullerPlan plan;
    cf w[gm::NL_A_MAX] = {};
};

// one call's kernels on `st`; the caller has checked every argument; n_in > 0
static int nuller_launch(gm_nuller* n, hipStream_t st, const void* d_in, int fmt, uint64_t n_in, cf* out, uint64_t, uint64_t n_out, cf* cap_R,
                         cf* cap_w) {
    gm::NullerArgs a{};
    array_fill_args(a, n, d_in, n_in, out, n_out, cap_R, cap_w);
    a.in_wide = reinterpret_cast<uintptr_t>(d_in) % gm::nuller_in_align(n->A, fmt) == 0 ? 1 : 0;
    for (int i = 0; i < gm::NL_A_MAX; ++i) { a.s[i] = n->plan.s[i]; a.w[i] = n->w[i]; }
    gm::launch_nuller(st, a, fmt);
    return stage_launched(n, st, n_in, n_out);
}

extern "C" {

int gm_nuller_plan(const gm_nuller_cfg* cfg, uint64_t inputs_so_far, uint64_t n_in, uint32_t* block, float* loading, uint64_t* n_out) {
    NullerPlan p;
    if (int rc = nuller_rules(cfg, p)) return rc;
    return array_plan(p.B, p.loading, inputs_so_far, n_in, block, loading, n_out);
}

int gm_nuller_create(const gm_nuller_cfg* cfg, gm_nuller** out) {
    if (!out) return set_err(GM_ERR_INVALID_ARG, "null out");
    *out = nullptr;
    NullerPlan p;
    if (int rc = nuller_rules(cfg, p)) return rc;
    if (int rc = ensure_device(g_device)) return rc;
    gm_nuller* n = new gm_nuller;
    n->device = g_device; n->plan = p;
    array_shape(n, "nuller", p.A, p.B, p.loading, size_t(p.A) * p.A, p.A);
    hipError_t e = stage_create(n, size_t(p.B) * p.A * sizeof(cf));
    if (e != hipSuccess) { gm_nuller_destroy(n); return hip_fail(e, "gm_nuller_create"); }
    *out = n;
    return GM_OK;
}

int gm_nuller_destroy(gm_nuller* n) {
    if (!n) return GM_OK;
    array_destroy(n);
    delete n;
    return GM_OK;
}

int gm_nuller_reset(gm_nuller* n, uint64_t input_index) {
    return stage_reset(n, input_index, [] { return hipSuccess; });
}

int gm_nuller_stats(gm_nuller* n, uint64_t* inputs, uint64_t* outputs, uint64_t* blocks) {
    return array_stats(n, inputs, outputs, blocks, nullptr);
}

int gm_nuller_synchronize(gm_nuller* n) { return stage_synchronize(n); }

int gm_nuller_set_weights(gm_nuller* n, const gm_c32* w) { return array_set_host_weights(n, w); }

int gm_nuller_capture(gm_nuller* n, void* d_R, void* d_w, size_t cap_blocks) { return array_capture(n, d_R, d_w, cap_blocks); }

int gm_nuller_process_dev(gm_nuller* n, const void* d_in, int fmt, size_t n_in, void* d_out, size_t out_cap, size_t* n_out, void* stream) {
    return array_process_dev(n, nuller_launch, d_in, fmt, n_in, d_out, out_cap, n_out, stream);
}

int gm_nuller_process(gm_nuller* n, const void* in, int fmt, size_t n_in, gm_c32* out, size_t out_cap, size_t* n_out, gm_c32* R, gm_c32* w,
                      size_t cap_blocks) {
    return array_process(n, nuller_launch, in, fmt, n_in, out, out_cap, n_out, R, w, cap_blocks);
}

}  // extern "C"

// ====================================================================== space-time adaptive nulling, taps on every antenna (gm_stap)
// gnss_mi355x.h states the definition; tests/stap_model.py restates it in float64.
namespace {
struct StapPlan {
    uint32_t A = 0, L = 0, M = 0, B = 0;
    float loading = 0.0f;
    cf s[gm::ST_M_MAX] = {};
};

int stap_rules(const gm_stap_cfg* c, StapPlan& p) {
    if (!c) return set_err(GM_ERR_INVALID_ARG, "null cfg");
    if (c->reserved) return set_err(GM_ERR_INVALID_ARG, "gm_stap_cfg.reserved must be 0");
    if (c->n_antennas < 2 || c->n_antennas > uint32_t(gm::NL_A_MAX)) return set_err(GM_ERR_INVALID_ARG, "n_antennas: 2 .. 8");
    if (c->taps < 1 || c->taps > uint32_t(gm::ST_L_MAX)) return set_err(GM_ERR_INVALID_ARG, "taps: 1 .. 8");
    if (c->n_antennas * c->taps > uint32_t(gm::ST_M_MAX)) return set_err(GM_ERR_INVALID_ARG, "n_antennas * taps: at most 32");
    if (int rc = array_block_rules(c->block, c->loading, &p.B, &p.loading)) return rc;
    p.A = c->n_antennas; p.L = c->taps; p.M = p.A * p.L;
    return array_steering_rules(c->steering, p.M, p.s, uint32_t(gm::ST_M_MAX));
}
// the history both tap stages keep: the L - 1 converted time samples in front of the unfinished block, then that block's (cf [L - 1 + B][A])
size_t stap_hist_bytes(const StapPlan& p) { return (size_t(p.B) + p.L - 1) * p.A * sizeof(cf); }
}  // namespace

struct gm_stap : ArrayStage {               // history: stap_hist_bytes; d_blanked counts the fallback blocks; R is [M][M], w is [M]
    StapPlan plan;
    cf w[gm::ST_M_MAX] = {};
};

// one call's kernels on `st`; the caller has checked every argument; n_in > 0
static int stap_launch(gm_stap* n, hipStream_t st, const void* d_in, int fmt, uint64_t n_in, cf* out, uint64_t, uint64_t n_out, cf* cap_R,
                       cf* cap_w) {
    gm::StapArgs a{};
    array_fill_args(a, n, d_in, n_in, out, n_out, cap_R, cap_w);
    a.fmt = fmt; a.L = n->plan.L;
    a.fallbacks = n->d_blanked;
    for (int i = 0; i < gm::ST_M_MAX; ++i) { a.s[i] = n->plan.s[i]; a.w[i] = n->w[i]; }
    gm::launch_stap(st, a);
    return stage_launched(n, st, n_in, n_out);
}

extern "C" {

int gm_stap_plan(const gm_stap_cfg* cfg, uint64_t inputs_so_far, uint64_t n_in, uint32_t* block, float* loading, uint64_t* n_out) {
    StapPlan p;
    if (int rc = stap_rules(cfg, p)) return rc;
    return array_plan(p.B, p.loading, inputs_so_far, n_in, block, loading, n_out);
}

int gm_stap_create(const gm_stap_cfg* cfg, gm_stap** out) {
    if (!out) return set_err(GM_ERR_INVALID_ARG, "null out");
    *out = nullptr;
    StapPlan p;
    if (int rc = stap_rules(cfg, p)) return rc;
    if (int rc = ensure_device(g_device)) return rc;
    gm_stap* n = new gm_stap;
    n->device = g_device; n->plan = p;
    array_shape(n, "stap", p.A, p.B, p.loading, size_t(p.M) * p.M, p.M);
    hipError_t e = stage_create(n, stap_hist_bytes(p));
    if (e != hipSuccess) { gm_stap_destroy(n); return hip_fail(e, "gm_stap_create"); }
    *out = n;
    return GM_OK;
}

int gm_stap_destroy(gm_stap* n) {
    if (!n) return GM_OK;
    array_destroy(n);
    delete n;
    return GM_OK;
}

int gm_stap_reset(gm_stap* n, uint64_t input_index) {
    return stage_reset(n, input_index, [] { return hipSuccess; });
}

int gm_stap_stats(gm_stap* n, uint64_t* inputs, uint64_t* outputs, uint64_t* blocks, uint64_t* fallback_blocks) {
    return array_stats(n, inputs, outputs, blocks, fallback_blocks);
}

int gm_stap_synchronize(gm_stap* n) { return stage_synchronize(n); }

int gm_stap_set_weights(gm_stap* n, const gm_c32* w) { return array_set_host_weights(n, w); }

int gm_stap_capture(gm_stap* n, void* d_R, void* d_w, size_t cap_blocks) { return array_capture(n, d_R, d_w, cap_blocks); }

int gm_stap_process_dev(gm_stap* n, const void* d_in, int fmt, size_t n_in, void* d_out, size_t out_cap, size_t* n_out, void* stream) {
    return array_process_dev(n, stap_launch, d_in, fmt, n_in, d_out, out_cap, n_out, stream);
}

int gm_stap_process(gm_stap* n, const void* in, int fmt, size_t n_in, gm_c32* out, size_t out_cap, size_t* n_out, gm_c32* R, gm_c32* w,
                    size_t cap_blocks) {
    return array_process(n, stap_launch, in, fmt, n_in, out, out_cap, n_out, R, w, cap_blocks);
}

}  // extern "C"

// ====================================================================== one beam per constraint row from a shared Gram matrix (gm_beamformer)
// gnss_mi355x.h states the definition; tests/beam_model.py restates it in float64 on stap_model.py.
namespace {
struct BeamPlan {
    StapPlan st;                            // A, L, M, B, loading: gm_stap's rules (st.s is not used)
    uint32_t P = 0;
};

int beam_rules(const gm_beamformer_cfg* c, BeamPlan& p) {
    if (!c) return set_err(GM_ERR_INVALID_ARG, "null cfg");
    if (c->reserved || c->reserved32) return set_err(GM_ERR_INVALID_ARG, "gm_beamformer_cfg.reserved32 and reserved must be 0");
    gm_stap_cfg sc{};
    sc.n_antennas = c->n_antennas; sc.taps = c->taps; sc.block = c->block; sc.loading = c->loading;
    if (int rc = stap_rules(&sc, p.st)) return rc;
    if (c->n_beams < 1 || c->n_beams > uint32_t(gm::BM_P_MAX)) return set_err(GM_ERR_INVALID_ARG, "n_beams: 1 .. 16");
    if (!c->steering) return set_err(GM_ERR_INVALID_ARG, "steering is required: n_beams rows of taps * n_antennas words");
    for (uint32_t b = 0; b < c->n_beams; ++b)
        if (int rc = array_row_rules(c->steering + size_t(b) * p.st.M, p.st.M, "a steering row is all zero")) return rc;
    p.P = c->n_beams;
    return GM_OK;
}
}  // namespace

struct gm_beamformer : ArrayStage {         // history: gm_stap's; d_blanked is not used, the counters are per beam; R is [M][M], w is [P][M]
    BeamPlan plan;
    cf* d_s = nullptr; cf* d_w = nullptr;   // [P][M] each: the constraint rows, the fixed weights (too many words for the argument block)
    unsigned long long* d_fb = nullptr;     // [P] fallback counters
};

// one call's kernels on `st`; the caller has checked every argument; n_in > 0
static int beam_launch(gm_beamformer* n, hipStream_t st, const void* d_in, int fmt, uint64_t n_in, cf* out, uint64_t out_stride, uint64_t n_out,
                       cf* cap_R, cf* cap_w) {
    gm::BeamArgs a{};
    array_fill_args(a, n, d_in, n_in, out, n_out, cap_R, cap_w);
    a.fmt = fmt; a.L = n->plan.st.L; a.P = n->plan.P;
    a.out_stride = out_stride;
    a.fallbacks = n->d_fb; a.s = n->d_s; a.w = n->d_w;
    gm::launch_beam(st, a);
    return stage_launched(n, st, n_in, n_out);
}
// the words of the handle that kernels read are replaced only when no call of the handle is in flight, on any stream
static int beam_install(gm_beamformer* n, cf* d_dst, const gm_c32* src, size_t words) {
    if (int rc = ensure_device(n->device)) return rc;
    if (int rc = stage_sync(n)) return rc;
    HIPC(hipMemcpy(d_dst, src, words * sizeof(cf), hipMemcpyHostToDevice));
    return GM_OK;
}

extern "C" {

int gm_beamformer_plan(const gm_beamformer_cfg* cfg, uint64_t inputs_so_far, uint64_t n_in, uint32_t* block, float* loading, uint64_t* n_out) {
    BeamPlan p;
    if (int rc = beam_rules(cfg, p)) return rc;
    return array_plan(p.st.B, p.st.loading, inputs_so_far, n_in, block, loading, n_out);
}

int gm_beamformer_create(const gm_beamformer_cfg* cfg, gm_beamformer** out) {
    if (!out) return set_err(GM_ERR_INVALID_ARG, "null out");
    *out = nullptr;
    BeamPlan p;
    if (int rc = beam_rules(cfg, p)) return rc;
    if (int rc = ensure_device(g_device)) return rc;
    gm_beamformer* n = new gm_beamformer;
    n->device = g_device; n->plan = p;
    array_shape(n, "beamformer", p.st.A, p.st.B, p.st.loading, size_t(p.st.M) * p.st.M, size_t(p.P) * p.st.M, p.P);
    const size_t words = size_t(gm::BM_P_MAX) * gm::ST_M_MAX;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&n->d_s), words * sizeof(cf));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&n->d_w), words * sizeof(cf));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&n->d_fb), gm::BM_P_MAX * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(n->d_s, 0, words * sizeof(cf));
    if (e == hipSuccess) e = hipMemset(n->d_w, 0, words * sizeof(cf));
    if (e == hipSuccess) e = hipMemset(n->d_fb, 0, gm::BM_P_MAX * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemcpy(n->d_s, cfg->steering, size_t(p.P) * p.st.M * sizeof(cf), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = stage_create(n, stap_hist_bytes(p.st));
    if (e != hipSuccess) { gm_beamformer_destroy(n); return hip_fail(e, "gm_beamformer_create"); }
    *out = n;
    return GM_OK;
}

int gm_beamformer_destroy(gm_beamformer* n) {
    if (!n) return GM_OK;
    array_destroy(n);
    hipFree(n->d_s); hipFree(n->d_w); hipFree(n->d_fb);
    delete n;
    return GM_OK;
}

int gm_beamformer_reset(gm_beamformer* n, uint64_t input_index) {
    return stage_reset(n, input_index, [&] { return hipMemsetAsync(n->d_fb, 0, gm::BM_P_MAX * sizeof(unsigned long long), n->stream); });
}

int gm_beamformer_stats(gm_beamformer* n, uint64_t* inputs, uint64_t* outputs, uint64_t* blocks, uint64_t* fallbacks) {
    if (int rc = array_stats(n, inputs, outputs, blocks, nullptr)) return rc;
    if (fallbacks) {
        unsigned long long fb[gm::BM_P_MAX] = {};
        HIPC(hipMemcpy(fb, n->d_fb, n->plan.P * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (uint32_t p = 0; p < n->plan.P; ++p) fallbacks[p] = fb[p];
    }
    return GM_OK;
}

int gm_beamformer_synchronize(gm_beamformer* n) { return stage_synchronize(n); }

int gm_beamformer_set_steering(gm_beamformer* n, uint32_t beam, const gm_c32* s) {
    if (!n || !s) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (beam >= n->plan.P) return set_err(GM_ERR_INVALID_ARG, "beam: below n_beams");
    const uint32_t M = n->plan.st.M;
    if (int rc = array_row_rules(s, M, "a steering row is all zero")) return rc;
    return beam_install(n, n->d_s + size_t(beam) * M, s, M);
}

int gm_beamformer_set_weights(gm_beamformer* n, const gm_c32* w) {
    if (!n) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (!w) { n->fixed = false; return GM_OK; }
    if (!array_finite(w, n->w_words)) return set_err(GM_ERR_INVALID_ARG, "weights must be finite");
    if (int rc = beam_install(n, n->d_w, w, n->w_words)) return rc;
    n->fixed = true;
    return GM_OK;
}

int gm_beamformer_capture(gm_beamformer* n, void* d_R, void* d_w, size_t cap_blocks) { return array_capture(n, d_R, d_w, cap_blocks); }

int gm_beamformer_process_dev(gm_beamformer* n, const void* d_in, int fmt, size_t n_in, void* d_out, size_t out_stride, size_t* n_out,
                              void* stream) {
    return array_process_dev(n, beam_launch, d_in, fmt, n_in, d_out, out_stride, n_out, stream);
}

int gm_beamformer_process(gm_beamformer* n, const void* in, int fmt, size_t n_in, gm_c32* out, size_t out_stride, size_t* n_out, gm_c32* R,
                          gm_c32* w, size_t cap_blocks) {
    return array_process(n, beam_launch, in, fmt, n_in, out, out_stride, n_out, R, w, cap_blocks);
}

}  // extern "C"

// ====================================================================== several constraints on one beam (gm_lcmv; additive entries, ABI 9)
// gnss_mi355x.h states the definition; tests/lcmv_model.py restates it in float64 on stap_model.py.
namespace {
struct LcmvBeam {
    uint32_t Q = 0;
    cf c[gm::LC_Q_MAX][gm::ST_M_MAX] = {};  // the rows, each [L][A]
    cf f[gm::LC_Q_MAX] = {};                // the responses
    cf w0[gm::ST_M_MAX] = {};               // the quiescent weights C (C^H C)^-1 f, f64 rounded once
};
struct LcmvPlan {
    StapPlan st;                            // A, L, M, B, loading: gm_stap's rules (st.s is not used)
    uint32_t P = 0;
    LcmvBeam beam[gm::BM_P_MAX];
};

// one beam's rows and responses: the rules, and w0 = C (C^H C)^-1 f in f64 through the Cholesky factor of C^H C (columns ascending)
int lcmv_beam_rules(uint32_t M, uint32_t Q, const gm_c32* rows, const gm_c32* f, LcmvBeam& b) {
    if (Q < 1 || Q > uint32_t(gm::LC_Q_MAX) || Q > M) return set_err(GM_ERR_INVALID_ARG, "n_constraints: 1 .. 8 and at most taps * n_antennas");
    for (uint32_t q = 0; q < Q; ++q)
        if (int rc = array_row_rules(rows + size_t(q) * M, M, "a constraint row is all zero")) return rc;
    if (!array_finite(f, Q)) return set_err(GM_ERR_INVALID_ARG, "response must be finite");
    std::complex<double> G[gm::LC_Q_MAX][gm::LC_Q_MAX], v[gm::LC_Q_MAX];
    auto at = [&](uint32_t q, uint32_t j) { return std::complex<double>(rows[size_t(q) * M + j].re, rows[size_t(q) * M + j].im); };
    for (uint32_t q = 0; q < Q; ++q)
        for (uint32_t r = 0; r <= q; ++r) {
            std::complex<double> g = 0.0;
            for (uint32_t j = 0; j < M; ++j) g += std::conj(at(q, j)) * at(r, j);
            G[q][r] = g;
        }
    for (uint32_t j = 0; j < Q; ++j) {       // G = Lg Lg^H in place; a pivot not greater than 1e-10 of the row's squared norm: dependent
        const double norm = G[j][j].real();
        double pj = norm;
        for (uint32_t k = 0; k < j; ++k) pj -= std::norm(G[j][k]);
        if (!(pj > 1e-10 * norm) || !std::isfinite(pj)) return set_err(GM_ERR_INVALID_ARG, "the constraint rows of a beam are linearly dependent");
        const double d = std::sqrt(pj);
        for (uint32_t i = j + 1; i < Q; ++i) {
            std::complex<double> x = G[i][j];
            for (uint32_t k = 0; k < j; ++k) x -= G[i][k] * std::conj(G[j][k]);
            G[i][j] = x / d;
        }
        G[j][j] = d;
    }
    for (uint32_t j = 0; j < Q; ++j) {       // Lg y = f
        std::complex<double> x(f[j].re, f[j].im);
        for (uint32_t k = 0; k < j; ++k) x -= G[j][k] * v[k];
        v[j] = x / G[j][j].real();
    }
    for (uint32_t j = Q; j-- > 0;) {         // Lg^H v = y
        std::complex<double> x = v[j];
        for (uint32_t k = j + 1; k < Q; ++k) x -= std::conj(G[k][j]) * v[k];
        v[j] = x / G[j][j].real();
    }
    b = LcmvBeam{};
    b.Q = Q;
    for (uint32_t q = 0; q < Q; ++q) {
        b.f[q] = gm::cf_make(f[q].re, f[q].im);
        for (uint32_t j = 0; j < M; ++j) b.c[q][j] = gm::cf_make(rows[size_t(q) * M + j].re, rows[size_t(q) * M + j].im);
    }
    for (uint32_t j = 0; j < M; ++j) {
        std::complex<double> w = 0.0;
        for (uint32_t q = 0; q < Q; ++q) w += at(q, j) * v[q];
        if (!std::isfinite(w.real()) || !std::isfinite(w.imag()) || std::fabs(w.real()) > double(FLT_MAX) || std::fabs(w.imag()) > double(FLT_MAX))
            return set_err(GM_ERR_INVALID_ARG, "the quiescent weights of a beam are not finite in f32");
        b.w0[j] = gm::cf_make(float(w.real()), float(w.imag()));
    }
    return GM_OK;
}
uint32_t lcmv_q_sum(const LcmvPlan& p) {
    uint32_t s = 0;
    for (uint32_t b = 0; b < p.P; ++b) s += p.beam[b].Q;
    return s;
}

int lcmv_rules(const gm_lcmv_cfg* c, LcmvPlan& p) {
    if (!c) return set_err(GM_ERR_INVALID_ARG, "null cfg");
    if (c->reserved || c->reserved32) return set_err(GM_ERR_INVALID_ARG, "gm_lcmv_cfg.reserved32 and reserved must be 0");
    gm_stap_cfg sc{};
    sc.n_antennas = c->n_antennas; sc.taps = c->taps; sc.block = c->block; sc.loading = c->loading;
    if (int rc = stap_rules(&sc, p.st)) return rc;
    if (c->n_beams < 1 || c->n_beams > uint32_t(gm::BM_P_MAX)) return set_err(GM_ERR_INVALID_ARG, "n_beams: 1 .. 16");
    if (!c->n_constraints || !c->constraints || !c->response)
        return set_err(GM_ERR_INVALID_ARG, "n_constraints, constraints and response are required");
    uint32_t sum = 0;
    for (uint32_t b = 0; b < c->n_beams; ++b) {
        const uint32_t Q = c->n_constraints[b];
        if (Q < 1 || Q > uint32_t(gm::LC_Q_MAX) || Q > p.st.M) return set_err(GM_ERR_INVALID_ARG, "n_constraints: 1 .. 8 and at most taps * n_antennas");
        sum += Q;
    }
    if (sum > uint32_t(gm::LC_Q_SUM)) return set_err(GM_ERR_INVALID_ARG, "the constraint rows of all beams: at most 16");
    p.P = c->n_beams;
    uint32_t q0 = 0;
    for (uint32_t b = 0; b < p.P; ++b) {
        if (int rc = lcmv_beam_rules(p.st.M, c->n_constraints[b], c->constraints + size_t(q0) * p.st.M, c->response + q0, p.beam[b])) return rc;
        q0 += c->n_constraints[b];
    }
    return GM_OK;
}
}  // namespace

struct gm_lcmv : ArrayStage {               // history: gm_stap's; d_blanked is not used, the counters are per beam; R is [M][M], w is [P][M]
    LcmvPlan plan;
    cf* d_c = nullptr; cf* d_f = nullptr;   // [16][M] the rows of all beams, [16] their responses
    cf* d_w0 = nullptr; cf* d_w = nullptr;  // [P][M] each: the quiescent weights, the fixed weights
    unsigned long long* d_fb = nullptr;     // [P] fallback counters
};

// one call's kernels on `st`; the caller has checked every argument; n_in > 0
static int lcmv_launch(gm_lcmv* n, hipStream_t st, const void* d_in, int fmt, uint64_t n_in, cf* out, uint64_t out_stride, uint64_t n_out,
                       cf* cap_R, cf* cap_w) {
    gm::LcmvArgs a{};
    array_fill_args(a, n, d_in, n_in, out, n_out, cap_R, cap_w);
    a.fmt = fmt; a.L = n->plan.st.L; a.P = n->plan.P;
    a.out_stride = out_stride;
    a.fallbacks = n->d_fb; a.c = n->d_c; a.f = n->d_f; a.w0 = n->d_w0; a.w = n->d_w;
    for (uint32_t b = 0; b < n->plan.P; ++b) {
        a.nq[b] = uint8_t(n->plan.beam[b].Q); a.q0[b] = uint8_t(a.q_sum);
        a.q_sum += n->plan.beam[b].Q;
        a.q_max = std::max(a.q_max, n->plan.beam[b].Q);
    }
    gm::launch_lcmv(st, a);
    return stage_launched(n, st, n_in, n_out);
}
// the words of the handle that kernels read are replaced only when no call of the handle is in flight, on any stream
static int lcmv_install(gm_lcmv* n, cf* d_dst, const void* src, size_t words) {
    if (int rc = ensure_device(n->device)) return rc;
    if (int rc = stage_sync(n)) return rc;
    HIPC(hipMemcpy(d_dst, src, words * sizeof(cf), hipMemcpyHostToDevice));
    return GM_OK;
}
// the plan's rows, responses and quiescent weights, packed as the kernel reads them
static void lcmv_pack(const LcmvPlan& p, std::vector<cf>& c, std::vector<cf>& f, std::vector<cf>& w0) {
    const uint32_t M = p.st.M;
    c.assign(size_t(gm::LC_Q_SUM) * M, cf{}); f.assign(gm::LC_Q_SUM, cf{}); w0.assign(size_t(gm::BM_P_MAX) * M, cf{});
    uint32_t q0 = 0;
    for (uint32_t b = 0; b < p.P; ++b) {
        for (uint32_t q = 0; q < p.beam[b].Q; ++q, ++q0) {
            f[q0] = p.beam[b].f[q];
            for (uint32_t j = 0; j < M; ++j) c[size_t(q0) * M + j] = p.beam[b].c[q][j];
        }
        for (uint32_t j = 0; j < M; ++j) w0[size_t(b) * M + j] = p.beam[b].w0[j];
    }
}

extern "C" {

int gm_lcmv_plan(const gm_lcmv_cfg* cfg, uint64_t inputs_so_far, uint64_t n_in, uint32_t* block, float* loading, uint64_t* n_out) {
    LcmvPlan p;
    if (int rc = lcmv_rules(cfg, p)) return rc;
    return array_plan(p.st.B, p.st.loading, inputs_so_far, n_in, block, loading, n_out);
}

int gm_lcmv_create(const gm_lcmv_cfg* cfg, gm_lcmv** out) {
    if (!out) return set_err(GM_ERR_INVALID_ARG, "null out");
    *out = nullptr;
    LcmvPlan p;
    if (int rc = lcmv_rules(cfg, p)) return rc;
    if (int rc = ensure_device(g_device)) return rc;
    gm_lcmv* n = new gm_lcmv;
    n->device = g_device; n->plan = p;
    array_shape(n, "lcmv", p.st.A, p.st.B, p.st.loading, size_t(p.st.M) * p.st.M, size_t(p.P) * p.st.M, p.P);
    std::vector<cf> c, f, w0;
    lcmv_pack(p, c, f, w0);
    const size_t words = size_t(gm::BM_P_MAX) * gm::ST_M_MAX;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&n->d_c), words * sizeof(cf));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&n->d_f), gm::LC_Q_SUM * sizeof(cf));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&n->d_w0), words * sizeof(cf));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&n->d_w), words * sizeof(cf));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&n->d_fb), gm::BM_P_MAX * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(n->d_c, 0, words * sizeof(cf));
    if (e == hipSuccess) e = hipMemset(n->d_w0, 0, words * sizeof(cf));
    if (e == hipSuccess) e = hipMemset(n->d_w, 0, words * sizeof(cf));
    if (e == hipSuccess) e = hipMemset(n->d_fb, 0, gm::BM_P_MAX * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemcpy(n->d_c, c.data(), c.size() * sizeof(cf), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(n->d_f, f.data(), f.size() * sizeof(cf), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(n->d_w0, w0.data(), w0.size() * sizeof(cf), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = stage_create(n, stap_hist_bytes(p.st));
    if (e != hipSuccess) { gm_lcmv_destroy(n); return hip_fail(e, "gm_lcmv_create"); }
    *out = n;
    return GM_OK;
}

int gm_lcmv_destroy(gm_lcmv* n) {
    if (!n) return GM_OK;
    array_destroy(n);
    hipFree(n->d_c); hipFree(n->d_f); hipFree(n->d_w0); hipFree(n->d_w); hipFree(n->d_fb);
    delete n;
    return GM_OK;
}

int gm_lcmv_reset(gm_lcmv* n, uint64_t input_index) {
    return stage_reset(n, input_index, [&] { return hipMemsetAsync(n->d_fb, 0, gm::BM_P_MAX * sizeof(unsigned long long), n->stream); });
}

int gm_lcmv_stats(gm_lcmv* n, uint64_t* inputs, uint64_t* outputs, uint64_t* blocks, uint64_t* fallbacks) {
    if (int rc = array_stats(n, inputs, outputs, blocks, nullptr)) return rc;
    if (fallbacks) {
        unsigned long long fb[gm::BM_P_MAX] = {};
        HIPC(hipMemcpy(fb, n->d_fb, n->plan.P * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (uint32_t p = 0; p < n->plan.P; ++p) fallbacks[p] = fb[p];
    }
    return GM_OK;
}

int gm_lcmv_synchronize(gm_lcmv* n) { return stage_synchronize(n); }

int gm_lcmv_set_constraints(gm_lcmv* n, uint32_t beam, uint32_t n_rows, const gm_c32* rows, const gm_c32* response) {
    if (!n || !rows || !response) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (beam >= n->plan.P) return set_err(GM_ERR_INVALID_ARG, "beam: below n_beams");
    LcmvBeam b;
    if (int rc = lcmv_beam_rules(n->plan.st.M, n_rows, rows, response, b)) return rc;
    if (lcmv_q_sum(n->plan) - n->plan.beam[beam].Q + n_rows > uint32_t(gm::LC_Q_SUM))
        return set_err(GM_ERR_INVALID_ARG, "the constraint rows of all beams: at most 16");
    LcmvPlan p = n->plan;
    p.beam[beam] = b;
    std::vector<cf> c, f, w0;
    lcmv_pack(p, c, f, w0);
    if (int rc = lcmv_install(n, n->d_c, c.data(), c.size())) return rc;      // (waits for the calls in flight; the later copies find none)
    HIPC(hipMemcpy(n->d_f, f.data(), f.size() * sizeof(cf), hipMemcpyHostToDevice));
    HIPC(hipMemcpy(n->d_w0, w0.data(), w0.size() * sizeof(cf), hipMemcpyHostToDevice));
    n->plan = p;
    return GM_OK;
}

int gm_lcmv_set_weights(gm_lcmv* n, const gm_c32* w) {
    if (!n) return set_err(GM_ERR_INVALID_ARG, "null handle");
    if (!w) { n->fixed = false; return GM_OK; }
    if (!array_finite(w, n->w_words)) return set_err(GM_ERR_INVALID_ARG, "weights must be finite");
    if (int rc = lcmv_install(n, n->d_w, w, n->w_words)) return rc;
    n->fixed = true;
    return GM_OK;
}

int gm_lcmv_capture(gm_lcmv* n, void* d_R, void* d_w, size_t cap_blocks) { return array_capture(n, d_R, d_w, cap_blocks); }

int gm_lcmv_process_dev(gm_lcmv* n, const void* d_in, int fmt, size_t n_in, void* d_out, size_t out_stride, size_t* n_out, void* stream) {
    return array_process_dev(n, lcmv_launch, d_in, fmt, n_in, d_out, out_stride, n_out, stream);
}

int gm_lcmv_process(gm_lcmv* n, const void* in, int fmt, size_t n_in, gm_c32* out, size_t out_stride, size_t* n_out, gm_c32* R, gm_c32* w,
                    size_t cap_blocks) {
    return array_process(n, lcmv_launch, in, fmt, n_in, out, out_stride, n_out, R, w, cap_blocks);
}

}  // extern "C"

// ====================================================================== re-steering on the device (additive entries, ABI 9)
// gnss_mi355x.h states the contracts.  Three entries that enqueue and return: the tracker's array prompts into device buffers, the
// batched row solver (array_solve.hip), and the install of its rows into a beamformer's steering words.  Together with
// gm_beamformer_process_dev they put a whole update behind the block it belongs to, on one stream, with no host wait.
namespace {
// gm_array_solve_plan's rules; the resolved loading and strides, and the extents in c32 words
struct SolvePlan { double load = 1e-4; uint64_t row_stride = 0, vec_stride = 0, z_words = 0, R_words = 0, row_words = 0; };
int solve_rules(const gm_array_solve_cfg* c, SolvePlan& p) {
    if (!c) return set_err(GM_ERR_INVALID_ARG, "null cfg");
    for (uint32_t v : c->reserved)
        if (v) return set_err(GM_ERR_INVALID_ARG, "gm_array_solve_cfg.reserved must be 0");
    if (c->m < 2 || c->m > uint32_t(gm::ST_M_MAX)) return set_err(GM_ERR_INVALID_ARG, "m must be 2 .. 32");
    if (c->n < 1 || c->n > 4096) return set_err(GM_ERR_INVALID_ARG, "n must be 1 .. 4096");
    if (c->n_rows < 1 || c->n_rows > 1024) return set_err(GM_ERR_INVALID_ARG, "n_rows must be 1 .. 1024");
    if (c->n_blocks > (1u << 20)) return set_err(GM_ERR_INVALID_ARG, "n_blocks must be at most 2^20");
    if ((c->row_stride == 0) != (c->vec_stride == 0)) return set_err(GM_ERR_INVALID_ARG, "row_stride and vec_stride: both 0 or neither");
    p.row_stride = c->row_stride ? c->row_stride : uint64_t(c->n) * c->m;
    p.vec_stride = c->vec_stride ? c->vec_stride : uint64_t(c->m);
    if (p.vec_stride < c->m || p.row_stride < c->m) return set_err(GM_ERR_INVALID_ARG, "row_stride and vec_stride must be at least m");
    if (p.vec_stride > (1ull << 40) || p.row_stride > (1ull << 40)) return set_err(GM_ERR_INVALID_ARG, "row_stride and vec_stride must be at most 2^40");
    if (c->loading != 0.0f) {
        if (!(c->loading >= 1e-6f && c->loading <= 1.0f)) return set_err(GM_ERR_INVALID_ARG, "loading must be 0 or lie in [1e-6, 1]");   // (NaN fails too)
        p.load = double(c->loading);
    }
    p.z_words = uint64_t(c->n_rows - 1) * p.row_stride + uint64_t(c->n - 1) * p.vec_stride + c->m;
    p.R_words = uint64_t(c->n_blocks) * c->m * c->m;
    p.row_words = uint64_t(c->n_rows) * c->m;
    return GM_OK;
}
// the next pinned slot for a call's records and the event to record behind their copy; a caller ARRAY_SLOTS calls ahead of its
// stream waits here for the oldest copy
int trk_array_slot(gm_trk* t, void** h, hipEvent_t* ev) {
    constexpr size_t slot_bytes = size_t(gm::GM_TRK_ARRAY_MAX_STATES) * sizeof(gm::TrkBankRec);
    if (!t->array_recs) {
        void* blk = nullptr;
        HIPC(hipHostMalloc(&blk, slot_bytes * gm_trk::ARRAY_SLOTS, hipHostMallocDefault));
        for (auto& e : t->array_ev)
            if (hipError_t rc = hipEventCreateWithFlags(&e, hipEventDisableTiming); rc != hipSuccess) {
                for (auto& d : t->array_ev) { if (d) hipEventDestroy(d); d = nullptr; }
                hipHostFree(blk);
                return hip_fail(rc, "hipEventCreate");
            }
        t->array_recs = static_cast<uint8_t*>(blk);
    }
    const uint32_t k = t->array_next % gm_trk::ARRAY_SLOTS;
    HIPC(hipEventSynchronize(t->array_ev[k]));                // (returns at once for an event never recorded or already passed)
    *h = t->array_recs + slot_bytes * k; *ev = t->array_ev[k];
    ++t->array_next;
    return GM_OK;
}
}  // namespace

extern "C" {

int gm_trk_array_prompts_dev(gm_trk* t, const void* d_samples, int fmt, uint64_t first_index, uint64_t n_time, const gm_trk_state* states,
                             uint32_t n_states, const gm_trk_array_cfg* cfg, void* d_z, void* d_done, void* stream) {
    if (!t || !d_samples || !d_z || !d_done) return set_err(GM_ERR_INVALID_ARG, "null handle, samples, d_z or d_done");
    if (fmt != GM_FMT_C32 && fmt != GM_FMT_I8_IQ) return set_err(GM_ERR_INVALID_ARG, "fmt must be GM_FMT_C32 or GM_FMT_I8_IQ");
    if (!states) return set_err(GM_ERR_INVALID_ARG, "states NULL: the handle's own channels live on the device (take them from gm_trk_collect)");
    if (int rc = trk_array_call_rules(t, first_index, n_time, cfg, n_states)) return rc;
    const uint32_t R = n_states, M = cfg->n_antennas * cfg->taps;
    if (n_time <= (1ull << 40))
        if (stage_check_overlap(d_samples, size_t(n_time) * cfg->n_antennas * fmt_bytes(fmt), d_z, uint64_t(R) * M))
            return set_err(GM_ERR_INVALID_ARG, "d_z overlaps the samples");
    if (int rc = ensure_device(t->device)) return rc;
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : t->stream;
    if (int rc = trk_array_join(t, st)) return rc;
    std::vector<gm::TrkBankRec> recs;
    if (int rc = trk_call_records(t, states, n_states, recs)) return rc;
    TrkArrayCall c;
    if (int rc = trk_array_carve(t, st, recs, first_index, n_time, cfg, c)) return rc;
    void* h_recs = nullptr;
    hipEvent_t copied = nullptr;
    if (int rc = trk_array_slot(t, &h_recs, &copied)) return rc;
    memcpy(h_recs, recs.data(), R * sizeof(gm::TrkBankRec));
    uint8_t* d = static_cast<uint8_t*>(t->array.d);
    HIPC(hipMemcpyAsync(d + c.o_recs, h_recs, R * sizeof(gm::TrkBankRec), hipMemcpyHostToDevice, st));
    HIPC(hipEventRecord(copied, st));
    trk_array_launch(t, st, d_samples, fmt, first_index, cfg, c, R, static_cast<gm_c32*>(d_z), static_cast<uint8_t*>(d_done));
    HIPC(hipGetLastError());
    t->array_last = st;
    return GM_OK;
}

int gm_array_solve_plan(const gm_array_solve_cfg* cfg, uint64_t* z_words, uint64_t* R_words, uint64_t* row_words) {
    SolvePlan p;
    if (int rc = solve_rules(cfg, p)) return rc;
    if (z_words) *z_words = p.z_words;
    if (R_words) *R_words = p.R_words;
    if (row_words) *row_words = p.row_words;
    return GM_OK;
}

int gm_array_rows_solve_dev(const gm_array_solve_cfg* cfg, const void* d_z, const void* d_R, void* d_rows, void* d_info, void* stream) {
    SolvePlan p;
    if (int rc = solve_rules(cfg, p)) return rc;
    if (!d_z || !d_rows || !d_info) return set_err(GM_ERR_INVALID_ARG, "null d_z, d_rows or d_info");
    if ((d_R == nullptr) != (cfg->n_blocks == 0)) return set_err(GM_ERR_INVALID_ARG, "n_blocks: 0 exactly where d_R is null");
    if (int rc = ensure_device(g_device)) return rc;
    gm::ArraySolveArgs a{};
    a.z = static_cast<const cf*>(d_z); a.R = static_cast<const cf*>(d_R);
    a.rows = static_cast<cf*>(d_rows); a.info = d_info;
    a.row_stride = p.row_stride; a.vec_stride = p.vec_stride;
    a.m = cfg->m; a.n = cfg->n; a.n_rows = cfg->n_rows; a.n_blocks = cfg->n_blocks;
    a.load = p.load;
    gm::launch_array_solve(static_cast<hipStream_t>(stream), a);
    HIPC(hipGetLastError());
    return GM_OK;
}

int gm_beamformer_set_steering_dev(gm_beamformer* n, uint32_t first_beam, uint32_t n_rows, const void* d_rows, const void* d_info,
                                   float min_ratio, void* d_installed, void* stream) {
    if (!n || !d_rows) return set_err(GM_ERR_INVALID_ARG, "null pointer");
    if (!n_rows) return set_err(GM_ERR_INVALID_ARG, "n_rows = 0");
    if (first_beam >= n->plan.P || n_rows > n->plan.P - first_beam) return set_err(GM_ERR_INVALID_ARG, "first_beam + n_rows: at most n_beams");
    if (!std::isfinite(min_ratio) || min_ratio < 0.0f) return set_err(GM_ERR_INVALID_ARG, "min_ratio must be finite and not negative");
    if (int rc = ensure_device(n->device)) return rc;
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : n->stream;
    if (int rc = stage_join(n, st)) return rc;                // a call in flight elsewhere reads the old rows
    gm::BeamInstallArgs a{};
    a.rows = static_cast<const cf*>(d_rows); a.info = d_info; a.s = n->d_s; a.installed = static_cast<uint8_t*>(d_installed);
    a.M = n->plan.st.M; a.first_beam = first_beam; a.n_rows = n_rows; a.min_ratio = min_ratio;
    gm::launch_beam_install(st, a);
    HIPC(hipGetLastError());
    n->last_stream = st;
    return GM_OK;
}

}  // extern "C"

// ====================================================================== multi-GPU exchange
// The path's ONE exchange step: all-gather of the per-(worker, bin) metrics over RCCL, enqueued on the acquisition
// handle's stream, followed by the regroup to the [3][nranks*P][D] layout gm_acq_decide_dev replays.  RCCL is bound
// lazily (dlopen of librccl.so.1 — inside a PyTorch process that is the copy PyTorch already loaded), so single-GPU
// hosts never need it.
#include <rccl/rccl.h>

namespace {
struct RcclApi {
    void* so = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool ok = false;
};
RcclApi& rccl() {
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        const char* names[] = {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"};
        for (const char* n : names)
            if ((api.so = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
        if (!api.so) return;
        api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(dlsym(api.so, "ncclGetUniqueId"));
        api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(dlsym(api.so, "ncclCommInitRank"));
        api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(dlsym(api.so, "ncclCommDestroy"));
        api.AllGather = reinterpret_cast<decltype(api.AllGather)>(dlsym(api.so, "ncclAllGather"));
        api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(dlsym(api.so, "ncclGetErrorString"));
        api.ok = api.GetUniqueId && api.CommInitRank && api.CommDestroy && api.AllGather && api.GetErrorString;
    });
    return api;
}
int rccl_fail(ncclResult_t r, const char* where) {
    char buf[256];
    snprintf(buf, sizeof(buf), "%s: %s", where, rccl().GetErrorString ? rccl().GetErrorString(r) : "RCCL error");
    g_last_error = buf;
    return GM_ERR_HIP;
}
#define RCCLC(expr)                                           \
    do {                                                      \
        ncclResult_t _r = (expr);                             \
        if (_r != ncclSuccess) return rccl_fail(_r, #expr);   \
    } while (0)

// gathered [R][3][PD] -> out [3][R][PD]  (== [3][R*P][D])
__global__ void regroup_metrics_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t R, uint32_t PD) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t total = R * 3u * PD;
    if (i >= total) return;
    const uint32_t e = i % PD, q = (i / PD) % 3u, r = i / (3u * PD);
    out[(size_t(q) * R + r) * PD + e] = in[i];
}
}  // namespace

struct gm_comm {
    int device = -1;
    int nranks = 0, rank = 0;
    ncclComm_t comm = nullptr;
    uint32_t* d_stage = nullptr;   // [nranks][3][PD] as the all-gather lays it out
    size_t stage_words = 0;
    // overlapped exchange (gm_acq_allgather_metrics_async): the collective runs on the communicator's own stream between
    // two events, so the next dwell's kernels on the handle's stream do not wait for it
    hipStream_t xs = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    hipEvent_t ev_sync = nullptr;  // behind the last SYNCHRONOUS exchange's regroup (it reads d_stage on the caller's stream)
    bool pending = false, async_used = false, sync_used = false;
};

extern "C" {

int gm_comm_get_unique_id(uint8_t id[GM_COMM_ID_BYTES]) {
    if (!id) return set_err(GM_ERR_INVALID_ARG, "null id");
    static_assert(GM_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "id size");
    if (!rccl().ok) return set_err(GM_ERR_UNSUPPORTED, "librccl.so.1 not found");
    ncclUniqueId u;
    RCCLC(rccl().GetUniqueId(&u));
    memcpy(id, u.internal, GM_COMM_ID_BYTES);
    return GM_OK;
}

int gm_comm_init(int nranks, int rank, const uint8_t id[GM_COMM_ID_BYTES], gm_comm** out) {
    if (!out || !id || nranks < 1 || rank < 0 || rank >= nranks) return set_err(GM_ERR_INVALID_ARG, "bad nranks/rank/id");
    if (int rc = ensure_device(g_device)) return rc;
    if (!rccl().ok) return set_err(GM_ERR_UNSUPPORTED, "librccl.so.1 not found");
    ncclUniqueId u;
    memcpy(u.internal, id, GM_COMM_ID_BYTES);
    gm_comm* c = new gm_comm;
    c->device = g_device; c->nranks = nranks; c->rank = rank;
    ncclResult_t r = rccl().CommInitRank(&c->comm, nranks, u, rank);
    if (r != ncclSuccess) { delete c; return rccl_fail(r, "ncclCommInitRank"); }
    *out = c;
    return GM_OK;
}

int gm_comm_destroy(gm_comm* c) {
    if (!c) return GM_OK;
    if (c->device >= 0) hipSetDevice(c->device);
    if (c->xs) { hipStreamSynchronize(c->xs); hipStreamDestroy(c->xs); }
    if (c->ev_in) hipEventDestroy(c->ev_in);
    if (c->ev_out) hipEventDestroy(c->ev_out);
    if (c->ev_sync) hipEventDestroy(c->ev_sync);
    if (c->comm) rccl().CommDestroy(c->comm);
    hipFree(c->d_stage);
    delete c;
    return GM_OK;
}

int gm_comm_info(gm_comm* c, int* nranks, int* rank) {
    if (!c) return set_err(GM_ERR_INVALID_ARG, "null comm");
    if (nranks) *nranks = c->nranks;
    if (rank) *rank = c->rank;
    return GM_OK;
}

static int comm_gather_regroup(gm_acq* a, gm_comm* c, const void* d_local, void* d_all, hipStream_t st);
int gm_acq_allgather_metrics(gm_acq* a, gm_comm* c, const void* d_local, void* d_all) {
    if (!a || !c || !d_all) return set_err(GM_ERR_INVALID_ARG, "null handle/comm/output");
    if (a->device != c->device) return set_err(GM_ERR_INVALID_ARG, "handle and communicator live on different devices");
    if (int rc = ensure_device(a->device)) return rc;
    // d_stage is ONE buffer: an asynchronous exchange still running on the communicator's stream must have read it out before
    // this one overwrites it (whether or not gm_comm_wait has been called for it yet, and on whichever stream)
    if (c->async_used) HIPC(hipStreamWaitEvent(a->stream, c->ev_out, 0));
    if (int rc = comm_gather_regroup(a, c, d_local, d_all, a->stream)) return rc;
    if (!c->ev_sync) HIPC(hipEventCreateWithFlags(&c->ev_sync, hipEventDisableTiming));
    HIPC(hipEventRecord(c->ev_sync, a->stream));
    c->sync_used = true;
    return GM_OK;
}

static int comm_gather_regroup(gm_acq* a, gm_comm* c, const void* d_local, void* d_all, hipStream_t st) {
    const size_t PD = size_t(a->P) * a->D, words = 3 * PD;
    const uint32_t* src = d_local ? static_cast<const uint32_t*>(d_local) : a->d_metrics;
    if (c->stage_words < words * c->nranks) {
        if (c->xs) HIPC(hipStreamSynchronize(c->xs));
        hipFree(c->d_stage); c->d_stage = nullptr; c->stage_words = 0;
        HIPC(hipMalloc(&c->d_stage, words * c->nranks * sizeof(uint32_t)));
        c->stage_words = words * c->nranks;
    }
    RCCLC(rccl().AllGather(src, c->d_stage, words, ncclInt32, c->comm, st));
    const uint32_t total = uint32_t(words * c->nranks);
    regroup_metrics_kernel<<<(total + 255) / 256, 256, 0, st>>>(c->d_stage, static_cast<uint32_t*>(d_all),
                                                                 uint32_t(c->nranks), uint32_t(PD));
    HIPC(hipGetLastError());
    return GM_OK;
}

int gm_acq_allgather_metrics_async(gm_acq* a, gm_comm* c, const void* d_local, void* d_all) {
    if (!a || !c || !d_all) return set_err(GM_ERR_INVALID_ARG, "null handle/comm/output");
    if (a->device != c->device) return set_err(GM_ERR_INVALID_ARG, "handle and communicator live on different devices");
    if (int rc = ensure_device(a->device)) return rc;
    if (!c->xs) {
        HIPC(hipStreamCreateWithFlags(&c->xs, hipStreamNonBlocking));
        HIPC(hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming));
        HIPC(hipEventCreateWithFlags(&c->ev_out, hipEventDisableTiming));
    }
    HIPC(hipEventRecord(c->ev_in, a->stream));          // everything enqueued so far on the handle's stream (the search)
    HIPC(hipStreamWaitEvent(c->xs, c->ev_in, 0));
    if (c->sync_used) HIPC(hipStreamWaitEvent(c->xs, c->ev_sync, 0));     // ... and a synchronous exchange of ANOTHER handle through this communicator
    if (int rc = comm_gather_regroup(a, c, d_local, d_all, c->xs)) return rc;
    HIPC(hipEventRecord(c->ev_out, c->xs));
    c->pending = true;
    c->async_used = true;
    return GM_OK;
}

int gm_comm_wait(gm_comm* c, void* hip_stream) {
    if (!c) return set_err(GM_ERR_INVALID_ARG, "null comm");
    if (int rc = ensure_device(c->device)) return rc;
    if (c->pending) {
        HIPC(hipStreamWaitEvent(reinterpret_cast<hipStream_t>(hip_stream), c->ev_out, 0));
        c->pending = false;
    }
    return GM_OK;
}

int gm_comm_allgather_words(gm_comm* c, const void* d_local, void* d_all, size_t words, void* hip_stream) {
    if (!c || !d_local || !d_all || !words) return set_err(GM_ERR_INVALID_ARG, "null comm/buffer or zero words");
    if (int rc = ensure_device(c->device)) return rc;
    RCCLC(rccl().AllGather(d_local, d_all, words, ncclInt32, c->comm, reinterpret_cast<hipStream_t>(hip_stream)));
    return GM_OK;
}

}  // extern "C"

namespace {
// gathered [R][3][pmax][D] -> out [3][n_rows][D], row i taken from block row_map[i] = rank * pmax + row
__global__ void grid_assemble_kernel(const uint32_t* __restrict__ in, const uint32_t* __restrict__ row_map, uint32_t pmax,
                                     uint32_t D, uint32_t n_rows, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3u * n_rows * D) return;
    const uint32_t e = i % D, row = (i / D) % n_rows, q = i / (D * n_rows);
    const uint32_t src = row_map[row], r = src / pmax, k = src - r * pmax;
    out[i] = in[((size_t(r) * 3u + q) * pmax + k) * D + e];
}
}  // namespace

extern "C" {

int gm_grid_assemble_dev(const void* d_gathered, uint32_t nranks, uint32_t p_max, uint32_t n_bins, const uint32_t* d_row_map,
                         uint32_t n_rows, void* d_out, void* hip_stream) {
    if (!d_gathered || !d_row_map || !d_out || !nranks || !p_max || !n_bins || !n_rows)
        return set_err(GM_ERR_INVALID_ARG, "null buffer or zero dimension");
    if (n_rows > nranks * p_max) return set_err(GM_ERR_OUT_OF_RANGE, "more rows than the gathered blocks hold");
    if (int rc = ensure_device(g_device)) return rc;
    const uint32_t total = 3u * n_rows * n_bins;
    grid_assemble_kernel<<<(total + 255) / 256, 256, 0, reinterpret_cast<hipStream_t>(hip_stream)>>>(
        static_cast<const uint32_t*>(d_gathered), d_row_map, p_max, n_bins, n_rows, static_cast<uint32_t*>(d_out));
    HIPC(hipGetLastError());
    return GM_OK;
}

int gm_acq_decide_planes_dev(const float* d_max, const uint32_t* d_argmax, const float* d_sum, uint32_t n_prn, uint32_t n_bins,
                             const uint8_t* d_prn_ids, const float* d_table_freq, uint32_t fft_size, float fs, float code_rate,
                             float threshold, int decision_mode, uint64_t local_tail, gm_acq_result* d_results, uint8_t* d_found,
                             void* hip_stream) {
    if (!d_max || !d_argmax || !d_sum || !d_prn_ids || !d_table_freq || !d_results || !d_found || !n_prn || !n_bins || fft_size < 2)
        return set_err(GM_ERR_INVALID_ARG, "null buffer or zero dimension");
    if (n_bins > GM_ACQ_DECIDE_MAX_BINS) return set_err(GM_ERR_OUT_OF_RANGE, DECIDE_BINS_MSG);
    if (threshold == 0.0f) threshold = 7.0f;             // gm_acq_cfg's and gm_acq_decide_host's defaults
    if (!(code_rate > 0.0f)) code_rate = CA_RATE;
    if (int rc = ensure_device(g_device)) return rc;
    gm::DecideArgs da;
    da.mmax = d_max; da.margmax = d_argmax; da.msum = d_sum;
    da.table_freq = d_table_freq; da.prn_ids = d_prn_ids;
    da.mask_lo = ~0ull;
    da.n_prn = int(n_prn); da.n_bins = int(n_bins); da.fft_size = int(fft_size);
    da.fs = fs; da.threshold = threshold; da.code_rate = code_rate;
    da.best_bin_mode = decision_mode == GM_DECIDE_BEST_BIN ? 1 : 0;
    da.local_tail = local_tail;
    da.results = d_results; da.found = d_found;
    gm::launch_decide(reinterpret_cast<hipStream_t>(hip_stream), da);
    HIPC(hipGetLastError());
    return GM_OK;
}

}  // extern "C"

