"""Wall-clock time of the whole synchronous gm_trk_bank call — 32 records at 25 Msps (n = 25000) on a resident ring — at (T, F) =
(3, 1), (16, 1), (64, 1), (16, 8), beside one synchronous gm_trk_update_all(…, 1 epoch) of the same 32 channels in the same process as
the yardstick; writes profiles/trk_bank_times.json.  Each figure is the host's perf_counter time around ten back-to-back calls,
divided by ten; two warm-up rounds, then five repeats with the bank and the update alternating; the median and `spread` = (max - min)
/ median of the five.  The bank reads the records it is handed and moves nothing, so every bank call sees the same epoch; the update
advances its channels by one epoch a call, on a twin handle, and the ring holds enough periods for all of its calls.
Usage: python tools/trk_bank_time.py [--out profiles/trk_bank_times.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(3, 1), (16, 1), (64, 1), (16, 8)]
CALLS, REPEATS, WARMUP = 10, 5, 2
FS, N, CHANNELS = 25.0e6, 25000, 32


def _stats(v):
    med = float(np.median(v))
    return dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), spread=round((max(v) - min(v)) / med, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trk_bank_times.json"))
    args = ap.parse_args()
    from oracle import oracle as O
    from gnss_sdr_rs_amd import _lib, synth, tracking as T
    _lib.init(0)
    table = O.ca_code_table()
    prns = [1 + (i % 31) for i in range(CHANNELS)]
    uniq = sorted(set(prns))
    epochs = len(SHAPES) * (WARMUP + REPEATS) * CALLS + 4            # one per update call, and a few to spare
    ms = 12                                                          # the scene repeats: the ring is written with it over and over
    sc = synth.tracking_scene(table, FS, 0.0, uniq, ms, config_id=3, cn0=47.0)
    x = synth.to_c32(sc["x"])
    ring = T.MulticastRingBuffer(1 << 24)                            # 16.7 M samples: 671 periods
    assert epochs * N + N < (1 << 24)
    for k in range(0, epochs * N + N, x.size):
        ring.write_samples(x[:min(x.size, epochs * N + N - k)])
    by_prn = {s["prn"]: s for s in sc["sats"]}
    bank_mgr = T.TrackingManager(FS, n_channels=CHANNELS, code_index_mode=T.CODE_INDEX_FIXED)
    upd_mgr = T.TrackingManager(FS, n_channels=CHANNELS, code_index_mode=T.CODE_INDEX_FIXED)
    for m in (bank_mgr, upd_mgr):
        for i, p in enumerate(prns):
            m.channels[i].start(dict(prn=p, code_phase_samples=0, code_phase_chips=0.0, carrier_freq=by_prn[p]["doppler_hz"] + 20.0, fs=FS,
                                     mag_relative=10.0, sample_global_index=by_prn[p]["code_start"], doppler_bin=0))
    states = bank_mgr.get_states()

    def timed(fn):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        return (time.perf_counter() - t0) * 1e3 / CALLS

    def update():
        _, _, _, done = upd_mgr.update_all(ring, 1)
        assert done == 1

    rows = []
    for nt, nf in SHAPES:
        taps = np.linspace(-1.0, 1.0, nt) if nt > 1 else np.zeros(1)
        offs = np.linspace(-400.0, 400.0, nf) if nf > 1 else np.zeros(1)

        def bank():
            _, done = bank_mgr.bank(ring, taps, offs, states=states)
            assert done.all()

        for _ in range(WARMUP):
            timed(bank)
            timed(update)
        t_bank, t_upd = [], []
        for _ in range(REPEATS):
            t_bank.append(timed(bank))
            t_upd.append(timed(update))
        row = dict(n_taps=nt, n_offsets=nf, records=CHANNELS, samples_per_record=N, bank=_stats(t_bank), update_all_one_epoch=_stats(t_upd),
                   bank_over_update=round(float(np.median(t_bank)) / float(np.median(t_upd)), 4))
        print(json.dumps(row), flush=True)
        rows.append(row)
    bank_mgr.close(); upd_mgr.close(); ring.close()
    meta = dict(tool="tools/trk_bank_time.py", calls=CALLS, repeats=REPEATS, warmup_rounds=WARMUP,
                timing="host perf_counter time around ten back-to-back synchronous calls, divided by ten: gm_trk_bank on 32 records at 25 Msps "
                       "(uploads, two kernels, the copy back and the wait), and gm_trk_update_all(…, 1 epoch) of 32 channels of a twin handle on "
                       "the same ring; one process, two warm-up rounds each, five repeats with the two alternating; median and spread = "
                       "(max - min) / median")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(meta=meta, shapes=rows), f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
