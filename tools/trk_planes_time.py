"""Event time of gm_trk_update_planes_dev — 15 channels x 16 epochs at fs = 16.368 MHz (n = 16368), channel c on plane c of a 15-plane
ring — beside gm_trk_update_all_dev of the same 15 channels on ONE plain ring (the persistent kernel, the code path that existed before
tracking on planes) in the same process; writes profiles/trk_planes_times.json.  Each figure is the handle's own event pair around the
launch (gm_trk_enable_timing / gm_trk_last_timing) of one call of 16 passes from the same start states (gm_trk_set_states before every
call); one warm-up call each, then five repeats with the two alternating; the median and `spread` = (max - min) / median of the five.
The one condition reported (not tested): 16 epochs must take less than 16 code periods (16 ms) of wall time.
Usage: python tools/trk_planes_time.py [--out profiles/trk_planes_times.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS, N, CHANNELS, EPOCHS, REPEATS, WARMUP = 16.368e6, 16368, 15, 16, 5, 1


def _stats(v):
    med = float(np.median(v))
    return dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), spread=round((max(v) - min(v)) / med, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trk_planes_times.json"))
    args = ap.parse_args()
    from oracle import oracle as O
    from gnss_sdr_rs_amd import _lib, synth, tracking as T
    _lib.init(0)
    table = O.ca_code_table()
    prns = list(range(1, CHANNELS + 1))
    ms = EPOCHS + 2
    planes, starts = [], []
    for p, prn in enumerate(prns):                       # plane p holds satellite p alone; the plain ring holds their sum
        sc = synth.tracking_scene(table, FS, 0.0, [prn], ms, config_id=700 + p, cn0=47.0, quantize=False)
        planes.append(synth.to_c32(sc["x"]))
        s = sc["sats"][0]
        starts.append(dict(prn=prn, code_phase_samples=0, code_phase_chips=0.0, carrier_freq=s["doppler_hz"] + 20.0, fs=FS, mag_relative=10.0,
                           sample_global_index=s["code_start"], doppler_bin=0))
    x = np.ascontiguousarray(np.stack(planes))
    pr = T.PlaneRing(CHANNELS, 1 << 19)
    pr.write(x)
    ring = T.MulticastRingBuffer(1 << 19)
    ring.write_samples(x.sum(axis=0).astype(np.complex64))
    on_planes = T.TrackingManager(FS, n_channels=CHANNELS, code_index_mode=T.CODE_INDEX_FIXED)
    on_ring = T.TrackingManager(FS, n_channels=CHANNELS, code_index_mode=T.CODE_INDEX_FIXED)
    on_planes.set_channel_planes(list(range(CHANNELS)))
    for m in (on_planes, on_ring):
        for i, r in enumerate(starts):
            m.channels[i].start(r)
        m.enable_timing(True)
    start_states = on_planes.get_states()

    def timed(m, launch):
        m.set_states(start_states)
        launch()
        m.synchronize()
        ms_total, passes = m.last_timing()
        assert passes == EPOCHS
        assert all(s.next_sample_index == r["sample_global_index"] + EPOCHS * N for s, r in zip(m.get_states(), starts))      # every pass ran
        return ms_total

    def planes_call():
        return timed(on_planes, lambda: on_planes.update_planes_dev(pr, EPOCHS))

    def ring_call():
        return timed(on_ring, lambda: on_ring.update_all_dev(ring, EPOCHS))

    for _ in range(WARMUP):
        planes_call()
        ring_call()
    t_planes, t_ring = [], []
    for _ in range(REPEATS):
        t_planes.append(planes_call())
        t_ring.append(ring_call())
    row = dict(channels=CHANNELS, planes=CHANNELS, epochs=EPOCHS, fs=FS, samples_per_epoch=N, update_planes_dev=_stats(t_planes),
               update_all_dev_one_ring=_stats(t_ring), planes_over_ring=round(float(np.median(t_planes)) / float(np.median(t_ring)), 4),
               real_time_ms=EPOCHS * 1.0, faster_than_real_time=bool(max(t_planes) < EPOCHS * 1.0))
    print(json.dumps(row), flush=True)
    on_planes.close(); on_ring.close(); pr.close(); ring.close()
    meta = dict(tool="tools/trk_planes_time.py", repeats=REPEATS, warmup_calls=WARMUP,
                timing="the handle's event pair around one call of 16 passes (gm_trk_last_timing), the same start states before every call: "
                       "gm_trk_update_planes_dev, 15 channels on 15 planes, and gm_trk_update_all_dev of a twin handle on one plain ring that "
                       "holds the 15 satellites' sum; one process, one warm-up call each, five repeats with the two alternating; median and "
                       "spread = (max - min) / median")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(meta=meta, result=row), f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
