#!/usr/bin/env python3
"""bench.py — the hot path of BASELINE.json on N GPUs of one node (one process per GPU).

Workload at N = 1: BASELINE.json configs[1] — GPS L1 C/A, 32 PRN x 41 Doppler bins (+-5 kHz / 250 Hz),
8 Msps complex int8, 10 x 1 ms non-coherent (the reference's LONG_SAMPLES_LENGTH).  A "step" is one
acquisition dwell: stage F (carrier mix + forward FFT, shared by all PRNs) + stage C (x conj(code
spectrum), inverse FFT, |.|^2 accumulated over the 10 ms, {max, argmax, sum} per (PRN, bin)) + the
reference's decision replay, with the IF samples already resident in HBM.  `value` = (PRN, Doppler,
code-phase) cells decided per second over all ranks.

N > 1 (weak scaling, the shape of configs[3]): every rank searches its own 32-code block of a 32*N-code
grid on the same IF snapshot, then ONE all-gather (RCCL, torch.distributed) of the per-(code, bin)
{max, argmax, sum} metrics, and every rank replays the decision on the gathered grid.

A plain run sets up, warms up, times --steps dwells and prints the line, whose `roofline` comes from HIP events
recorded inside the timed region on the stream the kernels run on.  With --full it also measures what is not
part of `value`, each in runs of its own: the tracking leg of configs[2] (32 channels, 25 Msps, E/P/L +
DLL/PLL), the other BASELINE geometries, the receiver chain, the front-end, the measured copy ceiling and the
CPU oracle ("port" of the reference) timed on this host's cores.

--dump-outputs DIR writes what the last timed dwell computed, as a caller of the path receives it, to DIR/*.npy
(float32 / float64): the {max, argmax, sum} metrics per (PRN, bin) and the decision per PRN.  The inputs are
seeded, so two runs with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured float4 copy)
FP32_VALU_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: peak FP32 vector (256 CUs x 4 SIMD-32 x 2 flop x 2.4 GHz)
VALU_NS_PER_WAVE_INST = 1.02    # measured: one wave64 f32 VALU instruction per SIMD per 1.0-1.1 ns at 4 waves/SIMD (tools/ubench/valu_forms)


def gold_codes(delays):
    """Gold codes of the GPS C/A family for arbitrary G2 delays (the extra code blocks of ranks > 0)."""
    def lfsr(taps):
        reg = [1] * 10
        out = np.zeros(1023, np.uint8)
        for i in range(1023):
            out[i] = reg[9]
            fb = 0
            for t in taps:
                fb ^= reg[t - 1]
            reg = [fb] + reg[:9]
        return out
    g1, g2 = lfsr([3, 10]), lfsr([2, 3, 6, 8, 9, 10])
    return np.stack([np.where(g1 ^ np.roll(g2, d), 1, -1).astype(np.int8) for d in delays])


def rank_commands(n_gpus, argv, port, base_env=None, python=None, script=None):
    """The N child processes `python3 bench.py --gpus N ...` starts when no launcher set WORLD_SIZE: one per GPU, the
    environment torch.distributed.run would give them (RANK / LOCAL_RANK / WORLD_SIZE / LOCAL_WORLD_SIZE / MASTER_ADDR /
    MASTER_PORT; rendezvous on 127.0.0.1 — the container hostname may not resolve).  Returns [(argv, env)], rank order.
    The reference's counterpart is the rayon fan-out over its workers (do_acquisition.rs:302-313)."""
    env0 = dict(os.environ if base_env is None else base_env)
    env0.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL between processes needs it on this driver
    cmds = []
    for r in range(n_gpus):
        env = dict(env0)
        env.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(n_gpus), "LOCAL_WORLD_SIZE": str(n_gpus),
                    "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "GM_BENCH_LAUNCHED_BY_PARENT": "1"})
        cmds.append(([python or sys.executable, script or os.path.abspath(__file__)] + list(argv), env))
    return cmds


def _visible_filter(n, env=None):
    """Apply HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES / CUDA_VISIBLE_DEVICES (index lists) to a count of n physical devices."""
    env = os.environ if env is None else env
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = env.get(var)
        if v is None:
            continue
        ids = [t.strip() for t in v.split(",") if t.strip() != ""]
        if all(t.lstrip("-").isdigit() for t in ids):
            keep = []
            for t in ids:                       # the runtime stops at the first invalid index
                if not (0 <= int(t) < n):
                    break
                keep.append(int(t))
            n = len(set(keep))
        # (UUID lists: left alone — every listed device is assumed present)
        elif ids:
            n = min(n, len(ids))
    return n


def visible_gpus(sysfs="/sys/class/kfd/kfd/topology/nodes", env=None):
    """Devices this process could hand to its ranks, counted WITHOUT touching HIP: the KFD topology in sysfs (a node with
    simd_count > 0 is a GPU), filtered by the *_VISIBLE_DEVICES variables.  The launcher starts its ranks as child processes and
    must not hold a GPU context of its own; torch.cuda.device_count() may fall back to hipGetDeviceCount (which initialises HIP)
    on builds without amdsmi, so it is asked only in a short-lived child process when sysfs is not there."""
    n = None
    try:
        n = 0
        for node in sorted(os.listdir(sysfs)):
            try:
                props = dict(l.split(None, 1) for l in open(os.path.join(sysfs, node, "properties")).read().splitlines() if " " in l)
            except OSError:
                continue
            if int(props.get("simd_count", "0")) > 0:
                n += 1
    except OSError:
        n = None
    if n is None:
        import subprocess
        try:
            r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], stdout=subprocess.PIPE,
                               stderr=subprocess.DEVNULL, timeout=300, text=True)
            return int(r.stdout.strip().splitlines()[-1])       # (the child applied the visibility variables itself)
        except Exception:
            return 0
    return _visible_filter(n, env)


def launch_ranks(n_gpus, argv, timeout_s, script=None, have=None, grace_s=30.0):
    """Start the N ranks, relay rank 0's stdout (its JSON line is this process's last stdout line), send the other ranks'
    stdout to stderr, and return the worst exit code.  A rank that dies ends the others after a grace period (they would
    wait in a collective for ever); so does the deadline.  No os.exec*: children are plain subprocesses."""
    import signal
    import socket
    import subprocess
    import threading
    debug_gloo = os.environ.get("GM_BENCH_DEBUG_GLOO") == "1"
    have = visible_gpus() if have is None else have
    if (have < 1) or (have < n_gpus and not debug_gloo):
        print("bench.py: --gpus %d asked for, %d GPU(s) visible%s" % (n_gpus, have, "" if have else " (none at all)") +
              "; set GM_BENCH_DEBUG_GLOO=1 to rehearse the N-rank code path on one GPU (never a reported number)",
              file=sys.stderr, flush=True)
        return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r, (cmd, env) in enumerate(rank_commands(n_gpus, argv, port, script=script)):
        procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE if r == 0 else sys.stderr, stderr=sys.stderr,
                           text=True, start_new_session=True))

    def relay(f):
        for line in f:
            sys.stdout.write(line)
            sys.stdout.flush()
    t = threading.Thread(target=relay, args=(procs[0].stdout,), daemon=True)
    t.start()

    def end_all(sig):
        for p in procs:
            if p.poll() is None:
                try:
                    os.killpg(p.pid, sig)       # the exact process groups started above, never a pattern
                except (ProcessLookupError, PermissionError):
                    pass
    deadline = time.monotonic() + timeout_s
    first_failure, why = None, None
    while any(p.poll() is None for p in procs):
        now = time.monotonic()
        bad = [p for p in procs if p.poll() not in (None, 0)]
        if bad and first_failure is None:
            first_failure = now
        if first_failure is not None and now - first_failure > grace_s:
            why = "a rank exited with code %d; ending the others" % bad[0].returncode
        elif now > deadline:
            why = "the ranks did not finish within %.0f s (--launch-timeout); ending them" % timeout_s
        if why:
            print("bench.py launcher: " + why, file=sys.stderr, flush=True)
            end_all(signal.SIGTERM)
            time.sleep(5.0)
            end_all(signal.SIGKILL)
            break
        time.sleep(0.2)
    codes = [p.wait() for p in procs]
    t.join(timeout=10.0)
    worst = max((abs(c) for c in codes), default=0)
    return worst if not why else (worst or 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-tracking", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="CPU-baseline budget (bounded sample)")
    ap.add_argument("--three-dwells", action="store_true",
                    help="also time three dwells in flight on three streams (informative; off by default because the "
                         "co-executing launches would pollute the per-kernel averages of a rocprofv3 --stats run)")
    ap.add_argument("--launch-timeout", type=float, default=float(os.environ.get("GM_BENCH_LAUNCH_TIMEOUT", "1500")),
                    help="--gpus N > 1 started without a launcher: seconds the parent waits for its N ranks before it ends them")
    ap.add_argument("--full", action="store_true",
                    help="also run the informative legs (tracking, receiver chain, other geometries, front-end, copy ceiling, "
                         "host-buffer API, CPU baselines); a plain run times the headline dwell only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed to DIR/<name>.npy")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # started plainly (`python3 bench.py --gpus N`), not under torch.distributed.run: this process becomes the launcher
        # and never touches the GPU (no torch.cuda call that initialises it, no gm_* call, no exec)
        sys.exit(launch_ranks(args.gpus, sys.argv[1:], args.launch_timeout))

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # GM_BENCH_DEBUG_GLOO=1: rehearse the N > 1 code path on ONE GPU (all ranks on cuda:0, gloo exchange through host
    # memory); RCCL refuses two ranks on one device.  Never used for reported numbers.
    debug_gloo = os.environ.get("GM_BENCH_DEBUG_GLOO") == "1"
    if debug_gloo:
        local_rank = 0
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if debug_gloo:
            dist.init_process_group(backend="gloo")
        else:
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
    assert world == args.gpus or world == 1, "launch with torch.distributed.run --nproc-per-node == --gpus"
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    from gnss_sdr_rs_amd import _lib, acquisition as A, synth, tracking as T
    _lib.init(local_rank)                      # raises if the HIP library is missing: no fallback
    # inputs: SURVEY §8 d2's C++ generator (splitmix64-seeded xoshiro256**, Box-Muller; gnss-sdr-rs_amd/synthgen) unless told
    # otherwise — identical bytes on every rank and every box for a given seed, no numpy version in the loop
    if "GM_SYNTH_GENERATOR" not in os.environ:
        synth.DEFAULT_GENERATOR = "xoshiro"

    # ------------------------------------------------------------------ the whole receiver chain, informative — FIRST.
    # The chain lives on four or five streams of its own (ring copies, front-end, tracking, acquisition + its side stream) that must
    # run beside each other.  HIP deals a process's streams to its hardware queues in creation order (GPU_MAX_HW_QUEUES, 4), and the
    # first torch.cuda.Stream() of a process creates torch's whole pool of them: measured on one box, the same chain runs at 217 x real
    # time in a process that has created no other stream and at 118 - 190 x behind four torch streams (tools/rx_order_probe.py: two of
    # the chain's streams then share a queue and the front-end kernel holds the tracking launches back).  The library now gives the ring's
    # copy stream the lowest and the front-end stream the highest priority (their own queues: 216 x behind four torch streams, 220 x without);
    # the leg still runs first — a receiver process creates its receiver's streams first.
    receiver_first = None
    if args.full and rank == 0 and world == 1 and os.environ.get("GM_BENCH_NO_RECEIVER") != "1":
        try:
            receiver_first = receiver_leg(A.ca_code_table(), A, T, synth, not args.no_cpu_baseline)
        except Exception as e:
            receiver_first = {"error": repr(e)}

    # one explicit stream for everything this process enqueues (library kernels through gm_*_set_stream, torch's copies and
    # collectives through torch's current stream): nothing relies on the NULL stream's implicit ordering
    bench_stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(bench_stream)

    # ------------------------------------------------------------------ acquisition workload (configs[1])
    ca = A.ca_code_table()
    sc = synth.cfg2_scene(ca)
    P, D, N, M = 32, int(sc["doppler_hz"].size), sc["N"], sc["M"]
    xi8 = synth.to_i8_iq(sc["x"])
    if rank == 0:
        eng = A.AcquisitionEngine(sc["fs"], sc["f_if"], N, doppler_hz=sc["doppler_hz"], n_integrations=M)
        prn_ids_local = np.arange(1, 33, dtype=np.uint8)
    else:   # further code blocks of the grid: other members of the same Gold family
        gps = {5, 6, 7, 8, 17, 18, 139, 140, 141, 251, 252, 254, 255, 256, 257, 258, 469, 470, 471, 472, 473, 474, 509,
               512, 513, 514, 515, 516, 859, 860, 861, 862}
        free = [d for d in range(1, 1023) if d not in gps]
        delays = free[(rank - 1) * 32:(rank - 1) * 32 + 32]
        prn_ids_local = np.arange(1, 33, dtype=np.uint8)
        eng = A.AcquisitionEngine(sc["fs"], sc["f_if"], N, doppler_hz=sc["doppler_hz"], n_integrations=M,
                                  prn_ids=prn_ids_local, codes=gold_codes(delays))
    stream = torch.cuda.current_stream().cuda_stream
    eng.set_stream(stream)
    d_samples = torch.from_numpy(xi8).to(dev)                       # IF snapshot resident in HBM
    d_metrics = torch.zeros(3 * P * D, dtype=torch.int32, device=dev)
    # The exchange carrier.  torch.distributed (backend nccl = RCCL) is the default at N > 1.  GM_BENCH_NATIVE_COMM=1 opts in
    # to the C ABI's own RCCL communicator (gm_comm_*: what a Rust host calls — all-gather + regroup inside the library,
    # overlapped with the next dwell on the communicator's stream); it also exercises that carrier at N = 1.  Before the timed
    # region one dwell then goes through BOTH carriers — the native one through the SAME asynchronous entries the timed loop
    # uses (gm_acq_allgather_metrics_async + gm_comm_wait + the device decision) — and the native result must equal
    # torch.distributed's bit for bit and give the scene's detections on every rank, else (or on any error) the run falls back
    # to torch.distributed and says so in config.exchange_fallback_reason.  gm_comm stays opt-in until one multi-GPU run of it
    # is on record (no multi-GPU box has run either carrier yet).
    from gnss_sdr_rs_amd import distributed as Dm
    native_comm, carrier_note = None, None
    want_native = os.environ.get("GM_BENCH_NATIVE_COMM") == "1"
    if want_native and not debug_gloo:
        try:
            native_comm = Dm.NativeComm.from_torch_dist() if world > 1 else Dm.NativeComm(1, 0, Dm.NativeComm.unique_id())
        except Exception as e:
            native_comm, carrier_note = None, "gm_comm_init failed: %r" % (e,)
    if world > 1 or native_comm:
        d_gather = torch.zeros(world * 3 * P * D, dtype=torch.int32, device=dev)
        ids_all = np.tile(np.arange(1, 33, dtype=np.uint8), world)
    if world > 1:
        met2 = [d_metrics, torch.zeros_like(d_metrics)]
        gat2 = [d_gather, torch.zeros_like(d_gather)]
    if world > 1 and not debug_gloo:
        ok = 1
        if native_comm:
            try:
                eng.search_dev(d_samples.data_ptr(), A.FMT_I8_IQ, d_metrics.data_ptr())
                native_comm.allgather_metrics_async(eng, gat2[1].data_ptr(), d_metrics.data_ptr())   # -> [3][world*P][D]
                native_comm.wait(stream)
                eng.decide_dev(gat2[1].data_ptr(), n_prn=world * P, prn_ids=ids_all)
                ref = torch.empty_like(d_gather)
                dist.all_gather_into_tensor(ref, d_metrics)
                torch.cuda.synchronize()
                ok = int(torch.equal(ref.view(world, 3, P * D).permute(1, 0, 2).contiguous().view(-1), gat2[1]))
                if not ok:
                    carrier_note = "gm_comm all-gather differed from torch.distributed's"
                else:
                    tr = eng.fetch_results(world * P)
                    want = {s_["prn"]: s_["code_start"] for s_ in sc["sats"]}
                    if {r_["prn"]: r_["code_phase_samples"] for r_ in tr[:P] if r_} != want or any(r_ is not None for r_ in tr[P:]):
                        ok, carrier_note = 0, "the decision on gm_comm's gathered grid did not give the scene's detections"
            except Exception as e:
                ok, carrier_note = 0, "gm_comm trial failed: %r" % (e,)
        else:
            ok = 0
        flag = torch.tensor([ok], dtype=torch.int32, device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)          # one carrier for every rank
        if int(flag.item()) == 0 and native_comm:
            native_comm.close()
            native_comm = None
            carrier_note = carrier_note or "another rank could not use gm_comm"

    # N > 1: the exchange of dwell i overlaps the search of dwell i + 1 — the all-gather is issued behind search(i) on the
    # carrier's own stream, and regroup + decision of dwell i are enqueued after search(i + 1).  Metrics / gather buffers
    # alternate.  Every timed step is still issued AND finished inside the region.
    def issue(i):
        k = i & 1
        eng.search_dev(d_samples.data_ptr(), A.FMT_I8_IQ, met2[k].data_ptr())
        if debug_gloo:       # rehearsal only: exchange through host memory (synchronous)
            h = [torch.empty(3 * P * D, dtype=torch.int32) for _ in range(world)]
            dist.all_gather(h, met2[k].cpu())
            gat2[k].copy_(torch.cat(h))
            return None, k
        return dist.all_gather_into_tensor(gat2[k], met2[k], async_op=True), k    # the path's one exchange step

    def finish(pending):
        work, k = pending
        if work is not None:
            work.wait()      # the current stream waits for the collective; the host does not
        g = gat2[k].view(world, 3, P * D).permute(1, 0, 2).contiguous()            # -> [3][world*P][D]
        eng.decide_dev(g.data_ptr(), n_prn=world * P, prn_ids=ids_all)
        return g

    overlap = {"on": os.environ.get("GM_BENCH_NO_OVERLAP") != "1"}

    def run(n_steps):
        keep = None
        if world > 1 and native_comm:
            # search(i) | wait gather(i-1), decide(i-1) | gather(i) on the communicator's stream, beside search(i+1)
            for i in range(n_steps):
                k = i & 1
                eng.search_dev(d_samples.data_ptr(), A.FMT_I8_IQ, met2[k].data_ptr())
                if overlap["on"]:
                    if i > 0:
                        native_comm.wait(stream)
                        eng.decide_dev(gat2[k ^ 1].data_ptr(), n_prn=world * P, prn_ids=ids_all)
                    native_comm.allgather_metrics_async(eng, gat2[k].data_ptr(), met2[k].data_ptr())
                else:
                    native_comm.allgather_metrics(eng, gat2[k].data_ptr(), met2[k].data_ptr())
                    eng.decide_dev(gat2[k].data_ptr(), n_prn=world * P, prn_ids=ids_all)
            if overlap["on"] and n_steps > 0:
                native_comm.wait(stream)
                eng.decide_dev(gat2[(n_steps - 1) & 1].data_ptr(), n_prn=world * P, prn_ids=ids_all)
            return keep
        if world > 1 and overlap["on"]:
            try:
                prev = None
                for i in range(n_steps):
                    cur = issue(i)
                    if prev is not None:
                        keep = finish(prev)
                    prev = cur
                if prev is not None:
                    keep = finish(prev)
                return keep
            except Exception as e:      # never lose the N > 1 measurement to the overlap: fall back to the plain order
                overlap["on"] = False
                if rank == 0:
                    print(f"overlapped exchange failed ({e!r}); using the synchronous order", file=sys.stderr, flush=True)
        if world > 1:
            for i in range(n_steps):    # search -> all-gather -> regroup -> decision, in order on one stream
                work, k = issue(i)
                keep = finish((work, k))
            return keep
        for _ in range(n_steps):
            eng.search_dev(d_samples.data_ptr(), A.FMT_I8_IQ, d_metrics.data_ptr())
            if native_comm:      # all-gather + regroup inside the library, on the handle's stream
                native_comm.allgather_metrics(eng, d_gather.data_ptr(), d_metrics.data_ptr())
                eng.decide_dev(d_gather.data_ptr(), n_prn=world * P, prn_ids=ids_all)
            else:
                eng.decide_dev(d_metrics.data_ptr())
        eng.synchronize()        # runs the last dwell's decision if it is still pending (set_deferred_decision): all n_steps decisions are inside
        return keep

    if world == 1 and os.environ.get("GM_BENCH_NO_DEFER") != "1":
        eng.set_deferred_decision(True)      # back-to-back dwells: dwell k's decision runs beside dwell k+1's forward transforms
    keep = run(args.warmup)
    torch.cuda.synchronize()
    # every 5th dwell carries HIP events (four records cost ~8 us of stream time per dwell when all are timed)
    eng.enable_timing(0 if os.environ.get("GM_BENCH_NO_EVENTS") == "1" else 5)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    keep = run(args.steps)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    try:
        tsum = eng.timing_summary()
    except Exception:      # GM_BENCH_NO_EVENTS=1 (diagnostic): no per-kernel timing
        tsum = {"avg_corr_ms": 0.0, "avg_mix_fft_ms": 0.0, "launches": 0}
    eng.enable_timing(False)
    if world > 1:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())

    if args.dump_outputs and rank == 0:
        # the metrics block the last timed dwell's decision read, and that decision
        if world > 1:
            grid = gat2[(args.steps - 1) & 1] if native_comm else keep
        else:
            grid = d_gather if native_comm else d_metrics
        dump_outputs(args.dump_outputs, grid, eng.fetch_results(world * P), world * P, D)

    # the exchange alone (all-gather + regroup of the 3*P*D-word blocks, no search in front), in order on the stream:
    # what a dwell would pay for it without the overlap
    exchange_us = None
    if world > 1 and args.full:
        try:
            def xchg():
                if debug_gloo:      # rehearsal: through host memory
                    h = [torch.empty(3 * P * D, dtype=torch.int32) for _ in range(world)]
                    dist.all_gather(h, met2[0].cpu())
                    gat2[0].copy_(torch.cat(h))
                elif native_comm:
                    native_comm.allgather_metrics(eng, gat2[0].data_ptr(), met2[0].data_ptr())
                else:
                    dist.all_gather_into_tensor(gat2[0], met2[0])
                    gat2[0].view(world, 3, P * D).permute(1, 0, 2).contiguous()
            for _ in range(5):
                xchg()
            torch.cuda.synchronize()
            dist.barrier()
            tx = time.perf_counter()
            for _ in range(50):
                xchg()
            torch.cuda.synchronize()
            txe = torch.tensor([(time.perf_counter() - tx) / 50 * 1e6], dtype=torch.float64, device="cpu" if debug_gloo else dev)
            dist.all_reduce(txe, op=dist.ReduceOp.MAX)
            exchange_us = float(txe.item())
        except Exception as e:
            exchange_us = repr(e)

    # detections must be the simulated satellites (rank 0's block), every step's result identical by construction
    res = eng.fetch_results(world * P if world > 1 else P)
    truth = {s["prn"]: s["code_start"] for s in sc["sats"]}
    got = {r["prn"]: r["code_phase_samples"] for r in res[:P] if r}
    detections_ok = (got == truth) and all(r is None for r in res[P:])

    cells_per_step = world * P * D * N
    value = cells_per_step * args.steps / elapsed
    # roofline of the dominant kernel: algorithmic bytes per launch (SURVEY §8d stage C): P*D*M*N*16
    corr_bytes = P * D * M * N * 16
    mix_bytes = D * M * N * (2 + 8)
    corr_s = tsum["avg_corr_ms"] * 1e-3
    achieved = corr_bytes / corr_s / 1e9 if corr_s > 0 else 0.0
    # measured fabric traffic and SQ counters of this kernel: collected by separate rocprofv3 --pmc passes of this same
    # command (tools/profile_round.sh) and committed under profiles/ — read from there, not measured by this run
    traffic, sq = None, None
    try:
        traffic = json.load(open(os.path.join(ROOT, "profiles", "traffic.json"))).get("acq_corr_kernel_hbm_bytes_per_launch")
    except Exception:
        traffic = None
    try:
        sq = json.load(open(os.path.join(ROOT, "profiles", "sq_counters.json")))["gm::acq_corr_kernel"]
    except Exception:
        sq = None
    n_transforms = P * D * M
    # useful flops per launch: 5 N log2 N per transform (the usual FFT convention) + 6 N (x conj(code), num-complex order)
    # + 4 N (|.|^2 and the accumulation)
    flops = n_transforms * (5.0 * N * np.log2(N) + 10.0 * N)
    compute = {"bound": "valu-f32", "achieved": flops / corr_s / 1e12 if corr_s > 0 else 0.0, "peak": FP32_VALU_PEAK_TFLOPS,
               "unit": "TFLOP/s", "flops_per_launch": flops, "transforms_per_launch": n_transforms,
               "flop_model": "5*N*log2(N) + 10*N per inverse transform of N = %d" % N}
    compute["frac"] = compute["achieved"] / FP32_VALU_PEAK_TFLOPS
    if sq and corr_s > 0:
        insts = sq.get("SQ_INSTS_VALU")
        if insts:
            compute["valu_wave_insts_per_launch"] = insts
            compute["valu_wave_insts_per_transform"] = insts / n_transforms
            # a gfx950 SIMD issues one wave64 f32 VALU instruction per 2 cycles with >= 2 waves resident
            # (MI355X_MICROARCH.md; tools/ubench/valu_forms: 1.0-1.1 ns per instruction per SIMD at 4 waves, every CU busy)
            compute["valu_issue_frac"] = insts / 1024.0 * VALU_NS_PER_WAVE_INST * 1e-9 / corr_s
            compute["valu_issue_model"] = "insts / 1024 SIMDs x %.2f ns (profiles/r02_ubench_valu_forms.txt) / kernel time" % VALU_NS_PER_WAVE_INST
        for k in ("SQ_WAVE_CYCLES", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY", "SQ_INSTS_LDS", "SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE"):
            if k in sq:
                compute[k] = sq[k]
        compute["counters_source"] = "profiles/sq_counters.json (rocprofv3 --pmc passes of this command, per-launch averages)"
    out = {
        "metric": "acq PRN×Doppler cells/s + tracking ch×Msps at 1/2/4/8 GPU; % HBM roofline",
        "value": value, "unit": "cells/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic" + (" (DEBUG gloo rehearsal, one GPU shared)" if debug_gloo else ""),
        "data_generator": synth.DEFAULT_GENERATOR + (" (C++: splitmix64-seeded xoshiro256**, Box-Muller; seed 0x6E5553445200 + config id)" if synth.DEFAULT_GENERATOR == "xoshiro" else ""),
        "config": {"workload": "GPS L1 C/A 32-PRN x +-5 kHz/250 Hz (41 bins) acquisition, 8 Msps complex int8, "
                               "N=8000, 10 x 1 ms non-coherent, per GPU" + ("; all-gather of {max,argmax,sum}[P][D]" if world > 1 else ""),
                   "prns_per_gpu": P, "doppler_bins": D, "fft_size": N, "integrations": M,
                   "cells_per_step": cells_per_step, "cell_integrations_per_s": value * M,
                   "parallelism": f"prn-shard x{world}", "exchange_overlapped_with_next_dwell": bool(world > 1 and overlap["on"] and not debug_gloo),
                   "exchange": ("gm_comm (RCCL through the C ABI: gm_acq_allgather_metrics_async + gm_comm_wait)" if (native_comm and world > 1)
                                else "gm_comm (one rank)" if native_comm else "gloo through host memory (rehearsal)" if (world > 1 and debug_gloo)
                                else "torch.distributed nccl" if world > 1 else None),
                   "exchange_fallback_reason": carrier_note, "exchange_us_per_dwell": exchange_us,
                   "detections_ok": bool(detections_ok)},
        # the binding roof of the dominant kernel is f32 VALU issue.  (Matrix instructions ARE used on this path where a pass is a
        # dense contraction — the radix-31 pass of N = 16368, csrc/ws31_core.h — but not in this kernel: every pass of N = 8000 has a
        # fast algorithm, and v_mfma_f32_16x16x4_f32 holds its SIMD's vector issue for its whole duration, so the dense form of the
        # radix-16 pass is 3 x the issue time of the vector form: tools/corr_lab/mfma16_8000, profiles/r05_ubench_mfma_coissue.txt.)
        # SURVEY 8d's algorithmic-byte model sits beside it as `hbm_model`, without a `frac` of a physical peak: it counts
        # every worker's re-read of a Doppler bin's spectra (P x) as HBM bytes, and on the chip those are L2 hits
        "roofline": {"bound": "valu-f32", "kernel": "acq_corr_kernel", "achieved": compute["achieved"], "peak": FP32_VALU_PEAK_TFLOPS,
                     "unit": "TFLOP/s", "frac": compute["frac"], "issue_frac": compute.get("valu_issue_frac"),
                     "traffic": traffic,
                     "traffic_source": "profiles/traffic.json (2 x FETCH_SIZE + WRITE_SIZE, separate --pmc passes of this command, launches of the benchmarked grid size only)",
                     "traffic_over_algorithmic": (traffic / corr_bytes) if traffic else None,
                     "fabric_GBs": (traffic / corr_s / 1e9) if (traffic and corr_s > 0) else None,
                     "fabric_frac_of_hbm_peak": (traffic / corr_s / 1e9 / HBM_PEAK_GBS) if (traffic and corr_s > 0) else None,
                     "reading": "frac = useful f32 flops (5 N log2 N + 10 N per inverse transform) / kernel time / the 157.3 TF vector "
                                "peak; issue_frac = VALU wave-instructions x 1.02 ns per SIMD / kernel time (the share of the f32 issue "
                                "slots the kernel fills; f32 matrix instructions share that issue port — measured, tools/corr_lab/mfma16_8000 — "
                                "and are used only for the dense radix-31 pass of N = 16368); traffic = measured fabric bytes per launch (a few % "
                                "of the HBM peak: the kernel is not HBM-bound); hbm_model = SURVEY 8d's algorithmic bytes / time, a model figure that "
                                "can exceed the 8 TB/s peak because the re-reads it counts are served by L2",
                     "compute": compute,
                     "hbm_model": {"algorithmic_bytes_per_launch": corr_bytes, "model_GBs": achieved, "hbm_peak_GBs": HBM_PEAK_GBS,
                                   "model_over_peak": achieved / HBM_PEAK_GBS,
                                   "note": "16 B per (PRN, bin, ms, k): not a fraction of a physical roof"},
                     # the physical path those algorithmic bytes DO take: L2 -> CU through the load path, which streams cache-resident
                     # 16-byte loads at 125 GB/s per CU (tools/ubench/l2_read.hip, profiles/r04_ubench_l2_read.txt)
                     "load_path": {"bytes_per_launch": corr_bytes, "achieved_GBs_per_cu": achieved / 256.0, "measured_peak_GBs_per_cu": 125.0,
                                   "frac": achieved / 256.0 / 125.0,
                                   "note": "the kernel's loads (spectrum + code spectrum, 16 B per cell and integration) against the measured L2-resident read rate of a CU: the second busiest resource after vector issue"},
                     "avg_launch_ms": tsum["avg_corr_ms"], "launches_timed": tsum["launches"],
                     "stage_F": {"kernel": "acq_mix_fft_kernel", "algorithmic_bytes_per_launch": mix_bytes,
                                 "avg_launch_ms": tsum["avg_mix_fft_ms"],
                                 "algorithmic_GBs": (mix_bytes / (tsum["avg_mix_fft_ms"] * 1e-3) / 1e9) if tsum["avg_mix_fft_ms"] > 0 else None},
                     "whole_step_algorithmic_GBs": (corr_bytes + mix_bytes) * args.steps / elapsed / 1e9},
    }
    del keep
    # the informative legs below run with --full only (--three-dwells: its own switch); a plain run measures the headline
    if args.full and rank == 0 and world == 1:
        try:
            c = hbm_ceiling(torch, dev)
            out["roofline"]["measured_d2d_copy_GBs"] = c      # the measured copy ceiling beside the 8 TB/s peak
        except Exception as e:
            out["roofline"]["measured_d2d_copy_GBs"] = repr(e)
    if args.full and rank == 0:
        # the drop-in host-buffer entry (gm_acq_search: H2D of the 160 KB snapshot + kernels + D2H of results);
        # PCIe-inclusive, reported for DESIGN.md, never `value`
        eng.search(xi8)
        t1 = time.perf_counter()
        for _ in range(20):
            eng.search(xi8)
        out["config"]["host_buffer_api_ms_per_dwell"] = (time.perf_counter() - t1) / 20 * 1e3
        # fine-Doppler refinement of the detections (2^20-point zero-padded FFT per satellite), informative
        try:
            r_host = eng.search(xi8)
            fine = eng.finer_doppler(r_host)
            t1 = time.perf_counter()
            for _ in range(10):
                fine = eng.finer_doppler(r_host)
            errs = [abs(f["freq_hz"] - (sc["f_if"] + s["doppler_hz"])) for s in sc["sats"] for f in [fine[s["prn"] - 1]] if f]
            out["fine_doppler"] = {"satellites": len(errs), "fft_size": fine[sc["sats"][0]["prn"] - 1]["fft_size"],
                                   "ms_per_call": (time.perf_counter() - t1) / 10 * 1e3, "max_abs_error_hz": max(errs)}
        except Exception as e:
            out["fine_doppler"] = {"error": repr(e)}

    # ------------------------------------------------------------------ configs[1] with ONE integration ("also report M = 1")
    if args.full and rank == 0 and world == 1:
        try:
            out["cfg2_single_integration"] = m1_leg(torch, dev, stream, sc, A, synth, xi8)
        except Exception as e:
            out["cfg2_single_integration"] = {"error": repr(e)}

    # ------------------------------------------------------------------ three dwells in flight (informative, never `value`)
    if rank == 0 and world == 1 and args.three_dwells:
        try:
            out["config"]["three_dwells_in_flight"] = pipelined_leg(torch, dev, sc, A, d_samples, P, D, N, M)
        except Exception as e:
            out["config"]["three_dwells_in_flight"] = {"error": repr(e)}

    # ------------------------------------------------------------------ configs[3]'s Galileo part (informative, no reference code)
    if args.full and rank == 0 and world == 1:
        try:
            out["cfg4_galileo_geometry"] = cfg4_leg(torch, dev, A, synth)
        except Exception as e:
            out["cfg4_galileo_geometry"] = {"error": repr(e)}

    # ------------------------------------------------------------------ configs[3] as written: the 90-code mixed grid, sharded
    if args.full and os.environ.get("GM_BENCH_NO_GRID") != "1":
        try:
            g4 = cfg4_grid_leg(torch, dev, stream, ca, A, synth, world, rank, dist, debug_gloo, native_comm)
            if rank == 0:
                out["cfg4_grid"] = g4
        except Exception as e:
            if rank == 0:
                out["cfg4_grid"] = {"error": repr(e)}

    # ------------------------------------------------------------------ configs[0] geometry on the GPU (informative)
    if args.full and rank == 0 and world == 1:
        try:
            out["cfg1_geometry"] = cfg1_leg(torch, dev, stream, ca, A, synth, with_cpu=not args.no_cpu_baseline)
        except Exception as e:
            out["cfg1_geometry"] = {"error": repr(e)}

    # ------------------------------------------------------------------ tracking leg (configs[2]), rank-local
    if args.full and not args.no_tracking:
        try:
            out["tracking"] = tracking_leg(torch, dev, stream, ca, T, synth, world, dist,
                                           0.0 if (args.no_cpu_baseline or rank != 0) else min(args.cpu_seconds, 8.0))
        except Exception as e:   # the headline number stands on its own
            out["tracking"] = {"error": repr(e)}

    # ------------------------------------------------------------------ the same kernel with 256 channels (informative)
    if args.full and rank == 0 and world == 1 and not args.no_tracking and os.environ.get("GM_BENCH_NO_TRK256") != "1":   # (off in the counter passes: same grid size as C = 32)
        try:
            t256 = tracking_leg(torch, dev, stream, ca, T, synth, 1, dist, 0.0, C=256)
            out["tracking_256ch"] = {k: t256[k] for k in ("value", "unit", "channels_per_gpu", "ms_per_epoch", "channels_locked", "roofline")}
        except Exception as e:
            out["tracking_256ch"] = {"error": repr(e)}

    # ------------------------------------------------------------------ configs[4] geometry (informative, no reference code)
    if args.full and not args.no_tracking and os.environ.get("GM_BENCH_NO_CFG5") != "1":      # every rank takes part (strong scaling at N > 1)
        try:
            c5 = cfg5_leg(torch, stream, T, world, rank, dist, dev, debug_gloo)
        except Exception as e:
            c5 = {"error": repr(e)}
        if rank == 0:
            out["cfg5_geometry"] = c5

    # ------------------------------------------------------------------ digital front-end, informative
    if args.full and rank == 0 and world == 1:
        try:
            out["frontend"] = frontend_leg(torch, dev, not args.no_cpu_baseline)
        except Exception as e:
            out["frontend"] = {"error": repr(e)}

    # ------------------------------------------------------------------ the whole receiver chain, informative
    if receiver_first is not None:
        out["receiver"] = receiver_first          # (measured at the start of this process: see there)

    # ------------------------------------------------------------------ CPU baseline (rank 0, N = 1 only)
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(sc, args.cpu_seconds)

    eng.close()
    if rank == 0:
        # The other half of BASELINE's metric (tracking ch x Msps) and the informative legs' headline numbers once more as SCALARS
        # inside `config`: a record that keeps only the flat part of the line (the driver's `parsed`) then still carries them
        # (VERDICT round 4, item 3a).  Same values as in the legs' own objects; None where a leg did not run.
        def pick(leg, *path):
            v = out.get(leg)
            for k in path:
                v = v.get(k) if isinstance(v, dict) else None
            return v if isinstance(v, (int, float, bool)) else None
        cfg = out["config"]
        cfg.update({
            "tracking_ch_msps": pick("tracking", "value"), "tracking_ms_per_epoch": pick("tracking", "ms_per_epoch"),
            "tracking_frac": pick("tracking", "roofline", "frac"), "tracking_channels_locked": pick("tracking", "channels_locked"),
            "tracking_cpu_ch_msps": pick("tracking", "cpu_baseline", "value"),
            "tracking_256ch_ch_msps": pick("tracking_256ch", "value"), "tracking_256ch_frac": pick("tracking_256ch", "roofline", "frac"),
            "cfg1_ms_per_dwell": pick("cfg1_geometry", "ms_per_dwell"), "cfg1_corr_kernel_ms": pick("cfg1_geometry", "corr_kernel_ms"),
            "cfg1_stage_f_ahead_ms_per_dwell": pick("cfg1_geometry", "stage_f_ahead", "ms_per_dwell"),
            "cfg1_cells_per_s": pick("cfg1_geometry", "cells_per_s"),
            "cfg2_m1_ms_per_dwell": pick("cfg2_single_integration", "ms_per_dwell"),
            "cfg4_galileo_ms_per_dwell": pick("cfg4_galileo_geometry", "ms_per_dwell"),
            "cfg4_galileo_corr_kernel_ms": pick("cfg4_galileo_geometry", "corr_kernel_ms"),
            "cfg4_grid_ms_per_dwell": pick("cfg4_grid", "ms_per_dwell"), "cfg4_grid_cells_per_s": pick("cfg4_grid", "cells_per_s"),
            "cfg5_ch_msps": pick("cfg5_geometry", "ch_msps"), "cfg5_ms_per_code_period": pick("cfg5_geometry", "ms_per_code_period"),
            "cfg5_channels_locked": pick("cfg5_geometry", "channels_locked"),
            "frontend_msps": pick("frontend", "msps"),
            "receiver_x_real_time": pick("receiver", "x_real_time"), "receiver_tracking_wall_s": pick("receiver", "wall_seconds_per_stage", "tracking"),
            "receiver_channels_frame_synchronised": pick("receiver", "channels_frame_synchronised"),
            "receiver_warmup_async_calls": pick("receiver", "warmup_async_calls"), "receiver_python_gc_disabled": pick("receiver", "python_gc_disabled"),
        })
        # A record that keeps only the head of `config` (the driver's `parsed.config` held the first 24 keys in round 5 and cut the
        # receiver / cfg4 / cfg5 scalars) must still carry BOTH halves of BASELINE's metric and one number per BASELINE config: the
        # keys go out in this order — workload first, then the other half of the metric (tracking), then one headline scalar per
        # leg; what merely repeats a top-level field, and legs that did not run (None), travel behind them.
        head = ["workload", "prns_per_gpu", "doppler_bins", "fft_size", "integrations", "cells_per_step", "parallelism", "detections_ok"]
        if world > 1:
            head += ["exchange", "exchange_us_per_dwell", "exchange_overlapped_with_next_dwell"]
        head += ["tracking_ch_msps", "tracking_ms_per_epoch", "tracking_frac", "tracking_channels_locked",
                 "receiver_x_real_time", "receiver_channels_frame_synchronised",
                 "cfg4_grid_ms_per_dwell", "cfg4_galileo_corr_kernel_ms", "cfg5_ch_msps", "cfg5_ms_per_code_period", "frontend_msps",
                 "cfg1_ms_per_dwell", "cfg1_corr_kernel_ms", "cfg1_cells_per_s", "cfg4_galileo_ms_per_dwell", "host_buffer_api_ms_per_dwell"]
        first = [k for k in head if cfg.get(k) is not None]
        out["config"] = {**{k: cfg[k] for k in first}, **{k: v for k, v in cfg.items() if k not in first}}
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


RESULT_FIELDS = ("code_phase_samples", "code_phase_chips", "carrier_freq", "mag_relative", "sample_global_index", "doppler_bin")


def dump_outputs(path, d_grid, results, n_prn, D):
    """--dump-outputs: the metrics block a dwell's decision reads ([3][n_prn][D] words: max f32, argmax u32, sum f32,
    include/gnss_mi355x.h) and the decision per PRN (found, and each AcquisitionResult field; 0 where nothing was found)."""
    os.makedirs(path, exist_ok=True)
    words = d_grid.detach().cpu().numpy().astype(np.int32).reshape(3, n_prn, D)
    np.save(os.path.join(path, "metrics_max.npy"), words[0].view(np.float32))
    np.save(os.path.join(path, "metrics_argmax.npy"), words[1].view(np.uint32).astype(np.float64))
    np.save(os.path.join(path, "metrics_sum.npy"), words[2].view(np.float32))
    np.save(os.path.join(path, "found.npy"), np.array([r is not None for r in results], np.float64))
    np.save(os.path.join(path, "prn.npy"), np.array([r["prn"] if r else 0 for r in results], np.float64))
    for k in RESULT_FIELDS:
        np.save(os.path.join(path, k + ".npy"), np.array([r[k] if r else 0 for r in results], np.float64))


def m1_leg(torch, dev, stream, sc, A, synth, xi8):
    """BASELINE configs[1] with M = 1: the same 32 PRN x 41 bins x 8000 phases on the FIRST millisecond of the bench scene, one
    coherent integration and no non-coherent sum (SURVEY §8's "also report M = 1"; the reference's LONG_SAMPLES_LENGTH is 10).
    1312 single-transform workgroups: the launch is 2.56 rounds of ONE transform each, so it is bound by launch + one transform's
    latency per round, not by issue.  Informative, never `value`."""
    P, D, N = 32, int(sc["doppler_hz"].size), sc["N"]
    eng = A.AcquisitionEngine(sc["fs"], sc["f_if"], N, doppler_hz=sc["doppler_hz"], n_integrations=1)
    eng.set_stream(stream)
    d_x = torch.from_numpy(np.ascontiguousarray(xi8[:N])).to(dev)
    d_met = torch.zeros(3 * P * D, dtype=torch.int32, device=dev)
    for _ in range(5):
        eng.search_dev(d_x.data_ptr(), A.FMT_I8_IQ, d_met.data_ptr()); eng.decide_dev(d_met.data_ptr())
    torch.cuda.synchronize()
    eng.enable_timing(5)
    K = 40      # (fewer launches than the timed region's: the per-shape counter summaries key the headline on the busiest shape)
    t0 = time.perf_counter()
    for _ in range(K):
        eng.search_dev(d_x.data_ptr(), A.FMT_I8_IQ, d_met.data_ptr()); eng.decide_dev(d_met.data_ptr())
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / K
    ts = eng.timing_summary()
    res = eng.fetch_results(P)
    mx, am, _ = eng.metrics()
    # one integration of 8000 cells: max / mean of a noise-only plane is ~ln(8000) = 9 > 7, so the reference's detector declares EVERY
    # PRN at its first Doppler bin (the oracle does the same) — M = 1 is a throughput figure, not a usable detector.  The check is on
    # the planes: the strongest bin of each strong satellite peaks at its true code phase.
    strong = {s_["prn"]: s_["code_start"] for s_ in sc["sats"] if s_["cn0_dbhz"] >= 47.0}
    ok = all(int(am[p_ - 1][int(np.argmax(mx[p_ - 1]))]) == c_ for p_, c_ in strong.items())
    eng.close()
    return {"workload": "32 PRN x 41 bins x 8000 phases, ONE 1 ms integration (M = 1), 8 Msps complex int8", "integrations": 1,
            "ms_per_dwell": dt * 1e3, "cells_per_s": P * D * N / dt, "cell_integrations_per_s": P * D * N / dt,
            "corr_kernel_ms": ts["avg_corr_ms"], "mix_fft_kernel_ms": ts["avg_mix_fft_ms"],
            "strong_satellites_peak_at_true_phase": bool(ok), "prns_declared_by_the_reference_detector": sum(1 for r in res if r),
            "note": "max/mean > 7 passes on noise with one integration of 8000 cells (ln 8000 = 9): every PRN is declared, as by the reference"}


def cfg4_leg(torch, dev, A, synth):
    """The Galileo E1 share of BASELINE configs[3] on one GPU: 36 codes of 4092 chips (4 ms) x 41 bins x 32 000 phases at
    8 Msps, two code periods.  N = 32000 exceeds one LDS buffer: the composite path (2 x the 16000-point in-LDS plan,
    intermediates through HBM / L2).  Stand-in random codes; no reference code exists for this constellation."""
    fs, L, rate, N, M, P = 8.0e6, 4092, 1.023e6, 32000, 2, 36
    rng = np.random.default_rng(4)
    codes = np.where(rng.integers(0, 2, (P, L)) > 0, 1, -1).astype(np.int8)
    dop = np.arange(-5000.0, 5000.1, 250.0, dtype=np.float32)
    sats = [dict(prn_row=r, cn0_dbhz=48.0, doppler_hz=float(rng.uniform(-4500, 4500)), code_start=int(rng.integers(0, N)))
            for r in (1, 7, 19, 30)]
    x = synth.to_i8_iq(synth.make_scene(codes, fs, 0.0, M * N, sats, config_id=44, code_rate=rate))
    eng = A.AcquisitionEngine(fs, 0.0, N, doppler_hz=dop, prn_ids=np.arange(1, P + 1), n_integrations=M, codes=codes,
                              code_rate=rate, decision_mode=A.DECIDE_BEST_BIN)
    d_x = torch.from_numpy(x).to(dev)
    d_met = torch.zeros(3 * P * dop.size, dtype=torch.int32, device=dev)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        eng.search_dev(d_x.data_ptr(), A.FMT_I8_IQ, d_met.data_ptr())
        eng.decide_dev(d_met.data_ptr())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    K = 20
    for _ in range(K):
        eng.search_dev(d_x.data_ptr(), A.FMT_I8_IQ, d_met.data_ptr())
        eng.decide_dev(d_met.data_ptr())
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / K
    res = eng.fetch_results(P)
    ok = all(res[s["prn_row"]] and res[s["prn_row"]]["code_phase_samples"] == s["code_start"] for s in sats)
    # the two stages by the library's HIP events (a few more dwells, outside the clocked ones: an event record costs stream time)
    eng.enable_timing(True)
    for _ in range(10):
        eng.search_dev(d_x.data_ptr(), A.FMT_I8_IQ, d_met.data_ptr())
        eng.decide_dev(d_met.data_ptr())
    torch.cuda.synchronize()
    tm = eng.timing_summary()
    eng.close()
    return {"workload": "36 codes x 41 bins x 32000 phases (4092-chip code, 4 ms), 2 periods, 8 Msps int8; N = 2 x 16000 composite (decimated in time, inverse fused with the power reduction; base 16000 on the wave-specialised kernel)",
            "cells_per_s": P * dop.size * N / dt, "ms_per_dwell": dt * 1e3, "corr_kernel_ms": tm.get("avg_corr_ms"), "forward_ms": tm.get("avg_mix_fft_ms"),
            "simulated_found_at_true_phase": bool(ok)}


def pipelined_leg(torch, dev, sc, A, d_samples, P, D, N, M):
    """Three independent dwells kept in flight on three engines / streams: what the chip does when the grid tail of one
    dwell (1312 workgroups on 512 slots = 2.56 rounds) and the short stage-F / decision kernels are filled by the next
    dwell's work.  Per-kernel durations double under co-execution, so this is reported beside `value`, not as it."""
    engs, mets, streams = [], [], []
    for _ in range(3):
        e = A.AcquisitionEngine(sc["fs"], sc["f_if"], N, doppler_hz=sc["doppler_hz"], n_integrations=M)
        streams.append(torch.cuda.Stream(device=dev))      # kept alive until the engines are closed
        e.set_stream(streams[-1].cuda_stream)
        engs.append(e)
        mets.append(torch.zeros(3 * P * D, dtype=torch.int32, device=dev))

    def step(i):
        engs[i % 3].search_dev(d_samples.data_ptr(), A.FMT_I8_IQ, mets[i % 3].data_ptr())
        engs[i % 3].decide_dev(mets[i % 3].data_ptr())
    for i in range(6):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    K = 60
    for i in range(K):
        step(i)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ok = sorted(r["prn"] for r in engs[0].fetch_results(P) if r) == sorted(s["prn"] for s in sc["sats"])
    for e in engs:
        e.close()
    return {"cells_per_s": P * D * N * K / dt, "ms_per_dwell": dt / K * 1e3, "detections_ok": bool(ok)}


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return "unknown"


def cfg1_cpu_single_prn(sc, prn, reps=3):
    """BASELINE configs[0] as the reference runs it (test_acquisition_with_real_data, do_acquisition.rs:399-466): ONE
    AcquisitionWorker, one thread, 29 Doppler tables, 10 x 16368 samples, early exit — the oracle on this host."""
    from oracle import oracle as O
    from gnss_sdr_rs_amd import synth
    O.build(native=True)
    x = synth.to_c32(sc["x"])
    tables = [O.DopplerShiftTable(sc["f_if"], float(d), sc["fs"], sc["N"]) for d in sc["doppler_hz"]]
    w = O.AcquisitionWorker(prn, sc["N"], sc["fs"], native=True)
    if reps > 1:
        O.search_all([w], 1, x, tables, 0, sc["M"], n_threads=1, native=True)
    ts, cells = [], 0
    for _ in range(reps):
        t0 = time.perf_counter()
        res, cells = O.search_all([w], 1, x, tables, 0, sc["M"], n_threads=1, native=True)
        ts.append(time.perf_counter() - t0)
    dt = float(np.median(ts))
    return {"ms_per_search": dt * 1e3, "cells_per_s": cells / dt, "bins_visited": cells // sc["N"], "cores": 1, "kind": "port",
            "cpu": cpu_model(), "found": bool(res[0])}


def cfg4_grid_leg(torch, dev, stream, ca, A, synth, world, rank, dist, debug_gloo, native_comm=None):
    """BASELINE configs[3] as written: ONE 90-code grid — 32 GPS L1 C/A + 36 Galileo-E1-geometry codes (4092 chips, 4 ms:
    stand-in memory codes, the ICD's hex tables are not available offline) + 22 BeiDou B1I codes (real: gm_b1i_code) — on one
    10 ms IF snapshot at 8 Msps int8, sharded over the ranks in contiguous blocks (12, 12, 11, ... codes at 8 ranks; a rank may
    hold two families with different transform sizes), ONE all-gather of the padded {max, argmax, sum}[P_max][41] blocks, then
    assemble + the reference's decision per family on the gathered grid ON THE DEVICE on every rank (gm_grid_assemble_dev +
    gm_acq_decide_planes_dev): no device-to-host copy inside a dwell.  STRONG scaling (the grid is fixed); informative,
    never `value`.  The same path is parity-tested at these sizes in tests/test_gpu_mixed_grid.py."""
    from gnss_sdr_rs_amd import distributed as Dm
    b1i = A.b1i_codes(range(1, 23))
    sc = synth.cfg4_grid_scene(ca, b1i)          # same seed on every rank: identical bytes
    fams = Dm.baseline_grid_families(sc, b1i)
    D, truth = sc["D"], sc["truth"]
    d_x = torch.from_numpy(synth.to_i8_iq(sc["x"])).to(dev)
    grid, err = None, None
    try:
        grid = Dm.MixedGrid(fams, world, rank, stream=stream)
    except Exception as e:      # a rank that cannot build its engines must not leave the others waiting in the all-gather
        err = repr(e)
    if world > 1:
        flag = torch.tensor([0 if err else 1], dtype=torch.int32, device=dev if not debug_gloo else "cpu")
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if int(flag.item()) == 0:
            if grid:
                grid.close()
            return {"error": err or "another rank failed to build its part of the grid"}
    elif err:
        return {"error": err}
    ptrs = {0: d_x.data_ptr(), 1: d_x.data_ptr(), 2: d_x.data_ptr()}
    gathered = torch.zeros(world * grid.block.numel(), dtype=torch.int32, device=dev)

    def dwell():
        blk = grid.search_dev(ptrs, A.FMT_I8_IQ)
        if world > 1:
            if debug_gloo:
                h = [torch.empty(blk.numel(), dtype=torch.int32) for _ in range(world)]
                dist.all_gather(h, blk.cpu())
                gathered.copy_(torch.cat(h))
            elif native_comm:
                native_comm.allgather_words(blk.data_ptr(), gathered.data_ptr(), blk.numel(), stream)   # the path's one exchange step
            else:
                dist.all_gather_into_tensor(gathered, blk)
            grid.decide_dev(gathered)
        else:
            grid.decide_dev(blk)
    for _ in range(3):
        dwell()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    reps = 20
    t0 = time.perf_counter()
    for _ in range(reps):
        dwell()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = (time.perf_counter() - t0) / reps
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64, device=dev if not debug_gloo else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    res, asm = grid.fetch()
    if os.environ.get("GM_GRID_DEBUG"):
        for fam, sats in truth.items():
            print(fam, [(r["prn"], r["code_phase_samples"], r["doppler_bin"]) for r in res[fam] if r], "truth", sats, file=sys.stderr)
    # truth check on the strongest bin of each simulated satellite's plane (with two integrations of 32000 cells the
    # reference's max/mean > 7 test passes on noise at an early bin — the oracle agrees, tests/test_gpu_generalised.py — so
    # the early-exit result of an E1-geometry code is not where its satellite is)
    ok = True
    for fi, f in enumerate(fams):
        for prn, cp in truth[f.name].items():
            mxp, amp = asm[fi][0][prn - 1].view(np.float32), asm[fi][1][prn - 1].view(np.uint32)
            ok = ok and int(amp[int(np.argmax(mxp))]) == cp
    ok = ok and all(res[fam][prn - 1] is not None and res[fam][prn - 1]["code_phase_samples"] == truth[fam][prn]
                    for fam in ("gps", "b1i") for prn in truth[fam])
    shards = [sum(c for _, _, c in Dm.shard_grid(fams, world, r)) for r in range(world)]
    out = {"workload": "90-code grid: 32 GPS (N=8000, 10 ms) + 36 E1-geometry stand-in codes (N=32000, 2 x 4 ms) + 22 BeiDou B1I (N=8000, "
                       "10 ms), 41 bins, one 10 ms snapshot at 8 Msps int8; contiguous code blocks per rank + one all-gather + decision",
           "scaling": "strong", "n_gpus": world, "codes_per_rank": shards, "cells_per_dwell": grid.cells(),
           "ms_per_dwell": dt * 1e3, "cells_per_s": grid.cells() / dt, "simulated_satellites_found_at_true_phase": bool(ok),
           "exchange": ("gm_comm_allgather_words (RCCL through the C ABI)" if (native_comm and world > 1 and not debug_gloo)
                        else "gloo through host memory (rehearsal)" if (world > 1 and debug_gloo) else "torch.distributed nccl" if world > 1 else None),
           "decision": "on the device (gm_grid_assemble_dev + gm_acq_decide_planes_dev per family); results fetched once after the timed dwells"}
    grid.close()
    return out


def cfg1_leg(torch, dev, stream, ca, A, synth, with_cpu=False):
    """The reference's own test geometry (do_acquisition.rs:399-466: fs 16.3676 MHz, IF 4.1304 MHz, N = 16368, 29 bins,
    10 ms, real int8, 32 PRNs) on the synthetic stand-in for the missing capture; not part of `value`."""
    cap = json.load(open(os.path.join(ROOT, "tests", "golden", "capture_config.json")))
    sc = synth.cfg1_scene(ca, cap)
    x = torch.from_numpy(synth.to_i8_real(sc["x"])).to(dev)
    eng = A.AcquisitionEngine(sc["fs"], sc["f_if"], sc["N"], doppler_hz=sc["doppler_hz"], n_integrations=sc["M"])
    eng.set_stream(stream)
    P, D, N, M = 32, int(sc["doppler_hz"].size), sc["N"], sc["M"]
    for _ in range(2):
        eng.search_dev(x.data_ptr(), A.FMT_I8_REAL)
        eng.decide_dev()
    torch.cuda.synchronize()
    reps = 20
    t0 = time.perf_counter()
    for _ in range(reps):
        eng.search_dev(x.data_ptr(), A.FMT_I8_REAL)
        eng.decide_dev()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    res = eng.fetch_results()
    found = sorted(r["prn"] for r in res if r)
    # the stages by the library's HIP events, outside the clocked dwells (four event records cost ~8 us of stream time per dwell)
    eng.enable_timing(True)
    for _ in range(10):
        eng.search_dev(x.data_ptr(), A.FMT_I8_REAL)
        eng.decide_dev()
    torch.cuda.synchronize()
    ts = eng.timing_summary()
    eng.enable_timing(False)
    # dwell after dwell with stage F of dwell k + 1 beside stage C of dwell k (gm_acq_prepare_dev: second stream, second spectrum
    # buffer): 928 one-per-CU workgroups are 3.6 rounds, stage F fits into the rest
    tok = eng.prepare_dev(x.data_ptr(), A.FMT_I8_REAL)
    for i in range(3):
        eng.search_prepared_dev(tok); tok = eng.prepare_dev(x.data_ptr(), A.FMT_I8_REAL); eng.decide_dev()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(reps):
        eng.search_prepared_dev(tok)
        if i + 1 < reps:
            tok = eng.prepare_dev(x.data_ptr(), A.FMT_I8_REAL)
        eng.decide_dev()
    torch.cuda.synchronize()
    dt_ahead = (time.perf_counter() - t0) / reps
    res_ahead = eng.fetch_results()
    same = sorted(r["prn"] for r in res_ahead if r) == found and \
        all((a is None) == (b is None) and (a is None or (a["code_phase_samples"], a["doppler_bin"], a["mag_relative"]) ==
                                            (b["code_phase_samples"], b["doppler_bin"], b["mag_relative"])) for a, b in zip(res, res_ahead))
    eng.close()
    # BASELINE configs[0] proper: ONE PRN (the reference's test_acquisition_with_real_data searches a single worker at a
    # time): 29 items would leave the chip idle, so every item is cut into five parts (grid split of acq_corr_kernel)
    one = A.AcquisitionEngine(sc["fs"], sc["f_if"], sc["N"], doppler_hz=sc["doppler_hz"], n_integrations=sc["M"],
                              prn_ids=[sc["sats"][0]["prn"]])
    one.set_stream(stream)
    for _ in range(2):
        one.search_dev(x.data_ptr(), A.FMT_I8_REAL)
        one.decide_dev()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        one.search_dev(x.data_ptr(), A.FMT_I8_REAL)
        one.decide_dev()
    torch.cuda.synchronize()
    dt1 = (time.perf_counter() - t0) / reps
    r1 = one.fetch_results(1)[0]
    one.close()
    corr_bytes = P * D * M * N * 16
    cpu1 = None
    if with_cpu:
        try:
            cpu1 = cfg1_cpu_single_prn(sc, sc["sats"][0]["prn"])
        except Exception as e:
            cpu1 = {"error": repr(e)}
    # a satellite of the scene the GPU did not declare (the weakest ones sit at the reference's threshold of 7): what does the CPU
    # restatement of the reference decide for it on the same samples?  (The decision is the reference's, not the kernel's.)
    missed = sorted(set(s["prn"] for s in sc["sats"]) - set(found))
    missed_cpu = None
    if with_cpu and missed:
        try:
            missed_cpu = {str(p): cfg1_cpu_single_prn(sc, p, reps=1)["found"] for p in missed[:3]}
        except Exception as e:
            missed_cpu = {"error": repr(e)}
    return {"prns_not_declared": missed, "cpu_port_declares_them": missed_cpu, "single_prn": {"ms_per_dwell": dt1 * 1e3, "cells_per_s": D * N / dt1, "cpu_baseline": cpu1,
                           "found_within_3_samples_of_truth": bool(r1 and min((r1["code_phase_samples"] - sc["sats"][0]["code_start"]) % N,
                                                                                (sc["sats"][0]["code_start"] - r1["code_phase_samples"]) % N) <= 3)},
            "workload": "32 PRN x 29 bins (+-7 kHz / 500 Hz) x 16368 phases, 10 x 1 ms, real int8 (reference test geometry)",
            "cells_per_s": P * D * N / dt, "ms_per_dwell": dt * 1e3, "corr_kernel_ms": ts["avg_corr_ms"],
            "stage_f_ahead": {"ms_per_dwell": dt_ahead * 1e3, "cells_per_s": P * D * N / dt_ahead, "same_results": bool(same),
                              "api": "search_prepared_dev(token k), prepare_dev(k + 1) -> token, decide_dev(k): stage F of the next dwell on the handle's second stream"},
            "corr_algorithmic_GBs": corr_bytes / (ts["avg_corr_ms"] * 1e-3) / 1e9 if ts["avg_corr_ms"] > 0 else None,
            "prns_found": found, "prns_in_scene": sorted(s["prn"] for s in sc["sats"])}


def cfg5_leg(torch, stream, T, world=1, rank=0, dist=None, dev=None, debug_gloo=False):
    """BASELINE configs[4]: 36 channels, 50 Msps, 4092-chip codes at 1.023 Mcps (4 ms period, 200 000 samples), BOC(1,1), five
    arms (VE/E/P/L/VL), "1 -> 8 GPU scaling": STRONG scaling — the 36 channels are sharded over the ranks in contiguous blocks
    (5/5/5/5/4/4/4/4 at 8 ranks), every rank holds the same IF stream in its own ring mirror, no collective on the data path
    (channels are independent, do_tracking.rs:364-371); ch_msps = 36 x 50 x signal time / the slowest rank's wall time.
    The reference has no Galileo/BOC code: stand-in random codes, GPU-only number."""
    from gnss_sdr_rs_amd import distributed as Dm
    # 24 code periods (96 ms of signal) per launch since round 6 (6 before): the launch's fixed costs — the dispatcher reaches one XCD
    # 8 us after the others, the host's launch + synchronise — weighed 2-3 us per period on six periods; a receiver's launches are
    # long (one per block of samples).  The scene is built period by period from one period of (code x sub-carrier x carrier) per
    # satellite and a phasor per period: every satellite is code-aligned at sample 0 and a code period is exactly n samples.
    fs, L, rate, C, periods = 50.0e6, 4092, 1.023e6, 36, 24
    n = int(round(fs / (rate / L)))
    mine = Dm.shard_prns(list(range(C)), world, rank)
    rng = np.random.default_rng(5)
    codes = np.where(rng.integers(0, 2, (C, L)) > 0, 1, -1).astype(np.int8)
    t1p = np.arange(n, dtype=np.float64)
    cp = (t1p * rate / fs) % L
    sub = np.where((cp - np.floor(cp)) < 0.5, 1.0, -1.0).astype(np.float32)
    ci = np.floor(cp).astype(np.int64)
    x = (rng.standard_normal((periods + 1) * n) + 1j * rng.standard_normal((periods + 1) * n)).astype(np.complex64) * np.float32(8.0)
    dopp = rng.uniform(-2000, 2000, C)
    xv = x.reshape(periods + 1, n)
    for c in range(C):   # all satellites code-aligned at sample 0 (keeps the generator cheap); the whole sky on every rank
        one = (np.float32(0.6) * codes[c][ci] * sub * np.exp(2j * np.pi * dopp[c] * t1p / fs)).astype(np.complex64)
        step = np.exp(2j * np.pi * dopp[c] * n / fs)
        xv += one[None, :] * (step ** np.arange(periods + 1))[:, None].astype(np.complex64)
    ring = T.MulticastRingBuffer(1 << 23)
    ring.write_samples(x)
    Cl = len(mine)
    mgr = T.TrackingManager(fs, n_channels=Cl, n_arms=5, code_index_mode=T.CODE_INDEX_FIXED, early_late_space=0.25,
                            very_early_late_space=0.6, boc11=True, codes=codes[mine], nominal_code_rate=rate)
    mgr.set_stream(stream)

    def restart():
        for j, c in enumerate(mine):
            mgr.channels[j].start(dict(prn=j + 1, code_phase_samples=0, code_phase_chips=0.0, carrier_freq=float(dopp[c]) + 10.0,
                                       fs=fs, mag_relative=1.0, sample_global_index=0, doppler_bin=0))
            mgr.channels[j].set_state(code_rate=rate, num_samples_per_code=n, carrier_phase=0.0, code_error=0.0,
                                      carrier_error=0.0, lost_counter=0)
    err, locked = None, 0
    try:
        restart()
        mgr.update_all_dev(ring, periods)
        mgr.synchronize()
        locked = sum(1 for c in mgr.channels if c.is_active() and c.lost_counter == 0)
    except Exception as e:      # a rank that fails must not leave the others waiting at the barrier below
        err = repr(e)
    if world > 1:
        flag = torch.tensor([0 if err else 1], dtype=torch.int32, device="cpu" if debug_gloo else dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if int(flag.item()) == 0:
            err = err or "another rank failed"
    if err:
        return {"error": err}
    times, ktimes = [], []
    mgr.enable_timing(True)
    for _ in range(3):
        restart()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        mgr.update_all_dev(ring, periods)
        mgr.synchronize()
        t1 = time.perf_counter() - t0
        ktimes.append(mgr.last_timing()[0])
        if world > 1:      # the job is done when the slowest rank is
            tm = torch.tensor([t1], dtype=torch.float64, device="cpu" if debug_gloo else dev)
            dist.all_reduce(tm, op=dist.ReduceOp.MAX)
            t1 = float(tm.item())
        times.append(t1)
    dt = float(np.median(times))
    mgr.close()
    ring.close()
    if world > 1:
        lk = torch.tensor([locked], dtype=torch.int64, device="cpu" if debug_gloo else dev)
        dist.all_reduce(lk, op=dist.ReduceOp.SUM)
        locked = int(lk.item())
    sig_s = periods * n / fs
    return {"workload": "36 ch x 50 Msps, 4092-chip BOC(1,1), 5 arms, 4 ms code periods (no reference code: stand-in codes)",
            "scaling": "strong", "n_gpus": world,
            "channels_per_rank": [len(Dm.shard_prns(list(range(C)), world, r)) for r in range(world)],
            "ch_msps": C * fs / 1e6 * (sig_s / dt), "ms_per_code_period": dt / periods * 1e3, "channels_locked": locked,
            "code_periods_per_launch": periods, "kernel_ms_per_code_period": float(np.median(ktimes)) / periods,
            "algorithmic_GBs": C * n * 8 * periods / dt / 1e9}


def receiver_leg(ca, A, T, synth, with_cpu, n_ms=3200):
    """SURVEY §8 f1 as ONE chain, the receiver main.rs:182-227 wires — run by the DELIVERABLE C++ stage drivers (round 6: VERDICT
    round 5 item 2), not by a Python re-statement of their loops: host/receiver_harness.cpp puts a feeder (the SDR's sample blocks
    -> DigitalFrontend::write_ring, rf_thread's block step, rf/rf_thread.rs:43-48) on the calling thread, gnss::run_acquisition
    (do_acquisition.rs:241-327: snapshot + search on the ring, the AcquisitionManager's pacing counted in SIGNAL time, + fine Doppler)
    and gnss::run_tracking (do_tracking.rs:384-415: 15 channels, the reference's constants, FIXED code index, the ticket loop — no
    host wait per block) on threads of their own, talking through the two channels of main.rs:183-184, and nav-bit accumulation
    (bit sync / preamble) behind every collected tracking call.  3.2 s of int8 IQ at the reference capture's 16.3676 Msps /
    4.1304 MHz IF (N = 16368), eight satellites with 50 bit/s data (frame sync needs ~3 s).  Reported: sustained Msps and x real
    time over the whole chain, when the first satellite was handed to tracking / bit-synchronised / frame-synchronised (signal time
    and wall clock), and the wall clock each stage's thread spent inside its calls.  Informative, never `value`.  The same drivers are
    parity-tested in tests/test_gpu_stage_drivers.py (ticket loop == synchronous loop, bit for bit)."""
    from gnss_sdr_rs_amd import decoding as Dm, receiver as R
    fs, f_if, N, M = 16_367_600.0, 4_130_400.0, 16368, 10
    rng = np.random.default_rng(11)
    sats = []
    for i, (prn, cn0) in enumerate([(2, 50.0), (5, 48.0), (9, 47.0), (13, 46.0), (17, 46.0), (22, 45.0), (26, 44.0), (30, 44.0)]):
        data = rng.integers(0, 2, 200) * 2 - 1
        for at in range(10 + i, 190, 30):
            data[at:at + 8] = Dm.GPS_CA_PREAMBLE
        sats.append(dict(prn=prn, prn_row=prn - 1, cn0_dbhz=cn0, doppler_hz=float(rng.uniform(-5500, 5500)), code_start=int(rng.integers(0, N)),
                         phase=0.3 * i, data_bits=data, bit_edge_ms=int(rng.integers(0, 20))))
    t_gen = time.perf_counter()
    # the front-end's mix (nco_lut.rs:8-15) brings a spectrally INVERTED IF stream to baseband at +Doppler: that is what is fed
    x = np.conj(synth.make_scene(ca, fs, f_if, n_ms * N, sats, config_id=12))
    x += (5.0 - 3.0j)                                               # a DC offset for the front-end to remove
    xi8 = synth.to_i8_iq(np.clip(x.real, -127, 127) + 1j * np.clip(x.imag, -127, 127))
    del x
    t_gen = time.perf_counter() - t_gen
    BLK, WARM = 1 << 19, 48                                         # 32 ms per block (one staging slot of the ring's asynchronous writer)
    dop = np.arange(-7000.0, 7000.1, 500.0, dtype=np.float32)       # do_acquisition.rs:248-255
    # before the clock starts (inside the harness): one scratch dwell + fine Doppler and WARM asynchronous tracking calls on scratch
    # handles (code objects; the HIP runtime grows its signal / command pools in steps on the first few dozen asynchronous calls of a
    # stream), the first 64 samples through the ring (pinned staging, streams), both stage threads constructed and listening
    rep = R.receiver_run(xi8, fs, f_if, freq_search_hz=14e3, freq_step_hz=500.0, n_integrations=M, n_channels=15, block_samples=BLK,
                         ring_log2=23, decision_mode=A.DECIDE_BEST_BIN, code_index_mode=T.CODE_INDEX_FIXED, nav_mode=Dm.NAV_FIXED,
                         fine_doppler=True, async_tickets=True, first_round_signal_ms=10.0, pre_samples=64, warmup_calls=WARM)
    wall, sig_s = rep["wall_seconds"], n_ms * 1e-3
    truth = {s_["prn"]: s_ for s_ in sats}
    chans = [c for c in rep["channels"] if c["prn"]]
    locked = sum(1 for c in chans if c["active"] and c["prn"] in truth and abs(c["carrier_freq"] - truth[c["prn"]]["doppler_hz"]) < 25.0)
    ev = {k: {"signal_ms": rep["first_%s_signal_ms" % k], "wall_s": rep["first_%s_wall_s" % k]}
          for k in ("handover", "bit_sync", "frame_sync") if rep["first_%s_signal_ms" % k] >= 0}
    out = {"workload": "feeder -> digital front-end -> device ring -> acquisition (32 PRN x 29 bins x 16368, 10 ms) + fine Doppler -> 15-channel "
                       "tracking -> bit sync / nav bits; %.1f s of int8 IQ at 16.3676 Msps, IF 4.1304 MHz, 8 satellites, 32 ms blocks" % sig_s,
           "driver": "C++ stage drivers of host/gnss_sdr.hpp through host/receiver_harness.cpp: feeder on the calling thread, gnss::run_acquisition "
                     "and gnss::run_tracking (ticket loop) on threads of their own — the deliverable's loops, no Python in the timed region",
           "warmup_async_calls": WARM, "python_gc_disabled": False,
           "measured_before_other_streams_exist": "bench.py runs this leg first: HIP deals streams to hardware queues per priority in creation order; behind torch\'s 32-stream pool the chain ran at 118-190 x until its copy / front-end streams got priorities of their own (now 206-216 x there, 220 x here; tools/rx_order_probe.py)",
           "signal_seconds": sig_s, "wall_seconds": wall, "x_real_time": sig_s / wall, "sustained_msps": n_ms * N / wall / 1e6,
           "dwells": rep["dwells"], "channel_epochs": rep["channel_epochs"], "tracking_passes": rep["tracking_passes"],
           "frontend_blocks": rep["blocks"], "frontend_speculated_runs_done_again": rep["fe_runs_repaired"],
           "satellites_in_scene": len(sats), "channels_started": rep["channels_started"],
           "channels_on_true_doppler": locked,
           "channels_bit_synchronised": sum(1 for c in chans if c["bit_sync"]),
           "channels_frame_synchronised": sum(1 for c in chans if c["frame_sync"]),
           "events_signal_ms_and_wall_s": {"first_" + k: v for k, v in ev.items()},
           "wall_seconds_per_stage": {"frontend": rep["seconds_frontend"], "acquisition": rep["seconds_acquisition"],
                                      "fine_doppler": rep["seconds_fine_doppler"], "tracking": rep["seconds_tracking"],
                                      "nav_bits": rep["seconds_nav_bits"], "feeder_held_back": rep["feeder_held_back_s"]},
           "frontend_block_seconds": {"first": rep["fe_block_first_s"], "median": rep["fe_block_median_s"], "max_after_first": rep["fe_block_max_after_first_s"]},
           "scene_generation_seconds": t_gen,
           "bound": "the front-end per block of 2^19 samples: 1 MB host-to-device + the speculative front-end kernels (32 workgroups from guessed "
                    "DC-remover states, verified and repaired: ~0.11 ms against 0.52 ms for the sequential form, DESIGN 4.4) ~ 0.15 ms per 32 ms of "
                    "signal; the feeder thread only enqueues (%d blocks; reclaiming a staging slot is its only wait), the tracking thread enqueues "
                    "process_channels behind each block ON THE DEVICE (gm_trk_update_all_async) and collects a block or two later, the acquisition "
                    "thread snapshots the published head when a round is due in signal time" % rep["blocks"]}
    if with_cpu:
        try:
            out["cpu_oracle_chain"] = receiver_cpu_chain(ca, xi8, fs, f_if, N, M, dop, sats)
        except Exception as e:
            out["cpu_oracle_chain"] = {"error": repr(e)}
    return out


def receiver_cpu_chain(ca, xi8, fs, f_if, N, M, dop, sats):
    """The oracle's restatement of the same chain on this host, stage by stage on bounded samples of the same stream: the
    front-end (one thread: its recurrences are sequential), one 32-PRN acquisition dwell (min(32, nproc) threads, early exit as
    in the reference), eight tracking channels (one thread each), nav-bit steps.  seconds of CPU wall clock per second of signal
    = front-end + dwells per second x dwell + tracking + nav; x real time = its inverse (stages run one after the other here; the
    reference runs them as threads, so max(...) is its optimistic bound and is reported too)."""
    from oracle import oracle as O
    O.build(native=True)
    nthreads = min(32, os.cpu_count() or 1)
    n_fe = min(xi8.shape[0], 1 << 22)
    ofe = O.DigitalFrontend(f_if, fs, fs, native=True)
    xf = xi8[:n_fe].astype(np.float32).reshape(-1)
    t0 = time.perf_counter()
    ofe.process_block(xf)
    fe_s = (time.perf_counter() - t0) / (n_fe / fs)
    base = xf.view(np.complex64)[:60 * N].copy()                      # 60 ms of front-end output for the other stages
    tables = [O.DopplerShiftTable(0.0, float(d), fs, N) for d in dop]
    workers = [O.AcquisitionWorker(p, N, fs, native=True) for p in range(1, 33)]
    t0 = time.perf_counter()
    res, cells = O.search_all(workers, 0xFFFFFFFF, base[:M * N], tables, 0, M, n_threads=nthreads, native=True)
    acq_s = time.perf_counter() - t0
    ring = O.MulticastRingBuffer(1 << 20)
    ring.write_samples(base)
    chans = []
    for i, s_ in enumerate(sats):
        ch = O.TrackingChannel(i, fs, code_index_mode=O.CODE_INDEX_FIXED)
        ch.start(dict(prn=s_["prn"], code_phase_samples=0, code_phase_chips=0.0, carrier_freq=s_["doppler_hz"], fs=fs, mag_relative=1.0,
                      sample_global_index=s_["code_start"]))
        chans.append(ch)
    O.process_channels(chans, ring, 2, n_threads=min(nthreads, len(chans)), native=True)
    t0 = time.perf_counter()
    got = O.process_channels(chans, ring, 50, n_threads=min(nthreads, len(chans)), native=True)
    trk_s = (time.perf_counter() - t0) / max(got, 1) * len(chans) * 1000.0 / 1.0       # per channel-epoch x 8 channels x 1000 epochs per second
    nav = O.NavSyncStatus(fixed=True)
    t0 = time.perf_counter()
    for e in range(2000):
        nav.update(1.0, -1.0 if (e // 20) & 1 else 1.0, e)
    nav_s = (time.perf_counter() - t0) / 2000 * len(sats) * 1000.0
    dwells_per_s = 0.5                                                # steady state: one dwell per 2 s (do_acquisition.rs:57-61)
    total = fe_s + dwells_per_s * acq_s + trk_s + nav_s
    return {"kind": "port", "cores": nthreads, "cpu": cpu_model(),
            "seconds_per_signal_second": {"frontend_1_thread": fe_s, "acquisition_dwell_s": acq_s, "tracking_8_channels": trk_s, "nav_bits": nav_s,
                                          "total_sequential": total},
            "x_real_time_sequential": 1.0 / total, "x_real_time_if_stages_overlap_perfectly": 1.0 / max(fe_s, dwells_per_s * acq_s, trk_s, nav_s),
            "sample": "front-end: %.2f s of the stream; acquisition: one 32-PRN dwell (%d threads); tracking: 50 epochs x 8 channels" % (n_fe / fs, nthreads)}


def frontend_leg(torch, dev, with_cpu):
    """DigitalFrontend::process_block (rf/frontend.rs:33-62) on 4 Mi samples of int8 IQ resident in HBM -> c32.  The
    two f32 recurrences (NCO phase, DC bias) are sequential by construction (bit-exactness): the NCO phase is a tabulated orbit,
    the DC remover's sixteen chains run speculatively on 32 workgroups from guessed states and are verified / repaired (round 6,
    fe_kernels.hip) — exact, and several times the one-workgroup form; the requirement is the live sample rate (8-50 Msps)."""
    from gnss_sdr_rs_amd import frontend as F, _lib
    n = 1 << 22
    rng = np.random.default_rng(2)
    xi = rng.integers(-127, 128, 2 * n).astype(np.int8)
    d_in = torch.from_numpy(xi).to(dev)
    d_out = torch.empty(2 * n, dtype=torch.float32, device=dev)
    fe = F.DigitalFrontend(4.1304e6, 16.3676e6, 16.3676e6)
    st = torch.cuda.current_stream().cuda_stream
    fe.process_dev(d_in.data_ptr(), _lib.FMT_I8_IQ, d_out.data_ptr(), n, st)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        fe.process_dev(d_in.data_ptr(), _lib.FMT_I8_IQ, d_out.data_ptr(), n, st)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 3
    fe.close()
    res = {"workload": "DC removal + LUT NCO down-mix, 4 Mi int8 IQ samples -> c32, one stream, bit-exact",
           "msps": n / dt / 1e6, "ms": dt * 1e3}
    # 64 independent streams (antennas / bands) in one launch, one workgroup per stream (gm_frontend_process_dev_batch)
    S, nb = 64, 1 << 20
    fes = [F.DigitalFrontend(4.1304e6 + 1000.0 * i, 16.3676e6, 16.3676e6) for i in range(S)]
    outs = torch.empty((S, 2 * nb), dtype=torch.float32, device=dev)
    ins = [d_in.data_ptr()] * S
    ops = [outs[i].data_ptr() for i in range(S)]
    F.process_dev_batch(fes, ins, _lib.FMT_I8_IQ, ops, nb, st)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    F.process_dev_batch(fes, ins, _lib.FMT_I8_IQ, ops, nb, st)
    torch.cuda.synchronize()
    dtb = time.perf_counter() - t0
    for f_ in fes:
        f_.close()
    res["aggregate_msps_64_streams"] = S * nb / dtb / 1e6
    if with_cpu:
        from oracle import oracle as O
        O.build(native=True)
        ofe = O.DigitalFrontend(4.1304e6, 16.3676e6, 16.3676e6, native=True)
        xf = xi.astype(np.float32)
        ofe.process_block(xf[:1 << 16].copy())
        t0 = time.perf_counter()
        ofe.process_block(xf)
        res["cpu_msps_one_thread"] = n / (time.perf_counter() - t0) / 1e6
    return res


def tracking_leg(torch, dev, stream, ca, T, synth, world, dist, cpu_seconds=0.0, C=32):
    """C channels x 25 Msps, 1 ms E/P/L correlators + DLL/PLL on-device, FIXED code indexing
    (FAITHFUL cannot run PRN 32: the reference indexes GPS_CA_CODE_32_PRN[32]).  C = 32 is BASELINE configs[2];
    larger C (channels beyond 32 re-track the same 32 satellites) shows the kernel away from the per-epoch latency floor."""
    fs, reps = 25.0e6, 5
    epochs = 480 if C == 32 else 120     # one persistent launch; its ~10 us of launch + hand-shake amortise over the epochs (120: +0.1 us per epoch)
    n = 25000
    prns = list(range(1, 33))
    sc = synth.tracking_scene(ca, fs, 0.0, prns, epochs + 2, config_id=3, cn0=47.0)
    ring = T.MulticastRingBuffer(1 << 24 if epochs > 320 else 1 << 23 if epochs > 160 else 1 << 22 if epochs > 80 else 1 << 21)
    ring.write_samples(synth.to_c32(sc["x"]))
    mgr = T.TrackingManager(fs, n_channels=C, code_index_mode=T.CODE_INDEX_FIXED)
    mgr.set_stream(stream)

    def restart(m=None):
        m = m or mgr
        for i in range(C):
            s = sc["sats"][i % 32]
            m.channels[i].start(dict(prn=s["prn"], code_phase_samples=0, code_phase_chips=0.0, carrier_freq=s["doppler_hz"] + 20.0,
                                     fs=fs, mag_relative=1.0, sample_global_index=s["code_start"], doppler_bin=0))
            m.channels[i].set_state(code_rate=1.023e6, num_samples_per_code=n, carrier_phase=0.0, code_error=0.0,
                                    carrier_error=0.0, lost_counter=0)
    restart()
    mgr.update_all_dev(ring, epochs)
    mgr.synchronize()
    locked = sum(1 for c in mgr.channels if c.is_active() and abs(c.carrier_freq - sc["sats"][c.id % 32]["doppler_hz"]) < 25.0)
    times = []
    for _ in range(reps):
        restart()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mgr.update_all_dev(ring, epochs)
        mgr.synchronize()
        times.append(time.perf_counter() - t0)
    dt = float(np.median(times))
    ch_msps = C * fs / 1e6 * (epochs * 1e-3 / dt)
    bytes_per_epoch = C * n * 8
    gbs = bytes_per_epoch * epochs / dt / 1e9
    mgr.close()
    strict = None
    if world == 1 and C == 32 and os.environ.get("GM_BENCH_NO_STRICT") != "1":
        # what gm_trk_cfg.strict_libm costs (the carrier's cos / sin as glibc's cosf / sinf, f64, sample by sample): informative,
        # never part of `value`
        try:
            ms = T.TrackingManager(fs, n_channels=C, code_index_mode=T.CODE_INDEX_FIXED, strict_libm=True)
            ms.set_stream(stream)
            se = 120
            st = []
            for _ in range(3):
                restart(ms)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ms.update_all_dev(ring, se)
                ms.synchronize()
                st.append(time.perf_counter() - t0)
            strict = {"us_per_epoch": float(np.median(st[1:])) / se * 1e6, "epochs": se,
                      "note": "strict_libm = 1: per-sample products bit-identical to the reference host's (tests/test_gpu_tracking_shapes.py)"}
            ms.close()
            # ... and with the reference's sequential sums as well: sums and channel state bit-identical, free-running
            ms = T.TrackingManager(fs, n_channels=C, code_index_mode=T.CODE_INDEX_FIXED, strict_libm=True, strict_sum_order=True)
            ms.set_stream(stream)
            se2 = 40
            st = []
            for _ in range(3):
                restart(ms)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ms.update_all_dev(ring, se2)
                ms.synchronize()
                st.append(time.perf_counter() - t0)
            strict["with_strict_sum_order_us_per_epoch"] = float(np.median(st[1:])) / se2 * 1e6
            strict["with_strict_sum_order_x_real_time"] = 1e3 / strict["with_strict_sum_order_us_per_epoch"]
            ms.close()
        except Exception as e:      # informative leg: never fails the bench
            strict = {"error": repr(e)}
    ring.close()
    trk_cpu = None
    if world == 1 and cpu_seconds > 0 and C == 32:
        trk_cpu = tracking_cpu_baseline(sc, fs, n, cpu_seconds)
    return {"metric": "tracking ch×Msps", "cpu_baseline": trk_cpu, "value": ch_msps * world, "unit": "ch*Msps", "channels_per_gpu": C,
            "fs_msps": 25.0, "epochs": epochs, "ms_per_epoch": dt / epochs * 1e3, "channels_locked": locked,
            "strict_libm": strict, "roofline": trk_roofline(gbs, bytes_per_epoch, epochs, C)}


def trk_roofline(gbs, bytes_per_epoch, epochs, C):
    """The tracking kernel's record: its byte model is SURVEY 8d's (every channel streams its own window, C*n*8 bytes per
    epoch), but an epoch of one channel is a dependent chain (correlate -> reduce -> exchange -> loop filters -> next NCO
    values, do_tracking.rs:160-302), so the bound at C = 32 is that chain's latency, not bytes: `frac` is the share of the
    HBM peak the model bytes reach, `traffic` the measured fabric bytes per epoch (channels share the ring window through L2)."""
    r = {"bound": "latency-chain", "kernel": "trk_persistent_kernel", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
         "frac": gbs / HBM_PEAK_GBS, "algorithmic_bytes_per_epoch": bytes_per_epoch, "traffic": None,
         "traffic_over_algorithmic": None,
         "reading": "one epoch per channel is a serial chain of ~3 us (DESIGN 4.3); HBM sees a few % of its peak"}
    try:
        t = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
        per_launch, ep = t.get("trk_persistent_kernel_hbm_bytes_per_launch"), t.get("trk_persistent_kernel_epochs_per_launch", 480)
        if per_launch and C == 32:
            r["traffic"] = per_launch / ep
            r["traffic_over_algorithmic"] = per_launch / ep / bytes_per_epoch
            r["traffic_source"] = "profiles/traffic.json (2 x FETCH_SIZE + WRITE_SIZE per launch / %d epochs per launch)" % ep
    except Exception:
        pass
    return r


def tracking_cpu_baseline(sc, fs, n, budget_s):
    """The oracle's TrackingManager::process_channels (do_tracking.rs:351-371: one rayon task per channel ->
    OpenMP) on this host: the same 32 channels and ring contents as the GPU leg, FIXED code index, whole passes of
    all channels until ~budget_s seconds.  Per-sample libm cosf/sinf + fmodf like the reference (:233-252)."""
    from oracle import oracle as O
    from gnss_sdr_rs_amd import synth
    O.build(native=True)
    nthreads = min(32, os.cpu_count() or 1)
    ring = O.MulticastRingBuffer(1 << 22)
    x_cpu = sc["x"][: min(int(sc["x"].size), 122 * n)]      # the first 122 ms of the GPU leg's scene: a bounded sample for the CPU
    ring.write_samples(synth.to_c32(x_cpu))
    avail = int(x_cpu.size // n) - 2

    def fresh():
        chans = []
        for i, s_ in enumerate(sc["sats"]):
            ch = O.TrackingChannel(i, fs, code_index_mode=O.CODE_INDEX_FIXED)
            ch.start(dict(prn=s_["prn"], code_phase_samples=0, code_phase_chips=0.0, carrier_freq=s_["doppler_hz"] + 20.0,
                          fs=fs, mag_relative=1.0, sample_global_index=s_["code_start"]))
            ch.c.code_rate, ch.c.num_samples_per_code = 1.023e6, n
            chans.append(ch)
        return chans
    O.process_channels(fresh(), ring, 2, n_threads=nthreads, native=True)     # warm-up
    done, secs, t_start = 0, [], time.perf_counter()
    while time.perf_counter() - t_start < budget_s or not secs:
        chans = fresh()
        t0 = time.perf_counter()
        got = O.process_channels(chans, ring, avail, n_threads=nthreads, native=True)
        secs.append((time.perf_counter() - t0) / max(got, 1))
        done += got
    per_ch_epoch = float(np.median(secs))                       # seconds per channel-epoch with all threads busy
    one_ch = fresh()[:1]
    O.process_channels(one_ch, ring, 2, n_threads=1, native=True)        # settle the OpenMP team on one thread
    t0 = time.perf_counter()
    got1 = O.process_channels(one_ch, ring, min(avail - 2, 40), n_threads=1, native=True)
    one = (time.perf_counter() - t0) / max(got1, 1)
    return {"value": n / per_ch_epoch / 1e6, "unit": "ch*Msps", "cores": nthreads, "kind": "port", "cpu": cpu_model(),
            "sample": f"{done} channel-epochs (32 ch x 25 Msps scene of the GPU leg, 1 ms epochs)",
            "single_thread_ch_msps": n / one / 1e6}


def hbm_ceiling(torch, dev):
    """the measured device-to-device copy ceiling next to the 8 TB/s datasheet peak (1 GiB -> 1 GiB,
    read + write counted)."""
    nbytes = 1 << 30
    a = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 10
    del a, b
    return 2 * nbytes / (ms * 1e-3) / 1e9


def cpu_baseline(sc, budget_s):
    """The oracle (CPU restatement of the reference: one worker per PRN redoing mix + FFT + IFFT, early exit,
    do_acquisition.rs:302-313) on this host's cores, threads = min(32, nproc) like rayon.  Bounded sample:
    whole dwells of the same scene until ~budget_s seconds."""
    from oracle import oracle as O
    from gnss_sdr_rs_amd import synth
    O.build(native=True)
    nthreads = min(32, os.cpu_count() or 1)
    x = synth.to_c32(sc["x"])
    tables = [O.DopplerShiftTable(sc["f_if"], float(d), sc["fs"], sc["N"]) for d in sc["doppler_hz"]]
    workers = [O.AcquisitionWorker(p, sc["N"], sc["fs"], native=True) for p in range(1, 33)]
    O.search_all(workers, 0xFFFFFFFF, x, tables, 0, sc["M"], n_threads=nthreads, native=True)     # warm-up dwell
    rates, dwell_s, t_start = [], [], time.perf_counter()
    while len(rates) < 3 or (time.perf_counter() - t_start < budget_s and len(rates) < 25):
        t0 = time.perf_counter()
        _, cells = O.search_all(workers, 0xFFFFFFFF, x, tables, 0, sc["M"], n_threads=nthreads, native=True)
        dt = time.perf_counter() - t0
        rates.append(cells / dt)
        dwell_s.append(dt)
    # single-thread rate on a bounded slice (4 PRNs) for reference
    t0 = time.perf_counter()
    _, cells1 = O.search_all(workers[:4], 0xF, x, tables, 0, sc["M"], n_threads=1, native=True)
    r1 = cells1 / (time.perf_counter() - t0)
    return {"value": float(np.median(rates)), "unit": "cells/s", "cores": nthreads, "kind": "port", "cpu": cpu_model(),
            "sample": f"{len(rates)} dwells of the bench scene (32 PRN x 41 bins x 8000 phases, 10 ms, early exit as in "
                      f"the reference; cells = bins visited x 8000), median dwell {np.median(dwell_s):.3f} s",
            "single_thread_cells_per_s": float(r1),
            "note": "oracle's own f32 mixed-radix FFT, not rustfft 6.1.0 (AVX); reported baseline, not the target"}


if __name__ == "__main__":
    main()
