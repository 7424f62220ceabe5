"""`python3 bench.py --gpus N` without a launcher starts its N ranks itself.  CPU tests of the
launcher: the environment / argument construction, the refusal when fewer GPUs are visible than asked for, the relay of
rank 0's stdout, the worst exit code, and the end of the surviving ranks when one dies.  The ranks here are a stand-in
script that never imports torch: the launcher must work without touching a GPU."""
import importlib.util
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_rank_commands_env_and_argv():
    b = _bench()
    cmds = b.rank_commands(4, ["--gpus", "4", "--steps", "7"], 29517, base_env={"PATH": "/bin", "RANK": "99"}, python="py", script="bench.py")
    assert len(cmds) == 4
    for r, (argv, env) in enumerate(cmds):
        assert argv == ["py", "bench.py", "--gpus", "4", "--steps", "7"]
        assert env["RANK"] == str(r) and env["LOCAL_RANK"] == str(r)
        assert env["WORLD_SIZE"] == "4" and env["LOCAL_WORLD_SIZE"] == "4"
        assert env["MASTER_ADDR"] == "127.0.0.1" and env["MASTER_PORT"] == "29517"
        assert env["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
        assert env["PATH"] == "/bin"
    # an inherited setting of the IPC mode is kept
    cmds = b.rank_commands(1, [], 1, base_env={"HSA_ENABLE_IPC_MODE_LEGACY": "1"})
    assert cmds[0][1]["HSA_ENABLE_IPC_MODE_LEGACY"] == "1"


def test_refuses_when_fewer_gpus_than_asked(capsys, monkeypatch):
    b = _bench()
    monkeypatch.delenv("GM_BENCH_DEBUG_GLOO", raising=False)
    assert b.launch_ranks(8, ["--gpus", "8"], 5.0, have=1) == 2
    assert "8 asked for, 1 GPU(s) visible" in capsys.readouterr().err
    assert b.launch_ranks(2, ["--gpus", "2"], 5.0, have=0) == 2


def _script(tmp_path, body):
    p = tmp_path / "rank.py"
    p.write_text(textwrap.dedent(body))
    return str(p)


def test_relays_rank0_and_returns_worst_code(tmp_path):
    script = _script(tmp_path, """
        import json, os, sys
        r, w = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
        assert os.environ["LOCAL_RANK"] == str(r) and os.environ["MASTER_ADDR"] == "127.0.0.1" and int(os.environ["MASTER_PORT"]) > 0
        print("noise from rank %d" % r)
        if r == 0:
            print(json.dumps({"n_gpus": w, "argv": sys.argv[1:]}))
        sys.exit(3 if (r == 1 and "--fail" in sys.argv) else 0)
    """)
    drv = "import sys; sys.path.insert(0, %r); import importlib.util as u; s = u.spec_from_file_location('b', %r); b = u.module_from_spec(s); s.loader.exec_module(b); sys.exit(b.launch_ranks(3, sys.argv[1:], 60.0, script=%r, have=3, grace_s=1.0))" % (ROOT, os.path.join(ROOT, "bench.py"), script)
    r = subprocess.run([sys.executable, "-c", drv, "--gpus", "3", "--steps", "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == '{"n_gpus": 3, "argv": ["--gpus", "3", "--steps", "2"]}'
    assert "noise from rank 0" in r.stdout and "noise from rank 1" not in r.stdout and "noise from rank 2" in r.stderr
    r = subprocess.run([sys.executable, "-c", drv, "--gpus", "3", "--fail"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 3


def test_a_dead_rank_ends_the_waiting_ones(tmp_path):
    script = _script(tmp_path, """
        import os, sys, time
        if os.environ["RANK"] == "1":
            sys.exit(7)
        time.sleep(600)       # a rank waiting in a collective for a peer that is gone
    """)
    drv = "import sys; sys.path.insert(0, %r); import importlib.util as u; s = u.spec_from_file_location('b', %r); b = u.module_from_spec(s); s.loader.exec_module(b); sys.exit(b.launch_ranks(2, [], 300.0, script=%r, have=2, grace_s=1.0))" % (ROOT, os.path.join(ROOT, "bench.py"), script)
    r = subprocess.run([sys.executable, "-c", drv], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode != 0 and "ending the others" in r.stderr


def test_plain_invocation_without_gpus_exits_nonzero_with_a_message():
    """`python3 bench.py --gpus 2` on a box with no GPU: a message and a non-zero exit, not a silent one-GPU measurement."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "GM_BENCH_DEBUG_GLOO")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    import torch
    if torch.cuda.device_count() >= 2:
        return      # a real multi-GPU host: the launcher would run the bench; not this test's business
    assert r.returncode == 2 and "GPU(s) visible" in r.stderr and r.stdout.strip() == ""


def test_visible_gpus_counts_from_sysfs_without_hip(tmp_path):
    """The launcher counts its devices from the KFD topology (a node with simd_count > 0 is a GPU) and the *_VISIBLE_DEVICES
    variables — no HIP call, no torch import in the parent: a made-up topology of one CPU node and three GPU nodes."""
    b = _bench()
    for i, simd in enumerate((0, 1024, 1024, 1024)):
        d = tmp_path / str(i)
        d.mkdir()
        (d / "properties").write_text("cpu_cores_count %d\nsimd_count %d\nmem_banks_count 1\n" % (64 if simd == 0 else 0, simd))
    nodes = str(tmp_path)
    assert b.visible_gpus(nodes, env={}) == 3
    assert b.visible_gpus(nodes, env={"HIP_VISIBLE_DEVICES": "0,2"}) == 2
    assert b.visible_gpus(nodes, env={"HIP_VISIBLE_DEVICES": ""}) == 0
    assert b.visible_gpus(nodes, env={"ROCR_VISIBLE_DEVICES": "1", "HIP_VISIBLE_DEVICES": "0"}) == 1
    assert b.visible_gpus(nodes, env={"HIP_VISIBLE_DEVICES": "0,7,1"}) == 1          # the runtime stops at the first invalid index
    assert b.visible_gpus(nodes, env={"CUDA_VISIBLE_DEVICES": "2,1,0"}) == 3
    src = open(os.path.join(ROOT, "bench.py")).read()
    body = src[src.index("def visible_gpus"):src.index("def launch_ranks")]
    assert "import torch" not in body.replace('"import torch; print(torch.cuda.device_count())"', "")   # only inside the child's -c string


def test_config_head_fits_the_drivers_parse():
    """The driver's `parsed.config` kept the first 24 keys of `config` in round 5 and so lost the receiver / cfg4 / cfg5 scalars
    (VERDICT round 5, item 3).  bench.py now sends an explicit head: at N = 1 it must fit in 24 keys and hold one scalar per
    BASELINE config plus the other half of the metric; the multi-GPU head (with the exchange keys) may not push the tracking
    half of the metric out either."""
    import ast
    import re
    src = open(os.path.join(ROOT, "bench.py")).read()
    body = src[src.index("        head = [\"workload\""):src.index("        first = [k for k in head")]
    lists = [ast.literal_eval(m) for m in re.findall(r"(\[[^\]]*\])", body)]
    single = lists[0] + lists[2]
    multi = lists[0] + lists[1] + lists[2]
    assert len(single) == len(set(single)) <= 24, len(single)
    for k in ("workload", "tracking_ch_msps", "tracking_frac", "receiver_x_real_time", "cfg4_grid_ms_per_dwell",
              "cfg4_galileo_corr_kernel_ms", "cfg5_ch_msps", "cfg5_ms_per_code_period", "frontend_msps", "cfg1_ms_per_dwell"):
        assert k in single[:24], k
    for k in ("exchange", "tracking_ch_msps", "tracking_frac", "cfg4_grid_ms_per_dwell", "cfg5_ch_msps"):
        assert k in multi[:24], k
    # every head key is one the line actually carries
    for k in multi:
        assert ('"%s"' % k) in src.replace(body, ""), k


def test_help_lists_full_and_dump_outputs():
    """A plain run times the headline only; the informative legs need --full, the outputs --dump-outputs."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


def test_dump_outputs_writes_the_metrics_block_and_the_decision(tmp_path):
    """bench.py --dump-outputs: the [3][P][D] metrics words (max f32, argmax u32, sum f32) and the decision per PRN, each as a
    float32 / float64 .npy with the values the words and the results hold."""
    import numpy as np
    import torch
    b = _bench()
    P, D = 3, 4
    mx = (np.arange(P * D, dtype=np.float32) * 1.25 + 0.5).reshape(P, D)
    am = (np.arange(P * D, dtype=np.uint32) * 977 + 3).reshape(P, D)
    sm = (np.arange(P * D, dtype=np.float32) * -3.5 + 1e6).reshape(P, D)
    words = np.concatenate([mx.view(np.int32).ravel(), am.view(np.int32).ravel(), sm.view(np.int32).ravel()])
    hit = dict(prn=2, code_phase_samples=7123, code_phase_chips=911.25, carrier_freq=-1250.0, fs=8e6, mag_relative=12.5,
               sample_global_index=80000, doppler_bin=15)
    out = tmp_path / "out"
    b.dump_outputs(str(out), torch.from_numpy(words), [None, hit, None], P, D)
    got = {p.stem: np.load(p) for p in out.glob("*.npy")}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values()), {k: a.dtype for k, a in got.items()}
    assert np.array_equal(got["metrics_max"], mx) and np.array_equal(got["metrics_sum"], sm)
    assert np.array_equal(got["metrics_argmax"], am.astype(np.float64))
    assert got["found"].tolist() == [0.0, 1.0, 0.0] and got["prn"].tolist() == [0.0, 2.0, 0.0]
    for k in b.RESULT_FIELDS:
        assert got[k].tolist() == [0.0, float(hit[k]), 0.0], k
