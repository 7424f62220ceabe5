"""The plane ring and tracking on planes on the CPU: the additive entries in every layer (this file fails without the feature), the ABI
number they leave alone, gm_plane_ring_plan and gm_trk_planes_plan (host only, no device) against a Python restatement of their rules
with every boundary on both sides, the NULL-handle refusals of every new entry, gm_plane_ring_create without a device, and the C++
mirror's plans (tests/cpp/trk_planes_plans.cpp, compiled here as the other C++ host tests compile theirs) word for word with Python's."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RING_ENTRIES = ["gm_plane_ring_plan", "gm_plane_ring_create", "gm_plane_ring_destroy", "gm_plane_ring_info", "gm_plane_ring_write_dev",
                "gm_plane_ring_write", "gm_plane_ring_get_head", "gm_plane_ring_copy_to_slice", "gm_plane_ring_synchronize"]
TRK_ENTRIES = ["gm_trk_planes_plan", "gm_trk_set_channel_planes", "gm_trk_get_channel_planes", "gm_trk_update_planes", "gm_trk_update_planes_dev"]
OK, INVALID_ARG, NO_DEVICE, OUT_OF_RANGE = 0, -1, -3, -5


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


# ---- the rules, restated --------------------------------------------------------------------------------------------------------------
def ring_model(n_planes, plane_size):
    """-> bytes, or the status of the refusal"""
    if not 1 <= n_planes <= 64:
        return OUT_OF_RANGE
    if plane_size < 1 or plane_size & (plane_size - 1):
        return OUT_OF_RANGE
    if n_planes * plane_size * 8 > 1 << 34:
        return OUT_OF_RANGE
    return n_planes * plane_size * 8


def samples_model(fs, code_rate, code_len):
    """round(fs / (code_rate / code_len)) in f32, the tracker's samples_per_code; roundf rounds halves away from zero"""
    v = np.float32(fs) / (np.float32(code_rate) / np.float32(code_len))
    return int(np.floor(np.float64(v) + 0.5)) if v > 0 else 0


def planes_model(fs, n_channels, n_planes, planes=None, max_epochs=1, n_arms=3, code_rate=0.0, code_len=0, strict_sum_order=False):
    """-> the plan's dict, or the status of the refusal, in the order the library checks"""
    if not (fs > 0 and np.isfinite(fs)) or n_channels < 1:
        return INVALID_ARG
    if strict_sum_order:
        return INVALID_ARG
    if max_epochs == 0:
        return INVALID_ARG
    if max_epochs > 4095:
        return OUT_OF_RANGE
    if not 1 <= n_planes <= 64:
        return OUT_OF_RANGE
    if code_len > 16384:
        return OUT_OF_RANGE
    m = [0] * n_channels if planes is None else list(planes)
    if any(p >= n_planes for p in m):
        return OUT_OF_RANGE
    n = samples_model(fs, code_rate or 1.023e6, code_len or 1023)
    return dict(workgroups=n_channels, threads=256, chip_row_bytes=code_len or 1023, planes_used=len(set(m)), samples=n,
                samples_per_lane=(n + 255) // 256 if 0 < n < 1 << 31 else 0, result_bytes=(max_epochs * n_channels * 43 + 3) // 4 * 4)


RING_TABLE = [(0, 16), (1, 16), (64, 16), (65, 16), (3, 0), (3, 1), (3, 2), (3, 3), (3, 6), (3, 1 << 14), (3, (1 << 14) + 1), (3, (1 << 14) - 1),
              (64, 1 << 25), (64, 1 << 26), (1, 1 << 31), (1, 1 << 32), (2, 1 << 30), (3, 1 << 30), (32, 1 << 26), (33, 1 << 26), (1, 1 << 63)]
MAP = [2, 0, 2, 1, 0]
TRK_TABLE = [
    dict(n_planes=3, planes=MAP, max_epochs=12), dict(n_planes=3, planes=None, max_epochs=1), dict(n_planes=5, planes=[4, 2, 4, 3, 2]),
    dict(n_planes=3, planes=MAP, max_epochs=0), dict(n_planes=3, planes=MAP, max_epochs=1), dict(n_planes=3, planes=MAP, max_epochs=4095),
    dict(n_planes=3, planes=MAP, max_epochs=4096),
    dict(n_planes=0), dict(n_planes=1), dict(n_planes=64, planes=[63, 0, 63, 1, 0]), dict(n_planes=65), dict(n_planes=64, planes=[64, 0, 0, 0, 0]),
    dict(n_planes=3, planes=[2, 0, 2, 1, 3]), dict(n_planes=2, planes=MAP), dict(n_planes=3, planes=[0, 0, 0, 0, 2]),
    dict(n_planes=3, planes=MAP, code_len=16384, code_rate=1.023e6), dict(n_planes=3, planes=MAP, code_len=16385, code_rate=1.023e6),
    dict(n_planes=3, planes=MAP, code_len=4092, code_rate=1.023e6, fs=4.092e6, n_arms=5), dict(n_planes=3, planes=MAP, strict_sum_order=True),
    dict(n_planes=3, planes=MAP, fs=0.0), dict(n_planes=3, n_channels=0, planes=None), dict(n_planes=3, n_channels=1, planes=[2]),
    dict(n_planes=3, planes=MAP, code_rate=1.0235e6), dict(n_planes=3, planes=MAP, code_rate=1.0225e6), dict(n_planes=3, planes=MAP, fs=5.0e6),
    dict(n_planes=3, planes=MAP, fs=16.368e6, n_channels=5, max_epochs=16), dict(n_planes=3, planes=MAP, fs=1.0e-3),
]


def _trk_kw(kw):
    return dict(dict(fs=2.048e6, n_channels=5), **kw)


# ---- layers ---------------------------------------------------------------------------------------------------------------------------
def test_the_entries_are_in_every_layer(gm):
    import gnss_sdr_rs_amd
    from gnss_sdr_rs_amd import _lib, tracking
    header = _read("include", "gnss_mi355x.h")
    rust = _read("rust", "src", "mi355x.rs")
    L = gm.lib()
    pattern = re.search(r"global:\s*([^;]+);", _read("gnss-sdr-rs_amd", "csrc", "exports.map")).group(1).strip()
    with open(_lib.library_path(), "rb") as f:      # the dynamic symbols of the built library, read from its file
        blob = f.read()
    hpp = _read("gnss-sdr-rs_amd", "host", "gnss_sdr.hpp")
    for name in RING_ENTRIES + TRK_ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert "pub fn %s(" % name in rust, name
        assert re.fullmatch(pattern.replace("*", ".*"), name), (pattern, name)
        assert getattr(L, name) is not None
        assert name.encode() + b"\0" in blob, name
        assert name + "(" in hpp, name
        for doc in ("README.md", "INTEGRATION.md"):
            assert name in _read(doc), (doc, name)
    for method in ("write_dev", "write", "get_head", "copy_to_slice", "synchronize", "close"):
        assert callable(getattr(tracking.PlaneRing, method)), method
    for method in ("set_channel_planes", "channel_planes", "update_planes", "update_planes_dev"):
        assert callable(getattr(tracking.TrackingManager, method)), method
        assert method + "(" in hpp, method
    assert callable(tracking.plane_ring_plan) and callable(tracking.planes_plan)
    assert gnss_sdr_rs_amd.PlaneRing is tracking.PlaneRing and gnss_sdr_rs_amd.trk_planes_plan is tracking.planes_plan
    assert "class PlaneRing" in hpp and "planes_plan(" in hpp
    internal = _read("gnss-sdr-rs_amd", "csrc", "gm_internal.h")
    assert "launch_trk_planes" in internal and "TrkPlanesArgs" in internal and "launch_plane_ring_write" in internal
    kernel = _read("gnss-sdr-rs_amd", "csrc", "trk_planes.hip")
    assert "trk_planes_kernel" in kernel and "plane_ring_write_kernel" in kernel
    assert "correlate_sample<ARMS, true>" in kernel and "correlate_sample<ARMS, false>" in kernel and "epoch_epilogue<ARMS>" in kernel
    assert "atomic" not in re.sub(r"//[^\n]*", "", kernel)                    # no atomics, no spin wait: nothing is shared between workgroups
    assert '#include "trk_planes.hip"' in _read("gnss-sdr-rs_amd", "csrc", "trk_kernels.hip")
    assert "trk_planes.hip" in _read("gnss-sdr-rs_amd", "build.py")
    for words in ("ONE head", "ENQUEUED", "ORDERING, all on the device", "EVERY OTHER ENTRY IGNORES IT", "FIXED TREE",
                  "THE SEQUENTIAL-SUM PARITY PATH ON PLANES IS NOT\n * BUILT", 'UNLIKE gm_trk_bank it makes no "already overwritten" test',
                  "(int64)(head - (next_sample_index + n)) >= 0", "ALONE"):
        assert words in header, words
    readme = _read("README.md")
    assert "## Tracking on planes" in readme and readme.index("## Tracking on planes") > readme.index("Correlator bank at tracked states")
    assert "trk_planes.hip" in readme and "4.3c" in _read("DESIGN.md")
    stats = _read("profiles", "trk_planes_kernel_stats.txt")
    for row in re.findall(r"^.*trk_planes_kernel<\d>.*$", stats, re.M):
        assert re.match(r"\s*0 scratch insts\s+0 B", row), row                  # scratch must be 0
    assert len(re.findall(r"trk_planes_kernel<\d>", stats)) == 2 and "plane_ring_write_kernel" in stats and "trk_persistent_kernel" in stats
    # the struct layout, in every layer
    P = _lib.TrkPlanesPlanOut
    assert C.sizeof(P) == 40 and (P.samples.offset, P.samples_per_lane.offset, P.result_bytes.offset) == (16, 24, 32)
    body = re.search(r"pub struct GmTrkPlanesPlanOut\s*\{([^}]*)\}", rust, re.S).group(1)
    assert re.findall(r"pub\s+(\w+)\s*:", re.sub(r"//[^\n]*", "", body)) == [f[0] for f in P._fields_]
    cstruct = re.search(r"typedef struct \{([^}]*)\}\s*gm_trk_planes_plan_out;", header, re.S).group(1)
    names = []
    for decl in re.sub(r"/\*.*?\*/", "", cstruct, flags=re.S).split(";"):
        names += [w.strip(" *") for w in re.sub(r"^\s*(const\s+)?\w+\s", "", decl.strip()).split(",") if w.strip()]
    assert names == [f[0] for f in P._fields_], names


def test_the_abi_number_stays(gm):
    from gnss_sdr_rs_amd import _lib
    import __graft_entry__ as entry
    assert gm.lib().gm_abi_version() == entry.header_abi_version() == 9
    assert C.sizeof(_lib.TrkState) == 64 and C.sizeof(_lib.TrkOut) == 40 and C.sizeof(_lib.TrkCfg) == 104      # no existing struct changed


# ---- the two plans --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_planes,plane_size", RING_TABLE)
def test_plane_ring_plan_holds_every_rule(gm, n_planes, plane_size):
    from gnss_sdr_rs_amd import _lib, tracking
    want = ring_model(n_planes, plane_size)
    if want >= 0:
        assert tracking.plane_ring_plan(n_planes, plane_size) == want
        assert gm.lib().gm_plane_ring_plan(n_planes, plane_size, None) == OK          # the output may be NULL
    else:
        b = C.c_uint64(77)
        assert gm.lib().gm_plane_ring_plan(n_planes, plane_size, C.byref(b)) == want and b.value == 77 and gm.lib().gm_last_error()
        with pytest.raises(_lib.GmError) as e:
            tracking.plane_ring_plan(n_planes, plane_size)
        assert e.value.status == want


def test_the_ring_tables_boundaries_fall_on_both_sides():
    got = {k: ring_model(*k) for k in RING_TABLE}
    assert got[(1, 16)] == 128 and got[(64, 16)] == 8192 and got[(0, 16)] == got[(65, 16)] == OUT_OF_RANGE
    assert got[(3, 1)] == 24 and got[(3, 0)] == got[(3, 3)] == got[(3, (1 << 14) + 1)] == OUT_OF_RANGE
    assert got[(64, 1 << 25)] == got[(1, 1 << 31)] == got[(2, 1 << 30)] == got[(32, 1 << 26)] == 1 << 34
    assert got[(64, 1 << 26)] == got[(1, 1 << 32)] == got[(3, 1 << 30)] == got[(33, 1 << 26)] == got[(1, 1 << 63)] == OUT_OF_RANGE


@pytest.mark.parametrize("kw", TRK_TABLE, ids=[str(i) for i in range(len(TRK_TABLE))])
def test_planes_plan_holds_every_rule(gm, kw):
    from gnss_sdr_rs_amd import _lib, tracking
    kw = _trk_kw(kw)
    want = planes_model(**kw)
    if isinstance(want, dict):
        assert tracking.planes_plan(**kw) == want, kw
    else:
        with pytest.raises(_lib.GmError) as e:
            tracking.planes_plan(**kw)
        assert e.value.status == want, kw


def test_the_trk_tables_boundaries_fall_on_both_sides():
    st = [planes_model(**_trk_kw(kw)) for kw in TRK_TABLE]
    ok = [isinstance(s, dict) for s in st]
    assert ok == [True, True, True, False, True, True, False, False, True, True, False, False, False, False, True, True, False, True, False,
                  False, False, True, True, True, True, True, True]
    assert st[3] == INVALID_ARG and st[6] == OUT_OF_RANGE and st[7] == st[10] == st[11] == st[12] == st[13] == st[16] == OUT_OF_RANGE
    assert st[18] == st[19] == st[20] == INVALID_ARG
    assert st[0] == dict(workgroups=5, threads=256, chip_row_bytes=1023, planes_used=3, samples=2048, samples_per_lane=8, result_bytes=2580)
    assert (st[22]["samples"], st[23]["samples"], st[24]["samples"], st[17]["samples"], st[25]["samples"]) == (2047, 2049, 5000, 16368, 16368)
    assert st[17]["chip_row_bytes"] == 4092 and st[1]["planes_used"] == 1 and st[26]["samples"] == 0 and st[26]["samples_per_lane"] == 0


def test_planes_plan_names_the_channel_and_leaves_the_output(gm):
    from gnss_sdr_rs_amd import _lib
    L = gm.lib()
    trk = _lib.TrkCfg()
    trk.fs, trk.n_channels = 2.048e6, 5
    out = _lib.TrkPlanesPlanOut()
    out.samples = 77
    m = (C.c_uint32 * 5)(2, 0, 2, 3, 0)
    assert L.gm_trk_planes_plan(C.byref(trk), 3, m, 4, C.byref(out)) == OUT_OF_RANGE and b"channel 3" in L.gm_last_error()
    assert L.gm_trk_planes_plan(None, 3, m, 4, C.byref(out)) == INVALID_ARG
    trk.strict_sum_order = 1
    m[3] = 1
    assert L.gm_trk_planes_plan(C.byref(trk), 3, m, 4, C.byref(out)) == INVALID_ARG and b"strict_sum_order" in L.gm_last_error()
    assert out.samples == 77                                       # a refusal leaves the output untouched
    trk.strict_sum_order = 0
    assert L.gm_trk_planes_plan(C.byref(trk), 3, m, 4, None) == OK          # the output may be NULL
    assert L.gm_trk_planes_plan(C.byref(trk), 3, m, 4, C.byref(out)) == OK and out.samples == 2048 and out.result_bytes == 4 * 5 * 43


# ---- NULL handles, no device ----------------------------------------------------------------------------------------------------------
def test_every_new_entry_refuses_a_null_handle(gm):
    L = gm.lib()
    buf = (C.c_uint8 * 256)()
    v32, v64, vp = C.c_uint32(9), C.c_uint64(9), C.c_void_p(9)
    calls = {
        "gm_plane_ring_info": lambda: L.gm_plane_ring_info(None, C.byref(v32), C.byref(v64), C.byref(v64), C.byref(vp)),
        "gm_plane_ring_write_dev": lambda: L.gm_plane_ring_write_dev(None, C.c_void_p(4096), 16, 16, None),
        "gm_plane_ring_write": lambda: L.gm_plane_ring_write(None, C.cast(buf, C.c_void_p), 16, 16),
        "gm_plane_ring_get_head": lambda: L.gm_plane_ring_get_head(None, C.byref(v64)),
        "gm_plane_ring_copy_to_slice": lambda: L.gm_plane_ring_copy_to_slice(None, 0, 0, C.cast(buf, C.c_void_p), 4),
        "gm_plane_ring_synchronize": lambda: L.gm_plane_ring_synchronize(None),
        "gm_trk_set_channel_planes": lambda: L.gm_trk_set_channel_planes(None, C.cast(buf, C.c_void_p)),
        "gm_trk_get_channel_planes": lambda: L.gm_trk_get_channel_planes(None, C.cast(buf, C.c_void_p)),
        "gm_trk_update_planes": lambda: L.gm_trk_update_planes(None, None, 4, C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p), C.byref(v32)),
        "gm_trk_update_planes_dev": lambda: L.gm_trk_update_planes_dev(None, None, 4),
        "gm_trk_planes_plan": lambda: L.gm_trk_planes_plan(None, 3, None, 1, None),
        "gm_plane_ring_create": lambda: L.gm_plane_ring_create(3, 16, None),
    }
    for name, f in calls.items():
        assert f() == INVALID_ARG and b"null" in L.gm_last_error(), (name, L.gm_last_error())
    assert set(calls) | {"gm_plane_ring_plan", "gm_plane_ring_destroy"} == set(RING_ENTRIES + TRK_ENTRIES)
    assert L.gm_plane_ring_destroy(None) == OK                     # destroy(NULL) is a no-op, as for every handle
    assert (v32.value, v64.value, vp.value) == (9, 9, 9) and not any(buf)


def test_plane_ring_create_fails_loudly_without_a_device(gm):
    """in a process that has selected no device (gm_init was never called): GM_ERR_NO_DEVICE, a message, no handle"""
    code = ("import sys; sys.path.insert(0, %r); import ctypes as C; import gnss_sdr_rs_amd as g; L = g.lib(); h = C.c_void_p(5);"
            "rc = L.gm_plane_ring_create(3, 1 << 14, C.byref(h)); print(rc, h.value, L.gm_last_error().decode())") % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    assert out.returncode == 0, out.stderr
    rc, handle, message = out.stdout.strip().splitlines()[-1].split(" ", 2)
    assert int(rc) == NO_DEVICE and handle == "None" and "device" in message, out.stdout


# ---- the C++ mirror -------------------------------------------------------------------------------------------------------------------
def _line(kind, got):
    if not isinstance(got, dict):
        return "%s refused %d" % (kind, got)
    return kind + " " + " ".join("%s %d" % (k, v) for k, v in got.items())


def test_cpp_mirror_prints_the_same_plans(gm, tmp_path):
    from gnss_sdr_rs_amd import _lib, tracking
    exe = os.path.join(ROOT, "gnss-sdr-rs_amd", "build", "trk_planes_plans")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    libdir = os.path.dirname(gm.library_path())
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "gnss-sdr-rs_amd", "host"),
           os.path.join(ROOT, "tests", "cpp", "trk_planes_plans.cpp"), "-o", exe, "-L", libdir, "-lgnss_mi355x",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lines, want = [], []
    for n_planes, plane_size in RING_TABLE:
        lines.append("ring %d %d" % (n_planes, plane_size))
        try:
            want.append("ring bytes %d" % tracking.plane_ring_plan(n_planes, plane_size))
        except _lib.GmError as e:
            want.append("ring refused %d" % e.status)
    for kw in TRK_TABLE:
        kw = _trk_kw(kw)
        if kw["n_channels"] == 0:
            continue                                               # (the C++ mirror tells "no map" by an empty vector)
        m = kw.get("planes")
        lines.append("trk %r %d %d %d %r %d %d %d %s" % (kw["fs"], kw["n_channels"], kw.get("n_arms", 3), kw.get("code_len", 0), kw.get("code_rate", 0.0),
                                                         int(kw.get("strict_sum_order", False)), kw["n_planes"], kw.get("max_epochs", 1),
                                                         "-" if m is None else ",".join(str(p) for p in m)))
        try:
            want.append(_line("trk", tracking.planes_plan(**kw)))
        except _lib.GmError as e:
            want.append("trk refused %d" % e.status)
    case = tmp_path / "cases.txt"
    case.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(case)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0, r.stdout
    got = r.stdout.strip().splitlines()
    assert len(got) == len(want) >= 40
    for g, w, l in zip(got, want, lines):
        assert g == w, (l, g, w)
    assert sum("refused" in w for w in want) >= 15 and sum("refused" not in w for w in want) >= 20
