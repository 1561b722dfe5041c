"""Key-frames of a session and the session map, the parts that need no device: mh_map_insert_frames is declared, exported and
bound, and mh_map_frame has the layout the binding assumes; the key-frame file round-trips bit for bit, has the documented
layout and its reader refuses every damaged file; KeyFrameStore decides as its numpy restatement (tests/simplemap_ref.py); the
driver reads the simplemap: block and refuses what it does not implement."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import simplemap_ref
from mola_lidar_odometry_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "molahip.h")
PIPE = os.path.join(ROOT, "pipelines", "lidar3d-default-hip.yaml")
F = np.float32


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_insert_frames_is_declared_exported_and_bound():
    src = open(HEADER).read()
    L = capi.lib()
    assert re.search(r"MH_API\s+mh_status\s+mh_map_insert_frames\s*\(", src)
    assert hasattr(L, "mh_map_insert_frames") and "mh_map_insert_frames" in capi._SIGNATURES
    assert callable(capi.Map.insert_frames) and callable(capi.Map.insert_frames_device)
    assert capi.MAX_INSERT_FRAMES == int(re.search(r"#define\s+MH_MAX_INSERT_FRAMES\s+(\d+)", src).group(1)) == 1 << 20
    assert int(L.mh_abi_version()) == 7 and re.search(r"^#define\s+MH_ABI_VERSION\s+7\s*$", src, re.M)


def test_map_frame_layout_in_c_and_in_the_binding(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "molahip.h"\nint main(void){ printf("%zu %zu %zu %zu %zu %zu\\n", '
                    'sizeof(mh_map_frame), offsetof(mh_map_frame, x), offsetof(mh_map_frame, y), offsetof(mh_map_frame, z), '
                    'offsetof(mh_map_frame, n), offsetof(mh_map_frame, T)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["128", "0", "8", "16", "24", "32"]
    M = capi.MapFrame
    assert (C.sizeof(M), M.x.offset, M.y.offset, M.z.offset, M.n.offset, M.T.offset) == (128, 0, 8, 16, 24, 32)


# ---- the key-frame file ------------------------------------------------------------------------------------------------------------
def _params(**kw):
    p = dict(voxel_size=1.5, max_points_per_voxel=20, index_mode=0, min_distance_between_points=0.05, ndt_max_eigen_ratio=0.1,
             ndt_min_points=4, far_voxel_metric=1)
    p.update(kw)
    return p


def _set():
    """two target maps, four frames: one without points, one with an empty layer, one carrying -0.0, a denormal and 3.4e38"""
    rng = np.random.default_rng(2)
    maps = [dict(name="localmap", class_name="NDT", params=_params(), remove_voxels_farther_than=80.0),
            dict(name="", class_name="CVoxelMap", params=_params(voxel_size=0.25, max_points_per_voxel=0, index_mode=1,
                                                                 min_distance_between_points=0.0, ndt_max_eigen_ratio=0.0,
                                                                 ndt_min_points=0, far_voxel_metric=0), remove_voxels_farther_than=0.0)]

    def frame(t, layers, twist=None, seed=0):
        r = np.random.default_rng(seed)
        return dict(timestamp=t, pose=list(np.asarray(synth.pose_from_ypr(r.uniform(-1, 1, 6))).reshape(12)),
                    cov=list(r.normal(0, 1e-3, 36)), twist=twist, layers=layers)
    odd = rng.normal(0, 20, (9, 3)).astype(F)
    odd[4] = [F(-0.0), F(1e-42), F(3.4e38)]
    frames = [frame(1700000000.125, [(0, rng.normal(0, 20, (37, 3)).astype(F)), (1, rng.normal(0, 5, (5, 3)).astype(F))], seed=1),
              frame(1700000000.225, None, twist=[1.0, -0.5, 0.0, 0.01, 0.0, -0.2], seed=2),
              frame(1700000000.325, [(0, np.zeros((0, 3), F)), (1, odd)], twist=[0.0] * 6, seed=3),
              frame(1700000000.425, [(1, rng.normal(0, 5, (3, 3)).astype(F))], seed=4)]
    frames[0]["cov"] = [0.0] * 36   # a first scan
    return dict(maps=maps, frames=frames)


def _same_set(got, ref):
    assert len(got["maps"]) == len(ref["maps"]) and len(got["frames"]) == len(ref["frames"])
    for g, r in zip(got["maps"], ref["maps"]):
        assert g["name"] == r["name"] and g["class_name"] == r["class_name"]
        assert F(g["remove_voxels_farther_than"]) == F(r["remove_voxels_farther_than"])
        for k, v in r["params"].items():
            assert (F(g["params"][k]).tobytes() == F(v).tobytes()) if isinstance(v, float) else (g["params"][k] == v), k
    for g, r in zip(got["frames"], ref["frames"]):
        assert g["timestamp"] == r["timestamp"]
        assert np.asarray(g["pose"]).tobytes() == np.asarray(r["pose"], np.float64).tobytes()
        assert np.asarray(g["cov"]).tobytes() == np.asarray(r["cov"], np.float64).tobytes()
        assert (g["twist"] is None) == (r["twist"] is None) and (r["twist"] is None or list(g["twist"]) == list(r["twist"]))
        assert (g["layers"] is None) == (r["layers"] is None)
        if r["layers"] is not None:
            assert len(g["layers"]) == len(r["layers"])
            for (gi, gx), (ri, rx) in zip(g["layers"], r["layers"]):
                assert gi == ri and gx.dtype == F and gx.shape == rx.shape and gx.tobytes() == rx.tobytes()


def _fnv1a(b):
    h = 0xcbf29ce484222325
    for c in b:
        h = ((h ^ c) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def _pack(s, checksum=True, version=1):
    """the byte layout of INTEGRATION.md, restated independently of the writer"""
    b = b"MHKEYFRM" + struct.pack("<II", version, len(s["maps"]))
    for m in s["maps"]:
        p = m["params"]
        for text in (m["name"], m["class_name"]):
            b += struct.pack("<I", len(text.encode())) + text.encode()
        b += struct.pack("<fIIffII", p["voxel_size"], p["max_points_per_voxel"], p["index_mode"], p["min_distance_between_points"],
                         p["ndt_max_eigen_ratio"], p["ndt_min_points"], p["far_voxel_metric"])
        b += struct.pack("<f", m["remove_voxels_farther_than"])
    b += struct.pack("<Q", len(s["frames"]))
    for f in s["frames"]:
        b += struct.pack("<d12d36d", f["timestamp"], *f["pose"], *f["cov"])
        b += b"\x00" if f["twist"] is None else b"\x01" + struct.pack("<6d", *f["twist"])
        if f["layers"] is None:
            b += b"\x00"
            continue
        b += b"\x01" + struct.pack("<I", len(f["layers"]))
        for idx, xyz in f["layers"]:
            b += struct.pack("<IQ", idx, len(xyz)) + b"".join(np.ascontiguousarray(xyz[:, a], "<f4").tobytes() for a in range(3))
    return b + (struct.pack("<Q", _fnv1a(b)) if checksum else b"")


def _sections(s):
    """byte offsets at which a section of the file ends"""
    ends, at = [], 0

    def step(size):
        nonlocal at
        at += size
        ends.append(at)
    for size in (8, 4, 4):
        step(size)
    for m in s["maps"]:
        for size in (4 + len(m["name"].encode()), 4 + len(m["class_name"].encode()), 7 * 4, 4):
            step(size)
    step(8)
    for f in s["frames"]:
        for size in (8, 96, 288, 1 if f["twist"] is None else 49, 1):
            step(size)
        if f["layers"] is not None:
            step(4)
            for _, xyz in f["layers"]:
                for size in (4, 8, 4 * len(xyz), 4 * len(xyz), 4 * len(xyz)):
                    step(size)
    ends.append(at + 8)
    return ends


def test_keyframe_file_round_trip_and_layout(host, tmp_path):
    path = str(tmp_path / "drive.mhkf")
    s = _set()
    host.write_keyframe_file(path, s)
    back = host.read_keyframe_file(path)
    _same_set(back, s)
    xyz = back["frames"][2]["layers"][1][1]
    assert np.signbit(xyz[4, 0]) and xyz[4, 0] == 0 and 0 < xyz[4, 1] < 1.2e-38 and xyz[4, 2] > 3e38
    assert back["frames"][1]["layers"] is None and back["frames"][2]["layers"][0][1].shape == (0, 3)
    raw = open(path, "rb").read()
    assert raw == _pack(s)                      # the layout, independently of the writer
    assert _sections(s)[-1] == len(raw)
    host.write_keyframe_file(path + "2", back)  # a rewrite gives the same bytes
    assert open(path + "2", "rb").read() == raw
    assert host.KEYFRAME_FILE_VERSION == 1 and host.LOCAL_MAP_FILE_VERSION == 1
    # an empty store is a file too
    host.write_keyframe_file(path + "3", dict(maps=[], frames=[]))
    assert host.read_keyframe_file(path + "3") == dict(maps=[], frames=[])


def test_damaged_keyframe_files_are_refused(host, tmp_path):
    s = _set()
    good = _pack(s)
    path = str(tmp_path / "bad.mhkf")

    def refused(data, match):
        open(path, "wb").write(data)
        with pytest.raises(RuntimeError, match=match):
            host.read_keyframe_file(path)

    open(path, "wb").write(good)
    _same_set(host.read_keyframe_file(path), s)
    refused(b"MHLOCMAP" + good[8:], "wrong magic")
    refused(b"", "wrong magic")
    newer = _pack(s, version=2)
    refused(newer, "newer")
    refused(_pack(s, version=0), "version 0")
    ends = _sections(s)
    for cut in ends[:-1]:                      # truncated at every section boundary ...
        refused(good[:cut], "truncated|trailing|checksum|wrong magic|flag|names target")
    for cut in ends[:-2]:                      # ... and there with a checksum that holds for what is left
        body = good[:cut]
        if len(body) >= 16:
            refused(body + struct.pack("<Q", _fnv1a(body)), "truncated")
    refused(good + b"\x00", "trailing|checksum|truncated")
    body = good[:-8] + b"\x00\x00\x00\x00"
    refused(body + struct.pack("<Q", _fnv1a(body)), "trailing")
    for at in (9, len(good) // 2, len(good) - 9):   # one flipped bit anywhere
        flipped = bytearray(good)
        flipped[at] ^= 0x10
        refused(bytes(flipped), "checksum|truncated|newer|trailing|flag|names target")
    # a layer that names a map the header does not hold; a flag byte that is neither 0 nor 1
    t = _set()
    t["frames"][3]["layers"] = [(2, np.zeros((1, 3), F))]
    refused(_pack(t), "names target map 2")
    with pytest.raises(RuntimeError, match="names target map 2"):
        host.write_keyframe_file(path, t)
    flag_at = _sections(s)[3 + 4 * 2 + 1 + 3] - 1   # frame 0's twist flag
    assert good[flag_at] == 0
    body = bytearray(good[:-8])
    body[flag_at] = 2
    refused(bytes(body) + struct.pack("<Q", _fnv1a(bytes(body))), "neither 0 nor 1")


# ---- the key-frame decision --------------------------------------------------------------------------------------------------------
def _pose_list():
    """a hand-made drive: forward in steps of 0.4 m, a turn on the spot, back towards the start (so that the closest key-frame
    is not the last one), with two rejected alignments on the way"""
    rows, x, y, yaw = [], 0.0, 0.0, 0.0
    for k in range(40):
        if k < 12:
            x += 0.4
        elif k < 20:
            yaw += np.deg2rad(7.0)
        elif k < 32:
            x -= 0.4
            y += 0.05
        else:
            y += 0.7
        rows.append(np.asarray(synth.pose_from_ypr([x, y, 0.01 * k, yaw, 0.0, 0.0])).reshape(12))
    good = np.ones(40, bool)
    good[[0, 7, 25]] = False     # (scan 0 is the first scan: no ICP)
    return rows, good


@pytest.mark.parametrize("add_non_keyframes_too", [False, True])
@pytest.mark.parametrize("last_only", [False, True])
def test_keyframe_store_decides_as_the_restatement(host, last_only, add_non_keyframes_too):
    poses, good = _pose_list()
    lim_t = np.where(np.arange(40) % 2 == 0, 1.0, 1.3)   # the limits are formulas: they change scan by scan
    lim_r = np.full(40, 20.0)
    want_stored, want_kf = simplemap_ref.decide(poses, good, lim_t, lim_r, last_only, add_non_keyframes_too)
    store = host.KeyFrameStore(last_only)
    got = [store.decide(k == 0, bool(good[k]), list(poses[k]), float(lim_t[k]), float(lim_r[k]), add_non_keyframes_too) for k in range(40)]
    assert [g[0] for g in got] == list(want_stored) and [g[1] for g in got] == list(want_kf)
    # the list exercises the rule: key-frames by translation and by rotation, scans in between, rejected ones never stored
    assert want_kf[0] and want_kf[1] and 6 < want_kf.sum() < 30 and not want_stored[7] and not want_stored[25]
    assert want_kf[12:20].any() and (want_stored.sum() == 38 if add_non_keyframes_too else (want_stored == want_kf).all())


def test_the_two_checkers_differ_where_the_drive_comes_back(host):
    poses, good = _pose_list()
    a = simplemap_ref.decide(poses, good, 1.0, 20.0, False)[1]
    b = simplemap_ref.decide(poses, good, 1.0, 20.0, True)[1]
    assert (a != b).any() and (a[:12] == b[:12]).all()   # (the same on the way out: there the closest key-frame is the last one)


# ---- the driver's parameters -------------------------------------------------------------------------------------------------------
def _with_simplemap(block):
    txt = open(PIPE).read()
    head, rest = txt.split("  simplemap:\n", 1)
    tail = rest.split("  adaptive_threshold:\n", 1)[1]
    return head + block + "  adaptive_threshold:\n" + tail


def test_driver_reads_the_simplemap_block(host, monkeypatch):
    for v in ("MOLA_GENERATE_SIMPLEMAP", "MOLA_LOAD_SM", "MOLA_SIMPLEMAP_OUTPUT", "MOLA_SIMPLEMAP_MIN_XYZ", "MOLA_SIMPLEMAP_MIN_ROT",
              "MOLA_SIMPLEMAP_GENERATE_LAZY_LOAD", "MOLA_SIMPLEMAP_ALSO_NON_KEYFRAMES"):
        monkeypatch.delenv(v, raising=False)
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlFile(PIPE))
    o = lo.simplemapOptions()
    assert not o["generate"] and not o["add_non_keyframes_too"] and not o["measure_from_last_kf_only"]
    assert o["save_final_map_to_file"] == "final_map.simplemap" and o["load_existing_simple_map"] == ""
    assert lo.keyFrames() == dict(maps=[], frames=[])
    lo2 = host.LidarOdometry()
    lo2.initialize(host.Config.FromYamlText(_with_simplemap(
        "  simplemap:\n    generate: true\n    measure_from_last_kf_only: true\n    add_non_keyframes_too: true\n"
        "    min_translation_between_keyframes: 2.5\n    min_rotation_between_keyframes: 11\n    save_gnss_max_age: 3.0\n")))
    o = lo2.simplemapOptions()
    assert o["generate"] and o["measure_from_last_kf_only"] and o["add_non_keyframes_too"] and o["save_final_map_to_file"] == ""
    assert o["save_gnss_max_age"] == 3.0
    del lo2   # (generate is on and no file is named: nothing is written)


def test_lazy_load_scan_files_are_refused_at_initialize(host):
    with pytest.raises(RuntimeError, match="generate_lazy_load_scan_files"):
        host.LidarOdometry().initialize(host.Config.FromYamlText(_with_simplemap("  simplemap:\n    generate_lazy_load_scan_files: true\n")))


def test_a_missing_or_foreign_simple_map_is_refused_at_initialize(host, tmp_path):
    with pytest.raises(RuntimeError, match="cannot open"):
        host.LidarOdometry().initialize(host.Config.FromYamlText(_with_simplemap(
            "  simplemap:\n    load_existing_simple_map: '%s'\n" % str(tmp_path / "none.mhkf"))))
    path = str(tmp_path / "other.mhkf")
    host.write_keyframe_file(path, _set())   # recorded for the maps 'localmap' and '': not this pipeline's
    with pytest.raises(RuntimeError, match="other target maps"):
        host.LidarOdometry().initialize(host.Config.FromYamlText(_with_simplemap("  simplemap:\n    load_existing_simple_map: '%s'\n" % path)))


def test_build_session_maps_refuses_an_occupancy_map_target(host):
    with pytest.raises(RuntimeError, match="occupancy map has no snapshot"):
        host.build_session_maps(_set())


def test_build_session_maps_names_an_unknown_class_as_such(host):
    s = _set()
    s["maps"][1]["class_name"] = "HashedVoxelPointcloud"   # misspelt: not an occupancy map, and said so
    with pytest.raises(RuntimeError, match="unknown class 'HashedVoxelPointcloud'") as e:
        host.build_session_maps(s)
    assert "occupancy" not in str(e.value)
