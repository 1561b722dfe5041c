"""Localization in a saved map, the parts that need no device: the two new entry points are declared, exported and bound; the
local-map file round-trips bit for bit and its reader refuses every damaged file; the candidate grid of a relocalization
agrees with its numpy restatement (tests/score_ref.py); the -hip pipelines carry the new keys."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import score_ref as sr
from mola_lidar_odometry_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "molahip.h")
PIPES = [os.path.join(ROOT, "pipelines", n) for n in ("lidar3d-default-hip.yaml", "lidar3d-ndt-hip.yaml")]
F = np.float32


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_exported_and_bound():
    src = open(HEADER).read()
    L = capi.lib()
    for fn in ("mh_map_restore", "mh_score_poses"):
        assert re.search(r"MH_API\s+mh_status\s+%s\s*\(" % fn, src), fn
        assert hasattr(L, fn) and fn in capi._SIGNATURES
    assert callable(capi.score_poses) and callable(capi.Map.restore) and callable(capi.Map.restore_device)
    assert capi.SCORE_MAX_POSES == int(re.search(r"#define\s+MH_SCORE_MAX_POSES\s+(\d+)", src).group(1)) == 1 << 20


def test_pose_score_is_16_bytes_in_c_and_in_the_binding(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "molahip.h"\nint main(void){ printf("%zu %zu %zu %zu\\n", '
                    'sizeof(mh_pose_score), offsetof(mh_pose_score, n_paired), offsetof(mh_pose_score, reserved_), '
                    'offsetof(mh_pose_score, cost)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["16", "0", "4", "8"]
    assert C.sizeof(capi.PoseScore) == 16 and capi.PoseScore.cost.offset == 8
    assert capi.POSE_SCORE_DTYPE.itemsize == 16 and capi.POSE_SCORE_DTYPE.fields["cost"][1] == 8
    assert sr.SCORE_DTYPE == capi.POSE_SCORE_DTYPE


def test_abi_version_is_still_7():
    assert int(capi.lib().mh_abi_version()) == 7
    assert re.search(r"^#define\s+MH_ABI_VERSION\s+7\s*$", open(HEADER).read(), re.M)


# ---- the map file ------------------------------------------------------------------------------------------------------------------
def _maps():
    rng = np.random.default_rng(1)
    n = 1234
    a = dict(name="localmap", class_name="NDT",
             params=dict(voxel_size=1.5, max_points_per_voxel=20, index_mode=0, min_distance_between_points=0.05,
                         ndt_max_eigen_ratio=0.1, ndt_min_points=4, far_voxel_metric=1),
             remove_voxels_farther_than=80.0, n_offered=98765432109, xyz=rng.normal(0, 30, (n, 3)).astype(F),
             src_idx=rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32))
    a["xyz"][7] = [np.float32(-0.0), np.float32(1e-42), np.float32(3.4e38)]   # a negative zero, a denormal, a huge value
    b = dict(name="", class_name="SparseTreesPointCloud",
             params=dict(voxel_size=10.0, max_points_per_voxel=0, index_mode=1, min_distance_between_points=0.0,
                         ndt_max_eigen_ratio=0.0, ndt_min_points=0, far_voxel_metric=0),
             remove_voxels_farther_than=0.0, n_offered=0, xyz=np.zeros((0, 3), F), src_idx=np.zeros(0, np.uint32))
    return [a, b]


def _same_map(got, ref):
    assert got["name"] == ref["name"] and got["class_name"] == ref["class_name"] and got["n_offered"] == ref["n_offered"]
    for k, v in ref["params"].items():
        assert np.float32(got["params"][k]).tobytes() == np.float32(v).tobytes() if isinstance(v, float) else got["params"][k] == v, k
    assert np.float32(got["remove_voxels_farther_than"]) == np.float32(ref["remove_voxels_farther_than"])
    assert got["xyz"].dtype == F and got["xyz"].shape == ref["xyz"].shape and got["xyz"].tobytes() == ref["xyz"].tobytes()
    assert got["src_idx"].dtype == np.uint32 and got["src_idx"].tobytes() == ref["src_idx"].tobytes()


def _sections(maps):
    """byte offsets at which a section of the file ends (the layout of INTEGRATION.md, restated)"""
    ends, at = [], 0
    for size in (8, 4, 4):   # magic, version, map count
        at += size
        ends.append(at)
    for m in maps:
        n = len(m["src_idx"])
        for size in (4 + len(m["name"].encode()), 4 + len(m["class_name"].encode()), 7 * 4, 4, 8, 8, 4 * n, 4 * n, 4 * n, 4 * n):
            at += size
            ends.append(at)
    ends.append(at + 8)   # checksum
    return ends


def _fnv1a(b):
    h = 0xcbf29ce484222325
    for c in b:
        h = ((h ^ c) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_map_file_round_trip_two_maps_one_empty(host, tmp_path):
    path = str(tmp_path / "maps.mhmap")
    maps = _maps()
    host.write_local_map_file(path, maps)
    back = host.read_local_map_file(path)
    assert len(back) == 2
    for g, r in zip(back, maps):
        _same_map(g, r)
    # the layout, independently of the writer: sizes, little-endian fields, FNV-1a over everything before the checksum
    raw = open(path, "rb").read()
    assert len(raw) == _sections(maps)[-1]
    assert raw[:8] == b"MHLOCMAP" and struct.unpack_from("<II", raw, 8) == (host.LOCAL_MAP_FILE_VERSION, 2) and host.LOCAL_MAP_FILE_VERSION == 1
    assert struct.unpack_from("<I", raw, 16)[0] == 8 and raw[20:28] == b"localmap" and raw[32:35] == b"NDT"
    vs, cap, mode, md, ratio, minpts, metric, far = struct.unpack_from("<fIIffIIf", raw, 35)
    assert (vs, cap, mode, minpts, metric, far) == (1.5, 20, 0, 4, 1, 80.0) and np.float32(md) == np.float32(0.05)
    assert struct.unpack_from("<QQ", raw, 67) == (1234, 98765432109)
    assert raw[83:83 + 4 * 1234] == np.ascontiguousarray(maps[0]["xyz"][:, 0]).tobytes()
    assert struct.unpack_from("<Q", raw, len(raw) - 8)[0] == _fnv1a(raw[:-8])
    # writing the same maps again gives the same bytes
    host.write_local_map_file(path + "2", back)
    assert open(path + "2", "rb").read() == raw


def test_map_file_reader_refuses_every_damaged_file(host, tmp_path):
    path = str(tmp_path / "maps.mhmap")
    maps = _maps()
    host.write_local_map_file(path, maps)
    raw = open(path, "rb").read()
    bad = str(tmp_path / "damaged.mhmap")

    def refused(data, reason):
        open(bad, "wb").write(data)
        with pytest.raises(RuntimeError) as e:
            host.read_local_map_file(bad)
        assert "damaged.mhmap" in str(e.value) and re.search(reason, str(e.value)), str(e.value)

    ends = _sections(maps)
    assert ends[-1] == len(raw)
    for cut in sorted(set([0, 1] + ends[:-1] + [len(raw) - 1])):   # truncated at every section boundary
        refused(raw[:cut], "truncated|magic" if cut >= 8 else "magic")
    for at in (9, 17, 40, 70, 100, 83 + 4 * 1234 * 3 + 5, len(raw) - 20, len(raw) - 3):   # one flipped byte, anywhere behind the magic
        flipped = bytearray(raw)
        flipped[at] ^= 0x40
        refused(bytes(flipped), "checksum|truncated|trailing|version|class")
    for at in (0, 7):
        flipped = bytearray(raw)
        flipped[at] ^= 0x01
        refused(bytes(flipped), "magic")
    newer = bytearray(raw)
    newer[8:12] = struct.pack("<I", host.LOCAL_MAP_FILE_VERSION + 1)
    newer[-8:] = struct.pack("<Q", _fnv1a(bytes(newer[:-8])))   # (a well-formed file of a later format)
    refused(bytes(newer), "newer")
    refused(raw + b"\0", "trailing")
    refused(raw[:-8] + b"\0" + raw[-8:], "trailing|checksum")
    # a class the loader cannot build: refused by the reader (a well-formed file otherwise) and by the writer
    other = bytearray(raw)
    other[32:35] = b"XYZ"
    other[-8:] = struct.pack("<Q", _fnv1a(bytes(other[:-8])))
    refused(bytes(other), "XYZ.*cannot build")
    with pytest.raises(RuntimeError, match="CVoxelMap"):
        host.write_local_map_file(bad, [dict(maps[1], class_name="CVoxelMap")])
    with pytest.raises(RuntimeError, match="no_such_file"):
        host.read_local_map_file(str(tmp_path / "no_such_file"))
    # the undamaged file still reads
    assert len(host.read_local_map_file(path)) == 2


# ---- the candidate grid -----------------------------------------------------------------------------------------------------------
def _cov(sx, sy, syaw):
    c = np.zeros((6, 6))
    c[0, 0], c[1, 1], c[3, 3] = sx * sx, sy * sy, syaw * syaw
    c[0, 1] = c[1, 0] = 0.3 * sx * sy   # (off-diagonal entries are not read)
    c[2, 2], c[4, 4], c[5, 5] = 4.0, 0.1, 0.1   # (nor are z, pitch, roll)
    return c.reshape(36)


@pytest.mark.parametrize("sig,steps,sigmas", [((1.0, 1.0, np.deg2rad(4.0)), (0.5, np.deg2rad(3.0)), 3.0),
                                               ((0.7, 0.0, np.deg2rad(10.0)), (0.3, np.deg2rad(2.5)), 2.0),
                                               ((0.0, 0.0, 0.0), (0.5, 0.1), 3.0)])
def test_relocalization_grid_matches_the_numpy_restatement(host, sig, steps, sigmas):
    w = synth.workload_small()
    mean = w.pose_gt_ypr + sr.MEAN_OFFSET
    poses, rows = host.relocalization_grid(list(mean), list(_cov(*sig)), steps[0], steps[1], sigmas, 65536)
    ref_poses, ref_rows = sr.relocalization_grid(mean, _cov(*sig), steps[0], steps[1], sigmas)
    assert poses.shape == ref_poses.shape and rows.shape == ref_rows.shape
    if sig[0] == 1.0:
        assert len(rows) == 13 * 13 * 9
    if sig == (0.0, 0.0, 0.0):
        assert len(rows) == 1 and np.array_equal(rows[0], mean)
    assert rows.tobytes() == ref_rows.tobytes()       # counts, order and every field, to the last bit
    assert poses.tobytes() == ref_poses.tobytes()     # ... and the matrices are synth.pose_from_ypr's


def test_relocalization_grid_refuses_more_than_max_candidates(host):
    mean, cov = [0.0] * 6, list(_cov(1.0, 1.0, np.deg2rad(4.0)))
    assert len(host.relocalization_grid(mean, cov, 0.5, np.deg2rad(3.0), 3.0, 1521)[0]) == 1521
    with pytest.raises(RuntimeError, match="13 x 13 x 9.*max_candidates.*coarsen"):
        host.relocalization_grid(mean, cov, 0.5, np.deg2rad(3.0), 3.0, 1520)
    with pytest.raises(RuntimeError, match="max_candidates"):
        host.relocalization_grid(mean, list(_cov(1e6, 1e6, 1.0)), 1e-3, 1e-3, 3.0, 65536)
    for bad in ((0.0, 0.1), (0.5, 0.0), (np.nan, 0.1), (0.5, -1.0)):
        with pytest.raises(RuntimeError):
            host.relocalization_grid(mean, cov, bad[0], bad[1], 3.0, 65536)
    with pytest.raises(RuntimeError):
        host.relocalization_grid(mean, list(-np.asarray(cov)), 0.5, 0.1, 3.0, 65536)


# ---- the pipelines ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", PIPES, ids=["default", "ndt"])
def test_hip_pipelines_load_with_the_new_keys(host, pipe, monkeypatch):
    for v in ("MOLA_LOAD_MM", "MOLA_INITIAL_LOCALIZATION_ENABLED", "MOLA_INITIAL_X", "MOLA_INITIAL_YAW"):
        monkeypatch.delenv(v, raising=False)
    txt = open(pipe).read()
    assert 'load_existing_local_map: ${MOLA_LOAD_MM|""}' in txt and "initial_localization:" in txt and "relocalization:" in txt
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlFile(pipe))   # (no device needed: nothing to load)
    assert lo.loadExistingLocalMap() == ""
    il = lo.initialLocalization()
    assert (il["enabled"], il["method"], il["relocalize"]) == (False, "InitLocalization::FixedPose", False)
    ro = lo.relocalizationOptions()
    assert (ro["score_threshold"], ro["step_xy"], ro["step_yaw_deg"], ro["sigmas"], ro["refine_top_k"], ro["max_candidates"]) == \
        ("", 0.0, 3.0, 3.0, 4, 65536)
    # the keys follow the environment, as in the reference
    monkeypatch.setenv("MOLA_INITIAL_LOCALIZATION_ENABLED", "true")
    monkeypatch.setenv("MOLA_INITIAL_X", "12.5")
    monkeypatch.setenv("MOLA_INITIAL_YAW", "0.25")
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlFile(pipe))
    il = lo.initialLocalization()
    assert il["enabled"] and il["fixed_initial_pose"] == [12.5, 0.0, 0.0, 0.25, 0.0, 0.0]


def test_initial_localization_method_other_than_fixed_pose_is_refused(host, tmp_path):
    txt = open(PIPES[0]).read()
    assert "method: 'InitLocalization::FixedPose'" in txt
    p = tmp_path / "gnss.yaml"
    p.write_text(txt.replace("method: 'InitLocalization::FixedPose'", "method: 'InitLocalization::FromStateEstimator'"))
    with pytest.raises(RuntimeError, match="FromStateEstimator.*FixedPose"):
        host.LidarOdometry().initialize(host.Config.FromYamlFile(str(p)))
    # relocalize_sigmas: three values, and the request is announced in the options
    p2 = tmp_path / "reloc.yaml"
    p2.write_text(txt.replace("relocalize_sigmas: []", "relocalize_sigmas: [1.0, 0.5, 4.0]"))
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlFile(str(p2)))
    assert lo.initialLocalization()["relocalize"] and lo.initialLocalization()["relocalize_sigmas"] == [1.0, 0.5, 4.0]
    p3 = tmp_path / "reloc2.yaml"
    p3.write_text(txt.replace("relocalize_sigmas: []", "relocalize_sigmas: [1.0, 0.5]"))
    with pytest.raises(RuntimeError, match="relocalize_sigmas"):
        host.LidarOdometry().initialize(host.Config.FromYamlFile(str(p3)))


def test_a_map_file_with_other_names_is_refused_at_initialize(host, tmp_path, monkeypatch):
    path = str(tmp_path / "other.mhmap")
    host.write_local_map_file(path, [dict(_maps()[0], name="some_other_layer", class_name="HashedVoxelPointCloud")])
    monkeypatch.setenv("MOLA_LOAD_MM", path)
    with pytest.raises(RuntimeError, match="some_other_layer.*localmap.*names must match"):
        host.LidarOdometry().initialize(host.Config.FromYamlFile(PIPES[0]))
    monkeypatch.setenv("MOLA_LOAD_MM", str(tmp_path / "missing.mhmap"))
    with pytest.raises(RuntimeError, match="missing.mhmap"):
        host.LidarOdometry().initialize(host.Config.FromYamlFile(PIPES[0]))
