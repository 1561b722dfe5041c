"""Key-frames of a session on the device driver (mola_hip::LidarOdometry, params.simplemap) and the session map built from them:
the decisions against tests/simplemap_ref.py; the pinning identity -- the session map built from exactly the key-frames the
local map merged IS the local map, bit for bit, on the default chain and on the dual-map chain; a session map serves scans
the sliding local map has long dropped; recording does not perturb the odometry."""
import os
import re

import numpy as np
import pytest

import simplemap_ref
import test_odometry_chains as chains
from mola_lidar_odometry_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPE = os.path.join(ROOT, "pipelines", "lidar3d-default-hip.yaml")
ENV = ("MOLA_LOAD_MM", "MOLA_MAPPING_ENABLED", "MOLA_INITIAL_LOCALIZATION_ENABLED", "MOLA_GENERATE_SIMPLEMAP", "MOLA_LOAD_SM",
       "MOLA_SIMPLEMAP_OUTPUT", "MOLA_SIMPLEMAP_MIN_XYZ", "MOLA_SIMPLEMAP_MIN_ROT", "MOLA_SIMPLEMAP_GENERATE_LAZY_LOAD",
       "MOLA_SIMPLEMAP_ALSO_NON_KEYFRAMES", "MOLA_LOCAL_MAP_MAX_SIZE", "MOLA_LOCALMAP_MAX_POINTS_PER_VOXEL")
KEYS = ("dropped", "first_scan", "icp_run", "icp_good", "had_motion_model", "map_updated", "restarted", "icp_iterations",
        "twist_corrections", "align_calls", "termination", "n_raw", "n_for_map", "n_for_icp", "n_map_points", "n_map_voxels",
        "goodness", "sigma", "pose", "init_guess", "twist")


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


@pytest.fixture(scope="module")
def drive():
    return synth.make_drive(10)


@pytest.fixture(scope="module")
def long_drive():
    """44 thin sweeps: the vehicle ends more than 30 m from where it started"""
    return synth.make_drive(44, rings=16, azimuths=300)


def _env(monkeypatch, **kw):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv(k, v)


def _run(host, drive, text=None, n=None):
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlText(text) if text is not None else host.Config.FromYamlFile(PIPE))
    for (xyz, t), st in list(zip(drive["scans"], drive["stamps"]))[:n]:
        lo.onLidar(st, xyz, t)
    return lo


def _same_dump(a, b):
    for k in ("xyz", "src_idx"):
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def _same_frames(a, b):
    assert a["maps"] == b["maps"] and len(a["frames"]) == len(b["frames"])
    for f, g in zip(a["frames"], b["frames"]):
        assert f["timestamp"] == g["timestamp"] and f["pose"] == g["pose"] and f["cov"] == g["cov"] and f["twist"] == g["twist"]
        assert (f["layers"] is None) == (g["layers"] is None)
        if f["layers"] is not None:
            assert len(f["layers"]) == len(g["layers"])
            for (i, x), (j, y) in zip(f["layers"], g["layers"]):
                assert i == j and x.tobytes() == y.tobytes()


def test_decisions_with_the_reference_formulas(host, drive, monkeypatch, tmp_path):
    """(a) simplemap_* of the records = the restated rule on those records; stored poses = the records'; the file written at
    the end reads back as keyFrames()"""
    out = str(tmp_path / "final.mhkf")
    _env(monkeypatch, MOLA_GENERATE_SIMPLEMAP="true", MOLA_SIMPLEMAP_ALSO_NON_KEYFRAMES="true", MOLA_SIMPLEMAP_OUTPUT=out)
    lo = _run(host, drive)
    recs = [r for r in lo.records() if not r["dropped"]]
    assert len(recs) == 10 and recs[0]["first_scan"]
    w = np.array([np.linalg.norm(r["twist"][3:]) for r in recs])
    rng = np.array([r["estimated_sensor_max_range"] for r in recs])
    lim_t, lim_r = (1.0e-2 + w * 1.0) * rng, 15 + w * 500    # the formulas of the pipeline file, on the variables the records show
    stored, keyframe = simplemap_ref.decide([r["pose"] for r in recs], [r["icp_good"] for r in recs], lim_t, lim_r,
                                            add_non_keyframes_too=True, first_scan=[r["first_scan"] for r in recs])
    assert [r["simplemap_frame"] for r in recs] == list(stored) and [r["simplemap_keyframe"] for r in recs] == list(keyframe)
    assert 2 <= keyframe.sum() < stored.sum()          # key-frames at their own spacing, the scans between them without points
    kf = lo.keyFrames()
    assert [m["name"] for m in kf["maps"]] == ["localmap"] and kf["maps"][0]["class_name"] == "HashedVoxelPointCloud"
    kept = [r for r in recs if r["simplemap_frame"]]
    assert len(kf["frames"]) == len(kept)
    for f, r in zip(kf["frames"], kept):
        assert f["pose"] == r["pose"] and f["timestamp"] == r["timestamp"] and (f["layers"] is not None) == r["simplemap_keyframe"]
        if r["simplemap_keyframe"]:
            assert len(f["layers"]) == 1 and f["layers"][0][0] == 0 and len(f["layers"][0][1]) == r["n_for_map"] > 100
        assert (f["cov"] == [0.0] * 36) == r["first_scan"]
    del lo                                             # written at destruction
    _same_frames(host.read_keyframe_file(out), kf)


def _pinned(host, drive, text, names, merges_per_frame):
    lo = _run(host, drive, text)
    recs = [r for r in lo.records() if not r["dropped"]]
    kf = lo.keyFrames()
    kept = [r for r in recs if r["simplemap_frame"]]
    assert len(kf["frames"]) == len(kept) and all(r["simplemap_keyframe"] for r in kept)   # limits 0 m / 0 deg: every good scan
    assert [r["simplemap_frame"] for r in recs] == [r["first_scan"] or r["icp_good"] for r in recs]
    merged = [f for f, r in zip(kf["frames"], kept) if r["map_updated"]]
    assert len(merged) >= 3 and len(merged) < len(kept), (len(merged), len(kept))
    assert all(len(f["layers"]) == merges_per_frame for f in merged)
    for passes in (0, 1000):
        maps = host.build_session_maps(dict(maps=kf["maps"], frames=merged), passes)
        assert [m["name"] for m in maps] == names
        for m in maps:
            _same_dump(m, lo.downloadMap(m["name"]))
            assert m["n_offered"] >= len(m["src_idx"]) > 500
    return lo, kf


def test_session_map_of_the_merged_keyframes_is_the_local_map(host, drive, monkeypatch, tmp_path):
    """(b) the pinning identity on the default chain"""
    _env(monkeypatch, MOLA_GENERATE_SIMPLEMAP="true", MOLA_SIMPLEMAP_OUTPUT=str(tmp_path / "kf.mhkf"), MOLA_SIMPLEMAP_MIN_XYZ="0", MOLA_SIMPLEMAP_MIN_ROT="0", MOLA_LOCAL_MAP_MAX_SIZE="0")
    _pinned(host, drive, None, ["localmap"], 1)


def test_session_maps_of_the_dual_map_chain(host, drive, monkeypatch, tmp_path):
    """(c) the same with two FilterMerge steps into two maps"""
    _env(monkeypatch, MOLA_GENERATE_SIMPLEMAP="true", MOLA_SIMPLEMAP_OUTPUT=str(tmp_path / "kf.mhkf"), MOLA_SIMPLEMAP_MIN_XYZ="0", MOLA_SIMPLEMAP_MIN_ROT="0", MOLA_LOCAL_MAP_MAX_SIZE="0")
    text = re.sub(r"remove_voxels_farther_than: .*", "remove_voxels_farther_than: 0", chains.inline_pipeline(chains.DUAL_TAIL, chains.DUAL_MATCHES))
    lo, kf = _pinned(host, drive, text, ["localmap", "localmap_far"], 2)
    assert [[i for i, _ in f["layers"]] for f in kf["frames"]] == [[0, 1]] * len(kf["frames"])   # step order


def _near(xyz, centre, radius=5.0):
    return int((np.linalg.norm(xyz - np.asarray(centre, np.float32), axis=1) < radius).sum())


def test_session_map_serves_where_the_local_map_has_moved_on(host, long_drive, monkeypatch, tmp_path):
    """(d) a run whose local map removes everything farther than 20 m; its session map still holds the start of the drive, and the
    first scans register in it"""
    _env(monkeypatch, MOLA_GENERATE_SIMPLEMAP="true", MOLA_LOCAL_MAP_MAX_SIZE="20", MOLA_SIMPLEMAP_OUTPUT=str(tmp_path / "kf.mhkf"))
    lo = _run(host, long_drive)
    recs = lo.records()
    end = np.array(recs[-1]["pose"]).reshape(3, 4)[:, 3]
    assert np.abs(end).max() > 27.0 and sum(r["simplemap_keyframe"] for r in recs) >= 3
    session_file, local_file = str(tmp_path / "session.mhmap"), str(tmp_path / "local.mhmap")
    session = host.build_session_maps(lo.keyFrames(), 0, session_file)
    lo.saveLocalMaps(local_file)
    local = host.read_local_map_file(local_file)
    assert [m["name"] for m in session] == ["localmap"] and session[0]["remove_voxels_farther_than"] == 20.0
    start = np.array(recs[0]["pose"]).reshape(3, 4)[:, 3]
    print("points within 5 m of the first pose: session map", _near(session[0]["xyz"], start), "local map", _near(local[0]["xyz"], start))
    assert _near(session[0]["xyz"], start) > 100 and _near(local[0]["xyz"], start) == 0
    assert _near(session[0]["xyz"], end) > 100 and _near(local[0]["xyz"], end) > 100
    back = host.read_local_map_file(session_file)
    assert back[0]["xyz"].tobytes() == session[0]["xyz"].tobytes() and back[0]["src_idx"].tobytes() == session[0]["src_idx"].tobytes()
    # localization only, in the session map, from the start of the drive
    _env(monkeypatch, MOLA_LOAD_MM=session_file, MOLA_MAPPING_ENABLED="false")
    loc = _run(host, long_drive, n=4)
    for r, m in zip(loc.records(), recs):
        assert r["icp_run"] and r["icp_good"] and not r["map_updated"] and not r["first_scan"]
        print("scan at", r["timestamp"], "localized", np.abs(np.array(r["pose"]) - np.array(m["pose"])).max(), "from the mapping run's pose")
    _same_dump(loc.downloadMap("localmap"), session[0])


def test_recording_does_not_perturb_the_odometry(host, drive, monkeypatch, tmp_path):
    """(e) generate: false stores nothing; with generate: true every record, the trajectory and the local map are the same"""
    _env(monkeypatch)
    off = _run(host, drive)
    assert off.keyFrames() == dict(maps=[], frames=[]) and not any(r["simplemap_frame"] or r["simplemap_keyframe"] for r in off.records())
    _env(monkeypatch, MOLA_GENERATE_SIMPLEMAP="true", MOLA_SIMPLEMAP_OUTPUT=str(tmp_path / "kf.mhkf"))
    on = _run(host, drive)
    assert len(on.keyFrames()["frames"]) >= 2
    for a, b in zip(off.records(), on.records()):
        for k in KEYS:
            assert a[k] == b[k], k
    assert off.trajectory() == on.trajectory()
    _same_dump(off.downloadMap("localmap"), on.downloadMap("localmap"))


def test_a_loaded_keyframe_file_is_continued_only_by_a_plan_with_its_map_parameters(host, drive, monkeypatch, tmp_path):
    """load_existing_simple_map: the store starts with the file's frames and appends under the file's header; a pipeline whose map
    has another cap is refused by the scan that makes the map, since build_session_maps would build with the file's"""
    kf_file = str(tmp_path / "first.mhkf")
    every = dict(MOLA_GENERATE_SIMPLEMAP="true", MOLA_SIMPLEMAP_OUTPUT="", MOLA_SIMPLEMAP_MIN_XYZ="0", MOLA_SIMPLEMAP_MIN_ROT="0")
    _env(monkeypatch, **every)
    first = _run(host, drive, n=4)
    first.saveKeyFrames(kf_file)
    kf1 = first.keyFrames()
    _env(monkeypatch, MOLA_LOAD_SM=kf_file, **every)
    kf2 = _run(host, drive, n=4).keyFrames()
    n1 = len(kf1["frames"])
    assert n1 >= 2 and len(kf2["frames"]) == 2 * n1 and kf2["maps"] == kf1["maps"]
    _same_frames(dict(maps=kf2["maps"], frames=kf2["frames"][:n1]), kf1)
    _same_frames(dict(maps=kf2["maps"], frames=kf2["frames"][n1:]), kf1)      # the same drive again: the same frames again
    _env(monkeypatch, MOLA_LOAD_SM=kf_file, MOLA_LOCALMAP_MAX_POINTS_PER_VOXEL="10", **every)
    with pytest.raises(RuntimeError, match="load_existing_simple_map.*cap 20.*cap 10"):
        _run(host, drive, n=1)


def test_cli_records_every_sequence_into_a_file_of_its_own(host, monkeypatch, tmp_path):
    """molahip-lo-cli with two --seq-dir, --output-simplemap and --output-session-map and NO --save-local-map: FILE_<k> per
    sequence, none shared.  The two sequences run with prefetch on and their alignments in one AlignBatcher; their key-frame
    files are, byte for byte, those of each sequence alone with --no-prefetch, and each session map is what build_session_maps
    makes of its key-frame file."""
    import subprocess
    _env(monkeypatch)
    cli = os.path.join(ROOT, "mola_lidar_odometry_amd", "molahip-lo-cli")
    dirs = [synth.write_kitti_sequence(str(tmp_path / ("s%d" % k)), synth.make_drive(n, seed=s, speed=v))
            for k, (n, s, v) in enumerate(((8, 4242, 8.0), (7, 777, 5.0)))]
    kf, sm = str(tmp_path / "multi.mhkf"), str(tmp_path / "multi.mhmap")
    cmd = [cli, "--pipeline", PIPE, "--out", str(tmp_path / "multi.tum"), "--output-simplemap", kf, "--output-session-map", sm]
    for d in dirs:
        cmd += ["--seq-dir", d]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(kf) and not os.path.exists(sm)
    recorded = []
    for k, d in enumerate(dirs):
        solo = str(tmp_path / ("solo%d.mhkf" % k))
        r = subprocess.run([cli, "--pipeline", PIPE, "--seq-dir", d, "--out", str(tmp_path / ("solo%d.tum" % k)), "--no-prefetch",
                            "--output-simplemap", solo], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        recorded.append(open("%s_%d" % (kf, k), "rb").read())
        assert recorded[k] == open(solo, "rb").read(), "sequence %d: recorded differently beside another sequence and under prefetch" % k
        assert sum(f["layers"] is not None for f in host.read_keyframe_file(solo)["frames"]) >= 2
        lib = str(tmp_path / ("lib%d.mhmap" % k))
        host.build_session_maps(solo, 0, lib)
        assert open("%s_%d" % (sm, k), "rb").read() == open(lib, "rb").read()
    assert recorded[0] != recorded[1]


def test_cli_builds_the_session_map_from_a_keyframe_file(host, drive, monkeypatch, tmp_path):
    """molahip-lo-cli --build-session-map KEYFRAMES --save-local-map FILE: no sequence, the file build_session_maps gives"""
    import json
    import subprocess
    kf_file, cli_file, lib_file = (str(tmp_path / n) for n in ("drive.mhkf", "cli.mhmap", "lib.mhmap"))
    _env(monkeypatch, MOLA_GENERATE_SIMPLEMAP="true", MOLA_SIMPLEMAP_OUTPUT=str(tmp_path / "unused.mhkf"))
    lo = _run(host, drive)
    lo.saveKeyFrames(kf_file)
    host.build_session_maps(kf_file, 0, lib_file)
    cli = os.path.join(ROOT, "mola_lidar_odometry_amd", "molahip-lo-cli")
    r = subprocess.run([cli, "--build-session-map", kf_file, "--save-local-map", cli_file], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert rep["frames"] == len(lo.keyFrames()["frames"]) and rep["maps"][0]["name"] == "localmap" and rep["maps"][0]["points"] > 500
    assert open(cli_file, "rb").read() == open(lib_file, "rb").read()
    r = subprocess.run([cli, "--build-session-map", kf_file], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--save-local-map" in r.stderr
