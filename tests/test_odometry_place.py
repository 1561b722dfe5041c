"""relocalizeInKeyFrames on the device driver (mola_hip::LidarOdometry) against tests/place_localize_ref.py, the restatement on
the CPU oracle driver.  Twelve key-frames along the street of tests/place_cases.py are written as a key-frame file, their session
map as a map file; fresh drivers load both with mapping off, get the request and are fed sweeps taken beside three of the
key-frames under an arbitrary yaw: the place search equals tests/place_ref.py entry by entry, the rest of the record equals the
reference (the keys and the 1e-6 pose bar of test_odometry_localize.py), and the pose is the ground truth's within that test's
0.1 m.  tests/test_place_cpu.py shows on the CPU that the reference alone ranks the true frames first and meets the bound.

Measured (reference on the CPU = device within 1e-6): errors 0.048, 0.093 and 0.032 m; qualities 0.999, 0.995, 0.974; a query 95 m
beyond the last key-frame reaches 0.73 at a wrong place of the self-similar street and is refused at the 0.9 every run here asks."""
import os
import subprocess

import numpy as np
import pytest

import place_cases as pc
import place_localize_ref as plr
import test_odometry_localize as tl
from mola_lidar_odometry_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPE = os.path.join(ROOT, "pipelines", "lidar3d-default-hip.yaml")
CLI = os.path.join(ROOT, "mola_lidar_odometry_amd", "molahip-lo-cli")
ENV = tl.ENV + ("MOLA_LOAD_SM", "MOLA_GENERATE_SIMPLEMAP", "MOLA_SIMPLEMAP_OUTPUT", "MOLA_MINIMUM_ICP_QUALITY")


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


def _env(mp, **kw):
    for v in ENV:
        mp.delenv(v, raising=False)
    for k, v in kw.items():
        mp.setenv(k, v)


@pytest.fixture(scope="module")
def session(host, oracle, tmp_path_factory):
    """the key-frame file and the session map file, made on the device: every key-frame sweep is the first scan of a recording
    driver, whose stored frame (the layer its FilterMerge step merges) gets the pose the sweep was taken at"""
    d = tmp_path_factory.mktemp("place")
    sc = pc.scene()
    frames, maps = [], None
    with pytest.MonkeyPatch.context() as mp:
        _env(mp, MOLA_GENERATE_SIMPLEMAP="true")
        for k, (xyz, t) in enumerate(pc.kf_sweeps(sc)):
            lo = host.LidarOdometry()
            lo.initialize(host.Config.FromYamlFile(PIPE))
            assert lo.onLidar(1000.0 + k, xyz, t)["simplemap_keyframe"]
            kf = lo.keyFrames()
            maps = maps or kf["maps"]
            f = dict(kf["frames"][0])
            f["pose"] = [float(v) for v in synth.pose_from_ypr(pc.kf_pose(k))]
            frames.append(f)
    kf_file, map_file, text_file = str(d / "session.mhkf"), str(d / "session.mhmap"), str(d / "pipeline.yaml")
    host.write_keyframe_file(kf_file, dict(maps=maps, frames=frames))
    host.build_session_maps(kf_file, 0, map_file)
    text = pc.pipeline_text(PIPE)
    open(text_file, "w").write(text)
    queries = pc.query_sweeps(sc) + [pc.sweep(sc, np.array(pc.FAR_QUERY), 300)]
    return dict(kf_file=kf_file, map_file=map_file, text=text, text_file=text_file, queries=queries, dir=d)


def _load_env(mp, s):
    _env(mp, MOLA_LOAD_MM=s["map_file"], MOLA_LOAD_SM=s["kf_file"], MOLA_MAPPING_ENABLED="false", MOLA_MINIMUM_ICP_QUALITY=pc.MIN_QUALITY)


def _pair(host, s):
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlText(s["text"]))
    o = plr.PlaceOracle(None, text=s["text"])
    o.preload(host.read_local_map_file(s["map_file"])[0])
    o.set_keyframes(host.read_keyframe_file(s["kf_file"])["frames"])
    lo.relocalizeInKeyFrames()
    o.relocalize_in_keyframes()
    assert lo.relocalizationPending()
    return lo, o


def _place_compare(a, b):
    assert a["place_tried"] and b["place_tried"]
    for key in ("place_frames", "place_shifts", "place_dists"):
        assert list(a[key]) == list(b[key]), (key, a[key], b[key])
    tl._reloc_compare(a, b)


def test_the_session_holds_what_the_reference_makes_on_the_cpu(host, session):
    """the device-made key-frame layers are the CPU reference's, so tests/test_place_cpu.py's verdicts are about this session"""
    frames, rec = plr.cpu_session(PIPE, pc.scene())
    got = host.read_keyframe_file(session["kf_file"])["frames"]
    assert len(got) == len(frames) == 12
    for f, g in zip(frames, got):
        assert f["pose"] == g["pose"] and np.asarray(f["layers"][0][1], np.float32).tobytes() == g["layers"][0][1].tobytes()
    # the driver's PlaceIndex over the file ranks a key-frame's own layer first, at shift 0 and distance 0
    ix = host.PlaceIndex()
    assert ix.add_keyframes(session["kf_file"]) == 12 and ix.size() == 12
    assert ix.query(got[4]["layers"][0][1])[0] == (4, 0, 0)
    import place_ref as pr
    assert np.array_equal(host.place_describe(got[4]["layers"][0][1]), pr.describe(got[4]["layers"][0][1], **pr.DEFAULT))


@pytest.mark.parametrize("q", range(len(pc.QUERIES)))
def test_a_sweep_beside_a_keyframe_is_found_without_a_prior_pose(host, session, monkeypatch, q):
    _load_env(monkeypatch, session)
    lo, o = _pair(host, session)
    xyz, t = session["queries"][q]
    a, b = lo.onLidar(2000.0, xyz, t), o.on_lidar(2000.0, xyz, t)
    _place_compare(a, b)
    k, yaw, _ = pc.QUERIES[q]
    assert a["place_frames"][0] == k and len(a["place_frames"]) == 2   # place_top_k of the scenario
    worst = tl._compare(q, a, b)
    assert worst < 1e-6, worst
    assert a["relocalized"] and not lo.relocalizationPending() and a["had_motion_model"] and a["icp_good"]
    err = float(np.abs(np.array(a["pose"])[[3, 7, 11]] - pc.query_pose(q)[:3]).max())
    print("query", q, "frames", a["place_frames"], "shifts", a["place_shifts"], "dists", a["place_dists"], "candidates", a["reloc_candidates"],
          "quality", a["reloc_best_quality"], "|pose - reference|", worst, "error against the ground truth [m]", err)
    assert err < pc.GT_BOUND
    # the next scan is an ordinary one
    a2, b2 = lo.onLidar(2000.1, xyz, t), o.on_lidar(2000.1, xyz, t)
    assert not a2["place_tried"] and not a2["relocalization_tried"] and tl._compare(q, a2, b2) < 1e-6


def test_a_place_far_from_every_keyframe_leaves_the_request_pending(host, session, monkeypatch):
    _load_env(monkeypatch, session)
    lo, o = _pair(host, session)
    xyz, t = session["queries"][-1]
    a, b = lo.onLidar(2000.0, xyz, t), o.on_lidar(2000.0, xyz, t)
    _place_compare(a, b)
    assert not a["relocalized"] and lo.relocalizationPending() and o.request is not None
    assert tl._compare(-1, a, b) < 1e-6   # the scan proceeds as it would have


def test_a_store_without_frames_names_the_keyframe_file(host, session, monkeypatch):
    _load_env(monkeypatch, session)
    monkeypatch.delenv("MOLA_LOAD_SM")
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlText(session["text"]))
    lo.relocalizeInKeyFrames()
    with pytest.raises(RuntimeError, match="load_existing_simple_map"):
        lo.onLidar(2000.0, *session["queries"][0])


def test_the_request_is_refused_with_an_align_batcher(host, session, monkeypatch):
    _load_env(monkeypatch, session)
    batched = host.LidarOdometry(device=0, own_context=True)   # (a batch member has a device context of its own)
    batched.initialize(host.Config.FromYamlText(session["text"]))
    batcher = host.AlignBatcher(1)
    batched.setAlignBatcher(batcher)
    with pytest.raises(RuntimeError, match="relocalizeInKeyFrames.*AlignBatcher"):
        batched.relocalizeInKeyFrames()
    assert not batched.relocalizationPending()
    batcher.leave()


def test_the_command_line_gives_the_first_pose_of_the_api_route(host, session, monkeypatch, tmp_path):
    _load_env(monkeypatch, session)
    xyz, t = session["queries"][0]
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlText(session["text"]))
    lo.relocalizeInKeyFrames()
    # (the sequence's files hold x, y, z, intensity: no per-point time stamps, and times.txt starts at 0)
    seq = synth.write_kitti_sequence(str(tmp_path), dict(scans=[(xyz, t)], stamps=np.array([0.0])))
    stamp = float(open(os.path.join(seq, "times.txt")).read().split()[0])
    a = lo.onLidar(stamp, xyz, None)
    assert a["relocalized"]
    out = str(tmp_path / "cli.tum")
    r = subprocess.run([CLI, "--pipeline", session["text_file"], "--seq-dir", seq, "--out", out, "--relocalize-in-keyframes", "--no-prefetch"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    row = [float(v) for v in open(out).read().split("\n")[0].split()]
    assert np.abs(np.array(row[1:4]) - np.array(a["pose"])[[3, 7, 11]]).max() < 1e-6, (row, a["pose"])
    # two sequences on one device share an AlignBatcher: refused
    r = subprocess.run([CLI, "--pipeline", session["text_file"], "--seq-dir", seq, "--seq-dir", seq, "--out", out, "--relocalize-in-keyframes"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "one sequence per device" in r.stderr
