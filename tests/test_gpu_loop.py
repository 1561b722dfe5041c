"""Loop closure on the device (mola_hip::close_loops) against tests/loop_ref.py, the restatement on the CPU oracle, on the scenario
of tests/loop_cases.py: 66 key-frames around one block and 36 m into it again, recorded with 3.29 m of drift.  The tried pairs, the
candidate counts, the kept ranks, the decisions and the iteration counts are the reference's; the edges are its edges within the
1e-6 tests/test_odometry_localize.py holds relocalized poses to; the optimised poses within 1e-5 (ten times the edge bound: the
graph is a chain, an edge's perturbation reaches every node with a gain of order one); and the ground-truth bounds
tests/test_loop_cpu.py holds the reference to hold for the device's result.  Then: a drive without a revisit, a threshold nothing
reaches, the relocalization's shared score -> rank -> refine step on its own, the command line.

Measured on an MI355X: the four pairs (56, 1), (59, 2), (62, 5), (65, 8) at quality 0.9881-0.9941, |Z - reference| 3e-17, optimised
poses 7e-12 m / 8e-14 rad from the reference's, end error 3.29 m -> 0.23 m, maximum 4.13 m -> 0.78 m; profiles/loop_closure.md."""
import json
import os
import subprocess

import numpy as np
import pytest

import loop_cases as lc
import loop_ref as lr
import place_cases as pc
import test_loop_cpu as tc
import test_odometry_localize as tl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPE = os.path.join(ROOT, "pipelines", "lidar3d-default-hip.yaml")
CLI = os.path.join(ROOT, "mola_lidar_odometry_amd", "molahip-lo-cli")
ENV = tl.ENV + ("MOLA_LOAD_SM", "MOLA_GENERATE_SIMPLEMAP", "MOLA_SIMPLEMAP_OUTPUT", "MOLA_MINIMUM_ICP_QUALITY")
REJECT = "  min_quality: 0.999\n"   # the reference's best pair reaches 0.9941


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


@pytest.fixture(scope="module")
def session(host, tmp_path_factory):
    """the scenario as a key-frame set and file, and the pipeline text with the scenario's options"""
    d = tmp_path_factory.mktemp("loop")
    s = lc.scenario()
    kf = lc.keyframe_set(s["est"], s["sweeps"])
    text = open(PIPE).read() + lc.OPTIONS
    kf_file, text_file = str(d / "drive.mhkf"), str(d / "pipeline.yaml")
    host.write_keyframe_file(kf_file, kf)
    open(text_file, "w").write(text)
    return dict(dir=d, kf=kf, kf_file=kf_file, text=text, text_file=text_file, gt=s["gt"], est=s["est"])


@pytest.fixture(scope="module")
def closed(host, session):
    with pytest.MonkeyPatch.context() as mp:
        for v in ENV:
            mp.delenv(v, raising=False)
        corrected, report = host.close_loops(session["kf"], host.Config.FromYamlText(session["text"]))
    return corrected, report


def _same_decisions(report, ref):
    assert [(p["i"], p["j"], p["shift"], p["dist"]) for p in report["pairs"]] == [(p["i"], p["j"], p["shift"], p["dist"]) for p in ref["pairs"]]
    worst = 0.0
    for a, b in zip(report["pairs"], ref["pairs"]):
        assert a["candidates"] == b["candidates"] and list(a["ranks"]) == b["ranks"], (a["i"], a["j"], a["ranks"], b["ranks"])
        assert a["accepted"] == b["accepted"] and a["iterations"] == b["iterations"], (a["i"], a["j"], a["quality"], b["quality"], a["iterations"], b["iterations"])
        assert abs(a["quality"] - b["quality"]) <= 1e-9
        worst = max(worst, float(np.abs(np.array(a["Z"]) - b["Z"]).max()))
    return worst


def _unchanged_but_for_poses(corrected, kf):
    assert corrected["maps"] == kf["maps"] and len(corrected["frames"]) == len(kf["frames"])
    for a, b in zip(corrected["frames"], kf["frames"]):
        assert a["timestamp"] == b["timestamp"] and a["cov"] == b["cov"] and a["twist"] == b["twist"] and len(a["layers"]) == len(b["layers"])
        for (ma, xa), (mb, xb) in zip(a["layers"], b["layers"]):
            assert ma == mb and xa.tobytes() == np.asarray(xb, np.float32).tobytes()


def test_the_scenario_s_loop_is_closed_as_the_reference_closes_it(host, session, closed, oracle):
    corrected, report = closed
    ref = lr.scenario_reference(session["text"])
    worst_edge = _same_decisions(report, ref)
    assert sum(p["accepted"] for p in report["pairs"]) >= 1
    got = np.array([f["pose"] for f in corrected["frames"]])
    dt, dr = tc._pose_distance(got, ref["poses"])
    print("pairs", [(p["i"], p["j"], round(p["quality"], 4), p["iterations"], p["accepted"]) for p in report["pairs"]])
    print("|Z - reference|", worst_edge, "optimised poses against the reference: |dt|", dt, "|dr|", dr, "cost", report["cost_before"], "->",
          report["cost_after"], "iterations", report["optimizer_iterations"])
    print("seconds", report["seconds"], "counts", report["counts"])
    assert worst_edge < 1e-6
    assert dt < 1e-5 and dr < 1e-5
    # against the ground truth: the bounds the reference is held to
    for p in report["pairs"]:
        if p["accepted"]:
            err = float(np.linalg.norm((np.array(p["Z"]) - lc.relative(session["gt"][p["j"]], session["gt"][p["i"]]))[[3, 7, 11]]))
            assert err < tc.EDGE_BOUND, (p["i"], p["j"], err)
    e0, e1 = lc.position_errors(session["est"], session["gt"]), lc.position_errors(got, session["gt"])
    print("end error", e0[-1], "->", e1[-1], "max over the frames", e0.max(), "->", e1.max())
    assert e1[-1] <= tc.END_BOUND and e1.max() <= tc.MAX_BOUND
    # only the poses changed, node 0 not even that; every frame was described and searched once, every pair scored once
    _unchanged_but_for_poses(corrected, session["kf"])
    assert corrected["frames"][0]["pose"] == session["kf"]["frames"][0]["pose"]
    n = len(report["pairs"])
    assert report["counts"]["describe"] == 66 and report["counts"]["search"] == 66 and report["counts"]["score"] == n and report["counts"]["submap"] == n
    assert report["counts"]["refine"] == 4 * n and report["counts"]["optimize"] == 1
    assert json.loads(report["json"])["pairs"][0]["i"] == report["pairs"][0]["i"]


def test_the_corrected_file_differs_in_the_pose_bytes_only(host, session, closed):
    out = str(session["dir"] / "corrected.mhkf")
    host.write_keyframe_file(out, closed[0])
    tc.assert_only_poses_differ(open(session["kf_file"], "rb").read(), open(out, "rb").read(), session["kf"])
    # ... and the file-to-file form writes that very file
    again = str(session["dir"] / "corrected_again.mhkf")
    host.close_loops(session["kf_file"], host.Config.FromYamlText(session["text"]), again)
    assert open(again, "rb").read() == open(out, "rb").read()


def test_a_drive_without_a_revisit_comes_back_bit_for_bit(host, tmp_path):
    """the twelve street key-frames of tests/place_cases.py, 10 m apart: frames 30 m of travel apart stand 30 m apart, far outside the gate"""
    sweeps = [xyz for xyz, _ in pc.kf_sweeps(pc.scene())]
    kf = lc.keyframe_set([lc.synth.pose_from_ypr(pc.kf_pose(k)) for k in range(len(pc.KF_X))], sweeps)
    corrected, report = host.close_loops(kf, host.Config.FromYamlFile(PIPE))
    assert report["pairs"] == [] and report["optimizer_iterations"] == 0
    assert report["counts"]["describe"] == 12 and report["counts"]["search"] == 12
    assert not any(k in report["counts"] for k in ("submap", "score", "refine", "optimize"))   # nothing was verified: no score, no ICP
    a, b = str(tmp_path / "in.mhkf"), str(tmp_path / "out.mhkf")
    host.write_keyframe_file(a, kf)
    host.write_keyframe_file(b, corrected)
    assert open(a, "rb").read() == open(b, "rb").read()


def test_a_quality_nothing_reaches_rejects_every_pair(host, session, oracle):
    text = session["text"] + REJECT
    corrected, report = host.close_loops(session["kf"], host.Config.FromYamlText(text))
    ref = lr.scenario_reference(text)
    assert max(p["quality"] for p in ref["pairs"]) < 0.999   # (else the option would have to rise to what the reference rejects)
    worst = _same_decisions(report, ref)
    print("pairs", [(p["i"], p["j"], round(p["quality"], 4)) for p in report["pairs"]], "|Z - reference|", worst)
    assert len(report["pairs"]) > 4 and not any(p["accepted"] for p in report["pairs"]) and worst < 1e-6
    assert "optimize" not in report["counts"] and report["optimizer_iterations"] == 0
    a, b = str(session["dir"] / "rejected.mhkf"), session["kf_file"]
    host.write_keyframe_file(a, corrected)
    assert open(a, "rb").read() == open(b, "rb").read()


def test_the_shared_step_gives_what_relocalize_near_pose_records(host, oracle, monkeypatch, tmp_path):
    """tests/test_odometry_localize.py::test_relocalization_from_a_coarse_pose: a map of six scans, scan 6 relocalized from a pose 0.9 m /
    -0.6 m / 4 deg off.  The driver's record against mola_hip::score_rank_refine called with the same map, layer, grid and ICP block."""
    import score_ref as sr
    drive = lc.synth.make_drive(10)
    path = str(tmp_path / "session1.mhmap")
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    recs, _ = tl._mapping_run(host, drive, PIPE, path)
    pose6 = np.round(lr.oc.pose_to_ypr(np.array(recs[tl.N_MAPPED]["pose"])), 3)
    tl._set_env(monkeypatch, path, mapping=False)
    lo, o = tl._pair(host, PIPE, path)
    mean, cov = tl._coarse(pose6), sr.grid_cov(tl.SIGMAS[0], tl.SIGMAS[1], np.deg2rad(tl.SIGMAS[2]))
    lo.relocalizeNearPose(list(lc.synth.pose_from_ypr(mean)), list(cov))
    o.relocalize_near_pose(mean, cov)
    (xyz, t), st = drive["scans"][tl.N_MAPPED], drive["stamps"][tl.N_MAPPED]
    a, b = lo.onLidar(st, xyz, t), o.on_lidar(st, xyz, t)
    assert a["relocalized"] and a["n_for_icp"] == len(o.for_icp)
    # the same inputs by hand: the saved map, the layer the filters left (the reference's, which the device's equals), the grid
    cfg = host.Config.FromYamlFile(PIPE)
    icp, params = host.icp_pipeline_from_yaml(cfg["icp_settings_with_vel"])
    src = host.ParameterSource()
    icp.attachToParameterSource(src)
    icp.setKeepFinalPairings(False)
    for name, v in dict(lo.dynamicVariables(), ADAPTIVE_THRESHOLD_SIGMA=2.0, ICP_ITERATION=0.0).items():
        src.updateVariable(name, v)   # (the request is served before the scan's own registration: sigma is still the initial one)
    src.realize()
    saved = host.read_local_map_file(path)[0]["params"]
    m = host.HashedVoxelPointCloud(saved["voxel_size"], saved["max_points_per_voxel"])
    m.loadFromFile(path)
    glob, loc = host.metric_map_t(), host.metric_map_t()
    glob.set_layer("localmap", m)
    loc.set_layer("decimated_for_icp", host.PointCloud(o.for_icp))
    thr = 0.5 * saved["voxel_size"]   # half the map's voxel: the default score threshold, and the default step
    _, rows = host.relocalization_grid(list(mean), list(cov), thr, np.deg2rad(3.0))
    r = host.score_rank_refine(icp, params, loc, glob, "localmap", "decimated_for_icp", rows, thr, 4)
    print("ranks", r["ranks"], "n_paired", r["n_paired"], "quality", r["quality"], "iterations", r["iterations"])
    assert len(rows) == a["reloc_candidates"] and r["have"]
    assert list(r["ranks"]) == list(a["reloc_ranks"]) == b["reloc_ranks"] and r["n_paired"][0] == a["reloc_best_n_paired"]
    assert abs(r["quality"] - a["reloc_best_quality"]) <= 1e-9
    assert np.abs(np.array(r["pose"]) - np.array(a["init_guess"])).max() < 1e-9   # the scan's registration started from the winner


def test_the_command_line_closes_the_loops_of_a_file(host, session, closed, monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)
    d = session["dir"]
    out, rep, mp_file, want = str(d / "cli.mhkf"), str(d / "cli.json"), str(d / "cli.mhmap"), str(d / "api.mhkf")
    r = subprocess.run([CLI, "--close-loops", session["kf_file"], "--pipeline", session["text_file"], "--output-simplemap", out,
                        "--output-session-map", mp_file, "--loop-report", rep], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    host.write_keyframe_file(want, closed[0])
    assert open(out, "rb").read() == open(want, "rb").read()
    report = json.load(open(rep))
    assert [(p["i"], p["j"], p["accepted"]) for p in report["pairs"]] == [(p["i"], p["j"], p["accepted"]) for p in closed[1]["pairs"]]
    assert report["cost_after"] == closed[1]["cost_after"] and set(report["seconds"]) >= {"describe", "search", "submap", "score", "refine", "optimize"}
    summary = json.loads(r.stdout.strip().split("\n")[-1])
    assert summary["loops_closed"] == sum(p["accepted"] for p in closed[1]["pairs"]) and summary["frames"] == 66
    # the session map is build_session_maps of the corrected set, and a driver loads it
    built = host.build_session_maps(closed[0])
    recorded = host.build_session_maps(session["kf"])
    got = host.read_local_map_file(mp_file)
    assert len(got) == 1 and got[0]["xyz"].tobytes() == built[0]["xyz"].tobytes() and got[0]["src_idx"].tobytes() == built[0]["src_idx"].tobytes()
    monkeypatch.setenv("MOLA_LOAD_MM", mp_file)
    monkeypatch.setenv("MOLA_MAPPING_ENABLED", "false")
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlFile(PIPE))
    dump = lo.downloadMap("localmap")
    assert dump["xyz"].tobytes() == built[0]["xyz"].tobytes()
    print("occupied voxels of the session map: recorded poses", len(np.unique(np.floor(recorded[0]["xyz"]), axis=0)), "corrected poses", len(dump["vox_count"]),
          "points", len(recorded[0]["xyz"]), len(built[0]["xyz"]))
    # a form that is not complete is refused with the usage
    r = subprocess.run([CLI, "--close-loops", session["kf_file"], "--pipeline", session["text_file"]], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--output-simplemap" in r.stderr
