"""Online loop closure on the device: mola_hip::OnlineLoopCloser against mola_hip::close_loops, bit for bit, on the scenario of
tests/loop_cases.py (66 key-frames around one block and 36 m into it again), and LidarOdometry's online_loop_closure: block on the
out-and-back drive of tests/loop_online_ref.py (120 sweeps of 32 x 600: 31 m down a street and back in reverse gear) -- observing
only, feeding the closure back into pose, motion model, key-frame store and local map, and from the command line.

The identity is the specification: fed the frames one at a time, the closer tries the pairs close_loops tries, with the same
candidate counts, ranks, iterations, qualities, decisions and edges, and after every push its corrected poses are close_loops' for the
frames pushed so far.  Through tests/test_gpu_loop.py (close_loops against tests/loop_ref.py) the online result inherits the
reference, and the ground-truth bounds of tests/test_loop_cpu.py are asserted on it here as well.  The conditions -- the reference
closes the scenario's four pairs, and closes a loop on the CPU oracle's key-frames of the drive -- are held by
tests/test_loop_online_cpu.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import loop_cases as lc
import loop_online_ref as ol
import loop_ref as lr
import test_loop_cpu as tc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPE = os.path.join(ROOT, "pipelines", "lidar3d-default-hip.yaml")
CLI = os.path.join(ROOT, "mola_lidar_odometry_amd", "molahip-lo-cli")
REJECT = "  min_quality: 0.999\n"   # the reference's best pair reaches 0.9941 (tests/test_gpu_loop.py)
PAIR_FIELDS = ("i", "j", "shift", "dist", "candidates", "ranks", "iterations", "quality", "accepted")
NEW_FIELDS = ("loop_tried", "loop_closed", "loop_pairs", "loop_correction_trans", "loop_correction_rot", "loop_rebuilt_frames")


def _same_existing_fields(a, b):
    """every field of two scan records but those this feature adds"""
    assert set(a) == set(b) and set(NEW_FIELDS) <= set(a)
    for k in a:
        if k not in NEW_FIELDS:
            assert a[k] == b[k], (a["timestamp"], k, a[k], b[k])


# the usage text of the commit before this feature: what a run without the block and without the new option still prints
PARENT_USAGE_HEAD = ("usage: molahip-lo-cli --pipeline FILE.yaml --seq-dir DIR [--seq-dir DIR ...] --out FILE.tum [--device N | --devices 0,1,..|all] "
                     "[--no-prefetch] [--max-scans N] [--profile] [--time-field BYTES] [--intensity-field BYTES] [--scan-log FILE|auto] [--plan-only]\n"
                     "                      [--save-local-map FILE] [--output-simplemap FILE] [--output-session-map FILE] [--relocalize-in-keyframes]\n"
                     "       molahip-lo-cli --build-session-map KEYFRAMES --save-local-map FILE [--device N]\n")
PARENT_USAGE_TAIL = "  --devices: the sequences are spread over the listed GPUs (longest first onto the least loaded device)\n"
PARENT_SUMMARY_KEYS = ["sequences", "devices", "scans", "wall_seconds", "scans_per_s", "steady_scans_per_s", "batches", "jobs_per_batch",
                       "ms_per_batch_assembling", "ms_per_batch_running", "filter_batches", "filter_jobs", "filter_timeouts", "one_launch_loops",
                       "one_launch_loops_abandoned", "per_device"]
PARENT_SEQUENCE_KEYS = ["sequence_dir", "device", "scans", "good", "keyframes", "icp_iterations", "seconds", "scans_per_s", "steady_scans_per_s",
                       "mean_raw_points", "mean_icp_points", "mean_map_layer_points", "final_map_points", "max_map_points", "final_map_voxels", "tum"]


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in ol.ENV:
        monkeypatch.delenv(v, raising=False)


# ---- the closer against close_loops ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def session():
    s = lc.scenario()
    return dict(kf=lc.keyframe_set(s["est"], s["sweeps"]), text=open(PIPE).read() + lc.OPTIONS, gt=s["gt"], est=s["est"], sweeps=s["sweeps"])


def _poses(kf):
    return np.array([f["pose"] for f in kf["frames"]], np.float64)


def _same_pairs(a, b):
    assert len(a) == len(b)
    for p, q in zip(a, b):
        for k in PAIR_FIELDS:
            assert (list(p[k]) if k == "ranks" else p[k]) == (list(q[k]) if k == "ranks" else q[k]), (p["i"], p["j"], k, p[k], q[k])
        assert np.array(p["Z"], np.float64).tobytes() == np.array(q["Z"], np.float64).tobytes(), (p["i"], p["j"])


def test_frame_by_frame_is_close_loops_bit_for_bit(host, session):
    kf, cfg = session["kf"], host.Config.FromYamlText(session["text"])
    closer = host.OnlineLoopCloser(kf["maps"], cfg)
    assert closer.options() == dict(enabled=False, correct_driver=True, check_every_n_keyframes=1) and closer.size() == 0
    checks, steps = {}, []
    for i, f in enumerate(kf["frames"]):
        st = closer.push(f)
        steps.append(st)
        assert st["tried"] == (len(st["pairs"]) > 0) and st["closed"] == any(p["accepted"] for p in st["pairs"])
        if st["closed"] or i == 60:   # after every push that closed -- and once between two closures
            checks[i] = closer.correctedPoses().copy()
        elif not closer.loops():
            assert closer.correctedPoses().tobytes() == closer.rawPoses().tobytes()
    corrected, report = host.close_loops(kf, cfg)
    rep = closer.report()
    print("pairs", [(p["i"], p["j"], round(p["quality"], 4), p["iterations"], p["accepted"]) for p in rep["pairs"]], "seconds", rep["seconds"], "counts", rep["counts"])
    _same_pairs(rep["pairs"], report["pairs"])
    _same_pairs([p for st in steps for p in st["pairs"]], report["pairs"])
    assert closer.correctedPoses().tobytes() == _poses(corrected).tobytes()
    assert closer.rawPoses().tobytes() == np.asarray(session["est"], np.float64).tobytes() and closer.size() == 66
    closed_at = [i for i, st in enumerate(steps) if st["closed"]]
    assert closed_at == [56, 59, 62, 65] and sorted(checks) == [56, 59, 60, 62, 65]
    for i, poses in checks.items():
        part, _ = host.close_loops(dict(maps=kf["maps"], frames=kf["frames"][:i + 1]), cfg)
        assert poses.tobytes() == _poses(part).tobytes(), i
    assert [(a, b) for a, b, _ in closer.loops()] == [(p["j"], p["i"]) for p in report["pairs"] if p["accepted"]]
    n = len(rep["pairs"])
    assert rep["counts"]["describe"] == 66 and rep["counts"]["search"] == 66 and rep["counts"]["optimize"] == 4
    assert rep["counts"]["score"] == n and rep["counts"]["submap"] == n and rep["counts"]["refine"] == 4 * n
    assert rep["cost_before"] == report["cost_before"] and rep["cost_after"] == report["cost_after"] and rep["optimizer_iterations"] == report["optimizer_iterations"]
    assert json.loads(rep["json"])["pairs"][0]["i"] == 56
    # the ground-truth bounds the reference is held to (tests/test_loop_cpu.py), on the online result
    got = closer.correctedPoses()
    for p in rep["pairs"]:
        if p["accepted"]:
            err = float(np.linalg.norm((np.array(p["Z"]) - lc.relative(session["gt"][p["j"]], session["gt"][p["i"]]))[[3, 7, 11]]))
            assert err < tc.EDGE_BOUND, (p["i"], p["j"], err)
    e0, e1 = lc.position_errors(session["est"], session["gt"]), lc.position_errors(got, session["gt"])
    print("end error", e0[-1], "->", e1[-1], "max over the frames", e0.max(), "->", e1.max())
    assert e1[-1] <= tc.END_BOUND and e1.max() <= tc.MAX_BOUND
    raw = closer.rawKeyFrames()
    assert raw["maps"] == kf["maps"] and [f["pose"] for f in raw["frames"]] == [f["pose"] for f in kf["frames"]]


def test_every_third_key_frame_and_a_quality_nothing_reaches(host, session):
    kf = session["kf"]
    text = session["text"] + REJECT + ol.online_block(every=3)
    cfg = host.Config.FromYamlText(text)
    assert host.loop_closure_options(cfg)["min_quality"] == 0.999
    closer = host.OnlineLoopCloser(kf["maps"], cfg)
    assert closer.options()["check_every_n_keyframes"] == 3
    for f in kf["frames"]:
        st = closer.push(f)
        assert not st["closed"]
    has = [True] * 66
    want = ol.fold_candidates(host.loop_candidates_step, session["est"], has, lr.match_lists(session["sweeps"], has), host.loop_closure_options(cfg),
                              lambda i, j, shift, dist: False, frames=range(0, 66, 3))
    rep = closer.report()
    print("pairs", [(p["i"], p["j"], round(p["quality"], 4)) for p in rep["pairs"]])
    assert [(p["i"], p["j"], p["shift"], p["dist"]) for p in rep["pairs"]] == want and len(want) >= 3 and all(i % 3 == 0 for i, _, _, _ in want)
    assert not any(p["accepted"] for p in rep["pairs"]) and closer.loops() == []
    assert closer.correctedPoses().tobytes() == closer.rawPoses().tobytes() == np.asarray(session["est"], np.float64).tobytes()
    assert rep["counts"]["describe"] == 66 and rep["counts"]["search"] == 22 and "optimize" not in rep["counts"]


def test_a_push_that_throws_leaves_the_closer_as_it_was(host, session):
    """a candidate grid larger than relocalization.max_candidates makes the verification of frame 56 throw on the host, before anything
    is scored: frames 0 .. 55 stay pushed, frame 56 is not, and nothing of it is left behind"""
    text = session["text"]
    assert text.count("  max_candidates: 65536") == 1
    kf, cfg = session["kf"], host.Config.FromYamlText(text.replace("  max_candidates: 65536", "  max_candidates: 100"))
    closer = host.OnlineLoopCloser(kf["maps"], cfg)
    for f in kf["frames"][:56]:
        assert not closer.push(f)["tried"]
    before = (closer.size(), closer.rawPoses().tobytes(), closer.correctedPoses().tobytes(), closer.loops(), closer.report()["pairs"])
    for _ in range(2):   # ... so the same frame can be offered again, and is refused for the same reason
        with pytest.raises(RuntimeError, match="candidates"):
            closer.push(kf["frames"][56])
        assert (closer.size(), closer.rawPoses().tobytes(), closer.correctedPoses().tobytes(), closer.loops(), closer.report()["pairs"]) == before
    assert closer.size() == 56 and len(closer.rawKeyFrames()["frames"]) == 56
    with pytest.raises(RuntimeError, match="non-finite pose"):
        closer.push(dict(kf["frames"][56], pose=[float("nan")] * 12))
    assert closer.size() == 56


# ---- the driver ----------------------------------------------------------------------------------------------------------------------
def _dump_equal(a, b):
    for k in ("xyz", "src_idx"):
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def _run(host, text, drive, watch=None):
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlText(text))
    for n, ((xyz, t), st) in enumerate(zip(drive["scans"], drive["stamps"])):
        rec = lo.onLidar(st, xyz, t)
        if watch is not None:
            watch(lo, n, rec)
    return lo


@pytest.fixture(scope="module")
def plain(host, tmp_path_factory):
    """the drive without the block: records, trajectory, local map, key-frame file"""
    with pytest.MonkeyPatch.context() as mp:
        for v in ol.ENV:
            mp.delenv(v, raising=False)
        lo = _run(host, ol.pipeline_text(), ol.drive())
    path = str(tmp_path_factory.mktemp("online") / "plain.mhkf")
    lo.saveKeyFrames(path)
    return dict(records=lo.records(), trajectory=lo.trajectory(), map=lo.downloadMap("localmap"), file=open(path, "rb").read(), kf=lo.keyFrames())


def test_observing_only_changes_nothing_but_the_new_record_fields(host, plain, tmp_path):
    lo = _run(host, ol.pipeline_text(ol.online_block(correct_driver=False)), ol.drive())
    recs = lo.records()
    assert len(recs) == len(plain["records"]) == ol.N_SCANS
    for a, b in zip(recs, plain["records"]):
        _same_existing_fields(a, b)
    assert lo.trajectory() == plain["trajectory"]
    _dump_equal(lo.downloadMap("localmap"), plain["map"])
    path = str(tmp_path / "observed.mhkf")
    lo.saveKeyFrames(path)
    assert open(path, "rb").read() == plain["file"]
    closed = [r for r in recs if r["loop_closed"]]
    print("key-frames", len(plain["kf"]["frames"]), "closures", [(r["loop_pairs"]) for r in closed])
    assert len(closed) >= 1 and all(r["loop_tried"] and r["simplemap_keyframe"] and r["loop_pairs"][-1][3] for r in closed)
    assert all(r["loop_correction_trans"] == 0.0 and r["loop_rebuilt_frames"] == 0 for r in recs)      # nothing was fed back
    assert not any(r["loop_tried"] or r["loop_closed"] or r["loop_pairs"] for r in plain["records"])
    # the closer saw the stored frames with the poses the store holds (nothing corrected them), and its result is the off-line one
    c = lo.loopCloser()
    raw = lo.rawKeyFrames()
    assert c.rawPoses().tobytes() == _poses(plain["kf"]).tobytes() == _poses(raw).tobytes()
    off, report = host.close_loops(raw, host.Config.FromYamlText(ol.pipeline_text()))
    assert c.correctedPoses().tobytes() == _poses(off).tobytes() and len(c.loops()) == sum(p["accepted"] for p in report["pairs"]) == len(closed)
    # the corrected trajectory hangs on the closer's poses; the estimated one is what it was
    ct = lo.correctedTrajectory()
    assert [t for t, _ in ct] == [t for t, _ in plain["trajectory"]] and ct != plain["trajectory"]


def test_a_closure_fed_back_into_the_driver(host, plain, tmp_path):
    drive = ol.drive()
    text = ol.pipeline_text(ol.online_block(correct_driver=True))
    cfg = host.Config.FromYamlText(text)
    seen = dict(first=None, anchors=[], rels=[], traj_len=0, n_stored=0, store_pose=None)
    step_gt = np.linalg.norm(np.diff(drive["poses"][:, [3, 7, 11]], axis=0), axis=1)

    def watch(lo, n, rec):
        kf = lo.keyFrames()
        # the corrected-trajectory rule's inputs, as recorded: the entry this scan made, the last stored frame at or before it, and the
        # pose the store held for that frame when the entry was made -- the scan's own pose for a stored scan, else what the store held
        # after the scan before (a closure of this very scan comes after the entry)
        traj = lo.trajectory()
        seen["n_stored"] += int(rec["simplemap_frame"])
        if len(traj) > seen["traj_len"]:
            seen["traj_len"] = len(traj)
            a = seen["n_stored"] - 1
            S = traj[-1][1] if rec["simplemap_frame"] else seen["store_pose"]
            seen["anchors"].append(a)
            seen["rels"].append(None if a < 0 else ol.anchor(traj[-1][1], S))
        if kf["frames"]:
            seen["store_pose"] = kf["frames"][-1]["pose"]
        if rec["loop_closed"] and seen["first"] is None:
            seen["first"] = n
            raw = lo.rawKeyFrames()
            assert len(raw["frames"]) == len(kf["frames"])
            off, _ = host.close_loops(raw, cfg)
            assert _poses(kf).tobytes() == _poses(off).tobytes()                                   # 1. the store holds the off-line result
            assert rec["pose"] == kf["frames"][-1]["pose"]                                          # 2. the vehicle stands at C_i
            P = lo.trajectory()[-1][1]                                                              #    (the trajectory keeps P_i)
            delta = ol.correction(rec["pose"], P)
            assert abs(rec["loop_correction_trans"] - np.linalg.norm(delta[[3, 7, 11]])) < 1e-9 and rec["loop_correction_trans"] > 0.0
            assert abs(rec["loop_correction_rot"] - np.linalg.norm(lr.log_so3(lc.to44(delta)[:3, :3]))) < 1e-9 and rec["loop_correction_rot"] > 0.0
            for k, m in enumerate(kf["maps"]):                                                     # 3. every local map rebuilt from the key-frames around
                keep = ol.rebuild_frames(kf, k, rec["pose"])
                built = host.build_session_maps(dict(maps=kf["maps"], frames=[kf["frames"][q] for q in keep]))
                _dump_equal(lo.downloadMap(m["name"]), built[k])
                if k == 0:
                    assert rec["loop_rebuilt_frames"] == len(keep) >= 10
            assert rec["n_map_points"] == len(lo.downloadMap("localmap")["xyz"])
            print("closing scan", n, "pairs", rec["loop_pairs"], "correction [m, rad]", rec["loop_correction_trans"], rec["loop_correction_rot"],
                  "rebuilt from", rec["loop_rebuilt_frames"], "frames")

    lo = _run(host, text, drive, watch)
    recs = lo.records()
    first = seen["first"]
    assert first is not None and first < ol.N_SCANS - 10
    # up to the closing scan the run is the plain one
    for a, b in zip(recs[:first], plain["records"][:first]):
        _same_existing_fields(a, b)
    # 4. the drive goes on in the corrected frame: every later scan registers at the pipeline's min_icp_goodness or better, and no pose
    #    jumps.  The pose-by-pose agreement of this run (1e-6) is with the CPU oracle's driver under the same feedback rules, in the
    #    test below; here, against the ground truth alone: consecutive poses stand the drive's own step apart within 0.1 m.  That
    #    figure is tests/test_loop_cpu.py's EDGE_BOUND, the accuracy a verified loop edge is held to against the truth on sweeps of
    #    this kind -- so it bounds what one registration may be off by -- and it is not taken from this run: a map and a pose that
    #    disagreed after the feedback would show as a jump of the size of a map voxel (0.5 m and more)
    min_goodness = float(lr.oo.load_pipeline_text(text)["params"]["min_icp_goodness"])
    assert 0.0 < min_goodness < 1.0
    poses = np.array([r["pose"] for r in recs])
    for n in range(first + 1, ol.N_SCANS):
        assert recs[n]["icp_good"] and recs[n]["goodness"] >= min_goodness, (n, recs[n]["goodness"])
        if not recs[n]["loop_closed"]:
            d = float(np.linalg.norm(poses[n][[3, 7, 11]] - poses[n - 1][[3, 7, 11]]))
            assert abs(d - step_gt[n - 1]) <= tc.EDGE_BOUND, (n, d, step_gt[n - 1])
    # 5. the corrected trajectory is the numpy rule on the recorded data
    C = lo.loopCloser().correctedPoses()
    traj = lo.trajectory()
    want = ol.corrected_trajectory(traj, seen["anchors"], seen["rels"], C)
    got = lo.correctedTrajectory()
    assert len(got) == len(want) == len(traj)
    worst = max(float(np.abs(np.array(p) - q).max()) for (_, p), (_, q) in zip(got, want))
    print("corrected trajectory against the numpy rule", worst)
    assert worst < 1e-9 and [t for t, _ in got] == [t for t, _ in traj]
    # 6. at the end of the drive the store still holds what close_loops gives on the raw frames
    kf, raw = lo.keyFrames(), lo.rawKeyFrames()
    off, report = host.close_loops(raw, cfg)
    assert _poses(kf).tobytes() == _poses(off).tobytes() and lo.loopCloser().correctedPoses().tobytes() == _poses(off).tobytes()
    assert sum(p["accepted"] for p in report["pairs"]) == sum(r["loop_closed"] for r in recs) == len(lo.loopCloser().loops()) >= 1
    path = str(tmp_path / "corrected.mhkf")
    lo.saveKeyFrames(path)
    assert _poses(host.read_keyframe_file(path)).tobytes() == _poses(kf).tobytes()
    # ground truth: the corrected end of the drive is where it started, as well as the uncorrected one was
    gt0 = np.linalg.inv(lc.to44(drive["poses"][0]))
    truth = np.array([lc.to12(gt0 @ lc.to44(p)) for p in drive["poses"]])
    e_plain = float(np.linalg.norm(np.array(plain["records"][-1]["pose"])[[3, 7, 11]] - truth[-1][[3, 7, 11]]))
    e_fed = float(np.linalg.norm(poses[-1][[3, 7, 11]] - truth[-1][[3, 7, 11]]))
    print("end position error: plain", e_plain, "with feedback", e_fed)
    assert e_fed <= e_plain + tc.EDGE_BOUND


def test_a_loaded_session_s_frames_go_first(host, plain, tmp_path, monkeypatch):
    """load_existing_simple_map: the file's frames are pushed before the first new one, with their file poses as raw poses; the loops
    among them are closed at the first stored scan and fed back like any other"""
    path = str(tmp_path / "session.mhkf")
    open(path, "wb").write(plain["file"])
    monkeypatch.setenv("MOLA_LOAD_SM", path)
    text = ol.pipeline_text(ol.online_block())
    cfg = host.Config.FromYamlText(text)
    drive, n_file = ol.drive(), len(plain["kf"]["frames"])
    lo = host.LidarOdometry()
    lo.initialize(cfg)
    assert lo.loopCloser() is None and len(lo.keyFrames()["frames"]) == n_file
    rec = lo.onLidar(drive["stamps"][0], *drive["scans"][0])
    assert rec["first_scan"] and rec["simplemap_keyframe"]
    c, kf, raw = lo.loopCloser(), lo.keyFrames(), lo.rawKeyFrames()
    assert c.size() == n_file + 1 == len(kf["frames"])
    assert c.rawPoses()[:n_file].tobytes() == _poses(plain["kf"]).tobytes()
    # the new frame hangs on the last loaded one by P (-) S: nothing had been corrected when it was stored, so its raw pose is its own
    assert c.rawPoses()[n_file].tobytes() == np.array(lo.trajectory()[0][1]).tobytes()
    off_file, rep_file = host.close_loops(plain["kf"], cfg)
    assert sum(p["accepted"] for p in rep_file["pairs"]) >= 1
    _same_pairs(c.report()["pairs"][:len(rep_file["pairs"])], rep_file["pairs"])
    off, _ = host.close_loops(raw, cfg)
    assert _poses(kf).tobytes() == _poses(off).tobytes() and rec["pose"] == kf["frames"][-1]["pose"] and rec["loop_correction_trans"] > 0.0
    keep = ol.rebuild_frames(kf, 0, rec["pose"])
    assert rec["loop_rebuilt_frames"] == len(keep) == n_file + 1
    _dump_equal(lo.downloadMap("localmap"), host.build_session_maps(dict(maps=kf["maps"], frames=[kf["frames"][q] for q in keep]))[0])


def test_set_align_batcher_on_an_instance_with_a_context_of_its_own(host):
    """(an instance on the default context is refused for that already: tests/test_loop_online_cpu.py)"""
    lo = host.LidarOdometry(device=0, own_context=True)
    lo.initialize(host.Config.FromYamlText(ol.pipeline_text(ol.online_block())))
    with pytest.raises(RuntimeError, match=r"online_loop_closure: enabled .*AlignBatcher"):
        lo.setAlignBatcher(host.AlignBatcher(1))
    plain = host.LidarOdometry(device=0, own_context=True)
    plain.initialize(host.Config.FromYamlText(ol.pipeline_text()))
    batcher = host.AlignBatcher(1)
    plain.setAlignBatcher(batcher)      # without the block: accepted as before
    batcher.leave()


def test_the_command_line(host, tmp_path):
    drive = ol.drive()
    stamps = np.asarray(drive["stamps"]) - drive["stamps"][0]
    seq = ol.synth.write_kitti_sequence(str(tmp_path / "kitti"), dict(scans=drive["scans"], stamps=np.asarray(drive["stamps"])),
                                        intensities=[t for _, t in drive["scans"]])      # the per-point time in the fourth float
    on, off = str(tmp_path / "on.yaml"), str(tmp_path / "off.yaml")
    open(on, "w").write(ol.pipeline_text(ol.online_block()))
    open(off, "w").write(ol.pipeline_text())
    out, cor = str(tmp_path / "est.tum"), str(tmp_path / "corrected.tum")
    r = subprocess.run([CLI, "--pipeline", on, "--seq-dir", seq, "--out", out, "--time-field", "12", "--no-prefetch", "--output-corrected-trajectory", cor],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.strip().split("\n")]
    per_sequence, summary = lines[0], lines[-1]
    # the same run in this process
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlFile(on))
    for (xyz, t), st in zip(drive["scans"], stamps):
        lo.onLidar(float("%.6e" % st), np.concatenate([xyz, t[:, None]], 1).astype(np.float32), t_field=3)
    want_est, want_cor = str(tmp_path / "api_est.tum"), str(tmp_path / "api_corrected.tum")
    lo.saveTrajectoryTUM(want_est)
    lo.saveCorrectedTrajectoryTUM(want_cor)
    assert open(out).read() == open(want_est).read() and open(cor).read() == open(want_cor).read()
    assert open(cor).read() != open(out).read()
    assert list(per_sequence) == PARENT_SEQUENCE_KEYS + ["loops_closed"] and list(summary) == PARENT_SUMMARY_KEYS + ["loops_closed"]
    assert summary["loops_closed"] == per_sequence["loops_closed"] == len(lo.loopCloser().loops()) >= 1
    # without the block: the summary's keys and the usage are the parent's
    r = subprocess.run([CLI, "--pipeline", off, "--seq-dir", seq, "--out", out, "--time-field", "12", "--max-scans", "5"], capture_output=True, text=True, timeout=300)
    lines = [json.loads(l) for l in r.stdout.strip().split("\n")]
    assert r.returncode == 0 and list(lines[0]) == PARENT_SEQUENCE_KEYS and list(lines[-1]) == PARENT_SUMMARY_KEYS
    r = subprocess.run([CLI, "--pipeline", off], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and r.stderr.startswith(PARENT_USAGE_HEAD) and r.stderr.endswith(PARENT_USAGE_TAIL) and "--output-corrected-trajectory" not in r.stderr
    r = subprocess.run([CLI, "--pipeline", on], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and r.stderr.startswith(PARENT_USAGE_HEAD) and "--output-corrected-trajectory" in r.stderr
    # several sequences of one process align through an AlignBatcher: refused with the block
    r = subprocess.run([CLI, "--pipeline", on, "--seq-dir", seq, "--seq-dir", seq, "--out", out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "AlignBatcher" in r.stderr and "online_loop_closure" in r.stderr


def test_the_fed_back_drive_scan_by_scan_against_the_oracle_s_driver(host, oracle):
    """tests/loop_online_ref.py restates the feedback rules on the CPU oracle's driver; the device's records against its records: the
    decisions identical, the poses within the 1e-6 the drivers are held to elsewhere (tests/test_odometry_localize.py)"""
    drive = ol.drive()
    block = ol.online_block(correct_driver=True)
    lo = _run(host, ol.pipeline_text(block), drive)
    o = ol.OnlineOracle(block, True)
    for (xyz, t), st in zip(drive["scans"], drive["stamps"]):
        o.on_lidar(st, xyz, t)
    worst, closures = 0.0, 0
    for n, (a, b) in enumerate(zip(lo.records(), o.records)):
        for k in ("dropped", "first_scan", "icp_run", "icp_good", "had_motion_model", "map_updated", "restarted", "icp_iterations", "twist_corrections",
                  "simplemap_frame", "loop_tried", "loop_closed", "n_map_points", "n_map_voxels"):
            assert a[k] == b[k], (n, k, a[k], b[k])
        assert [(i, j, acc) for i, j, _, acc in a["loop_pairs"]] == [(i, j, acc) for i, j, _, acc in b["loop_pairs"]], n
        assert all(abs(p[2] - q[2]) <= 1e-9 for p, q in zip(a["loop_pairs"], b["loop_pairs"]))
        if a["loop_closed"]:
            closures += 1
            assert a["loop_rebuilt_frames"] == b["loop_rebuilt_frames"]
        worst = max(worst, float(np.abs(np.array(a["pose"]) - np.asarray(b["pose"])).max()))
    print("closures", closures, "largest pose difference against the oracle's driver", worst)
    assert closures >= 1 and worst < 1e-6
    got, want = _poses(lo.keyFrames()), np.array([f["pose"] for f in o.frames])
    assert got.shape == want.shape and float(np.abs(got - want).max()) < 1e-6
    assert float(np.abs(_poses(lo.rawKeyFrames()) - np.array(o.raw)).max()) < 1e-6
