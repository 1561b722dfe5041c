"""lost_recovery: on the device driver (mola_hip::LidarOdometry) against tests/lost_recovery_ref.py, the restatement on the CPU oracle's
driver, on the drives of tests/lost_recovery_cases.py through the 12-key-frame session of tests/place_cases.py (made on the device as
tests/test_odometry_place.py makes it; it is the reference's own bit for bit, which is asserted here again).  Mapping is on, both
session files are loaded, the first scan's true pose is the fixed initial pose and every run asks for the place scenario's 0.9.

  * enabled, kidnapped by 49.6 m: the device agrees with the reference scan by scan (state, streak, attempts, gate, place search,
    candidates, poses within the 1e-6 of test_odometry_place.py), is within that test's 0.1 m of the ground truth from the recovering
    scan to the end, and its map is untouched from the scan that lost to the scan that recovered;
  * disabled and absent: byte-identical to each other, the new record fields at their defaults, the vehicle stays lost;
  * no kidnap, enabled: byte-identical to the run without the block;
  * an own request that cannot be served (relocalization.max_candidates below one key-frame's grid) is a failed attempt, not an
    exception out of every later scan; after max_attempts of them the driver has given up and the records say so;
  * method: near on a 3 m cut; a glitch of four foreign sweeps after which good alignments, not a request, bring the driver back; what
    initialize() refuses with the session loaded.

tests/test_lost_recovery_cpu.py shows on the CPU that the reference alone does what the first and fourth case rest on."""
import numpy as np
import pytest

import lost_recovery_cases as lc
import lost_recovery_ref as lrr
import place_cases as pc
import test_odometry_localize as tl
from mola_lidar_odometry_amd import synth

pytestmark = pytest.mark.gpu

NEW_FIELDS = dict(lost=False, recovery_attempt=0, recovery_succeeded=False, bad_streak=0, recovery_gave_up=False)
STATE = ("lost", "bad_streak", "recovery_attempt", "recovery_succeeded", "recovery_gave_up", "icp_good", "relocalization_tried", "relocalized", "place_tried")
SEARCH = ("place_frames", "place_shifts", "place_dists", "reloc_ranks")


@pytest.fixture(scope="module")
def host():
    from mola_lidar_odometry_amd import _mp2p_icp_hip as H
    return H


@pytest.fixture(scope="module")
def session(host, oracle, tmp_path_factory):
    """the key-frame file and the session map file, made on the device (the recipe of tests/test_odometry_place.py)"""
    d = tmp_path_factory.mktemp("lost")
    frames, maps = [], None
    with pytest.MonkeyPatch.context() as mp:
        for v in lc.ENV:
            mp.delenv(v, raising=False)
        mp.setenv("MOLA_GENERATE_SIMPLEMAP", "true")
        for k, (xyz, t) in enumerate(pc.kf_sweeps(pc.scene())):
            lo = host.LidarOdometry()
            lo.initialize(host.Config.FromYamlFile(lc.PIPE))
            assert lo.onLidar(1000.0 + k, xyz, t)["simplemap_keyframe"]
            kf = lo.keyFrames()
            maps = maps or kf["maps"]
            f = dict(kf["frames"][0])
            f["pose"] = [float(v) for v in synth.pose_from_ypr(pc.kf_pose(k))]
            frames.append(f)
    kf_file, map_file = str(d / "session.mhkf"), str(d / "session.mhmap")
    host.write_keyframe_file(kf_file, dict(maps=maps, frames=frames))
    host.build_session_maps(kf_file, 0, map_file)
    return dict(kf_file=kf_file, map_file=map_file, dir=d, runs={})


def _run(host, session, name, extra, max_candidates=None):
    """drive(name) through a fresh device driver under pipeline_text(extra, max_candidates): records, trajectory, map dump, key-frame file bytes and
    the counters; once per (name, extra), unchanged by whoever asks"""
    key = (name, extra, max_candidates)
    if key in session["runs"]:
        return session["runs"][key]
    with pytest.MonkeyPatch.context() as mp:
        for v in lc.ENV:
            mp.delenv(v, raising=False)
        for k, v in lc.environment(session["map_file"], session["kf_file"]).items():
            mp.setenv(k, v)
        lo = host.LidarOdometry()
        lo.initialize(host.Config.FromYamlText(lc.pipeline_text(extra, max_candidates)))
        d = lc.drive(name)
        recs = [lo.onLidar(st, xyz, t) for (xyz, t), st in zip(d["scans"], d["stamps"])]
    kf_out = str(session["dir"] / ("kf_%d.mhkf" % len(session["runs"])))
    lo.saveKeyFrames(kf_out)
    out = dict(records=lo.records(), returned=recs, trajectory=lo.trajectory(), dump=lo.downloadMap("localmap"), keyframes=open(kf_out, "rb").read(),
               counts=(lo.isLost(), lo.timesLost(), lo.recoveryAttempts(), lo.timesRecovered()), profile=dict(lo.profile()),
               pending=lo.relocalizationPending(), gave_up=lo.recoveryGaveUp(), error=lo.lastRecoveryError())
    session["runs"][key] = out
    return out


def _same_run(a, b):
    assert a["records"] == b["records"] and a["trajectory"] == b["trajectory"] and a["keyframes"] == b["keyframes"]
    tl._same_dump(a["dump"], b["dump"])


def _compare_records(got, want):
    """state, attempts, gate, place search and candidates identical; -> the largest pose difference"""
    worst = 0.0
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        for key in STATE:
            assert a[key] == b[key], (k, key, a[key], b[key])
        for key in SEARCH:
            assert list(a[key]) == list(b[key]), (k, key, a[key], b[key])
        assert a["reloc_candidates"] == b["reloc_candidates"] and a["reloc_best_n_paired"] == b["reloc_best_n_paired"], k
        assert abs(a["reloc_best_quality"] - b["reloc_best_quality"]) <= 1e-9, (k, a["reloc_best_quality"], b["reloc_best_quality"])
        worst = max(worst, tl._compare(k, a, b))
    return worst


def _against_the_reference(host, session, name, extra, max_candidates=None):
    got = _run(host, session, name, extra, max_candidates)
    want, o = lc.reference_run(name, extra, max_candidates)
    worst = _compare_records(got["records"], want)
    assert worst < 1e-6, worst
    assert got["counts"] == (o.m.lost, o.m.times_lost, o.m.attempts, o.m.times_recovered) and got["gave_up"] == o.m.gave_up()
    return got, want, o, worst


def test_the_session_is_the_one_the_reference_was_chosen_on(host, session):
    frames, rec = lc.cpu_session()
    got = host.read_keyframe_file(session["kf_file"])["frames"]
    assert len(got) == len(frames) == 12
    for f, g in zip(frames, got):
        assert f["pose"] == g["pose"] and np.asarray(f["layers"][0][1], np.float32).tobytes() == g["layers"][0][1].tobytes()
    dev = host.read_local_map_file(session["map_file"])[0]
    assert np.asarray(dev["xyz"], np.float32).tobytes() == np.asarray(rec["xyz"], np.float32).tobytes()
    assert float(dev["remove_voxels_farther_than"]) == rec["remove_voxels_farther_than"] > 0   # (mapping is on: the radius counts)


def test_a_kidnapped_vehicle_is_found_again_as_the_reference_finds_it(host, session):
    d = lc.drive("kidnap")
    got, want, o, worst = _against_the_reference(host, session, "kidnap", lc.block(True))
    recs, cut = got["records"], d["cut"]
    lost_at = next(k for k, r in enumerate(recs) if r["bad_streak"] >= lrr.DEFAULTS["bad_scans_to_lost"])   # the scan that lost
    won = next(k for k, r in enumerate(recs) if r["recovery_succeeded"])
    attempts = [(k, r["recovery_attempt"], r["recovery_succeeded"], round(r["reloc_best_quality"], 3)) for k, r in enumerate(recs) if r["recovery_attempt"]]
    errs = [lc.position_error(r, d["poses"][k]) for k, r in enumerate(recs)]
    print("lost at", lost_at, "rejected", [round(r["goodness"], 3) for r in recs[cut:lost_at + 1]], "attempts", attempts, "|pose - reference|", worst,
          "errors from scan", won, "on: max %.3f last %.3f" % (max(errs[won:]), errs[-1]),
          "profile", {k: v for k, v in got["profile"].items() if k.startswith(("lost_recovery.", "relocalize.", "onLidar.2.relocalize"))})
    assert lost_at == cut + 2 and not recs[lost_at]["lost"] and all(r["lost"] for r in recs[lost_at + 1:won + 1]) and not any(r["lost"] for r in recs[won + 1:])
    assert [a[1] for a in attempts] == [lrr.KEYFRAMES] * len(attempts) and len(attempts) >= 2 and attempts[-1][0] == won   # near: skipped
    assert got["counts"] == (False, 1, len(attempts), 1) and not got["pending"] and not got["gave_up"] and got["error"] == ""   # (a skip is no attempt)
    assert max(errs[won:]) < lc.GT_BOUND, errs[won:]
    # the map holds nothing of the time the driver was LOST
    counts = {(r["n_map_points"], r["n_map_voxels"]) for r in recs[lost_at:won]}
    assert len(counts) == 1 and not any(r["map_updated"] for r in recs[lost_at:won]), counts
    assert recs[won]["map_updated"] and recs[won]["n_map_points"] > recs[won - 1]["n_map_points"]
    assert got["profile"]["lost_recovery.attempts"] == len(attempts) and got["profile"]["lost_recovery.seconds"] > 0
    # the records onLidar returned say the same as records()
    for a, b in zip(got["returned"], recs):
        assert all(a[k] == b[k] for k in NEW_FIELDS)


def test_an_own_request_that_cannot_be_served_is_a_failed_attempt(host, session):
    """relocalization.max_candidates below the grid around one key-frame: serving a keyframes request throws.  A caller's request
    throws out of onLidar, as it always did, and the caller withdraws or repeats it; the driver's own has nobody to do that and
    would throw on every later scan.  It is a failed attempt: the drive goes on, the request is cleared, max_attempts: 2 is reached
    after two of them and the records say so."""
    got, want, o, worst = _against_the_reference(host, session, "brief", lc.NO_ROOM, lc.NO_ROOM_MAX_CANDIDATES)
    recs, cut = got["records"], lc.drive("brief")["cut"]
    assert [r["recovery_attempt"] for r in recs[cut:]] == [0, 0, 0, lrr.KEYFRAMES, lrr.KEYFRAMES, 0]
    assert [r["recovery_gave_up"] for r in recs[cut:]] == [False, False, False, False, True, True]
    assert not any(r["relocalization_tried"] or r["place_tried"] or r["recovery_succeeded"] or r["reloc_candidates"] for r in recs)
    assert got["counts"] == (True, 1, 2, 0) and got["gave_up"] and not got["pending"]
    assert "exceed max_candidates (100)" in got["error"] and o.last_error != ""
    assert got["profile"]["lost_recovery.attempts"] == 2 and got["profile"]["lost_recovery.not_served"] == 2
    # the same request from a caller still throws, and stays the caller's to withdraw
    with pytest.MonkeyPatch.context() as mp:
        for v in lc.ENV:
            mp.delenv(v, raising=False)
        for k, v in lc.environment(session["map_file"], session["kf_file"]).items():
            mp.setenv(k, v)
        lo = host.LidarOdometry()
        lo.initialize(host.Config.FromYamlText(lc.pipeline_text(lc.NO_ROOM, lc.NO_ROOM_MAX_CANDIDATES)))
        d = lc.drive("brief")
        lo.onLidar(d["stamps"][0], *d["scans"][0])
        lo.relocalizeInKeyFrames()
        with pytest.raises(RuntimeError, match=r"exceed max_candidates \(100\)"):
            lo.onLidar(d["stamps"][1], *d["scans"][1])
        assert lo.relocalizationPending() and lo.lastRecoveryError() == ""


def test_disabled_and_absent_are_the_driver_as_it_was(host, session):
    d = lc.drive("kidnap")
    absent, off = _run(host, session, "kidnap", ""), _run(host, session, "kidnap", lc.block(False))
    _same_run(absent, off)
    for r in absent["records"]:
        assert {k: r[k] for k in NEW_FIELDS} == NEW_FIELDS
    assert absent["counts"] == (False, 0, 0, 0) and not absent["pending"]
    assert not any(k.startswith("lost_recovery.") for k in absent["profile"])
    # field by field the run the reference makes without the block (the old fields, their old values)
    want, _ = lc.reference_run("kidnap", "")
    worst = max(tl._compare(k, a, b) for k, (a, b) in enumerate(zip(absent["records"], want)))
    assert worst < 1e-6, worst
    # ... and the vehicle stays lost
    cut = d["cut"]
    assert not any(r["icp_good"] for r in absent["records"][cut:])
    err = lc.position_error(absent["records"][-1], d["poses"][-1])
    print("without the block: final error %.2f m" % err)
    assert err > 10.0


def test_a_drive_that_is_never_lost_is_untouched_by_the_enabled_block(host, session):
    on, absent = _run(host, session, "none", lc.block(True)), _run(host, session, "none", "")
    _same_run(on, absent)
    assert all(r["icp_good"] and not r["lost"] and r["bad_streak"] == 0 for r in on["records"]) and on["counts"] == (False, 0, 0, 0)
    assert not any(k.startswith(("lost_recovery.", "onLidar.2.relocalize")) for k in on["profile"])


def test_method_near_recovers_from_a_short_cut(host, session):
    d = lc.drive("short")
    got, want, o, worst = _against_the_reference(host, session, "short", lc.NEAR_BLOCK)
    recs, won = got["records"], d["cut"] + 3
    assert [(k, r["recovery_attempt"], r["recovery_succeeded"]) for k, r in enumerate(recs) if r["recovery_attempt"]] == [(won, lrr.NEAR, True)]
    assert not recs[won]["place_tried"] and recs[won]["reloc_candidates"] == 20181
    errs = [lc.position_error(r, d["poses"][k]) for k, r in enumerate(recs)]
    print("near: quality %.3f, |pose - reference| %g, errors from scan %d on: max %.3f" % (recs[won]["reloc_best_quality"], worst, won, max(errs[won:])))
    assert max(errs[won:]) < lc.GT_BOUND and got["counts"] == (False, 1, 1, 1)


def test_good_alignments_while_lost_move_the_pose_but_not_the_map(host, session, monkeypatch):
    """tests/lost_recovery_cases.py's glitch: four sweeps from elsewhere (bad_scans_to_lost 4), then the drive goes on where it was; a
    caller's request for a wrong place replaces the driver's own and fails on every scan.  Scans 14 and 15 align without a motion
    model, scan 16 aligns with one and would be merged -- it is not, the driver is LOST; scan 17 is the fourth good one: TRACKING."""
    for v in lc.ENV:
        monkeypatch.delenv(v, raising=False)
    for k, v in lc.environment(session["map_file"], session["kf_file"]).items():
        monkeypatch.setenv(k, v)
    d = lc.glitch_drive()
    want, o = lc.glitch_reference_run()
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlText(lc.pipeline_text(lc.GLITCH_BLOCK)))
    pose12, _, cov = lc.wrong_request()
    for k, ((xyz, t), st) in enumerate(zip(d["scans"], d["stamps"])):
        lo.onLidar(st, xyz, t)
        if k == lc.GLITCH_AT[-1]:
            assert lo.isLost() and lo.relocalizationPending()      # (the driver's own request, which the caller's replaces)
            lo.relocalizeNearPose(pose12, cov)
    recs = lo.records()
    worst = _compare_records(recs, want)
    assert worst < 1e-6, worst
    last = lc.GLITCH_AT[-1]
    assert [r["bad_streak"] for r in recs[last - 3:last + 1]] == [1, 2, 3, 4] and not recs[last]["lost"]
    assert all(r["lost"] and r["icp_good"] and r["relocalization_tried"] and not r["relocalized"] and r["recovery_attempt"] == 0 and not r["map_updated"]
               for r in recs[last + 1:last + 5][:3])
    third, fourth = recs[last + 3], recs[last + 4]
    assert third["had_motion_model"] and third["n_map_points"] == recs[last]["n_map_points"]        # good, with a motion model, and kept out
    assert fourth["lost"] and fourth["map_updated"] and fourth["n_map_points"] > third["n_map_points"] and not recs[last + 5]["lost"]
    errs = [lc.position_error(r, d["poses"][k]) for k, r in enumerate(recs)]
    print("|pose - reference|", worst, "errors after the glitch [m]", [round(e, 3) for e in errs[last + 1:]])
    assert max(errs[last + 1:]) < lc.GT_BOUND                       # ... while the pose followed
    # a skipped near attempt is all the driver did, and no attempt; the way back was the good alignments'; the caller's request still waits
    assert (lo.isLost(), lo.timesLost(), lo.recoveryAttempts(), lo.timesRecovered()) == (False, 1, 0, 1) and lo.relocalizationPending()
    assert (o.m.lost, o.m.times_lost, o.m.attempts, o.m.times_recovered) == (False, 1, 0, 1)


def test_what_initialize_refuses_with_the_session_loaded(host, session, monkeypatch):
    for v in lc.ENV:
        monkeypatch.delenv(v, raising=False)
    env = lc.environment(session["map_file"], session["kf_file"])
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    # an AlignBatcher set before initialize(): refused there in the words of relocalizeInKeyFrames' refusal whatever the method, the
    # words setAlignBatcher uses when it comes second (tests/test_lost_recovery_cpu.py)
    batched = host.LidarOdometry(device=0, own_context=True)
    batcher = host.AlignBatcher(1)
    batched.setAlignBatcher(batcher)
    words = (r"lost_recovery: enabled: LidarOdometry::relocalizeInKeyFrames: not available with an AlignBatcher \(the batch protocol has no slot for the "
             r"extra alignments of one member\)")
    with pytest.raises(RuntimeError, match=r"^LidarOdometry \(HIP\): " + words):
        batched.initialize(host.Config.FromYamlText(lc.pipeline_text(lc.block(True, method="near"))))
    batcher.leave()
    # method: keyframes without a source of key-frames
    monkeypatch.delenv("MOLA_LOAD_SM")
    with pytest.raises(RuntimeError, match=r"lost_recovery: method 'keyframes' needs key-frames"):
        host.LidarOdometry().initialize(host.Config.FromYamlText(lc.pipeline_text(lc.block(True, method="keyframes"))))
    lo = host.LidarOdometry()
    lo.initialize(host.Config.FromYamlText(lc.pipeline_text(lc.block(True, method="near"))))   # near asks for none
    assert lo.lostRecoveryOptions()["method"] == "near"
