"""The scenario of tests/test_lost_recovery_cpu.py and tests/test_gpu_lost_recovery.py: the 12-key-frame session of
tests/place_cases.py (key-frame file + session map, key-frames every 10 m along the street), and drives through it at 32 rings x
600 azimuths, 2 m/s along the street from x = -100 m, one sweep every 0.1 s, of which a stretch is cut out (the kidnap): the scans
before the cut run normally, the scans after it arrive with the time stamps and at the places they have in the uncut drive.

  drive("kidnap"): 10 scans, 248 scans = 49.6 m cut, 30 scans: the vehicle reappears at x = -48.4 m, between two key-frames, and
                   reaches the next one's neighbourhood 13 scans later
  drive("short"):  10 scans, 15 scans = 3 m cut, 20 scans: the no-motion-model ICP bridges a cut of 1 m at once and one of 2 m after
                   one rejected scan; it does not bridge 3 m within the 20 scans
  drive("none"):   40 scans, nothing cut
  drive("brief"):  the first 16 scans of drive("kidnap"): lost at scan 12, three scans to serve requests

The cuts were chosen on the CPU with tests/lost_recovery_ref.py alone; profiles/lost_recovery.md holds what the reference shows
on them.  Data generation only (mola_lidar_odometry_amd.synth, place_cases); the reference runs are cached per process."""
import functools
import os

import numpy as np

import place_cases as pc
from mola_lidar_odometry_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPE = os.path.join(ROOT, "pipelines", "lidar3d-default-hip.yaml")

DT, SPEED = 0.1, 2.0
START = np.array([-100.0, 0.2, pc.SENSOR_Z, 0.0, 0.0, 0.0])   # (x, y, z, yaw, pitch, roll) of scan 0
DRIVES = dict(kidnap=(10, 248, 30), short=(10, 15, 20), none=(40, 0, 0), brief=(10, 248, 6))   # scans before, scans cut, scans after
MIN_QUALITY = pc.MIN_QUALITY        # the place scenario's acceptance: the street is self-similar (place_cases.py)
GT_BOUND = pc.GT_BOUND              # [m] per axis, the place test's bound
ENV = ("MOLA_LOAD_MM", "MOLA_LOAD_SM", "MOLA_MAPPING_ENABLED", "MOLA_MINIMUM_ICP_QUALITY", "MOLA_GENERATE_SIMPLEMAP", "MOLA_SIMPLEMAP_OUTPUT",
       "MOLA_INITIAL_LOCALIZATION_ENABLED", "MOLA_INITIAL_X", "MOLA_INITIAL_Y", "MOLA_INITIAL_Z", "MOLA_INITIAL_YAW", "MOLA_INITIAL_PITCH",
       "MOLA_INITIAL_ROLL", "MOLA_MAX_TIME_TO_USE_VELOCITY_MODEL", "MOLA_OPTIMIZE_TWIST", "MOLA_INITIAL_VX")


def block(enabled=True, **kw):
    """the lost_recovery: block as text, to be appended to a pipeline file"""
    return "\nlost_recovery:\n  enabled: %s\n" % ("true" if enabled else "false") + "".join("  %s: %s\n" % (k, v) for k, v in kw.items())


NEAR_BLOCK = block(True, method="near", near_sigma_xy=1.5, near_sigma_yaw_deg=10)   # +-4.5 m, +-30 deg: 20181 candidates on the session map


# a relocalization.max_candidates that the grid around ONE key-frame exceeds: no keyframes request can be served under it
NO_ROOM = block(True, method="keyframes", retry_every_n_scans=1, max_attempts=2)
NO_ROOM_MAX_CANDIDATES = 100


def pipeline_text(extra="", max_candidates=None):
    """place_cases' pipeline (two key-frames kept, +-1.5 m around each) and `extra`; max_candidates: relocalization.max_candidates"""
    txt = pc.pipeline_text(PIPE)
    if max_candidates is not None:
        assert txt.count("  max_candidates: 65536\n") == 1
        txt = txt.replace("  max_candidates: 65536\n", "  max_candidates: %d\n" % max_candidates)
    return txt + extra


def environment(map_file, kf_file):
    """what every run of the scenario sets: both session files loaded, mapping on (multi-session), the place scenario's acceptance,
    the first scan's true pose as the fixed initial pose"""
    env = dict(MOLA_LOAD_MM=map_file, MOLA_LOAD_SM=kf_file, MOLA_MAPPING_ENABLED="true", MOLA_MINIMUM_ICP_QUALITY=MIN_QUALITY,
               MOLA_INITIAL_LOCALIZATION_ENABLED="true")
    for name, v in zip(("X", "Y", "Z", "YAW", "PITCH", "ROLL"), START):
        env["MOLA_INITIAL_" + name] = repr(float(v))
    return env


def scan_indices(name):
    before, cut, after = DRIVES[name]
    return list(range(before)) + list(range(before + cut, before + cut + after))


def pose_of(k):
    """ground truth of sweep k of the uncut drive, (x, y, z, yaw, pitch, roll)"""
    return START + np.array([SPEED * DT * k, 0.0, 0.0, 0.0, 0.0, 0.0])


@functools.lru_cache(maxsize=None)
def drive(name):
    """dict(scans [(xyz, t)], stamps, poses [n, 6] ground truth, cut: index of the first scan after the cut (None: no cut))"""
    sc = pc.scene()
    ks = scan_indices(name)
    tw = np.array([SPEED, 0.0, 0.0, 0.0, 0.0, 0.0])
    scans = [synth.make_sweep(sc, synth.pose_from_ypr(pose_of(k)), tw, DT, 32, 600, 7000 + k) for k in ks]
    before, cut, _ = DRIVES[name]
    return dict(scans=scans, stamps=[1000.0 + DT * k for k in ks], poses=np.array([pose_of(k) for k in ks]), cut=before if cut else None)


def position_error(rec, gt6):
    """max over x, y, z of |pose - ground truth| [m]"""
    return float(np.abs(np.asarray(rec["pose"], np.float64)[[3, 7, 11]] - np.asarray(gt6)[:3]).max())


@functools.lru_cache(maxsize=1)
def cpu_session():
    """(frames, map record) of the session, made by the reference alone (place_localize_ref.cpu_session).  That record says 0 for
    remove_voxels_farther_than, which is of no account while mapping is off; here mapping is on, and the record gets what the session
    map file holds: the pipeline's formula as the first key-frame's scan evaluates it."""
    import place_localize_ref as plr
    frames, rec = plr.cpu_session(PIPE, pc.scene())
    o = plr.PlaceOracle(PIPE)
    assert o.on_lidar(1000.0, *pc.kf_sweeps(pc.scene())[0])["first_scan"]
    return frames, dict(rec, remove_voxels_farther_than=float(o.remove_far))


@functools.lru_cache(maxsize=None)
def reference_run(name, extra, max_candidates=None):
    """the records of tests/lost_recovery_ref.py's driver on drive(name) under pipeline_text(extra), the environment set for the
    session made on the CPU (the files' names do not matter to it); unchanged by whoever asks"""
    import lost_recovery_ref as lrr
    frames, rec = cpu_session()
    old = {k: os.environ.get(k) for k in ENV}
    try:
        for k in ENV:
            os.environ.pop(k, None)
        os.environ.update(environment("", ""))
        os.environ.pop("MOLA_LOAD_MM"), os.environ.pop("MOLA_LOAD_SM")
        o = lrr.LostOracle(None, text=pipeline_text(extra, max_candidates))
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    o.preload(rec)
    o.set_keyframes(frames)
    d = drive(name)
    return [dict(o.on_lidar(st, xyz, t)) for (xyz, t), st in zip(d["scans"], d["stamps"])], o


# ---- a glitch: four sweeps from elsewhere in an uncut drive, and a caller whose own request keeps failing ---------------------------------
GLITCH_BLOCK = block(True, bad_scans_to_lost=4)
GLITCH_AT = (10, 11, 12, 13)                                           # these scans of drive("none") are replaced by drive("kidnap")'s
GLITCH_SCANS = 20
WRONG_POSE = np.array([60.0, 0.2, pc.SENSOR_Z, 0.0, 0.0, 0.0])   # where the caller believes the vehicle to be: 55 m beyond the session
WRONG_SIGMAS = (0.2, 0.2, 1.0)                                 # [m, m, deg]: a grid of 3 x 3 x 3


@functools.lru_cache(maxsize=1)
def glitch_drive():
    """drive("none")'s first GLITCH_SCANS scans with the four of GLITCH_AT taken 50 m further on (their time stamps stay): the four
    are rejected, with bad_scans_to_lost 4 the driver is LOST, and the scans after them align again from the last good pose -- good
    alignments while LOST.  The first two of them have no motion model and would not be merged anyway; the third has one and is kept
    out of the map because the driver is LOST; the fourth is TRACKING again.  The caller's request (wrong_request(), placed after the
    last alien scan) replaces the driver's own and fails on every scan, so that the way back is the good alignments'."""
    a, b = drive("none"), drive("kidnap")
    scans = [b["scans"][k] if k in GLITCH_AT else a["scans"][k] for k in range(GLITCH_SCANS)]
    return dict(scans=scans, stamps=a["stamps"][:GLITCH_SCANS], poses=a["poses"][:GLITCH_SCANS], cut=None)


def wrong_request():
    """(pose as 12 values, as (x, y, z, yaw, pitch, roll), covariance as 36 values) of the caller's request"""
    import score_ref as sr
    cov = sr.grid_cov(WRONG_SIGMAS[0], WRONG_SIGMAS[1], np.deg2rad(WRONG_SIGMAS[2]))
    return [float(v) for v in synth.pose_from_ypr(WRONG_POSE)], WRONG_POSE.copy(), [float(v) for v in np.asarray(cov).reshape(36)]


@functools.lru_cache(maxsize=1)
def glitch_reference_run():
    """reference_run's recipe on glitch_drive() under GLITCH_BLOCK, the caller's request placed after scan GLITCH_AT[-1]"""
    import lost_recovery_ref as lrr
    frames, rec = cpu_session()
    old = {k: os.environ.get(k) for k in ENV}
    try:
        for k in ENV:
            os.environ.pop(k, None)
        os.environ.update(environment("", ""))
        os.environ.pop("MOLA_LOAD_MM"), os.environ.pop("MOLA_LOAD_SM")
        o = lrr.LostOracle(None, text=pipeline_text(GLITCH_BLOCK))
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    o.preload(rec)
    o.set_keyframes(frames)
    d, recs = glitch_drive(), []
    for k, ((xyz, t), st) in enumerate(zip(d["scans"], d["stamps"])):
        recs.append(dict(o.on_lidar(st, xyz, t)))
        if k == GLITCH_AT[-1]:
            o.relocalize_near_pose(wrong_request()[1], np.array(wrong_request()[2]))
    return recs, o
